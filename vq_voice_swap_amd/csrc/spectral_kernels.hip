// Conversion-quality scores (include/vqvs.h, vqvs_spectral_distance): per clip, the sum over frames of the mel-cepstral distortion
// and of the log-mel spectral distance between two waveforms a, b [B, T], in one kernel -- no spectrum, mel value or cepstrum goes
// to memory.  The arithmetic is that of the MFCC front end (mfcc_kernels.hip): a reflect-padded, centred frame times the window in
// f32, a direct DFT accumulated in f64 against an f64 twiddle table (n_fft need be no power of two), power, mel value and cepstral
// coefficient each an f64 accumulation rounded to f32.  The logarithm is taken in f64 and rounded to f32 once: a correctly rounded
// logf, so the values are those of a float64 evaluation that rounds at the same points.
//
// A workgroup owns SD_FR consecutive frames of one clip and runs the two signals as 2 * SD_FR "rows" of one loop nest: frame f of a
// and frame f of b go through the same instruction sequence, so d(a, a) is exactly 0 and d(a, b) == d(b, a) bitwise.  The frames of
// a workgroup are added in frame order by one thread, the workgroups' partials in tile order by the clip's one writer
// (spectral_finish_kernel): the order depends on (T, hop) alone, not on B, the clip's row or the schedule, and there are no
// floating-point atomics.
//
// vqvs_mel_cepstra writes the same per-frame values out -- cepstra and, on request, log-mel values -- for recordings of different
// lengths in one batch.  Both kernels frame through frame_sample() and run front_end(): one copy of the arithmetic.
#include <cmath>

#include "kernels.hpp"

namespace vqvs {

namespace {

constexpr int SD_FR = 4;             // frames per workgroup
constexpr int SD_ROWS = 2 * SD_FR;   // rows 0 .. SD_FR-1: the frames of a; SD_FR .. 2 SD_FR-1: those of b
constexpr int SD_NT = 256;
constexpr int SD_MAXN = 512;         // max n_fft
constexpr int SD_MAXK = 257;         // max n_fft / 2 + 1
constexpr int SD_MAXM = 128;         // max n_mels
constexpr int SD_MAXC = 64;          // max n_ceps
constexpr double SD_DB = 10.0 / 2.302585092994045684;  // 10 / ln 10

// what the per-frame front end reads beside the windowed frames
struct FrontEnd {
  const double* twiddle;   // [n_fft][2]: cos, sin of 2 pi i / n_fft
  const float* fb;         // [n_freqs][n_mels]
  const float* dct;        // [n_mels][n_ceps]
  int n_fft, n_freqs, n_mels, n_ceps;
  float eps;
};

struct SpectralArgs {
  const float *a, *b;      // [B][T]
  const float* window;     // [n_fft]
  FrontEnd fe;
  double* part;            // out [B][ntiles][2]: (mcd, lsd) summed over the tile's frames
  int T, frames, hop, ntiles;
};

// Power spectrum of every row.  A work item is (frequency bin k, group g of R rows); a thread walks the items tid, tid + 256, ...
// With R = SD_ROWS one thread per bin does all rows, as the MFCC kernel does; a smaller R spreads a short transform (33 bins at
// n_fft 64) over the idle lanes and evens out the 257th bin of n_fft 512.  Every (row, bin) is ONE chain over n whatever R is.
template <int R>
__device__ __forceinline__ void power_rows(const double* tw, const float (*xs)[SD_MAXN], float (*pw)[SD_MAXK], int N, int n_freqs, int tid) {
  constexpr int G = SD_ROWS / R;
  for (int item = tid; item < n_freqs * G; item += SD_NT) {
    const int g = item / n_freqs, k = item - g * n_freqs;
    double re[R], im[R];
#pragma unroll
    for (int r = 0; r < R; ++r) re[r] = im[r] = 0.0;
    int idx = 0;
    for (int n = 0; n < N; ++n) {
      const double c = tw[2 * idx], s = tw[2 * idx + 1];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double xv = (double)xs[g * R + r][n];
        re[r] = fma(xv, c, re[r]);
        im[r] = fma(xv, s, im[r]);
      }
      idx += k;
      if (idx >= N) idx -= N;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) pw[g * R + r][k] = (float)(re[r] * re[r] + im[r] * im[r]);
  }
}

// Sample n of the windowed frame `frame` of a signal of `len` samples: centred, reflect padding of n_fft / 2 about 0 and len
// (len > n_fft / 2: one reflection lands inside the signal).  Nothing at or beyond len is read.
__device__ __forceinline__ float frame_sample(const float* x, int len, int frame, int hop, int half, int n, const float* window) {
  int s = frame * hop + n - half;
  if (s < 0) s = -s;
  if (s >= len) s = 2 * (len - 1) - s;
  return x[s] * window[n];
}

// The per-frame front end of SD_ROWS windowed frames xs: power spectrum, mel filter bank, logarithm, DCT-II -> lg, cp.  Called by
// every thread of the workgroup; the caller has written xs and not yet synchronised, and finds lg and cp visible on return.
__device__ __forceinline__ void front_end(const FrontEnd& a, int rows_per_item, double* tw, const float (*xs)[SD_MAXN], float (*pw)[SD_MAXK],
                                          float (*lg)[SD_MAXM], float (*cp)[SD_MAXC], int tid) {
  const int N = a.n_fft;
  for (int i = tid; i < 2 * N; i += SD_NT) tw[i] = a.twiddle[i];
  __syncthreads();
  switch (rows_per_item) {
    case 1: power_rows<1>(tw, xs, pw, N, a.n_freqs, tid); break;
    case 2: power_rows<2>(tw, xs, pw, N, a.n_freqs, tid); break;
    case 4: power_rows<4>(tw, xs, pw, N, a.n_freqs, tid); break;
    default: power_rows<8>(tw, xs, pw, N, a.n_freqs, tid); break;
  }
  __syncthreads();
  // mel filter bank, then the logarithm: log in f64 of the f32 sum mel + eps, rounded to f32
  for (int i = tid; i < SD_ROWS * a.n_mels; i += SD_NT) {
    const int row = i / a.n_mels, m = i - row * a.n_mels;
    double acc = 0.0;
    for (int k = 0; k < a.n_freqs; ++k) acc = fma((double)pw[row][k], (double)a.fb[k * a.n_mels + m], acc);
    const float mel = (float)acc;
    lg[row][m] = (float)log((double)(mel + a.eps));
  }
  __syncthreads();
  // DCT-II
  for (int i = tid; i < SD_ROWS * a.n_ceps; i += SD_NT) {
    const int row = i / a.n_ceps, j = i - row * a.n_ceps;
    double acc = 0.0;
    for (int m = 0; m < a.n_mels; ++m) acc = fma((double)lg[row][m], (double)a.dct[m * a.n_ceps + j], acc);
    cp[row][j] = (float)acc;
  }
  __syncthreads();
}

__global__ __launch_bounds__(SD_NT) void spectral_distance_kernel(const SpectralArgs a, int rows_per_item) {
  __shared__ double tw[SD_MAXN * 2];
  __shared__ float xs[SD_ROWS][SD_MAXN];
  __shared__ float pw[SD_ROWS][SD_MAXK];
  __shared__ float lg[SD_ROWS][SD_MAXM];
  __shared__ float cp[SD_ROWS][SD_MAXC];
  __shared__ double fr[SD_FR][2];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * SD_FR;
  const int N = a.fe.n_fft, half = N >> 1;
  for (int i = tid; i < SD_ROWS * N; i += SD_NT) {
    const int row = i / N, n = i - row * N;
    const int f = row % SD_FR;
    const float* xb = (row < SD_FR ? a.a : a.b) + (size_t)b * a.T;
    xs[row][n] = f0 + f < a.frames ? frame_sample(xb, a.T, f0 + f, a.hop, half, n, a.window) : 0.f;
  }
  front_end(a.fe, rows_per_item, tw, xs, pw, lg, cp, tid);
  // the two distances of a frame, f64, terms in index order; a frame past the clip's last adds nothing
  if (tid < SD_FR) {
    double mcd = 0.0, lsd = 0.0;
    if (f0 + tid < a.frames) {
      double sc = 0.0, sl = 0.0;
      for (int j = 1; j < a.fe.n_ceps; ++j) {  // coefficient 0 is left out
        const double d = (double)cp[tid][j] - (double)cp[SD_FR + tid][j];
        sc = fma(d, d, sc);
      }
      for (int m = 0; m < a.fe.n_mels; ++m) {
        const double d = (double)lg[tid][m] - (double)lg[SD_FR + tid][m];
        sl = fma(d, d, sl);
      }
      mcd = SD_DB * sqrt(2.0 * sc);
      lsd = SD_DB * sqrt(sl / (double)a.fe.n_mels);
    }
    fr[tid][0] = mcd;
    fr[tid][1] = lsd;
  }
  __syncthreads();
  if (tid == 0) {
    double mcd = 0.0, lsd = 0.0;
#pragma unroll
    for (int f = 0; f < SD_FR; ++f) {
      mcd += fr[f][0];
      lsd += fr[f][1];
    }
    const size_t t = (size_t)b * a.ntiles + blockIdx.x;
    a.part[2 * t] = mcd;
    a.part[2 * t + 1] = lsd;
  }
}

// one thread -- one writer -- per clip adds the clip's tile partials in tile order
__global__ __launch_bounds__(64) void spectral_finish_kernel(const double* part, double* mcd, double* lsd, int B, int ntiles) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double sm = 0.0, sl = 0.0;
  for (int i = 0; i < ntiles; ++i) {
    const size_t t = (size_t)b * ntiles + i;
    sm += part[2 * t];
    sl += part[2 * t + 1];
  }
  if (mcd) mcd[b] = sm;
  if (lsd) lsd[b] = sl;
}

struct CepstraArgs {
  const float* x;          // [B][T]
  const int* len;          // [B] true lengths: device data, clamped into n_fft / 2 + 1 .. T before use
  const float* window;     // [n_fft]
  FrontEnd fe;
  float* ceps;             // out [B][fmax][n_ceps]
  float* logmel;           // out [B][fmax][n_mels] or nullptr
  int* frames;             // out [B]
  int T, fmax, hop;
};

// vqvs_mel_cepstra: a workgroup owns SD_ROWS consecutive frames of one recording -- the rows of the same front end -- and is the
// only writer of their cepstra and log-mel values; frames at or beyond the recording's own count are written as 0.
__global__ __launch_bounds__(SD_NT) void mel_cepstra_kernel(const CepstraArgs a, int rows_per_item) {
  __shared__ double tw[SD_MAXN * 2];
  __shared__ float xs[SD_ROWS][SD_MAXN];
  __shared__ float pw[SD_ROWS][SD_MAXK];
  __shared__ float lg[SD_ROWS][SD_MAXM];
  __shared__ float cp[SD_ROWS][SD_MAXC];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * SD_ROWS;
  const int N = a.fe.n_fft, half = N >> 1;
  const int len = min(max(a.len[b], half + 1), a.T);
  const int frames = len / a.hop + 1;  // <= fmax = T / hop + 1
  const float* xb = a.x + (size_t)b * a.T;
  for (int i = tid; i < SD_ROWS * N; i += SD_NT) {
    const int row = i / N, n = i - row * N;
    xs[row][n] = f0 + row < frames ? frame_sample(xb, len, f0 + row, a.hop, half, n, a.window) : 0.f;
  }
  front_end(a.fe, rows_per_item, tw, xs, pw, lg, cp, tid);
  const int rows = min(SD_ROWS, a.fmax - f0);
  for (int i = tid; i < rows * a.fe.n_ceps; i += SD_NT) {
    const int row = i / a.fe.n_ceps, j = i - row * a.fe.n_ceps;
    a.ceps[((size_t)b * a.fmax + f0 + row) * a.fe.n_ceps + j] = f0 + row < frames ? cp[row][j] : 0.f;
  }
  if (a.logmel)
    for (int i = tid; i < rows * a.fe.n_mels; i += SD_NT) {
      const int row = i / a.fe.n_mels, m = i - row * a.fe.n_mels;
      a.logmel[((size_t)b * a.fmax + f0 + row) * a.fe.n_mels + m] = f0 + row < frames ? lg[row][m] : 0.f;
    }
  if (blockIdx.x == 0 && tid == 0) a.frames[b] = frames;
}

// rows per work item of the power spectrum: the R in {8, 4, 2, 1} with the least work on the busiest thread.  A thread runs
// ceil(n_freqs * (8 / R) / 256) items; a step of an item is R rows (a 4-byte broadcast LDS read and two f64 FMAs each) behind one
// 16-byte twiddle read that every lane makes at its own address and that is weighed as TW_ROWS rows.  (With the twiddle read
// weighed as nothing, R = 1 wins at n_fft 400 by 7 rounds to 8 and the kernel, LDS-bound, measures 1.51 ms at (64, 64000).)
int spectral_rows_per_item(int n_freqs) {
  constexpr int TW_ROWS = 3;
  int best = SD_ROWS, best_cost = ((n_freqs + SD_NT - 1) / SD_NT) * (SD_ROWS + TW_ROWS);
  for (int R = SD_ROWS / 2; R >= 1; R /= 2) {
    const int cost = ((n_freqs * (SD_ROWS / R) + SD_NT - 1) / SD_NT) * (R + TW_ROWS);
    if (cost < best_cost) {
      best = R;
      best_cost = cost;
    }
  }
  return best;
}

}  // namespace

size_t spectral_distance_scratch_bytes(int B, int T, int hop) {
  const size_t ntiles = ((size_t)T / hop + 1 + SD_FR - 1) / SD_FR;
  return (size_t)B * ntiles * 2 * sizeof(double);
}

int run_spectral_distance(const float* a, const float* b, const float* window, const double* twiddle, const float* fb, const float* dct,
                          void* scratch, double* mcd, double* lsd, int B, int T, int n_fft, int hop, int n_mels, int n_ceps, float eps,
                          hipStream_t st) {
  SpectralArgs s;
  s.a = a, s.b = b, s.window = window;
  s.fe = FrontEnd{twiddle, fb, dct, n_fft, n_fft / 2 + 1, n_mels, n_ceps, eps};
  s.part = static_cast<double*>(scratch);
  s.T = T, s.frames = T / hop + 1, s.hop = hop;
  s.ntiles = (s.frames + SD_FR - 1) / SD_FR;
  if (n_fft > SD_MAXN || s.fe.n_freqs > SD_MAXK || n_mels > SD_MAXM || n_ceps > SD_MAXC || T <= n_fft / 2)
    VQVS_FAIL(-1, "spectral distance: n_fft=%d n_mels=%d n_ceps=%d T=%d outside the kernel's tables", n_fft, n_mels, n_ceps, T);
  hipLaunchKernelGGL(spectral_distance_kernel, dim3(s.ntiles, B), dim3(SD_NT), 0, st, s, spectral_rows_per_item(s.fe.n_freqs));
  VQVS_HIP(hipGetLastError());
  hipLaunchKernelGGL(spectral_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, st, s.part, mcd, lsd, B, s.ntiles);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int run_mel_cepstra(const float* x, const int* len, const float* window, const double* twiddle, const float* fb, const float* dct, float* ceps,
                    float* logmel, int* frames, int B, int T, int n_fft, int hop, int n_mels, int n_ceps, float eps, hipStream_t st) {
  CepstraArgs s;
  s.x = x, s.len = len, s.window = window;
  s.fe = FrontEnd{twiddle, fb, dct, n_fft, n_fft / 2 + 1, n_mels, n_ceps, eps};
  s.ceps = ceps, s.logmel = logmel, s.frames = frames;
  s.T = T, s.fmax = T / hop + 1, s.hop = hop;
  if (n_fft > SD_MAXN || s.fe.n_freqs > SD_MAXK || n_mels > SD_MAXM || n_ceps > SD_MAXC || T <= n_fft / 2)
    VQVS_FAIL(-1, "mel cepstra: n_fft=%d n_mels=%d n_ceps=%d T=%d outside the kernel's tables", n_fft, n_mels, n_ceps, T);
  hipLaunchKernelGGL(mel_cepstra_kernel, dim3((s.fmax + SD_ROWS - 1) / SD_ROWS, B), dim3(SD_NT), 0, st, s, spectral_rows_per_item(s.fe.n_freqs));
  VQVS_HIP(hipGetLastError());
  return 0;
}

}  // namespace vqvs
