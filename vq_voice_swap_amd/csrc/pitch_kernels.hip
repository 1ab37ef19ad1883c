// Pitch scores (include/vqvs.h, vqvs_pitch_distance): per frame the YIN period of two waveforms a, b [B, T], per clip the voicing
// counts and the sums of the frame-wise pitch distance in semitones and of its square, in one kernel -- no frame, difference
// function or normalised difference goes to memory.  The definition is DESIGN.md section 3.14: the samples are quantised to the 16
// bits a WAV would hold, so the difference function d(tau) = sum_j (q[j] - q[j + tau])^2 and its running sum are integers below
// 2^53, the same in any order of addition; d'(tau) = d(tau) tau / c(tau) is one IEEE division of two exact values, and the pick and
// the parabolic refinement are a fixed sequence of float64 operations compiled with contraction off.  The periods are therefore the
// definition's, bit for bit, whatever the schedule.
//
// A workgroup owns PD_FR consecutive frames of one clip and runs the two signals as 2 * PD_FR "rows" of one loop nest, as
// spectral_distance_kernel does: frame f of a and frame f of b go through the same instruction sequence, so b = a gives distance 0
// without a sign bit.  The tile's quantised span (S + (PD_FR - 1) hop words per signal, S = window + tau_max) is staged in LDS
// once, quantised on the way in.  A work item of the main loop is (row, lag): its loop over j reads q[j], one address for the lanes
// of a row, and q[j + lag], consecutive words across lanes, and adds the square with one 64-bit multiply-add.  Then one wave per
// row scans d over the lags (integers: order-free), writes d' over d, finds the first lag under the threshold by ballots, walks to
// the local minimum and refines.  The frames of a workgroup are added in frame order by one thread, the workgroups' partials in tile
// order by the clip's one writer (pitch_finish_kernel): no floating-point atomics.
#include <atomic>
#include <cmath>
#include <cstdint>

#include "kernels.hpp"

namespace vqvs {

namespace {

constexpr int PD_FR = 4;    // frames per workgroup
constexpr int PD_NT = 256;
constexpr int PD_WAVES = PD_NT / 64;

struct PitchPart {  // what a workgroup hands to the clip's finisher
  double s1, s2;    // sum of l_f and of l_f^2 over the tile's frames voiced in both signals, in frame order
  int va, vb, both, vuv;
};

struct PitchArgs {
  const float *a, *b;      // [B][T]; b may be nullptr: rows of a only
  double *pa, *pb;         // out [B][frames] or nullptr
  PitchPart* part;         // out [B][ntiles] or nullptr (neither counts nor sums wanted)
  int T, frames, W, hop, tau_min, tau_max, ntiles, span;
  double threshold;
};

// (quantise: common.hpp, the sample rule shared with pause_kernels.hip)
// Steps 5 and 6 for one row: y[tau] holds the bits of d'(tau), t the first lag under the threshold.  Every operation is one float64
// operation.
__device__ __forceinline__ double walk_and_refine(const unsigned long long* y, int t, int tau_max) {
#pragma clang fp contract(off)
  while (t + 1 <= tau_max && __longlong_as_double(y[t + 1]) < __longlong_as_double(y[t])) ++t;
  if (t == tau_max) return (double)t;
  const double y0 = __longlong_as_double(y[t - 1]), y1 = __longlong_as_double(y[t]), y2 = __longlong_as_double(y[t + 1]);
  const double den = (y0 - y1) + (y2 - y1);
  if (!(den > 0.0)) return (double)t;
  const double half = 0.5 * (y0 - y2);
  double off = half / den;
  off = off < -1.0 ? -1.0 : (off > 1.0 ? 1.0 : off);
  return (double)t + off;
}

// Step 7 for a workgroup's frames, in frame order, by one thread.
__device__ __forceinline__ PitchPart compare_frames(const double* per, int nframes) {
#pragma clang fp contract(off)
  PitchPart r = {0.0, 0.0, 0, 0, 0, 0};
  for (int f = 0; f < nframes; ++f) {
    const double pa = per[f], pb = per[PD_FR + f];
    const bool va = pa > 0.0, vb = pb > 0.0;
    r.va += va, r.vb += vb, r.vuv += va != vb;
    if (va && vb) {
      ++r.both;
      const bool up = pa >= pb;
      const double ratio = up ? pa / pb : pb / pa;
      const double mag = 12.0 * log2(ratio);
      const double l = up ? mag : -mag;
      const double sq = l * l;
      r.s1 = r.s1 + l;
      r.s2 = r.s2 + sq;
    }
  }
  return r;
}

__global__ __launch_bounds__(PD_NT) void pitch_distance_kernel(const PitchArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pd_lds[];
  const int nsig = a.b ? 2 : 1, nrows = nsig * PD_FR, ldd = a.tau_max + 1;
  double* per = reinterpret_cast<double*>(pd_lds);                                // [2 PD_FR]: the rows' periods
  unsigned long long* dd = reinterpret_cast<unsigned long long*>(per + 2 * PD_FR);  // [nrows][ldd]: d, then d' in the same words
  int* q = reinterpret_cast<int*>(dd + (size_t)nrows * ldd);                      // [nsig][span]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int clip = blockIdx.y;
  const int f0 = blockIdx.x * PD_FR;
  const int nframes = min(PD_FR, a.frames - f0);
  const int S = a.W + a.tau_max, L = a.span;
  const int s0 = f0 * a.hop - S / 2;  // the clip sample behind q[0]

  // ---- stage: the span of both signals, quantised; samples outside [0, T) are 0.  Groups of four samples that start on a 16-byte
  // boundary of the input and lie inside both the clip and the span are one 16-byte load; the rest go one by one.
  for (int sig = 0; sig < nsig; ++sig) {
    const float* xb = (sig ? a.b : a.a) + (size_t)clip * a.T;
    int* qs = q + sig * L;
    const int mis = (int)((reinterpret_cast<uintptr_t>(xb) >> 2) & 3);
    const int r = ((s0 + mis) % 4 + 4) % 4;
    const int n0 = s0 - r, ngroups = (L + r + 3) / 4;
    for (int g = tid; g < ngroups; g += PD_NT) {
      const int n = n0 + 4 * g, i = n - s0;
      if (n >= 0 && n + 3 < a.T && i >= 0 && i + 3 < L) {
        const float4 v = *reinterpret_cast<const float4*>(xb + n);
        qs[i] = quantise(v.x), qs[i + 1] = quantise(v.y), qs[i + 2] = quantise(v.z), qs[i + 3] = quantise(v.w);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (i + k >= 0 && i + k < L) qs[i + k] = (n + k >= 0 && n + k < a.T) ? quantise(xb[n + k]) : 0;
      }
    }
  }
  __syncthreads();

  // ---- the difference function: item = (row, lag), lags 1 .. tau_max of a row on consecutive lanes
  for (int item = tid; item < nrows * a.tau_max; item += PD_NT) {
    const int row = item / a.tau_max, tau = item - row * a.tau_max + 1;
    const int f = row % PD_FR;
    if (f >= nframes) continue;
    const int* p = q + (row / PD_FR) * L + f * a.hop;
    long long acc = 0;
#pragma unroll 8
    for (int j = 0; j < a.W; ++j) {
      const int d = p[j] - p[j + tau];   // |d| <= 65535
      acc += (long long)d * d;           // one 32 x 32 -> 64-bit multiply-add
    }
    dd[row * ldd + tau] = (unsigned long long)acc;
  }
  __syncthreads();

  // ---- per row, one wave: c = inclusive scan of d, d' over d, first lag under the threshold, walk, refinement
  for (int row = wave; row < nrows; row += PD_WAVES) {
    const int f = row % PD_FR;
    if (f >= nframes) continue;
    unsigned long long* y = dd + row * ldd;  // d, then the bits of d'
    unsigned long long carry = 0;
    for (int base = 1; base <= a.tau_max; base += 64) {
      const int tau = base + lane;
      const unsigned long long d = tau <= a.tau_max ? y[tau] : 0ull;
      unsigned long long c = d;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(c, o, 64);
        if (lane >= o) c += up;
      }
      c += carry;
      carry = __shfl(c, 63, 64);
      if (tau <= a.tau_max) y[tau] = __double_as_longlong(c == 0 ? 1.0 : (double)(d * (unsigned long long)tau) / (double)c);
    }
    if (lane == 0) y[0] = __double_as_longlong(1.0);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    int t0 = 0;
    for (int base = a.tau_min; base <= a.tau_max && !t0; base += 64) {
      const int tau = base + lane;
      const unsigned long long m = __ballot(tau <= a.tau_max && __longlong_as_double(y[tau]) < a.threshold);
      if (m) t0 = base + __ffsll((long long)m) - 1;
    }
    const double period = t0 ? walk_and_refine(y, t0, a.tau_max) : 0.0;
    if (lane == 0) {
      per[row] = period;
      double* out = row < PD_FR ? a.pa : a.pb;
      if (out) out[(size_t)clip * a.frames + f0 + f] = period;
    }
  }
  if (!a.part) return;  // (uniform: a kernel argument)
  __syncthreads();
  if (tid == 0) a.part[(size_t)clip * a.ntiles + blockIdx.x] = compare_frames(per, nframes);
}

// one thread -- one writer -- per clip adds the clip's tile partials in tile order
__global__ __launch_bounds__(64) void pitch_finish_kernel(const PitchPart* part, long long* counts, double* sums, int B, int ntiles) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double s1 = 0.0, s2 = 0.0;
  long long va = 0, vb = 0, both = 0, vuv = 0;
  for (int i = 0; i < ntiles; ++i) {
    const PitchPart p = part[(size_t)b * ntiles + i];
    s1 = s1 + p.s1, s2 = s2 + p.s2;
    va += p.va, vb += p.vb, both += p.both, vuv += p.vuv;
  }
  if (counts) counts[4 * b] = va, counts[4 * b + 1] = vb, counts[4 * b + 2] = both, counts[4 * b + 3] = vuv;
  if (sums) sums[2 * b] = s1, sums[2 * b + 1] = s2;
}

}  // namespace

size_t pitch_distance_scratch_bytes(int B, int T, int hop) {
  const size_t ntiles = ((size_t)T / hop + 1 + PD_FR - 1) / PD_FR;
  return (size_t)B * ntiles * sizeof(PitchPart);
}

int run_pitch_distance(const float* a, const float* b, double* period_a, double* period_b, long long* counts, double* sums, void* scratch,
                       int B, int T, int window, int hop, int tau_min, int tau_max, double threshold, hipStream_t st) {
  PitchArgs s;
  s.a = a, s.b = b, s.pa = period_a, s.pb = period_b;
  s.part = (counts || sums) ? static_cast<PitchPart*>(scratch) : nullptr;
  s.T = T, s.frames = T / hop + 1, s.W = window, s.hop = hop, s.tau_min = tau_min, s.tau_max = tau_max;
  s.ntiles = (s.frames + PD_FR - 1) / PD_FR;
  s.span = window + tau_max + (PD_FR - 1) * hop;
  s.threshold = threshold;
  if (window < 16 || window > 2048 || hop < 1 || hop > window || tau_min < 2 || tau_min >= tau_max || tau_max > 1023 ||
      (long long)window * tau_max > (1 << 20) || (!b && (period_b || counts || sums)))
    VQVS_FAIL(-1, "pitch distance: window=%d hop=%d tau_min=%d tau_max=%d outside the kernel's limits", window, hop, tau_min, tau_max);
  const int nsig = b ? 2 : 1;
  const size_t lds = 2 * PD_FR * sizeof(double) + (size_t)nsig * PD_FR * (tau_max + 1) * 8 + (size_t)nsig * s.span * 4;  // <= 107 KiB
  static std::atomic<bool> attr_done[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (!attr_done[dev].load(std::memory_order_acquire)) {
    VQVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pitch_distance_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_done[dev].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL(pitch_distance_kernel, dim3(s.ntiles, B), dim3(PD_NT), lds, st, s);
  VQVS_HIP(hipGetLastError());
  if (s.part) {
    hipLaunchKernelGGL(pitch_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, st, s.part, counts, sums, B, s.ntiles);
    VQVS_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace vqvs
