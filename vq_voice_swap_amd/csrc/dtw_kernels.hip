// Dynamic-time-warping alignment of cepstral sequences (include/vqvs.h, vqvs_dtw_distance): per pair the cost of the cheapest
// monotone path from (0, 0) to (Fa-1, Fb-1) under the mel-cepstral local cost, the path's length, and -- with per-frame tracks --
// the counts and sums of the track difference over the path's cells.  Every cell carries what its chosen predecessor carried plus
// its own contribution, so there is no direction matrix and no backtracking pass.
//
// One workgroup per pair walks the anti-diagonals k = i + j; a thread owns the rows i = i_lo + tid, + 256, ... of a diagonal.
// Cell (i, j) reads (i-1, j-1) of diagonal k-2 and (i-1, j), (i, j-1) of diagonal k-1, and one barrier follows the diagonal.  The
// three live diagonals sit in LDS in TWO rings of M slots (M a power of two >= Fa_max), diagonals of one parity sharing a ring:
// row i of diagonal k lives in slot (i - (k >> 1)) mod M, which is the slot of row i-1 of diagonal k-2.  That value is read by
// this very thread, for this very cell, and by nobody else -- so diagonal k is written over diagonal k-2 in place, behind the read,
// and no thread writes a slot another thread reads between two barriers.  (Rows 0..Fa-1 of a diagonal take distinct slots.)
//
// The arithmetic is a fixed sequence of float64 operations compiled with contraction off, in the order the header states; the
// minimum takes the first of equal predecessors in the order diagonal, i-1, j-1.  A pair's values depend on nothing but its own
// inputs: not on B, its row, the padded frame counts or M.
#include <cmath>

#include "kernels.hpp"

namespace vqvs {

namespace {

constexpr int DTW_NT = 256;
constexpr int DTW_MAXF = 2048;  // max Fa_max, Fb_max
constexpr double DTW_DB = 10.0 / 2.302585092994045684;  // 10 / ln 10

struct DtwArgs {
  const float *ca, *cb;    // [B][fa_max][n_ceps], [B][fb_max][n_ceps]
  const int *fa, *fb;      // [B] frame counts: device data, clamped into 1..f*_max before use
  const double *ta, *tb;   // [B][fa_max], [B][fb_max] tracks (NaN: no value) or nullptr
  double* cost;            // out [B]
  int* steps;              // out [B]
  long long* counts;       // out [B][2]: both, vuv -- or nullptr
  double* sums;            // out [B][2]: sum l, sum l^2 -- or nullptr
  int fa_max, fb_max, n_ceps, M;
};

template <bool TRACKS>
__global__ __launch_bounds__(DTW_NT) void dtw_kernel(const DtwArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double dtw_lds[];
  const int M = a.M, mask = M - 1;
  // rings [2][M]: accumulated cost, steps, and with tracks (both | vuv << 16) -- each at most 4095 --, sum l, sum l^2
  double* D = dtw_lds;
  double* S1 = D + 2 * M;
  double* S2 = S1 + (TRACKS ? 2 * M : 0);
  int* NS = reinterpret_cast<int*>(S2 + (TRACKS ? 2 * M : 0));
  unsigned* BV = reinterpret_cast<unsigned*>(NS + 2 * M);
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int Fa = min(max(a.fa[b], 1), a.fa_max), Fb = min(max(a.fb[b], 1), a.fb_max);  // the same in every thread
  const float* ca = a.ca + (size_t)b * a.fa_max * a.n_ceps;
  const float* cb = a.cb + (size_t)b * a.fb_max * a.n_ceps;
  const double* ta = TRACKS ? a.ta + (size_t)b * a.fa_max : nullptr;
  const double* tb = TRACKS ? a.tb + (size_t)b * a.fb_max : nullptr;
  for (int k = 0; k < Fa + Fb - 1; ++k) {
    const int i_lo = max(0, k - (Fb - 1)), i_hi = min(Fa - 1, k);
    const int cur = (k & 1) * M, prev = M - cur;
    for (int i = i_lo + tid; i <= i_hi; i += DTW_NT) {
      const int j = k - i;
      const float* pa = ca + (size_t)i * a.n_ceps;
      const float* pb = cb + (size_t)j * a.n_ceps;
      double s = 0.0;
      for (int c = 1; c < a.n_ceps; ++c) {  // coefficient 0 is left out
        const double d = (double)pa[c] - (double)pb[c];
        s = s + d * d;
      }
      const double d = DTW_DB * sqrt(2.0 * s);
      // slots: own row on diagonal k (= row i-1 on k-2), own row and row i-1 on diagonal k-1
      const int slot = cur + ((i - (k >> 1)) & mask);
      const int left = prev + ((i - ((k - 1) >> 1)) & mask), up = prev + ((i - 1 - ((k - 1) >> 1)) & mask);
      int from = -1;  // the first of the cheapest predecessors in the order diagonal, i-1, j-1
      double best = 0.0;
      if (i > 0 && j > 0) from = slot, best = D[slot];
      if (i > 0 && (from < 0 || D[up] < best)) from = up, best = D[up];
      if (j > 0 && (from < 0 || D[left] < best)) from = left, best = D[left];
      double acc = d, s1 = 0.0, s2 = 0.0;
      int ns = 1;
      unsigned bv = 0;
      if (from >= 0) {
        acc = d + best;
        ns = NS[from] + 1;
        if (TRACKS) bv = BV[from], s1 = S1[from], s2 = S2[from];
      }
      if (TRACKS) {
        const double va = ta[i], vb = tb[j];
        const bool ha = isfinite(va), hb = isfinite(vb);
        if (ha && hb) {
          const double l = vb - va;
          s1 = s1 + l;
          s2 = s2 + l * l;
          bv += 1u;
        } else if (ha != hb) {
          bv += 1u << 16;
        }
        BV[slot] = bv, S1[slot] = s1, S2[slot] = s2;
      }
      D[slot] = acc;
      NS[slot] = ns;
      if (k == Fa + Fb - 2) {  // the last diagonal is the one cell (Fa-1, Fb-1): the pair's one writer
        a.cost[b] = acc;
        a.steps[b] = ns;
        if (TRACKS) {
          a.counts[2 * b] = (long long)(bv & 0xffffu), a.counts[2 * b + 1] = (long long)(bv >> 16);
          a.sums[2 * b] = s1, a.sums[2 * b + 1] = s2;
        }
      }
    }
    __syncthreads();
  }
}

int ring_slots(int fa_max) {
  int M = 1;
  while (M < fa_max) M *= 2;
  return M;
}

size_t dtw_lds_bytes(int M, bool tracks) { return (size_t)2 * M * (tracks ? 8 + 8 + 8 + 4 + 4 : 8 + 4 + 4); }

}  // namespace

int run_dtw_distance(const float* ca, const float* cb, const int* fa, const int* fb, const double* ta, const double* tb, double* cost, int* steps,
                     long long* counts, double* sums, int B, int fa_max, int fb_max, int n_ceps, hipStream_t st) {
  if (fa_max < 1 || fa_max > DTW_MAXF || fb_max < 1 || fb_max > DTW_MAXF)
    VQVS_FAIL(-1, "dtw distance: Fa_max=%d Fb_max=%d outside the kernel's rings", fa_max, fb_max);
  DtwArgs s;
  s.ca = ca, s.cb = cb, s.fa = fa, s.fb = fb, s.ta = ta, s.tb = tb;
  s.cost = cost, s.steps = steps, s.counts = counts, s.sums = sums;
  s.fa_max = fa_max, s.fb_max = fb_max, s.n_ceps = n_ceps, s.M = ring_slots(fa_max);
  const bool tracks = ta != nullptr;
  const size_t lds = dtw_lds_bytes(s.M, tracks);  // at most 128 KiB of the CU's 160
  const void* kernel = tracks ? reinterpret_cast<const void*>(&dtw_kernel<true>) : reinterpret_cast<const void*>(&dtw_kernel<false>);
  if (lds > 64 * 1024) VQVS_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  if (tracks)
    hipLaunchKernelGGL(dtw_kernel<true>, dim3(B), dim3(DTW_NT), lds, st, s);
  else
    hipLaunchKernelGGL(dtw_kernel<false>, dim3(B), dim3(DTW_NT), lds, st, s);
  VQVS_HIP(hipGetLastError());
  return 0;
}

}  // namespace vqvs
