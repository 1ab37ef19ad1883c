// Streaming moments of classifier features (vqvs_feature_moments, include/vqvs.h): the on-device half of the reference's
// stat_generate.py:44-45 (np.mean / np.cov over every clip's feature vector), accumulated batch by batch about a shift K:
//   s1[F] += sum_b (f_b - K),   s2[F][F] += sum_b (f_b - K)(f_b - K)^T.
// Everything is f64: the differences are formed in f64 from the f32 inputs (exact), products and sums run on the f64 MFMA
// (v_mfma_f64_16x16x4_f64).  One workgroup owns one 64 x 64 tile of the upper triangle of s2 and walks b in a fixed order, then
// writes the tile and its mirror image; there are no atomics, so the same sequence of calls gives bitwise-identical sums.
#include "kernels.hpp"

namespace vqvs {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int MT = 64;  // output tile edge (4 waves x a 16-row strip of four 16 x 16 MFMA tiles)
constexpr int KC = 16;  // batch rows staged in LDS per pass (four k-steps of the 16x16x4 MFMA)

__global__ __launch_bounds__(256) void feature_moments_kernel(const float* __restrict__ feat, int B, int F, const float* __restrict__ shift,
                                                              double* __restrict__ s1, double* __restrict__ s2) {
  const int bi = blockIdx.y, bj = blockIdx.x;  // tile rows [64 bi, 64 bi + 64), columns [64 bj, ...): upper triangle only
  if (bj < bi) return;
  __shared__ double xa[KC][MT], xb[KC][MT];  // (f - K) of the staged rows at the tile's row / column features
  __shared__ double tile[MT][MT + 1];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r0 = bi * MT, c0 = bj * MT;
  const bool diag = bi == bj;
  const int col = tid & 63;
  const int ca = r0 + col, cb = c0 + col;
  const double ka = ca < F ? (double)shift[ca] : 0.0, kb = cb < F ? (double)shift[cb] : 0.0;
  f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  double colsum = 0.0;  // diagonal tiles: thread tid < 64 owns s1[r0 + tid]
  for (int b0 = 0; b0 < B; b0 += KC) {
#pragma unroll
    for (int i = 0; i < KC / 4; ++i) {  // rows past B and features past F stage as 0 and add nothing
      const int k = (tid >> 6) + 4 * i, b = b0 + k;
      double va = 0.0, vb = 0.0;
      if (b < B) {
        const float* row = feat + (size_t)b * F;
        if (ca < F) va = (double)row[ca] - ka;
        if (cb < F) vb = (double)row[cb] - kb;
      }
      xa[k][col] = va;
      xb[k][col] = vb;
    }
    __syncthreads();
    if (diag && tid < MT)
      for (int k = 0; k < KC; ++k) colsum += xa[k][tid];
    // A[i][k] = xa[k][16 wv + i], B[k][j] = xb[k][16 t + j]; lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15]
#pragma unroll
    for (int ks = 0; ks < KC; ks += 4) {
      const double av = xa[ks + (lane >> 4)][wv * 16 + (lane & 15)];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double bv = xb[ks + (lane >> 4)][t * 16 + (lane & 15)];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // f64 C/D layout (not the f32 one): lane l, register g holds row (l >> 4) + 4 g, column l & 15
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) tile[wv * 16 + (lane >> 4) + 4 * g][t * 16 + (lane & 15)] = acc[t][g];
  __syncthreads();
  // the tile (on a diagonal tile its upper half, diagonal included), coalesced along columns; the new values stay in LDS ...
  for (int e = tid; e < MT * MT; e += 256) {
    const int r = e >> 6, c = e & 63, gr = r0 + r, gc = c0 + c;
    if (gr < F && gc < F && (!diag || r <= c)) {
      double* p = s2 + (size_t)gr * F + gc;
      const double v = *p + tile[r][c];
      *p = v;
      tile[r][c] = v;
    }
  }
  __syncthreads();
  // ... and are copied to the mirror image, coalesced along its columns (a symmetric s2 stays exactly symmetric)
  for (int e = tid; e < MT * MT; e += 256) {
    const int c = e >> 6, r = e & 63, gr = r0 + r, gc = c0 + c;
    if (gr < F && gc < F && (!diag || r < c)) s2[(size_t)gc * F + gr] = tile[r][c];
  }
  if (diag && tid < MT && r0 + tid < F) s1[r0 + tid] += colsum;
}

}  // namespace

int launch_feature_moments(const float* feat, int B, int F, const float* shift, double* s1, double* s2, hipStream_t st) {
  if (B < 1 || F < 1 || F > 8192) VQVS_FAIL(-1, "feature moments: unsupported B=%d F=%d", B, F);
  const int nb = (F + MT - 1) / MT;
  hipLaunchKernelGGL(feature_moments_kernel, dim3(nb, nb), dim3(256), 0, st, feat, B, F, shift, s1, s2);
  VQVS_HIP(hipGetLastError());
  return 0;
}

}  // namespace vqvs
