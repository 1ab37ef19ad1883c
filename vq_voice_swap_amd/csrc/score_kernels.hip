// Cross-entropy scoring of the guidance-model evals: from logits [B, K, L] and targets [B, L], per clip the summed negative
// log-likelihood (f64), the number of positions whose target ranks first / among the first k, and the confusion counts
// [target, argmax] -- one pass over the logits for the integer results, a second (from L2) for the exponentials.
//
// rank(b, l) = #{j : x_j > x_y} + #{j < y : x_j == x_y} on the raw f32 logits: a count, so exact and independent of the order
// the classes are visited in.  The argmax is the first index of the maximum.  The maximum is found in f32 BEFORE any exponential
// is taken (comparisons only: exact and order-free), so every term of the sum is exp(x_j - max) with the final maximum and no
// rescaling factor ever multiplies a partial sum; differences, exp, log and the sums are f64, added in an order fixed by (K, L).
#include <cmath>

#include "kernels.hpp"
#include "sampler_kernels.hpp"

namespace vqvs {

namespace {

constexpr int XS_WAVES = 8;  // waves of a tile workgroup: wave w takes classes w, w + 8, ...

// one class of one position, folded into the running (max, first index of it, rank count)
__device__ __forceinline__ void score_step(float x, int j, float xy, int64_t y, float& m, int& am, int& rank) {
  if (x > m) {
    m = x;
    am = j;
  }
  rank += (x > xy || (x == xy && (int64_t)j < y)) ? 1 : 0;
}

// (max, first index) of two disjoint class subsets; an index of -1 means "no class compared greater than -inf yet"
__device__ __forceinline__ void argmax_merge(float& m, int& am, float om, int oi) {
  if (oi >= 0 && (am < 0 || om > m || (om == m && oi < am))) {
    m = om;
    am = oi;
  }
}

// L > 1.  A workgroup owns 64 consecutive positions of one clip, one per lane, so every load of a class row is 256 contiguous
// bytes; its 8 waves split the classes.  Per-lane partial results meet in LDS: the f32 maxima first (every wave needs the final
// one for its exponentials), then the f64 sums, which wave 0 adds in wave order.  Wave 0 folds the 64 positions by a fixed
// xor-shuffle tree and writes the tile's partials; nothing here depends on B or on the clip's row.
__global__ __launch_bounds__(64 * XS_WAVES) void xent_score_tile_kernel(const float* logits, const int64_t* targets, double* part_nll,
                                                                         int* part_cnt, int k, int64_t* confusion, int K, int L,
                                                                         int ntiles) {
  __shared__ float s_m[XS_WAVES][64];
  __shared__ int s_am[XS_WAVES][64];
  __shared__ int s_rank[XS_WAVES][64];
  __shared__ double s_sum[XS_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.y, l = blockIdx.x * 64 + lane;
  const bool live = l < L;
  const float* col = logits + (size_t)b * K * L + (live ? l : 0);
  const int64_t y = live ? targets[(size_t)b * L + l] : 0;
  const bool valid = live && y >= 0 && y < (int64_t)K;  // (a target outside 0..K-1 is never used as an index)
  const float xy = valid ? col[(size_t)y * L] : 0.f;

  float m = -INFINITY;
  int am = -1, rank = 0;
  if (live) {
#pragma unroll 4
    for (int j = w; j < K; j += XS_WAVES) score_step(col[(size_t)j * L], j, xy, y, m, am, rank);
  }
  s_m[w][lane] = m;
  s_am[w][lane] = am;
  s_rank[w][lane] = rank;
  __syncthreads();
  float M = s_m[0][lane];
#pragma unroll
  for (int i = 1; i < XS_WAVES; ++i) M = s_m[i][lane] > M ? s_m[i][lane] : M;

  double s = 0.0;
  if (live) {
    const double Md = (double)M;
#pragma unroll 4
    for (int j = w; j < K; j += XS_WAVES) s += exp((double)col[(size_t)j * L] - Md);
  }
  s_sum[w][lane] = s;
  __syncthreads();
  if (w != 0) return;

  double S = s_sum[0][lane];
  float mm = s_m[0][lane];
  am = s_am[0][lane];
  rank = s_rank[0][lane];
#pragma unroll
  for (int i = 1; i < XS_WAVES; ++i) {
    S += s_sum[i][lane];
    argmax_merge(mm, am, s_m[i][lane], s_am[i][lane]);
    rank += s_rank[i][lane];
  }
  if (am < 0) am = 0;      // (no logit above -inf: index 0 is the first index of the maximum)
  if (xy != xy) rank = K;  // NaN target logit: it ranks behind every class
  double nll = 0.0;
  if (live) nll = valid ? log(S) - ((double)xy - (double)M) : (double)NAN;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) nll += __shfl_xor(nll, d, 64);
  const int n1 = __popcll(__ballot(valid && rank == 0));
  const int nk = __popcll(__ballot(valid && rank < k));
  if (confusion && valid) atomicAdd(reinterpret_cast<unsigned long long*>(confusion + (size_t)y * K + am), 1ull);
  if (lane == 0) {
    const size_t t = (size_t)b * ntiles + blockIdx.x;
    part_nll[t] = nll;
    part_cnt[2 * t] = n1;
    part_cnt[2 * t + 1] = nk;
  }
}

// one thread -- one writer -- per clip adds the clip's tile partials in tile order
__global__ __launch_bounds__(64) void xent_score_finish_kernel(const double* part_nll, const int* part_cnt, double* nll, int64_t* top1,
                                                                int64_t* topk, int B, int ntiles) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  int64_t n1 = 0, nk = 0;
  for (int i = 0; i < ntiles; ++i) {
    const size_t t = (size_t)b * ntiles + i;
    s += part_nll[t];
    n1 += part_cnt[2 * t];
    nk += part_cnt[2 * t + 1];
  }
  nll[b] = s;
  if (top1) top1[b] = n1;
  if (topk) topk[b] = nk;
}

// L == 1 (a classifier's [B, K] logits).  Lanes run along K; one workgroup of NT threads (one wave when K <= 256) per row.
// Thread t takes classes t, t + NT, ...; the waves fold by xor-shuffles, then in wave order through LDS.
template <int NT>
__global__ __launch_bounds__(NT) void xent_score_row_kernel(const float* logits, const int64_t* targets, double* nll, int64_t* top1,
                                                            int64_t* topk, int k, int64_t* confusion, int K) {
  constexpr int NW = NT / 64;
  __shared__ float s_m[NW];
  __shared__ int s_am[NW];
  __shared__ int s_rank[NW];
  __shared__ double s_sum[NW];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int b = blockIdx.x;
  const float* row = logits + (size_t)b * K;
  const int64_t y = targets[b];
  const bool valid = y >= 0 && y < (int64_t)K;
  const float xy = valid ? row[y] : 0.f;

  float m = -INFINITY;
  int am = -1, rank = 0;
  for (int j = t; j < K; j += NT) score_step(row[j], j, xy, y, m, am, rank);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float om = __shfl_xor(m, d, 64);
    const int oi = __shfl_xor(am, d, 64);
    argmax_merge(m, am, om, oi);
    rank += __shfl_xor(rank, d, 64);
  }
  if (lane == 0) {
    s_m[w] = m;
    s_am[w] = am;
    s_rank[w] = rank;
  }
  __syncthreads();
  m = s_m[0];
  am = s_am[0];
  rank = s_rank[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) {
    argmax_merge(m, am, s_m[i], s_am[i]);
    rank += s_rank[i];
  }

  const double Md = (double)m;
  double s = 0.0;
  for (int j = t; j < K; j += NT) s += exp((double)row[j] - Md);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) s_sum[w] = s;
  __syncthreads();
  if (t != 0) return;
  double S = s_sum[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) S += s_sum[i];
  if (am < 0) am = 0;
  if (xy != xy) rank = K;
  nll[b] = valid ? log(S) - ((double)xy - Md) : (double)NAN;
  if (top1) top1[b] = (valid && rank == 0) ? 1 : 0;
  if (topk) topk[b] = (valid && rank < k) ? 1 : 0;
  if (confusion && valid) atomicAdd(reinterpret_cast<unsigned long long*>(confusion + (size_t)y * K + am), 1ull);
}

}  // namespace

size_t xent_score_scratch_bytes(int B, int L) {
  if (L == 1) return 0;
  return (size_t)B * ((L + 63) / 64) * 16;  // per tile: one double, two ints
}

int run_xent_score(const float* logits, const int64_t* targets, void* scratch, double* nll, int64_t* top1, int64_t* topk, int k,
                   int64_t* confusion, int B, int K, int L, hipStream_t st) {
  if (L == 1) {
    if (K <= 256)
      hipLaunchKernelGGL(xent_score_row_kernel<64>, dim3(B), dim3(64), 0, st, logits, targets, nll, top1, topk, k, confusion, K);
    else
      hipLaunchKernelGGL(xent_score_row_kernel<256>, dim3(B), dim3(256), 0, st, logits, targets, nll, top1, topk, k, confusion, K);
  } else {
    const int ntiles = (L + 63) / 64;
    double* part_nll = reinterpret_cast<double*>(scratch);
    int* part_cnt = reinterpret_cast<int*>(part_nll + (size_t)B * ntiles);
    hipLaunchKernelGGL(xent_score_tile_kernel, dim3(ntiles, B), dim3(64 * XS_WAVES), 0, st, logits, targets, part_nll, part_cnt, k, confusion,
                       K, L, ntiles);
    hipLaunchKernelGGL(xent_score_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, st, part_nll, part_cnt, nll, top1, topk, B, ntiles);
  }
  VQVS_HIP(hipGetLastError());
  return 0;
}

}  // namespace vqvs
