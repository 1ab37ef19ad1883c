// Speaker enrolment (reference train_vqvae_add.py, train_loop.py:438-485): the gradient of the noise-prediction MSE with respect to
// the conditioning vector of every clip, and the optimiser step on the new class_embed rows.  The transposed convolutions and the
// GroupNorm backward are the guidance schedule's (backward_kernels.hip, net.cpp resblock_backward); this file holds what that
// schedule lacks: the loss head, the backward of the one-channel output convolution, the FiLM-coefficient gradient of a block, the
// way back from the FiLM rows to the embedding, and AdamW.  fp32 activations only (VQVS_KIND_PREDICTOR_GRAD).
//
// Every reduction is in a fixed order and without atomics: a workgroup owns a tile, one thread owns an output.
#include <cmath>

#include "kernels.hpp"

namespace vqvs {

namespace {

// ------------------------------------------------------------------------------------
// mse_head: dout = 2 (pred - eps) / T and the squared-error partial sums of the clip, in the summation order of
// ddpm_sqerr_partial_kernel (loss_kernels.hip): a workgroup owns 4096 consecutive samples, thread t takes quads t, t + 256, ... and
// adds the fp32 squares into one fp64 accumulator, the 256 accumulators are folded by xor-shuffles and the four waves in order.
// ------------------------------------------------------------------------------------
constexpr int MSE_CHUNK = 4096;
constexpr int MSE_QUADS = MSE_CHUNK / 4 / 256;

__device__ __forceinline__ f32x4 load_quad(const float* row, int q, int T, bool vec) {
  if (vec) return *reinterpret_cast<const f32x4*>(row + (size_t)q * 4);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < 4; ++j)
    if (q * 4 + j < T) v[j] = row[(size_t)q * 4 + j];
  return v;
}

__global__ __launch_bounds__(256) void mse_head_kernel(const float* pred, const float* eps, float* dout, double* partial, int T, int nchunk,
                                                       float k, int vec) {
  __shared__ double red[4];
  const int b = blockIdx.y;
  const float* prow = pred + (size_t)b * T;
  const float* erow = eps + (size_t)b * T;
  float* drow = dout + (size_t)b * T;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < MSE_QUADS; ++i) {
    const int q = blockIdx.x * (MSE_CHUNK / 4) + i * 256 + threadIdx.x;
    if (q * 4 < T) {
      const f32x4 p = load_quad(prow, q, T, vec);
      const f32x4 e = load_quad(erow, q, T, vec);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (q * 4 + j < T) {
          const float d = e[j] - p[j];
          const float d2 = __fmul_rn(d, d);  // (rounded to fp32 before it meets the fp64 sum, as vqvs_ddpm_sqerr does)
          s += (double)d2;
          if (!vec) drow[(size_t)q * 4 + j] = (p[j] - e[j]) * k;
        }
      }
      if (vec) *reinterpret_cast<f32x4*>(drow + (size_t)q * 4) = (p - e) * k;  // (T % 4 == 0: the quad is whole)
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[(size_t)b * nchunk + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(64) void mse_finish_kernel(const double* partial, float* mse, int B, int T, int nchunk) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int i = 0; i < nchunk; ++i) s += partial[(size_t)b * nchunk + i];
  mse[b] = (float)(s / (double)T);
}

// ------------------------------------------------------------------------------------
// out_conv_bw: the transposed Conv1d(C -> 1, k = 3, pad = 1) of the output head and the GELU backward behind it,
//   d g[s][c] = w[0][c] dout[s+1] + w[1][c] dout[s] + w[2][c] dout[s-1],   du = d g * gelu'(u),  u = x * scale + shift,
// with the tile partial sums (sum du, sum du * u) in the layout gn_bw reads.  One workgroup = one (clip, tile of STAT_TILE rows);
// a thread owns 8 channels of every rpp-th row (bw_act_kernel's walk).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void out_conv_bw_kernel(const OutConvBwArgs a) {
  __shared__ float red[256 * 8 * 2];
  __shared__ float dy[STAT_TILE + 2];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * STAT_TILE;
  const int opr = a.C >> 3;
  const int rpp = 256 / opr;
  const int oct = tid % opr;
  const int r0 = tid / opr;
  const int c = oct * 8;
  for (int r = tid; r < STAT_TILE + 2; r += 256) {
    const int t = t0 - 1 + r;
    dy[r] = (t >= 0 && t < a.L) ? a.dout[(size_t)b * a.L + t] : 0.f;
  }
  __syncthreads();
  if (r0 < rpp) {
    f32x8 sc, sh, w0, w1, w2;
    const float2* p = a.ss + (size_t)b * a.C + c;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float2 q = p[j];
      sc[j] = q.x;
      sh[j] = q.y;
      w0[j] = a.w[0 * a.C + c + j];
      w1[j] = a.w[1 * a.C + c + j];
      w2[j] = a.w[2 * a.C + c + j];
    }
    const float* xb = reinterpret_cast<const float*>(a.xf) + (size_t)b * a.L * a.C + c;
    float* ob = reinterpret_cast<float*>(a.du) + (size_t)b * a.L * a.C + c;
    f32x8 s1 = f32x8_zero(), s2 = f32x8_zero();
    for (int r = r0; r < STAT_TILE; r += rpp) {
      const int t = t0 + r;
      if (t >= a.L) break;
      const float dm = dy[r], d0 = dy[r + 1], dp = dy[r + 2];  // dout[t-1], dout[t], dout[t+1]
      const f32x8 x = Elem<float>::load8(xb + (size_t)t * a.C);
      f32x8 du;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float u = fmaf(x[j], sc[j], sh[j]);
        const float g = fmaf(w0[j], dp, fmaf(w1[j], d0, w2[j] * dm));
        du[j] = g * gelu_grad_f(u);
        s1[j] += du[j];
        s2[j] = fmaf(du[j], u, s2[j]);
      }
      Elem<float>::store8(ob + (size_t)t * a.C, du);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[(r0 * a.C + c + j) * 2 + 0] = s1[j];
      red[(r0 * a.C + c + j) * 2 + 1] = s2[j];
    }
  }
  __syncthreads();
  for (int cc = tid; cc < a.C; cc += 256) {
    float q1 = 0.f, q2 = 0.f;
    for (int g = 0; g < rpp; ++g) {  // fixed order
      q1 += red[(g * a.C + cc) * 2 + 0];
      q2 += red[(g * a.C + cc) * 2 + 1];
    }
    float* o = a.partials + (((size_t)b * gridDim.x + blockIdx.x) * a.C + cc) * 2;
    o[0] = q1;
    o[1] = q2;
  }
}

// ------------------------------------------------------------------------------------
// film_grad: the gradient of one ResBlock's FiLM coefficients (unet.py:311-314, u2 = h^ (1 + a) + b):
//   d a_c = sum_l du2[c][l] h^[c][l],   d b_c = sum_l du2[c][l],   h^ = gamma rstd (h1 - mean) + beta
// reduced DIRECTLY from the two tensors (never from gn_bw's S1 / S2, which would divide by 1 + a).  Stage 1: a workgroup owns a
// tile of STAT_TILE rows of one clip and streams du2 and h1 once, fp32 per thread, the row groups folded in order.  Stage 2: one
// thread per (clip, channel) adds the tile partials in tile order in fp64 and is the only writer of its two dfilm entries.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void film_grad_tile_kernel(const FilmGradArgs a) {
  __shared__ float red[256 * 8 * 2];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * STAT_TILE;
  const int opr = a.C >> 3;   // octets per row (<= 256)
  const int rpp = 256 / opr;  // rows per pass
  const int oct = tid % opr;
  const int r0 = tid / opr;
  const int c = oct * 8;
  if (r0 < rpp) {
    f32x8 gr, mean, beta;
    const float2* mr = a.mr + (size_t)b * a.C + c;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float2 q = mr[j];
      mean[j] = q.x;
      gr[j] = a.gamma[c + j] * q.y;
      beta[j] = a.beta[c + j];
    }
    const float* db = reinterpret_cast<const float*>(a.du) + (size_t)b * a.L * a.C + c;
    const float* hb = reinterpret_cast<const float*>(a.h1) + (size_t)b * a.L * a.C + c;
    f32x8 sa = f32x8_zero(), sb = f32x8_zero();
    for (int r = r0; r < STAT_TILE; r += rpp) {
      const int t = t0 + r;
      if (t >= a.L) break;
      const f32x8 du = Elem<float>::load8(db + (size_t)t * a.C);
      const f32x8 h = Elem<float>::load8(hb + (size_t)t * a.C);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float hn = fmaf(gr[j], h[j] - mean[j], beta[j]);
        sa[j] = fmaf(du[j], hn, sa[j]);
        sb[j] += du[j];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[(r0 * a.C + c + j) * 2 + 0] = sa[j];
      red[(r0 * a.C + c + j) * 2 + 1] = sb[j];
    }
  }
  __syncthreads();
  for (int cc = tid; cc < a.C; cc += 256) {
    float q1 = 0.f, q2 = 0.f;
    for (int g = 0; g < rpp; ++g) {  // fixed order
      q1 += red[(g * a.C + cc) * 2 + 0];
      q2 += red[(g * a.C + cc) * 2 + 1];
    }
    float* o = a.partials + (((size_t)b * a.ntiles + blockIdx.x) * a.C + cc) * 2;
    o[0] = q1;
    o[1] = q2;
  }
}

__global__ __launch_bounds__(256) void film_grad_finish_kernel(const FilmGradArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (c >= a.C) return;
  const float* p = a.partials + (size_t)b * a.ntiles * a.C * 2;
  double s1 = 0.0, s2 = 0.0;
  for (int t = 0; t < a.ntiles; ++t) {
    const float2 q = *reinterpret_cast<const float2*>(p + ((size_t)t * a.C + c) * 2);
    s1 += (double)q.x;
    s2 += (double)q.y;
  }
  float* o = a.dfilm + (size_t)b * a.film_stride + a.film_off;
  o[c] = (float)s1;         // d a
  o[a.C + c] = (float)s2;   // d b
}

// ------------------------------------------------------------------------------------
// film_bw: d g = Wall^T dfilm (Wall is stored transposed, [E][R]: row e is contiguous), then d v = gelu'(emb) * d g.
// One workgroup per embedding entry e; up to FB_NB clips share one pass over the weight row.  fp64 accumulators, folded by
// xor-shuffles and the four waves in order.
// ------------------------------------------------------------------------------------
constexpr int FB_NB = 8;
__global__ __launch_bounds__(256) void film_bw_kernel(const FilmBwArgs a, int B) {
  __shared__ double red[4][FB_NB];
  const int e = blockIdx.x, tid = threadIdx.x;
  const float* w = a.wT + (size_t)e * a.R;
  for (int b0 = 0; b0 < B; b0 += FB_NB) {
    const int nb = min(FB_NB, B - b0);
    double acc[FB_NB];
#pragma unroll
    for (int k = 0; k < FB_NB; ++k) acc[k] = 0.0;
    for (int r = tid; r < a.R; r += 256) {
      const double wv = (double)w[r];
#pragma unroll
      for (int k = 0; k < FB_NB; ++k)
        if (k < nb) acc[k] += wv * (double)a.dfilm[(size_t)(b0 + k) * a.R + r];
    }
#pragma unroll
    for (int k = 0; k < FB_NB; ++k) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) acc[k] += __shfl_xor(acc[k], m, 64);
    }
    __syncthreads();  // (the previous pass has read red)
    if ((tid & 63) == 0) {
#pragma unroll
      for (int k = 0; k < FB_NB; ++k) red[tid >> 6][k] = acc[k];
    }
    __syncthreads();
    if (tid < nb) {
      const double dg = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
      const size_t i = (size_t)(b0 + tid) * a.E + e;
      a.grad[i] = (float)(dg * (double)gelu_grad_f(a.emb[i]));
    }
  }
}

// ------------------------------------------------------------------------------------
// embed_adamw: one thread per (row, e).  g = (sum of the gradients of the clips that name the row, in clip order) / B, then
// torch.optim.AdamW's update: p *= 1 - lr wd;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
// p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps).  Evaluated in fp64 from the fp32 state, rounded once per stored value.
// ------------------------------------------------------------------------------------
struct AdamArgs {
  float *rows, *m, *v;
  const float* grad;
  const int64_t* row_of_clip;
  int n, B, E;
  double lr, beta1, beta2, eps, wd, bc1, bc2_sqrt;
};
__global__ __launch_bounds__(256) void embed_adamw_kernel(const AdamArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.n * a.E) return;
  const int row = (int)(i / a.E), e = (int)(i % a.E);
  double g = 0.0;
  for (int b = 0; b < a.B; ++b)
    if (a.row_of_clip[b] == (int64_t)row) g += (double)a.grad[(size_t)b * a.E + e];
  g /= (double)a.B;
  const double m = a.beta1 * (double)a.m[i] + (1.0 - a.beta1) * g;
  const double v = a.beta2 * (double)a.v[i] + (1.0 - a.beta2) * g * g;
  double p = (double)a.rows[i] * (1.0 - a.lr * a.wd);
  p -= (a.lr / a.bc1) * m / (sqrt(v) / a.bc2_sqrt + a.eps);
  a.m[i] = (float)m;
  a.v[i] = (float)v;
  a.rows[i] = (float)p;
}

// ------------------------------------------------------------------------------------
// head_xent_grad: classifier enrolment (vqvs_head_xent_grad).  The head of the grown classifier, GELU -> Linear(F, K + n), on the stem's
// feature vector, its softmax cross-entropy, and the coefficients of the closed-form gradient of the n new rows:
//   d nll_b / d W[K + j, :] = (softmax_b[K + j] - [y_b == K + j]) * gelu(feat_b),   d nll_b / d bias[K + j] = the same coefficient.
// One workgroup of four waves per clip; nothing it does depends on B or on the clip's row.
//   1. act[f] = gelu_f(feat[f]) in f32: the value cls_head_kernel forms (common.hpp), kept in LDS.
//   2. wave w takes logits w, w + 4, ...: lane l adds the products of f = l, l + 64, ... into one f64 accumulator (the product of two
//      f32 values is exact in f64, so only the sums round), the 64 accumulators fold by xor-shuffles 32, 16, ... 1, the bias is added
//      last.  The f64 logits stay in LDS (8 bytes each: 64 KiB at the limit of 8192).
//   3. maximum and its first index over the f64 logits (comparisons: exact in any order).
//   4. S = sum exp(logit - max), and the same sum over the new labels alone: thread t adds k = t, t + 256, ..., lanes fold by
//      xor-shuffles, the four waves in wave order.  Every thread then holds the same S.
// One writer per output, no atomics.
// ------------------------------------------------------------------------------------
constexpr int HX_NT = 256, HX_NW = HX_NT / 64;
struct HeadXentArgs {
  const float* feat;        // [B][F]
  const float* w_old;       // [K][F]
  const float* b_old;       // [K]
  const float* rows;        // [n][F + 1], column F is the bias
  const int64_t* targets;   // [B]
  float* act;               // [B][F] or nullptr
  float* logits;            // [B][K + n] or nullptr
  double* nll;              // [B]
  int64_t* top1;            // [B] or nullptr
  double* new_mass;         // [B] or nullptr
  double* coef;             // [B][n]
  int F, K, n;
};
__global__ __launch_bounds__(HX_NT) void head_xent_grad_kernel(const HeadXentArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hx_lds[];
  __shared__ double s_m[HX_NW], s_sum[HX_NW], s_new[HX_NW];
  __shared__ int s_am[HX_NW];
  const int F = a.F, K = a.K, N = a.K + a.n;
  double* lg = reinterpret_cast<double*>(hx_lds);  // [N]
  float* act = reinterpret_cast<float*>(lg + N);   // [F]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int b = blockIdx.x;

  for (int f = t; f < F; f += HX_NT) {
    const float g = gelu_f(a.feat[(size_t)b * F + f]);
    act[f] = g;
    if (a.act) a.act[(size_t)b * F + f] = g;
  }
  __syncthreads();

  for (int k = w; k < N; k += HX_NW) {
    const float* row = k < K ? a.w_old + (size_t)k * F : a.rows + (size_t)(k - K) * (F + 1);
    double acc = 0.0;
    for (int f = lane; f < F; f += 64) acc += (double)row[f] * (double)act[f];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if (lane == 0) lg[k] = acc + (double)(k < K ? a.b_old[k] : row[F]);
  }
  __syncthreads();

  double m = -INFINITY;
  int am = -1;
  for (int k = t; k < N; k += HX_NT) {
    const double x = lg[k];
    if (a.logits) a.logits[(size_t)b * N + k] = (float)x;
    if (x > m) {
      m = x;
      am = k;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double om = __shfl_xor(m, d, 64);
    const int oi = __shfl_xor(am, d, 64);
    if (oi >= 0 && (am < 0 || om > m || (om == m && oi < am))) {
      m = om;
      am = oi;
    }
  }
  if (lane == 0) {
    s_m[w] = m;
    s_am[w] = am;
  }
  __syncthreads();
  m = s_m[0];
  am = s_am[0];
#pragma unroll
  for (int i = 1; i < HX_NW; ++i) {
    const double om = s_m[i];
    const int oi = s_am[i];
    if (oi >= 0 && (am < 0 || om > m || (om == m && oi < am))) {
      m = om;
      am = oi;
    }
  }

  double s = 0.0, sn = 0.0;
  for (int k = t; k < N; k += HX_NT) {
    const double e = exp(lg[k] - m);
    s += e;
    if (k >= K) sn += e;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    s += __shfl_xor(s, d, 64);
    sn += __shfl_xor(sn, d, 64);
  }
  if (lane == 0) {
    s_sum[w] = s;
    s_new[w] = sn;
  }
  __syncthreads();
  double S = s_sum[0], Sn = s_new[0];
#pragma unroll
  for (int i = 1; i < HX_NW; ++i) {
    S += s_sum[i];
    Sn += s_new[i];
  }

  const int64_t y = a.targets[b];
  const bool valid = y >= 0 && y < (int64_t)N;  // (an invalid target is never used as an index)
  for (int j = t; j < a.n; j += HX_NT) {
    const double p = exp(lg[K + j] - m) / S;
    a.coef[(size_t)b * a.n + j] = valid ? p - (y == (int64_t)(K + j) ? 1.0 : 0.0) : (double)NAN;
  }
  if (t != 0) return;
  a.nll[b] = valid ? log(S) - (lg[valid ? y : 0] - m) : (double)NAN;
  if (a.top1) a.top1[b] = (valid && (int64_t)am == y) ? 1 : 0;
  if (a.new_mass) a.new_mass[b] = Sn / S;
}

// ------------------------------------------------------------------------------------
// head_adamw: the gradient of the batch-mean NLL with respect to the new rows and one AdamW step on them (vqvs_head_adamw).  One thread
// per (row j, column f): g = (sum over b ascending of coef[b][j] * act[b][f], fused multiply-adds in f64) / B, act[b][F] = 1 for the
// bias column; then embed_adamw_kernel's update, to the letter.
// ------------------------------------------------------------------------------------
struct HeadAdamArgs {
  float *rows, *m, *v;  // [n][F + 1]
  const float* act;     // [B][F]
  const double* coef;   // [B][n]
  int n, B, F;
  double lr, beta1, beta2, eps, wd, bc1, bc2_sqrt;
};
__global__ __launch_bounds__(256) void head_adamw_kernel(const HeadAdamArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int W = a.F + 1;
  if (i >= (long long)a.n * W) return;
  const int j = (int)(i / W), f = (int)(i % W);
  double g = 0.0;
  if (f < a.F) {
    for (int b = 0; b < a.B; ++b) g = fma(a.coef[(size_t)b * a.n + j], (double)a.act[(size_t)b * a.F + f], g);
  } else {
    for (int b = 0; b < a.B; ++b) g += a.coef[(size_t)b * a.n + j];
  }
  g /= (double)a.B;
  const double m = a.beta1 * (double)a.m[i] + (1.0 - a.beta1) * g;
  const double v = a.beta2 * (double)a.v[i] + (1.0 - a.beta2) * g * g;
  double p = (double)a.rows[i] * (1.0 - a.lr * a.wd);
  p -= (a.lr / a.bc1) * m / (sqrt(v) / a.bc2_sqrt + a.eps);
  a.m[i] = (float)m;
  a.v[i] = (float)v;
  a.rows[i] = (float)p;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

int mse_head_scratch_doubles(int B, int T) { return B * ((T + MSE_CHUNK - 1) / MSE_CHUNK); }

int run_mse_head(const float* pred, const float* eps, float* dout, float* mse, double* scratch, int B, int T, hipStream_t st) {
  const int vec = (T % 4 == 0 && aligned16(pred) && aligned16(eps) && aligned16(dout)) ? 1 : 0;
  const int nchunk = (T + MSE_CHUNK - 1) / MSE_CHUNK;
  const float k = (float)(2.0 / (double)T);
  hipLaunchKernelGGL(mse_head_kernel, dim3(nchunk, B), dim3(256), 0, st, pred, eps, dout, scratch, T, nchunk, k, vec);
  hipLaunchKernelGGL(mse_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, st, scratch, mse, B, T, nchunk);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int launch_out_conv_bw(const OutConvBwArgs& a, int B, hipStream_t st) {
  const int opr = a.C / 8;
  if (a.C % 8 || opr > 256 || opr < 1) VQVS_FAIL(-1, "out_conv_bw: unsupported C=%d", a.C);
  dim3 grid((a.L + STAT_TILE - 1) / STAT_TILE, B);
  hipLaunchKernelGGL(out_conv_bw_kernel, grid, dim3(256), 0, st, a);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int launch_film_grad(const FilmGradArgs& a, int B, hipStream_t st) {
  const int opr = a.C / 8;
  if (a.C % 8 || opr > 256 || opr < 1) VQVS_FAIL(-1, "film_grad: unsupported C=%d", a.C);
  if (a.ntiles != (a.L + STAT_TILE - 1) / STAT_TILE) VQVS_FAIL(-1, "film_grad: %d tiles for %d rows", a.ntiles, a.L);
  if (a.film_off < 0 || a.film_off + 2 * a.C > a.film_stride) VQVS_FAIL(-1, "film_grad: rows %d..%d outside the %d FiLM rows", a.film_off, a.film_off + 2 * a.C, a.film_stride);
  hipLaunchKernelGGL(film_grad_tile_kernel, dim3(a.ntiles, B), dim3(256), 0, st, a);
  hipLaunchKernelGGL(film_grad_finish_kernel, dim3((a.C + 255) / 256, B), dim3(256), 0, st, a);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int launch_film_bw(const FilmBwArgs& a, int B, hipStream_t st) {
  if (a.E < 1 || a.R < 1) VQVS_FAIL(-1, "film_bw: bad shape E=%d R=%d", a.E, a.R);
  hipLaunchKernelGGL(film_bw_kernel, dim3(a.E), dim3(256), 0, st, a, B);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int run_embed_adamw(float* rows, float* m, float* v, const float* grad, const int64_t* row_of_clip, int n, int B, int E, int step, float lr,
                    float beta1, float beta2, float eps, float weight_decay, hipStream_t st) {
  AdamArgs a{rows, m, v, grad, row_of_clip, n, B, E, (double)lr, (double)beta1, (double)beta2, (double)eps, (double)weight_decay, 0.0, 0.0};
  a.bc1 = 1.0 - std::pow(a.beta1, (double)step);
  a.bc2_sqrt = std::sqrt(1.0 - std::pow(a.beta2, (double)step));
  const long long items = (long long)n * E;
  hipLaunchKernelGGL(embed_adamw_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, a);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int run_head_xent_grad(const float* feat, const float* w_old, const float* b_old, const float* rows, const int64_t* targets, float* act,
                       float* logits, double* nll, int64_t* top1, double* new_mass, double* coef, int B, int F, int K, int n,
                       hipStream_t st) {
  const HeadXentArgs a{feat, w_old, b_old, rows, targets, act, logits, nll, top1, new_mass, coef, F, K, n};
  const size_t lds = (size_t)(K + n) * sizeof(double) + (size_t)F * sizeof(float);  // at most 64 KiB + 16 KiB
  static bool attr_set = false;
  if (!attr_set) {
    VQVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&head_xent_grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL(head_xent_grad_kernel, dim3(B), dim3(HX_NT), lds, st, a);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int run_head_adamw(float* rows, float* m, float* v, const float* act, const double* coef, int n, int B, int F, int step, float lr,
                   float beta1, float beta2, float eps, float weight_decay, hipStream_t st) {
  HeadAdamArgs a{rows, m, v, act, coef, n, B, F, (double)lr, (double)beta1, (double)beta2, (double)eps, (double)weight_decay, 0.0, 0.0};
  a.bc1 = 1.0 - std::pow(a.beta1, (double)step);
  a.bc2_sqrt = std::sqrt(1.0 - std::pow(a.beta2, (double)step));
  const long long items = (long long)n * (F + 1);
  hipLaunchKernelGGL(head_adamw_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, a);
  VQVS_HIP(hipGetLastError());
  return 0;
}

}  // namespace vqvs
