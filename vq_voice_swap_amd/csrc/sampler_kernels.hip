// DDPM, DDIM and DPM-Solver++(2M) reverse-step kernels, the keep region, the counter-based normal generator, and the VQ codebook search.
// All of these are HBM-bound elementwise / small-reduction kernels.  A reverse step is a RULE on a LAYOUT ("Rules and layouts" below):
// DdpmRule, DdimRule<GUIDED> and DpmppRule<GUIDED> hold what is a sampler's own -- coefficients, x0-sum summand, noise, history and
// the per-sample arithmetic, whose device functions spell out every rounding --, and three kernel templates hold where the samples
// lie: step_clips_kernel (a batch of clips [B, T]), step_windows_kernel (ONE long row seen through overlapping windows) and
// step_packed_kernel (many such rows end to end, stepped by one launch through the same per-quad body, windows_quad).  Every step
// kernel takes one StepArgs by value; x0sum_kernel / x0sum_packed_kernel, which read five of its members, form the sums of CONSTRAIN.  The keep kernels come on clips
// and on windows too and share quad_windows and store_quad with the steps.
#include "kernels.hpp"
#include "pack_table.hpp"
#include "philox.hpp"
#include "sampler_kernels.hpp"

namespace vqvs {

namespace {

__global__ __launch_bounds__(256) void randn_kernel(float* out, int T, uint64_t seed, uint64_t clip_offset, uint32_t stream_id) {
  const int b = blockIdx.y;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q * 4 >= T) return;
  const f32x4 n = philox_normal4(seed, (uint32_t)q, clip_offset + b, 0u, stream_id);
  float* o = out + (size_t)b * T + q * 4;
  if (q * 4 + 3 < T) {
    *reinterpret_cast<f32x4*>(o) = n;
  } else {
    for (int j = 0; q * 4 + j < T; ++j) o[j] = n[j];
  }
}

struct StepCoef {
  float c1, c2, sig, sq1mat, rsat, sqat, rs1mat, c3;
};

// per-clip scalars, evaluated in the reference's operation order (diffusion.py:64-78)
__device__ __forceinline__ StepCoef step_coef(float a_t, float a_prev, bool sigma_large) {
  StepCoef k;
  const float alphas = a_t / a_prev;
  const float betas = 1.0f - alphas;
  const float om = 1.0f - a_t;
  k.c1 = 1.0f / sqrtf(alphas);
  k.c2 = betas * (1.0f / sqrtf(om));
  const float sig2 = sigma_large ? betas : betas * (1.0f - a_prev) / om;
  k.sig = sqrtf(sig2);
  k.sq1mat = sqrtf(om);
  k.rsat = 1.0f / sqrtf(a_t);
  k.sqat = sqrtf(a_t);
  k.rs1mat = 1.0f / sqrtf(om);
  k.c3 = sig2;
  return k;
}

constexpr int SUM_CHUNK = 4096;
inline int sum_chunks(int len) { return (len + SUM_CHUNK - 1) / SUM_CHUNK; }

// *out = the sum of `s` over the 256 threads of the workgroup, in fp64: the fixed tree whose stride halves from 128 to 1, thread 0 writes
__device__ __forceinline__ void block_sum_256(double s, double* out) {
  __shared__ double red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int m = 128; m >= 1; m >>= 1) {
    if (threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0];
}

// The step noise of one quad (quad `quad` of clip `clip` at `step_index`, stream 0) times noise_scale: read from `noise` -- `live`
// samples at element `base` --, or drawn when it is NULL.
__device__ __forceinline__ void step_noise_tail(float* nv, const float* noise, size_t base, int live, float noise_scale, uint64_t seed,
                                                uint32_t quad, uint64_t clip, uint32_t step_index) {
  if (noise) {
    for (int j = 0; j < live; ++j) nv[j] = noise[base + j] * noise_scale;
  } else {
    const f32x4 z = philox_normal4(seed, quad, clip, step_index, 0u);
    for (int j = 0; j < 4; ++j) nv[j] = z[j] * noise_scale;
  }
}
// ... of a whole, 16-byte aligned quad at element p
__device__ __forceinline__ f32x4 step_noise_quad(const float* noise, int p, float noise_scale, uint64_t seed, uint32_t quad, uint64_t clip,
                                                 uint32_t step_index) {
  const f32x4 z = noise ? *reinterpret_cast<const f32x4*>(noise + p) : philox_normal4(seed, quad, clip, step_index, 0u);
  f32x4 nv;
  for (int j = 0; j < 4; ++j) nv[j] = z[j] * noise_scale;
  return nv;
}

// ONE long signal x [Np], Np = (n - 1) * H + W, seen through n windows of W samples, one every H ([n, W] arrays); V = W - H <= H, so a
// sample lies in one window or in two.  A thread owns the quad at absolute position p = 4 q: W and H are multiples of 4, so the quad
// lies in the same window(s), and every access is 16 bytes wide.  Window `br` is the last one that starts at or before p, and the
// quad is at offset u = p - br * H in it; the window before covers it too (`two`) while u < V, at offset u + H.  at_r / at_l are the
// quad's elements in an [n, W] array: window br's copy, and window br - 1's (0 without one).
struct QuadWindows {
  int br, u;
  bool two;
  size_t at_r, at_l;
};
__device__ __forceinline__ QuadWindows quad_windows(int p, int n, int W, int H) {
  QuadWindows g;
  g.br = min(p / H, n - 1);
  g.u = p - g.br * H;
  g.two = g.br > 0 && g.u < W - H;
  g.at_r = (size_t)g.br * W + g.u;
  g.at_l = g.two ? (size_t)(g.br - 1) * W + g.u + H : 0;
  return g;
}
// a finished quad goes to the long row and, for the next forward, to its copy in every window that covers it (win NULL: not wanted)
template <typename Store>
__device__ __forceinline__ void store_quad(float* x, float* win, int p, const QuadWindows& g, Store store) {
  store(x + p);
  if (win) {
    store(win + g.at_r);
    if (g.two) store(win + g.at_l);
  }
}

// mean of x0 over one clip / window: the chunk partials of x0sum_kernel added in chunk order
__device__ __forceinline__ float x0_mean(const double* partial, int nchunk, int T) {
  double s = 0.0;
  for (int i = 0; i < nchunk; ++i) s += partial[i];
  return (float)(s / (double)T);
}

// One sample of the DDPM reverse step, on every layout (diffusion.py:84-90): with `constrain` the prediction is re-derived from x0
// clamped about the clip's (window's) own mean; BLEND cross-fades a left and a right window's predictions, each re-derived with its
// own mean, with weight w on the right one.  Without BLEND the right-hand arguments are unused.  Every rounding is spelled out
// (contraction off, fmaf where the single-clip step has always fused), so that the layouts -- and the two sides of BLEND -- round
// alike whatever surrounds the call: at one window the result is the clip's to the bit.
__device__ __forceinline__ float constrained_eps(const StepCoef& k, float x, float e, float mean) {
#pragma clang fp contract(off)
  float x0 = fmaf(fmaf(-k.sq1mat, e, x), k.rsat, -mean);
  x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
  return fmaf(-x0, k.sqat, x) * k.rs1mat;
}

template <bool BLEND>
__device__ __forceinline__ float step_sample(const StepCoef& k, bool constrain, float x, float nv, float e, float mean, float e_r = 0.f,
                                             float mean_r = 0.f, float w = 0.f) {
#pragma clang fp contract(off)
  if (constrain) e = constrained_eps(k, x, e, mean);
  if (BLEND) {
    if (constrain) e_r = constrained_eps(k, x, e_r, mean_r);
    e = fmaf(w, e_r - e, e);
  }
  return k.c1 * fmaf(-k.c2, e, x) + k.sig * nv;
}

// mean = eps_to_prev(eps)
__global__ __launch_bounds__(256) void ddpm_mean_kernel(const float* x_t, const float* eps, const float* a_t, const float* a_prev, float* out, int T) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const StepCoef k = step_coef(a_t[b], a_prev[b], false);
  const size_t i = (size_t)b * T + t;
  out[i] = k.c1 * (x_t[i] - k.c2 * eps[i]);
}

// eps' = prev_to_eps(mean + sigma^2 * grad) = (-(mean + s2 g) * sqrt(alpha) + x_t) * sqrt(1-a_t) / beta
__global__ __launch_bounds__(256) void ddpm_guided_eps_kernel(const float* x_t, const float* mean, const float* grad, const float* a_t,
                                                              const float* a_prev, float* out, int T, uint32_t flags) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const float at = a_t[b], ap = a_prev[b];
  const StepCoef k = step_coef(at, ap, flags & VQVS_DDPM_SIGMA_LARGE);
  const float alphas = at / ap;
  const float betas = 1.0f - alphas;
  const size_t i = (size_t)b * T + t;
  const float m = mean[i] + k.c3 * grad[i];
  out[i] = (-m * sqrtf(alphas) + x_t[i]) * k.sq1mat / betas;
}

// ---------------------------------------------------------------------------------
// DDIM step (Song et al. 2020; the reference has none), include/vqvs.h "DDIM step".  From alpha_bar a_t of the time the state is at
// to alpha_bar a_to of the time stepped TO:
//   x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t),   x_to = sqrt(a_to) x0 + sqrt(1 - a_to - sig^2) e' + sig z
// with e the prediction less sqrt(1 - a_t) * grad under guidance, and e' = e or, with CONSTRAIN, e re-derived from x0 clamped about
// the clip's mean (constrained_eps' two halves).  There is no reference operation order to follow, so the per-row scalars are formed
// in fp64 from the fp32 alphas and rounded to fp32 ONCE: no cancellation in 1 - a_to - sig^2, and every coefficient carries a single
// rounding (tests/ddim_ref.py counts them).
// ---------------------------------------------------------------------------------
struct DdimCoef {
  float sq1mat, rsat, sqat, rs1mat, sqto, sig, ce;
};

// the fp64 scalars of the x0 prediction: shared by the coefficients below and by DdimSum
struct DdimX0Coef {
  double sq1mat, rsat;
};
__device__ __forceinline__ DdimX0Coef ddim_x0_coef(float a_t) {
  const double at = (double)a_t;
  return {sqrt(1.0 - at), 1.0 / sqrt(at)};
}

__device__ __forceinline__ DdimCoef ddim_coef(float a_t, float a_to, float eta, bool invert) {
  const double at = (double)a_t, ato = (double)a_to, om = 1.0 - at;
  const DdimX0Coef x = ddim_x0_coef(a_t);
  double sig = 0.0;
  if (!invert && om != 0.0) sig = (double)eta * sqrt(fmax((1.0 - ato) / om, 0.0)) * sqrt(fmax(1.0 - at / ato, 0.0));
  DdimCoef k;
  k.sq1mat = (float)x.sq1mat;
  k.rsat = (float)x.rsat;
  k.sqat = (float)sqrt(at);
  k.rs1mat = (float)(1.0 / x.sq1mat);
  k.sqto = (float)sqrt(ato);
  k.sig = (float)sig;
  k.ce = (float)sqrt(fmax(1.0 - ato - sig * sig, 0.0));
  return k;
}

// (x0, e') of one sample under one clip's / window's prediction e and gradient g (guided: e <- e - sqrt(1 - a_t) g)
template <bool GUIDED>
__device__ __forceinline__ void ddim_x0_eps(const DdimCoef& k, bool constrain, float x, float e, float g, float mean, float& x0, float& ep) {
#pragma clang fp contract(off)
  if (GUIDED) e = fmaf(-k.sq1mat, g, e);
  if (constrain) {
    x0 = fmaf(fmaf(-k.sq1mat, e, x), k.rsat, -mean);
    x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    ep = fmaf(-x0, k.sqat, x) * k.rs1mat;
  } else {
    x0 = fmaf(-k.sq1mat, e, x) * k.rsat;
    ep = e;
  }
}

// One sample of the DDIM step, on every layout.  BLEND cross-fades the (x0, e') of a left and a right window, each guided and
// constrained on its own, with weight w on the right one; without BLEND the right-hand arguments are unused.  Every rounding is
// spelled out, as in step_sample: at one window the result is the clip's to the bit.
template <bool BLEND, bool GUIDED>
__device__ __forceinline__ float ddim_sample(const DdimCoef& k, bool constrain, float x, float nv, float e, float g, float mean,
                                             float e_r = 0.f, float g_r = 0.f, float mean_r = 0.f, float w = 0.f) {
#pragma clang fp contract(off)
  float x0, ep;
  ddim_x0_eps<GUIDED>(k, constrain, x, e, g, mean, x0, ep);
  if (BLEND) {
    float x0_r, ep_r;
    ddim_x0_eps<GUIDED>(k, constrain, x, e_r, g_r, mean_r, x0_r, ep_r);
    x0 = fmaf(w, x0_r - x0, x0);
    ep = fmaf(w, ep_r - ep, ep);
  }
  return fmaf(k.sqto, x0, fmaf(k.ce, ep, k.sig * nv));
}

// ---------------------------------------------------------------------------------
// DPM-Solver++(2M) step (Lu et al. 2022, "DPM-Solver++", Algorithm 2; the reference has none), include/vqvs.h "DPM-Solver++(2M)
// step".  The second-order multistep solver of the probability-flow ODE in data-prediction form: from alpha_bar a_t to a_to, with
// alpha = sqrt(a), sigma = sqrt(1 - a), lambda(a) = (log a - log1p(-a)) / 2,
//   x_to = (sigma_to / sigma_t) x + phi ((1 + q) x0 - q x0_prev),   phi = alpha_to - sigma_to alpha_t / sigma_t,   q = h / (2 h_prev)
// h = lambda(a_to) - lambda(a_t), h_prev = lambda(a_t) - lambda(a_from); x0 is the DDIM step's guided, constrained prediction
// (ddim_x0_coef, ddim_x0_eps, DdimSum) and x0_prev the one the step before formed.  Without a usable history q = 0, and the
// step is the eta = 0 DDIM step written in x0.  The scalars are formed in fp64 and rounded to fp32 once, as ddim_coef's are; the two
// logarithms and log1p's cost a few hundred fp64 instructions, so ONE thread of a workgroup forms them and the rest read them from
// LDS, instead of every wave repeating them in front of sixteen bytes of traffic per array.
// ---------------------------------------------------------------------------------
struct DpmppCoef {
  DdimCoef x0;  // sq1mat and rsat alone are set: the x0 half of ddim_x0_eps reads no other
  float cx, c0, c1;
  bool second;  // c1 != 0 is not the test: the history is not read at first order, whatever it holds
};

__device__ __forceinline__ double dpmpp_lambda(double a) { return 0.5 * (log(a) - log1p(-a)); }

// a_from NULL, or no x0_prev (`history` false): first order
__device__ __forceinline__ DpmppCoef dpmpp_coef(const float* a_from, bool history, float a_t, float a_to) {
  const double at = (double)a_t, ato = (double)a_to;
  const DdimX0Coef x = ddim_x0_coef(a_t);
  const double sig_to = sqrt(1.0 - ato);
  const double phi = sqrt(ato) - sig_to * sqrt(at) / x.sq1mat;
  double q = 0.0;
  bool second = false;
  if (history && a_from && 1.0 - ato != 0.0) {
    const double lt = dpmpp_lambda(at);
    const double h = dpmpp_lambda(ato) - lt, h_prev = lt - dpmpp_lambda((double)a_from[0]);
    q = h / (2.0 * h_prev);
    second = h_prev > 0.0 && isfinite(q);
  }
  if (!second) q = 0.0;
  DpmppCoef k;
  k.x0 = DdimCoef{(float)x.sq1mat, (float)x.rsat, 0.f, 0.f, 0.f, 0.f, 0.f};
  k.cx = (float)(sig_to / x.sq1mat);
  k.c0 = (float)(phi * (1.0 + q));
  k.c1 = (float)(-phi * q);
  k.second = second;
  return k;
}

// x0 of one sample under one clip's / window's prediction: the x0 half of ddim_x0_eps (its e' is not formed once inlined)
template <bool GUIDED>
__device__ __forceinline__ float dpmpp_x0(const DpmppCoef& k, bool constrain, float x, float e, float g, float mean) {
  float x0, ep;
  ddim_x0_eps<GUIDED>(k.x0, constrain, x, e, g, mean, x0, ep);
  return x0;
}

// the output line: every rounding spelled out, so that every layout rounds alike
__device__ __forceinline__ float dpmpp_out(const DpmppCoef& k, float x, float x0, float x0_prev) {
#pragma clang fp contract(off)
  return fmaf(k.cx, x, k.second ? fmaf(k.c0, x0, k.c1 * x0_prev) : k.c0 * x0);
}

// ---------------------------------------------------------------------------------
// Rules and layouts.  A step is a RULE -- what a sampler does to one sample -- run on a LAYOUT -- where the samples of a state lie:
// step_clips_kernel (B rows of T), step_windows_kernel (one long row under n overlapping windows) and step_packed_kernel (R such
// rows end to end) are each instantiated with DdpmRule, DdimRule<GUIDED> and DpmppRule<GUIDED>.  A layout finds a thread's quad,
// loads what every rule reads of it (x, eps and, for a GUIDED rule, grad -- per covering window --, the x0 means, the noise, the
// history), hands the values to the rule sample by sample and stores what comes back; it knows no sampler by name.  A rule holds
//   Coef, coef(a, b)     the scalars of row b (b = 0 for the one alpha of a windowed state) and how they are formed; SHARED: by one
//                        thread of the workgroup, the others reading them from LDS (workgroup_coef), else by every thread
//   Sum                  the summand of the x0 sums that CONSTRAIN needs (x0sum_kernel)
//   WIDE                 the clips layout may take 16-byte accesses where the arrays allow (else one sample at a time, as ever)
//   draws_noise(k, a)    whether noise enters at all          HISTORY, reads_history(k)   whether x0_out is written / x0_prev read
//   sample<BLEND>(...)   the arithmetic of one sample under one window's view of it (`one`), or blended from two (`left`, and `one` on the
//                        right with weight w); x0 is set by a HISTORY rule alone
// Members of StepArgs that a rule does not read may be NULL: a rule's code holds no access to them.
// ---------------------------------------------------------------------------------
constexpr uint32_t STEP_CONSTRAIN = VQVS_DDPM_CONSTRAIN;
static_assert(VQVS_DDIM_CONSTRAIN == STEP_CONSTRAIN, "the rules share the CONSTRAIN bit");

// one clip's / window's view of a sample: its prediction, its guidance gradient (0 unguided) and the mean of its x0 (0 unconstrained)
struct View {
  float e, g, mean;
};

// the x0 of CONSTRAIN, per sample of a row with alpha_bar `at`.  DDPM: fp32 arithmetic, accumulated in fp64
struct DdpmSum {
  float sq, rs;
  __device__ __forceinline__ explicit DdpmSum(float at) : sq(sqrtf(1.0f - at)), rs(1.0f / sqrtf(at)) {}
  __device__ __forceinline__ double operator()(const float* x_row, const float* eps_row, const float*, int t) const {
    return (double)((x_row[t] - sq * eps_row[t]) * rs);
  }
};
// DDIM and DPM-Solver++: x0 OF THE GUIDED PREDICTION, e = eps - sqrt(1 - a_t) grad (grad_row NULL: e = eps), formed in fp64 from the
// fp32 inputs and the fp64 scalars, so the mean that x0_mean rounds to fp32 carries that one rounding
struct DdimSum {
  DdimX0Coef k;
  __device__ __forceinline__ explicit DdimSum(float at) : k(ddim_x0_coef(at)) {}
  __device__ __forceinline__ double operator()(const float* x_row, const float* eps_row, const float* grad_row, int t) const {
    double e = (double)eps_row[t];
    if (grad_row) e -= k.sq1mat * (double)grad_row[t];
    return ((double)x_row[t] - k.sq1mat * e) * k.rsat;
  }
};

struct DdpmRule {
  using Coef = StepCoef;
  using Sum = DdpmSum;
  static constexpr bool GUIDED = false, SHARED = false, WIDE = false, HISTORY = false;
  static __device__ __forceinline__ Coef coef(const StepArgs& a, int b) { return step_coef(a.a_t[b], a.a_to[b], a.flags & VQVS_DDPM_SIGMA_LARGE); }
  static __device__ __forceinline__ bool draws_noise(const Coef&, const StepArgs& a) { return a.noise_scale != 0.f; }
  static __device__ __forceinline__ bool reads_history(const Coef&) { return false; }
  template <bool BLEND>
  static __device__ __forceinline__ float sample(const Coef& k, bool constrain, float x, float nv, float, const View& one, const View& left,
                                                 float w, float&) {
    if constexpr (BLEND) return step_sample<true>(k, constrain, x, nv, left.e, left.mean, one.e, one.mean, w);
    return step_sample<false>(k, constrain, x, nv, one.e, one.mean);
  }
};

template <bool GUIDED_>
struct DdimRule {
  using Coef = DdimCoef;
  using Sum = DdimSum;
  static constexpr bool GUIDED = GUIDED_, SHARED = false, WIDE = false, HISTORY = false;
  static __device__ __forceinline__ Coef coef(const StepArgs& a, int b) { return ddim_coef(a.a_t[b], a.a_to[b], a.eta, a.flags & VQVS_DDIM_INVERT); }
  // (eta = 0, INVERT, a_to = 1: nothing is drawn or read)
  static __device__ __forceinline__ bool draws_noise(const Coef& k, const StepArgs& a) { return a.noise_scale != 0.f && k.sig != 0.f; }
  static __device__ __forceinline__ bool reads_history(const Coef&) { return false; }
  template <bool BLEND>
  static __device__ __forceinline__ float sample(const Coef& k, bool constrain, float x, float nv, float, const View& one, const View& left,
                                                 float w, float&) {
    if constexpr (BLEND) return ddim_sample<true, GUIDED>(k, constrain, x, nv, left.e, left.g, left.mean, one.e, one.g, one.mean, w);
    return ddim_sample<false, GUIDED>(k, constrain, x, nv, one.e, one.g, one.mean);
  }
};

// The history x0_prev / x0_out holds, per position, the x0 the step formed -- on a windowed state the BLENDED one.  x0_out may be
// x0_prev itself: a layout reads a thread's quad of the history before it stores any.
template <bool GUIDED_>
struct DpmppRule {
  using Coef = DpmppCoef;
  using Sum = DdimSum;
  static constexpr bool GUIDED = GUIDED_, SHARED = true, WIDE = true, HISTORY = true;
  static __device__ __forceinline__ Coef coef(const StepArgs& a, int b) {
    return dpmpp_coef(a.a_from ? a.a_from + b : nullptr, a.x0_prev != nullptr, a.a_t[b], a.a_to[b]);
  }
  static __device__ __forceinline__ bool draws_noise(const Coef&, const StepArgs&) { return false; }
  static __device__ __forceinline__ bool reads_history(const Coef& k) { return k.second; }
  template <bool BLEND>
  static __device__ __forceinline__ float sample(const Coef& k, bool constrain, float x, float, float x0_prev, const View& one, const View& left,
                                                 float w, float& x0) {
#pragma clang fp contract(off)
    x0 = dpmpp_x0<GUIDED>(k, constrain, x, one.e, one.g, one.mean);
    if constexpr (BLEND) {
      const float x0_l = dpmpp_x0<GUIDED>(k, constrain, x, left.e, left.g, left.mean);
      x0 = fmaf(w, x0 - x0_l, x0_l);
    }
    return dpmpp_out(k, x, x0, x0_prev);
  }
};

// Row b's coefficients in every thread of the workgroup, each of which calls this
template <typename Rule>
__device__ __forceinline__ typename Rule::Coef workgroup_coef(const StepArgs& a, int b) {
  if constexpr (Rule::SHARED) {
    __shared__ typename Rule::Coef ks;
    if (threadIdx.x == 0) ks = Rule::coef(a, b);
    __syncthreads();
    return ks;
  } else {
    return Rule::coef(a, b);
  }
}

// Sum over time of a rule's x0, per (row, chunk of SUM_CHUNK samples); fp64 partials [rows, nchunk], which x0_mean adds in chunk
// order.  One chunk of one row:
template <typename Sum>
__device__ __forceinline__ void x0sum_chunk(const float* x_row, const float* eps_row, const float* grad_row, float at, double* out, int T,
                                            int chunk) {
  const Sum x0(at);
  const int beg = chunk * SUM_CHUNK, end = min(T, beg + SUM_CHUNK);
  double s = 0.0;
  for (int t = beg + threadIdx.x; t < end; t += 256) s += x0(x_row, eps_row, grad_row, t);
  block_sum_256(s, out);
}
// Row b of eps (and grad) is [T] contiguous; row b of x starts at b * x_stride and its alpha is a_t[b * a_stride]: (T, 1) for a
// batch of clips, (H, 0) for the overlapping windows of one long signal, which are then summed exactly as a clip is.
template <typename Sum>
__global__ __launch_bounds__(256) void x0sum_kernel(const float* x, const float* eps, const float* grad, const float* a_t, double* partial,
                                                    int T, int nchunk, int x_stride, int a_stride) {
  const int b = blockIdx.y;
  x0sum_chunk<Sum>(x + (size_t)b * x_stride, eps + (size_t)b * T, grad ? grad + (size_t)b * T : nullptr, a_t[b * a_stride],
                   partial + (size_t)b * nchunk + blockIdx.x, T, blockIdx.x);
}

// `live` samples at p: one 16-byte access when `vec` (the quad is whole and aligned in every array), one by one otherwise
__device__ __forceinline__ f32x4 load_quad(const float* p, int live, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    v = *reinterpret_cast<const f32x4*>(p);
  } else {
    for (int j = 0; j < live; ++j) v[j] = p[j];
  }
  return v;
}
__device__ __forceinline__ void store_quad_at(float* p, const f32x4& v, int live, bool vec) {
  if (vec) {
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    for (int j = 0; j < live; ++j) p[j] = v[j];
  }
}

// Clips: B rows of T, row b with its own alphas, mean and -- drawn as clip a.clip + b -- noise; a thread owns four consecutive
// samples of a row.  aligned: T % 4 == 0 and every base pointer is 16-byte aligned; a rule that is not WIDE holds no 16-byte access.
template <typename Rule>
__global__ __launch_bounds__(256) void step_clips_kernel(StepArgs a, int T, bool aligned) {
  const bool vec = Rule::WIDE && aligned;
  const int b = blockIdx.y;
  const int q = blockIdx.x * 256 + threadIdx.x;
  const bool constrain = a.flags & STEP_CONSTRAIN;
  typename Rule::Coef k;
  View v = {0.f, 0.f, 0.f};
  if constexpr (Rule::SHARED) {  // (workgroup_coef, with the row's mean sharing its barrier)
    __shared__ typename Rule::Coef ks;
    __shared__ float means;
    if (threadIdx.x == 0) {
      ks = Rule::coef(a, b);
      means = constrain ? x0_mean(a.partial + (size_t)b * a.nchunk, a.nchunk, T) : 0.f;
    }
    __syncthreads();
    if (q * 4 >= T) return;
    k = ks;
    v.mean = means;
  } else {
    if (q * 4 >= T) return;
    k = Rule::coef(a, b);
    if (constrain) v.mean = x0_mean(a.partial + (size_t)b * a.nchunk, a.nchunk, T);
  }
  const size_t base = (size_t)b * T + q * 4;
  const int n = min(4, T - q * 4);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4 xv = load_quad(a.x + base, n, vec), ev = load_quad(a.eps + base, n, vec);
  f32x4 gv = zero, pv = zero;
  if (Rule::GUIDED) gv = load_quad(a.grad + base, n, vec);
  if (Rule::reads_history(k)) pv = load_quad(a.x0_prev + base, n, vec);
  float nv[4] = {0.f, 0.f, 0.f, 0.f};
  if (Rule::draws_noise(k, a)) step_noise_tail(nv, a.noise, base, n, a.noise_scale, a.seed, (uint32_t)q, a.clip + b, a.step_index);
  f32x4 x0 = zero, o;
  for (int j = 0; j < 4; ++j) {
    v.e = ev[j];
    v.g = gv[j];
    float x0j = 0.f;
    o[j] = Rule::template sample<false>(k, constrain, xv[j], nv[j], pv[j], v, v, 0.f, x0j);
    x0[j] = x0j;
  }
  store_quad_at(a.x_to + base, o, n, vec);
  if constexpr (Rule::HISTORY)
    if (a.x0_out) store_quad_at(a.x0_out + base, x0, n, vec);
}

// Windows: one long signal x [Np] whose predictions came from its n windows (eps, grad [n, W]; quad_windows); partial holds n * nchunk
// chunk sums, one mean per window.  Where two windows cover a quad, what they make of it is cross-faded with w = (u + 1/2) / V on
// the later one.  The noise is one draw per absolute position -- row 0 of a [1, Np] batch at `clip`, as the clips layout draws it --
// so the overlapping windows share it; the history is per absolute position too.  The result goes to x_to [Np] and to win [n, W]
// (store_quad).
// (the body: quad q < Np / 4 of ONE row, every pointer of `a` at that row's first sample / window / partial.  step_windows_kernel runs
// it on the only row there is, step_packed_kernel on the row of a pack that PackRow finds.)
template <typename Rule>
__device__ __forceinline__ void windows_quad(int q, const typename Rule::Coef& k, const StepArgs& a, int n, int W, int H, uint64_t clip) {
  const int V = W - H;
  const int p = q * 4;
  const bool constrain = a.flags & STEP_CONSTRAIN;
  const QuadWindows g = quad_windows(p, n, W, H);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4 xv = *reinterpret_cast<const f32x4*>(a.x + p);
  const f32x4 er = *reinterpret_cast<const f32x4*>(a.eps + g.at_r);
  f32x4 el = er, gr = zero, gl = zero, pv = zero;
  if (g.two) el = *reinterpret_cast<const f32x4*>(a.eps + g.at_l);
  if (Rule::GUIDED) {
    gr = *reinterpret_cast<const f32x4*>(a.grad + g.at_r);
    if (g.two) gl = *reinterpret_cast<const f32x4*>(a.grad + g.at_l);
  }
  if (Rule::reads_history(k)) pv = *reinterpret_cast<const f32x4*>(a.x0_prev + p);
  float mean_r = 0.f, mean_l = 0.f;
  if (constrain) {
    mean_r = x0_mean(a.partial + (size_t)g.br * a.nchunk, a.nchunk, W);
    if (g.two) mean_l = x0_mean(a.partial + (size_t)(g.br - 1) * a.nchunk, a.nchunk, W);
  }
  f32x4 nv = zero;
  if (Rule::draws_noise(k, a)) nv = step_noise_quad(a.noise, p, a.noise_scale, a.seed, (uint32_t)q, clip, a.step_index);
  f32x4 x0 = zero, o;
  for (int j = 0; j < 4; ++j) {
    const View one = {er[j], gr[j], mean_r}, left = {el[j], gl[j], mean_l};
    float x0j = 0.f;
    if (g.two) {
      const float w = ((float)(g.u + j) + 0.5f) / (float)V;
      o[j] = Rule::template sample<true>(k, constrain, xv[j], nv[j], pv[j], one, left, w, x0j);
    } else {
      o[j] = Rule::template sample<false>(k, constrain, xv[j], nv[j], pv[j], one, left, 0.f, x0j);
    }
    x0[j] = x0j;
  }
  store_quad(a.x_to, a.win, p, g, [&](float* dst) { *reinterpret_cast<f32x4*>(dst) = o; });
  if constexpr (Rule::HISTORY)
    if (a.x0_out) *reinterpret_cast<f32x4*>(a.x0_out + p) = x0;
}
template <typename Rule>
__global__ __launch_bounds__(256) void step_windows_kernel(StepArgs a, int n, int W, int H) {
  const typename Rule::Coef k = workgroup_coef<Rule>(a, 0);
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= ((n - 1) * H + W) / 4) return;
  windows_quad<Rule>(q, k, a, n, W, H, a.clip);
}

// ---------------------------------------------------------------------------------
// Packed window steps (include/vqvs.h "Packed window steps"): R recordings of n_r windows each, their long
// rows laid end to end and their windows stacked in [N, W] arrays, stepped by ONE launch.  `first` [R + 1] holds the prefix sums of
// the window counts: recording r owns windows first[r] .. first[r + 1] - 1 and starts at sample first[r] * H + r * V of the long
// arrays (every row is n_r * H + V long).  A quad is handed, with every pointer moved to its recording's first sample / window /
// partial, to the windows_quad body the single-recording kernel runs, at clip + r: the arithmetic IS that kernel's on that
// recording alone, and the last window of one recording never meets the first of the next.
//
// N = first[R] lives on the device, so the host cannot size a grid by it: a fixed grid walks the quads in strides of one grid.  A
// workgroup covers 1024 consecutive samples per stride; the recording of its FIRST sample is found by a binary search whose every
// operand is uniform over the workgroup (scalar loads of a table that stays in the scalar cache), and a thread whose quad lies beyond that recording's end walks on from there -- at most a step or two, since a
// recording holds W samples or more.  Table entries are clamped to 0..N and N to 1..65535, and a quad is stepped only where it lies
// inside the row the table gives it, so a malformed table cannot send an access outside N * H + R * V samples or N windows.
// ---------------------------------------------------------------------------------
constexpr int PACK_GRID = 2048;  // 256 CUs x 8 workgroups of 256: every CU full, the rest of a long pack in further strides

// (PackTable, pack_row and pack_window_row: pack_table.hpp, shared with pause_kernels.hip)
__device__ __forceinline__ const float* pack_shift(const float* p, size_t by) { return p ? p + by : nullptr; }
__device__ __forceinline__ float* pack_shift(float* p, size_t by) { return p ? p + by : nullptr; }

// The x0 sums of every window of a pack, partial [N, nchunk]: window b starts at b * H + rec(b) * V of x.  One (window, chunk) per
// workgroup and stride, summed by the body -- and so in the order -- of the single-recording launch.
template <typename Sum>
__global__ __launch_bounds__(256) void x0sum_packed_kernel(const float* x, const float* eps, const float* grad, const float* a_t,
                                                           double* partial, const int* first, int R, int W, int H, int nchunk) {
  const PackTable t = pack_table(first, R, W, H);
  for (int item = blockIdx.x; item < t.N * nchunk; item += gridDim.x) {
    const int b = item / nchunk;
    const size_t start = (size_t)t.off(pack_window_row(t, b), b);
    x0sum_chunk<Sum>(x + start, eps + (size_t)b * W, pack_shift(grad, (size_t)b * W), a_t[0], partial + item, W, item - b * nchunk);
  }
}

template <typename Rule>
__global__ __launch_bounds__(256) void step_packed_kernel(StepArgs a, const int* first, int R, int W, int H) {
  const typename Rule::Coef k = workgroup_coef<Rule>(a, 0);
  const PackTable t = pack_table(first, R, W, H);
  const int64_t total = t.total();
  for (int64_t p0 = (int64_t)blockIdx.x * 1024; p0 < total; p0 += (int64_t)gridDim.x * 1024) {
    const int64_t p = p0 + threadIdx.x * 4;
    if (p >= total) continue;
    const PackRow w = pack_row(t, p0, p);
    if (!w.ok) continue;
    const size_t wo = (size_t)w.fb * W;
    StepArgs row = a;  // the recording's own row: long arrays from its first sample, window arrays and partials from its first window
    row.x = a.x + w.off;
    row.noise = pack_shift(a.noise, w.off);
    row.x0_prev = pack_shift(a.x0_prev, w.off);
    row.x_to = a.x_to + w.off;
    row.x0_out = pack_shift(a.x0_out, w.off);
    row.eps = a.eps + wo;
    row.grad = pack_shift(a.grad, wo);
    row.win = pack_shift(a.win, wo);
    row.partial = a.partial + (size_t)w.fb * a.nchunk;
    windows_quad<Rule>(w.q, k, row, w.n, W, H, a.clip + w.r);
  }
}
// ---------------------------------------------------------------------------------
// Keep region (the "replacement" method of Song et al. 2021; the reference has none), include/vqvs.h "Keep region".  Kept samples of a
// state are put back on the forward process of a source at alpha_bar = alpha:
//   x[p] = fmaf(ca, x0[p], cn * (noise_scale * z)),   ca = sqrt(alpha), cn = sqrt(max(1 - alpha, 0))
// with the coefficients formed in fp64 from the fp32 alpha and rounded to fp32 once, as ddim_coef forms its own.  The state itself is
// never read: a quad without a kept sample costs its four mask bytes, a quad that is kept whole is one 16-byte store, and a quad the
// mask cuts through stores its kept samples one by one, so that a sample outside the mask is not written at all.
// ---------------------------------------------------------------------------------
struct KeepCoef {
  float ca, cn;
};

__device__ __forceinline__ KeepCoef keep_coef(float alpha) {
  const double a = (double)alpha;
  return {(float)sqrt(a), (float)sqrt(fmax(1.0 - a, 0.0))};
}

// The values of the quad at element offset `at` of x0 / keep / noise (`live` of its four samples exist: the tail of a row has fewer)
// and the mask of its kept samples; o is set only where the mask is, and nothing but the mask bytes is read when it is empty.  `vec`:
// the quad is whole and 16-byte aligned in every array, so each array is read with one access.  The noise of quad `quad` of clip
// `clip` is drawn when `noise` is NULL; with cn == 0 or noise_scale == 0 none is drawn or read and the value is ca * x0 -- at
// alpha = 1 the source itself, sign of zero included.
__device__ __forceinline__ uint32_t keep_quad(const float* x0, const uint8_t* keep, const float* noise, size_t at, int live, bool vec,
                                              const KeepCoef& k, float noise_scale, uint64_t seed, uint32_t quad, uint64_t clip,
                                              uint32_t index, f32x4& o) {
#pragma clang fp contract(off)
  uint32_t mask = (1u << live) - 1u;
  if (keep) {
    uint32_t m = 0u;
    if (vec) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(keep + at);
      for (int j = 0; j < 4; ++j) m |= ((w >> (8 * j)) & 0xffu) ? 1u << j : 0u;
    } else {
      for (int j = 0; j < live; ++j) m |= keep[at + j] ? 1u << j : 0u;
    }
    mask &= m;
  }
  if (!mask) return 0u;
  f32x4 sv = {0.f, 0.f, 0.f, 0.f}, zv = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    sv = *reinterpret_cast<const f32x4*>(x0 + at);
  } else {
    for (int j = 0; j < live; ++j) sv[j] = x0[at + j];
  }
  const bool noisy = k.cn != 0.f && noise_scale != 0.f;
  if (noisy) {
    if (!noise) {
      zv = philox_normal4(seed, quad, clip, index, PHILOX_STREAM_KEEP);
    } else if (vec) {
      zv = *reinterpret_cast<const f32x4*>(noise + at);
    } else {
      for (int j = 0; j < live; ++j) zv[j] = noise[at + j];
    }
  }
  for (int j = 0; j < 4; ++j) o[j] = noisy ? fmaf(k.ca, sv[j], k.cn * (noise_scale * zv[j])) : k.ca * sv[j];
  return mask;
}

// the kept samples of a quad to dst: one 16-byte store when all four are kept and the quad is aligned, else the kept ones alone
__device__ __forceinline__ void keep_store(float* dst, const f32x4& o, uint32_t mask, bool vec) {
  if (vec && mask == 0xfu) {
    *reinterpret_cast<f32x4*>(dst) = o;
  } else {
    for (int j = 0; j < 4; ++j)
      if (mask & (1u << j)) dst[j] = o[j];
  }
}

// x [B, T] in place; row b is clip clip_offset + b and has its own alpha.  aligned: T % 4 == 0 and every base pointer is 16-byte
// aligned (keep: 4-byte), so every quad of every row is; otherwise the samples are accessed one by one.
__global__ __launch_bounds__(256) void keep_region_kernel(float* x, const float* x0, const uint8_t* keep, const float* noise,
                                                          const float* alpha, int T, bool aligned, float noise_scale, uint64_t seed,
                                                          uint64_t clip_offset, uint32_t index) {
  const int b = blockIdx.y;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q * 4 >= T) return;
  const KeepCoef k = keep_coef(alpha[b]);
  const size_t at = (size_t)b * T + q * 4;
  const int live = min(4, T - q * 4);
  f32x4 o;
  const uint32_t mask = keep_quad(x0, keep, noise, at, live, aligned, k, noise_scale, seed, (uint32_t)q, clip_offset + b, index, o);
  if (mask) keep_store(x + at, o, mask, aligned);
}

// The same operation on ONE long state x [Np] (quad_windows): x0, keep and noise are indexed by absolute position, there is one
// alpha, the drawn noise is that of one row of Np samples at `clip`, and a kept sample goes to x and to win [n, W] (store_quad).
__global__ __launch_bounds__(256) void keep_region_windows_kernel(float* x, float* win, const float* x0, const uint8_t* keep,
                                                                  const float* noise, const float* alpha, int n, int W, int H, bool aligned,
                                                                  float noise_scale, uint64_t seed, uint64_t clip, uint32_t index) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int Np = (n - 1) * H + W;
  if (q >= Np / 4) return;
  const int p = q * 4;
  const KeepCoef k = keep_coef(alpha[0]);
  f32x4 o;
  const uint32_t mask = keep_quad(x0, keep, noise, (size_t)p, 4, aligned, k, noise_scale, seed, (uint32_t)q, clip, index, o);
  if (!mask) return;
  store_quad(x, win, p, quad_windows(p, n, W, H), [&](float* dst) { keep_store(dst, o, mask, aligned); });
}

// ... and on a PACK of such states (the walk of step_packed_kernel: a fixed grid strides over the pack, pack_row finds the quad's
// recording).  x0, keep and noise are read at the quad's position in the pack; the noise is drawn at the quad's index in its own
// row and at clip + r, and the quad goes to the row's own windows alone, so recording r's slices are what
// keep_region_windows_kernel writes for (n_r, clip + r) on them.
__global__ __launch_bounds__(256) void keep_region_packed_kernel(float* x, float* win, const float* x0, const uint8_t* keep,
                                                                 const float* noise, const float* alpha, const int* first, int R, int W, int H,
                                                                 bool aligned, float noise_scale, uint64_t seed, uint64_t clip, uint32_t index) {
  const KeepCoef k = keep_coef(alpha[0]);
  const PackTable t = pack_table(first, R, W, H);
  const int64_t total = t.total();
  for (int64_t p0 = (int64_t)blockIdx.x * 1024; p0 < total; p0 += (int64_t)gridDim.x * 1024) {
    const int64_t p = p0 + threadIdx.x * 4;
    if (p >= total) continue;
    const PackRow w = pack_row(t, p0, p);
    if (!w.ok) continue;
    f32x4 o;
    const uint32_t mask = keep_quad(x0, keep, noise, (size_t)p, 4, aligned, k, noise_scale, seed, (uint32_t)w.q, clip + w.r, index, o);
    if (!mask) continue;
    const int u = w.q * 4;
    store_quad(x + w.off, pack_shift(win, (size_t)w.fb * W), u, quad_windows(u, w.n, W, H), [&](float* dst) { keep_store(dst, o, mask, aligned); });
  }
}

// ---------------------------------------------------------------------------------
// VQ nearest codeword (reference vq.py:127-131, 199-221).
//   dist[k] = ((-2 * <x, e_k>) + |e_k|^2) + |x|^2   in fp32, dot as an fmaf chain in channel
//   order; argmin with the FIRST minimal index (torch.argmin semantics).
// Workgroup = 32 time positions of one clip; thread (pos = tid&31, cg = tid>>5) scores 16
// codes of every 128-code tile.  z is read in its NCT layout, coalesced along time.
// ---------------------------------------------------------------------------------
constexpr int VQ_POS = 32, VQ_TILE = 128, VQ_KC = 64, VQ_DS = VQ_KC + 4;

__global__ void vq_norms_kernel(const float* dict, float* en, int K, int Cd) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  float s = 0.f;
  for (int c = 0; c < Cd; ++c) s = fmaf(dict[(size_t)k * Cd + c], dict[(size_t)k * Cd + c], s);
  en[k] = s;
}

// The search itself, shared by vq_argmin_kernel and vq_quantize_kernel: after the call thread tid < VQ_POS holds the winning code
// of position t0 + tid (every other thread's return value is meaningless).  The four LDS arrays belong to the caller, which may
// reuse them once it has passed a barrier of its own.
__device__ __forceinline__ int vq_search(const float* zb, const float* dict, const float* en, int Cd, int T1, int K, int t0,
                                         float (*xs)[VQ_POS], float (*ds)[VQ_DS], float (*bd)[VQ_POS], int (*bi)[VQ_POS]) {
  const int tid = threadIdx.x;
  const int pos = tid & 31, cg = tid >> 5;
  float best = INFINITY;
  int best_i = 0;
  float xn = 0.f;
  for (int k0 = 0; k0 < K; k0 += VQ_TILE) {
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    xn = 0.f;
    for (int c0 = 0; c0 < Cd; c0 += VQ_KC) {
      __syncthreads();
      for (int i = tid; i < VQ_KC * VQ_POS; i += 256) {
        const int c = i >> 5, p = i & 31;
        xs[c][p] = (c0 + c < Cd && t0 + p < T1) ? zb[(size_t)(c0 + c) * T1 + t0 + p] : 0.f;
      }
      for (int i = tid; i < VQ_TILE * (VQ_KC / 4); i += 256) {
        const int r = i / (VQ_KC / 4), c4 = (i % (VQ_KC / 4)) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (k0 + r < K) {
          if (c0 + c4 + 3 < Cd) {
            v = *reinterpret_cast<const f32x4*>(dict + (size_t)(k0 + r) * Cd + c0 + c4);
          } else {
            for (int j = 0; j < 4; ++j)
              if (c0 + c4 + j < Cd) v[j] = dict[(size_t)(k0 + r) * Cd + c0 + c4 + j];
          }
        }
        *reinterpret_cast<f32x4*>(&ds[r][c4]) = v;
      }
      __syncthreads();
#pragma unroll 2
      for (int c = 0; c < VQ_KC; c += 4) {
        const float x0 = xs[c][pos], x1 = xs[c + 1][pos], x2 = xs[c + 2][pos], x3 = xs[c + 3][pos];
        xn = fmaf(x0, x0, xn);
        xn = fmaf(x1, x1, xn);
        xn = fmaf(x2, x2, xn);
        xn = fmaf(x3, x3, xn);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const f32x4 e = *reinterpret_cast<const f32x4*>(&ds[cg * 16 + j][c]);
          acc[j] = fmaf(x0, e[0], acc[j]);
          acc[j] = fmaf(x1, e[1], acc[j]);
          acc[j] = fmaf(x2, e[2], acc[j]);
          acc[j] = fmaf(x3, e[3], acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int code = k0 + cg * 16 + j;
      if (code < K) {
        const float d = (-2.0f * acc[j] + en[code]) + xn;
        if (d < best) {
          best = d;
          best_i = code;
        }
      }
    }
  }
  bd[cg][pos] = best;
  bi[cg][pos] = best_i;
  __syncthreads();
  int i = 0;
  if (tid < VQ_POS) {
    float d = bd[0][tid];
    i = bi[0][tid];
    for (int g = 1; g < 8; ++g) {
      const float dg = bd[g][tid];
      const int ig = bi[g][tid];
      if (dg < d || (dg == d && ig < i)) {
        d = dg;
        i = ig;
      }
    }
  }
  return i;
}

__global__ __launch_bounds__(256) void vq_argmin_kernel(const float* z, const float* dict, const float* en, int64_t* idx_out, int Cd,
                                                        int T1, int K) {
  __shared__ __attribute__((aligned(16))) float xs[VQ_KC][VQ_POS];
  __shared__ __attribute__((aligned(16))) float ds[VQ_TILE][VQ_DS];
  __shared__ float bd[8][VQ_POS];
  __shared__ int bi[8][VQ_POS];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, t0 = blockIdx.x * VQ_POS;
  const int i = vq_search(z + (size_t)b * Cd * T1, dict, en, Cd, T1, K, t0, xs, ds, bd, bi);
  if (tid < VQ_POS && t0 + tid < T1) idx_out[(size_t)b * T1 + t0 + tid] = i;
}

// ---------------------------------------------------------------------------------
// Quantise and score: the search above, then -- in the same workgroup, on the same 32 positions -- the winners' rows written
// out in NCT, the tile's sum of (z - e)^2 and the tile's code counts.
//   * The winners' rows are staged through LDS (the search's dictionary tile, now free) with the row-contiguous 16-byte loads
//     of the search, and leave along time: 32 lanes write 128 contiguous bytes of one channel.
//   * z is read again from global memory.  The workgroup has just read these Cd x 32 floats K / 128 times in the search, so
//     they are L2 lines of its own XCD, not HBM traffic; keeping them in LDS instead would cost Cd x 128 bytes per workgroup
//     (64 KB at Cd = 512: one workgroup per CU instead of three; 128 KB at Cd = 1024: with the 35 KB dictionary tile, past the
//     160 KB of a CU) and bound Cd by the LDS size.
//   * Thread (pos, cg) owns channels cg * 8 .. cg * 8 + 7 of every 64-channel chunk: differences and squares in fp32 (the square
//     rounded before it meets the sum), one fp64 accumulator in channel order, then the fixed tree of ddpm_sqerr_partial_kernel
//     (xor-shuffles inside each wave, the four waves in order).  Nothing depends on B or on the clip's row.
//   * Counts: lane p < 32 adds the number of the tile's positions that chose its code, if it is the first of them, with one
//     64-bit integer atomic -- integer sums are order-free, so the histogram is exact and reproducible.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vq_quantize_kernel(const float* z, const float* dict, const float* en, int64_t* idx_out,
                                                          float* emb_out, double* partial, int64_t* hist, int Cd, int T1, int K,
                                                          int ntile) {
  __shared__ __attribute__((aligned(16))) float xs[VQ_KC][VQ_POS];
  __shared__ __attribute__((aligned(16))) float ds[VQ_TILE][VQ_DS];
  __shared__ float bd[8][VQ_POS];
  __shared__ int bi[8][VQ_POS];
  __shared__ int win[VQ_POS];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int pos = tid & 31, cg = tid >> 5;
  const int b = blockIdx.y, t0 = blockIdx.x * VQ_POS;
  const float* zb = z + (size_t)b * Cd * T1;
  const int w = vq_search(zb, dict, en, Cd, T1, K, t0, xs, ds, bd, bi);
  if (tid < VQ_POS) {
    const bool live = t0 + tid < T1;
    win[tid] = live ? w : -1;
    if (live) idx_out[(size_t)b * T1 + t0 + tid] = w;
  }
  __syncthreads();
  if (hist && tid < VQ_POS && win[tid] >= 0) {
    int count = 0;
    bool first = true;
    for (int p = 0; p < VQ_POS; ++p) {
      if (win[p] == win[tid]) {
        ++count;
        if (p < tid) first = false;
      }
    }
    if (first) atomicAdd(reinterpret_cast<unsigned long long*>(hist) + win[tid], (unsigned long long)count);
  }
  if (!emb_out && !partial) return;
  const bool live = t0 + pos < T1;
  double s = 0.0;
  for (int c0 = 0; c0 < Cd; c0 += VQ_KC) {
    __syncthreads();
    for (int i = tid; i < VQ_POS * (VQ_KC / 4); i += 256) {
      const int r = i / (VQ_KC / 4), c4 = (i % (VQ_KC / 4)) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (win[r] >= 0 && c0 + c4 + 3 < Cd) v = *reinterpret_cast<const f32x4*>(dict + (size_t)win[r] * Cd + c0 + c4);
      *reinterpret_cast<f32x4*>(&ds[r][c4]) = v;
    }
    __syncthreads();
    if (live) {
      const f32x4 e0 = *reinterpret_cast<const f32x4*>(&ds[pos][cg * 8]);
      const f32x4 e1 = *reinterpret_cast<const f32x4*>(&ds[pos][cg * 8 + 4]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + cg * 8 + j;
        if (c < Cd) {
          const float e = j < 4 ? e0[j] : e1[j - 4];
          const size_t at = (size_t)c * T1 + t0 + pos;
          if (emb_out) emb_out[(size_t)b * Cd * T1 + at] = e;
          if (partial) {
            const float d = zb[at] - e;
            const float d2 = __fmul_rn(d, d);  // (rounded to fp32 before it meets the fp64 sum: never contracted)
            s += (double)d2;
          }
        }
      }
    }
  }
  if (!partial) return;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) partial[(size_t)b * ntile + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// sqerr[b] = sum of the clip's tile partials in tile order: one thread -- one writer -- per clip
__global__ __launch_bounds__(64) void vq_sqerr_finish_kernel(const double* partial, double* sqerr, int B, int ntile) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int i = 0; i < ntile; ++i) s += partial[(size_t)b * ntile + i];
  sqerr[b] = s;
}

__global__ __launch_bounds__(256) void vq_embed_kernel(const int64_t* idx, const float* dict, float* out, int Cd, int T1, int K) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T1) return;
  long long k = idx[(size_t)b * T1 + t];
  k = k < 0 ? 0 : (k >= K ? K - 1 : k);
  out[((size_t)b * Cd + c) * T1 + t] = dict[(size_t)k * Cd + c];
}

}  // namespace

int run_randn(float* out, int B, int T, uint64_t seed, uint64_t clip_offset, uint32_t stream_id, hipStream_t st) {
  dim3 grid(((T + 3) / 4 + 255) / 256, B);
  hipLaunchKernelGGL(randn_kernel, grid, dim3(256), 0, st, out, T, seed, clip_offset, stream_id);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int ddpm_scratch_doubles(int B, int T) { return B * sum_chunks(T); }

// The partials of a packed CONSTRAIN step: N * nchunk doubles, N on the device.  The host leases the most a pack of this geometry can
// need: N <= 65535 and N * H + R * V < 2^31.
size_t packed_scratch_doubles(int W, int H) {
  const int64_t most = std::min<int64_t>(65535, (((int64_t)1 << 31) - 1) / H);
  return (size_t)most * sum_chunks(W);
}

namespace {

// One rule on one layout: the x0 sums when CONSTRAIN asks for them (a.partial: the scratch_doubles of the layout), then the step
template <typename Rule>
int launch_step(StepArgs a, const StepLayout& l, hipStream_t st) {
  using Sum = typename Rule::Sum;
  const bool constrain = a.flags & STEP_CONSTRAIN;
  const dim3 wg(256);
  a.nchunk = sum_chunks(l.W);
  switch (l.kind) {
    case StepLayout::CLIPS: {
      const int B = l.n, T = l.W;
      if (constrain) hipLaunchKernelGGL(x0sum_kernel<Sum>, dim3(a.nchunk, B), wg, 0, st, a.x, a.eps, a.grad, a.a_t, a.partial, T, a.nchunk, T, 1);
      uintptr_t bits = 0;
      for (const float* p : {a.x, a.eps, a.grad, a.x0_prev, (const float*)a.x_to, (const float*)a.x0_out}) bits |= reinterpret_cast<uintptr_t>(p);
      const bool aligned = T % 4 == 0 && bits % 16 == 0;
      hipLaunchKernelGGL(step_clips_kernel<Rule>, dim3(((T + 3) / 4 + 255) / 256, B), wg, 0, st, a, T, aligned);
      break;
    }
    case StepLayout::WINDOWS: {
      if (constrain) hipLaunchKernelGGL(x0sum_kernel<Sum>, dim3(a.nchunk, l.n), wg, 0, st, a.x, a.eps, a.grad, a.a_t, a.partial, l.W, a.nchunk, l.H, 0);
      const int quads = ((l.n - 1) * l.H + l.W) / 4;
      hipLaunchKernelGGL(step_windows_kernel<Rule>, dim3((quads + 255) / 256), wg, 0, st, a, l.n, l.W, l.H);
      break;
    }
    case StepLayout::PACK:
      if (constrain) hipLaunchKernelGGL(x0sum_packed_kernel<Sum>, dim3(PACK_GRID), wg, 0, st, a.x, a.eps, a.grad, a.a_t, a.partial, l.first, l.n, l.W, l.H,
                                    a.nchunk);
      hipLaunchKernelGGL(step_packed_kernel<Rule>, dim3(PACK_GRID), wg, 0, st, a, l.first, l.n, l.W, l.H);
      break;
  }
  VQVS_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int run_step(StepRule rule, const StepArgs& a, const StepLayout& l, hipStream_t st) {
  const bool guided = a.grad != nullptr;
  switch (rule) {
    case StepRule::DDPM: return launch_step<DdpmRule>(a, l, st);
    case StepRule::DDIM: return guided ? launch_step<DdimRule<true>>(a, l, st) : launch_step<DdimRule<false>>(a, l, st);
    case StepRule::DPMPP: return guided ? launch_step<DpmppRule<true>>(a, l, st) : launch_step<DpmppRule<false>>(a, l, st);
  }
  VQVS_FAIL(VQVS_ERR_ARG, "unknown step rule %d", (int)rule);
}

// 16-byte accesses need every array to start on a 16-byte boundary (the mask, read 4 bytes at a time, on a 4-byte one)
static bool keep_aligned(const float* x, const float* win, const float* x0, const uint8_t* keep, const float* noise) {
  const uintptr_t floats = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(win) | reinterpret_cast<uintptr_t>(x0) |
                           reinterpret_cast<uintptr_t>(noise);
  return floats % 16 == 0 && reinterpret_cast<uintptr_t>(keep) % 4 == 0;
}

int run_keep_region(float* x, const float* x0, const uint8_t* keep, const float* noise, const float* alpha, int B, int T, float noise_scale,
                    uint64_t seed, uint64_t clip_offset, uint32_t index, hipStream_t st) {
  const bool aligned = T % 4 == 0 && keep_aligned(x, nullptr, x0, keep, noise);
  dim3 grid(((T + 3) / 4 + 255) / 256, B);
  hipLaunchKernelGGL(keep_region_kernel, grid, dim3(256), 0, st, x, x0, keep, noise, alpha, T, aligned, noise_scale, seed, clip_offset, index);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int run_keep_region_windows(float* x, float* windows, const float* x0, const uint8_t* keep, const float* noise, const float* alpha, int n,
                            int W, int H, float noise_scale, uint64_t seed, uint64_t clip, uint32_t index, hipStream_t st) {
  const bool aligned = keep_aligned(x, windows, x0, keep, noise);
  const int quads = ((n - 1) * H + W) / 4;
  hipLaunchKernelGGL(keep_region_windows_kernel, dim3((quads + 255) / 256), dim3(256), 0, st, x, windows, x0, keep, noise, alpha, n, W, H,
                     aligned, noise_scale, seed, clip, index);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int run_keep_region_packed(float* x, float* windows, const float* x0, const uint8_t* keep, const float* noise, const float* alpha,
                           const int* first, int R, int W, int H, float noise_scale, uint64_t seed, uint64_t clip, uint32_t index,
                           hipStream_t st) {
  const bool aligned = keep_aligned(x, windows, x0, keep, noise);  // (every row starts a multiple of 4 samples into the pack)
  hipLaunchKernelGGL(keep_region_packed_kernel, dim3(PACK_GRID), dim3(256), 0, st, x, windows, x0, keep, noise, alpha, first, R, W, H, aligned,
                     noise_scale, seed, clip, index);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int run_ddpm_mean(const float* x_t, const float* eps, const float* a_t, const float* a_prev, float* out, int B, int T, hipStream_t st) {
  hipLaunchKernelGGL(ddpm_mean_kernel, dim3((T + 255) / 256, B), dim3(256), 0, st, x_t, eps, a_t, a_prev, out, T);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int run_ddpm_guided_eps(const float* x_t, const float* mean, const float* grad, const float* a_t, const float* a_prev, float* out,
                        int B, int T, uint32_t flags, hipStream_t st) {
  hipLaunchKernelGGL(ddpm_guided_eps_kernel, dim3((T + 255) / 256, B), dim3(256), 0, st, x_t, mean, grad, a_t, a_prev, out, T, flags);
  VQVS_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------
// Guidance mix (include/vqvs.h "Guidance mix"): eps = base + s1 (base - o1) [+ s2 (base - o2)] over the REPS blocks of one predictor
// output, `total` floats each.  The tensor expressions it replaces round every subtraction, product and sum on its own, left to right,
// so contraction is off here and the result is theirs bit for bit.  Each element is read REPS times and written once by the thread
// that read it, which is what lets eps lie over block 0.
// ---------------------------------------------------------------------------------
namespace {

template <int REPS>
__device__ __forceinline__ float guidance_mix_one(float base, float o1, float o2, float s1, float s2) {
#pragma clang fp contract(off)
  float p = base;
  if (REPS >= 2) {
    const float d = base - o1;
    const float m = s1 * d;
    p = p + m;
  }
  if (REPS >= 3) {
    const float d = base - o2;
    const float m = s2 * d;
    p = p + m;
  }
  return p;
}

// VEC: every block and eps start on 16 bytes (the launcher checks): quads [0, total / 4) as 16-byte accesses, grid-stride, and the
// total % 4 trailing floats -- REPS == 1 only, else total % 4 == 0 -- by the first threads of the grid.  Otherwise one float per thread.
template <int REPS, bool VEC>
__global__ __launch_bounds__(256) void guidance_mix_kernel(const float* outs, float* eps, int64_t total, float s1, float s2) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const float* b1 = outs + (REPS >= 2 ? total : 0);
  const float* b2 = outs + (REPS >= 3 ? 2 * total : 0);
  if (VEC) {
    const int64_t quads = total / 4;
    for (int64_t q = tid; q < quads; q += stride) {
      const f32x4 base = *reinterpret_cast<const f32x4*>(outs + q * 4);
      f32x4 o1 = base, o2 = base;
      if (REPS >= 2) o1 = *reinterpret_cast<const f32x4*>(b1 + q * 4);
      if (REPS >= 3) o2 = *reinterpret_cast<const f32x4*>(b2 + q * 4);
      f32x4 r;
      for (int j = 0; j < 4; ++j) r[j] = guidance_mix_one<REPS>(base[j], o1[j], o2[j], s1, s2);
      *reinterpret_cast<f32x4*>(eps + q * 4) = r;
    }
    const int64_t i = quads * 4 + tid;
    if (i < total) eps[i] = guidance_mix_one<REPS>(outs[i], b1[i], b2[i], s1, s2);
  } else {
    for (int64_t i = tid; i < total; i += stride) eps[i] = guidance_mix_one<REPS>(outs[i], b1[i], b2[i], s1, s2);
  }
}

template <int REPS>
void launch_guidance_mix(const float* outs, float* eps, int64_t total, float s1, float s2, hipStream_t st) {
  const bool blocks_aligned = REPS == 1 || total % 4 == 0;
  const bool vec = blocks_aligned && (reinterpret_cast<uintptr_t>(outs) | reinterpret_cast<uintptr_t>(eps)) % 16 == 0;
  const int64_t items = vec ? (total + 3) / 4 : total;  // (covers the tail: total % 4 < 4 <= the grid's threads)
  const int grid = (int)std::min<int64_t>((items + 255) / 256, 2048);
  if (vec)
    hipLaunchKernelGGL((guidance_mix_kernel<REPS, true>), dim3(grid), dim3(256), 0, st, outs, eps, total, s1, s2);
  else
    hipLaunchKernelGGL((guidance_mix_kernel<REPS, false>), dim3(grid), dim3(256), 0, st, outs, eps, total, s1, s2);
}

}  // namespace

int run_guidance_mix(const float* outs, float* eps, int64_t total, int reps, float s1, float s2, hipStream_t st) {
  if (reps == 1)
    launch_guidance_mix<1>(outs, eps, total, s1, s2, st);
  else if (reps == 2)
    launch_guidance_mix<2>(outs, eps, total, s1, s2, st);
  else
    launch_guidance_mix<3>(outs, eps, total, s1, s2, st);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int run_vq_argmin(const float* z, const float* dict, float* en_scratch, int64_t* idx, int B, int Cd, int T1, int K, hipStream_t st) {
  hipLaunchKernelGGL(vq_norms_kernel, dim3((K + 255) / 256), dim3(256), 0, st, dict, en_scratch, K, Cd);
  hipLaunchKernelGGL(vq_argmin_kernel, dim3((T1 + VQ_POS - 1) / VQ_POS, B), dim3(256), 0, st, z, dict, en_scratch, idx, Cd, T1, K);
  VQVS_HIP(hipGetLastError());
  return 0;
}

size_t vq_quantize_scratch_bytes(int B, int T1, int K) { return ((size_t)B * ((T1 + VQ_POS - 1) / VQ_POS)) * 8 + (size_t)K * 4; }

// scratch: [B * ntile] fp64 tile partials, then [K] fp32 code norms
int run_vq_quantize(const float* z, const float* dict, void* scratch, int64_t* idx, float* embedded, double* sqerr, int64_t* hist, int B,
                    int Cd, int T1, int K, hipStream_t st) {
  const int ntile = (T1 + VQ_POS - 1) / VQ_POS;
  double* partial = reinterpret_cast<double*>(scratch);
  float* en = reinterpret_cast<float*>(partial + (size_t)B * ntile);
  hipLaunchKernelGGL(vq_norms_kernel, dim3((K + 255) / 256), dim3(256), 0, st, dict, en, K, Cd);
  hipLaunchKernelGGL(vq_quantize_kernel, dim3(ntile, B), dim3(256), 0, st, z, dict, en, idx, embedded, sqerr ? partial : nullptr, hist,
                     Cd, T1, K, ntile);
  if (sqerr) hipLaunchKernelGGL(vq_sqerr_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, st, partial, sqerr, B, ntile);
  VQVS_HIP(hipGetLastError());
  return 0;
}

int run_vq_embed(const int64_t* idx, const float* dict, float* out, int B, int Cd, int T1, int K, hipStream_t st) {
  hipLaunchKernelGGL(vq_embed_kernel, dim3((T1 + 255) / 256, Cd, B), dim3(256), 0, st, idx, dict, out, Cd, T1, K);
  VQVS_HIP(hipGetLastError());
  return 0;
}

}  // namespace vqvs
