// Host launchers of the model-independent kernels (DDPM step, RNG, VQ).
#pragma once
#include "../../include/vqvs.h"
#include "common.hpp"

namespace vqvs {
int run_randn(float* out, int B, int T, uint64_t seed, uint64_t clip_offset, uint32_t stream_id, hipStream_t st);
// A reverse step is a RULE (the sampler) run on a LAYOUT (where the state's samples lie): sampler_kernels.hip "Rules and layouts".
enum class StepRule { DDPM, DDIM, DPMPP };
// Every array and scalar that any step takes (include/vqvs.h names them); what a rule or a layout has no use for stays NULL / 0.
// The step goes from alpha_bar a_t to a_to (the DDPM step's alpha_prev), DPM-Solver++ with the step before's x0_prev and a_from
// (NULL: first order); grad NULL: unguided; noise NULL: drawn from (seed, clip, step_index); win / x0_out NULL: not wanted.
struct StepArgs {
  const float *x = nullptr, *eps = nullptr, *grad = nullptr, *noise = nullptr, *x0_prev = nullptr;
  const float *a_from = nullptr, *a_t = nullptr, *a_to = nullptr;
  float *x_to = nullptr, *x0_out = nullptr, *win = nullptr;
  double* partial = nullptr;  // the x0 sums of CONSTRAIN, nchunk per row: ddpm_scratch_doubles / packed_scratch_doubles of them (not read without the flag)
  int nchunk = 0;             // (set by run_step)
  uint32_t flags = 0;
  float eta = 0.f, noise_scale = 0.f;
  uint64_t seed = 0, clip = 0;
  uint32_t step_index = 0;
};
// CLIPS: n rows of W samples, row b with its own alphas, stepped as clip + b.  WINDOWS: one long signal [(n - 1) * H + W] under its n
// overlapping windows [n, W], one alpha.  PACK: n recordings of such windows in one launch; first [n + 1] (device) holds the prefix
// sums of their window counts, the long arrays hold the rows end to end, the window arrays the windows stacked; recording r is
// stepped as clip + r.
struct StepLayout {
  enum Kind { CLIPS, WINDOWS, PACK } kind;
  int n, W, H;
  const int* first;
};
int ddpm_scratch_doubles(int rows, int len);  // CLIPS (B, T), WINDOWS (n, W)
size_t packed_scratch_doubles(int W, int H);  // PACK: the window total is on the device, so this is its bound
int run_step(StepRule rule, const StepArgs& args, const StepLayout& layout, hipStream_t st);
// kept samples of x (NULL keep: all) put back on the forward process of x0 at alpha, in place: B rows of T, and one long state with
// its window copies
int run_keep_region(float* x, const float* x0, const uint8_t* keep, const float* noise, const float* alpha, int B, int T, float noise_scale,
                    uint64_t seed, uint64_t clip_offset, uint32_t index, hipStream_t st);
int run_keep_region_windows(float* x, float* windows, const float* x0, const uint8_t* keep, const float* noise, const float* alpha, int n,
                            int W, int H, float noise_scale, uint64_t seed, uint64_t clip, uint32_t index, hipStream_t st);
// ... and a pack of such states (first [R + 1] on the device, as in StepLayout::PACK): recording r at clip + r
int run_keep_region_packed(float* x, float* windows, const float* x0, const uint8_t* keep, const float* noise, const float* alpha,
                           const int* first, int R, int W, int H, float noise_scale, uint64_t seed, uint64_t clip, uint32_t index,
                           hipStream_t st);
int run_ddpm_mean(const float* x_t, const float* eps, const float* a_t, const float* a_prev, float* out, int B, int T, hipStream_t st);
int run_ddpm_guided_eps(const float* x_t, const float* mean, const float* grad, const float* a_t, const float* a_prev, float* out,
                        int B, int T, uint32_t flags, hipStream_t st);
// guidance mix over the `reps` (1..3) blocks of `total` floats of one predictor output: eps = base + s1 (base - o1) + s2 (base - o2),
// every operation rounded on its own; eps may be block 0
int run_guidance_mix(const float* outs, float* eps, int64_t total, int reps, float s1, float s2, hipStream_t st);
// forward process and denoising loss (loss_kernels.hip)
int sqerr_scratch_doubles(int B, int T);
int run_ddpm_noise(const float* x0, int x0_rows, const float* alpha, const float* eps, int eps_rows, const int64_t* noise_index,
                   float* x_t, int B, int T, uint64_t seed, uint64_t clip_offset, hipStream_t st);
int run_ddpm_sqerr(const float* pred, const float* eps, int eps_rows, const int64_t* noise_index, float* loss, double* scratch, int B,
                   int T, uint64_t seed, uint64_t clip_offset, hipStream_t st);
int run_vq_argmin(const float* z, const float* dict, float* en_scratch, int64_t* idx, int B, int Cd, int T1, int K, hipStream_t st);
// fused search + embedding + per-clip sum of (z - e)^2 + code counts; scratch holds vq_quantize_scratch_bytes(B, T1, K) bytes
size_t vq_quantize_scratch_bytes(int B, int T1, int K);
int run_vq_quantize(const float* z, const float* dict, void* scratch, int64_t* idx, float* embedded, double* sqerr, int64_t* hist, int B,
                    int Cd, int T1, int K, hipStream_t st);
// cross-entropy scores of logits [B, K, L] against targets [B, L] (score_kernels.hip); scratch holds xent_score_scratch_bytes(B, L) bytes
size_t xent_score_scratch_bytes(int B, int L);
int run_xent_score(const float* logits, const int64_t* targets, void* scratch, double* nll, int64_t* top1, int64_t* topk, int k,
                   int64_t* confusion, int B, int K, int L, hipStream_t st);
int run_vq_embed(const int64_t* idx, const float* dict, float* out, int B, int Cd, int T1, int K, hipStream_t st);
}  // namespace vqvs
