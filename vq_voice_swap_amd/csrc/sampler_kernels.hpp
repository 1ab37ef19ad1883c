// Host launchers of the model-independent kernels (DDPM step, RNG, VQ).
#pragma once
#include "common.hpp"

namespace vqvs {
int run_randn(float* out, int B, int T, uint64_t seed, uint64_t clip_offset, uint32_t stream_id, hipStream_t st);
int ddpm_scratch_doubles(int B, int T);
int run_ddpm_step(const float* x_t, const float* eps, const float* noise, const float* a_t, const float* a_prev, float* out,
                  double* scratch, int B, int T, uint32_t flags, float noise_scale, uint64_t seed, uint64_t clip_offset,
                  uint32_t step_index, hipStream_t st);
// the step of one long signal [(n - 1) * H + W] from the predictions of its n overlapping windows [n, W]; scratch as run_ddpm_step(n, W)
int run_ddpm_step_windows(const float* x, const float* eps, const float* noise, const float* a_t, const float* a_prev, float* x_prev,
                          float* windows, double* scratch, int n, int W, int H, uint32_t flags, float noise_scale, uint64_t seed,
                          uint64_t clip, uint32_t step_index, hipStream_t st);
// DDIM step from alpha_bar a_t to a_to, single clips and the windows of one long signal; grad NULL: unguided; scratch as the DDPM steps'
int run_ddim_step(const float* x_t, const float* eps, const float* grad, const float* noise, const float* a_t, const float* a_to, float* out,
                  double* scratch, int B, int T, uint32_t flags, float eta, float noise_scale, uint64_t seed, uint64_t clip_offset,
                  uint32_t step_index, hipStream_t st);
int run_ddim_step_windows(const float* x, const float* eps, const float* grad, const float* noise, const float* a_t, const float* a_to,
                          float* x_to, float* windows, double* scratch, int n, int W, int H, uint32_t flags, float eta, float noise_scale,
                          uint64_t seed, uint64_t clip, uint32_t step_index, hipStream_t st);
// DPM-Solver++(2M) step from alpha_bar a_t to a_to with the previous step's x0 and alpha_bar (x0_prev / a_from NULL: first order),
// single clips and the windows of one long signal; x0_out NULL: not wanted; scratch as the DDPM steps'
int run_dpmpp_step(const float* x_t, const float* eps, const float* grad, const float* x0_prev, const float* a_from, const float* a_t,
                   const float* a_to, float* x_to, float* x0_out, double* scratch, int B, int T, uint32_t flags, hipStream_t st);
int run_dpmpp_step_windows(const float* x, const float* eps, const float* grad, const float* x0_prev, const float* a_from, const float* a_t,
                           const float* a_to, float* x_to, float* x0_out, float* windows, double* scratch, int n, int W, int H, uint32_t flags,
                           hipStream_t st);
// The three window steps on a PACK of R recordings in one launch: first [R + 1] (device) holds the prefix sums of the recordings' window
// counts, the long arrays hold the rows end to end, the window arrays the windows stacked; recording r is stepped as clip + r.
// scratch: packed_scratch_doubles(W, H) doubles when flags has CONSTRAIN -- the window total is on the device, so this is its bound.
size_t packed_scratch_doubles(int W, int H);
int run_ddpm_step_packed(const float* x, const float* eps, const float* noise, const float* a_t, const float* a_prev, float* x_prev,
                         float* windows, double* scratch, const int* first, int R, int W, int H, uint32_t flags, float noise_scale,
                         uint64_t seed, uint64_t clip, uint32_t step_index, hipStream_t st);
int run_ddim_step_packed(const float* x, const float* eps, const float* grad, const float* noise, const float* a_t, const float* a_to,
                         float* x_to, float* windows, double* scratch, const int* first, int R, int W, int H, uint32_t flags, float eta,
                         float noise_scale, uint64_t seed, uint64_t clip, uint32_t step_index, hipStream_t st);
int run_dpmpp_step_packed(const float* x, const float* eps, const float* grad, const float* x0_prev, const float* a_from, const float* a_t,
                          const float* a_to, float* x_to, float* x0_out, float* windows, double* scratch, const int* first, int R, int W,
                          int H, uint32_t flags, hipStream_t st);
// kept samples of x (NULL keep: all) put back on the forward process of x0 at alpha, in place: B rows of T, and one long state with
// its window copies
int run_keep_region(float* x, const float* x0, const uint8_t* keep, const float* noise, const float* alpha, int B, int T, float noise_scale,
                    uint64_t seed, uint64_t clip_offset, uint32_t index, hipStream_t st);
int run_keep_region_windows(float* x, float* windows, const float* x0, const uint8_t* keep, const float* noise, const float* alpha, int n,
                            int W, int H, float noise_scale, uint64_t seed, uint64_t clip, uint32_t index, hipStream_t st);
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
