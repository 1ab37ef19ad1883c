/*
 * vqvs.h -- C ABI of the MI355X (gfx950) native sampler library `libvqvs_hip.so`.
 *
 * The reference (unixpickle/vq-voice-swap) is pure Python: it has no C / FFI /
 * operator boundary of its own.  Its boundary for the DDPM sampling hot path is
 * the Python object surface listed in SURVEY.md section 8(b).  Every entry point
 * below states the reference interface (file:line under the reference repo) it
 * stands behind; the Python classes in `vq_voice_swap_amd/` bind them with ctypes
 * (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - plain pointers + sizes, no torch types.  All pointers named `d_*` are
 *     DEVICE pointers on the model's device; `h_*` are HOST pointers.
 *   - tensors at the boundary use the reference's layout: float32, NCT
 *     ([batch][channels][time], time contiguous); indices are int64.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the default stream).  The caller owns all boundary buffers; the
 *     library owns only the packed weights and a scratch arena per model handle.
 *   - return value 0 = success, negative = error (vqvs_last_error() describes
 *     it, thread-local).  Nothing here falls back to a CPU path.
 *   - a handle is not thread-safe (one scratch arena); different handles are
 *     independent.  The handle-less entry points (vqvs_ddpm_step and
 *     vqvs_ddpm_step_windows with CONSTRAIN, vqvs_vq_argmin) keep one small scratch buffer per (device, stream): calls on
 *     different streams never share it and may run concurrently; calls on one
 *     stream are ordered by the stream.  One process per GPU.
 */
#ifndef VQVS_H
#define VQVS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQVS_OK 0
#define VQVS_ERR_ARG (-1)     /* bad shape / null pointer / unsupported configuration */
#define VQVS_ERR_HIP (-2)     /* a HIP runtime call failed */
#define VQVS_ERR_STATE (-3)   /* handle misuse */

/* network kinds */
#define VQVS_KIND_PREDICTOR 0 /* UNetPredictor  (reference vq_voice_swap/models/unet.py:16-184) */
#define VQVS_KIND_ENCODER 1   /* UNetEncoder    (reference unet.py:187-245) */
#define VQVS_KIND_RESBLOCK 2  /* one ResBlock   (reference unet.py:248-316); unit-test granularity */
#define VQVS_KIND_CLASSIFIER 3 /* Classifier   (reference vq_voice_swap/models/classifier.py:18-191), base_channels + num_labels;
                                  reserved[1] = output_mult (0 = 16); topology_set = 1: channel_mult / depth_mult (n_dilations = 0) */
#define VQVS_KIND_ENCPRED 4    /* EncoderPredictor (reference models/encoder_predictor.py:14-75): base_channels, out_channels =
                                  bottleneck_dim, reserved[1] = downsample_rate, reserved[2] = num_latents */

#define VQVS_KIND_MFCC_ENCODER 5 /* ConvMFCCEncoder (reference models/conv_encoder.py:14-133): base_channels, out_channels,
                                  reserved[1] = version (1: n_fft 320, 40 mels, log; 2: n_fft 400, 80 mels, dB, normalized),
                                  reserved[2] = input_ulaw.  fp32 precision only.  Its parameter table starts with the three
                                  buffers of torchaudio.transforms.MFCC that a reference checkpoint carries (mfcc.dct_mat, ...) */

#define VQVS_KIND_PREDICTOR_GRAD 6 /* UNetPredictor for speaker enrolment (reference train_vqvae_add.py, train_loop.py:438-485): the cfg
                                  fields and the parameter table of VQVS_KIND_PREDICTOR with num_labels > 0 and out_channels == 1,
                                  cond_channels 0 or not; runs vqvs_unet_embed_grad.  fp32 precision only; VQVS_ERR_ARG for a 2-byte
                                  precision, a padded width (reserved[4] != 0), num_labels == 0 or out_channels != 1.  The handle keeps
                                  every intermediate of the batch resident.  class_embed.weight is in the table but not read: the
                                  conditioning vector of every clip is an argument of the call */

/* activation storage / arithmetic */
#define VQVS_PREC_F32 0  /* fp32 activations; convs as 3-term bf16-split MFMA, fp32 accumulate (~2^-17 rel.) */
#define VQVS_PREC_BF16 1 /* bf16 activations; bf16 MFMA, fp32 accumulate */
#define VQVS_PREC_F16 2  /* fp16 (IEEE binary16) activations and weights; f16 MFMA, fp32 accumulate; GroupNorm statistics,
                            FiLM, GELU and the residual add are evaluated in fp32.  Meets the 1e-3 waveform-RMS parity
                            bar at 2-byte storage; activations must stay below 65504 in magnitude */

typedef struct vqvs_model vqvs_model;

typedef struct vqvs_cfg {
  int32_t kind;          /* VQVS_KIND_* */
  int32_t base_channels; /* multiple of 32 in 32..256 (reference configs: 32, 64; tuned: 32, 64, 128); MFCC encoder: a power of two;
                            other widths of a predictor / encoder: the padded physical width, see reserved[4] */
  int32_t in_channels;   /* 1 (the reference's default and every caller's value, unet.py:25) .. 64; predictor / encoder handles only */
  int32_t out_channels;  /* predictor: 1 or a multiple of 32; encoder: multiple of 32 */
  int32_t cond_channels; /* 0 = unconditional (unet.py:46-47) */
  int32_t num_labels;    /* 0 = no class embedding (unet.py:44-45) */
  int32_t precision;     /* VQVS_PREC_* */
  int32_t max_batch;     /* scratch arena is sized for this many clips ... */
  int32_t max_T;         /* ... of this many samples (a multiple of the UNet's downsample rate: 256 for the default topology) */
  int32_t debug_taps;    /* 1 = keep every block output resident for vqvs_debug_read_tap */
  /* VQVS_KIND_RESBLOCK only: */
  int32_t rb_cin, rb_cout, rb_resize /*0 none, 1 avg-pool/2, 2 nearest x2*/, rb_dilation, rb_emb_channels /*0 = no FiLM*/;
  int32_t reserved[5];   /* [0] dropout flag (key names), [1] / [2] per kind (above), [3] predictor: conditioning-length code (below),
                            [4] predictor / encoder: the REAL base_channels of a width that is not a multiple of 32, 0 = base_channels.
                            The reference takes any width (unet.py:17-30).  Such a model is built at the PHYSICAL width base_channels =
                            2^k * q_p, where real = 2^k * q (q odd) and q_p = the next power of two >= q, widened until the product is
                            a multiple of 32 (48 -> 64, 40 -> 64, 24 -> 32, 100 -> 128): channels come in blocks of q_p whose first q
                            are the real ones, and the caller passes every parameter in the physical shapes of vqvs_param_info with
                            entry c of a channel axis at (c / q) * q_p + c % q and zeros elsewhere (concatenated inputs and FiLM's
                            (a | b) rows are whole numbers of blocks: one rule for every axis).  GroupNorm groups and counts follow the
                            real width (unet.py:345-349); pad channels are exactly zero in every tensor.
                            vq_voice_swap_amd/unet.py pad_state does this for the Python classes. */
  /* Topology of VQVS_KIND_PREDICTOR / VQVS_KIND_ENCODER / VQVS_KIND_CLASSIFIER (reference UNetPredictor.__init__ unet.py:17-30,
   * UNetEncoder.__init__ unet.py:188-196, ClassifierStem.__init__ classifier.py:52-58).  topology_set = 0: the reference's defaults -- channel_mult (1,1,2,2,2,4,4,8,8), depth_mult 2,
   * middle_dilations (4,8,16,32) / out_dilations () -- and the fields below are ignored.  topology_set = 1: they describe the
   * network: n_levels = len(channel_mult) in 1..VQVS_MAX_LEVELS, every channel_mult[i] * base_channels a multiple of 32 and at most
   * 1024; depth_mult in 1..8; n_dilations = len(middle_dilations) (predictor) or len(out_dilations) (encoder), 0 allowed, each
   * dilation in 1..32.  T must be a multiple of 2^(n_levels - 1).
   * Limits of the builder, checked by every entry point that takes a vqvs_cfg (VQVS_ERR_ARG): predictor: channel_mult[0] == 1 (the
   * output head normalises base_channels, unet.py:113-116 -- the reference builds such a model and fails in forward); classifier:
   * the final width channel_mult[n_levels - 1] * base_channels at most 64 or a multiple of 64 (attention heads of 64 channels,
   * classifier.py:131-150); every kind: the widest per-clip tensor -- max over levels of (max_T / 2^i) rows x 2 * channel_mult[i] *
   * base_channels -- below 2 GiB at 4 bytes per element (rows of a clip are addressed by 32-bit byte offsets). */
  int32_t topology_set;
  int32_t n_levels;
  int32_t channel_mult[12];
  int32_t depth_mult;
  int32_t n_dilations;
  int32_t dilations[12];
} vqvs_cfg;
#define VQVS_MAX_LEVELS 12

/* The padded-width rule of reserved[4], for callers that lay parameters out: *q and *q_p of a REAL base_channels (q_p == q for a multiple
 * of 32: nothing is padded); the physical width is real / q * q_p.  Host arithmetic only, no device is touched.  VQVS_ERR_ARG:
 * real_base_channels < 1 or a NULL output. */
int vqvs_pad_blocks(int real_base_channels, int* q, int* q_p);

/* ---- parameters -----------------------------------------------------------
 * The library owns the topology.  It enumerates the parameters it needs under
 * the reference's own state-dict key names (checkpoint format = reference
 * vq_voice_swap/models/base.py:74-104; key list in SURVEY.md 8(b)), relative to
 * the module (e.g. "down_blocks.3.pre_cond.2.weight"), so a caller can feed it
 * from any {"kwargs","state_dict"} checkpoint. */
int vqvs_param_count(const vqvs_cfg* cfg);
int vqvs_param_info(const vqvs_cfg* cfg, int index, char* name_out, int name_cap, int64_t shape_out[4], int* ndim_out);

/* Build a model: packs `h_params[i]` (host float32, contiguous, in vqvs_param_info
 * order) into device-resident MFMA operand layout and allocates the scratch arena.
 * Replaces nn.Module construction + .to(device): reference diffusion_model.py:14-40,
 * vq_vae.py:15-32, models/base.py:83-104. */
int vqvs_model_create(const vqvs_cfg* cfg, const float* const* h_params, int n_params, int device, vqvs_model** out);
void vqvs_model_destroy(vqvs_model* m);
/* bytes of device memory held by the handle (weights + arena) */
int64_t vqvs_model_device_bytes(const vqvs_model* m);

/* ---- UNet forward -----------------------------------------------------------
 * eps = UNetPredictor.forward(x, ts, cond=, labels=)   reference unet.py:118-163
 *   d_x     [B,in_channels,T] f32      d_ts [B] f32
 *   d_cond  [B,cond_channels,T1] f32 or NULL (must match cfg, unet.py:126-131); T1 = T/256 (cfg.reserved[3] = 0: cond from a
 *           UNet encoder), (T/160 + 1 - 2)/2 + 1 = T/320 (reserved[3] = 1: cond from the MFCC encoder), or ANY length L
 *           (reserved[3] = 1000 + L: the handle then expects exactly L rows per clip, for every T); it is added to the
 *           in_conv output through nearest-neighbour up-sampling to T, as F.interpolate(cond, T) does (unet.py:138-139),
 *           with PyTorch's own source index min(floor(t * (float)L / T), L - 1)
 *   d_labels[B] int64 or NULL (must match cfg)
 *   d_out   [B,out_channels,T] f32 */
int vqvs_unet_forward(vqvs_model* m, const float* d_x, const float* d_ts, const float* d_cond,
                      const int64_t* d_labels, float* d_out, int B, int T, void* stream);

/* The same forward with an EXPLICIT conditioning vector per clip in place of class_embed[labels[b]]: the embedding is
 * emb = time_mlp(t) + v (unet.py:133-135), so any v is a voice -- a blend of rows, a vector fitted to a recording.
 * VQVS_KIND_PREDICTOR handles with num_labels > 0, every precision mode.
 *   d_vec [B,E] f32, E = 4 * base_channels OF THE HANDLE (the physical width): on a padded handle (cfg.reserved[4]) the real
 *         entries sit where class_embed.weight's columns sit (entry c at (c / q) * q_p + c % q) and the rest are zero
 *   everything else as vqvs_unet_forward
 * The schedule is vqvs_unet_forward's with one argument changed: time_embed adds d_vec[b][r] where it adds class_embed[label][r], one
 * fp32 add of the same value in the same position.  So with d_vec[b] == class_embed[labels[b]] the result equals
 * vqvs_unet_forward(..., d_labels, ...) bit for bit in every precision mode, and in fp32 the forward-only form of
 * vqvs_unet_embed_grad.
 * VQVS_ERR_ARG before the device is touched: NULL d_x, d_ts, d_vec or d_out; d_cond not matching cfg; a handle of another kind or
 * with num_labels == 0; B or T outside the handle's limits. */
int vqvs_unet_forward_vec(vqvs_model* m, const float* d_x, const float* d_ts, const float* d_cond,
                          const float* d_vec, float* d_out, int B, int T, void* stream);

/* z = UNetEncoder.forward(x)   reference unet.py:229-241
 *   d_x [B,in_channels,T] f32 -> d_z [B,out_channels,T/downsample_rate] f32 (NCT) */
int vqvs_encoder_forward(vqvs_model* m, const float* d_x, float* d_z, int B, int T, void* stream);

/* z = ConvMFCCEncoder.forward(x)   reference models/conv_encoder.py:90-110 (VQVS_KIND_MFCC_ENCODER handles):
 * mu-law expansion, MFCC (13 coefficients at 100 frames/s) with first and second order deltas, convolution stack.
 *   d_x [B,1,T] f32 -> d_z [B,out_channels,(T/160 + 1 - 2)/2 + 1] f32 (NCT): 200 positions for 4 s at 16 kHz.
 * The dB variant (version 2) floors the log-mel spectrogram at (maximum over the WHOLE batch) - 80, as
 * torchaudio.functional.amplitude_to_DB does for a 3-D input: its results depend on the batch composition. */
int vqvs_mfcc_encoder_forward(vqvs_model* m, const float* d_x, float* d_z, int B, int T, void* stream);

/* Testing entry for the same handles: the front end's log-mel rows are INJECTED (d_logmel [B][T/160 + 1][n_mels] f32, version-1
 * / log_mels front end only) and everything behind them runs as above: DCT to 13 coefficients, `deltas` twice, concatenation
 * and the convolution stack -- the part of conv_encoder.py:96-110 that is the reference's own code.  With logmel = dct_mat . c the
 * encoder sees the MFCC tensor c (dct_mat has orthonormal columns), which is how tests/test_conv_mfcc.py holds this path to
 * fixture F12 (made from the reference with torchaudio.transforms.MFCC stubbed out). */
int vqvs_mfcc_encoder_forward_logmel(vqvs_model* m, const float* d_logmel, float* d_z, int B, int T, void* stream);

/* y = ResBlock.forward(x, emb)   reference unet.py:307-316 (VQVS_KIND_RESBLOCK handles)
 *   d_x [B,rb_cin,L] f32, d_emb [B,rb_emb_channels] f32 or NULL -> d_y [B,rb_cout,L'] f32 */
int vqvs_resblock_forward(vqvs_model* m, const float* d_x, const float* d_emb, float* d_y, int B, int L, void* stream);

/* Range guard: the device status word of a handle, read and cleared (synchronises the device).  Bit 0: a GroupNorm partial sum
 * was not finite -- an activation overflowed the storage type (fp16: 65504) or the input held NaN; bit 1 (VQVS_PREC_F16 only):
 * a 256-row tile's sum of squares reached 9e8, i.e. an activation may have passed 3e4 -- or the tile's RMS ~1.9e3, which fp16
 * still holds: advisory.  The reference (fp32 throughout, unet.py:337-349) has no such limit, so a caller that sees bit 0 must
 * re-run in VQVS_PREC_F32.  Only tensors that feed a GroupNorm are observed.  The call waits for the whole device
 * (hipDeviceSynchronize), whatever stream the forwards ran on. */
int vqvs_model_status(vqvs_model* m, unsigned* h_status);

/* ---- classifier guidance (BASELINE config 5) -------------------------------------
 * logits = Classifier.forward(x, ts)   reference models/classifier.py:31-36 (stem :111-121, attention pool
 * :153-191).  VQVS_KIND_CLASSIFIER handles; parameters are named relative to the Classifier module
 * ("stem.blocks.3.pre_cond.2.weight", "out.1.weight", ...).  T must be a multiple of 512.
 *   d_x [B,1,T] f32, d_ts [B] f32 -> d_logits [B,num_labels] f32 */
int vqvs_classifier_forward(vqvs_model* m, const float* d_x, const float* d_ts, float* d_logits, int B, int T, void* stream);
/* grad = scale * d/dx log_softmax(Classifier(x, ts))[labels]   -- what the reference's cond_fn obtains with
 * torch.autograd.grad (sample_diffusion.py:34-42).  Runs the forward pass, then an explicit input-gradient
 * schedule (transposed convolutions on the MFMA kernel, GroupNorm / GELU / attention-pool backward).
 *   d_labels [B] int64, d_grad [B,1,T] f32 out, d_logits [B,num_labels] f32 out or NULL */
int vqvs_classifier_guidance(vqvs_model* m, const float* d_x, const float* d_ts, const int64_t* d_labels, float scale,
                             float* d_grad, float* d_logits, int B, int T, void* stream);
/* feat = Classifier.stem(x, ts), the vector reference stat_generate.py:36-38 collects: the attention pool's c_proj output at
 * the query token (models/classifier.py:111-121, 153-158), before the head's GELU and Linear.  Forward schedule only (never
 * the backward phase); all three precision modes.  F = output_mult * base_channels.
 *   d_x [B,1,T] f32, d_ts [B] f32 -> d_feat [B,F] f32, d_logits [B,num_labels] f32 or NULL,
 *   d_probs [B,num_labels] f32 (softmax of the logits, stat_generate.py:39) or NULL */
int vqvs_classifier_features(vqvs_model* m, const float* d_x, const float* d_ts, float* d_feat,
                             float* d_logits, float* d_probs, int B, int T, void* stream);

/* ---- feature statistics (reference stat_generate.py:44-45: np.mean / np.cov over every clip's features) ---------------
 * Streaming moments about a shift K (handle-less):
 *   d_s1[F] += sum_b (f_b - K);  d_s2[F*F] += sum_b (f_b - K)(f_b - K)^T   (double accumulators, full symmetric matrix)
 *   d_feat [B,F] f32, d_shift [F] f32, d_s1 [F] f64 in/out, d_s2 [F,F] f64 in/out; B >= 1, F in 1..8192.
 * f64 throughout (differences formed in f64 from the f32 inputs, f64 MFMA products and sums).  Deterministic: every output
 * element is owned by one workgroup that walks b in a fixed order (no atomics), so the same sequence of calls gives
 * bitwise-identical accumulators.  Null pointers and bad sizes return VQVS_ERR_ARG before touching the device. */
int vqvs_feature_moments(const float* d_feat, int B, int F, const float* d_shift, double* d_s1, double* d_s2, void* stream);

/* ---- encoder-predictor guidance ---------------------------------------------------
 * logits = EncoderPredictor.forward(x, ts)   reference models/encoder_predictor.py:43-58: UNetPredictor with a
 * bottleneck output, nearest down-sampling by `downsample_rate`, 1x1 convolution to num_latents logits.
 * VQVS_KIND_ENCPRED handles; parameters are named relative to the module ("unet.in_conv.weight", "out.weight").
 *   d_x [B,1,T] f32, d_ts [B] f32 -> d_logits [B,num_latents,T/rate] f32 */
int vqvs_encpred_forward(vqvs_model* m, const float* d_x, const float* d_ts, float* d_logits, int B, int T, void* stream);
/* grad = -scale * d/dx sum_{b,i} cross_entropy(logits[b,:,i], targets[b,i]) -- the cond_fn of VQVAE.decode(enc_pred=...)
 * (reference vq_vae.py:125-130, encoder_predictor.py:60-64), computed by an explicit backward schedule through the
 * whole UNet (concatenating, up- and down-sampling blocks).
 *   d_targets [B,T/rate] int64, d_grad [B,1,T] f32 out, d_logits [B,num_latents,T/rate] f32 out or NULL */
int vqvs_encpred_guidance(vqvs_model* m, const float* d_x, const float* d_ts, const int64_t* d_targets, float scale,
                          float* d_grad, float* d_logits, int B, int T, void* stream);

/* ---- speaker enrolment ----------------------------------------------------------------
 * The gradient of every clip's noise-prediction MSE with respect to its conditioning vector: what the reference obtains with
 * loss.backward() when only predictor.label_parameters() -- the class_embed table -- is trained (train_loop.py:438-485, 76;
 * unet.py:133-135, 307-316).  VQVS_KIND_PREDICTOR_GRAD handles.  With emb_b = time_mlp(ts_b) + vec_b in place of
 * class_embed[label_b], the call runs the predictor's forward schedule and then an explicit backward schedule that reaches only the
 * FiLM coefficients of every ResBlock:
 *   pred = UNetPredictor(x_t, ts, cond) under emb: bit for bit vqvs_unet_forward of an fp32 VQVS_KIND_PREDICTOR handle whose
 *          class_embed rows are the vectors
 *   mse[b]  = mean_t (eps[b,t] - pred[b,t])^2, summed exactly as vqvs_ddpm_sqerr sums it
 *   grad[b] = d mse[b] / d vec_b = gelu'(emb_b) * Wall^T (d a | d b of every block), d a_c = sum_l du2[c,l] h^[c,l], d b_c = sum_l du2[c,l]
 * The batch mean and the sum over the clips that share a row are vqvs_embed_adamw's.  Deterministic: every reduction has a fixed
 * order and one writer per output, no atomics; the same call gives the same bits.
 *   d_x_t [B,in_channels,T] f32, d_ts [B] f32, d_cond as for vqvs_unet_forward (NULL iff cond_channels == 0)
 *   d_vec [B,E] f32, E = 4 * base_channels;  d_eps [B,1,T] f32
 *   d_mse [B] f32 out, d_grad [B,E] f32 out;  d_pred [B,1,T] f32 out or NULL
 *   d_mse == NULL and d_grad == NULL: the forward schedule alone (d_pred is then required and d_eps is not read)
 * VQVS_ERR_ARG before the device is touched: a NULL required pointer, d_cond not matching the cfg, exactly one of d_mse / d_grad
 * NULL, B or T outside the handle's limits. */
int vqvs_unet_embed_grad(vqvs_model* m, const float* d_x_t, const float* d_ts, const float* d_cond, const float* d_vec,
                         const float* d_eps, float* d_mse, float* d_grad, float* d_pred, int B, int T, void* stream);
/* One AdamW step on n embedding rows from per-clip gradients (handle-less; torch.optim.AdamW's update, decoupled weight decay and
 * bias correction; `step` is the 1-based count of this step).  One kernel, one thread per (row, e):
 *   g = (sum of d_grad[b, e] over the clips with d_row_of_clip[b] == row, in clip order) / B      -- losses.mean(), train_loop.py:76
 *   p *= 1 - lr * weight_decay;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * evaluated in fp64 from the fp32 state and rounded once per stored value.  A row that no clip names has g = 0: with weight_decay 0
 * and zero moments it is bitwise unchanged.  A clip whose index is outside 0..n-1 contributes to no row (the Python binding raises
 * IndexError first).
 *   d_rows, d_m, d_v [n,E] f32 in/out;  d_grad [B,E] f32;  d_row_of_clip [B] int64
 * VQVS_ERR_ARG before the device is touched: a NULL pointer; n, B or E not positive; step < 1; lr, eps or weight_decay negative or
 * not finite; a beta outside [0, 1). */
int vqvs_embed_adamw(float* d_rows, float* d_m, float* d_v, const float* d_grad, const int64_t* d_row_of_clip, int n, int B, int E,
                     int step, float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ---- classifier enrolment (handle-less) -------------------------------------------------
 * New speakers of a trained Classifier are new rows of its head, GELU -> Linear(F, num_labels) on the stem's feature vector
 * (vqvs_classifier_features, F = output_mult * base_channels).  With the stem and the K old rows frozen, the gradient of the loss
 * the reference trains the classifier on (train_loop.py:551-561: the NLL of the label) has a closed form in the n new rows,
 *   d nll_b / d W[K+j, :] = (softmax_b[K+j] - [y_b == K+j]) * gelu(feat_b),   d nll_b / d bias[K+j] = softmax_b[K+j] - [y_b == K+j],
 * so there is no backward schedule: this call gives the per-clip loss and the coefficients, vqvs_head_adamw the gradient and the step.
 *   d_feat [B,F] f32       stem features, before the head's GELU
 *   d_w_old [K,F] f32, d_b_old [K] f32   the checkpoint's head (out.1.weight, out.1.bias), read only
 *   d_new [n,F+1] f32      the new rows, column F is the bias
 *   d_targets [B] int64    labels of the grown model, 0..K+n-1; a target < K is a replay clip of an old speaker
 *   d_act [B,F] f32 out, or NULL: gelu_f(feat), the library's f32 GELU: exactly the value vqvs_classifier_forward's head forms
 *   d_logits [B,K+n] f32 out, or NULL: logit_k = bias_k + sum_f w[k,f] act[f].  Products and sums in f64 from the f32 inputs (a
 *               product of two f32 values is exact in f64: only the sums round); lane l of a wave adds f = l, l+64, ... in
 *               ascending order, the 64 lanes fold by a fixed xor tree (32, 16, ... 1), the bias is added last; rounded to f32
 *               once, on store.  Everything below is taken from the f64 logits, never from the stored ones.
 *   d_nll [B] f64 out:  logsumexp_k logit_k - logit_y.  The maximum M is exact; d_k = logit_k - M, exp, the sum S (thread t of
 *               256 adds k = t, t+256, ..., lanes fold by the xor tree, the four waves are added in order), log S and
 *               log S - d_y are f64
 *   d_top1 [B] int64 out, or NULL: 1 if the first index of the maximum of the f64 logits is y, else 0
 *   d_new_mass [B] f64 out, or NULL: sum_j softmax[K+j] = (sum of exp d_k over k >= K, in the order of S) / S: what the grown
 *               head gives to any new label; on a replay clip the number to watch
 *   d_coef [B,n] f64 out: exp(d_{K+j}) / S - [y == K+j]
 * One workgroup per clip, one writer per output, no floating-point atomics: a clip's outputs are bitwise the same whatever B and
 * its row are, and the same call gives the same bits.  A target outside 0..K+n-1 is never used as an index: that clip's d_nll and
 * its d_coef row become NaN and its d_top1 is 0 (the Python binding raises IndexError first).
 * B in 1..65535, F in 1..4096, K >= 1, n >= 1, K+n <= 8192.  Asynchronous on `stream`.  VQVS_ERR_ARG before the device is touched:
 * NULL d_feat / d_w_old / d_b_old / d_new / d_targets / d_nll / d_coef, or a size outside the limits. */
int vqvs_head_xent_grad(const float* d_feat, const float* d_w_old, const float* d_b_old, const float* d_new, const int64_t* d_targets,
                        float* d_act, float* d_logits, double* d_nll, int64_t* d_top1, double* d_new_mass, double* d_coef, int B, int F,
                        int K, int n, void* stream);
/* The gradient of the batch-mean NLL with respect to the new rows and one AdamW step on them, in one kernel, one thread per
 * (row j, column f) of [n, F+1]:
 *   g[j,f] = (sum over b ascending of d_coef[b,j] * act[b,f], fused multiply-adds in f64) / B,  act[b,F] = 1 for the bias column
 *            -- nlls.mean().backward() of train_loop.py:551-561 restricted to the new rows
 *   p *= 1 - lr * weight_decay;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * vqvs_embed_adamw's update to the letter: torch.optim.AdamW's, decoupled weight decay and bias correction, `step` the 1-based count
 * of this step, evaluated in f64 from the f32 state and rounded once per stored value.  A row whose d_coef column is all zero has
 * g = 0: with weight_decay 0 and zero moments it is bitwise unchanged.  No atomics; the same call gives the same bits.
 *   d_new, d_m, d_v [n,F+1] f32 in/out;  d_act [B,F] f32 and d_coef [B,n] f64 as vqvs_head_xent_grad wrote them
 * VQVS_ERR_ARG before the device is touched: a NULL pointer; n, B or F not positive (or above 8192, 65535, 4096, the limits of
 * vqvs_head_xent_grad); step < 1; lr, eps or weight_decay negative or not finite; a beta outside [0, 1). */
int vqvs_head_adamw(float* d_new, float* d_m, float* d_v, const float* d_act, const double* d_coef, int n, int B, int F, int step,
                    float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ---- DDPM reverse step --------------------------------------------------------
 * x_prev = Diffusion.ddpm_previous(x_t, ts, step, eps, noise, sigma_large, constrain)
 * reference diffusion/diffusion.py:48-90 (without cond_fn; with cond_fn the caller
 * uses the two half-steps below around its own cond_fn, diffusion.py:80-83).
 *   d_alpha_t, d_alpha_prev [B] f32: schedule(ts), schedule(ts-step) (schedule.py:30-41)
 *   d_noise [B,1,T] f32, or NULL to draw N(0,1) in-kernel from Philox4x32-10 keyed by
 *     (seed, clip_offset + row, step_index) -- independent of how clips are sharded;
 *     noise_scale 0 reproduces the reference's zero-noise last iteration (diffusion.py:127) */
#define VQVS_DDPM_SIGMA_LARGE 1u
#define VQVS_DDPM_CONSTRAIN 2u
int vqvs_ddpm_step(const float* d_x_t, const float* d_eps, const float* d_noise, const float* d_alpha_t,
                   const float* d_alpha_prev, float* d_x_prev, int B, int T, uint32_t flags, float noise_scale,
                   uint64_t seed, uint64_t clip_offset, uint32_t step_index, void* stream);
/* The reverse step of ONE long signal whose predictions came from overlapping windows of the trained length (handle-less; the
 * reference has no counterpart).  n windows of W samples, one every H: sample j of window b is absolute position p = b * H + j of a
 * signal of Np = (n - 1) * H + W samples, and V = W - H is the overlap.
 *   d_x [Np] f32 the long state; d_eps [n,W] f32 the predictor's output on the windows
 *   d_alpha_t, d_alpha_prev: ONE float each (all windows of a recording share t)
 *   d_noise [Np] f32, one value per absolute position, or NULL to draw philox_normal4(seed, quad = p / 4, clip, step_index, stream 0):
 *     exactly what vqvs_ddpm_step draws for ONE row of length Np at clip_offset = clip, shared by the windows that overlap
 *   d_x_prev [Np] f32 out; d_windows [n,W] f32 out or NULL: d_windows[b,j] = d_x_prev[b * H + j], the next forward's input, written
 *     in the same pass (both copies of an overlap sample are the same value)
 *   flags, noise_scale: as for vqvs_ddpm_step
 * Per sample p, with the coefficients of vqvs_ddpm_step: a window b that covers p contributes e_b = eps[b,j], with CONSTRAIN
 * re-derived as there, x0 = clamp((x[p] - sqrt(1-a_t) e_b) / sqrt(a_t) - mean_b, -1, 1), about window b's OWN mean of x0 over its W
 * samples (fp64 partials per 4096 samples added in chunk order: n * ceil(W / 4096) doubles of the per-(device, stream) scratch
 * buffer).  One window: e = e_b.  Two, left b and right b + 1: u = p - (b + 1) * H in [0, V), w = (u + 1/2) / V,
 * e = fmaf(w, e_right - e_left, e_left).  Then x_prev[p] = c1 * (x[p] - c2 * e) + sigma * noise: means are blended and the noise is
 * shared, so the step has the variance of a single clip's and the windows agree on their common samples at every step.  At n = 1 the
 * result equals vqvs_ddpm_step(B = 1, T = W, clip_offset = clip) bit for bit.
 * Limits (VQVS_ERR_ARG before the device is touched): n in 1..65535; W and H positive multiples of 4 (every access is 16 bytes wide:
 * a quad never straddles a window boundary); 0 <= V <= H, so at most two windows cover a sample; Np < 2^31; NULL d_x, d_eps,
 * d_alpha_t, d_alpha_prev or d_x_prev; d_x_prev overlapping d_x. */
int vqvs_ddpm_step_windows(const float* d_x, const float* d_eps, const float* d_noise, const float* d_alpha_t,
                           const float* d_alpha_prev, float* d_x_prev, float* d_windows, int n, int W, int H, uint32_t flags,
                           float noise_scale, uint64_t seed, uint64_t clip, uint32_t step_index, void* stream);
/* mean = eps_to_prev(eps)  and  eps' = prev_to_eps(mean + sigma^2 * grad)   (diffusion.py:69-83) */
int vqvs_ddpm_mean(const float* d_x_t, const float* d_eps, const float* d_alpha_t, const float* d_alpha_prev,
                   float* d_mean, int B, int T, void* stream);
int vqvs_ddpm_guided_eps(const float* d_x_t, const float* d_mean, const float* d_grad, const float* d_alpha_t,
                         const float* d_alpha_prev, float* d_eps_out, int B, int T, uint32_t flags, void* stream);
/* ---- Guidance mix (handle-less): the extrapolation of classifier-free-style guidance (reference vq_vae.py:205-214) in one pass ----
 * d_outs [reps * rows, row_len] f32, contiguous: the predictor's output on the reps-fold batch.  Block k is rows k * rows ..
 * (k + 1) * rows - 1; block 0 is the fully conditioned prediction `base`, blocks 1 and 2 (o1, o2) the predictions with something
 * dropped.  d_eps [rows, row_len] f32 out:
 *   reps == 1: eps = base
 *   reps == 2: eps = base + s1 * (base - o1)
 *   reps == 3: eps = (base + s1 * (base - o1)) + s2 * (base - o2)
 * Every subtraction, product and sum is an fp32 operation rounded on its own, in the order written (contraction off): the result is,
 * bit for bit, what the tensor expressions `pred = base; pred = pred + s * (base - o_k)` give, whatever the batch the elements came in.
 * reps reads and one write per element, 16 bytes wide when d_outs and d_eps are 16-byte aligned and -- for reps > 1 -- rows * row_len
 * is a multiple of 4 (blocks 1 and 2 start rows * row_len floats in); one float per access otherwise.  Elements are indexed in 64 bits.
 * d_eps == d_outs is allowed (in place over block 0).
 * VQVS_ERR_ARG before the device is touched: NULL d_outs or d_eps; rows < 1; row_len < 1; reps outside 1..3; d_eps overlapping
 * d_outs in any other way (blocks 1 or 2, or block 0 at an offset). */
int vqvs_guidance_mix(const float* d_outs, float* d_eps, int rows, int64_t row_len, int reps, float s1, float s2, void* stream);
/* ---- Speaker mix (handle-less): conditioning vectors for vqvs_unet_forward_vec made on the device from rows of a table ----
 *   d_table [K,E] f32   the rows (class_embed.weight, possibly with further rows behind it)
 *   d_idx   [B,J] int32 row indices; a NEGATIVE index marks an unused slot      d_w [B,J] f32 weights
 *   d_out   [B,E] f32:  out[b][e] = sum over the used slots j, in slot order, of w[b][j] * table[idx[b][j]][e]
 * Every product and every sum is an fp32 operation rounded on its own (contraction off, as in vqvs_guidance_mix), and the first used
 * slot's product is the initial value -- nothing is added to a zero.  A float32 restatement on the host gives the same bits; one used
 * slot of weight 1 copies the row bit for bit.  A row without a used slot is all zeros.  An index >= K reads row K - 1 (never outside
 * the table; callers are expected to have checked).  One thread per four entries of a row, 16 bytes per access when E % 4 == 0 and
 * d_table and d_out are 16-byte aligned, one float at a time otherwise; the grid strides over B.
 * VQVS_ERR_ARG before the device is touched: a NULL pointer; K, E or B below 1; J outside 1..16; d_out overlapping an input. */
int vqvs_speaker_mix(const float* d_table, int K, int E, const int32_t* d_idx, const float* d_w, int J,
                     float* d_out, int B, void* stream);
/* ---- DDIM step (handle-less; Song, Meng, Ermon: "Denoising diffusion implicit models", 2020 -- the reference has no counterpart) ----
 * One step from the time the state is at, alpha_bar = a_t, to the time stepped TO, alpha_bar = a_to, of B rows of T samples:
 *   e    = eps                       or, with d_grad, e = fmaf(-sqrt(1-a_t), grad, eps): a cond_fn's gradient at (x_t, t) enters the
 *                                    prediction, so a guided step is this ONE call (vqvs_ddpm_mean / _guided_eps are not involved)
 *   x0   = fmaf(-sqrt(1-a_t), e, x) * (1/sqrt(a_t)),  e' = e
 *          with CONSTRAIN: x0 = clamp(fmaf(fmaf(-sqrt(1-a_t), e, x), 1/sqrt(a_t), -mean), -1, 1), e' = fmaf(-x0, sqrt(a_t), x) * (1/sqrt(1-a_t))
 *          -- the two halves of vqvs_ddpm_step's CONSTRAIN -- about the row's mean of x0 OF THE GUIDED PREDICTION (summed in fp64 from
 *          the fp32 inputs per 4096 samples, the chunk sums added in chunk order, rounded to fp32 once: B * ceil(T / 4096) doubles of the
 *          per-(device, stream) scratch buffer)
 *   sig  = eta * sqrt(max((1-a_to)/(1-a_t), 0)) * sqrt(max(1 - a_t/a_to, 0));  0 under INVERT or when 1 - a_t == 0
 *   x_to = fmaf(sqrt(a_to), x0, fmaf(sqrt(max(1 - a_to - sig^2, 0)), e', sig * (noise_scale * z)))
 * Coefficients: there is no reference operation order to follow here, so every per-row scalar above is computed IN FP64 from the fp32
 * alphas and rounded to fp32 ONCE -- no cancellation in 1 - a_to - sig^2, one rounding per coefficient; the per-sample operations are
 * fp32 with the fmaf's where they are written (contraction off elsewhere).
 * Direction: a_to is alpha_bar of the time stepped TO.  Sampling steps towards t = 0, a_to > a_t; under VQVS_DDIM_INVERT the same
 * step runs towards LARGER t, a_to < a_t, with sig = 0: for a fixed prediction it is the exact inverse of the eta = 0 step back.
 * eta = 0 is deterministic; at eta = 1, sig^2 = (1 - a_t/a_to)(1-a_to)/(1-a_t) and the step is algebraically vqvs_ddpm_step's with the
 * small sigma (flags 0 / CONSTRAIN) on the same eps -- not under guidance, which the DDPM path applies to the mean at t - step.
 *   d_x_t, d_eps [B,T] f32; d_grad [B,T] f32 or NULL; d_alpha_t, d_alpha_to [B] f32; d_x_to [B,T] f32 out
 *   d_noise [B,T] f32, or NULL to draw z = philox_normal4(seed, quad, clip_offset + row, step_index, stream 0): the words
 *     vqvs_ddpm_step draws, so a run at eta = 1 with its seed sees its noise.  Nothing is drawn, and d_noise is not read, when sig == 0
 *     (eta = 0, INVERT, a_to = 1) or noise_scale == 0.
 * VQVS_ERR_ARG before the device is touched: NULL d_x_t, d_eps, d_alpha_t, d_alpha_to or d_x_to; B outside 1..65535, T outside
 * 1..2^30; eta negative or not finite; flag bit 1 (SIGMA_LARGE has no meaning here) or any undefined bit; INVERT with CONSTRAIN;
 * INVERT with eta != 0; d_x_to overlapping an input. */
#define VQVS_DDIM_CONSTRAIN 2u /* same bit as VQVS_DDPM_CONSTRAIN */
#define VQVS_DDIM_INVERT 4u
int vqvs_ddim_step(const float* d_x_t, const float* d_eps, const float* d_grad, const float* d_noise, const float* d_alpha_t,
                   const float* d_alpha_to, float* d_x_to, int B, int T, uint32_t flags, float eta, float noise_scale,
                   uint64_t seed, uint64_t clip_offset, uint32_t step_index, void* stream);
/* The DDIM step of ONE long signal predicted through overlapping windows: the geometry, limits, 16-byte accesses, per-window means,
 * shared noise per absolute position and d_windows side output of vqvs_ddpm_step_windows, the arithmetic of vqvs_ddim_step.
 *   d_x [Np], d_eps [n,W], d_grad [n,W] or NULL (guidance enters per window, before the blend), d_noise [Np] or NULL,
 *   ONE d_alpha_t / d_alpha_to, d_x_to [Np] out, d_windows [n,W] out or NULL
 * A window b that covers p contributes its own (x0_b, e'_b), guided by its own gradient and constrained about its own mean.  One
 * window: they are used as they are.  Two, left and right, w = (u + 1/2) / V as there: x0 = fmaf(w, x0_r - x0_l, x0_l) and
 * e' = fmaf(w, e'_r - e'_l, e'_l), then the last line above.  At n = 1 the result equals vqvs_ddim_step(B = 1, T = W,
 * clip_offset = clip) bit for bit; at V = 0 without CONSTRAIN it equals one row of n * W samples.
 * VQVS_ERR_ARG before the device is touched: every limit of vqvs_ddpm_step_windows, the eta and flag rules of vqvs_ddim_step, and
 * d_x_to or d_windows overlapping an input or each other. */
int vqvs_ddim_step_windows(const float* d_x, const float* d_eps, const float* d_grad, const float* d_noise, const float* d_alpha_t,
                           const float* d_alpha_to, float* d_x_to, float* d_windows, int n, int W, int H, uint32_t flags, float eta,
                           float noise_scale, uint64_t seed, uint64_t clip, uint32_t step_index, void* stream);
/* ---- DPM-Solver++(2M) step (handle-less; Lu, Zhou, Bao, Chen, Li, Zhu: "DPM-Solver++: fast solver for guided sampling of diffusion
 * probabilistic models", 2022, Algorithm 2 -- the reference has no counterpart) ----
 * The second-order multistep solver of the probability-flow ODE in data-prediction form: one step of B rows of T samples from
 * alpha_bar = a_t to a_to, with the x0 prediction and the alpha_bar (a_from) of the step before as history.  With alpha = sqrt(a),
 * sigma = sqrt(1 - a) and lambda(a) = (log a - log1p(-a)) / 2:
 *   x0   = exactly what vqvs_ddim_step forms: e = eps or, with d_grad, fmaf(-sigma_t, grad, eps); x0 = fmaf(-sigma_t, e, x) * (1/alpha_t)
 *          or, with VQVS_DDIM_CONSTRAIN (bit 2, the only defined flag), clamp(fmaf(fmaf(-sigma_t, e, x), 1/alpha_t, -mean), -1, 1) about
 *          the row's mean of x0 of the guided prediction (fp64 sums per 4096 samples, as there: B * ceil(T / 4096) doubles of the
 *          per-(device, stream) scratch buffer)
 *   h    = lambda(a_to) - lambda(a_t),  h_prev = lambda(a_t) - lambda(a_from),  q = h / (2 h_prev)
 *   c_x  = sigma_to / sigma_t,  phi = alpha_to - sigma_to alpha_t / sigma_t   ( = alpha_to (1 - exp(-h)), without forming h)
 *   c0   = phi (1 + q),  c1 = -phi q
 *   x_to = fmaf(c_x, x, fmaf(c0, x0, c1 * x0_prev));  d_x0_out = x0, the history of the next call
 * Order: the step is FIRST order -- q = 0, x_to = fmaf(c_x, x, c0 * x0), d_x0_prev is not read -- when d_x0_prev is NULL, d_alpha_from
 * is NULL, 1 - a_to == 0, h_prev is not > 0 (a_from == a_t, or a history from a smaller t), or q is not finite; otherwise second
 * order.  At first order the step is algebraically vqvs_ddim_step's at eta = 0; at 1 - a_to == 0, c_x = 0 and phi = 1: the result
 * is x0.  No noise is drawn: the step is deterministic.
 * Coefficients: every per-row scalar (sigma_t, 1/alpha_t, c_x, c0, c1, the mean) is computed IN FP64 from the fp32 alphas and rounded
 * to fp32 ONCE, the rule of vqvs_ddim_step; the per-sample operations are fp32 with the fmaf's where they are written (contraction off
 * elsewhere).  Alphas outside (0, 1) give whatever the formulas give, as there.
 *   d_x_t, d_eps [B,T] f32; d_grad [B,T] f32 or NULL; d_x0_prev [B,T] f32 or NULL; d_alpha_from [B] f32 or NULL;
 *   d_alpha_t, d_alpha_to [B] f32; d_x_to [B,T] f32 out; d_x0_out [B,T] f32 out or NULL
 * Aliasing: d_x0_out may be the SAME pointer as d_x0_prev (each element is read, then written, by one thread).  Any T: 16-byte
 * accesses when T % 4 == 0 and the buffers are 16-byte aligned, one sample at a time otherwise; the values do not depend on which.
 * VQVS_ERR_ARG before the device is touched: NULL d_x_t, d_eps, d_alpha_t, d_alpha_to or d_x_to; B outside 1..65535, T outside
 * 1..2^30; any flag bit but VQVS_DDIM_CONSTRAIN; d_x_to or d_x0_out overlapping an input (but for d_x0_out == d_x0_prev) or each other. */
int vqvs_dpmpp_step(const float* d_x_t, const float* d_eps, const float* d_grad, const float* d_x0_prev, const float* d_alpha_from,
                    const float* d_alpha_t, const float* d_alpha_to, float* d_x_to, float* d_x0_out, int B, int T, uint32_t flags,
                    void* stream);
/* The DPM-Solver++(2M) step of ONE long signal predicted through overlapping windows: the geometry, limits, 16-byte accesses,
 * per-window means and d_windows side output of vqvs_ddim_step_windows, the arithmetic of vqvs_dpmpp_step.
 *   d_x [Np], d_eps [n,W], d_grad [n,W] or NULL, d_x0_prev [Np] or NULL, ONE d_alpha_from (or NULL) / d_alpha_t / d_alpha_to,
 *   d_x_to [Np] out, d_x0_out [Np] out or NULL, d_windows [n,W] out or NULL: d_windows[b,j] = d_x_to[b * H + j]
 * A window b that covers p contributes its own x0_b, guided by its own gradient and constrained about its own mean.  One window: it is
 * used as it is.  Two, left and right, w = (u + 1/2) / V as there: x0 = fmaf(w, x0_r - x0_l, x0_l).  The history d_x0_prev / d_x0_out
 * is this BLENDED x0 in the long layout, one value per absolute position; then the x_to line above.  d_x0_out may be d_x0_prev itself.
 * At n = 1 the result equals vqvs_dpmpp_step(B = 1, T = W) bit for bit; at V = 0 without CONSTRAIN it equals one row of n * W samples.
 * VQVS_ERR_ARG before the device is touched: every limit of vqvs_ddpm_step_windows, the flag rule of vqvs_dpmpp_step, and d_x_to,
 * d_x0_out or d_windows overlapping an input (but for d_x0_out == d_x0_prev) or each other. */
int vqvs_dpmpp_step_windows(const float* d_x, const float* d_eps, const float* d_grad, const float* d_x0_prev, const float* d_alpha_from,
                            const float* d_alpha_t, const float* d_alpha_to, float* d_x_to, float* d_x0_out, float* d_windows, int n, int W,
                            int H, uint32_t flags, void* stream);
/* ---- Packed window steps (handle-less) ----
 * The three ..._step_windows calls on a PACK of R recordings in one launch (two with CONSTRAIN), for converting a corpus: the windows of
 * many short recordings fill one forward, and the step that follows is one call whatever R is.
 *   d_first [R + 1] int32 (device): prefix sums of the recordings' window counts.  first[0] = 0, first[R] = N, the pack's window total;
 *     recording r has n_r = first[r + 1] - first[r] >= 1 windows.
 *   long arrays (d_x, d_noise, d_x_prev / d_x_to, d_x0_prev, d_x0_out): the recordings' rows end to end.  Recording r starts at
 *     off_r = first[r] * H + r * V (V = W - H) and holds n_r * H + V samples; N * H + R * V < 2^31 in all.
 *   window arrays (d_eps, d_grad, d_windows) [N, W]: recording r's windows are rows first[r] .. first[r + 1] - 1.
 *   ONE d_alpha_* each: the recordings of a pack are at the same step.
 * Recording r's slices of the outputs are EXACTLY what the single-recording call writes for (n = n_r, clip = clip + r) on recording r's
 * slices of the inputs, bit for bit: the same cross-fade weights, each window's own CONSTRAIN mean from the same fp64 chunk partials in
 * the same order, drawn noise philox_normal4(seed, quad = (p - off_r) / 4, clip + r, step_index, stream 0).  The last window of
 * recording r and the first of r + 1 are neighbours in [N, W] and are NOT an overlap: nothing of one recording reaches another.
 * Every off_r is a multiple of 4, so a quad never straddles two recordings and every access stays 16 bytes wide.
 * N is read on the device.  The grid is fixed and strides over the pack; with CONSTRAIN the per-(device, stream) scratch buffer is
 * leased at the bound min(65535, (2^31 - 1) / H) * ceil(W / 4096) doubles.  The kernel clamps first[R] to 1..65535 and every other entry
 * to 0..N, and steps a quad only inside the row the table gives it: a table that is not one of prefix sums gives wrong samples, never
 * an access outside N * H + R * V samples or N windows.
 * VQVS_ERR_ARG before the device is touched: every rule of the single-recording call on (W, H, flags, eta, NULL pointers); R outside
 * 1..65535; NULL d_first; and the aliasing rules of the single-recording call, checked over the R * W samples that every array of a pack
 * of R recordings holds at the least (the true extents are on the device). */
int vqvs_ddpm_step_windows_packed(const float* d_x, const float* d_eps, const float* d_noise, const float* d_alpha_t,
                                  const float* d_alpha_prev, float* d_x_prev, float* d_windows, const int32_t* d_first, int R, int W, int H,
                                  uint32_t flags, float noise_scale, uint64_t seed, uint64_t clip, uint32_t step_index, void* stream);
int vqvs_ddim_step_windows_packed(const float* d_x, const float* d_eps, const float* d_grad, const float* d_noise, const float* d_alpha_t,
                                  const float* d_alpha_to, float* d_x_to, float* d_windows, const int32_t* d_first, int R, int W, int H,
                                  uint32_t flags, float eta, float noise_scale, uint64_t seed, uint64_t clip, uint32_t step_index,
                                  void* stream);
int vqvs_dpmpp_step_windows_packed(const float* d_x, const float* d_eps, const float* d_grad, const float* d_x0_prev,
                                   const float* d_alpha_from, const float* d_alpha_t, const float* d_alpha_to, float* d_x_to,
                                   float* d_x0_out, float* d_windows, const int32_t* d_first, int R, int W, int H, uint32_t flags,
                                   void* stream);
/* ---- Keep region (handle-less; the "replacement" method of Song et al., "Score-based generative modeling through stochastic
 * differential equations", 2021, as in RePaint and SDEdit -- the reference has no counterpart) ----
 * IN PLACE on the state d_x [B,T]: every sample with d_keep[row,p] != 0 -- every sample when d_keep is NULL -- is put back on the
 * forward process q(x_t | x0) of a source at alpha_bar = d_alpha[row]:
 *   x[p] = fmaf(ca, x0[p], cn * (noise_scale * z)),   ca = sqrt(alpha), cn = sqrt(max(1 - alpha, 0))
 * ca and cn are computed in fp64 from the fp32 alpha and rounded to fp32 once, the rule of vqvs_ddim_step's coefficients.  A sample
 * that is not kept is not written, and the state is never read.
 *   d_x0 [B,T] f32 the source; d_keep [B,T] uint8 or NULL; d_alpha [B] f32
 *   d_noise [B,T] f32, or NULL to draw z = philox_normal4(seed, quad = p / 4, clip_offset + row, index, stream 3): a stream of its own,
 *     independent of the step noise (0), of x_T (1) and of the loss noise (2).  A sampler passes as `index` the number of the step
 *     that will consume the state.
 * Nothing is drawn, and d_noise is not read, when cn == 0 or noise_scale == 0: then x[p] = ca * x0[p], at alpha = 1 the source bit for
 * bit.  Any T: 16-byte accesses when T % 4 == 0 and the buffers are 16-byte aligned (d_keep: 4-byte), one sample at a time otherwise,
 * and a quad that the mask cuts through stores its kept samples one by one; the values do not depend on which.
 * VQVS_ERR_ARG before the device is touched: NULL d_x, d_x0 or d_alpha; B outside 1..65535, T outside 1..2^30; noise_scale not finite;
 * d_x overlapping d_x0, d_keep, d_noise or d_alpha. */
int vqvs_keep_region(float* d_x, const float* d_x0, const uint8_t* d_keep, const float* d_noise, const float* d_alpha, int B, int T,
                     float noise_scale, uint64_t seed, uint64_t clip_offset, uint32_t index, void* stream);
/* The same on ONE long state in the geometry of vqvs_ddpm_step_windows: d_x [Np], d_x0 [Np], d_keep [Np] or NULL and d_noise [Np] or NULL
 * are indexed by absolute position, Np = (n - 1) * H + W, and there is ONE d_alpha.  A kept sample is written to d_x and, with the same
 * value, to its copy d_windows[b,j] in every window that covers it (d_windows [n,W] in/out, or NULL).  Drawn noise is
 * philox_normal4(seed, p / 4, clip, index, stream 3): what vqvs_keep_region draws for one row of Np samples at clip_offset = clip.  At
 * n = 1 the result equals vqvs_keep_region(B = 1, T = W, clip_offset = clip) bit for bit.
 * VQVS_ERR_ARG before the device is touched: the rules above; every limit of vqvs_ddpm_step_windows on (n, W, H); d_windows overlapping
 * an input or d_x. */
int vqvs_keep_region_windows(float* d_x, float* d_windows, const float* d_x0, const uint8_t* d_keep, const float* d_noise,
                             const float* d_alpha, int n, int W, int H, float noise_scale, uint64_t seed, uint64_t clip, uint32_t index,
                             void* stream);
/* The same on a PACK of R such states in the geometry of "Packed window steps": d_first [R + 1]; the long arrays d_x, d_x0, d_keep (or
 * NULL) and d_noise (or NULL) hold the rows end to end, recording r at off_r = first[r] * H + r * V; d_windows [N,W] or NULL; ONE
 * d_alpha.  Recording r's slices of d_x and d_windows are EXACTLY what vqvs_keep_region_windows writes for (n = n_r, clip = clip + r)
 * on recording r's slices, bit for bit: the same coefficients, drawn noise philox_normal4(seed, quad = (p - off_r) / 4, clip + r,
 * index, stream 3).  A kept sample is written to d_x and to each window copy that covers it inside its own recording only -- the last
 * window of recording r and the first of r + 1 are not an overlap --, and a sample outside the mask is not written.  N is read on the
 * device; the grid is fixed and strides over the pack, and the table is clamped as the packed steps clamp it: a table that is not one
 * of prefix sums gives wrong samples, never an access outside N * H + R * V samples or N windows.
 * VQVS_ERR_ARG before the device is touched: every rule of vqvs_keep_region_windows on (W, H, noise_scale, NULL pointers); R outside
 * 1..65535; NULL d_first; and its aliasing rules (d_first among the inputs), checked over the R * W samples a pack holds at the least. */
int vqvs_keep_region_windows_packed(float* d_x, float* d_windows, const float* d_x0, const uint8_t* d_keep, const float* d_noise,
                                    const float* d_alpha, const int32_t* d_first, int R, int W, int H, float noise_scale, uint64_t seed,
                                    uint64_t clip, uint32_t index, void* stream);
/* ---- Pauses (handle-less; the reference has no counterpart) ----
 * The mask of the samples of a pack's source rows that lie in a pause, for vqvs_keep_region_windows_packed.  Integer arithmetic
 * throughout, as in vqvs_pitch_distance: the mask equals its definition bit for bit, and a recording's mask does not depend on R,
 * on its place in the pack or on the run.
 *   d_x [N * H + R * V] f32: the padded source rows in the layout of "Packed window steps" (the zero padding is part of a row)
 *   d_keep, same layout, uint8: fully written with 0 or 1.   d_counts [R,2] int64 or NULL: kept samples and pauses per recording
 *   frame: samples per frame, a multiple of 4 in 4..4096; thr: energy per sample, 0..2^30; min_frames 1..2^20; guard_frames 0..2^20
 * Per recording row of L = n_r * H + V samples: q[n] = clamp(rint(x[n] * 32768), -32768, 32767), NaN -> 0 (the sample rule of
 * vqvs_pitch_distance).  Frame f covers [f * frame, min((f + 1) * frame, L)) and holds c_f samples; E_f = sum q^2; the frame is
 * QUIET iff E_f <= thr * c_f.  A PAUSE is a maximal run of quiet frames at least min_frames long; its kept part is the run less
 * guard_frames at each end that touches a loud frame (an end at the row's start or end is not trimmed); keep[n] = 1 iff n's frame
 * lies in a kept part.  Equivalently, with left(f) the last loud frame <= f or -1 and right(f) the first loud frame >= f or F, frame
 * f is kept iff it is quiet, right - left - 1 >= min_frames, (left < 0 or f - left > guard) and (right >= F or right - f > guard).
 * N is read on the device and the table clamped as above; the per-(device, stream) scratch buffer is leased at
 * 8 * (min(65535 H + R V, 2^31) / (256 frame) + R + 1) bytes.  No floating-point atomics.
 * VQVS_ERR_ARG before the device is touched: NULL d_x, d_keep or d_first; R outside 1..65535; the rules on (W, H) above; frame, thr,
 * min_frames or guard_frames outside their ranges; d_keep or d_counts overlapping d_x, d_first or each other (over R * W samples). */
int vqvs_pause_mask(const float* d_x, uint8_t* d_keep, int64_t* d_counts, const int32_t* d_first, int R, int W, int H, int frame,
                    int64_t thr, int min_frames, int guard_frames, void* stream);
/* d_out [N] uint8: out[b] = 1 iff all W bytes of window b of the mask d_keep (any mask in the layout above) are non-zero -- a window
 * whose every sample the keep region overwrites after every step, so that its forward cannot reach the result.
 * VQVS_ERR_ARG before the device is touched: NULL d_keep, d_out or d_first; R outside 1..65535; the rules on (W, H); d_out overlapping
 * d_keep or d_first. */
int vqvs_windows_kept(const uint8_t* d_keep, uint8_t* d_out, const int32_t* d_first, int R, int W, int H, void* stream);
/* x_T ~ N(0,1) from the same counter-based generator (replaces torch.randn, sample_diffusion.py:86) */
int vqvs_randn(float* d_out, int B, int T, uint64_t seed, uint64_t clip_offset, uint32_t stream_id, void* stream);

/* ---- forward process and denoising loss (handle-less) ------------------------------------
 * x_t = Diffusion.sample_q(x_0, ts, epsilon) = sqrt(a) * x_0 + sqrt(1 - a) * eps   reference diffusion/diffusion.py:17-26
 *   d_x0    [x0_rows,T] f32, x0_rows = B or 1 (one clip broadcast to every row: speaker search)
 *   d_alpha [B] f32: schedule(ts), evaluated by the caller as for vqvs_ddpm_step
 *   d_eps   [eps_rows,T] f32 with eps_rows = B or 1 (one noise row broadcast), or NULL to draw N(0,1) in the kernel from the
 *           Philox generator of vqvs_ddpm_step / vqvs_randn on stream id 2, keyed by (seed, index of the row) with
 *           index = d_noise_index[b] (int64 [B]) or, when d_noise_index is NULL, clip_offset + b.  Rows with equal indices get
 *           equal noise -- the reference's "fix a noise seed for every example" (voice_search_vqvae.py:79-80) without a tensor
 *           of copies.  eps_rows is not read when d_eps is NULL (0, 1 or B are accepted).
 *   d_x_t   [B,T] f32 out.  Any T in 1..2^30; B in 1..65535.  16-byte accesses when T % 4 == 0 and the buffers are 16-byte
 *           aligned, scalar ones otherwise: the values do not depend on which. */
int vqvs_ddpm_noise(const float* d_x0, int x0_rows, const float* d_alpha, const float* d_eps, int eps_rows,
                    const int64_t* d_noise_index, float* d_x_t, int B, int T, uint64_t seed, uint64_t clip_offset, void* stream);
/* loss[b] = mean_t (eps[b,t] - pred[b,t])^2   reference diffusion.py:151, voice_search_vqvae.py:98
 *   d_pred [B,T] f32; the noise arguments of vqvs_ddpm_noise -- given, broadcast, or REGENERATED from the same counters, so the
 *   noise of a generated batch is never written to memory; d_loss [B] f32 out.
 * Differences and squares in f32, sums in f64 in a fixed order: a workgroup folds 4096 consecutive samples of one row, one
 * thread adds the row's chunk sums in chunk order and is the row's only writer (no atomics).  Equal rows give bitwise-equal
 * losses whatever B and the row's position are.  Keeps B * ceil(T / 4096) doubles in the per-(device, stream) scratch buffer. */
int vqvs_ddpm_sqerr(const float* d_pred, const float* d_eps, int eps_rows, const int64_t* d_noise_index, float* d_loss,
                    int B, int T, uint64_t seed, uint64_t clip_offset, void* stream);

/* ---- vector quantisation -------------------------------------------------------
 * idx = argmin_k ((-2 z.e_k) + |e_k|^2) + |z|^2, first index on ties
 * reference vq.py:112-143, 199-243.   d_z [B,Cd,T1] f32 NCT, d_dict [K,Cd] f32 -> d_idx [B,T1] int64
 * B in 1..65535 (a grid dimension), Cd a positive multiple of 4, T1 and K positive: anything else, or a NULL pointer, returns
 * VQVS_ERR_ARG with a message before the device is touched.  A position of z that holds a NaN gets code 0 (no distance
 * compares below the running best), which is what torch.argmin returns for an all-NaN row.  tests/vq_ref.py states the bound
 * the fp32 distance is held to against a float64 nearest-code reference. */
int vqvs_vq_argmin(const float* d_z, const float* d_dict, int64_t* d_idx, int B, int Cd, int T1, int K, void* stream);
/* Quantise and score in one pass (handle-less): what VQ.forward and StandardVQLoss need of z (reference vq.py:45-51, 112-143),
 * plus the code counts of an evaluation pass.
 *   d_z [B,Cd,T1] f32 NCT, d_dict [K,Cd] f32; the limits of vqvs_vq_argmin (Cd a multiple of 4), B in 1..65535
 *   d_idx      [B,T1] int64 out: bit-identical to vqvs_vq_argmin on the same inputs (the two kernels call one search routine:
 *              same distance formula, same fmaf order, first index on ties)
 *   d_embedded [B,Cd,T1] f32 NCT out, or NULL: d_embedded[b,:,t] = d_dict[idx[b,t],:], an exact copy, written along time
 *   d_sqerr    [B] f64 out, or NULL: sum over c,t of (z[b,c,t] - e[b,c,t])^2.  Differences and squares in f32, sums in f64 in a
 *              fixed order: a workgroup folds its 32 positions x Cd channels, one thread adds the clip's tile sums in tile order
 *              and is the clip's only writer (no floating-point atomics).  A clip's value is bitwise the same whatever B and
 *              its row are; a clip whose columns are dictionary rows scores exactly 0.
 *   d_hist     [K] int64 in/out, or NULL: d_hist[k] += number of positions of THIS call that chose code k (integer atomics:
 *              exact in any order).  The caller zeroes it once and passes it to every call of a pass.
 * z is not fetched from HBM again: the epilogue re-reads the workgroup's own tile, which the search has just walked K / 128
 * times, from L2.  Keeps B * ceil(T1 / 32) doubles and K floats in the per-(device, stream) scratch buffer.  Asynchronous on
 * `stream`; NULL d_z / d_dict / d_idx or non-positive sizes return VQVS_ERR_ARG before the device is touched. */
int vqvs_vq_quantize(const float* d_z, const float* d_dict, int64_t* d_idx, float* d_embedded, double* d_sqerr, int64_t* d_hist,
                     int B, int Cd, int T1, int K, void* stream);
/* out[b,:,t] = dict[idx[b,t],:]   reference vq.py:98-110
 *   d_idx [B,T1] int64 (values outside 0..K-1 are clamped into it), d_dict [K,Cd] f32 -> d_out [B,Cd,T1] f32 NCT, an exact copy.
 * B and Cd in 1..65535 (grid dimensions z and y; any Cd, not only multiples of 4), T1 and K positive: a NULL pointer, a
 * non-positive size, or B or Cd above 65535 returns VQVS_ERR_ARG with a message before anything is launched. */
int vqvs_vq_embed(const int64_t* d_idx, const float* d_dict, float* d_out, int B, int Cd, int T1, int K, void* stream);

/* ---- guidance-model scores (handle-less) -------------------------------------------------
 * Cross-entropy, accuracy, top-k and confusion counts of classification logits in one call: what the reference logs while it
 * trains its two guidance models (train_loop.py:551-561 the classifier's NLL of the label, :602-613 the encoder predictor's code
 * cross-entropy), plus the counts an evaluation wants.
 *   d_logits  [B,K,L] f32, NCT with L contiguous: what vqvs_encpred_forward writes; a classifier's [B,K] logits are L = 1
 *   d_targets [B,L] int64.  B in 1..65535, K in 1..8192, L in 1..2^24
 * For a position (b, l) with target y:  rank = #{j : logit_j > logit_y} + #{j < y : logit_j == logit_y}, on the raw f32 logits:
 * ties go to the first index, as in vqvs_vq_argmin; a NaN target logit ranks K.  A count: exact, whatever order it is taken in.
 *   d_nll       [B] f64 out: sum over l of (logsumexp_j logit_j - logit_y).  The maximum is found in f32, the differences from
 *               it are formed in f64 from the f32 inputs, exp and log are f64, and all sums are f64 in a fixed order: a
 *               workgroup folds 64 positions, one thread adds the clip's tile sums in tile order and is the clip's only writer
 *               (no floating-point atomics).  A clip's value is bitwise the same whatever B and its row are.
 *   d_top1      [B] int64 out, or NULL: number of positions with rank 0
 *   d_topk      [B] int64 out, or NULL: number of positions with rank < k; k in 1..K when given (k is not read otherwise)
 *   d_confusion [K,K] int64 in/out, or NULL: d_confusion[y, argmax] += 1 per position, argmax = first index of the maximum
 *               (integer atomics: exact in any order).  The caller zeroes it once and passes it to every call of a pass.
 * A target outside 0..K-1 is never used as an index: that clip's d_nll becomes NaN and the position is counted nowhere.
 * L > 1: lanes run along L (coalesced rows), eight waves split K and meet in LDS; keeps 16 bytes per (clip, 64-position tile)
 * in the per-(device, stream) scratch buffer.  L = 1: lanes run along K, one workgroup (one wave up to K = 256) per row.
 * Asynchronous on `stream`; NULL d_logits / d_targets / d_nll, sizes outside the limits or k out of range return VQVS_ERR_ARG
 * before the device is touched. */
int vqvs_xent_score(const float* d_logits, const int64_t* d_targets, double* d_nll, int64_t* d_top1, int64_t* d_topk, int k,
                    int64_t* d_confusion, int B, int K, int L, void* stream);

/* ---- conversion-quality scores (handle-less) ---------------------------------------------
 * Two frame-synchronous spectral distances between waveform batches a and b, per clip the SUM over frames, in one kernel
 * (spectral_kernels.hip; no spectrum, mel value or cepstrum goes to memory).  Frames F = T / hop + 1, centred, reflect padding of
 * n_fft / 2 on both sides.  Per frame, with the rounding points of the MFCC front end:
 *   xw[n] = f32(x[s] * window[n]);  P[k] = |sum_n xw[n] e^{-2 pi i k n / n_fft}|^2, a direct DFT accumulated in f64 against
 *   d_twiddle, rounded to f32;  mel[m] = sum_k P[k] fb[k,m] in f64 -> f32;  L[m] = log(mel[m] + eps), the sum in f32, the logarithm
 *   in f64 rounded to f32 once;  c[j] = sum_m L[m] dct[m,j] in f64 -> f32;  then in f64
 *   mcd = (10 / ln 10) sqrt(2 sum_{j=1}^{n_ceps-1} (c_a[j] - c_b[j])^2)      (coefficient 0 is left out)
 *   lsd = (10 / ln 10) sqrt((1 / n_mels) sum_m (L_a[m] - L_b[m])^2)
 *   d_a, d_b  [B,T] f32;  d_window [n_fft] f32;  d_twiddle [n_fft][2] f64: cos and sin of 2 pi i / n_fft
 *   d_fb [n_fft/2+1, n_mels] f32;  d_dct [n_mels, n_ceps] f32  (caller-owned device constants)
 *   d_mcd, d_lsd  [B] f64 out: either may be NULL, not both
 * Both signals of a frame run through the same instruction sequence, a workgroup adds its four frames in frame order, and one
 * thread adds a clip's workgroup partials (16 bytes per (clip, workgroup) in the per-(device, stream) scratch buffer) in order and
 * is the clip's only writer -- no floating-point atomics.  So d(a, a) is exactly 0, d(a, b) == d(b, a) bitwise, and a clip's value
 * is bitwise the same from run to run and whatever B and its row are.
 * Limits: B in 1..65535; n_fft even, in 16..512; n_fft / 2 < T <= 2^30 with at most 2^25 frames; hop in 1..n_fft; n_mels in
 * 1..128; n_ceps in 2..min(n_mels, 64); eps finite and positive; an output may not overlap an input or the other output.
 * Asynchronous on `stream`; a NULL required pointer, both outputs NULL or anything outside the limits returns VQVS_ERR_ARG with
 * a message before the device is touched. */
int vqvs_spectral_distance(const float* d_a, const float* d_b, const float* d_window, const double* d_twiddle,
                           const float* d_fb, const float* d_dct, double* d_mcd, double* d_lsd,
                           int B, int T, int n_fft, int hop, int n_mels, int n_ceps, float eps, void* stream);

/* ---- mel cepstra per frame (handle-less) --------------------------------------------------
 * The per-frame values that vqvs_spectral_distance forms and throws away, written to memory for recordings of different lengths
 * in one batch (spectral_kernels.hip).  The arithmetic is that of "conversion-quality scores" above bit for bit, rounding points
 * included: both kernels call one copy of the front end (window, DFT, power, mel, log, DCT).
 *   d_x       [B,T] f32; row b holds len_b samples, what lies at or beyond len_b is never read (zeros, garbage or NaN alike)
 *   d_len     [B] int32: device data, clamped into n_fft/2+1 .. T before use, so that no value can index outside an array
 *   d_window, d_twiddle, d_fb, d_dct: the constant tables of vqvs_spectral_distance
 *   d_ceps    [B, Fmax, n_ceps] f32 out, Fmax = T / hop + 1;  d_logmel [B, Fmax, n_mels] f32 out or NULL
 *   d_frames  [B] int32 out: F_b = len_b / hop + 1 (of the clamped length)
 * Row b has F_b frames, centred and reflect-padded about ITS OWN ends 0 and len_b; frames f >= F_b are written as 0.  One writer
 * per output and no atomics: a row's values are bitwise the same whatever B, its row index, T and the padding are, and equal those
 * of the row alone at T = len_b.
 * Limits: those of vqvs_spectral_distance (B, n_fft, T, hop, n_mels, n_ceps, eps); an output may not overlap an input or another
 * output.  Asynchronous on `stream`; a NULL required pointer (everything but d_logmel) or anything outside the limits returns
 * VQVS_ERR_ARG with a message before the device is touched. */
int vqvs_mel_cepstra(const float* d_x, const int* d_len, const float* d_window, const double* d_twiddle, const float* d_fb,
                     const float* d_dct, float* d_ceps, float* d_logmel, int* d_frames,
                     int B, int T, int n_fft, int hop, int n_mels, int n_ceps, float eps, void* stream);

/* ---- alignment: dynamic time warping under the mel-cepstral cost (handle-less) -------------
 * For B pairs of cepstral sequences, the cheapest monotone warping path and what it carries (dtw_kernels.hip; DESIGN.md section
 * 3.18).  With Fa, Fb the pair's frame counts:
 *   local cost, f64 from the f32 cepstra, c in index order, single operations without contraction:
 *     d(i,j) = (10 / ln 10) sqrt(2 sum_{c=1}^{n_ceps-1} (ca[i,c] - cb[j,c])^2)              (coefficient 0 is left out)
 *   D(0,0) = d(0,0);  D(i,j) = d(i,j) + min(D(i-1,j-1), D(i-1,j), D(i,j-1)) over the predecessors that exist; of equal ones the
 *   first in that order (diagonal, then i-1, then j-1) is chosen.  The path runs from (0,0) to (Fa-1,Fb-1): no band, no slope
 *   constraint.  Every cell carries what its chosen predecessor carried plus its own contribution: steps (cells on the path so
 *   far), and with tracks both (cells where ta[i] and tb[j] are finite), vuv (cells where exactly one is), and sum l, sum l^2 over
 *   the `both` cells, l = tb[j] - ta[i].  The path itself is not an output.
 *   d_ca [B, Fa_max, n_ceps], d_cb [B, Fb_max, n_ceps] f32;  d_fa, d_fb [B] int32: device data, clamped into 1..F*_max
 *   d_ta [B, Fa_max], d_tb [B, Fb_max] f64 or NULL (both or neither): per-frame tracks, NaN = no value in this frame
 *   d_cost [B] f64 out: D(Fa-1, Fb-1);  d_steps [B] int32 out: the path's length
 *   d_track_counts [B,2] int64 out: both, vuv;  d_track_sums [B,2] f64 out: sum l, sum l^2 -- required if and only if tracks are given
 * One workgroup per pair walks the anti-diagonals i + j with one barrier per diagonal; the live diagonals sit in LDS (at most
 * 128 KiB) and the thread of the last cell is the pair's only writer -- no scratch, no direction matrix, no atomics.  A pair's
 * outputs are bitwise the same from run to run and whatever B, its row and F*_max are; cost(a,b) == cost(b,a).
 * Limits: B in 1..65535; Fa_max, Fb_max in 1..2048; n_ceps in 2..64; an output may not overlap an input or another output.
 * Asynchronous on `stream`; a NULL required pointer, exactly one track, exactly one track output, track outputs without tracks or
 * tracks without track outputs, or a size outside the limits returns VQVS_ERR_ARG with a message before the device is touched. */
int vqvs_dtw_distance(const float* d_ca, const float* d_cb, const int* d_fa, const int* d_fb, const double* d_ta, const double* d_tb,
                      double* d_cost, int* d_steps, long long* d_track_counts, double* d_track_sums,
                      int B, int Fa_max, int Fb_max, int n_ceps, void* stream);

/* ---- pitch scores (handle-less) -----------------------------------------------------------
 * YIN periods of waveform batches a and b, frame for frame, and per clip the voicing counts and the sums of the pitch distance in
 * semitones, in one kernel (pitch_kernels.hip; no frame or difference function goes to memory).  Frames F = T / hop + 1.  The
 * definition, per signal and frame f, with S = window + tau_max:
 *   q[n] = clamp(rint(x[n] * 32768), -32768, 32767), NaN -> 0: the samples of a 16-bit WAV; frame f reads q[s .. s + S),
 *   s = f hop - S / 2, zeros outside [0, T);  d(tau) = sum_{j < window} (q[s+j] - q[s+j+tau])^2, c(tau) = sum_{k=1..tau} d(k):
 *   integers below 2^53, the same in any order;  d'(tau) = 1 if c(tau) = 0, else double(d(tau) tau) / double(c(tau));
 *   tau0 = the smallest tau in [tau_min, tau_max] with d'(tau) < threshold (none: the frame is unvoiced, period 0.0), then tau
 *   walks up while d'(tau + 1) < d'(tau);  period = tau if tau = tau_max, else with y0, y1, y2 = d'(tau-1), d'(tau), d'(tau+1) and
 *   den = (y0 - y1) + (y2 - y1): tau + clamp(0.5 (y0 - y2) / den, -1, 1) if den > 0, else tau -- single float64 operations in
 *   this order, no contraction.
 * Over the frames voiced (period > 0) in both signals: l_f = +-12 log2(hi / lo) of the larger and smaller period, positive where
 * period_a >= period_b: the semitones by which b is higher than a.
 *   a, b       [B,T] f32; b may be NULL: track a only (then period_b, counts and sums must be NULL and period_a given)
 *   period_a, period_b  [B,F] f64 out or NULL: samples, 0 = unvoiced
 *   counts     [B,4] int64 out or NULL: frames voiced in a, in b, in both, and frames whose voicing differs
 *   sums       [B,2] f64 out or NULL: sum of l_f and of l_f^2
 * The periods are the definition's bit for bit.  Both signals of a frame run through the same instruction sequence, a workgroup
 * adds its four frames in frame order and one thread adds a clip's workgroup partials (32 bytes per (clip, workgroup) in the
 * per-(device, stream) scratch buffer) in order and is the clip's only writer -- no floating-point atomics.  So b = a gives sums
 * (0, 0) without a sign bit, swapping a and b negates the first sum bitwise, and a clip's values are the same from run to run and
 * whatever B and its row are.  Every non-NULL output is fully written; a NULL output leaves the others unchanged.
 * Limits: B in 1..65535; T in 1..2^30 with at most 2^25 frames; window in 16..2048; hop in 1..window; 2 <= tau_min < tau_max <=
 * 1023; window * tau_max <= 2^20; threshold finite, in (0, 1]; an output may not overlap an input or another output.
 * Asynchronous on `stream`; NULL a, every output NULL or anything outside the limits returns VQVS_ERR_ARG with a message before
 * the device is touched. */
int vqvs_pitch_distance(const float* a, const float* b, double* period_a, double* period_b, long long* counts, double* sums,
                        int B, int T, int window, int hop, int tau_min, int tau_max, double threshold, void* stream);

/* ---- test / profiling hooks ------------------------------------------------------ */
int vqvs_debug_tap_count(const vqvs_model* m);
int vqvs_debug_tap_info(const vqvs_model* m, int i, char* name_out, int name_cap, int* channels, int* length_shift);
/* rows per clip of tap i at clip length T (UNet taps: T >> length_shift; MFCC encoder taps: frame counts) */
int vqvs_debug_tap_rows(const vqvs_model* m, int i, int T);
/* copies tap i of the LAST forward to host as float32 NCT [B][C][L]; synchronises the device */
int vqvs_debug_read_tap(vqvs_model* m, int i, int B, int T, float* h_out);
/* copies the conditioning vector of the LAST forward -- time_embed_extra(time_embed(ts)) [+ class_embed(labels)], reference
 * unet.py:133-135 with wavegrad.py:359-373 -- to host as float32 [B][4*base_channels]; returns its width; synchronises */
int vqvs_debug_read_embedding(vqvs_model* m, int B, float* h_out);
/* copies d mse_b / d (FiLM rows) of the LAST vqvs_unet_embed_grad -- per clip the (d a | d b) rows of every ResBlock in the order
 * down_blocks, middle_blocks, up_blocks, 2 * cout rows each -- to host as float32 [B][R]; returns R; synchronises */
int vqvs_debug_read_dfilm(vqvs_model* m, int B, float* h_out);
/* copies the FiLM rows of the LAST forward -- per clip the (a | b) rows bias + W . gelu(embedding) of every ResBlock's cond_layers in
 * the order down_blocks, middle_blocks, up_blocks, 2 * cout rows each (physical widths on a padded handle) -- to host as float32
 * [B][R]; returns R; synchronises.  VQVS_ERR_STATE on a model kind without a FiLM table */
int vqvs_debug_read_film(vqvs_model* m, int B, float* h_out);
/* GroupNorm i (schedule order, 0..count-1) of a handle created with debug_taps = 1 -- other handles count 0 and every entry below
 * returns VQVS_ERR_STATE -- as the LAST forward at (B, T) ran it.  Read-only: no entry changes the arena or the status word.
 * info (24 x int64): [0] Ctot, [1] groups, [2] values per group behind inv_count = (real channels per group) * rows, [3] FiLM applies,
 * [4] its offset into a clip's FiLM rows (a at [4] .. [4] + Ctot, b behind them), [5] sources (1, or 2 for a GroupNorm over a
 * concatenation), [6] the schedule keeps a (mean, rstd) table, [7] the consuming convolution built the (scale, shift) table itself
 * at this (B, T) -- then the global table was not written --, and per source s at [8 + 4 s ..]: C, rows per clip, rows per
 * statistics tile of its producer, tiles per clip; at [16 + s]: its producer summed the values as STORED (0: the float32 values before
 * they were rounded to a 2-byte storage type -- in_conv_kernel and conv_mfma_kernel in the bf16 / fp16 modes). */
int vqvs_debug_gn_count(const vqvs_model* m);
int vqvs_debug_gn_info(vqvs_model* m, int i, int B, int T, char* name_out, int name_cap, int64_t* info);
/* what 0: source `src` as stored, float32 NCT [B][C][rows];  1: its tile partials (sum x, sum x^2) [B][tiles][C][2];
 * 2: the (scale, shift) table [B][Ctot][2] -- where info[7] is set, what the schedule's gn_prepare launch makes of the resident
 * partials, written to a scratch table --;  3: the (mean, rstd) table [B][Ctot][2] (VQVS_ERR_STATE without one).  Synchronises. */
int vqvs_debug_gn_read(vqvs_model* m, int i, int B, int T, int what, int src, float* h_out);
/* xform entry i (the stand-alone gelu(scale * x + shift) [+ avg_pool(2)] pass in front of some convolutions), same rules.
 * info (8 x int64): [0] GroupNorm whose table it reads, [1] C, [2] input rows, [3] output rows, [4] avg, [5] the table's row stride,
 * [6] its first column.  vqvs_debug_xform_read: the input (output = 0) or output (1) tensor as float32 NCT. */
int vqvs_debug_xform_count(const vqvs_model* m);
int vqvs_debug_xform_info(vqvs_model* m, int i, int B, int T, int64_t* info);
int vqvs_debug_xform_read(vqvs_model* m, int i, int B, int T, int output, float* h_out);
/* handle-less: d_out[i] = one of the library's GELU device functions (csrc/common.hpp) of d_in[i], n float32 device values each.
 * form 0: gelu_f; 1, 2, 3: gelu2 at GELU_EXACT, GELU_POLY6, GELU_POLY7 (the fp32, bf16 and fp16 modes' prologues), evaluated on the
 * pairs (2i, 2i+1) as the prologues evaluate them, an odd tail paired with 0; 4: gelu_grad_f.  VQVS_ERR_ARG before the device is
 * touched: NULL d_in or d_out; n < 1 or n > 2^30; form outside 0..4 */
int vqvs_debug_gelu(const float* d_in, float* d_out, int n, int form, void* stream);
/* number of kernels one forward enqueues, and the algorithmic activation bytes it moves (SURVEY 8d Model A) */
int vqvs_forward_kernel_count(const vqvs_model* m);
int64_t vqvs_forward_model_bytes(const vqvs_model* m, int B, int T);
int64_t vqvs_forward_flops(const vqvs_model* m, int B, int T);

/* live per-kernel timing: when on, every forward brackets each enqueued kernel with hipEvents on
 * the launch stream; vqvs_profile_read returns the elapsed ms of each op of the last forward and
 * vqvs_op_info its kind ("conv", "gn_prepare", ...) and algorithmic bytes / flops for (B, T). */
int vqvs_set_profiling(vqvs_model* m, int on);
int vqvs_op_info(const vqvs_model* m, int i, char* kind_out, int kind_cap, int64_t* bytes_out, int64_t* flops_out, int B, int T);
int vqvs_op_desc(const vqvs_model* m, int i, char* out, int cap);
int vqvs_profile_read(vqvs_model* m, float* h_ms, int cap);
/* In-kernel phase counters of the instrumented build (`make -C vq_voice_swap_amd/csrc timing`, -DVQVS_TIMING: libvqvs_timing.so), summed
 * over the sampled waves of every launch since the last reset and copied to host; reset != 0 clears them; synchronises the device.
 * Every other build exports the two entries and returns VQVS_ERR_STATE.
 * conv_timing (conv_mfma.hip): 24 x uint64 -- [0..17] shader-clock ticks per phase (tools/conv_phases.py names them), [18..21] spread
 * of the workgroups' starts and ends in 100 MHz ticks, [23] sampled waves.
 * ws_timing (conv_ws.hip): 32 x uint64 -- [0..4] producer phases, [8..14] consumer phases (tools/ws_phases.py), [16] / [17] sampled
 * producer / consumer waves, [18] steps, [19] tiles, [20] / [21] shader-clock and 100 MHz ticks per workgroup, [22..25] startup. */
int vqvs_debug_conv_timing(unsigned long long* h_counters, int reset);
int vqvs_debug_ws_timing(unsigned long long* h_counters, int reset);

const char* vqvs_last_error(void);
const char* vqvs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VQVS_H */
