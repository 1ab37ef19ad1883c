// extern "C" surface of libvqvs_hip.so (declared and documented in include/vqvs.h).
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "net.hpp"
#include "sampler_kernels.hpp"

namespace vqvs {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

// scratch of the handle-less entry points (DDPM step partial sums, VQ code norms, discarded logits): one buffer per
// (device, stream), so calls issued on different streams never share it -- work on ONE stream is ordered by the stream itself.
// A buffer only ever grows.  An entry point holds a LEASE on its buffer (ScratchLease, an in-flight count under the mutex) from
// scratch_get until its kernels are ENQUEUED: a buffer is only freed -- by a grow on the same stream or by the eviction of the
// least recently used buffer once a device has more than MAX_STREAMS of them -- when no lease is out on it and after the owning
// device (the current one: the map is keyed by hipGetDevice) was synchronised, so neither a thread that has the pointer but has
// not launched yet nor a queued kernel can still be using it.  A leased buffer that has to grow is retired instead and freed by
// the first later call that finds the entry without leases.
struct DeviceScratch {
  void* p = nullptr;
  size_t bytes = 0;
  unsigned long long used = 0;
  int leases = 0;
  std::vector<void*> retired;
};
static std::map<std::pair<int, void*>, DeviceScratch> g_scratch;
static std::mutex g_scratch_mu;
static unsigned long long g_scratch_tick = 0;
struct ScratchLease {
  DeviceScratch* sc = nullptr;
  void* p = nullptr;
  ScratchLease() = default;
  ScratchLease(const ScratchLease&) = delete;
  ScratchLease& operator=(const ScratchLease&) = delete;
  ~ScratchLease() {
    if (!sc) return;
    std::lock_guard<std::mutex> lk(g_scratch_mu);  // (std::map nodes are stable: the entry cannot have moved, and a leased one is never erased)
    --sc->leases;
  }
};
static int scratch_get(size_t bytes, void* stream, ScratchLease& lease) {
  constexpr size_t MIN_BYTES = (size_t)1 << 20;
  constexpr size_t MAX_STREAMS = 32;
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  int dev = 0;
  VQVS_HIP(hipGetDevice(&dev));
  const auto key = std::make_pair(dev, stream);
  if (g_scratch.find(key) == g_scratch.end()) {
    size_t n_dev = 0;
    auto lru = g_scratch.end();
    for (auto it = g_scratch.begin(); it != g_scratch.end(); ++it)
      if (it->first.first == dev) {
        ++n_dev;
        if (it->second.leases == 0 && (lru == g_scratch.end() || it->second.used < lru->second.used)) lru = it;
      }
    if (n_dev >= MAX_STREAMS && lru != g_scratch.end()) {  // (streams come and go: their buffers are reclaimed here, oldest idle one first;
      VQVS_HIP(hipDeviceSynchronize());                     //  with every buffer leased the cap is exceeded for the moment)
      if (lru->second.p) VQVS_HIP(hipFree(lru->second.p));
      for (void* q : lru->second.retired) VQVS_HIP(hipFree(q));
      g_scratch.erase(lru);
    }
  }
  DeviceScratch& sc = g_scratch[key];
  if (sc.leases == 0 && (!sc.retired.empty() || (sc.p && sc.bytes < bytes))) {
    VQVS_HIP(hipDeviceSynchronize());
    for (void* q : sc.retired) VQVS_HIP(hipFree(q));
    sc.retired.clear();
    if (sc.p && sc.bytes < bytes) {
      VQVS_HIP(hipFree(sc.p));
      sc.p = nullptr;
      sc.bytes = 0;
    }
  } else if (sc.p && sc.bytes < bytes) {  // (another thread on the same stream still holds the smaller buffer: retire it, free it later)
    sc.retired.push_back(sc.p);
    sc.p = nullptr;
    sc.bytes = 0;
  }
  if (!sc.p) {
    size_t n = bytes < MIN_BYTES ? MIN_BYTES : bytes;
    VQVS_HIP(hipMalloc(&sc.p, n));
    sc.bytes = n;
  }
  sc.used = ++g_scratch_tick;
  ++sc.leases;
  lease.sc = &sc;
  lease.p = sc.p;
  return 0;
}
}  // namespace vqvs

using namespace vqvs;

extern "C" {

const char* vqvs_last_error(void) { return g_err.c_str(); }
#ifndef VQVS_BUILD_ID
#define VQVS_BUILD_ID "unstamped"
#endif
const char* vqvs_version(void) { return "vqvs-hip 0.1 (gfx950) build " VQVS_BUILD_ID; }  // (build id: hash of the sources, csrc/Makefile)

int vqvs_pad_blocks(int real_base_channels, int* q, int* q_p) {
  if (real_base_channels < 1 || !q || !q_p) VQVS_FAIL(VQVS_ERR_ARG, "vqvs_pad_blocks: real_base_channels must be positive and q, q_p not NULL");
  pad_blocks(real_base_channels, q, q_p);
  return 0;
}

int vqvs_param_count(const vqvs_cfg* cfg) {
  if (!cfg) VQVS_FAIL(VQVS_ERR_ARG, "cfg is NULL");
  std::vector<ParamDef> p;
  if (int e = enumerate_params(*cfg, p)) return e;
  return (int)p.size();
}

int vqvs_param_info(const vqvs_cfg* cfg, int index, char* name_out, int name_cap, int64_t shape_out[4], int* ndim_out) {
  if (!cfg) VQVS_FAIL(VQVS_ERR_ARG, "cfg is NULL");
  std::vector<ParamDef> p;
  if (int e = enumerate_params(*cfg, p)) return e;
  if (index < 0 || index >= (int)p.size()) VQVS_FAIL(VQVS_ERR_ARG, "param index %d out of range", index);
  const ParamDef& d = p[index];
  if (name_out && name_cap > 0) {
    strncpy(name_out, d.name.c_str(), name_cap - 1);
    name_out[name_cap - 1] = 0;
  }
  if (shape_out)
    for (int i = 0; i < 4; ++i) shape_out[i] = i < (int)d.shape.size() ? d.shape[i] : 1;
  if (ndim_out) *ndim_out = (int)d.shape.size();
  return 0;
}

int vqvs_model_create(const vqvs_cfg* cfg, const float* const* h_params, int n_params, int device, vqvs_model** out) {
  if (!cfg || !h_params || !out) VQVS_FAIL(VQVS_ERR_ARG, "NULL argument");
  *out = nullptr;
  std::vector<ParamDef> p;
  if (int e = enumerate_params(*cfg, p)) return e;
  if (n_params != (int)p.size()) VQVS_FAIL(VQVS_ERR_ARG, "expected %d parameters, got %d", (int)p.size(), n_params);
  for (int i = 0; i < n_params; ++i)
    if (!h_params[i]) VQVS_FAIL(VQVS_ERR_ARG, "parameter %d (%s) is NULL", i, p[i].name.c_str());
  int ndev = 0;
  VQVS_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) VQVS_FAIL(VQVS_ERR_ARG, "device %d not present (%d visible)", device, ndev);
  VQVS_HIP(hipSetDevice(device));
  vqvs_model* m = new vqvs_model();
  m->cfg = *cfg;
  m->device = device;
  if (int e = build_model(m, h_params)) {
    vqvs_model_destroy(m);
    return e;
  }
  *out = m;
  return 0;
}

void vqvs_model_destroy(vqvs_model* m) {
  if (!m) return;
  for (auto e : m->events) (void)hipEventDestroy(e);
  if (m->d_weights) (void)hipFree(m->d_weights);
  if (m->d_arena) (void)hipFree(m->d_arena);
  delete m;
}

int64_t vqvs_model_device_bytes(const vqvs_model* m) { return m ? (int64_t)(m->weights_bytes + m->arena_bytes) : 0; }

static int check_run(vqvs_model* m, int kind, int B, int L) {
  if (!m) VQVS_FAIL(VQVS_ERR_ARG, "model is NULL");
  if (m->cfg.kind != kind) VQVS_FAIL(VQVS_ERR_STATE, "handle kind %d used as kind %d", m->cfg.kind, kind);
  if (B < 1 || B > m->cfg.max_batch) VQVS_FAIL(VQVS_ERR_ARG, "batch %d outside 1..%d", B, m->cfg.max_batch);
  if (L < 1 || L > m->cfg.max_T) VQVS_FAIL(VQVS_ERR_ARG, "length %d outside 1..%d", L, m->cfg.max_T);
  if (kind == VQVS_KIND_CLASSIFIER && (L % (2 * unet_rate(m->cfg))))  // (the stem halves the length after EVERY level: 2^levels, classifier.py:79-96)
    VQVS_FAIL(VQVS_ERR_ARG, "T=%d is not a multiple of the classifier downsample rate %d", L, 2 * unet_rate(m->cfg));
  if (kind != VQVS_KIND_RESBLOCK && kind != VQVS_KIND_MFCC_ENCODER && (L % unet_rate(m->cfg)))
    VQVS_FAIL(VQVS_ERR_ARG, "T=%d is not a multiple of the UNet downsample rate %d", L, unet_rate(m->cfg));
  if (kind == VQVS_KIND_RESBLOCK && m->cfg.rb_resize == RESIZE_AVG2 && (L % 2)) VQVS_FAIL(VQVS_ERR_ARG, "avg-pool resblock needs even L");
  return 0;
}

int vqvs_unet_forward(vqvs_model* m, const float* d_x, const float* d_ts, const float* d_cond, const int64_t* d_labels, float* d_out,
                      int B, int T, void* stream) {
  if (int e = check_run(m, VQVS_KIND_PREDICTOR, B, T)) return e;
  if (!d_x || !d_ts || !d_out) VQVS_FAIL(VQVS_ERR_ARG, "x, ts and out must be non-NULL");
  // reference unet.py:126-131
  if ((d_labels == nullptr) != (m->cfg.num_labels == 0)) VQVS_FAIL(VQVS_ERR_ARG, "must provide labels if and only if model is class conditional");
  if ((d_cond == nullptr) != (m->cfg.cond_channels == 0)) VQVS_FAIL(VQVS_ERR_ARG, "must provide cond sequence if and only if model is conditional");
  RunCtx c;
  c.B = B;
  c.Lbase = T;
  c.x = d_x;
  c.ts = d_ts;
  c.cond = d_cond;
  c.labels = d_labels;
  c.out = d_out;
  c.st = reinterpret_cast<hipStream_t>(stream);
  return run_model(m, c);
}

int vqvs_unet_forward_vec(vqvs_model* m, const float* d_x, const float* d_ts, const float* d_cond, const float* d_vec, float* d_out, int B,
                          int T, void* stream) {
  if (m && m->cfg.kind != VQVS_KIND_PREDICTOR) VQVS_FAIL(VQVS_ERR_ARG, "handle kind %d: an explicit vector needs a predictor handle", m->cfg.kind);
  if (int e = check_run(m, VQVS_KIND_PREDICTOR, B, T)) return e;
  if (m->cfg.num_labels <= 0) VQVS_FAIL(VQVS_ERR_ARG, "an explicit vector stands in for a class embedding: the model has no labels");
  if (!d_x || !d_ts || !d_vec || !d_out) VQVS_FAIL(VQVS_ERR_ARG, "x, ts, vec and out must be non-NULL");
  if ((d_cond == nullptr) != (m->cfg.cond_channels == 0)) VQVS_FAIL(VQVS_ERR_ARG, "must provide cond sequence if and only if model is conditional");
  RunCtx c;
  c.B = B;
  c.Lbase = T;
  c.x = d_x;
  c.ts = d_ts;
  c.cond = d_cond;
  c.class_vec = d_vec;  // (time_embed adds it where it adds class_embed[labels[b]]: the schedule is vqvs_unet_forward's otherwise)
  c.out = d_out;
  c.st = reinterpret_cast<hipStream_t>(stream);
  return run_model(m, c);
}

int vqvs_unet_embed_grad(vqvs_model* m, const float* d_x_t, const float* d_ts, const float* d_cond, const float* d_vec, const float* d_eps,
                         float* d_mse, float* d_grad, float* d_pred, int B, int T, void* stream) {
  if (int e = check_run(m, VQVS_KIND_PREDICTOR_GRAD, B, T)) return e;
  if (!d_x_t || !d_ts || !d_vec) VQVS_FAIL(VQVS_ERR_ARG, "x_t, ts and vec must be non-NULL");
  if ((d_cond == nullptr) != (m->cfg.cond_channels == 0)) VQVS_FAIL(VQVS_ERR_ARG, "must provide cond sequence if and only if model is conditional");
  if ((d_mse == nullptr) != (d_grad == nullptr)) VQVS_FAIL(VQVS_ERR_ARG, "mse and grad must be given together (both NULL: the forward alone)");
  const bool backward = d_grad != nullptr;
  if (backward && !d_eps) VQVS_FAIL(VQVS_ERR_ARG, "eps must be non-NULL when mse and grad are asked for");
  if (!backward && !d_pred) VQVS_FAIL(VQVS_ERR_ARG, "nothing to compute: mse, grad and pred are all NULL");
  RunCtx c;
  c.B = B;
  c.Lbase = T;
  c.x = d_x_t;
  c.ts = d_ts;
  c.cond = d_cond;
  c.class_vec = d_vec;
  c.eps = d_eps;
  c.mse = d_mse;
  c.egrad = d_grad;
  c.out = d_pred;
  c.backward = backward;
  c.st = reinterpret_cast<hipStream_t>(stream);
  return run_model(m, c);
}

int vqvs_embed_adamw(float* d_rows, float* d_m, float* d_v, const float* d_grad, const int64_t* d_row_of_clip, int n, int B, int E,
                     int step, float lr, float beta1, float beta2, float eps, float weight_decay, void* stream) {
  if (!d_rows || !d_m || !d_v || !d_grad || !d_row_of_clip) VQVS_FAIL(VQVS_ERR_ARG, "rows, m, v, grad and row_of_clip must be non-NULL");
  if (n < 1 || B < 1 || E < 1) VQVS_FAIL(VQVS_ERR_ARG, "bad shape n=%d B=%d E=%d", n, B, E);
  if (step < 1) VQVS_FAIL(VQVS_ERR_ARG, "step=%d: the count of this step starts at 1", step);
  if (!std::isfinite(lr) || lr < 0.f) VQVS_FAIL(VQVS_ERR_ARG, "lr=%g must be finite and not negative", (double)lr);
  if (!std::isfinite(eps) || eps < 0.f) VQVS_FAIL(VQVS_ERR_ARG, "eps=%g must be finite and not negative", (double)eps);
  if (!std::isfinite(weight_decay) || weight_decay < 0.f) VQVS_FAIL(VQVS_ERR_ARG, "weight_decay=%g must be finite and not negative", (double)weight_decay);
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) VQVS_FAIL(VQVS_ERR_ARG, "betas (%g, %g) must lie in [0, 1)", (double)beta1, (double)beta2);
  return run_embed_adamw(d_rows, d_m, d_v, d_grad, d_row_of_clip, n, B, E, step, lr, beta1, beta2, eps, weight_decay,
                         reinterpret_cast<hipStream_t>(stream));
}

int vqvs_head_xent_grad(const float* d_feat, const float* d_w_old, const float* d_b_old, const float* d_new, const int64_t* d_targets,
                        float* d_act, float* d_logits, double* d_nll, int64_t* d_top1, double* d_new_mass, double* d_coef, int B, int F,
                        int K, int n, void* stream) {
  if (!d_feat || !d_w_old || !d_b_old || !d_new || !d_targets || !d_nll || !d_coef)
    VQVS_FAIL(VQVS_ERR_ARG, "feat, w_old, b_old, new, targets, nll and coef must be non-NULL");
  if (B < 1 || B > 65535) VQVS_FAIL(VQVS_ERR_ARG, "batch %d outside 1..65535", B);
  if (F < 1 || F > 4096) VQVS_FAIL(VQVS_ERR_ARG, "feature width %d outside 1..4096", F);
  if (K < 1 || n < 1 || K > 8192 || n > 8192 || K + n > 8192) VQVS_FAIL(VQVS_ERR_ARG, "K=%d old and n=%d new labels: each at least 1, together at most 8192", K, n);
  return run_head_xent_grad(d_feat, d_w_old, d_b_old, d_new, d_targets, d_act, d_logits, d_nll, d_top1, d_new_mass, d_coef, B, F, K, n,
                            reinterpret_cast<hipStream_t>(stream));
}

int vqvs_head_adamw(float* d_new, float* d_m, float* d_v, const float* d_act, const double* d_coef, int n, int B, int F, int step,
                    float lr, float beta1, float beta2, float eps, float weight_decay, void* stream) {
  if (!d_new || !d_m || !d_v || !d_act || !d_coef) VQVS_FAIL(VQVS_ERR_ARG, "new, m, v, act and coef must be non-NULL");
  if (n < 1 || B < 1 || F < 1) VQVS_FAIL(VQVS_ERR_ARG, "bad shape n=%d B=%d F=%d", n, B, F);
  if (n > 8192 || B > 65535 || F > 4096) VQVS_FAIL(VQVS_ERR_ARG, "n=%d B=%d F=%d outside 1..8192, 1..65535, 1..4096", n, B, F);
  if (step < 1) VQVS_FAIL(VQVS_ERR_ARG, "step=%d: the count of this step starts at 1", step);
  if (!std::isfinite(lr) || lr < 0.f) VQVS_FAIL(VQVS_ERR_ARG, "lr=%g must be finite and not negative", (double)lr);
  if (!std::isfinite(eps) || eps < 0.f) VQVS_FAIL(VQVS_ERR_ARG, "eps=%g must be finite and not negative", (double)eps);
  if (!std::isfinite(weight_decay) || weight_decay < 0.f) VQVS_FAIL(VQVS_ERR_ARG, "weight_decay=%g must be finite and not negative", (double)weight_decay);
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) VQVS_FAIL(VQVS_ERR_ARG, "betas (%g, %g) must lie in [0, 1)", (double)beta1, (double)beta2);
  return run_head_adamw(d_new, d_m, d_v, d_act, d_coef, n, B, F, step, lr, beta1, beta2, eps, weight_decay,
                        reinterpret_cast<hipStream_t>(stream));
}

int vqvs_encoder_forward(vqvs_model* m, const float* d_x, float* d_z, int B, int T, void* stream) {
  if (int e = check_run(m, VQVS_KIND_ENCODER, B, T)) return e;
  if (!d_x || !d_z) VQVS_FAIL(VQVS_ERR_ARG, "x and z must be non-NULL");
  RunCtx c;
  c.B = B;
  c.Lbase = T;
  c.x = d_x;
  c.out = d_z;
  c.st = reinterpret_cast<hipStream_t>(stream);
  return run_model(m, c);
}

int vqvs_mfcc_encoder_forward(vqvs_model* m, const float* d_x, float* d_z, int B, int T, void* stream) {
  if (int e = check_run(m, VQVS_KIND_MFCC_ENCODER, B, T)) return e;
  if (!d_x || !d_z) VQVS_FAIL(VQVS_ERR_ARG, "x and z must be non-NULL");
  if (T < 800) VQVS_FAIL(VQVS_ERR_ARG, "T=%d is too short for the MFCC front end (needs at least 800 samples)", T);
  RunCtx c;
  c.B = B;
  c.Lbase = T;
  c.x = d_x;
  c.out = d_z;
  c.st = reinterpret_cast<hipStream_t>(stream);
  return run_model(m, c);
}

int vqvs_mfcc_encoder_forward_logmel(vqvs_model* m, const float* d_logmel, float* d_z, int B, int T, void* stream) {
  if (int e = check_run(m, VQVS_KIND_MFCC_ENCODER, B, T)) return e;
  if (!d_logmel || !d_z) VQVS_FAIL(VQVS_ERR_ARG, "logmel and z must be non-NULL");
  if (T < 800) VQVS_FAIL(VQVS_ERR_ARG, "T=%d is too short for the MFCC front end (needs at least 800 samples)", T);
  RunCtx c;
  c.B = B;
  c.Lbase = T;
  c.logmel = d_logmel;
  c.out = d_z;
  c.st = reinterpret_cast<hipStream_t>(stream);
  return run_model(m, c);
}

int vqvs_resblock_forward(vqvs_model* m, const float* d_x, const float* d_emb, float* d_y, int B, int L, void* stream) {
  if (int e = check_run(m, VQVS_KIND_RESBLOCK, B, L)) return e;
  if (!d_x || !d_y) VQVS_FAIL(VQVS_ERR_ARG, "x and y must be non-NULL");
  if ((d_emb == nullptr) != (m->cfg.rb_emb_channels == 0)) VQVS_FAIL(VQVS_ERR_ARG, "emb must be given iff the block has cond_layers");
  RunCtx c;
  c.B = B;
  c.Lbase = L;
  c.x = d_x;
  c.emb = d_emb;
  c.out = d_y;
  c.st = reinterpret_cast<hipStream_t>(stream);
  return run_model(m, c);
}

int vqvs_classifier_forward(vqvs_model* m, const float* d_x, const float* d_ts, float* d_logits, int B, int T, void* stream) {
  if (int e = check_run(m, VQVS_KIND_CLASSIFIER, B, T)) return e;
  if (!d_x || !d_ts || !d_logits) VQVS_FAIL(VQVS_ERR_ARG, "x, ts and logits must be non-NULL");
  RunCtx c;
  c.B = B;
  c.Lbase = T;
  c.x = d_x;
  c.ts = d_ts;
  c.out = d_logits;
  c.st = reinterpret_cast<hipStream_t>(stream);
  return run_model(m, c);
}

int vqvs_classifier_features(vqvs_model* m, const float* d_x, const float* d_ts, float* d_feat, float* d_logits, float* d_probs, int B,
                             int T, void* stream) {
  if (int e = check_run(m, VQVS_KIND_CLASSIFIER, B, T)) return e;
  if (!d_x || !d_ts || !d_feat) VQVS_FAIL(VQVS_ERR_ARG, "x, ts and feat must be non-NULL");
  RunCtx c;
  c.B = B;
  c.Lbase = T;
  c.x = d_x;
  c.ts = d_ts;
  c.out = d_logits;  // (NULL: the head does not store them)
  c.feat = d_feat;
  c.probs = d_probs;
  c.st = reinterpret_cast<hipStream_t>(stream);
  return run_model(m, c);  // (phase 0 only: c.backward stays false)
}

int vqvs_feature_moments(const float* d_feat, int B, int F, const float* d_shift, double* d_s1, double* d_s2, void* stream) {
  if (!d_feat || !d_shift || !d_s1 || !d_s2) VQVS_FAIL(VQVS_ERR_ARG, "feat, shift, s1 and s2 must be non-NULL");
  if (B < 1) VQVS_FAIL(VQVS_ERR_ARG, "batch %d must be at least 1", B);
  if (F < 1 || F > 8192) VQVS_FAIL(VQVS_ERR_ARG, "feature width %d outside 1..8192", F);
  return launch_feature_moments(d_feat, B, F, d_shift, d_s1, d_s2, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_classifier_guidance(vqvs_model* m, const float* d_x, const float* d_ts, const int64_t* d_labels, float scale, float* d_grad,
                             float* d_logits, int B, int T, void* stream) {
  if (int e = check_run(m, VQVS_KIND_CLASSIFIER, B, T)) return e;
  if (!d_x || !d_ts || !d_labels || !d_grad) VQVS_FAIL(VQVS_ERR_ARG, "x, ts, labels and grad must be non-NULL");
  float* logits = d_logits;
  ScratchLease lease;  // (held until run_model has enqueued every kernel)
  if (!logits) {
    if (int e = scratch_get((size_t)B * m->cfg.num_labels * 4, stream, lease)) return e;
    logits = reinterpret_cast<float*>(lease.p);
  }
  RunCtx c;
  c.B = B;
  c.Lbase = T;
  c.x = d_x;
  c.ts = d_ts;
  c.labels = d_labels;
  c.out = logits;
  c.backward = true;
  c.gscale = scale;
  c.grad_out = d_grad;
  c.st = reinterpret_cast<hipStream_t>(stream);
  return run_model(m, c);
}

int vqvs_encpred_forward(vqvs_model* m, const float* d_x, const float* d_ts, float* d_logits, int B, int T, void* stream) {
  if (int e = check_run(m, VQVS_KIND_ENCPRED, B, T)) return e;
  if (!d_x || !d_ts || !d_logits) VQVS_FAIL(VQVS_ERR_ARG, "x, ts and logits must be non-NULL");
  if (T % m->cfg.reserved[1]) VQVS_FAIL(VQVS_ERR_ARG, "T=%d is not a multiple of the downsample rate %d", T, m->cfg.reserved[1]);
  RunCtx c;
  c.B = B;
  c.Lbase = T;
  c.x = d_x;
  c.ts = d_ts;
  c.out = d_logits;
  c.st = reinterpret_cast<hipStream_t>(stream);
  return run_model(m, c);
}

int vqvs_encpred_guidance(vqvs_model* m, const float* d_x, const float* d_ts, const int64_t* d_targets, float scale, float* d_grad,
                          float* d_logits, int B, int T, void* stream) {
  if (int e = check_run(m, VQVS_KIND_ENCPRED, B, T)) return e;
  if (!d_x || !d_ts || !d_targets || !d_grad) VQVS_FAIL(VQVS_ERR_ARG, "x, ts, targets and grad must be non-NULL");
  if (T % m->cfg.reserved[1]) VQVS_FAIL(VQVS_ERR_ARG, "T=%d is not a multiple of the downsample rate %d", T, m->cfg.reserved[1]);
  RunCtx c;
  c.B = B;
  c.Lbase = T;
  c.x = d_x;
  c.ts = d_ts;
  c.labels = d_targets;  // the head reads them as targets; the UNet itself is label-free
  c.out = d_logits;
  c.backward = true;
  c.gscale = scale;
  c.grad_out = d_grad;
  c.st = reinterpret_cast<hipStream_t>(stream);
  return run_model(m, c);
}

// [a, a + na) against [b, b + nb) in bytes (NULL: absent)
static bool bytes_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
  return pa && pb && pa < pb + nb && pb < pa + na;
}
// No output may overlap an input or another output (a NULL array is absent).  The one exception: an output marked `history` -- the
// DPM-Solver++ x0_out -- may BE the input so marked -- x0_prev --, updated in place, though not overlap it in part.
struct Span {
  const char* name;
  const void* p;
  int64_t bytes;
  bool history = false;
};
static int check_disjoint(std::initializer_list<Span> outs, std::initializer_list<Span> ins) {
  for (const Span& out : outs) {
    for (const Span& in : ins)
      if (!(out.history && in.history && out.p == in.p) && bytes_overlap(out.p, out.bytes, in.p, in.bytes))
        VQVS_FAIL(VQVS_ERR_ARG, "%s must not overlap %s%s", out.name, in.name, out.history && in.history ? " in part (it may be it)" : "");
    for (const Span& other : outs)
      if (&other != &out && bytes_overlap(out.p, out.bytes, other.p, other.bytes))
        VQVS_FAIL(VQVS_ERR_ARG, "%s must not overlap %s", out.name, other.name);
  }
  return 0;
}

// The window geometry of the ..._windows entry points: n windows of W samples, one every H, span *Np = (n - 1) * H + W.
static int check_window_geometry(int n, int W, int H, int64_t* Np) {
  if (n < 1 || n > 65535) VQVS_FAIL(VQVS_ERR_ARG, "window count n=%d outside 1..65535", n);
  if (W < 4 || H < 4 || W % 4 || H % 4) VQVS_FAIL(VQVS_ERR_ARG, "window W=%d and hop H=%d must be positive multiples of 4", W, H);
  if (W < H || W - H > H) VQVS_FAIL(VQVS_ERR_ARG, "overlap %d (window W=%d - hop H=%d) outside 0..hop: at most two windows may cover a sample", W - H, W, H);
  *Np = (int64_t)(n - 1) * H + W;
  if (*Np >= ((int64_t)1 << 31)) VQVS_FAIL(VQVS_ERR_ARG, "n=%d windows every H=%d samples span %lld samples: 2^31 or more", n, H, (long long)*Np);
  return 0;
}
// The geometry of the three ..._windows_packed entry points: R recordings in windows of W every H.  The window total is on the device;
// *least = R * W is what every array of such a pack holds at the least, the extent the aliasing rules are checked over.
static int check_pack_geometry(const int32_t* d_first, int R, int W, int H, int64_t* least) {
  if (R < 1 || R > 65535) VQVS_FAIL(VQVS_ERR_ARG, "recording count R=%d outside 1..65535", R);
  if (!d_first) VQVS_FAIL(VQVS_ERR_ARG, "first must be non-NULL");
  int64_t Np;
  if (int e = check_window_geometry(1, W, H, &Np)) return e;
  *least = (int64_t)R * W;
  return 0;
}
// the x0-sum partials of a CONSTRAIN step over `rows` clips / windows of `len` samples; nothing is leased without the flag
static int lease_x0sum(bool constrain, int rows, int len, void* stream, ScratchLease& lease) {
  return constrain ? scratch_get((size_t)ddpm_scratch_doubles(rows, len) * 8, stream, lease) : 0;
}
static int lease_x0sum_packed(bool constrain, int W, int H, void* stream, ScratchLease& lease) {
  return constrain ? scratch_get(packed_scratch_doubles(W, H) * 8, stream, lease) : 0;
}

// argument rules of the DDIM step
static int check_ddim_args(uint32_t flags, float eta) {
  if (!std::isfinite(eta) || eta < 0.f) VQVS_FAIL(VQVS_ERR_ARG, "eta %g must be finite and not negative", (double)eta);
  if (flags & ~(VQVS_DDIM_CONSTRAIN | VQVS_DDIM_INVERT))
    VQVS_FAIL(VQVS_ERR_ARG, "flags %#x: only VQVS_DDIM_CONSTRAIN and VQVS_DDIM_INVERT are defined for the DDIM step", flags);
  if ((flags & VQVS_DDIM_INVERT) && (flags & VQVS_DDIM_CONSTRAIN)) VQVS_FAIL(VQVS_ERR_ARG, "INVERT cannot be combined with CONSTRAIN");
  if ((flags & VQVS_DDIM_INVERT) && eta != 0.f) VQVS_FAIL(VQVS_ERR_ARG, "INVERT needs eta = 0 (got %g)", (double)eta);
  return 0;
}

// What the nine step entry points share once each has filled a StepArgs and a StepLayout by name (designated initialisers, in the
// order of the members): required pointers, the layout's geometry, the rule's own
// argument rules, aliasing, the scratch of CONSTRAIN, the launch.  Aliasing is checked over what every array holds at the least:
// long arrays (x, noise, x_to, the history) and window arrays (eps, grad, windows) are both B * T on clips and R * W on a pack.  The
// DDPM step has always checked less than the others -- nothing on clips, where x_prev may be x_t itself, and x_prev against x alone
// under windows -- and takes any flag word and, on clips, any positive B and T; callers rely on it.
static int step(StepRule rule, StepArgs a, const StepLayout& l, void* stream) {
  const bool ddpm = rule == StepRule::DDPM;
  const char* to = ddpm ? "x_prev" : "x_to";
  if (!a.x || !a.eps || !a.a_t || !a.a_to || !a.x_to) VQVS_FAIL(VQVS_ERR_ARG, "x, eps, alpha_t, alpha_%s and %s must be non-NULL", ddpm ? "prev" : "to", to);
  int64_t n_long = 0, n_win = 0, n_alpha = 1;
  switch (l.kind) {
    case StepLayout::CLIPS:
      if (ddpm && (l.n < 1 || l.W < 1)) VQVS_FAIL(VQVS_ERR_ARG, "bad shape B=%d T=%d", l.n, l.W);
      if (!ddpm && (l.n < 1 || l.n > 65535)) VQVS_FAIL(VQVS_ERR_ARG, "batch %d outside 1..65535", l.n);
      if (!ddpm && (l.W < 1 || l.W > (1 << 30))) VQVS_FAIL(VQVS_ERR_ARG, "row length %d outside 1..2^30", l.W);
      n_long = n_win = (int64_t)l.n * l.W;
      n_alpha = l.n;
      break;
    case StepLayout::WINDOWS:
      if (int e = check_window_geometry(l.n, l.W, l.H, &n_long)) return e;
      n_win = (int64_t)l.n * l.W;
      break;
    case StepLayout::PACK:
      if (int e = check_pack_geometry(l.first, l.n, l.W, l.H, &n_long)) return e;
      n_win = n_long;
      break;
  }
  if (rule == StepRule::DDIM)
    if (int e = check_ddim_args(a.flags, a.eta)) return e;
  if (rule == StepRule::DPMPP && (a.flags & ~VQVS_DDIM_CONSTRAIN))
    VQVS_FAIL(VQVS_ERR_ARG, "flags %#x: only VQVS_DDIM_CONSTRAIN is defined for the DPM-Solver++ step", a.flags);
  const Span x{"x", a.x, n_long * 4}, eps{"eps", a.eps, n_win * 4}, grad{"grad", a.grad, n_win * 4}, noise{"noise", a.noise, n_long * 4},
      x0_prev{"x0_prev", a.x0_prev, n_long * 4, true}, a_from{"alpha_from", a.a_from, n_alpha * 4}, a_t{"alpha_t", a.a_t, n_alpha * 4},
      a_to{"alpha_to", a.a_to, n_alpha * 4}, first{"first", l.kind == StepLayout::PACK ? l.first : nullptr, ((int64_t)l.n + 1) * 4},
      x_to{to, a.x_to, n_long * 4}, x0_out{"x0_out", a.x0_out, n_long * 4, true}, win{"windows", a.win, n_win * 4};
  if (ddpm) {
    if (l.kind != StepLayout::CLIPS)
      if (int e = check_disjoint({x_to}, {x})) return e;
  } else if (int e = check_disjoint({x0_out, x_to, win}, {x0_prev, x, eps, grad, noise, a_from, a_t, a_to, first})) {
    return e;
  }
  ScratchLease lease;
  const bool constrain = a.flags & VQVS_DDPM_CONSTRAIN;  // (VQVS_DDIM_CONSTRAIN is the same bit)
  if (int e = l.kind == StepLayout::PACK ? lease_x0sum_packed(constrain, l.W, l.H, stream, lease) : lease_x0sum(constrain, l.n, l.W, stream, lease))
    return e;
  a.partial = reinterpret_cast<double*>(lease.p);
  return run_step(rule, a, l, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_ddpm_step(const float* d_x_t, const float* d_eps, const float* d_noise, const float* d_alpha_t, const float* d_alpha_prev,
                   float* d_x_prev, int B, int T, uint32_t flags, float noise_scale, uint64_t seed, uint64_t clip_offset,
                   uint32_t step_index, void* stream) {
  return step(StepRule::DDPM,
              {.x = d_x_t, .eps = d_eps, .noise = d_noise, .a_t = d_alpha_t, .a_to = d_alpha_prev, .x_to = d_x_prev, .flags = flags,
               .noise_scale = noise_scale, .seed = seed, .clip = clip_offset, .step_index = step_index},
              {StepLayout::CLIPS, B, T, 0, nullptr}, stream);
}

int vqvs_ddpm_step_windows(const float* d_x, const float* d_eps, const float* d_noise, const float* d_alpha_t, const float* d_alpha_prev,
                           float* d_x_prev, float* d_windows, int n, int W, int H, uint32_t flags, float noise_scale, uint64_t seed,
                           uint64_t clip, uint32_t step_index, void* stream) {
  return step(StepRule::DDPM,
              {.x = d_x, .eps = d_eps, .noise = d_noise, .a_t = d_alpha_t, .a_to = d_alpha_prev, .x_to = d_x_prev, .win = d_windows,
               .flags = flags, .noise_scale = noise_scale, .seed = seed, .clip = clip, .step_index = step_index},
              {StepLayout::WINDOWS, n, W, H, nullptr}, stream);
}

int vqvs_ddpm_step_windows_packed(const float* d_x, const float* d_eps, const float* d_noise, const float* d_alpha_t,
                                  const float* d_alpha_prev, float* d_x_prev, float* d_windows, const int32_t* d_first, int R, int W, int H,
                                  uint32_t flags, float noise_scale, uint64_t seed, uint64_t clip, uint32_t step_index, void* stream) {
  return step(StepRule::DDPM,
              {.x = d_x, .eps = d_eps, .noise = d_noise, .a_t = d_alpha_t, .a_to = d_alpha_prev, .x_to = d_x_prev, .win = d_windows,
               .flags = flags, .noise_scale = noise_scale, .seed = seed, .clip = clip, .step_index = step_index},
              {StepLayout::PACK, R, W, H, d_first}, stream);
}

int vqvs_ddim_step(const float* d_x_t, const float* d_eps, const float* d_grad, const float* d_noise, const float* d_alpha_t,
                   const float* d_alpha_to, float* d_x_to, int B, int T, uint32_t flags, float eta, float noise_scale, uint64_t seed,
                   uint64_t clip_offset, uint32_t step_index, void* stream) {
  return step(StepRule::DDIM,
              {.x = d_x_t, .eps = d_eps, .grad = d_grad, .noise = d_noise, .a_t = d_alpha_t, .a_to = d_alpha_to, .x_to = d_x_to, .flags = flags,
               .eta = eta, .noise_scale = noise_scale, .seed = seed, .clip = clip_offset, .step_index = step_index},
              {StepLayout::CLIPS, B, T, 0, nullptr}, stream);
}

int vqvs_ddim_step_windows(const float* d_x, const float* d_eps, const float* d_grad, const float* d_noise, const float* d_alpha_t,
                           const float* d_alpha_to, float* d_x_to, float* d_windows, int n, int W, int H, uint32_t flags, float eta,
                           float noise_scale, uint64_t seed, uint64_t clip, uint32_t step_index, void* stream) {
  return step(StepRule::DDIM,
              {.x = d_x, .eps = d_eps, .grad = d_grad, .noise = d_noise, .a_t = d_alpha_t, .a_to = d_alpha_to, .x_to = d_x_to, .win = d_windows,
               .flags = flags, .eta = eta, .noise_scale = noise_scale, .seed = seed, .clip = clip, .step_index = step_index},
              {StepLayout::WINDOWS, n, W, H, nullptr}, stream);
}

int vqvs_ddim_step_windows_packed(const float* d_x, const float* d_eps, const float* d_grad, const float* d_noise, const float* d_alpha_t,
                                  const float* d_alpha_to, float* d_x_to, float* d_windows, const int32_t* d_first, int R, int W, int H,
                                  uint32_t flags, float eta, float noise_scale, uint64_t seed, uint64_t clip, uint32_t step_index,
                                  void* stream) {
  return step(StepRule::DDIM,
              {.x = d_x, .eps = d_eps, .grad = d_grad, .noise = d_noise, .a_t = d_alpha_t, .a_to = d_alpha_to, .x_to = d_x_to, .win = d_windows,
               .flags = flags, .eta = eta, .noise_scale = noise_scale, .seed = seed, .clip = clip, .step_index = step_index},
              {StepLayout::PACK, R, W, H, d_first}, stream);
}

int vqvs_dpmpp_step(const float* d_x_t, const float* d_eps, const float* d_grad, const float* d_x0_prev, const float* d_alpha_from,
                    const float* d_alpha_t, const float* d_alpha_to, float* d_x_to, float* d_x0_out, int B, int T, uint32_t flags,
                    void* stream) {
  return step(StepRule::DPMPP,
              {.x = d_x_t, .eps = d_eps, .grad = d_grad, .x0_prev = d_x0_prev, .a_from = d_alpha_from, .a_t = d_alpha_t, .a_to = d_alpha_to,
               .x_to = d_x_to, .x0_out = d_x0_out, .flags = flags},
              {StepLayout::CLIPS, B, T, 0, nullptr}, stream);
}

int vqvs_dpmpp_step_windows(const float* d_x, const float* d_eps, const float* d_grad, const float* d_x0_prev, const float* d_alpha_from,
                            const float* d_alpha_t, const float* d_alpha_to, float* d_x_to, float* d_x0_out, float* d_windows, int n, int W,
                            int H, uint32_t flags, void* stream) {
  return step(StepRule::DPMPP,
              {.x = d_x, .eps = d_eps, .grad = d_grad, .x0_prev = d_x0_prev, .a_from = d_alpha_from, .a_t = d_alpha_t, .a_to = d_alpha_to,
               .x_to = d_x_to, .x0_out = d_x0_out, .win = d_windows, .flags = flags},
              {StepLayout::WINDOWS, n, W, H, nullptr}, stream);
}

int vqvs_dpmpp_step_windows_packed(const float* d_x, const float* d_eps, const float* d_grad, const float* d_x0_prev,
                                   const float* d_alpha_from, const float* d_alpha_t, const float* d_alpha_to, float* d_x_to,
                                   float* d_x0_out, float* d_windows, const int32_t* d_first, int R, int W, int H, uint32_t flags,
                                   void* stream) {
  return step(StepRule::DPMPP,
              {.x = d_x, .eps = d_eps, .grad = d_grad, .x0_prev = d_x0_prev, .a_from = d_alpha_from, .a_t = d_alpha_t, .a_to = d_alpha_to,
               .x_to = d_x_to, .x0_out = d_x0_out, .win = d_windows, .flags = flags},
              {StepLayout::PACK, R, W, H, d_first}, stream);
}

// Shared argument rules of the two keep-region entry points.  N: samples of the state (and of x0, keep, noise); n_alpha: entries of
// d_alpha; NW: samples of d_windows (0 when the entry point has none).
static int check_keep_args(const float* d_x, const float* d_windows, const float* d_x0, const uint8_t* d_keep, const float* d_noise,
                           const float* d_alpha, int64_t N, int64_t n_alpha, int64_t NW, float noise_scale) {
  if (!std::isfinite(noise_scale)) VQVS_FAIL(VQVS_ERR_ARG, "noise_scale %g must be finite", (double)noise_scale);
  return check_disjoint({{"d_x", d_x, N * 4}, {"d_windows", d_windows, NW * 4}},
                        {{"d_x0", d_x0, N * 4}, {"d_keep", d_keep, N}, {"d_noise", d_noise, N * 4}, {"d_alpha", d_alpha, n_alpha * 4}});
}

int vqvs_keep_region(float* d_x, const float* d_x0, const uint8_t* d_keep, const float* d_noise, const float* d_alpha, int B, int T,
                     float noise_scale, uint64_t seed, uint64_t clip_offset, uint32_t index, void* stream) {
  if (!d_x) VQVS_FAIL(VQVS_ERR_ARG, "d_x must be non-NULL");
  if (!d_x0) VQVS_FAIL(VQVS_ERR_ARG, "d_x0 must be non-NULL");
  if (!d_alpha) VQVS_FAIL(VQVS_ERR_ARG, "d_alpha must be non-NULL");
  if (B < 1 || B > 65535) VQVS_FAIL(VQVS_ERR_ARG, "batch B=%d outside 1..65535", B);
  if (T < 1 || T > (1 << 30)) VQVS_FAIL(VQVS_ERR_ARG, "row length T=%d outside 1..2^30", T);
  if (int e = check_keep_args(d_x, nullptr, d_x0, d_keep, d_noise, d_alpha, (int64_t)B * T, B, 0, noise_scale)) return e;
  return run_keep_region(d_x, d_x0, d_keep, d_noise, d_alpha, B, T, noise_scale, seed, clip_offset, index, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_keep_region_windows(float* d_x, float* d_windows, const float* d_x0, const uint8_t* d_keep, const float* d_noise,
                             const float* d_alpha, int n, int W, int H, float noise_scale, uint64_t seed, uint64_t clip, uint32_t index,
                             void* stream) {
  if (!d_x) VQVS_FAIL(VQVS_ERR_ARG, "d_x must be non-NULL");
  if (!d_x0) VQVS_FAIL(VQVS_ERR_ARG, "d_x0 must be non-NULL");
  if (!d_alpha) VQVS_FAIL(VQVS_ERR_ARG, "d_alpha must be non-NULL");
  int64_t Np;
  if (int e = check_window_geometry(n, W, H, &Np)) return e;
  if (int e = check_keep_args(d_x, d_windows, d_x0, d_keep, d_noise, d_alpha, Np, 1, (int64_t)n * W, noise_scale)) return e;
  return run_keep_region_windows(d_x, d_windows, d_x0, d_keep, d_noise, d_alpha, n, W, H, noise_scale, seed, clip, index,
                                 reinterpret_cast<hipStream_t>(stream));
}

int vqvs_keep_region_windows_packed(float* d_x, float* d_windows, const float* d_x0, const uint8_t* d_keep, const float* d_noise,
                                    const float* d_alpha, const int32_t* d_first, int R, int W, int H, float noise_scale, uint64_t seed,
                                    uint64_t clip, uint32_t index, void* stream) {
  if (!d_x) VQVS_FAIL(VQVS_ERR_ARG, "d_x must be non-NULL");
  if (!d_x0) VQVS_FAIL(VQVS_ERR_ARG, "d_x0 must be non-NULL");
  if (!d_alpha) VQVS_FAIL(VQVS_ERR_ARG, "d_alpha must be non-NULL");
  int64_t least;
  if (int e = check_pack_geometry(d_first, R, W, H, &least)) return e;
  if (int e = check_keep_args(d_x, d_windows, d_x0, d_keep, d_noise, d_alpha, least, 1, least, noise_scale)) return e;
  if (int e = check_disjoint({{"d_x", d_x, least * 4}, {"d_windows", d_windows, least * 4}}, {{"d_first", d_first, ((int64_t)R + 1) * 4}})) return e;
  return run_keep_region_packed(d_x, d_windows, d_x0, d_keep, d_noise, d_alpha, d_first, R, W, H, noise_scale, seed, clip, index,
                                reinterpret_cast<hipStream_t>(stream));
}

int vqvs_pause_mask(const float* d_x, uint8_t* d_keep, int64_t* d_counts, const int32_t* d_first, int R, int W, int H, int frame,
                    int64_t thr, int min_frames, int guard_frames, void* stream) {
  if (!d_x) VQVS_FAIL(VQVS_ERR_ARG, "d_x must be non-NULL");
  if (!d_keep) VQVS_FAIL(VQVS_ERR_ARG, "d_keep must be non-NULL");
  int64_t least;
  if (int e = check_pack_geometry(d_first, R, W, H, &least)) return e;
  if (frame < 4 || frame > 4096 || frame % 4) VQVS_FAIL(VQVS_ERR_ARG, "frame=%d must be a multiple of 4 in 4..4096", frame);
  if (thr < 0 || thr > ((int64_t)1 << 30)) VQVS_FAIL(VQVS_ERR_ARG, "thr=%lld outside 0..2^30", (long long)thr);
  if (min_frames < 1 || min_frames > (1 << 20)) VQVS_FAIL(VQVS_ERR_ARG, "min_frames=%d outside 1..2^20", min_frames);
  if (guard_frames < 0 || guard_frames > (1 << 20)) VQVS_FAIL(VQVS_ERR_ARG, "guard_frames=%d outside 0..2^20", guard_frames);
  if (int e = check_disjoint({{"d_keep", d_keep, least}, {"d_counts", d_counts, (int64_t)R * 16}},
                             {{"d_x", d_x, least * 4}, {"d_first", d_first, ((int64_t)R + 1) * 4}}))
    return e;
  ScratchLease lease;
  if (int e = scratch_get(pause_mask_scratch_bytes(R, W, H, frame), stream, lease)) return e;
  return run_pause_mask(d_x, d_keep, reinterpret_cast<long long*>(d_counts), d_first, lease.p, R, W, H, frame, (long long)thr, min_frames,
                        guard_frames, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_windows_kept(const uint8_t* d_keep, uint8_t* d_out, const int32_t* d_first, int R, int W, int H, void* stream) {
  if (!d_keep) VQVS_FAIL(VQVS_ERR_ARG, "d_keep must be non-NULL");
  if (!d_out) VQVS_FAIL(VQVS_ERR_ARG, "d_out must be non-NULL");
  int64_t least;
  if (int e = check_pack_geometry(d_first, R, W, H, &least)) return e;
  if (int e = check_disjoint({{"d_out", d_out, R}}, {{"d_keep", d_keep, least}, {"d_first", d_first, ((int64_t)R + 1) * 4}})) return e;
  return run_windows_kept(d_keep, d_out, d_first, R, W, H, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_ddpm_mean(const float* d_x_t, const float* d_eps, const float* d_alpha_t, const float* d_alpha_prev, float* d_mean, int B, int T,
                   void* stream) {
  if (!d_x_t || !d_eps || !d_alpha_t || !d_alpha_prev || !d_mean) VQVS_FAIL(VQVS_ERR_ARG, "NULL argument");
  return run_ddpm_mean(d_x_t, d_eps, d_alpha_t, d_alpha_prev, d_mean, B, T, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_ddpm_guided_eps(const float* d_x_t, const float* d_mean, const float* d_grad, const float* d_alpha_t, const float* d_alpha_prev,
                         float* d_eps_out, int B, int T, uint32_t flags, void* stream) {
  if (!d_x_t || !d_mean || !d_grad || !d_alpha_t || !d_alpha_prev || !d_eps_out) VQVS_FAIL(VQVS_ERR_ARG, "NULL argument");
  return run_ddpm_guided_eps(d_x_t, d_mean, d_grad, d_alpha_t, d_alpha_prev, d_eps_out, B, T, flags, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_guidance_mix(const float* d_outs, float* d_eps, int rows, int64_t row_len, int reps, float s1, float s2, void* stream) {
  if (!d_outs || !d_eps) VQVS_FAIL(VQVS_ERR_ARG, "d_outs and d_eps must be non-NULL");
  if (rows < 1) VQVS_FAIL(VQVS_ERR_ARG, "rows=%d must be at least 1", rows);
  if (row_len < 1) VQVS_FAIL(VQVS_ERR_ARG, "row_len=%lld must be at least 1", (long long)row_len);
  if (reps < 1 || reps > 3) VQVS_FAIL(VQVS_ERR_ARG, "reps=%d outside 1..3", reps);
  if (row_len > (INT64_MAX / 16) / rows) VQVS_FAIL(VQVS_ERR_ARG, "rows=%d of row_len=%lld: too many elements", rows, (long long)row_len);
  const int64_t total = (int64_t)rows * row_len;
  // in place means eps IS block 0: element i is read and written by the same thread.  Any other overlap -- blocks 1 and 2, or block 0
  // at an offset -- would let one thread's store reach another's load.
  if (d_eps != d_outs && bytes_overlap(d_eps, total * 4, d_outs, (int64_t)reps * total * 4))
    VQVS_FAIL(VQVS_ERR_ARG, "d_eps must be d_outs itself (in place over block 0) or not overlap d_outs at all");
  return run_guidance_mix(d_outs, d_eps, total, reps, s1, s2, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_speaker_mix(const float* d_table, int K, int E, const int32_t* d_idx, const float* d_w, int J, float* d_out, int B, void* stream) {
  if (!d_table || !d_idx || !d_w || !d_out) VQVS_FAIL(VQVS_ERR_ARG, "d_table, d_idx, d_w and d_out must be non-NULL");
  if (K < 1 || E < 1 || B < 1) VQVS_FAIL(VQVS_ERR_ARG, "bad shape K=%d E=%d B=%d", K, E, B);
  if (J < 1 || J > 16) VQVS_FAIL(VQVS_ERR_ARG, "J=%d outside 1..16", J);
  const int64_t out_bytes = (int64_t)B * E * 4, slot_bytes = (int64_t)B * J * 4;
  if (int e = check_disjoint({{"d_out", d_out, out_bytes}}, {{"d_table", d_table, (int64_t)K * E * 4}, {"d_idx", d_idx, slot_bytes}, {"d_w", d_w, slot_bytes}}))
    return e;
  return run_speaker_mix(d_table, K, E, d_idx, d_w, J, d_out, B, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_randn(float* d_out, int B, int T, uint64_t seed, uint64_t clip_offset, uint32_t stream_id, void* stream) {
  if (!d_out || B < 1 || T < 1) VQVS_FAIL(VQVS_ERR_ARG, "bad argument");
  return run_randn(d_out, B, T, seed, clip_offset, stream_id, reinterpret_cast<hipStream_t>(stream));
}

// shared argument rules of the two forward-process entry points: B rows of T samples, noise given as 1 or B rows or generated
static int check_noise_args(const float* d_eps, int eps_rows, int B, int T) {
  if (B < 1 || B > 65535) VQVS_FAIL(VQVS_ERR_ARG, "batch %d outside 1..65535", B);
  if (T < 1 || T > (1 << 30)) VQVS_FAIL(VQVS_ERR_ARG, "row length %d outside 1..2^30", T);
  if (d_eps && eps_rows != 1 && eps_rows != B) VQVS_FAIL(VQVS_ERR_ARG, "eps_rows %d must be 1 or the batch %d", eps_rows, B);
  if (!d_eps && eps_rows != 0 && eps_rows != 1 && eps_rows != B)
    VQVS_FAIL(VQVS_ERR_ARG, "eps_rows %d must be 0, 1 or the batch %d when the noise is generated", eps_rows, B);
  return 0;
}

int vqvs_ddpm_noise(const float* d_x0, int x0_rows, const float* d_alpha, const float* d_eps, int eps_rows, const int64_t* d_noise_index,
                    float* d_x_t, int B, int T, uint64_t seed, uint64_t clip_offset, void* stream) {
  if (!d_x0 || !d_alpha || !d_x_t) VQVS_FAIL(VQVS_ERR_ARG, "x0, alpha and x_t must be non-NULL");
  if (int e = check_noise_args(d_eps, eps_rows, B, T)) return e;
  if (x0_rows != 1 && x0_rows != B) VQVS_FAIL(VQVS_ERR_ARG, "x0_rows %d must be 1 or the batch %d", x0_rows, B);
  return run_ddpm_noise(d_x0, x0_rows, d_alpha, d_eps, eps_rows, d_noise_index, d_x_t, B, T, seed, clip_offset,
                        reinterpret_cast<hipStream_t>(stream));
}

int vqvs_ddpm_sqerr(const float* d_pred, const float* d_eps, int eps_rows, const int64_t* d_noise_index, float* d_loss, int B, int T,
                    uint64_t seed, uint64_t clip_offset, void* stream) {
  if (!d_pred || !d_loss) VQVS_FAIL(VQVS_ERR_ARG, "pred and loss must be non-NULL");
  if (int e = check_noise_args(d_eps, eps_rows, B, T)) return e;
  ScratchLease lease;
  if (int e = scratch_get((size_t)sqerr_scratch_doubles(B, T) * 8, stream, lease)) return e;
  return run_ddpm_sqerr(d_pred, d_eps, eps_rows, d_noise_index, d_loss, reinterpret_cast<double*>(lease.p), B, T, seed, clip_offset,
                        reinterpret_cast<hipStream_t>(stream));
}

int vqvs_vq_argmin(const float* d_z, const float* d_dict, int64_t* d_idx, int B, int Cd, int T1, int K, void* stream) {
  if (!d_z || !d_dict || !d_idx) VQVS_FAIL(VQVS_ERR_ARG, "NULL argument");
  if (B < 1 || Cd < 1 || T1 < 1 || K < 1) VQVS_FAIL(VQVS_ERR_ARG, "bad shape B=%d Cd=%d T1=%d K=%d", B, Cd, T1, K);
  if (B > 65535) VQVS_FAIL(VQVS_ERR_ARG, "batch %d outside 1..65535", B);
  if (Cd % 4) VQVS_FAIL(VQVS_ERR_ARG, "Cd must be a multiple of 4 (got %d)", Cd);
  ScratchLease lease;
  if (int e = scratch_get((size_t)K * 4, stream, lease)) return e;
  return run_vq_argmin(d_z, d_dict, reinterpret_cast<float*>(lease.p), d_idx, B, Cd, T1, K, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_vq_quantize(const float* d_z, const float* d_dict, int64_t* d_idx, float* d_embedded, double* d_sqerr, int64_t* d_hist, int B,
                     int Cd, int T1, int K, void* stream) {
  if (!d_z || !d_dict || !d_idx) VQVS_FAIL(VQVS_ERR_ARG, "z, dict and idx must be non-NULL");
  if (B < 1 || Cd < 1 || T1 < 1 || K < 1) VQVS_FAIL(VQVS_ERR_ARG, "bad shape B=%d Cd=%d T1=%d K=%d", B, Cd, T1, K);
  if (B > 65535) VQVS_FAIL(VQVS_ERR_ARG, "batch %d outside 1..65535", B);
  if (Cd % 4) VQVS_FAIL(VQVS_ERR_ARG, "Cd must be a multiple of 4 (got %d)", Cd);
  ScratchLease lease;
  if (int e = scratch_get(vq_quantize_scratch_bytes(B, T1, K), stream, lease)) return e;
  return run_vq_quantize(d_z, d_dict, lease.p, d_idx, d_embedded, d_sqerr, d_hist, B, Cd, T1, K, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_xent_score(const float* d_logits, const int64_t* d_targets, double* d_nll, int64_t* d_top1, int64_t* d_topk, int k,
                    int64_t* d_confusion, int B, int K, int L, void* stream) {
  if (!d_logits || !d_targets || !d_nll) VQVS_FAIL(VQVS_ERR_ARG, "logits, targets and nll must be non-NULL");
  if (B < 1 || B > 65535) VQVS_FAIL(VQVS_ERR_ARG, "batch %d outside 1..65535", B);
  if (K < 1 || K > 8192) VQVS_FAIL(VQVS_ERR_ARG, "class count %d outside 1..8192", K);
  if (L < 1 || L > (1 << 24)) VQVS_FAIL(VQVS_ERR_ARG, "positions per clip %d outside 1..2^24", L);
  if (d_topk && (k < 1 || k > K)) VQVS_FAIL(VQVS_ERR_ARG, "k=%d outside 1..%d", k, K);
  ScratchLease lease;
  if (L > 1)
    if (int e = scratch_get(xent_score_scratch_bytes(B, L), stream, lease)) return e;
  return run_xent_score(d_logits, d_targets, lease.p, d_nll, d_top1, d_topk, d_topk ? k : 0, d_confusion, B, K, L,
                        reinterpret_cast<hipStream_t>(stream));
}

int vqvs_spectral_distance(const float* d_a, const float* d_b, const float* d_window, const double* d_twiddle, const float* d_fb,
                           const float* d_dct, double* d_mcd, double* d_lsd, int B, int T, int n_fft, int hop, int n_mels, int n_ceps,
                           float eps, void* stream) {
  if (!d_a || !d_b || !d_window || !d_twiddle || !d_fb || !d_dct) VQVS_FAIL(VQVS_ERR_ARG, "a, b, window, twiddle, fb and dct must be non-NULL");
  if (!d_mcd && !d_lsd) VQVS_FAIL(VQVS_ERR_ARG, "mcd and lsd are both NULL: nothing to compute");
  if (B < 1 || B > 65535) VQVS_FAIL(VQVS_ERR_ARG, "batch %d outside 1..65535", B);
  if (n_fft < 16 || n_fft > 512 || n_fft % 2) VQVS_FAIL(VQVS_ERR_ARG, "n_fft=%d must be even and in 16..512", n_fft);
  if (T <= n_fft / 2) VQVS_FAIL(VQVS_ERR_ARG, "clip of %d samples is no longer than the reflect padding (%d)", T, n_fft / 2);
  if (T > (1 << 30)) VQVS_FAIL(VQVS_ERR_ARG, "clip of %d samples: more than 2^30", T);
  if (hop < 1 || hop > n_fft) VQVS_FAIL(VQVS_ERR_ARG, "hop=%d outside 1..n_fft=%d", hop, n_fft);
  if (T / hop + 1 > (1 << 25)) VQVS_FAIL(VQVS_ERR_ARG, "T=%d at hop=%d is more than 2^25 frames per clip", T, hop);
  if (n_mels < 1 || n_mels > 128) VQVS_FAIL(VQVS_ERR_ARG, "n_mels=%d outside 1..128", n_mels);
  if (n_ceps < 2 || n_ceps > (n_mels < 64 ? n_mels : 64)) VQVS_FAIL(VQVS_ERR_ARG, "n_ceps=%d outside 2..min(n_mels=%d, 64)", n_ceps, n_mels);
  if (!std::isfinite(eps) || !(eps > 0.f)) VQVS_FAIL(VQVS_ERR_ARG, "eps=%g must be finite and positive", (double)eps);
  const int64_t N = (int64_t)B * T;
  if (int e = check_disjoint({{"mcd", d_mcd, (int64_t)B * 8}, {"lsd", d_lsd, (int64_t)B * 8}},
                             {{"a", d_a, N * 4}, {"b", d_b, N * 4}, {"window", d_window, (int64_t)n_fft * 4}, {"twiddle", d_twiddle, (int64_t)n_fft * 16},
                              {"fb", d_fb, (int64_t)(n_fft / 2 + 1) * n_mels * 4}, {"dct", d_dct, (int64_t)n_mels * n_ceps * 4}}))
    return e;
  ScratchLease lease;
  if (int e = scratch_get(spectral_distance_scratch_bytes(B, T, hop), stream, lease)) return e;
  return run_spectral_distance(d_a, d_b, d_window, d_twiddle, d_fb, d_dct, lease.p, d_mcd, d_lsd, B, T, n_fft, hop, n_mels, n_ceps, eps,
                               reinterpret_cast<hipStream_t>(stream));
}

int vqvs_mel_cepstra(const float* d_x, const int* d_len, const float* d_window, const double* d_twiddle, const float* d_fb, const float* d_dct,
                     float* d_ceps, float* d_logmel, int* d_frames, int B, int T, int n_fft, int hop, int n_mels, int n_ceps, float eps,
                     void* stream) {
  if (!d_x || !d_len || !d_window || !d_twiddle || !d_fb || !d_dct) VQVS_FAIL(VQVS_ERR_ARG, "x, len, window, twiddle, fb and dct must be non-NULL");
  if (!d_ceps || !d_frames) VQVS_FAIL(VQVS_ERR_ARG, "ceps and frames must be non-NULL");
  if (B < 1 || B > 65535) VQVS_FAIL(VQVS_ERR_ARG, "batch %d outside 1..65535", B);
  if (n_fft < 16 || n_fft > 512 || n_fft % 2) VQVS_FAIL(VQVS_ERR_ARG, "n_fft=%d must be even and in 16..512", n_fft);
  if (T <= n_fft / 2) VQVS_FAIL(VQVS_ERR_ARG, "rows of %d samples are no longer than the reflect padding (%d)", T, n_fft / 2);
  if (T > (1 << 30)) VQVS_FAIL(VQVS_ERR_ARG, "rows of %d samples: more than 2^30", T);
  if (hop < 1 || hop > n_fft) VQVS_FAIL(VQVS_ERR_ARG, "hop=%d outside 1..n_fft=%d", hop, n_fft);
  if (T / hop + 1 > (1 << 25)) VQVS_FAIL(VQVS_ERR_ARG, "T=%d at hop=%d is more than 2^25 frames per row", T, hop);
  if (n_mels < 1 || n_mels > 128) VQVS_FAIL(VQVS_ERR_ARG, "n_mels=%d outside 1..128", n_mels);
  if (n_ceps < 2 || n_ceps > (n_mels < 64 ? n_mels : 64)) VQVS_FAIL(VQVS_ERR_ARG, "n_ceps=%d outside 2..min(n_mels=%d, 64)", n_ceps, n_mels);
  if (!std::isfinite(eps) || !(eps > 0.f)) VQVS_FAIL(VQVS_ERR_ARG, "eps=%g must be finite and positive", (double)eps);
  const int64_t NF = (int64_t)B * (T / hop + 1);
  if (int e = check_disjoint({{"ceps", d_ceps, NF * n_ceps * 4}, {"logmel", d_logmel, NF * n_mels * 4}, {"frames", d_frames, (int64_t)B * 4}},
                             {{"x", d_x, (int64_t)B * T * 4}, {"len", d_len, (int64_t)B * 4}, {"window", d_window, (int64_t)n_fft * 4},
                              {"twiddle", d_twiddle, (int64_t)n_fft * 16}, {"fb", d_fb, (int64_t)(n_fft / 2 + 1) * n_mels * 4},
                              {"dct", d_dct, (int64_t)n_mels * n_ceps * 4}}))
    return e;
  return run_mel_cepstra(d_x, d_len, d_window, d_twiddle, d_fb, d_dct, d_ceps, d_logmel, d_frames, B, T, n_fft, hop, n_mels, n_ceps, eps,
                         reinterpret_cast<hipStream_t>(stream));
}

int vqvs_dtw_distance(const float* d_ca, const float* d_cb, const int* d_fa, const int* d_fb, const double* d_ta, const double* d_tb,
                      double* d_cost, int* d_steps, long long* d_track_counts, double* d_track_sums, int B, int Fa_max, int Fb_max,
                      int n_ceps, void* stream) {
  if (!d_ca || !d_cb || !d_fa || !d_fb) VQVS_FAIL(VQVS_ERR_ARG, "ca, cb, fa and fb must be non-NULL");
  if (!d_cost || !d_steps) VQVS_FAIL(VQVS_ERR_ARG, "cost and steps must be non-NULL");
  if (!d_ta != !d_tb) VQVS_FAIL(VQVS_ERR_ARG, "the tracks ta and tb come together: both or neither");
  if (!d_track_counts != !d_track_sums) VQVS_FAIL(VQVS_ERR_ARG, "track_counts and track_sums come together: both or neither");
  if (!d_ta != !d_track_counts) VQVS_FAIL(VQVS_ERR_ARG, "track_counts and track_sums are required if and only if the tracks are given");
  if (B < 1 || B > 65535) VQVS_FAIL(VQVS_ERR_ARG, "batch %d outside 1..65535", B);
  if (Fa_max < 1 || Fa_max > 2048) VQVS_FAIL(VQVS_ERR_ARG, "Fa_max=%d outside 1..2048", Fa_max);
  if (Fb_max < 1 || Fb_max > 2048) VQVS_FAIL(VQVS_ERR_ARG, "Fb_max=%d outside 1..2048", Fb_max);
  if (n_ceps < 2 || n_ceps > 64) VQVS_FAIL(VQVS_ERR_ARG, "n_ceps=%d outside 2..64", n_ceps);
  const int64_t NA = (int64_t)B * Fa_max, NB = (int64_t)B * Fb_max;
  if (int e = check_disjoint({{"cost", d_cost, (int64_t)B * 8}, {"steps", d_steps, (int64_t)B * 4}, {"track_counts", d_track_counts, (int64_t)B * 16},
                              {"track_sums", d_track_sums, (int64_t)B * 16}},
                             {{"ca", d_ca, NA * n_ceps * 4}, {"cb", d_cb, NB * n_ceps * 4}, {"fa", d_fa, (int64_t)B * 4}, {"fb", d_fb, (int64_t)B * 4},
                              {"ta", d_ta, NA * 8}, {"tb", d_tb, NB * 8}}))
    return e;
  return run_dtw_distance(d_ca, d_cb, d_fa, d_fb, d_ta, d_tb, d_cost, d_steps, d_track_counts, d_track_sums, B, Fa_max, Fb_max, n_ceps,
                          reinterpret_cast<hipStream_t>(stream));
}

int vqvs_pitch_distance(const float* a, const float* b, double* period_a, double* period_b, long long* counts, double* sums, int B, int T,
                        int window, int hop, int tau_min, int tau_max, double threshold, void* stream) {
  if (!a) VQVS_FAIL(VQVS_ERR_ARG, "a must be non-NULL");
  if (!b && (period_b || counts || sums)) VQVS_FAIL(VQVS_ERR_ARG, "b is NULL: period_b, counts and sums must be NULL too");
  if (!b && !period_a) VQVS_FAIL(VQVS_ERR_ARG, "b is NULL: period_a must be given");
  if (!period_a && !period_b && !counts && !sums) VQVS_FAIL(VQVS_ERR_ARG, "every output is NULL: nothing to compute");
  if (B < 1 || B > 65535) VQVS_FAIL(VQVS_ERR_ARG, "batch %d outside 1..65535", B);
  if (T < 1 || T > (1 << 30)) VQVS_FAIL(VQVS_ERR_ARG, "clip of %d samples outside 1..2^30", T);
  if (window < 16 || window > 2048) VQVS_FAIL(VQVS_ERR_ARG, "window=%d outside 16..2048", window);
  if (hop < 1 || hop > window) VQVS_FAIL(VQVS_ERR_ARG, "hop=%d outside 1..window=%d", hop, window);
  if (T / hop + 1 > (1 << 25)) VQVS_FAIL(VQVS_ERR_ARG, "T=%d at hop=%d is more than 2^25 frames per clip", T, hop);
  if (tau_max < 3 || tau_max > 1023) VQVS_FAIL(VQVS_ERR_ARG, "tau_max=%d outside 3..1023", tau_max);
  if (tau_min < 2 || tau_min >= tau_max) VQVS_FAIL(VQVS_ERR_ARG, "tau_min=%d outside 2..tau_max-1=%d", tau_min, tau_max - 1);
  if ((int64_t)window * tau_max > (1 << 20))
    VQVS_FAIL(VQVS_ERR_ARG, "window=%d times tau_max=%d is more than 2^20: the sums would not stay below 2^53", window, tau_max);
  if (!std::isfinite(threshold) || !(threshold > 0.0) || threshold > 1.0) VQVS_FAIL(VQVS_ERR_ARG, "threshold=%g must lie in (0, 1]", threshold);
  const int64_t N = (int64_t)B * T, NF = (int64_t)B * (T / hop + 1);
  if (int e = check_disjoint({{"period_a", period_a, NF * 8}, {"period_b", period_b, NF * 8}, {"counts", counts, (int64_t)B * 32}, {"sums", sums, (int64_t)B * 16}},
                             {{"a", a, N * 4}, {"b", b, N * 4}}))
    return e;
  ScratchLease lease;
  if (counts || sums)
    if (int e = scratch_get(pitch_distance_scratch_bytes(B, T, hop), stream, lease)) return e;
  return run_pitch_distance(a, b, period_a, period_b, counts, sums, lease.p, B, T, window, hop, tau_min, tau_max, threshold,
                            reinterpret_cast<hipStream_t>(stream));
}

int vqvs_vq_embed(const int64_t* d_idx, const float* d_dict, float* d_out, int B, int Cd, int T1, int K, void* stream) {
  if (!d_idx || !d_dict || !d_out) VQVS_FAIL(VQVS_ERR_ARG, "idx, dict and out must be non-NULL");
  if (B < 1 || Cd < 1 || T1 < 1 || K < 1) VQVS_FAIL(VQVS_ERR_ARG, "bad shape B=%d Cd=%d T1=%d K=%d", B, Cd, T1, K);
  if (B > 65535) VQVS_FAIL(VQVS_ERR_ARG, "batch %d outside 1..65535", B);           // grid dimension z
  if (Cd > 65535) VQVS_FAIL(VQVS_ERR_ARG, "channels %d outside 1..65535", Cd);      // grid dimension y
  return run_vq_embed(d_idx, d_dict, d_out, B, Cd, T1, K, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_debug_tap_count(const vqvs_model* m) { return m ? (int)m->taps.size() : 0; }

int vqvs_debug_tap_info(const vqvs_model* m, int i, char* name_out, int name_cap, int* channels, int* length_shift) {
  if (!m || i < 0 || i >= (int)m->taps.size()) VQVS_FAIL(VQVS_ERR_ARG, "bad tap index");
  if (name_out && name_cap > 0) {
    strncpy(name_out, m->taps[i].name.c_str(), name_cap - 1);
    name_out[name_cap - 1] = 0;
  }
  if (channels) *channels = m->taps[i].t.C;
  if (length_shift) *length_shift = m->taps[i].t.lshift;
  return 0;
}

int vqvs_debug_tap_rows(const vqvs_model* m, int i, int T) {
  if (!m || i < 0 || i >= (int)m->taps.size()) VQVS_FAIL(VQVS_ERR_ARG, "bad tap index");
  return tensor_rows(T, m->taps[i].t.lshift);
}

int vqvs_debug_read_tap(vqvs_model* m, int i, int B, int T, float* h_out) {
  if (!m || i < 0 || i >= (int)m->taps.size() || !h_out) VQVS_FAIL(VQVS_ERR_ARG, "bad argument");
  if (!m->cfg.debug_taps) VQVS_FAIL(VQVS_ERR_STATE, "model was not created with debug_taps=1");
  const TensorH& t = m->taps[i].t;
  const int L = tensor_rows(T, t.lshift);
  const size_t n = (size_t)B * t.C * L;
  float* d_tmp = nullptr;
  VQVS_HIP(hipSetDevice(m->device));
  VQVS_HIP(hipMalloc(reinterpret_cast<void**>(&d_tmp), n * 4));
  int e = launch_ntc_to_nct(m->act(t.off), d_tmp, B, t.C, L, t.f32 ? 0 : m->cfg.precision, nullptr);
  if (!e) {
    hipError_t he = hipMemcpy(h_out, d_tmp, n * 4, hipMemcpyDeviceToHost);
    if (he != hipSuccess) {
      set_error(std::string("hipMemcpy failed: ") + hipGetErrorString(he));
      e = VQVS_ERR_HIP;
    }
  }
  (void)hipFree(d_tmp);
  return e;
}

int vqvs_debug_read_embedding(vqvs_model* m, int B, float* h_out) {
  if (!m || !h_out || B < 1 || B > m->cfg.max_batch) VQVS_FAIL(VQVS_ERR_ARG, "bad argument");
  if (!m->emb_E) VQVS_FAIL(VQVS_ERR_STATE, "this model kind has no timestep embedding");
  VQVS_HIP(hipSetDevice(m->device));
  VQVS_HIP(hipDeviceSynchronize());
  const float* src = m->miscp(m->emb_misc_off);
  VQVS_HIP(hipMemcpy(h_out, src, (size_t)B * m->emb_E * sizeof(float), hipMemcpyDeviceToHost));
  return m->emb_E;
}

int vqvs_debug_read_dfilm(vqvs_model* m, int B, float* h_out) {
  if (!m || !h_out || B < 1 || B > m->cfg.max_batch) VQVS_FAIL(VQVS_ERR_ARG, "bad argument");
  if (!m->dfilm_R) VQVS_FAIL(VQVS_ERR_STATE, "this model kind has no FiLM-gradient buffer");
  VQVS_HIP(hipSetDevice(m->device));
  VQVS_HIP(hipDeviceSynchronize());
  const float* src = m->miscp(m->dfilm_misc_off);
  VQVS_HIP(hipMemcpy(h_out, src, (size_t)B * m->dfilm_R * sizeof(float), hipMemcpyDeviceToHost));
  return m->dfilm_R;
}

int vqvs_debug_read_film(vqvs_model* m, int B, float* h_out) {
  if (!m || !h_out || B < 1 || B > m->cfg.max_batch) VQVS_FAIL(VQVS_ERR_ARG, "bad argument");
  if (!m->film_R) VQVS_FAIL(VQVS_ERR_STATE, "this model kind has no FiLM table");
  VQVS_HIP(hipSetDevice(m->device));
  VQVS_HIP(hipDeviceSynchronize());
  const float* src = m->miscp(m->film_misc_off);
  VQVS_HIP(hipMemcpy(h_out, src, (size_t)B * m->film_R * sizeof(float), hipMemcpyDeviceToHost));
  return m->film_R;
}

// ---- GroupNorm / xform debug entries (tests/test_groupnorm_gpu.py) -----------------------------------------------------------
namespace {
int debug_shape_ok(const vqvs_model* m, int B, int T) {
  if (!m) VQVS_FAIL(VQVS_ERR_ARG, "model is NULL");
  if (!m->cfg.debug_taps) VQVS_FAIL(VQVS_ERR_STATE, "model was not created with debug_taps=1");
  if (B < 1 || B > m->cfg.max_batch || T < 1 || T > m->cfg.max_T) VQVS_FAIL(VQVS_ERR_ARG, "B=%d T=%d outside the handle's 1..%d x 1..%d", B, T, m->cfg.max_batch, m->cfg.max_T);
  return 0;
}
RunCtx debug_ctx(int B, int T) {
  RunCtx c;
  c.B = B;
  c.Lbase = T;
  return c;
}
// an arena tensor [B][L][C] of the handle's storage type -> host float32 NCT [B][C][L]
int debug_read_tensor(vqvs_model* m, const TensorH& t, int B, int T, float* h_out) {
  const int L = tensor_rows(T, t.lshift);
  const size_t n = (size_t)B * t.C * L;
  float* d_tmp = nullptr;
  VQVS_HIP(hipSetDevice(m->device));
  VQVS_HIP(hipMalloc(reinterpret_cast<void**>(&d_tmp), n * 4));
  int e = launch_ntc_to_nct(m->act(t.off), d_tmp, B, t.C, L, t.f32 ? 0 : m->cfg.precision, nullptr);
  if (!e && hipMemcpy(h_out, d_tmp, n * 4, hipMemcpyDeviceToHost) != hipSuccess) {
    set_error("hipMemcpy failed");
    e = VQVS_ERR_HIP;
  }
  (void)hipFree(d_tmp);
  return e;
}
}  // namespace

int vqvs_debug_gn_count(const vqvs_model* m) { return m ? (int)m->gns.size() : 0; }

int vqvs_debug_gn_info(vqvs_model* m, int i, int B, int T, char* name_out, int name_cap, int64_t* info) {
  if (int e = debug_shape_ok(m, B, T)) return e;
  if (i < 0 || i >= (int)m->gns.size() || !info) VQVS_FAIL(VQVS_ERR_ARG, "bad GroupNorm index or NULL info");
  const GnDef& g = m->gns[i];
  if (name_out && name_cap > 0) {
    strncpy(name_out, g.name.c_str(), name_cap - 1);
    name_out[name_cap - 1] = 0;
  }
  const int L = tensor_rows(T, g.lshift);
  info[0] = g.Ctot;
  info[1] = g.groups;
  info[2] = (int64_t)g.cpg_real * L;
  info[3] = g.film ? 1 : 0;
  info[4] = g.film_off;
  info[5] = (int64_t)g.srcs.size();
  info[6] = g.has_mr ? 1 : 0;
  info[7] = g.fused(debug_ctx(B, T)) ? 1 : 0;
  for (size_t s = 0; s < 2; ++s) {
    const bool on = s < g.srcs.size();
    const int rows = on ? tensor_rows(T, g.srcs[s].lshift) : 0;
    info[8 + 4 * s] = on ? g.srcs[s].C : 0;
    info[9 + 4 * s] = rows;
    info[10 + 4 * s] = on ? g.tile_rows[s] : 0;
    info[11 + 4 * s] = on ? (rows + g.tile_rows[s] - 1) / g.tile_rows[s] : 0;
    info[16 + s] = on && g.sums_stored[s](debug_ctx(B, T)) ? 1 : 0;
  }
  return 0;
}

int vqvs_debug_gn_read(vqvs_model* m, int i, int B, int T, int what, int src, float* h_out) {
  if (int e = debug_shape_ok(m, B, T)) return e;
  if (i < 0 || i >= (int)m->gns.size() || !h_out) VQVS_FAIL(VQVS_ERR_ARG, "bad GroupNorm index or NULL h_out");
  const GnDef& g = m->gns[i];
  if (what < 0 || what > 3) VQVS_FAIL(VQVS_ERR_ARG, "what=%d outside 0..3", what);
  if (what <= 1 && (src < 0 || src >= (int)g.srcs.size())) VQVS_FAIL(VQVS_ERR_ARG, "source %d of a GroupNorm over %d", src, (int)g.srcs.size());
  VQVS_HIP(hipSetDevice(m->device));
  VQVS_HIP(hipDeviceSynchronize());
  if (what == 0) return debug_read_tensor(m, g.srcs[src], B, T, h_out);
  if (what == 1) {
    const TensorH& t = g.srcs[src];
    const int rows = tensor_rows(T, t.lshift), nt = (rows + g.tile_rows[src] - 1) / g.tile_rows[src];
    const float* p = m->statp(t.stats_off);
    VQVS_HIP(hipMemcpy(h_out, p, (size_t)B * nt * t.C * 2 * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
  }
  if (what == 3 && !g.has_mr) VQVS_FAIL(VQVS_ERR_STATE, "the schedule keeps no (mean, rstd) table for this GroupNorm");
  const size_t bytes = (size_t)B * g.Ctot * 2 * sizeof(float);
  const RunCtx c = debug_ctx(B, T);
  if (what == 2 && g.fused(c)) {
    // the consuming convolution built this call's table in LDS: the schedule's own gn_prepare launch, on the resident partials, into
    // a scratch table (the status word is left alone: reading does not change what vqvs_model_status reports)
    GnArgs a{};
    g.fill(c, a);
    float2* d_tmp = nullptr;
    VQVS_HIP(hipMalloc(reinterpret_cast<void**>(&d_tmp), bytes));
    a.ss = d_tmp;
    a.mr = nullptr;
    a.status = nullptr;
    int e = launch_gn_prepare(a, B, nullptr);
    if (!e && hipMemcpy(h_out, d_tmp, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("hipMemcpy failed");
      e = VQVS_ERR_HIP;
    }
    (void)hipFree(d_tmp);
    return e;
  }
  const float* p = m->ssp(what == 2 ? g.ss_off : g.mr_off);
  VQVS_HIP(hipMemcpy(h_out, p, bytes, hipMemcpyDeviceToHost));
  return 0;
}

int vqvs_debug_xform_count(const vqvs_model* m) { return m ? (int)m->xforms.size() : 0; }

int vqvs_debug_xform_info(vqvs_model* m, int i, int B, int T, int64_t* info) {
  if (int e = debug_shape_ok(m, B, T)) return e;
  if (i < 0 || i >= (int)m->xforms.size() || !info) VQVS_FAIL(VQVS_ERR_ARG, "bad xform index or NULL info");
  const XformDef& x = m->xforms[i];
  info[0] = x.gn;
  info[1] = x.in.C;
  info[2] = tensor_rows(T, x.in.lshift);
  info[3] = tensor_rows(T, x.out.lshift);
  info[4] = x.avg ? 1 : 0;
  info[5] = x.ss_stride;
  info[6] = x.ss_c0;
  return 0;
}

int vqvs_debug_xform_read(vqvs_model* m, int i, int B, int T, int output, float* h_out) {
  if (int e = debug_shape_ok(m, B, T)) return e;
  if (i < 0 || i >= (int)m->xforms.size() || !h_out) VQVS_FAIL(VQVS_ERR_ARG, "bad xform index or NULL h_out");
  VQVS_HIP(hipSetDevice(m->device));
  VQVS_HIP(hipDeviceSynchronize());
  return debug_read_tensor(m, output ? m->xforms[i].out : m->xforms[i].in, B, T, h_out);
}

int vqvs_debug_gelu(const float* d_in, float* d_out, int n, int form, void* stream) {
  if (!d_in || !d_out) VQVS_FAIL(VQVS_ERR_ARG, "d_in and d_out must be non-NULL");
  if (n < 1 || n > (1 << 30)) VQVS_FAIL(VQVS_ERR_ARG, "n=%d outside 1..2^30", n);
  if (form < 0 || form > 4) VQVS_FAIL(VQVS_ERR_ARG, "form=%d outside 0..4", form);
  return launch_debug_gelu(d_in, d_out, n, form, reinterpret_cast<hipStream_t>(stream));
}

int vqvs_forward_kernel_count(const vqvs_model* m) { return m ? (int)m->ops.size() : 0; }

int64_t vqvs_forward_model_bytes(const vqvs_model* m, int B, int T) {
  if (!m) return 0;
  const double es = m->cfg.precision == VQVS_PREC_F32 ? 4.0 : 2.0;  // BF16 and F16 store 2 bytes
  return (int64_t)((m->cost.elems_T * es + m->cost.bytes_f32) * (double)T * (double)B);
}

int64_t vqvs_forward_flops(const vqvs_model* m, int B, int T) {
  if (!m) return 0;
  return (int64_t)(m->cost.flops * (double)T * (double)B);
}

}  // extern "C"

// ---- profiling hooks (bench.py: live per-kernel timing with HIP events on the launch stream) ----
extern "C" {

int vqvs_set_profiling(vqvs_model* m, int on) {
  if (!m) VQVS_FAIL(VQVS_ERR_ARG, "model is NULL");
  m->profiling = on != 0;
  return 0;
}

// kind / algorithmic bytes / flops of op i for the given problem size
int vqvs_op_info(const vqvs_model* m, int i, char* kind_out, int kind_cap, int64_t* bytes_out, int64_t* flops_out, int B, int T) {
  if (!m || i < 0 || i >= (int)m->meta.size()) VQVS_FAIL(VQVS_ERR_ARG, "bad op index");
  const auto& mt = m->meta[i];
  if (kind_out && kind_cap > 0) {
    strncpy(kind_out, mt.kind.c_str(), kind_cap - 1);
    kind_out[kind_cap - 1] = 0;
  }
  const double es = m->cfg.precision == VQVS_PREC_F32 ? 4.0 : 2.0;  // BF16 and F16 store 2 bytes
  if (bytes_out) *bytes_out = (int64_t)((mt.elems_T * es + mt.bytes_f32) * (double)T * (double)B);
  if (flops_out) *flops_out = (int64_t)(mt.flops * (double)T * (double)B);
  return 0;
}

int vqvs_op_desc(const vqvs_model* m, int i, char* out, int cap) {
  if (!m || i < 0 || i >= (int)m->meta.size() || !out || cap < 1) VQVS_FAIL(VQVS_ERR_ARG, "bad argument");
  strncpy(out, m->meta[i].desc.c_str(), cap - 1);
  out[cap - 1] = 0;
  return 0;
}

// Device status word of the handle (synchronises the device; the word is cleared): bit 0 = a GroupNorm partial was not finite
// (an activation overflowed the storage type, or NaN input), bit 1 = fp16 mode, a tile's sum of squares reached 9e8 (an
// activation may be beyond 3e4 of fp16's 65504).  Callers check it once per sample, not per step.
int vqvs_model_status(vqvs_model* m, unsigned* h_status) {
  if (!m || !h_status) VQVS_FAIL(VQVS_ERR_ARG, "NULL argument");
  *h_status = 0;
  if (m->status_misc_off == (size_t)-1) return 0;
  unsigned* d = reinterpret_cast<unsigned*>(m->miscp(m->status_misc_off));
  VQVS_HIP(hipDeviceSynchronize());  // (forwards run on the caller's stream; a blocking copy on the null stream alone does not wait for a non-blocking one)
  VQVS_HIP(hipMemcpy(h_status, d, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (*h_status) VQVS_HIP(hipMemset(d, 0, sizeof(unsigned)));
  return 0;
}

// elapsed milliseconds of every op of the LAST profiled forward (synchronises the device)
int vqvs_profile_read(vqvs_model* m, float* h_ms, int cap) {
  if (!m || !h_ms) VQVS_FAIL(VQVS_ERR_ARG, "NULL argument");
  if (m->events.size() != m->ops.size() + 1) VQVS_FAIL(VQVS_ERR_STATE, "no profiled forward has run");
  VQVS_HIP(hipEventSynchronize(m->events.back()));
  const int n = (int)m->ops.size() < cap ? (int)m->ops.size() : cap;
  for (int i = 0; i < n; ++i) VQVS_HIP(hipEventElapsedTime(&h_ms[i], m->events[i], m->events[i + 1]));
  return n;
}

}  // extern "C"

// The in-kernel phase counters of the instrumented build (`make timing`, -DVQVS_TIMING); every other build exports the two entries too,
// so that the header and the library agree in every build, and refuses the call.
#ifdef VQVS_TIMING
namespace vqvs { int conv_timing_read(unsigned long long* out24, int reset); }
extern "C" int vqvs_debug_conv_timing(unsigned long long* h_counters, int reset) { return vqvs::conv_timing_read(h_counters, reset); }
namespace vqvs { int ws_timing_read(unsigned long long* out32, int reset); }
extern "C" int vqvs_debug_ws_timing(unsigned long long* h_counters, int reset) { return vqvs::ws_timing_read(h_counters, reset); }
#else
extern "C" int vqvs_debug_conv_timing(unsigned long long*, int) { VQVS_FAIL(VQVS_ERR_STATE, "this library was built without -DVQVS_TIMING"); }
extern "C" int vqvs_debug_ws_timing(unsigned long long*, int) { VQVS_FAIL(VQVS_ERR_STATE, "this library was built without -DVQVS_TIMING"); }
#endif
