// Host-side network description: topology -> parameter table -> packed device weights ->
// static launch schedule over a liveness-planned scratch arena.  Nothing here runs per
// element; it decides what the kernels in conv_mfma.hip / misc_kernels.hip are pointed at.
#pragma once

#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vqvs.h"
#include "kernels.hpp"

namespace vqvs {

struct ParamDef {
  std::string name;
  std::vector<int64_t> shape;
  size_t numel() const {
    size_t n = 1;
    for (auto s : shape) n *= (size_t)s;
    return n;
  }
};

// Activation tensor in the arena: [max_batch][L][C], L = base length shifted by lshift.
struct TensorH {
  int id = -1;
  size_t off = 0;        // byte offset in the arena
  int C = 0;
  int lshift = 0;        // L = lshift >= 0 ? Lbase >> lshift : Lbase << -lshift
  bool f32 = false;      // forced float32 storage (boundary tensors)
  size_t stats_off = 0;  // float offset in the statistics region, valid if has_stats
  bool has_stats = false;
};

struct RunCtx {
  int B = 0;
  int Lbase = 0;  // T for UNets, L of the input for a resblock handle
  const float* x = nullptr;
  const float* ts = nullptr;
  const float* cond = nullptr;
  const int64_t* labels = nullptr;
  const float* emb = nullptr;  // resblock handle: external embedding
  const float* logmel = nullptr;  // MFCC encoder handle, testing entry: [B][frames][n_mels] log-mel rows replacing the front end's
  float* out = nullptr;
  // classifier handles: logits [B][num_labels]; with backward, grad_out [B][T] = gscale * d log p(labels) / dx
  bool backward = false;
  float gscale = 1.0f;
  float* grad_out = nullptr;
  // classifier handles, vqvs_classifier_features: [B][F] features and [B][num_labels] probabilities, or nullptr (out may be too)
  float* feat = nullptr;
  float* probs = nullptr;
  // predictor-gradient handles (vqvs_unet_embed_grad): the conditioning vector of every clip [B][E] in place of class_embed[labels],
  // the target noise [B][T], and the outputs mse [B] and egrad [B][E]; `out` (the prediction) may be nullptr.
  // class_vec is honoured by class-conditional predictor handles as well (vqvs_unet_forward_vec): labels is then nullptr
  const float* class_vec = nullptr;
  const float* eps = nullptr;
  float* mse = nullptr;
  float* egrad = nullptr;
  hipStream_t st = nullptr;
};

struct TapDef {
  std::string name;
  TensorH t;
};

// What the debug entries of include/vqvs.h (vqvs_debug_gn_*, vqvs_debug_xform_*) need to know about one GroupNorm / one xform entry of
// the schedule; recorded by Builder::add_gn / add_xform on handles created with debug_taps = 1, in schedule order.
struct GnDef {
  std::string name;
  std::vector<TensorH> srcs;   // 1 tensor, or 2 for a GroupNorm over torch.cat
  std::vector<int> tile_rows;  // rows per statistics tile of each source's producer
  // per source: did its producer sum the values as STORED at this (B, L)?  (false: the float32 values before they were rounded to a
  // 2-byte storage type -- in_conv_kernel and conv_mfma_kernel; conv_ws_kernel and ntc_stats_kernel sum what they store)
  std::vector<std::function<bool(const RunCtx&)>> sums_stored;
  int Ctot = 0, groups = 0, cpg_real = 0, lshift = 0;  // cpg_real: channels per group at the REAL width (inv_count = 1 / (cpg_real * L))
  bool film = false;
  int film_off = 0, film_stride = 0;
  size_t ss_off = 0, mr_off = 0;  // float offsets in the ss region
  bool has_mr = false;
  std::function<bool(const RunCtx&)> fused;            // did the consuming convolution build the table itself at this (B, L)?
  std::function<void(const RunCtx&, GnArgs&)> fill;    // the arguments the schedule's gn_prepare entry launches with
};
struct XformDef {
  TensorH in, out;
  bool avg = false;
  int gn = -1;  // index of the GroupNorm whose table it reads
  int ss_stride = 0, ss_c0 = 0;
};

}  // namespace vqvs

struct vqvs_model {
  vqvs_cfg cfg{};
  int device = 0;
  std::vector<vqvs::ParamDef> params;
  // device memory
  char* d_weights = nullptr;
  size_t weights_bytes = 0;
  char* d_arena = nullptr;
  size_t arena_bytes = 0;
  // arena regions, laid out by build_model after planning: [activations | stats | ss | misc]
  size_t act_bytes = 0, stats_off = 0, stats_floats = 0, ss_off = 0, ss_floats = 0, misc_off = 0, misc_floats = 0;
  // ---- pointer resolution at run time: the one statement of that layout (the schedule entries and the debug readers of api.cpp hold
  // byte offsets into the activations and the weight blob, float offsets into the other three regions)
  char* act(size_t off) const { return d_arena + off; }
  float* statp(size_t foff) const { return reinterpret_cast<float*>(d_arena + stats_off) + foff; }
  float* ssp(size_t foff) const { return reinterpret_cast<float*>(d_arena + ss_off) + foff; }
  float* miscp(size_t foff) const { return reinterpret_cast<float*>(d_arena + misc_off) + foff; }
  char* wp(size_t off) const { return d_weights + off; }
  const float* wf(size_t off) const { return reinterpret_cast<const float*>(wp(off)); }  // a float32 entry of the weight blob
  float2* ssf2(size_t foff) const { return reinterpret_cast<float2*>(ssp(foff)); }       // a (scale, shift) / (mean, rstd) table
  std::vector<std::function<int(const vqvs::RunCtx&)>> ops;
  struct OpMeta {
    std::string kind;      // "conv", "gn_prepare", "in_conv", ...
    std::string desc;      // human-readable shape (profiling tables)
    double elems_T = 0;    // algorithmic activation elements (storage type) per clip per unit of base length
    double bytes_f32 = 0;  // float32 boundary bytes per clip per unit of base length
    double flops = 0;      // per clip per unit of base length
  };
  std::vector<OpMeta> meta;  // parallel to ops
  // ops of phase 0 always run; phase 1 ops (a backward schedule) only when asked for.  Parallel to ops too: the three vectors are
  // appended to together, by Builder::op in net.cpp and nowhere else
  std::vector<uint8_t> op_phase;
  bool profiling = false;
  std::vector<hipEvent_t> events;  // ops.size() + 1 when profiling
  std::vector<vqvs::TapDef> taps;
  std::vector<vqvs::GnDef> gns;        // debug_taps handles only
  std::vector<vqvs::XformDef> xforms;  // debug_taps handles only
  // accounting (per clip, per unit of base length): elements moved / flops, as (coefficient, lshift) lists
  struct Cost {
    double elems_T = 0;    // activation elements of type T moved per clip at Lbase = 1 (scaled by L)
    double bytes_f32 = 0;  // boundary float32 bytes per clip per unit length
    double flops = 0;      // per clip per unit length
  } cost;
  int last_B = 0, last_L = 0;
  size_t status_misc_off = (size_t)-1;  // device status word (misc region, floats) or -1: the handle has no GroupNorm
  size_t emb_misc_off = 0;  // conditioning vector [max_batch][emb_E] of the last forward (misc region, floats); emb_E = 0: none
  int emb_E = 0;
  size_t dfilm_misc_off = 0;  // predictor-gradient handles: d loss / d FiLM rows [max_batch][dfilm_R] of the last call (misc region, floats)
  int dfilm_R = 0;
  size_t film_misc_off = 0;  // FiLM rows [max_batch][film_R] of the last forward, the `film` op's output (misc region, floats); film_R = 0: none
  int film_R = 0;
};

namespace vqvs {
int enumerate_params(const vqvs_cfg& cfg, std::vector<ParamDef>& out);
int build_model(vqvs_model* m, const float* const* h_params);
int run_model(vqvs_model* m, const RunCtx& ctx);
int gn_groups(int ch);
int real_base(const vqvs_cfg& c);  // the reference width of a padded predictor / encoder handle (vqvs_cfg.reserved[4]), else base_channels
int padded_base(int real);
void pad_blocks(int real, int* q, int* qp);  // pad_map(real), for vqvs_pad_blocks
int unet_rate(const vqvs_cfg& cfg);  // downsample rate of a predictor / encoder handle's topology (256 for the reference's default)
int tensor_rows(int Lbase, int lshift);  // rows per clip of a tensor with length code `lshift` at base length Lbase
}  // namespace vqvs
