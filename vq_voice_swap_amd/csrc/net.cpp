// Topology of the reference's UNets (reference vq_voice_swap/models/unet.py:17-116, 188-227),
// restated as a static schedule of fused kernels.  Per ResBlock (unet.py:248-316):
//
//   gn_prepare(x stats, pre_cond.0.0)                 -> scale/shift of GroupNorm 1
//   conv  [GN1+GELU -> resize -> Conv3]               -> h1   (+ statistics of h1)
//   gn_prepare(h1 stats, pre_cond.3, FiLM a|b)        -> scale/shift of GroupNorm 2 (+FiLM)
//   conv  [GN2*FiLM+GELU -> dilated Conv3] + skip     -> out  (+ statistics of out)
//
// i.e. two streaming passes over the activations per block (SURVEY.md 8d "Model A").
#include "net.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <optional>

namespace vqvs {

namespace {

// The UNets' topology (unet.py:17-30, 188-196): the reference's defaults unless the configuration carries its own
// (vqvs_cfg.topology_set; predictor and encoder handles -- the classifier stem and the encoder predictor are built with the defaults).
struct Topo {
  std::vector<int> mult;  // channel_mult
  int depth = 2;          // depth_mult
  std::vector<int> dil;   // middle_dilations (predictor) / out_dilations (encoder)
  int levels() const { return (int)mult.size(); }
};
Topo topo_of(const vqvs_cfg& c) {
  Topo t;
  const bool custom = c.topology_set != 0 && (c.kind == VQVS_KIND_PREDICTOR || c.kind == VQVS_KIND_PREDICTOR_GRAD || c.kind == VQVS_KIND_ENCODER ||
                                              c.kind == VQVS_KIND_CLASSIFIER);
  if (custom) {
    t.mult.assign(c.channel_mult, c.channel_mult + std::max(0, std::min(c.n_levels, (int)VQVS_MAX_LEVELS)));
    t.depth = c.depth_mult;
    t.dil.assign(c.dilations, c.dilations + std::max(0, std::min(c.n_dilations, 12)));
  } else {
    t.mult = {1, 1, 2, 2, 2, 4, 4, 8, 8};  // unet.py:20
    t.depth = 2;                            // unet.py:22
    if (c.kind != VQVS_KIND_ENCODER && c.kind != VQVS_KIND_CLASSIFIER) t.dil = {4, 8, 16, 32};  // unet.py:21 (UNetEncoder: out_dilations = (), unet.py:192)
  }
  return t;
}

struct BlockSpec {
  std::string prefix;
  int cin, cout, resize, dil;
  bool cat;
};

void predictor_blocks(int base, const Topo& tp, std::vector<BlockSpec>& down, std::vector<BlockSpec>& mid, std::vector<BlockSpec>& up) {
  const int NLEVEL = tp.levels(), DEPTH_MULT = tp.depth;
  std::vector<int> stack{base};
  int cur = base;
  for (int depth = 0; depth < NLEVEL; ++depth) {
    const int mult = tp.mult[depth];
    for (int i = 0; i < DEPTH_MULT; ++i) {
      down.push_back({"down_blocks." + std::to_string(down.size()), cur, mult * base, RESIZE_NONE, 2, false});
      cur = mult * base;
      stack.push_back(cur);
    }
    if (depth != NLEVEL - 1) {
      down.push_back({"down_blocks." + std::to_string(down.size()), cur, cur, RESIZE_AVG2, 2, false});
      stack.push_back(cur);
    }
  }
  for (size_t i = 0; i < tp.dil.size(); ++i) mid.push_back({"middle_blocks." + std::to_string(i), cur, cur, RESIZE_NONE, tp.dil[i], false});
  for (int depth = NLEVEL - 1; depth >= 0; --depth) {
    const int mult = tp.mult[depth];
    for (int i = 0; i < DEPTH_MULT + 1; ++i) {
      const int sk = stack.back();
      stack.pop_back();
      up.push_back({"up_blocks." + std::to_string(up.size()), cur + sk, mult * base, RESIZE_NONE, 2, true});
      cur = mult * base;
    }
    if (depth) up.push_back({"up_blocks." + std::to_string(up.size()), cur, cur, RESIZE_UP2, 2, false});
  }
}

int encoder_blocks(int base, const Topo& tp, std::vector<BlockSpec>& blocks) {  // returns the width of the last block
  const int NLEVEL = tp.levels(), DEPTH_MULT = tp.depth;
  int cur = base;
  for (int depth = 0; depth < NLEVEL; ++depth) {
    const int mult = tp.mult[depth];
    for (int i = 0; i < DEPTH_MULT; ++i) {
      blocks.push_back({"blocks." + std::to_string(blocks.size()), cur, mult * base, RESIZE_NONE, 2, false});
      cur = mult * base;
    }
    if (depth != NLEVEL - 1) blocks.push_back({"blocks." + std::to_string(blocks.size()), cur, cur, RESIZE_AVG2, 2, false});
  }
  for (int d : tp.dil) blocks.push_back({"blocks." + std::to_string(blocks.size()), cur, cur, RESIZE_NONE, d, false});  // out_dilations, unet.py:219-220
  return cur;
}

// ClassifierStem (classifier.py:79-96): like the encoder, but FiLM-conditioned and with a x0.5 block after EVERY level
// (classifier.py:52-58: channel_mult and depth_mult with the UNets' defaults; output_mult = vqvs_cfg.reserved[1], 0 = 16.)  Returns the
// width of the last block.
int classifier_blocks(int base, const Topo& tp, std::vector<BlockSpec>& blocks) {
  const int NLEVEL = tp.levels(), DEPTH_MULT = tp.depth;
  int cur = base;
  for (int depth = 0; depth < NLEVEL; ++depth) {
    const int mult = tp.mult[depth];
    for (int i = 0; i < DEPTH_MULT; ++i) {
      blocks.push_back({"stem.blocks." + std::to_string(blocks.size()), cur, mult * base, RESIZE_NONE, 2, false});
      cur = mult * base;
    }
    blocks.push_back({"stem.blocks." + std::to_string(blocks.size()), cur, cur, RESIZE_AVG2, 2, false});
  }
  return cur;
}
int classifier_output_mult(const vqvs_cfg& c) { return c.reserved[1] > 0 ? c.reserved[1] : 16; }

void block_params(std::vector<ParamDef>& out, const std::string& p, const BlockSpec& s, int emb, bool dropout) {
  const std::string pre = p.empty() ? "" : p + ".";
  out.push_back({pre + "pre_cond.0.0.weight", {s.cin}});
  out.push_back({pre + "pre_cond.0.0.bias", {s.cin}});
  out.push_back({pre + "pre_cond.2.weight", {s.cout, s.cin, 3}});
  out.push_back({pre + "pre_cond.2.bias", {s.cout}});
  out.push_back({pre + "pre_cond.3.weight", {s.cout}});
  out.push_back({pre + "pre_cond.3.bias", {s.cout}});
  if (emb) {
    out.push_back({pre + "cond_layers.1.weight", {2 * s.cout, emb}});
    out.push_back({pre + "cond_layers.1.bias", {2 * s.cout}});
  }
  const std::string c2 = pre + (dropout ? "post_cond.2" : "post_cond.1");  // unet.py:295-305
  out.push_back({c2 + ".weight", {s.cout, s.cout, 3}});
  out.push_back({c2 + ".bias", {s.cout}});
  if (s.cin != s.cout) {
    out.push_back({pre + "skip.1.weight", {s.cout, s.cin, 1}});
    out.push_back({pre + "skip.1.bias", {s.cout}});
  }
}

bool cfg_dropout(const vqvs_cfg& c) { return c.reserved[0] != 0; }

uint16_t f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
// float32 -> IEEE binary16, round to nearest even (VQVS_PREC_F16 packs the convolution weights in the operand type)
uint16_t f2h(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  const uint32_t a = u & 0x7fffffffu;
  if (a >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (a > 0x7f800000u ? 0x200u : 0u));
  if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // >= 65520 rounds to infinity
  if (a < 0x33000001u) return (uint16_t)sign;                // < 2^-25 rounds to zero
  int e = (int)(a >> 23) - 127;
  uint32_t m = (a & 0x7fffffu) | 0x800000u;
  int shift = e < -14 ? (13 + (-14 - e)) : 13;               // subnormal results lose further bits
  uint32_t r = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (r & 1u))) ++r;
  if (e < -14) return (uint16_t)(sign | r);                  // r may carry into the smallest normal: still correct bits
  return (uint16_t)(sign | (((uint32_t)(e + 15) << 10) + (r - 0x400u)));
}
float bf2f(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

struct Blob {
  std::vector<char> data;
  size_t add(const void* p, size_t bytes) {
    size_t off = (data.size() + 255) & ~(size_t)255;
    data.resize(off + bytes);
    if (p) memcpy(data.data() + off, p, bytes);
    return off;
  }
};

// conv weights in MFMA B-operand order: [segment][chunk of 32 ci][tap][Cout][32 ci]
struct PackedConv {
  std::vector<uint16_t> hi, lo;
  bool f16 = false;  // VQVS_PREC_F16: `hi` holds binary16 bits, `lo` is unused
  explicit PackedConv(int precision = VQVS_PREC_F32) : f16(precision == VQVS_PREC_F16) {}
  long long append(const float* W, int Cout, int Cin_total, int ktaps, int cb, int C) {
    const long long off = (long long)hi.size();
    for (int ch = 0; ch < C / 32; ++ch)
      for (int k = 0; k < ktaps; ++k)
        for (int co = 0; co < Cout; ++co)
          for (int j = 0; j < 32; ++j) {
            const float w = W[((size_t)co * Cin_total + cb + ch * 32 + j) * ktaps + k];
            if (f16) {
              hi.push_back(f2h(w));
              continue;
            }
            const uint16_t h = f2bf(w);
            hi.push_back(h);
            lo.push_back(f2bf(w - bf2f(h)));
          }
    return off;
  }
};

// weights of the transposed convolution (gradient w.r.t. the input): Wt[ci][co][k] = W[co][ci][K-1-k]
std::vector<float> transpose_flip(const float* W, int Cout, int Cin, int ktaps) {
  std::vector<float> t((size_t)Cout * Cin * ktaps);
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int k = 0; k < ktaps; ++k) t[((size_t)ci * Cout + co) * ktaps + k] = W[((size_t)co * Cin + ci) * ktaps + (ktaps - 1 - k)];
  return t;
}

// A tensor's length is a function of the base length of the run.  UNets: a power-of-two shift.  ConvMFCCEncoder
// (conv_encoder.py:44-58, 65-71): lengths derived from the MFCC frame count T / hop + 1, encoded as lshift >= LEN_FRAMES.
constexpr int MFCC_HOP = 160;     // input_rate / mfcc_rate = 16000 / 100 (conv_encoder.py:29-30, never changed by make_encoder)
constexpr int LEN_FRAMES = 100;   // T / hop + 1                      (torch.stft, center=True)
constexpr int LEN_FRAMES_PAD = 101;  // frames rounded up to even: allocation of the tensor the stride-2 convolution reads
constexpr int LEN_PAIRS = 102;    // LEN_FRAMES_PAD / 2: rows of that tensor viewed as [pairs][2 * channels]
constexpr int LEN_HALF = 103;     // (frames + 2 - 4) / 2 + 1: output length of Conv1d(k = 4, stride = 2, padding = 1)
constexpr int LEN_ABS = 1000;     // lshift >= LEN_ABS: a fixed number of rows, lshift - LEN_ABS, whatever the base length (a conditioning
                                  // sequence of arbitrary length: the reference up-samples ANY length to T, unet.py:138-139)
double lscale(int lshift) {
  if (lshift >= LEN_ABS) return 0.0;  // (not proportional to the base length: left out of the per-unit-length accounting)
  if (lshift >= LEN_FRAMES) return (lshift == LEN_PAIRS || lshift == LEN_HALF ? 0.5 : 1.0) / MFCC_HOP;
  return lshift >= 0 ? 1.0 / (double)(1 << lshift) : (double)(1 << -lshift);
}
int shiftL(int L, int lshift) {
  if (lshift >= LEN_ABS) return lshift - LEN_ABS;
  if (lshift >= LEN_FRAMES) {
    const int frames = L / MFCC_HOP + 1;
    if (lshift == LEN_FRAMES) return frames;
    if (lshift == LEN_FRAMES_PAD) return (frames + 1) & ~1;
    if (lshift == LEN_PAIRS) return (frames + 1) >> 1;
    return (frames - 2) / 2 + 1;
  }
  return lshift >= 0 ? (L >> lshift) : (L << -lshift);
}
int ntiles_of(int L, int rows = STAT_TILE) { return (L + rows - 1) / rows; }
constexpr int MIN_TILE_ROWS = 124;  // the smallest statistics tile any producer uses (128-row tiles, dilation 2)

// Widths that are not multiples of 32 (vqvs_cfg.reserved[4] = the REAL base_channels of a predictor / encoder, 0 = base_channels itself):
// the handle is built at the PHYSICAL width base_channels = padded_base(real), whose channels come in blocks of q_p of which the
// first q carry the real channels and the rest are zero (weights, biases, affine parameters and FiLM rows of the pad channels are
// zero: a pad channel is exactly 0 in every tensor).  real = 2^k * q with q odd; q_p = the next power of two >= q, widened until
// 2^k * q_p is a multiple of 32.  Every real width m * real is a multiple of q and every GroupNorm group of the reference
// (unet.py:345-349: 32 groups halved until they divide the width -- a power of two) is a whole number of blocks, so the reference's
// groups are runs of physical channels too: the zero channels add nothing to a group's sums, and only the group COUNT and the number
// of values per group (inv_count) have to come from the real width.
struct PadMap {
  int q = 1, qp = 1;
  int phys(int c) const { return (c / q) * qp + c % q; }
};
PadMap pad_map(int real) {
  PadMap m;
  int k = 0;
  while (((real >> k) & 1) == 0 && k < 5) ++k;
  m.q = real >> k;
  m.qp = 1;
  while (m.qp < m.q) m.qp <<= 1;
  while (((1 << k) * m.qp) % 32) m.qp <<= 1;
  if (real % 32 == 0) m.qp = m.q;  // (nothing to pad)
  return m;
}

// The guidance gradients d log p / d activation are O(1e-6 ... 1e-3): in fp16 storage they would sit in or below the
// subnormal range (6e-5).  The backward schedule is linear in the gradient, so the fp16 mode carries it multiplied by 2^10
// from the head (gscale) to the last kernel (in_conv_bw), which divides it out again in fp32.  bf16 / fp32 have the range.
// The caller's guidance scale is NOT part of what the backward schedule carries (it is linear in it): in_conv_bw applies it in fp32,
// so neither a very large --classifier-scale can overflow fp16 nor a very small one push the gradients into its subnormals.
float grad_scale(int precision) { return precision == VQVS_PREC_F16 ? 1024.0f : 1.0f; }

class Builder {
 public:
  Builder(vqvs_model* m, const float* const* hp) : m_(m), hp_(hp) {
    for (size_t i = 0; i < m->params.size(); ++i) pidx_[m->params[i].name] = (int)i;
    es_ = m->cfg.precision == VQVS_PREC_F32 ? 4 : 2;
    maxB_ = m->cfg.max_batch;
    maxL_ = m->cfg.max_T;
    ws_f32_kind = m->cfg.kind == VQVS_KIND_PREDICTOR || m->cfg.kind == VQVS_KIND_RESBLOCK || m->cfg.kind == VQVS_KIND_PREDICTOR_GRAD;
  }
  // fp32 mode: may the convolutions added from here on run on conv_ws_kernel's fp32 form?  The forward of a predictor-gradient handle
  // must (its prediction is the predictor handle's bit for bit); its backward phase turns this off and runs where the guidance
  // schedules' transposed convolutions run.
  bool ws_f32_kind = false;

  const float* P(const std::string& name) const {
    auto it = pidx_.find(name);
    if (it == pidx_.end()) return nullptr;
    return hp_[it->second];
  }
  // [rows][cols] host matrix uploaded as [cols][rows]
  size_t blob_f32_transposed(const float* w, int rows, int cols) {
    std::vector<float> t((size_t)rows * cols);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) t[(size_t)c * rows + r] = w[(size_t)r * cols + c];
    return blob.add(t.data(), t.size() * 4);
  }
  size_t blob_f32(const std::string& name) {
    auto it = pidx_.find(name);
    return blob.add(hp_[it->second], m_->params[it->second].numel() * 4);
  }

  // ---- arena planning -------------------------------------------------------------
  TensorH new_tensor(int C, int lshift, bool f32, bool stats) {
    TensorH t;
    t.id = next_id_++;
    t.C = C;
    t.lshift = lshift;
    t.f32 = f32;
    const size_t bytes = ((size_t)maxB_ * shiftL(maxL_, lshift) * C * (f32 ? 4 : es_) + 255) & ~(size_t)255;
    t.off = arena_alloc(bytes);
    sizes_[t.id] = bytes;
    offs_[t.id] = t.off;
    refs_[t.id] = 1;
    if (stats) {
      t.has_stats = true;
      t.stats_off = stats_floats;
      stats_floats += (size_t)maxB_ * ntiles_of(shiftL(maxL_, lshift), MIN_TILE_ROWS) * C * 2;
      tile_rows_[t.id] = STAT_TILE;
    }
    return t;
  }
  int stat_rows(const TensorH& t) const { return tile_rows_.at(t.id); }
  void retain(const TensorH& t) { refs_[t.id]++; }
  void release(const TensorH& t) {
    if (persist) return;  // forward tensors of a model with a backward pass stay resident
    if (--refs_[t.id] == 0 && !m_->cfg.debug_taps) arena_free(offs_[t.id], sizes_[t.id]);
  }
  bool persist = false;
  size_t alloc_stats(int C, int lshift) {
    const size_t off = stats_floats;
    stats_floats += (size_t)maxB_ * ntiles_of(shiftL(maxL_, lshift), MIN_TILE_ROWS) * C * 2;
    return off;
  }
  // what the backward pass needs to know about one forward ResBlock
  struct BlockRec {
    BlockSpec s;
    TensorH x, x2, h1, out;  // x2: the skip-stack tensor of a concatenating block (id < 0 otherwise)
    size_t ss1 = 0, ss2 = 0, mr1 = 0, mr2 = 0;
  };
  size_t alloc_ss(int C) {
    const size_t off = ss_floats;
    ss_floats += (size_t)maxB_ * C * 2;
    return off;
  }
  size_t alloc_misc(size_t floats) {
    const size_t off = misc_floats;
    misc_floats += (floats + 63) & ~(size_t)63;
    return off;
  }
  // the handle's device status word (range guard of gn_prepare; read and cleared by vqvs_model_status)
  size_t status_off() {
    if (status_off_ == (size_t)-1) {
      status_off_ = alloc_misc(64);
      m_->status_misc_off = status_off_;
    }
    return status_off_;
  }
  size_t status_off_ = (size_t)-1;

  // ---- ops ---------------------------------------------------------------------------
  // The one place a schedule entry is made: its accounting row, its function and its phase go in together (run_model, vqvs_op_info and
  // vqvs_profile_read index all three with one number).  `fn` itself becomes the std::function: nothing is wrapped around it.
  // Phase 0 entries always run; phase 1 entries (a backward schedule) only when the call asks for them.
  int phase = 0;
  template <class F>
  void op(const std::string& kind, const std::string& desc, double elems_T, double bytes_f32, double flops, F fn) {
    m_->meta.push_back({kind, desc, elems_T, bytes_f32, flops});
    m_->ops.emplace_back(std::move(fn));
    m_->op_phase.push_back((uint8_t)phase);
  }

  // A GroupNorm whose only consumer is the prologue of ONE convolution can be built by that convolution's producers (conv_ws.hip
  // WsGn): the link lets the two schedule entries agree at run time -- `fused` (set by add_conv) says whether the convolution
  // takes it for this batch / length, in which case the gn_prepare entry does nothing.
  struct GnLink {
    std::function<bool(const RunCtx&)> fused;
    std::function<void(const RunCtx&, GnArgs&)> fill;
  };
  // Where one block's FiLM rows (a | b) lie: the [max_batch][stride] table of all blocks' rows in the misc region, and the block's
  // first row in it.  A GroupNorm without FiLM (GroupNorm 1, the encoder's blocks, the heads) is given none.
  struct FilmRows {
    size_t misc_off = 0;
    int off = 0, stride = 0;
  };
  // A GroupNorm's coefficient tables in the ss region: (scale, shift), and (mean, rstd) where a backward schedule wants them kept
  struct GnTables {
    size_t ss = 0, mr = 0;
    bool want_mr = false;
  };
  GnTables alloc_gn_tables(int C, bool want_mr) {
    GnTables t;
    t.ss = alloc_ss(C);
    t.mr = want_mr ? alloc_ss(C) : 0;
    t.want_mr = want_mr;
    return t;
  }
  std::shared_ptr<GnLink> add_gn(const std::vector<TensorH>& srcs, const std::string& gn_name, const std::optional<FilmRows>& film,
                                 const GnTables& tb) {
    const FilmRows fr = film.value_or(FilmRows{});
    int Ctot = 0;
    for (auto& s : srcs) Ctot += s.C;
    const size_t g_off = blob_f32(gn_name + ".weight");
    const size_t b_off = blob_f32(gn_name + ".bias");
    // (a padded handle: the reference's groups and counts follow the REAL width, see pad_map)
    const int Creal = (int)((long long)Ctot * real_base(m_->cfg) / m_->cfg.base_channels);
    const int groups = gn_groups(Creal);
    const int lshift = srcs[0].lshift;
    const vqvs_model* const m = m_;
    std::vector<TensorH> S = srcs;
    std::vector<int> SR;
    for (auto& t : srcs) SR.push_back(stat_rows(t));
    const size_t st_off = status_off();
    const int guard = m_->cfg.precision == VQVS_PREC_F16 ? 1 : 0;
    auto link = std::make_shared<GnLink>();
    link->fill = [=](const RunCtx& c, GnArgs& a) {
      const int L = shiftL(c.Lbase, lshift);
      a.nsrc = (int)S.size();
      for (int i = 0; i < a.nsrc; ++i) a.src[i] = GnSrc{m->statp(S[i].stats_off), ntiles_of(L, SR[i]), S[i].C};
      a.Ctot = Ctot;
      a.groups = groups;
      a.inv_count = 1.0 / ((double)(Creal / groups) * (double)L);
      a.gamma = m->wf(g_off);
      a.beta = m->wf(b_off);
      a.film = film ? m->miscp(fr.misc_off) : nullptr;
      a.film_stride = fr.stride;
      a.film_off = fr.off;
      a.ss = m->ssf2(tb.ss);
      a.mr = tb.want_mr ? m->ssf2(tb.mr) : nullptr;
      a.status = reinterpret_cast<unsigned*>(m->miscp(st_off));
      a.guard = guard;
    };
    if (m_->cfg.debug_taps) {  // (read-only record for vqvs_debug_gn_*: nothing the schedule runs depends on it)
      GnDef d;
      d.name = gn_name;
      d.srcs = S;
      d.tile_rows = SR;
      for (auto& t : srcs) {
        std::function<bool(const RunCtx&)> f = [](const RunCtx&) { return true; };  // (ntc_stats_kernel reads the tensor back)
        if (sums_stored_.count(t.id)) f = sums_stored_.at(t.id);
        d.sums_stored.push_back(f);
      }
      d.Ctot = Ctot;
      d.groups = groups;
      d.cpg_real = Creal / groups;
      d.lshift = lshift;
      d.film = film.has_value();
      d.film_off = fr.off;
      d.film_stride = fr.stride;
      d.ss_off = tb.ss;
      d.mr_off = tb.mr;
      d.has_mr = tb.want_mr;
      d.fused = [link](const RunCtx& c) { return link->fused && link->fused(c); };
      d.fill = [link](const RunCtx& c, GnArgs& a) { link->fill(c, a); };
      m_->gns.push_back(std::move(d));
    }
    op("gn_prepare", gn_name + " C=" + std::to_string(Ctot) + " L>>" + std::to_string(lshift), 0, 0, 0, [=](const RunCtx& c) -> int {
      if (link->fused && link->fused(c)) return 0;
      GnArgs a{};
      link->fill(c, a);
      return launch_gn_prepare(a, c.B, c.st);
    });
    return link;
  }

  // g = gelu(GN(x)) [avg-pooled] written once (deep levels, see XformArgs)
  TensorH add_xform(const TensorH& src, size_t ss_off, int ss_stride, int ss_c0, bool avg) {
    TensorH g = new_tensor(src.C, src.lshift + (avg ? 1 : 0), false, false);
    const vqvs_model* const m = m_;
    const int prec = m_->cfg.precision;
    const TensorH S = src;
    if (m_->cfg.debug_taps) {
      XformDef d;
      d.in = src;
      d.out = g;
      d.avg = avg;
      d.ss_stride = ss_stride;
      d.ss_c0 = ss_c0;
      for (size_t i = 0; i < m_->gns.size(); ++i)
        if (m_->gns[i].ss_off == ss_off) d.gn = (int)i;
      m_->xforms.push_back(d);
    }
    op("xform", "C=" + std::to_string(src.C) + " L>>" + std::to_string(g.lshift) + (avg ? " avg" : ""),
       src.C * (lscale(src.lshift) + lscale(g.lshift)), 0, 0, [=](const RunCtx& c) -> int {
      XformArgs a{};
      a.in = m->act(S.off);
      a.ss = m->ssf2(ss_off);
      a.out = m->act(g.off);
      a.C = S.C;
      a.Lin = shiftL(c.Lbase, S.lshift);
      a.Lout = shiftL(c.Lbase, g.lshift);
      a.avg = avg ? 1 : 0;
      a.ss_stride = ss_stride;
      a.ss_c0 = ss_c0;
      return launch_xform(a, c.B, prec, c.st);
    });
    return g;
  }

  // One source of a convolution: channels [c0, c0 + C) of `t` through `ntaps` taps.  Made by raw_seg / norm_seg; what differs from
  // the defaults is then set by name.
  struct SegSpec {
    TensorH t;
    int c0 = 0, C = 0, ntaps = 3, dil = 1, resize = RESIZE_NONE;
    bool xform = false;  // the rows go through the GroupNorm + GELU prologue: (scale, shift) rows of ss_stride channels at ss_off (ss
    size_t ss_off = 0;   // region), of which this source's begin at channel ss_c0
    int ss_stride = 0, ss_c0 = 0;
    long long w_off = 0;  // where PackedConv::append put its weights
    // two-tensor affine prologue (kernels.hpp SegDesc.src2): staged row = P * t + Q * t2 + R with (P, Q, R, 0) rows at coef_off (misc region)
    bool aff2 = false;
    TensorH t2{};
    size_t coef_off = 0;
  };
  // every channel of `t`, read as stored ...
  static SegSpec raw_seg(const TensorH& t) {
    SegSpec g;
    g.t = t;
    g.C = t.C;
    return g;
  }
  // ... or normalised on the way in by the table `ss_off`, whose rows are ss_stride channels wide and hold `t` from channel ss_c0 on
  static SegSpec norm_seg(const TensorH& t, size_t ss_off, int ss_stride, int ss_c0 = 0) {
    SegSpec g = raw_seg(t);
    g.xform = true;
    g.ss_off = ss_off;
    g.ss_stride = ss_stride;
    g.ss_c0 = ss_c0;
    return g;
  }

  // GELU backward fused into a transposed convolution's epilogue (kernels.hpp BwActFuse): forward tensors covering the output
  // channels in order, the forward (scale, shift) table and the partial-sum block the GroupNorm backward reads
  struct BwFuse {
    std::vector<TensorH> xf;
    size_t ss_off;
    int ss_stride;
    size_t part_off;
  };
  static bool bw_fuse_enabled() {
    static int v = -1;
    if (v < 0) {
      const char* e = getenv("VQVS_BW_FUSE");  // 0: keep the separate bw_act kernel (A/B measurements)
      v = e ? atoi(e) : 1;
    }
    return v != 0;
  }

  // One convolution entry: out = bias + sum over segs [+ skip].  The weights are appended to `pk` segment by segment as `segs` is filled.
  struct ConvSpec {
    explicit ConvSpec(int precision) : pk(precision) {}
    std::vector<SegSpec> segs;
    PackedConv pk;
    std::vector<float> bias;
    int Cout = 0;
    TensorH out;
    std::optional<TensorH> skip;       // identity skip added in the epilogue, read through skip_resize
    int skip_resize = RESIZE_NONE;
    std::optional<int> out_lshift;     // logical output length where it differs from the allocation of `out` (padding rows)
    bool epi_gelu = false;             // out = skip + gelu(acc)
    std::optional<BwFuse> fuse;
    std::shared_ptr<GnLink> gn;        // the GroupNorm of the prologue, where this convolution may build its table itself
  };
  ConvSpec conv_spec(int Cout, const TensorH& out) const {
    ConvSpec cv(m_->cfg.precision);
    cv.Cout = Cout;
    cv.out = out;
    return cv;
  }
  // Returns the rows per workgroup tile (= rows per statistics / partial-sum tile of the output).
  int add_conv(const ConvSpec& cv) {
    // (what the entries below capture is copied out of the spec: they outlive it, and must not carry its packed weights)
    const std::vector<SegSpec>& segs = cv.segs;
    const TensorH& out = cv.out;
    const int Cout = cv.Cout, skip_resize = cv.skip_resize, out_lshift = cv.out_lshift.value_or(out.lshift);
    const bool epi_gelu = cv.epi_gelu;
    const std::shared_ptr<GnLink> gn = cv.gn;
    const size_t hi_off = blob.add(cv.pk.hi.data(), cv.pk.hi.size() * 2);
    const size_t lo_off = m_->cfg.precision == VQVS_PREC_F32 ? blob.add(cv.pk.lo.data(), cv.pk.lo.size() * 2) : 0;
    const size_t bias_off = blob.add(cv.bias.data(), cv.bias.size() * 4);
    const long long w_bytes = (long long)cv.pk.hi.size() * 2;
    const bool x3 = m_->cfg.precision == VQVS_PREC_F32;
    const int prec = m_->cfg.precision;
    const vqvs_model* const m = m_;
    std::vector<SegSpec> S = segs;
    const TensorH O = out;
    const bool has_skip = cv.skip.has_value();
    const TensorH K = cv.skip.value_or(TensorH{});
    int dmax = 0;
    for (auto& g : segs)
      if (g.ntaps == 3 && g.dil > dmax) dmax = g.dil;
    int kchunks = has_skip ? 2 : 0;  // (K chunks of 32 channels per tile: a one-chunk tile is only covered at 32 output channels)
    for (auto& g : segs) kchunks += g.C / 32;
    bool ws_ok = !out.f32 && !epi_gelu && !cv.fuse && !cv.out_lshift && kchunks >= 2;
    for (auto& g : segs) ws_ok = ws_ok && !g.aff2;  // (conv_mfma_kernel's two-tensor prologue)
    if (m_->cfg.precision == VQVS_PREC_F32) {
      // fp32 storage: a tile geometry other than the default one may only be chosen where conv_ws_kernel is certain to take the
      // launch (conv_mfma_kernel has one geometry): its fp32 form has no avg-pooled sources, wants 32-channel chunks, and
      // addresses a clip's rows through 32-bit descriptors -- checked here against the model's largest clip
      const bool kind_ok = ws_f32_kind;
      bool ok = kind_ok && Cout % 64 == 0 && !(has_skip && skip_resize == RESIZE_AVG2);
      auto clip_bytes = [&](const TensorH& t) { return (long long)shiftL(m_->cfg.max_T, t.lshift) * t.C * 4; };
      for (auto& g : segs) ok = ok && g.resize != RESIZE_AVG2 && g.C % 32 == 0 && (g.ntaps == 1 || g.ntaps == 3) && clip_bytes(g.t) < (1LL << 29);
      if (has_skip) ok = ok && K.C == Cout && clip_bytes(K) < (1LL << 29);
      ok = ok && clip_bytes(out) < (1LL << 31);
      ws_ok = ws_ok && ok;
    }
    const int tile_rows = conv_tile_rows(dmax, Cout, m_->cfg.precision, ws_ok);
    if (out.has_stats) tile_rows_[out.id] = tile_rows;
    // cost
    double ktot = 0;
    double conv_elems = 0, conv_f32 = 0;
    for (auto& s : segs) {
      conv_elems += s.C * lscale(s.t.lshift) * (s.aff2 ? 2 : 1);
      ktot += (double)s.C * s.ntaps;
    }
    if (has_skip) conv_elems += K.C * lscale(K.lshift);
    if (cv.fuse) conv_elems += Cout * lscale(out.lshift);  // the forward tensor(s) read by the fused GELU backward
    const bool has_fuse = cv.fuse.has_value();
    const BwFuse F = cv.fuse.value_or(BwFuse{});
    if (out.f32) conv_f32 += 4.0 * Cout * lscale(out.lshift);
    else conv_elems += Cout * lscale(out.lshift);
    const double conv_flops = 2.0 * Cout * ktot * lscale(out.lshift);
    std::string desc;
    for (auto& s : segs) desc += (desc.empty() ? "" : "+") + std::to_string(s.C) + "x" + std::to_string(s.ntaps) + (s.resize == RESIZE_AVG2 ? "v" : s.resize == RESIZE_UP2 ? "^" : "") + (s.ntaps == 3 && s.dil > 1 ? "d" + std::to_string(s.dil) : "");
    desc += "->" + std::to_string(Cout) + " L>>" + std::to_string(out.lshift) + (has_skip ? " +id" : "");
    const int ws_f32 = ws_f32_kind ? 1 : 0;
    const int rev = (conv_seq_++) & 1;  // consecutive convolutions walk their tiles in opposite directions (ConvArgs.rev)
    auto build = [=](const RunCtx& c, ConvArgs& a) {
      a.nseg = (int)S.size();
      for (int i = 0; i < a.nseg; ++i) {
        SegDesc& g = a.seg[i];
        g.src = m->act(S[i].t.off);
        g.ss = S[i].xform ? m->ssf2(S[i].ss_off) : nullptr;
        g.w_off = S[i].w_off;
        g.Csrc = S[i].t.C;
        g.c0 = S[i].c0;
        g.C = S[i].C;
        g.Lsrc = shiftL(c.Lbase, S[i].t.lshift);
        g.ntaps = S[i].ntaps;
        g.dil = S[i].dil;
        g.resize = S[i].resize;
        g.ss_stride = S[i].ss_stride;
        g.ss_c0 = S[i].ss_c0;
        if (S[i].aff2) {
          g.src2 = m->act(S[i].t2.off);
          g.coef = reinterpret_cast<const float4*>(m->miscp(S[i].coef_off));
          g.coef_stride = S[i].C;
          g.coef_c0 = 0;
        }
      }
      a.w_hi = reinterpret_cast<const bf16_t*>(m->wp(hi_off));
      a.w_lo = x3 ? reinterpret_cast<const bf16_t*>(m->wp(lo_off)) : nullptr;
      a.w_bytes = w_bytes;
      a.bias = m->wf(bias_off);
      a.Cout = Cout;
      a.Lout = shiftL(c.Lbase, out_lshift);
      a.out_rows = shiftL(c.Lbase, O.lshift);
      a.epi_gelu = epi_gelu ? 1 : 0;
      if (has_skip) {
        a.skip = m->act(K.off);
        a.skip_C = K.C;
        a.skip_L = shiftL(c.Lbase, K.lshift);
        a.skip_resize = skip_resize;
      }
      a.out = m->act(O.off);
      a.out_f32 = O.f32 ? 1 : 0;
      a.stats = O.has_stats ? m->statp(O.stats_off) : nullptr;
      a.ntiles = ntiles_of(a.Lout, tile_rows);
      a.tile_rows = tile_rows;
      a.rev = rev;
      a.ws_f32 = ws_f32;
      if (has_fuse) {
        a.nbw = (int)F.xf.size();
        int c0 = 0;
        for (int i = 0; i < a.nbw; ++i) {
          a.bw[i] = BwActFuse{m->act(F.xf[i].off), F.xf[i].C, c0};
          c0 += F.xf[i].C;
        }
        a.bw_ss = m->ssf2(F.ss_off);
        a.bw_ss_stride = F.ss_stride;
        a.stats = m->statp(F.part_off);
      }
    };
    // The launch at this (B, L), as all three users below see it: `a` with the GroupNorm `g` of link `gl` hung in where
    // conv_ws_kernel builds the table itself (otherwise the gn_prepare entry before this one has run)
    auto launch_args = [=](const RunCtx& c, ConvArgs& a, GnArgs& g, const GnLink* gl) {
      build(c, a);
      if (!gl) return;
      gl->fill(c, g);
      a.gn = &g;
      if (!ws_fuses_gn(a, c.B, prec)) a.gn = nullptr;
    };
    if (gn) {
      GnLink* const gl = gn.get();  // (`fused` is stored INSIDE the link: holding the shared_ptr there would be a cycle)
      gl->fused = [=](const RunCtx& c) -> bool {
        ConvArgs a{};
        GnArgs g{};
        launch_args(c, a, g, gl);
        return a.gn != nullptr;
      };
    }
    if (m_->cfg.debug_taps && out.has_stats)  // (for vqvs_debug_gn_info: which kernel this launch's statistics come from)
      sums_stored_[out.id] = [=](const RunCtx& c) -> bool {
        if (x3) return true;  // (float32 storage: the accumulators are what is stored)
        ConvArgs a{};
        GnArgs g{};
        launch_args(c, a, g, gn.get());
        return ws_takes(a, c.B, prec);
      };
    op("conv", desc, conv_elems, conv_f32, conv_flops, [=](const RunCtx& c) -> int {
      ConvArgs a{};
      GnArgs g{};
      launch_args(c, a, g, gn.get());
      return launch_conv(a, c.B, prec, c.st);
    });
    return tile_rows;
  }

  // One reference ResBlock (unet.py:248-316).  `ins` = 1 tensor, or 2 for torch.cat([h, skip], 1).
  // film: this block's (a | b) rows, none for a block without an embedding (the encoder's).  rec: filled for a backward schedule,
  // which also keeps the (mean, rstd) tables.
  TensorH resblock(const std::string& p, const BlockSpec& s, const std::vector<TensorH>& ins, const std::optional<FilmRows>& film,
                   BlockRec* rec = nullptr) {
    const std::string pre = p.empty() ? "" : p + ".";
    const int cin = s.cin, cout = s.cout;
    const int in_shift = ins[0].lshift;
    const int out_shift = in_shift + (s.resize == RESIZE_AVG2 ? 1 : (s.resize == RESIZE_UP2 ? -1 : 0));
    // Prologue hoisted into its own kernel (the convolution then reads transformed rows raw):
    //  - fp32 mode (conv_mfma_kernel: every channel-tile workgroup repeats the prologue of the same input rows): from 4 tiles up;
    //  - 2-byte modes (conv_ws_kernel: the producers' prologue runs beside the MFMAs, measured cheaper than the extra pass from
    //    512 channels too): only where the per-clip (scale, shift) table of the launch does not fit the CU's LDS next to the
    //    tiles -- conv 1 over a concatenated input of more than 640 channels (768 and 1024 in the UNets).
    static const int pre_xform_min = getenv("VQVS_PRE_XFORM_MIN") ? atoi(getenv("VQVS_PRE_XFORM_MIN")) : 0;  // (A/B: > 0 = hoist from this Cout up, both convs)
    const bool two_byte = m_->cfg.precision != VQVS_PREC_F32;
    const bool pre_xform1 = pre_xform_min > 0 ? cout >= pre_xform_min : (two_byte ? cin > 640 : cout >= 512);  // (2 x 8 B x cin of table beside the tiles)
    const bool pre_xform2 = pre_xform_min > 0 ? cout >= pre_xform_min : (two_byte ? false : cout >= 512);
    // GroupNorm 1 coefficients over the (virtually concatenated) input
    const GnTables t1 = alloc_gn_tables(cin, rec != nullptr);
    const size_t ss1 = t1.ss, mr1 = t1.mr;
    // (a model with a backward pass keeps every table in memory: no fusion there)
    auto gn1 = add_gn(ins, pre + "pre_cond.0.0", std::nullopt, t1);
    const bool fuse_gn = rec == nullptr && two_byte;
    // conv 1
    TensorH h1 = new_tensor(cout, out_shift, false, true);
    {
      ConvSpec cv = conv_spec(cout, h1);
      const float* W = P(pre + "pre_cond.2.weight");
      int cb = 0;
      std::vector<TensorH> tmp;
      for (auto& t : ins) {
        SegSpec g = norm_seg(t, ss1, cin, cb);
        g.resize = s.resize;
        if (pre_xform1) {  // prologue hoisted out of the GEMM: the conv reads g raw
          g.t = add_xform(t, ss1, cin, cb, s.resize == RESIZE_AVG2);
          g.xform = false;
          if (s.resize == RESIZE_AVG2) g.resize = RESIZE_NONE;
          tmp.push_back(g.t);
        }
        g.w_off = cv.pk.append(W, cout, cin, 3, cb, t.C);
        cv.segs.push_back(g);
        cb += t.C;
      }
      const float* b = P(pre + "pre_cond.2.bias");
      cv.bias.assign(b, b + cout);
      if (fuse_gn && !pre_xform1) cv.gn = gn1;
      add_conv(cv);
      for (auto& t : tmp) release(t);
    }
    // GroupNorm 2 (+FiLM) coefficients
    const GnTables t2 = alloc_gn_tables(cout, rec != nullptr);
    const size_t ss2 = t2.ss, mr2 = t2.mr;
    auto gn2 = add_gn({h1}, pre + "pre_cond.3", film, t2);
    // conv 2 + skip
    TensorH out = new_tensor(cout, out_shift, false, true);
    {
      ConvSpec cv = conv_spec(cout, out);
      if (fuse_gn && !pre_xform2) cv.gn = gn2;
      const std::string c2 = pre + (cfg_dropout(m_->cfg) ? "post_cond.2" : "post_cond.1");
      const float* W = P(c2 + ".weight");
      const float* b = P(c2 + ".bias");
      std::vector<float>& bias = cv.bias;
      bias.assign(b, b + cout);
      SegSpec g = norm_seg(h1, ss2, cout);
      g.dil = s.dil;
      TensorH g2{};
      if (pre_xform2) {
        g2 = add_xform(h1, ss2, cout, 0, false);
        g.t = g2;
        g.xform = false;
      }
      g.w_off = cv.pk.append(W, cout, cout, 3, 0, cout);
      cv.segs.push_back(g);
      if (cin != cout) {  // 1x1 skip conv folded into the same GEMM as raw 1-tap segments
        const float* Ws = P(pre + "skip.1.weight");
        const float* bs = P(pre + "skip.1.bias");
        for (int i = 0; i < cout; ++i) bias[i] += bs[i];
        int cb = 0;
        for (auto& t : ins) {
          SegSpec r = raw_seg(t);
          r.ntaps = 1;
          r.w_off = cv.pk.append(Ws, cout, cin, 1, cb, t.C);
          cv.segs.push_back(r);
          cb += t.C;
        }
      } else {  // identity skip (never together with a concatenated input in this topology)
        cv.skip = ins[0];
        cv.skip_resize = s.resize;
      }
      add_conv(cv);
      if (pre_xform2) release(g2);
    }
    release(h1);
    if (rec) *rec = BlockRec{s, ins[0], ins.size() > 1 ? ins[1] : TensorH{}, h1, out, ss1, ss2, mr1, mr2};
    return out;
  }

  // ---- backward pieces (classifier guidance) ------------------------------------------------------
  // slice [c0, c0 + xf.C) of the (possibly wider) gradient tensor `t` / output `du`; statistics into columns
  // [c0, c0 + xf.C) of a partials block that is Ctot channels wide
  void add_bw_act(const TensorH& t, int resize, const TensorH& xf, size_t ss_off, const TensorH& du, size_t part_off, int c0 = 0,
                  int Ctot = 0) {
    const vqvs_model* const m = m_;
    const int prec = m_->cfg.precision;
    if (Ctot == 0) Ctot = xf.C;
    op("bw_act", "C=" + std::to_string(xf.C) + " L>>" + std::to_string(xf.lshift) +
                     (resize == BW_FROM_HALF ? " from L/2" : resize == BW_FROM_DOUBLE ? " from 2L" : ""),
       xf.C * (2 * lscale(xf.lshift) + lscale(t.lshift)), 0, 0, [=](const RunCtx& c) -> int {
      BwActArgs a{};
      a.t = m->act(t.off);
      a.xf = m->act(xf.off);
      a.ss = m->ssf2(ss_off);
      a.du = m->act(du.off);
      a.partials = m->statp(part_off);
      a.C = xf.C;
      a.L = shiftL(c.Lbase, xf.lshift);
      a.resize = resize;
      a.t_C = t.C;
      a.t_c0 = t.C == xf.C ? 0 : c0;
      a.du_C = du.C;
      a.du_c0 = du.C == xf.C ? 0 : c0;
      a.ss_stride = Ctot;
      a.ss_c0 = c0;
      a.part_C = Ctot;
      a.part_c0 = c0;
      return launch_bw_act(a, c.B, prec, c.st);
    });
  }
  size_t add_gn_bw(int C, int lshift, size_t part_off, size_t ss_off, size_t mr_off, int tile_rows = STAT_TILE) {
    const size_t coef = alloc_misc((size_t)maxB_ * C * 4);
    const vqvs_model* const m = m_;
    const int groups = gn_groups(C);
    op("gn_bw", "C=" + std::to_string(C) + " L>>" + std::to_string(lshift), 0, 0, 0, [=](const RunCtx& c) -> int {
      GnBwArgs a{};
      const int L = shiftL(c.Lbase, lshift);
      a.partials = m->statp(part_off);
      a.ntiles = ntiles_of(L, tile_rows);
      a.C = C;
      a.groups = groups;
      a.inv_count = 1.0 / ((double)(C / groups) * (double)L);
      a.ss = m->ssf2(ss_off);
      a.mr = m->ssf2(mr_off);
      a.coef = reinterpret_cast<float4*>(m->miscp(coef));
      return launch_gn_bw(a, c.B, c.st);
    });
    return coef;
  }
  // out = P*du + Q*xf + R (+ skip) (+ extra); du / extra / coef may be slices [c0, c0 + xf.C) of Ctot-wide buffers
  void add_bw_affine(const TensorH& du, const TensorH& xf, size_t coef, const TensorH* skip, int skip_mode, const TensorH* extra,
                     const TensorH& out, int c0 = 0, int Ctot = 0) {
    const vqvs_model* const m = m_;
    const int prec = m_->cfg.precision;
    if (Ctot == 0) Ctot = xf.C;
    const bool has_skip = skip != nullptr, has_extra = extra != nullptr;
    const TensorH K = skip ? *skip : TensorH{}, E = extra ? *extra : TensorH{};
    op("bw_affine", "C=" + std::to_string(xf.C) + " L>>" + std::to_string(xf.lshift),
       xf.C * lscale(xf.lshift) * (3 + (has_extra ? 1 : 0)) + (has_skip ? K.C * lscale(K.lshift) : 0.0), 0, 0, [=](const RunCtx& c) -> int {
      BwAffineArgs a{};
      a.du = m->act(du.off);
      a.xf = m->act(xf.off);
      a.coef = reinterpret_cast<const float4*>(m->miscp(coef));
      a.skip = has_skip ? m->act(K.off) : nullptr;
      a.skip_mode = skip_mode;
      a.extra = has_extra ? m->act(E.off) : nullptr;
      a.out = m->act(out.off);
      a.C = xf.C;
      a.L = shiftL(c.Lbase, xf.lshift);
      a.du_C = du.C;
      a.du_c0 = du.C == xf.C ? 0 : c0;
      a.coef_stride = Ctot;
      a.coef_c0 = c0;
      a.extra_C = has_extra ? E.C : 0;
      a.extra_c0 = has_extra && E.C != xf.C ? c0 : 0;
      return launch_bw_affine(a, c.B, prec, c.st);
    });
  }
  void add_bw_add(const TensorH& x, const TensorH& y, const TensorH& out) {  // out = x + y (same shape)
    const vqvs_model* const m = m_;
    const int prec = m_->cfg.precision;
    op("bw_add", "C=" + std::to_string(x.C) + " L>>" + std::to_string(x.lshift), 3 * x.C * lscale(x.lshift), 0, 0, [=](const RunCtx& c) -> int {
      const long long n = (long long)c.B * shiftL(c.Lbase, x.lshift) * x.C;
      return launch_bw_add(m->act(x.off), m->act(y.off), m->act(out.off), n, prec, c.st);
    });
  }
  // plain convolution of a raw tensor with transposed weights (no prologue, no statistics, zero bias)
  // aff_xf / aff_coef: the source is read through the two-tensor affine prologue P * src + Q * aff_xf + R (GroupNorm's backward folded
  // into this convolution's staging instead of a bw_affine pass in front of it)
  int add_conv_t(const TensorH& src, const float* W, int Cout_fwd, int Cin_fwd, int ktaps, int dil, const TensorH& out,
                 const BwFuse* fuse = nullptr, const TensorH* aff_xf = nullptr, size_t aff_coef = 0) {
    const std::vector<float> Wt = transpose_flip(W, Cout_fwd, Cin_fwd, ktaps);
    ConvSpec cv = conv_spec(Cin_fwd, out);
    SegSpec g = raw_seg(src);
    g.C = Cout_fwd;
    g.ntaps = ktaps;
    g.dil = dil;
    if (aff_xf) {
      g.aff2 = true;
      g.t2 = *aff_xf;
      g.coef_off = aff_coef;
    }
    g.w_off = cv.pk.append(Wt.data(), Cin_fwd, Cout_fwd, ktaps, 0, Cout_fwd);
    cv.segs.push_back(g);
    cv.bias.assign(Cin_fwd, 0.f);
    if (fuse) cv.fuse = *fuse;
    return add_conv(cv);
  }

  // Gradient of one ResBlock with respect to its input(s):
  //   out = skip(resize(x)) + conv2(gelu(GN2(conv1(resize(gelu(GN1(x)))))))       (unet.py:307-316)
  // x may be the concatenation [x, x2] (up path, unet.py:156).  Consumes `dout` (released); returns dx and sets
  // *dx2 to the gradient of the second input when the block concatenates.
  // on_du2 (predictor-gradient handles; empty for the guidance schedules): called once du2 = conv2^T(dout) * gelu'(u2) exists and
  // before anything overwrites or releases it -- where the FiLM-coefficient gradient of the block is reduced.  input_grad = false: the
  // block's input gradient is not wanted (the first block of such a handle): everything behind du2 is left out and an empty handle
  // is returned.  A concatenating block called without dx2 leaves the second input's gradient out.
  using Du2Hook = std::function<void(const BlockRec&, const TensorH&)>;
  TensorH resblock_backward(const BlockRec& r, const TensorH& dout, TensorH* dx2 = nullptr, bool input_grad = true, const Du2Hook& on_du2 = {}) {
    const BlockSpec& s = r.s;
    const std::string pre = s.prefix.empty() ? "" : s.prefix + ".";
    const int cin = s.cin, cout = s.cout;
    const int in_shift = r.x.lshift, out_shift = r.out.lshift;
    const bool cat = r.x2.id >= 0;
    // gradient at the input resolution from a tensor at the output resolution
    const int rs = s.resize == RESIZE_AVG2 ? BW_FROM_HALF : (s.resize == RESIZE_UP2 ? BW_FROM_DOUBLE : BW_SAME);
    // d gelu2 = conv2^T(dout);  du2 = . * gelu'(u2);  d h1 = GN2 backward
    TensorH t1 = new_tensor(cout, out_shift, false, false);
    const std::string c2 = pre + (cfg_dropout(m_->cfg) ? "post_cond.2" : "post_cond.1");
    const size_t pa = alloc_stats(cout, out_shift);
    const bool fuse = bw_fuse_enabled();  // the multiplication by gelu'(u) and its partial sums ride in the convolution's epilogue
    const BwFuse f2{{r.h1}, r.ss2, cout, pa};
    const int tr2 = add_conv_t(dout, P(c2 + ".weight"), cout, cout, 3, s.dil, t1, fuse ? &f2 : nullptr);
    if (!fuse) add_bw_act(t1, BW_SAME, r.h1, r.ss2, t1, pa);
    if (on_du2) on_du2(r, t1);
    if (!input_grad) {
      release(t1);
      release(dout);
      return TensorH{};
    }
    const size_t cf2 = add_gn_bw(cout, out_shift, pa, r.ss2, r.mr2, fuse ? tr2 : STAT_TILE);
    // d h1 = P * du2 + Q * h1 + R: evaluated by conv1^T while it stages its input (kernels.hpp SegDesc.src2) instead of a streaming
    // pass that writes d h1 and a convolution that reads it back.  VQVS_BW_AFF2=0: the separate bw_affine launch (A/B measurements).
    static const bool aff2 = getenv("VQVS_BW_AFF2") ? atoi(getenv("VQVS_BW_AFF2")) != 0 : true;
    if (!aff2) add_bw_affine(t1, r.h1, cf2, nullptr, BW_SAME, nullptr, t1);
    // d resize(gelu1) = conv1^T(d h1);  du1 = resize^T(.) * gelu'(u1);  dx = GN1 backward + skip path
    TensorH t2 = new_tensor(cin, out_shift, false, false);
    const size_t pb = alloc_stats(cin, in_shift);
    const bool fuse1 = fuse && rs == BW_SAME;  // (resizing blocks keep the separate kernel: their gradient changes resolution first)
    BwFuse f1{{r.x}, r.ss1, cin, pb};
    if (cat) f1.xf.push_back(r.x2);
    const int tr1 = add_conv_t(t1, P(pre + "pre_cond.2.weight"), cout, cin, 3, 1, t2, fuse1 ? &f1 : nullptr, aff2 ? &r.h1 : nullptr, cf2);
    release(t1);
    if (!cat) {
      TensorH du1 = rs != BW_SAME ? new_tensor(cin, in_shift, false, false) : t2;
      if (!fuse1) add_bw_act(t2, rs, r.x, r.ss1, du1, pb);
      if (rs != BW_SAME) release(t2);
      const size_t cf1 = add_gn_bw(cin, in_shift, pb, r.ss1, r.mr1, fuse1 ? tr1 : STAT_TILE);
      if (cin != cout) {
        TensorH t3 = new_tensor(cin, out_shift, false, false);
        add_conv_t(dout, P(pre + "skip.1.weight"), cout, cin, 1, 1, t3);
        add_bw_affine(du1, r.x, cf1, nullptr, BW_SAME, &t3, du1);
        release(t3);
      } else {
        add_bw_affine(du1, r.x, cf1, &dout, rs, nullptr, du1);
      }
      release(dout);
      return du1;
    }
    // concatenated input (never resized, always a 1x1 skip convolution): t2 and t3 are cin wide, the two sources
    // take their column slices; GroupNorm 1 runs over the concatenation
    const TensorH srcs[2] = {r.x, r.x2};
    int c0 = 0;
    for (int i = 0; i < 2 && !fuse1; ++i) {
      add_bw_act(t2, BW_SAME, srcs[i], r.ss1, t2, pb, c0, cin);
      c0 += srcs[i].C;
    }
    const size_t cf1 = add_gn_bw(cin, in_shift, pb, r.ss1, r.mr1, fuse1 ? tr1 : STAT_TILE);
    TensorH t3 = new_tensor(cin, out_shift, false, false);
    add_conv_t(dout, P(pre + "skip.1.weight"), cout, cin, 1, 1, t3);
    release(dout);
    TensorH outs[2];
    c0 = 0;
    for (int i = 0; i < (dx2 ? 2 : 1); ++i) {
      outs[i] = new_tensor(srcs[i].C, in_shift, false, false);
      add_bw_affine(t2, srcs[i], cf1, nullptr, BW_SAME, &t3, outs[i], c0, cin);
      c0 += srcs[i].C;
    }
    release(t2);
    release(t3);
    if (dx2) *dx2 = outs[1];
    return outs[0];
  }

  // The blocks of a whole UNet in reverse, from the gradient `g` of the last block's output.  Gradients of skip-stack tensors wait in
  // `pending` until the down path reaches their producer.  input_grad: return the gradient of recs[0].x (the in_conv output, which is
  // also the first skip-stack entry); otherwise neither it nor the skip gradient that would be added to it is computed.
  TensorH unet_backward(const std::vector<BlockRec>& recs, TensorH g, bool input_grad = true, const Du2Hook& on_du2 = {}) {
    std::map<int, TensorH> pending;
    auto add_pending = [&](const TensorH& produced) {  // produced = forward tensor whose gradient g currently is
      auto it = pending.find(produced.id);
      if (it == pending.end()) return;
      add_bw_add(g, it->second, g);
      release(it->second);
      pending.erase(it);
    };
    for (size_t i = recs.size(); i-- > 0;) {
      add_pending(recs[i].out);
      TensorH dsk{};
      const bool cat = recs[i].x2.id >= 0;
      const bool want_dsk = cat && (input_grad || recs[i].x2.id != recs[0].x.id);
      g = resblock_backward(recs[i], g, cat && !want_dsk ? nullptr : &dsk, input_grad || i > 0, on_du2);
      if (want_dsk) pending[recs[i].x2.id] = dsk;
    }
    if (input_grad) add_pending(recs[0].x);
    return g;
  }

  // ---- stem and head pieces shared by the kinds -------------------------------------------------------
  // (every piece allocates and uploads in a fixed order: blob offsets, arena offsets and the op list follow from it)
  struct TimeEmb {
    size_t emb_off, gemb_off;  // misc region: the conditioning vector [max_batch][E] and its GELU
    int E;
  };
  // Time embedding under `px` (unet.py:132-136; the classifier stem's is the same module, classifier.py:111-114): frequency table,
  // both linear layers, one kernel.  class_table: the kernel adds class_embed[labels] unless the call brings a vector per clip;
  // class_vec: a call may bring one (RunCtx.class_vec).
  TimeEmb time_embedding(const std::string& px, int num_labels, bool class_table, bool class_vec) {
    const vqvs_cfg& c = m_->cfg;
    const int E = 4 * c.base_channels;
    // wavegrad.py:361-369 (float32 tensor math) at the REAL embedding width 4 * real base; a padded handle keeps the real entries at
    // their physical positions (the halves of the embedding -- cos | sin -- are whole numbers of blocks), pad entries are 0 and meet
    // zero weight rows
    std::vector<float> freqs(E / 2, 0.0f);
    const int Er = 4 * real_base(c);
    const PadMap pm = pad_map(real_base(c));
    for (int i = 0; i < Er / 2; ++i)
      freqs[pm.phys(i)] = (float)(std::exp((double)(float)(-std::log(100.0 / 0.1)) * (double)i / (double)(Er / 2 - 1))) * 100.0f;
    const size_t freq_off = blob.add(freqs.data(), freqs.size() * 4);
    const size_t w1 = blob_f32_transposed(P(px + "time_embed.proj.weight"), E, E), b1 = blob_f32(px + "time_embed.proj.bias");
    const size_t w2 = blob_f32_transposed(P(px + "time_embed_extra.1.weight"), E, E), b2 = blob_f32(px + "time_embed_extra.1.bias");
    const size_t ce = class_table ? blob_f32(px + "class_embed.weight") : 0;
    const size_t emb_off = alloc_misc((size_t)maxB_ * E);
    const size_t gemb_off = alloc_misc((size_t)maxB_ * E);
    m_->emb_misc_off = emb_off;
    m_->emb_E = E;
    const vqvs_model* const m = m_;
    op("time_embed", "", 0, 0, 0, [=](const RunCtx& r) -> int {
      TimeEmbedArgs a{};
      a.ts = r.ts;
      a.freqs = m->wf(freq_off);
      a.w1 = m->wf(w1);
      a.b1 = m->wf(b1);
      a.w2 = m->wf(w2);
      a.b2 = m->wf(b2);
      // an explicit vector per clip (vqvs_unet_forward_vec, vqvs_unet_embed_grad) takes the table's place: the kernel adds one or the other
      a.class_embed = class_table && !r.class_vec ? m->wf(ce) : nullptr;
      a.labels = r.labels;  // (read beside class_embed only)
      a.class_vec = class_vec ? r.class_vec : nullptr;
      a.num_labels = num_labels;
      a.emb = m->miscp(emb_off);
      a.gemb = m->miscp(gemb_off);
      a.E = E;
      return launch_time_embed(a, r.B, r.st);
    });
    return {emb_off, gemb_off, E};
  }

  // The (a | b) rows of every block's cond_layers.1 stacked into one matrix: one kernel writes all blocks' FiLM rows [max_batch][R]
  struct Film {
    std::vector<int> row;  // first row of block i
    int R = 0;
    size_t wall_off = 0, film_off = 0;  // the stacked weights (transposed, weight blob) and the rows (misc region)
    FilmRows rows(size_t i) const {     // block i's
      FilmRows r;
      r.misc_off = film_off;
      r.off = row[i];
      r.stride = R;
      return r;
    }
  };
  Film film_table(const std::vector<BlockSpec>& blocks, int E, size_t gemb_off) {
    Film f;
    std::vector<float> Wall, ball;
    for (auto& s : blocks) {
      f.row.push_back(f.R);
      const float* W = P(s.prefix + ".cond_layers.1.weight");
      const float* bb = P(s.prefix + ".cond_layers.1.bias");
      const int rows = 2 * s.cout;
      Wall.insert(Wall.end(), W, W + (size_t)rows * E);
      ball.insert(ball.end(), bb, bb + rows);
      f.R += rows;
    }
    const int R = f.R;
    const size_t wall_off = f.wall_off = blob_f32_transposed(Wall.data(), R, E);
    const size_t ball_off = blob.add(ball.data(), ball.size() * 4);
    const size_t film_off = f.film_off = alloc_misc((size_t)maxB_ * R);
    m_->film_misc_off = film_off;
    m_->film_R = R;
    const vqvs_model* const m = m_;
    op("film", "", 0, 0, 0, [=](const RunCtx& r) -> int {
      FilmArgs a{m->miscp(gemb_off), m->wf(wall_off), m->wf(ball_off), m->miscp(film_off), E, R};
      return launch_film(a, r.B, r.st);
    });
    return f;
  }

  // in_conv (unet.py:49, 137-139): Conv1d(Cin -> base, 3) over the NCT input [+ the nearest-upsampled conditioning projection].
  // w_off: where the weights went in the blob, for a backward schedule's in_conv_bw.  row_cin: the input channels the accounting
  // row shows and counts (the encoder's row has always said one, whatever in_channels is: kept, the tables are compared entry by entry).
  TensorH in_conv(const std::string& px, int Cin, const TensorH* condp = nullptr, size_t* w_off = nullptr, int row_cin = 0) {
    if (row_cin == 0) row_cin = Cin;
    const int base = m_->cfg.base_channels, prec = m_->cfg.precision;
    const TensorH h = new_tensor(base, 0, false, true);
    const size_t w = blob_f32(px + "in_conv.weight"), bi = blob_f32(px + "in_conv.bias");
    if (w_off) *w_off = w;
    const bool has_cond = condp != nullptr;
    const TensorH cp = condp ? *condp : TensorH{};
    const vqvs_model* const m = m_;
    if (m_->cfg.debug_taps) sums_stored_[h.id] = [prec](const RunCtx&) { return prec == VQVS_PREC_F32; };
    op("in_conv", std::to_string(row_cin) + "->" + std::to_string(base), base + (has_cond ? base * lscale(cp.lshift) : 0.0), 4.0 * row_cin, 0,
       [=](const RunCtx& r) -> int {
      InConvArgs a{};
      a.x = r.x;
      a.Cin = Cin;
      a.w = m->wf(w);
      a.bias = m->wf(bi);
      a.condp = has_cond ? m->act(cp.off) : nullptr;
      a.cond_len = has_cond ? shiftL(r.Lbase, cp.lshift) : 0;
      a.out = m->act(h.off);
      a.stats = m->statp(h.stats_off);
      a.C = base;
      a.T = r.Lbase;
      a.ntiles = ntiles_of(r.Lbase);
      return launch_in_conv(a, r.B, prec, r.st);
    });
    return h;
  }
  // ... and its transpose, the last kernel of a guidance schedule: grad_out = (gscale / grad_scale) * in_conv^T(g)
  void in_conv_bw(const TensorH& g, size_t w_off) {
    const int base = m_->cfg.base_channels, prec = m_->cfg.precision;
    const vqvs_model* const m = m_;
    op("in_conv_bw", std::to_string(base) + "->1", (double)base, 4.0, 0, [=](const RunCtx& r) -> int {
      InConvBwArgs a{};
      a.dh = m->act(g.off);
      a.w = m->wf(w_off);
      a.out = r.grad_out;
      a.C = base;
      a.T = r.Lbase;
      a.out_scale = r.gscale / grad_scale(prec);
      return launch_in_conv_bw(a, r.B, prec, r.st);
    });
  }

  // Output heads begin with GroupNorm + GELU over the last block's output (unet.py:113-116, classifier.py:94): its coefficient
  // tables (mr: mean / rstd, kept for a backward schedule) and the gn_prepare entry
  GnTables head_gn(const TensorH& h, const std::string& gn_name, bool want_mr) {
    const GnTables g = alloc_gn_tables(h.C, want_mr);
    add_gn({h}, gn_name, std::nullopt, g);
    return g;
  }
  // ... followed, in the UNets, by a 3-tap convolution into a float32 boundary tensor
  TensorH head_conv(const TensorH& h, const GnTables& gh, const std::string& conv_name, int Cout, int out_lshift) {
    TensorH o = new_tensor(Cout, out_lshift, true, false);
    ConvSpec cv = conv_spec(Cout, o);
    SegSpec g = norm_seg(h, gh.ss, h.C);
    g.w_off = cv.pk.append(P(conv_name + ".weight"), Cout, h.C, 3, 0, h.C);
    cv.segs.push_back(g);
    const float* bb = P(conv_name + ".bias");
    cv.bias.assign(bb, bb + Cout);
    add_conv(cv);
    return o;
  }
  // the handle's output in the boundary's NCT layout
  void to_nct(const TensorH& o) {
    const int prec = o.f32 ? 0 : m_->cfg.precision;
    const vqvs_model* const m = m_;
    op("ntc_to_nct", "", 0, 0, 0, [=](const RunCtx& r) -> int {
      return launch_ntc_to_nct(m->act(o.off), r.out, r.B, o.C, shiftL(r.Lbase, o.lshift), prec, r.st);
    });
  }

  void tap(const std::string& name, const TensorH& t) { m_->taps.push_back({name, t}); }
  std::map<int, std::function<bool(const RunCtx&)>> sums_stored_;  // debug_taps handles: by tensor id (GnDef.sums_stored)

  // region sizes after planning
  size_t act_high = 0, stats_floats = 0, ss_floats = 0, misc_floats = 0;
  Blob blob;
  int es() const { return es_; }

 private:
  size_t arena_alloc(size_t bytes) {
    for (size_t i = 0; i < free_.size(); ++i) {
      if (free_[i].second >= bytes) {
        const size_t off = free_[i].first;
        if (free_[i].second == bytes) free_.erase(free_.begin() + i);
        else { free_[i].first += bytes; free_[i].second -= bytes; }
        return off;
      }
    }
    const size_t off = act_high;
    act_high += bytes;
    return off;
  }
  void arena_free(size_t off, size_t bytes) {
    free_.push_back({off, bytes});
    // coalesce
    std::sort(free_.begin(), free_.end());
    std::vector<std::pair<size_t, size_t>> merged;
    for (auto& f : free_) {
      if (!merged.empty() && merged.back().first + merged.back().second == f.first) merged.back().second += f.second;
      else merged.push_back(f);
    }
    // (a free block that ends at the high-water mark stays in the list: the arena's size is the maximum ever needed)
    free_ = merged;
  }

  vqvs_model* m_;
  const float* const* hp_;
  std::map<std::string, int> pidx_;
  int es_, maxB_, maxL_;
  int next_id_ = 0;
  int conv_seq_ = 0;
  std::map<int, size_t> sizes_, offs_;
  std::map<int, int> refs_;
  std::map<int, int> tile_rows_;  // rows per statistics tile of each tensor (set by its producer)
  std::vector<std::pair<size_t, size_t>> free_;
};

}  // namespace

int tensor_rows(int Lbase, int lshift) { return shiftL(Lbase, lshift); }

int unet_rate(const vqvs_cfg& c) {  // UNetPredictor / UNetEncoder.downsample_rate (unet.py:182-184, 243-245): 2^(len(channel_mult) - 1)
  return 1 << (topo_of(c).levels() - 1);
}

int gn_groups(int ch) {  // unet.py:345-349
  int g = 32;
  while (ch % g) g /= 2;
  return g;
}

int padded_base(int real) {
  const PadMap m = pad_map(real);
  return real / m.q * m.qp;
}
void pad_blocks(int real, int* q, int* qp) {
  const PadMap m = pad_map(real);
  *q = m.q, *qp = m.qp;
}
int real_base(const vqvs_cfg& c) {
  const bool unet = c.kind == VQVS_KIND_PREDICTOR || c.kind == VQVS_KIND_ENCODER;
  return unet && c.reserved[4] > 0 ? c.reserved[4] : c.base_channels;
}

static int check_topology(const vqvs_cfg& c) {
  if (c.topology_set && c.kind != VQVS_KIND_PREDICTOR && c.kind != VQVS_KIND_PREDICTOR_GRAD && c.kind != VQVS_KIND_ENCODER && c.kind != VQVS_KIND_CLASSIFIER)
    VQVS_FAIL(VQVS_ERR_ARG, "a custom topology is built for predictor, encoder and classifier handles only (kind %d)", c.kind);
  if (c.topology_set) {
    if (c.n_levels < 1 || c.n_levels > VQVS_MAX_LEVELS) VQVS_FAIL(VQVS_ERR_ARG, "n_levels must be in 1..%d (got %d)", VQVS_MAX_LEVELS, c.n_levels);
    for (int i = 0; i < c.n_levels; ++i)
      if (c.channel_mult[i] < 1 || c.channel_mult[i] * c.base_channels > 1024)
        VQVS_FAIL(VQVS_ERR_ARG, "channel_mult[%d] = %d: widths must be in base_channels..1024", i, c.channel_mult[i]);
    if (c.depth_mult < 1 || c.depth_mult > 8) VQVS_FAIL(VQVS_ERR_ARG, "depth_mult must be in 1..8 (got %d)", c.depth_mult);
    if (c.n_dilations < 0 || c.n_dilations > 12) VQVS_FAIL(VQVS_ERR_ARG, "at most 12 middle / output dilations (got %d)", c.n_dilations);
    for (int i = 0; i < c.n_dilations; ++i)
      if (c.dilations[i] < 1 || c.dilations[i] > 32) VQVS_FAIL(VQVS_ERR_ARG, "dilation %d is outside 1..32", c.dilations[i]);
    // Limits of the BUILDER, enforced here for every caller of the C ABI (the Python wrappers raise the same errors earlier):
    // * predictor: the output head (out.0.0 GroupNorm + out.1 conv, unet.py:113-116) is built for base_channels, the last up block
    //   returns channel_mult[0] * base_channels -- the reference constructs such a model and fails in forward;
    // * classifier: the attention pool splits the final width into heads of 64 channels (classifier.py:131-150 asserts the same).
    if ((c.kind == VQVS_KIND_PREDICTOR || c.kind == VQVS_KIND_PREDICTOR_GRAD) && c.channel_mult[0] != 1)
      VQVS_FAIL(VQVS_ERR_ARG, "predictor channel_mult[0] must be 1 (got %d): the output head is built for base_channels", c.channel_mult[0]);
    if (c.kind == VQVS_KIND_CLASSIFIER) {
      const int cur = c.channel_mult[c.n_levels - 1] * c.base_channels;
      if (cur > 64 && cur % 64)
        VQVS_FAIL(VQVS_ERR_ARG, "classifier: the final width %d must be at most 64 or a multiple of 64 (attention heads of 64 channels)", cur);
    }
  }
  return 0;
}

// elements of the widest per-clip tensor a launch may address: level i holds max_T / 2^i rows of channel_mult[i] * base channels, and a
// concatenated input (the predictor's up path) is twice that wide.  (The default topology: max_T rows of 2 * base channels.)
static long long widest_clip_elems(const vqvs_cfg& c) {
  const Topo t = topo_of(c);
  long long best = 0;
  for (int i = 0; i < t.levels(); ++i) {
    const long long rows = ((long long)c.max_T >> i) + 1;
    best = std::max(best, rows * t.mult[i] * c.base_channels * 2);
  }
  return best;
}

// What a predictor-gradient handle (speaker enrolment) is built for: the class-conditional fp32 predictor with one output channel at a
// width that needs no padding.  Checked by every entry point that takes a vqvs_cfg.
static int check_grad_kind(const vqvs_cfg& c) {
  if (c.kind != VQVS_KIND_PREDICTOR_GRAD) return 0;
  if (c.precision != VQVS_PREC_F32) VQVS_FAIL(VQVS_ERR_ARG, "predictor-gradient handle: precision %d is not built, fp32 (precision 0) only", c.precision);
  if (c.reserved[4] != 0)
    VQVS_FAIL(VQVS_ERR_ARG, "predictor-gradient handle: a padded width (reserved[4] = %d) is not built, base_channels must be a multiple of 32", c.reserved[4]);
  if (c.num_labels < 1) VQVS_FAIL(VQVS_ERR_ARG, "predictor-gradient handle: num_labels must be positive (got %d): the model has no class embedding", c.num_labels);
  if (c.out_channels != 1) VQVS_FAIL(VQVS_ERR_ARG, "predictor-gradient handle: out_channels must be 1 (got %d): the loss is the noise-prediction MSE", c.out_channels);
  return 0;
}

int enumerate_params(const vqvs_cfg& c, std::vector<ParamDef>& out) {
  out.clear();
  if (int e = check_grad_kind(c)) return e;
  if (int e = check_topology(c)) return e;
  const int base = c.base_channels;
  const bool drop = cfg_dropout(c);
  if (c.kind == VQVS_KIND_PREDICTOR || c.kind == VQVS_KIND_ENCPRED || c.kind == VQVS_KIND_PREDICTOR_GRAD) {
    const int E = 4 * base;
    out.push_back({"time_embed.proj.weight", {E, E}});
    out.push_back({"time_embed.proj.bias", {E}});
    out.push_back({"time_embed_extra.1.weight", {E, E}});
    out.push_back({"time_embed_extra.1.bias", {E}});
    if (c.num_labels > 0) out.push_back({"class_embed.weight", {c.num_labels, E}});
    if (c.cond_channels > 0) {
      out.push_back({"cond_proj.weight", {base, c.cond_channels, 3}});
      out.push_back({"cond_proj.bias", {base}});
    }
    out.push_back({"in_conv.weight", {base, c.in_channels, 3}});
    out.push_back({"in_conv.bias", {base}});
    std::vector<BlockSpec> d, mdl, u;
    predictor_blocks(base, topo_of(c), d, mdl, u);
    for (auto& s : d) block_params(out, s.prefix, s, E, drop);
    for (auto& s : mdl) block_params(out, s.prefix, s, E, drop);
    for (auto& s : u) block_params(out, s.prefix, s, E, drop);
    out.push_back({"out.0.0.weight", {base}});
    out.push_back({"out.0.0.bias", {base}});
    out.push_back({"out.1.weight", {c.out_channels, base, 3}});
    out.push_back({"out.1.bias", {c.out_channels}});
    if (c.kind == VQVS_KIND_ENCPRED) {  // encoder_predictor.py:40-41: self.unet = UNetPredictor(...), self.out = Conv1d(bottleneck, latents, 1)
      for (auto& d : out) d.name = "unet." + d.name;
      out.push_back({"out.weight", {c.reserved[2], c.out_channels, 1}});
      out.push_back({"out.bias", {c.reserved[2]}});
    }
  } else if (c.kind == VQVS_KIND_ENCODER) {
    out.push_back({"in_conv.weight", {base, c.in_channels, 3}});
    out.push_back({"in_conv.bias", {base}});
    std::vector<BlockSpec> blocks;
    const int cur = encoder_blocks(base, topo_of(c), blocks);
    for (auto& s : blocks) block_params(out, s.prefix, s, 0, false);
    out.push_back({"out.0.0.weight", {cur}});
    out.push_back({"out.0.0.bias", {cur}});
    out.push_back({"out.1.weight", {c.out_channels, cur, 3}});
    out.push_back({"out.1.bias", {c.out_channels}});
  } else if (c.kind == VQVS_KIND_RESBLOCK) {
    BlockSpec s{"", c.rb_cin, c.rb_cout, c.rb_resize, c.rb_dilation, false};
    block_params(out, "", s, c.rb_emb_channels, drop);
  } else if (c.kind == VQVS_KIND_CLASSIFIER) {  // classifier.py:18-104, 131-150
    const int E = 4 * base, F = classifier_output_mult(c) * base;
    std::vector<BlockSpec> blocks;
    const int cur = classifier_blocks(base, topo_of(c), blocks);
    out.push_back({"stem.time_embed.proj.weight", {E, E}});
    out.push_back({"stem.time_embed.proj.bias", {E}});
    out.push_back({"stem.time_embed_extra.1.weight", {E, E}});
    out.push_back({"stem.time_embed_extra.1.bias", {E}});
    out.push_back({"stem.in_conv.weight", {base, 1, 3}});
    out.push_back({"stem.in_conv.bias", {base}});
    for (auto& s : blocks) block_params(out, s.prefix, s, E, false);
    out.push_back({"stem.out.0.0.weight", {cur}});
    out.push_back({"stem.out.0.0.bias", {cur}});
    out.push_back({"stem.out.1.qkv_proj.weight", {3 * cur, cur, 1}});
    out.push_back({"stem.out.1.qkv_proj.bias", {3 * cur}});
    out.push_back({"stem.out.1.c_proj.weight", {F, cur, 1}});
    out.push_back({"stem.out.1.c_proj.bias", {F}});
    out.push_back({"out.1.weight", {c.num_labels, F}});
    out.push_back({"out.1.bias", {c.num_labels}});
  } else if (c.kind == VQVS_KIND_MFCC_ENCODER) {  // conv_encoder.py:42-84; buffers of torchaudio.transforms.MFCC first
    const int version = c.reserved[1];
    const int n_fft = version == 2 ? 400 : 2 * MFCC_HOP, n_mels = version == 2 ? 80 : 40, mid = 12 * base;
    out.push_back({"mfcc.dct_mat", {n_mels, 13}});
    out.push_back({"mfcc.MelSpectrogram.spectrogram.window", {n_fft}});
    out.push_back({"mfcc.MelSpectrogram.mel_scale.fb", {n_fft / 2 + 1, n_mels}});
    out.push_back({"blocks.0.0.weight", {mid, 39, 3}});
    out.push_back({"blocks.0.0.bias", {mid}});
    out.push_back({"blocks.1.conv.weight", {mid, mid, 3}});
    out.push_back({"blocks.1.conv.bias", {mid}});
    out.push_back({"blocks.2.0.weight", {mid, mid, 4}});
    out.push_back({"blocks.2.0.bias", {mid}});
    for (int i = 3; i <= 8; ++i) {
      out.push_back({"blocks." + std::to_string(i) + ".conv.weight", {mid, mid, i <= 4 ? 3 : 1}});
      out.push_back({"blocks." + std::to_string(i) + ".conv.bias", {mid}});
    }
    out.push_back({"blocks.9.weight", {c.out_channels, mid, 1}});
    out.push_back({"blocks.9.bias", {c.out_channels}});
  } else {
    VQVS_FAIL(VQVS_ERR_ARG, "unknown model kind %d", c.kind);
  }
  return 0;
}

static int check_cfg(const vqvs_cfg& c) {
  if (int e = check_grad_kind(c)) return e;
  if (c.precision != VQVS_PREC_F32 && c.precision != VQVS_PREC_BF16 && c.precision != VQVS_PREC_F16) VQVS_FAIL(VQVS_ERR_ARG, "bad precision %d", c.precision);
  if (c.max_batch < 1 || c.max_T < 1) VQVS_FAIL(VQVS_ERR_ARG, "max_batch/max_T must be positive");
  if (c.kind == VQVS_KIND_RESBLOCK) {
    if (c.rb_cin % 32 || c.rb_cout % 32 || c.rb_cin < 32 || c.rb_cout < 32) VQVS_FAIL(VQVS_ERR_ARG, "resblock channels must be multiples of 32");
    if (c.rb_dilation < 1 || c.rb_dilation > 32) VQVS_FAIL(VQVS_ERR_ARG, "resblock dilation must be in 1..32");
    if (c.rb_resize != RESIZE_NONE && c.rb_cin != c.rb_cout) VQVS_FAIL(VQVS_ERR_ARG, "resizing resblock cannot change channels");
    if (c.rb_emb_channels % 64) VQVS_FAIL(VQVS_ERR_ARG, "resblock emb channels must be a multiple of 64");
    return 0;
  }
  // the reference accepts any width (models/unet.py:17-30); here: powers of two from 32 to 128 (in_conv / out_conv distribute
  // C / 8 row pieces over a 256-thread workgroup; every convolution works on 32-channel K chunks)
  // predictor / encoder: any multiple of 32 up to 256 (unusual widths run the generic forms: 32-channel tiles, the stand-alone GroupNorm
  // pass, the row-per-thread output convolution); the guidance models' backward kernels want a power of two
  if (c.base_channels % 32 || c.base_channels < 32 || c.base_channels > 256)
    VQVS_FAIL(VQVS_ERR_ARG, "base_channels must be a multiple of 32 in 32..256 (got %d)", c.base_channels);
  // (round 6: the guidance models take any multiple of 32 too -- in_conv_bw and bw_act have row-per-thread / partial-pass forms for widths
  //  whose octet count is not a power of two; the MFCC encoder's 12 * base wide stack stays on powers of two)
  if (c.kind == VQVS_KIND_MFCC_ENCODER && (c.base_channels & (c.base_channels - 1)))
    VQVS_FAIL(VQVS_ERR_ARG, "base_channels must be a power of two for this kind of model (got %d)", c.base_channels);
  if ((c.kind == VQVS_KIND_PREDICTOR || c.kind == VQVS_KIND_ENCODER) && c.reserved[4] != 0) {
    // a padded handle (pad_map): reserved[4] = the real base_channels, base_channels = its physical width
    if (c.reserved[4] < 1 || c.reserved[4] > c.base_channels || padded_base(c.reserved[4]) != c.base_channels)
      VQVS_FAIL(VQVS_ERR_ARG, "real base_channels %d (reserved[4]) does not pad to base_channels %d (expected %d)", c.reserved[4], c.base_channels,
                c.reserved[4] >= 1 ? padded_base(c.reserved[4]) : 0);
  }
  if (c.in_channels < 1 || c.in_channels > 64) VQVS_FAIL(VQVS_ERR_ARG, "in_channels must be in 1..64 (got %d)", c.in_channels);
  if (c.in_channels != 1 && c.kind != VQVS_KIND_PREDICTOR && c.kind != VQVS_KIND_PREDICTOR_GRAD && c.kind != VQVS_KIND_ENCODER)
    VQVS_FAIL(VQVS_ERR_ARG, "in_channels = %d: only predictor and encoder handles take more than one input channel (the classifier stem and the "
                            "encoder predictor are mono in the reference too, classifier.py:73, encoder_predictor.py:40)", c.in_channels);
  if (c.kind == VQVS_KIND_MFCC_ENCODER) {
    if (c.precision != VQVS_PREC_F32) VQVS_FAIL(VQVS_ERR_ARG, "the MFCC encoder feeds the VQ layer (bit-exact indices): fp32 precision only");
    if (c.reserved[1] != 1 && c.reserved[1] != 2) VQVS_FAIL(VQVS_ERR_ARG, "ConvMFCCEncoder version must be 1 or 2 (got %d)", c.reserved[1]);
    if (c.out_channels % 32 || c.out_channels < 32) VQVS_FAIL(VQVS_ERR_ARG, "encoder out_channels must be a multiple of 32");
    if (c.max_T < 2 * 400) VQVS_FAIL(VQVS_ERR_ARG, "max_T must be at least 800 samples");
    return 0;
  }
  if (int e = check_topology(c)) return e;
  {
    const int rate = unet_rate(c);
    if (c.max_T % rate) VQVS_FAIL(VQVS_ERR_ARG, "max_T must be a multiple of the downsample rate %d (got %d)", rate, c.max_T);
  }
  // the kernels address rows of one clip with 32-bit byte offsets (buffer loads): the widest per-clip tensor must stay below 2 GiB
  // (4 bytes per element in the fp32 mode; the widest tensor a launch addresses is a level's concatenated input, 2 x its width)
  if (widest_clip_elems(c) * 4 > 0x7fffffffLL)
    VQVS_FAIL(VQVS_ERR_ARG, "max_T=%d is too long for base_channels=%d with this topology (a clip's widest tensor would exceed 2 GiB)", c.max_T, c.base_channels);
  if (c.kind == VQVS_KIND_PREDICTOR || c.kind == VQVS_KIND_PREDICTOR_GRAD) {
    if (c.out_channels != 1 && (c.out_channels % 32)) VQVS_FAIL(VQVS_ERR_ARG, "out_channels must be 1 or a multiple of 32");
    if (c.cond_channels % 32) VQVS_FAIL(VQVS_ERR_ARG, "cond_channels must be a multiple of 32");
    if (c.reserved[3] != 0 && c.reserved[3] != 1 && (c.reserved[3] <= LEN_ABS || c.reserved[3] > LEN_ABS + (1 << 20)))
      VQVS_FAIL(VQVS_ERR_ARG, "cond length code (reserved[3]) must be 0 (T/256), 1 (T/320) or 1000 + rows per clip (1 .. 2^20)");
  } else if (c.kind == VQVS_KIND_ENCPRED) {
    if (c.out_channels % 32 || c.out_channels < 32 || c.out_channels > 256) VQVS_FAIL(VQVS_ERR_ARG, "bottleneck_dim must be a multiple of 32 in 32..256");
    if (c.cond_channels) VQVS_FAIL(VQVS_ERR_ARG, "the encoder predictor's UNet is unconditional");
    if (c.num_labels) VQVS_FAIL(VQVS_ERR_ARG, "the encoder predictor's UNet has no class embedding");
    if (c.reserved[2] < 1) VQVS_FAIL(VQVS_ERR_ARG, "num_latents (reserved[2]) must be positive");
    if (c.reserved[1] < 1 || c.max_T % c.reserved[1]) VQVS_FAIL(VQVS_ERR_ARG, "downsample_rate %d must divide max_T", c.reserved[1]);
  } else if (c.kind == VQVS_KIND_CLASSIFIER) {
    if (c.num_labels < 1 || c.num_labels > 8192) VQVS_FAIL(VQVS_ERR_ARG, "classifier num_labels must be in 1..8192 (got %d)", c.num_labels);
    if (c.max_T % (2 * unet_rate(c))) VQVS_FAIL(VQVS_ERR_ARG, "classifier max_T must be a multiple of %d (got %d)", 2 * unet_rate(c), c.max_T);
    if (c.reserved[1] < 0 || c.reserved[1] * c.base_channels > 4096) VQVS_FAIL(VQVS_ERR_ARG, "classifier output_mult (reserved[1]) out of range (got %d)", c.reserved[1]);
    if (c.topology_set && c.n_dilations != 0) VQVS_FAIL(VQVS_ERR_ARG, "the classifier stem has no dilation list");
  } else {
    if (c.out_channels % 32 || c.out_channels < 32) VQVS_FAIL(VQVS_ERR_ARG, "encoder out_channels must be a multiple of 32");
  }
  return 0;
}

// ---- one schedule builder per kind -----------------------------------------------------------------------------------------------
// (the ops capture the vqvs_model* for pointer resolution, never the Builder: it is gone when build_model returns)

// A single ResBlock (unit-test granularity): NCT in, the external embedding through GELU + cond_layers.1, the block, NCT out
static void build_resblock(vqvs_model* m, Builder& b) {
  const vqvs_cfg& c = m->cfg;
  const int prec = c.precision, Cin = c.rb_cin, E = c.rb_emb_channels, R = 2 * c.rb_cout;
  const BlockSpec s{"", c.rb_cin, c.rb_cout, c.rb_resize, c.rb_dilation, false};
  TensorH x = b.new_tensor(Cin, 0, false, true);
  b.op("nct_to_ntc", "", 0, 0, 0, [=](const RunCtx& r) -> int {
    return launch_nct_to_ntc(r.x, m->act(x.off), m->statp(x.stats_off), r.B, Cin, r.Lbase, ntiles_of(r.Lbase), prec, r.st);
  });
  std::optional<Builder::FilmRows> film;
  if (E) {
    const size_t gemb = b.alloc_misc((size_t)c.max_batch * E);
    const size_t film_misc = b.alloc_misc((size_t)c.max_batch * R);
    film = Builder::FilmRows{film_misc, 0, R};  // (the one block's rows are the whole table)
    m->film_misc_off = film_misc;
    m->film_R = R;
    const size_t w_off = b.blob_f32_transposed(b.P("cond_layers.1.weight"), R, E);
    const size_t bias_off = b.blob_f32("cond_layers.1.bias");
    b.op("film", "", 0, 0, 0, [=](const RunCtx& r) -> int {
      if (!r.emb) VQVS_FAIL(VQVS_ERR_ARG, "resblock handle was built with an embedding; d_emb is NULL");
      if (int e = launch_gelu_rows(r.emb, m->miscp(gemb), r.B * E, r.st)) return e;
      FilmArgs f{m->miscp(gemb), m->wf(w_off), m->wf(bias_off), m->miscp(film_misc), E, R};
      return launch_film(f, r.B, r.st);
    });
  }
  TensorH y = b.resblock("", s, {x}, film);
  b.to_nct(y);
  b.tap("out", y);
}

// Predictor-gradient handles (speaker enrolment), behind the forward of build_unet: the loss head and the embedding-gradient schedule
// (phase 1): d mse_b / d v_b for every clip b.  out_w: the output convolution's [3][base] weights; pred: where the prediction of a
// call that does not ask for it goes.
static void unet_embed_grad_tail(vqvs_model* m, Builder& b, const std::vector<Builder::BlockRec>& recs, const Builder::TimeEmb& te,
                                 const Builder::Film& film, const TensorH& h, const Builder::GnTables& gh, size_t out_w, const TensorH& pred) {
  const vqvs_cfg& c = m->cfg;
  const int base = c.base_channels, E = te.E, R = film.R;
  const bool ws_f32_kind = b.ws_f32_kind;
  b.ws_f32_kind = false;  // (the transposed convolutions run where the guidance schedules' run)
  b.phase = 1;
  TensorH dout = b.new_tensor(1, 0, true, false);
  const size_t sq_off = b.alloc_misc(2 * (size_t)mse_head_scratch_doubles(c.max_batch, c.max_T));
  b.op("mse_head", "", 0, 12.0, 0, [=](const RunCtx& r) -> int {
    const float* p = r.out ? r.out : reinterpret_cast<const float*>(m->act(pred.off));
    return run_mse_head(p, r.eps, reinterpret_cast<float*>(m->act(dout.off)), r.mse, reinterpret_cast<double*>(m->miscp(sq_off)), r.B,
                        r.Lbase, r.st);
  });
  // out.1 (3-tap conv base -> 1 over gelu(GN(h))) backwards: conv^T and gelu' in one kernel, then GroupNorm backward
  TensorH t = b.new_tensor(base, 0, false, false);
  const size_t po = b.alloc_stats(base, 0);
  const size_t ss = gh.ss;
  b.op("out_conv_bw", "1->" + std::to_string(base), 2.0 * base, 4.0, 0, [=](const RunCtx& r) -> int {
    OutConvBwArgs a{};
    a.dout = reinterpret_cast<const float*>(m->act(dout.off));
    a.xf = m->act(h.off);
    a.ss = m->ssf2(ss);
    a.w = m->wf(out_w);
    a.du = m->act(t.off);
    a.partials = m->statp(po);
    a.C = base;
    a.L = r.Lbase;
    return launch_out_conv_bw(a, r.B, r.st);
  });
  b.release(dout);
  const size_t cfo = b.add_gn_bw(base, 0, po, gh.ss, gh.mr, STAT_TILE);
  b.add_bw_affine(t, h, cfo, nullptr, BW_SAME, nullptr, t);
  // per block, as soon as du2 exists: (d a | d b) into the block's rows of dfilm [B][R]
  const size_t dfilm_off = b.alloc_misc((size_t)c.max_batch * R);
  m->dfilm_misc_off = dfilm_off;
  m->dfilm_R = R;
  std::map<std::string, int> row_of;
  for (size_t i = 0; i < recs.size(); ++i) row_of[recs[i].s.prefix] = film.row[i];
  const Builder::Du2Hook film_grad = [&](const Builder::BlockRec& rec, const TensorH& du2) {
    const int C = rec.s.cout, row = row_of.at(rec.s.prefix), ls = rec.out.lshift;
    const size_t g_off = b.blob_f32(rec.s.prefix + ".pre_cond.3.weight"), be_off = b.blob_f32(rec.s.prefix + ".pre_cond.3.bias");
    const size_t pf = b.alloc_stats(C, ls);
    const TensorH D = du2, H1 = rec.h1;
    const size_t mr2 = rec.mr2;
    b.op("film_grad", "C=" + std::to_string(C) + " L>>" + std::to_string(ls), 2.0 * C * lscale(ls), 0, 0, [=](const RunCtx& r) -> int {
      FilmGradArgs a{};
      a.du = m->act(D.off);
      a.h1 = m->act(H1.off);
      a.mr = m->ssf2(mr2);
      a.gamma = m->wf(g_off);
      a.beta = m->wf(be_off);
      a.partials = m->statp(pf);
      a.dfilm = m->miscp(dfilm_off);
      a.film_stride = R;
      a.film_off = row;
      a.C = C;
      a.L = shiftL(r.Lbase, ls);
      a.ntiles = ntiles_of(a.L);
      return launch_film_grad(a, r.B, r.st);
    });
  };
  b.unet_backward(recs, t, false, film_grad);  // (the first block's input gradient and the skip path into in_conv are not needed)
  // d v = gelu'(emb) * Wall^T dfilm
  const size_t wall_off = film.wall_off, emb_off = te.emb_off;
  b.op("film_bw", "", 0, 0, 0, [=](const RunCtx& r) -> int {
    FilmBwArgs a{m->miscp(dfilm_off), m->wf(wall_off), m->miscp(emb_off), r.egrad, E, R};
    return launch_film_bw(a, r.B, r.st);
  });
  b.phase = 0;
  b.ws_f32_kind = ws_f32_kind;
}

// EncoderPredictor (encoder_predictor.py:25-58), behind the forward of build_unet with a bottleneck output `o`: the 1x1 head with its
// cross-entropy gradient (vq_vae.py:125-130: grads of the summed cross-entropy), then the backward schedule (phase 1) down to the input
static void unet_encpred_tail(vqvs_model* m, Builder& b, const std::vector<Builder::BlockRec>& recs, const TensorH& h,
                              const Builder::GnTables& gh, const TensorH& o) {
  const vqvs_cfg& c = m->cfg;
  const int prec = c.precision, base = c.base_channels, OC = c.out_channels, D = c.reserved[2], rate = c.reserved[1];
  const size_t hw = b.blob_f32("out.weight"), hb = b.blob_f32("out.bias");
  TensorH dO = b.new_tensor(OC, 0, false, false);
  const int es = b.es();
  b.op("enc_head", "D=" + std::to_string(D), 0, 0, 0, [=](const RunCtx& r) -> int {
    if (r.backward) VQVS_HIP(hipMemsetAsync(m->act(dO.off), 0, (size_t)r.B * r.Lbase * OC * es, r.st));
    EncHeadArgs a{};
    a.o = reinterpret_cast<const float*>(m->act(o.off));
    a.w = m->wf(hw);
    a.bias = m->wf(hb);
    a.logits = r.out;
    a.targets = r.backward ? r.labels : nullptr;
    a.gscale = grad_scale(prec);  // (the caller's scale multiplies the finished gradient in fp32, in_conv_bw: the 2-byte gradient tensors never see it)
    a.dO = m->act(dO.off);
    a.Cb = OC;
    a.D = D;
    a.T = r.Lbase;
    a.T1 = r.Lbase / rate;
    a.rate = rate;
    return launch_enc_head(a, r.B, prec, r.st);
  });
  b.phase = 1;
  // out.1 (3-tap conv base -> bottleneck over gelu(GN(h))) backwards: conv^T, gelu', GroupNorm backward
  TensorH t = b.new_tensor(base, 0, false, false);
  const size_t po = b.alloc_stats(base, 0);
  const bool fuse = Builder::bw_fuse_enabled();
  const Builder::BwFuse fo{{h}, gh.ss, base, po};
  const int tro = b.add_conv_t(dO, b.P("unet.out.1.weight"), OC, base, 3, 1, t, fuse ? &fo : nullptr);
  b.release(dO);
  if (!fuse) b.add_bw_act(t, BW_SAME, h, gh.ss, t, po);
  const size_t cfo = b.add_gn_bw(base, 0, po, gh.ss, gh.mr, fuse ? tro : STAT_TILE);
  b.add_bw_affine(t, h, cfo, nullptr, BW_SAME, nullptr, t);
  const TensorH gi = b.unet_backward(recs, t);  // blocks in reverse, down to the in_conv output
  b.in_conv_bw(gi, b.blob_f32("unet.in_conv.weight"));
  b.phase = 0;
}

// UNetPredictor.forward (unet.py:118-162) for three kinds of handle:
//   predictor           the forward alone;
//   EncoderPredictor    the same UNet under the "unet." prefix with a bottleneck output, every intermediate kept resident for the
//                       backward schedule of unet_encpred_tail;
//   predictor-gradient  the class-conditional predictor's own forward ops with the conditioning vector given per clip, every
//                       intermediate kept resident too, and unet_embed_grad_tail behind the output convolution.
static void build_unet(vqvs_model* m, Builder& b) {
  const vqvs_cfg& c = m->cfg;
  const int prec = c.precision, base = c.base_channels, NL = c.num_labels;
  const bool encpred = c.kind == VQVS_KIND_ENCPRED, gradk = c.kind == VQVS_KIND_PREDICTOR_GRAD;
  const bool keep_bw = encpred || gradk;
  const std::string px = encpred ? "unet." : "";
  std::vector<BlockSpec> down, mid, up, all;
  predictor_blocks(base, topo_of(c), down, mid, up);
  for (auto* v : {&down, &mid, &up})
    for (auto& s : *v) {
      all.push_back(s);
      all.back().prefix = px + s.prefix;
    }
  b.persist = keep_bw;  // (forward tensors of a handle with a backward schedule stay resident)
  // ---- embedding + all blocks' FiLM rows (unet.py:132-136)
  const Builder::TimeEmb te = b.time_embedding(px, NL, NL > 0 && !gradk, gradk || NL > 0);
  const Builder::Film film = b.film_table(all, te.E, te.gemb_off);
  // ---- conditioning projection (unet.py:46-47, 138-139)
  TensorH condp{};
  const bool has_cond = c.cond_channels > 0;
  if (has_cond) {
    // conditioning rows per clip: T / 256 behind a UNet encoder, (T / 160 + 1 - 2) / 2 + 1 = T / 320 behind the MFCC encoder
    // or, reserved[3] = 1000 + rows, exactly that many rows for any T (nearest up-sampling to T with PyTorch's index formula, in_conv)
    const int cond_ls = c.reserved[3] >= LEN_ABS ? c.reserved[3] : (c.reserved[3] == 1 ? LEN_HALF : 8);
    const int CC = c.cond_channels;
    TensorH ct = b.new_tensor(CC, cond_ls, false, false);
    b.op("nct_to_ntc", "", 0, 0, 0, [=](const RunCtx& r) -> int {
      return launch_nct_to_ntc(r.cond, m->act(ct.off), nullptr, r.B, CC, shiftL(r.Lbase, cond_ls), 0, prec, r.st);
    });
    condp = b.new_tensor(base, cond_ls, false, false);
    Builder::ConvSpec cv = b.conv_spec(base, condp);
    Builder::SegSpec g = Builder::raw_seg(ct);
    g.w_off = cv.pk.append(b.P(px + "cond_proj.weight"), base, CC, 3, 0, CC);
    cv.segs.push_back(g);
    const float* bb = b.P(px + "cond_proj.bias");
    cv.bias.assign(bb, bb + base);
    b.add_conv(cv);
    b.release(ct);
  }
  TensorH h = b.in_conv(px, c.in_channels, has_cond ? &condp : nullptr);
  if (has_cond) b.release(condp);
  b.tap("in_conv", h);
  // ---- down / middle / up with the skip stack (unet.py:141-160)
  std::vector<TensorH> skips{h};
  b.retain(h);  // one reference held by `h`, one by the stack
  std::vector<Builder::BlockRec> recs(all.size());
  for (size_t i = 0; i < all.size(); ++i) {
    const BlockSpec& s = all[i];
    std::vector<TensorH> ins{h};
    if (s.cat) {
      ins.push_back(skips.back());
      skips.pop_back();
    }
    TensorH o = b.resblock(s.prefix, s, ins, film.rows(i), keep_bw ? &recs[i] : nullptr);
    if (s.cat) b.release(ins[1]);
    b.release(h);
    h = o;
    if (i < down.size()) {  // every down block's output waits on the stack for its up block
      skips.push_back(h);
      b.retain(h);
    }
    b.tap(s.prefix, h);
  }
  // ---- output head (unet.py:113-116, 162)
  const Builder::GnTables gh = b.head_gn(h, px + "out.0.0", keep_bw);
  // (persist is read by release() alone, and nothing between here and the tails releases -- new_tensor, blob entries and add_conv do
  //  not -- so the forward ends here for every kind, although the tails allocate a little more before their first release)
  b.persist = false;
  if (c.out_channels != 1) {
    TensorH o = b.head_conv(h, gh, px + "out.1", c.out_channels, 0);
    if (encpred) unet_encpred_tail(m, b, recs, h, gh, o);
    else b.to_nct(o);
    return;
  }
  const float* W = b.P(px + "out.1.weight");  // [1][base][3] -> [3][base]
  std::vector<float> wt(3 * base);
  for (int k = 0; k < 3; ++k)
    for (int ci = 0; ci < base; ++ci) wt[k * base + ci] = W[ci * 3 + k];
  const size_t w = b.blob.add(wt.data(), wt.size() * 4);
  const float bias = b.P(px + "out.1.bias")[0];
  const TensorH pred = gradk ? b.new_tensor(1, 0, true, false) : TensorH{};  // (the prediction of a call that does not ask for it)
  const size_t ss = gh.ss;
  b.op("out_conv", std::to_string(base) + "->1", (double)base, 4.0, 0, [=](const RunCtx& r) -> int {
    OutConvArgs a{};
    a.in = m->act(h.off);
    a.ss = m->ssf2(ss);
    a.w = m->wf(w);
    a.bias = bias;
    a.out = gradk && !r.out ? reinterpret_cast<float*>(m->act(pred.off)) : r.out;
    a.C = base;
    a.L = r.Lbase;
    return launch_out_conv(a, r.B, prec, r.st);
  });
  if (gradk) unet_embed_grad_tail(m, b, recs, te, film, h, gh, w, pred);
}

// Classifier.forward (classifier.py:31-36, 111-121) + the input gradient used by cond_fn (sample_diffusion.py:34-42)
static void build_classifier(vqvs_model* m, Builder& b) {
  const vqvs_cfg& c = m->cfg;
  const int prec = c.precision, base = c.base_channels, F = classifier_output_mult(c) * base, NL = c.num_labels;
  std::vector<BlockSpec> blocks;
  const int cur = classifier_blocks(base, topo_of(c), blocks);
  b.persist = true;  // the backward pass re-reads every block input, h1 and their GroupNorm coefficients
  const Builder::TimeEmb te = b.time_embedding("stem.", 0, false, false);
  const Builder::Film film = b.film_table(blocks, te.E, te.gemb_off);
  size_t inw = 0;
  TensorH h = b.in_conv("stem.", 1, nullptr, &inw);
  b.tap("stem.in_conv", h);
  std::vector<Builder::BlockRec> recs(blocks.size());
  for (size_t i = 0; i < blocks.size(); ++i) {
    h = b.resblock(blocks[i].prefix, blocks[i], {h}, film.rows(i), &recs[i]);
    b.tap(blocks[i].prefix, h);
  }
  // ---- head: GroupNorm + GELU + attention pool (query token only) + c_proj + GELU + Linear, and its backward
  const Builder::GnTables gh = b.head_gn(h, "stem.out.0.0", true);
  const int ch = std::min(cur, 64), heads = cur / ch;
  const float* Wqkv = b.P("stem.out.1.qkv_proj.weight");  // [3*cur][cur][1]: q rows, k rows, v rows
  const float* bqkv = b.P("stem.out.1.qkv_proj.bias");
  const double sc2 = 1.0 / std::sqrt((double)ch);  // both q and k carry ch^-1/4 (classifier.py:181-186)
  std::vector<float> rvec((size_t)heads * cur), c0(heads);
  for (int hd = 0; hd < heads; ++hd) {
    double cc = 0.0;
    for (int j = 0; j < ch; ++j) cc += (double)bqkv[hd * ch + j] * (double)bqkv[cur + hd * ch + j];
    c0[hd] = (float)(cc * sc2);
    for (int ci = 0; ci < cur; ++ci) {
      double acc = 0.0;
      for (int j = 0; j < ch; ++j) acc += (double)bqkv[hd * ch + j] * (double)Wqkv[(size_t)(cur + hd * ch + j) * cur + ci];
      rvec[(size_t)hd * cur + ci] = (float)(acc * sc2);
    }
  }
  const size_t r_off = b.blob.add(rvec.data(), rvec.size() * 4), c0_off = b.blob.add(c0.data(), c0.size() * 4);
  const size_t wv_off = b.blob.add(Wqkv + (size_t)2 * cur * cur, (size_t)cur * cur * 4);
  const size_t wvT_off = b.blob_f32_transposed(Wqkv + (size_t)2 * cur * cur, cur, cur);
  const size_t wcT_off = b.blob_f32_transposed(b.P("stem.out.1.c_proj.weight"), F, cur);
  const size_t wlT_off = b.blob_f32_transposed(b.P("out.1.weight"), NL, F);
  const size_t bv_off = b.blob.add(bqkv + 2 * cur, (size_t)cur * 4);
  const size_t wc_off = b.blob_f32("stem.out.1.c_proj.weight"), bc_off = b.blob_f32("stem.out.1.c_proj.bias");
  const size_t wl_off = b.blob_f32("out.1.weight"), bl_off = b.blob_f32("out.1.bias");
  b.persist = false;
  TensorH dh = b.new_tensor(cur, h.lshift, false, false);
  const int groups_h = gn_groups(cur);
  b.op("cls_head", "C=" + std::to_string(cur), 0, 0, 0, [=](const RunCtx& r) -> int {
    HeadArgs a{};
    a.h = m->act(h.off);
    a.ss = m->ssf2(gh.ss);
    a.mr = m->ssf2(gh.mr);
    a.C = cur;
    a.L = shiftL(r.Lbase, h.lshift);
    a.heads = heads;
    a.F = F;
    a.NL = NL;
    a.groups = groups_h;
    a.inv_count = 1.0 / ((double)(cur / groups_h) * (double)a.L);
    a.r = m->wf(r_off);
    a.c0 = m->wf(c0_off);
    a.wv = m->wf(wv_off);
    a.wvT = m->wf(wvT_off);
    a.wcT = m->wf(wcT_off);
    a.wlT = m->wf(wlT_off);
    a.bv = m->wf(bv_off);
    a.wc = m->wf(wc_off);
    a.bc = m->wf(bc_off);
    a.wl = m->wf(wl_off);
    a.bl = m->wf(bl_off);
    a.logits = r.out;
    a.feat = r.feat;
    a.probs = r.probs;
    a.labels = r.backward ? r.labels : nullptr;
    a.gscale = grad_scale(prec);  // (the caller's scale multiplies the finished gradient in fp32, in_conv_bw: the 2-byte gradient tensors never see it)
    a.dh = m->act(dh.off);
    return launch_cls_head(a, r.B, prec, r.st);
  });
  // ---- backward schedule (phase 1): blocks in reverse, then the 1 -> base input convolution
  b.phase = 1;
  TensorH g = dh;
  for (size_t i = blocks.size(); i-- > 0;) g = b.resblock_backward(recs[i], g);
  b.in_conv_bw(g, inw);
  b.phase = 0;
}

// ConvMFCCEncoder.forward (conv_encoder.py:90-110).  The convolution stack runs on the fused MFMA kernel in the fp32
// mode: every layer is a raw segment with the GELU in the EPILOGUE (out = skip + gelu(conv(x)), conv_encoder.py:113-120);
// Conv1d(k = 4, stride = 2, padding = 1) is a 3-tap stride-1 convolution over the input viewed as [pairs][2 * mid]:
//   out[t] = W0 x[2t-1] + W1 x[2t] + W2 x[2t+1] + W3 x[2t+2]  =  sum over taps j = -1, 0, +1 of pair rows t + j with
//   even half: (0, W1, W3), odd half: (W0, W2, 0).
static void build_mfcc_encoder(vqvs_model* m, Builder& b) {
  const vqvs_cfg& c = m->cfg;
  const int base = c.base_channels;
  const int version = c.reserved[1], ulaw = c.reserved[2] ? 1 : 0;
  const int n_fft = version == 2 ? 400 : 2 * MFCC_HOP, n_mels = version == 2 ? 80 : 40, n_freqs = n_fft / 2 + 1, mid = 12 * base;
  const int OC = c.out_channels;
  std::vector<double> tw(2 * (size_t)n_fft);
  for (int n = 0; n < n_fft; ++n) {
    tw[2 * n] = std::cos(2.0 * M_PI * n / n_fft);
    tw[2 * n + 1] = -std::sin(2.0 * M_PI * n / n_fft);
  }
  const size_t tw_off = b.blob.add(tw.data(), tw.size() * 8);
  const size_t win_off = b.blob_f32("mfcc.MelSpectrogram.spectrogram.window"), fb_off = b.blob_f32("mfcc.MelSpectrogram.mel_scale.fb");
  const size_t dct_off = b.blob_f32("mfcc.dct_mat");
  double wss = 0.0;
  for (int n = 0; n < n_fft; ++n) wss += (double)b.P("mfcc.MelSpectrogram.spectrogram.window")[n] * (double)b.P("mfcc.MelSpectrogram.spectrogram.window")[n];
  const double power_scale = version == 2 ? 1.0 / wss : 1.0;  // Spectrogram(normalized=True): spec / sqrt(sum w^2), then |.|^2
  const int max_frames = c.max_T / MFCC_HOP + 1;
  const size_t logmel_off = b.alloc_misc((size_t)c.max_batch * max_frames * n_mels);
  const size_t wgmax_off = b.alloc_misc((size_t)c.max_batch * mfcc_groups(max_frames) + 64);
  const bool db = version == 2;
  TensorH feat = b.new_tensor(64, LEN_FRAMES, false, false);  // fp32 handle: the activation type is float
  b.op("mfcc_logmel", "n_fft=" + std::to_string(n_fft) + " mels=" + std::to_string(n_mels), 0, 4.0, 0, [=](const RunCtx& r) -> int {
    if (r.logmel != nullptr) {  // testing entry (vqvs_mfcc_encoder_forward_logmel): injected log-mel rows, the transform is skipped
      if (db) VQVS_FAIL(-1, "the injected log-mel entry exists for the log_mels (version 1) front end only");
      VQVS_HIP(hipMemcpyAsync(m->miscp(logmel_off), r.logmel, (size_t)r.B * shiftL(r.Lbase, LEN_FRAMES) * n_mels * sizeof(float),
                              hipMemcpyDeviceToDevice, r.st));
      return 0;
    }
    MfccArgs a{};
    a.x = r.x;
    a.twiddle = reinterpret_cast<const double*>(m->wp(tw_off));
    a.window = m->wf(win_off);
    a.fb = m->wf(fb_off);
    a.logmel = m->miscp(logmel_off);
    a.wgmax = db ? m->miscp(wgmax_off) + 64 : nullptr;
    a.T = r.Lbase;
    a.n_fft = n_fft;
    a.hop = MFCC_HOP;
    a.n_freqs = n_freqs;
    a.n_mels = n_mels;
    a.frames = shiftL(r.Lbase, LEN_FRAMES);
    a.ulaw = ulaw;
    a.log_mels = db ? 0 : 1;
    a.power_scale = power_scale;
    if (int e = launch_mfcc_logmel(a, r.B, r.st)) return e;
    if (db) return launch_mfcc_batch_max(m->miscp(wgmax_off) + 64, r.B * mfcc_groups(a.frames), m->miscp(wgmax_off), r.st);
    return 0;
  });
  b.op("mfcc_features", "13 x 3 -> 64 channels", 64.0 / MFCC_HOP, 0, 0, [=](const RunCtx& r) -> int {
    MfccFeatArgs a{};
    a.logmel = m->miscp(logmel_off);
    a.dct = m->wf(dct_off);
    a.batch_max = db ? m->miscp(wgmax_off) : nullptr;
    a.feat = reinterpret_cast<float*>(m->act(feat.off));
    a.frames = shiftL(r.Lbase, LEN_FRAMES);
    a.rows_alloc = a.frames;
    a.n_mels = n_mels;
    return launch_mfcc_features(a, r.B, r.st);
  });
  b.tap("features", feat);
  auto conv_layer = [&](const TensorH& in, int in_C, int in_lshift, const std::vector<float>& W, int cout, int cin, int ktaps,
                        const float* bias, const TensorH& out, int out_lshift, const TensorH* skip, bool gelu) {
    TensorH view = in;
    view.C = in_C;
    view.lshift = in_lshift;
    Builder::ConvSpec cv = b.conv_spec(cout, out);
    Builder::SegSpec g = Builder::raw_seg(view);
    g.ntaps = ktaps;
    g.w_off = cv.pk.append(W.data(), cout, cin, ktaps, 0, in_C);
    cv.segs.push_back(g);
    cv.bias.assign(bias, bias + cout);
    if (skip) cv.skip = *skip;
    cv.out_lshift = out_lshift;  // (the allocation of `out` may hold a padding row more)
    cv.epi_gelu = gelu;
    b.add_conv(cv);
  };
  auto wvec = [&](const std::string& name, size_t n) { return std::vector<float>(b.P(name), b.P(name) + n); };
  // blocks.0: Conv1d(39 -> mid, 3) + GELU over the zero-padded 64-channel feature rows
  TensorH h0 = b.new_tensor(mid, LEN_FRAMES, false, false);
  {
    std::vector<float> W((size_t)mid * 64 * 3, 0.f);
    const float* w = b.P("blocks.0.0.weight");
    for (int co = 0; co < mid; ++co)
      for (int ci = 0; ci < 39; ++ci)
        for (int k = 0; k < 3; ++k) W[((size_t)co * 64 + ci) * 3 + k] = w[((size_t)co * 39 + ci) * 3 + k];
    conv_layer(feat, 64, LEN_FRAMES, W, mid, 64, 3, b.P("blocks.0.0.bias"), h0, LEN_FRAMES, nullptr, true);
  }
  b.release(feat);
  b.tap("blocks.0", h0);
  // blocks.1: ResConv(3), written into an allocation with an even number of rows (last row zero: "pad_row")
  TensorH h1 = b.new_tensor(mid, LEN_FRAMES_PAD, false, false);
  b.op("pad_row", "", 0, 0, 0, [=](const RunCtx& r) -> int {
    const int frames = shiftL(r.Lbase, LEN_FRAMES), rows = shiftL(r.Lbase, LEN_FRAMES_PAD);
    if (rows == frames) return 0;
    VQVS_HIP(hipMemset2DAsync(m->act(h1.off) + (size_t)frames * mid * 4, (size_t)rows * mid * 4, 0, (size_t)mid * 4, r.B, r.st));
    return 0;
  });
  conv_layer(h0, mid, LEN_FRAMES, wvec("blocks.1.conv.weight", (size_t)mid * mid * 3), mid, mid, 3, b.P("blocks.1.conv.bias"), h1,
             LEN_FRAMES, &h0, true);
  b.release(h0);
  // blocks.2: Conv1d(mid -> mid, 4, stride 2, padding 1) + GELU as a 3-tap convolution over [pairs][2 * mid]
  TensorH h2 = b.new_tensor(mid, LEN_HALF, false, false);
  {
    std::vector<float> W((size_t)mid * 2 * mid * 3, 0.f);
    const float* w = b.P("blocks.2.0.weight");  // [mid][mid][4]
    for (int co = 0; co < mid; ++co)
      for (int ci = 0; ci < mid; ++ci) {
        const float* wk = w + ((size_t)co * mid + ci) * 4;
        float* even = &W[((size_t)co * 2 * mid + ci) * 3];
        float* odd = &W[((size_t)co * 2 * mid + mid + ci) * 3];
        even[1] = wk[1];  // x[2t]
        even[2] = wk[3];  // x[2t+2] = even half of pair row t+1
        odd[0] = wk[0];   // x[2t-1] = odd half of pair row t-1
        odd[1] = wk[2];   // x[2t+1]
      }
    conv_layer(h1, 2 * mid, LEN_PAIRS, W, mid, 2 * mid, 3, b.P("blocks.2.0.bias"), h2, LEN_HALF, nullptr, true);
  }
  b.release(h1);
  b.tap("blocks.2", h2);
  TensorH h = h2;
  for (int i = 3; i <= 8; ++i) {  // ResConv(3) x 2, ResConv(1) x 4
    const int k = i <= 4 ? 3 : 1;
    TensorH o = b.new_tensor(mid, LEN_HALF, false, false);
    const std::string nm = "blocks." + std::to_string(i) + ".conv";
    conv_layer(h, mid, LEN_HALF, wvec(nm + ".weight", (size_t)mid * mid * k), mid, mid, k, b.P(nm + ".bias"), o, LEN_HALF, &h, true);
    b.release(h);
    h = o;
  }
  b.tap("blocks.8", h);
  TensorH o = b.new_tensor(OC, LEN_HALF, true, false);
  conv_layer(h, mid, LEN_HALF, wvec("blocks.9.weight", (size_t)OC * mid), OC, mid, 1, b.P("blocks.9.bias"), o, LEN_HALF, nullptr, false);
  b.release(h);
  b.to_nct(o);
}

// UNetEncoder.forward (unet.py:229-241): the blocks without FiLM, the output has T / downsample_rate rows
static void build_encoder(vqvs_model* m, Builder& b) {
  const vqvs_cfg& c = m->cfg;
  std::vector<BlockSpec> blocks;
  encoder_blocks(c.base_channels, topo_of(c), blocks);
  TensorH h = b.in_conv("", c.in_channels, nullptr, nullptr, 1);
  b.tap("in_conv", h);
  for (auto& s : blocks) {
    TensorH o = b.resblock(s.prefix, s, {h}, std::nullopt);
    b.release(h);
    h = o;
    b.tap(s.prefix, h);
  }
  const Builder::GnTables gh = b.head_gn(h, "out.0.0", false);
  b.to_nct(b.head_conv(h, gh, "out.1", c.out_channels, topo_of(c).levels() - 1));
}

int build_model(vqvs_model* m, const float* const* hp) {
  const vqvs_cfg& c = m->cfg;
  if (int e = check_cfg(c)) return e;
  if (int e = enumerate_params(c, m->params)) return e;
  Builder b(m, hp);
  switch (c.kind) {
    case VQVS_KIND_RESBLOCK: build_resblock(m, b); break;
    case VQVS_KIND_PREDICTOR:
    case VQVS_KIND_ENCPRED:
    case VQVS_KIND_PREDICTOR_GRAD: build_unet(m, b); break;
    case VQVS_KIND_CLASSIFIER: build_classifier(m, b); break;
    case VQVS_KIND_MFCC_ENCODER: build_mfcc_encoder(m, b); break;
    default: build_encoder(m, b); break;  // (enumerate_params has refused every unknown kind)
  }

  for (auto& mt : m->meta) {
    if (mt.kind == "xform") continue;  // overhead traffic, not part of the algorithmic (Model A) bytes
    m->cost.elems_T += mt.elems_T;
    m->cost.bytes_f32 += mt.bytes_f32;
    m->cost.flops += mt.flops;
  }
  // ---- lay out the arena and upload the weights ------------------------------------------
  m->act_bytes = (b.act_high + 255) & ~(size_t)255;
  m->stats_off = m->act_bytes;
  m->stats_floats = b.stats_floats;
  m->ss_off = (m->stats_off + b.stats_floats * 4 + 255) & ~(size_t)255;
  m->ss_floats = b.ss_floats;
  m->misc_off = (m->ss_off + b.ss_floats * 4 + 255) & ~(size_t)255;
  m->misc_floats = b.misc_floats;
  m->arena_bytes = m->misc_off + b.misc_floats * 4 + 256;
  m->weights_bytes = b.blob.data.size() + 256;
  VQVS_HIP(hipMalloc(reinterpret_cast<void**>(&m->d_weights), m->weights_bytes));
  VQVS_HIP(hipMemcpy(m->d_weights, b.blob.data.data(), b.blob.data.size(), hipMemcpyHostToDevice));
  VQVS_HIP(hipMalloc(reinterpret_cast<void**>(&m->d_arena), m->arena_bytes));
  VQVS_HIP(hipMemset(m->d_arena, 0, m->arena_bytes));
  return 0;
}

int run_model(vqvs_model* m, const RunCtx& ctx) {
  if (m->profiling) {
    if (m->events.size() != m->ops.size() + 1) {
      for (auto e : m->events) (void)hipEventDestroy(e);
      m->events.assign(m->ops.size() + 1, nullptr);
      for (auto& e : m->events) VQVS_HIP(hipEventCreate(&e));
    }
    VQVS_HIP(hipEventRecord(m->events[0], ctx.st));
    for (size_t i = 0; i < m->ops.size(); ++i) {
      if (m->op_phase[i] == 0 || ctx.backward)
        if (int e = m->ops[i](ctx)) return e;
      VQVS_HIP(hipEventRecord(m->events[i + 1], ctx.st));
    }
    m->last_B = ctx.B;
    m->last_L = ctx.Lbase;
    return 0;
  }
  for (size_t i = 0; i < m->ops.size(); ++i)
    if (m->op_phase[i] == 0 || ctx.backward)
      if (int e = m->ops[i](ctx)) return e;
  m->last_B = ctx.B;
  m->last_L = ctx.Lbase;
  return 0;
}

}  // namespace vqvs
