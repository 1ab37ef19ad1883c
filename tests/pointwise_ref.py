"""The cases, the float64 references and the per-entry bounds of tests/test_pointwise.py and tests/test_pointwise_gpu.py: the kernels of a
UNet forward that are not convolutions -- the GELU device functions (csrc/common.hpp), `time_embed_kernel`, `film_kernel`,
`in_conv_kernel`, `out_conv_kernel` / `out_conv_rows_kernel` (csrc/misc_kernels.hip) -- held entry by entry, not by an RMS of a whole
tensor.  u = 2^-24 is float32's unit roundoff throughout.  Every bound is derived here; none is a measured value.

Stage A, the GELU forms (`vqvs_debug_gelu`: 0 gelu_f, 1 gelu2<EXACT>, 2 gelu2<POLY6>, 3 gelu2<POLY7>, 4 gelu_grad_f).
  Reference: erf-GELU in float64; Phi(v) + v phi(v) for form 4.  Gates on [-8, 8], common.hpp's own statements rounded up to one
  digit: 1e-6 (forms 0, 1), 6e-4 (form 2), 5e-5 on [-4, 4] and 3.5e-4 on [-8, 8] (form 3).  Beyond +-8 the error is held relative to
  |v|, each form to the storage rounding it serves: 2^-22 |v| (exact forms: 0.5 v (1 + 1) is v itself), 2^-9 |v| (degree 6, bf16),
  2^-12 |v| (degree 7, fp16).
  Form 4, |v| <= 8.  Phi = 0.5 (1 + e), e = 1 - rcp(p^16), p the degree-6 Horner form in z = |v| / sqrt 2.
    e.  Abramowitz-Stegun 7.1.28 itself: 3e-7.  The argument z rounds once (and its constant once): d erf = (2 / sqrt pi) z exp(-z^2)
        * 2u <= 0.49 * 2u = 5.8e-8.  Roundings: rcp(p^16) = erfc~(z) carries the relative error of p^16 and v_rcp_f32's own ulp, and
        `1 - rcp` rounds once.  The four squarings add (8 + 4 + 2 + 1) u = 15u relative, the Horner form 16 times its own: its
        last fma rounds p (u), the five before it reach p only through z * q <= p - 1.  The first-order total,
        erfc(z) (16 (1 + 5 (p - 1) / p) + 15 + 2) u, is largest at z -> 0: 33u = 2.0e-6 IF every rounding fell the same way; they are
        independent, so the expected size is the root of the sum of squares, sqrt(16^2 + 8^2 + 4^2 + 2^2 + 1 + 2) u = 18.6u = 1.1e-6.
        With 3e-7 and 5.8e-8: |de| <= 1.5e-6 expected, 2.4e-6 at the very worst.  Phi takes half: 7.4e-7 expected (1.2e-6 worst).
    v phi(v).  The argument a = -v^2 / 2 in [-32, 0] rounds twice, v_exp_f32's scaling by log2 e once more and its result to an ulp:
        relative (4 |a| + 4) u; |v| phi(v) (2 v^2 + 4) u <= 1.7u = 1.0e-7 (at |v| = 1.5; |v| phi(v) <= 0.25 everywhere).
    The final fma rounds a value <= 1.13 once: 6.7e-8.
    Sum: 9.1e-7 with roundings of independent sign, which is the issue's gate of 1e-6 -- kept.  A strict worst case (every one of
    33 roundings the same way at the same v) would be 1.4e-6; the gate holds the kernel to the expected-size figure.
    Beyond +-8 both terms saturate (rcp -> 0, exp -> 0): the same absolute gate.
  NaN gives NaN in every form; +-0 and denormals are held to the absolute gates; +-inf is recorded, not gated; forms 0 and 1 agree
  to 2 ulps of each other (their products are grouped differently: 0.5 v (1 + e) against (0.5 v) (e + 1)).

Stage B, the conditioning vector (`time_embed_kernel`, read with `read_embedding`).
  Reference: `embedding` below in float64 -- `oracle.ref_cpu.unet_embedding` with the argument t * f formed as the float32 oracle forms
  it (the float32 product of the float32 timestep and the float32 frequency table, widened), and with a vector per clip where the
  call brings one; in float32 it IS ref_cpu.unet_embedding, bit for bit (tests/test_pointwise.py).
  Bound of entry r: 1e-6 * sum_j |w2[r][j]|  (the kernel's gelu_f between the two mat-vecs, at Stage A's bound: the one thing it
  does differently by design)  +  8 * E_ref  (E_ref: the largest absolute error, over the case, of the same reference in float32 on
  the CPU, floored at u max|want|: both are float32 evaluations of one expression in different summation orders; their maxima over a
  few thousand entries rarely differ by more than 2-3x),  capped at 2e-5, the gate of test_time_embedding_vs_golden.
  E_ref <= 1e-5 is asserted for every case on the CPU.  The vector is float32 in every mode: fp32 and fp16 agree bit for bit.

Stage C, the FiLM rows (`film_kernel`, read with `read_film`).
  Reference: bias + W gelu64(emb) in float64 from the embedding as read back (its own error is Stage B's).
  Bound of entry (b, r): 1e-6 * sum_e |W[r][e]| + (E / 4 + 6) u S_r,  S_r = |bias_r| + sum_e |W[r][e] gelu(emb_e)|.
  The first term is gelu_f (Stage A).  The second counts roundings as film_kernel performs them: each of its four waves chains
  E / 4 fused multiply-adds into an accumulator that starts at 0 (E / 4 roundings at most on a term's path), wave 0 adds the three
  other waves' sums in wave order (3), then the bias (1): E / 4 + 4, and two to spare for the rounding of the stored gelu_f value and
  the second-order terms.  On a padded handle the pad entries are exact zeros: a wave's 64 physical entries hold E_real / 4 real ones.

Stage D, stem and head from the debug taps.
  Stem (`in_conv_kernel`): the `in_conv` tap against float64 conv1d(x) [+ the projected conditioning, nearest-upsampled with
  PyTorch's index rule].  fp32 mode: (3 Cin + 2) u S per element, S the sum of the absolute terms (three chained fmas per input
  channel starting from the bias, one addition of the conditioning row, one to spare).  fp16 mode: that + the two stored half
  roundings, 2^-11 (|v| + |condp|) -- each at least 2^-25, half the spacing of fp16's subnormals, which a tap of a few thousand
  entries does reach (|v| < 2^-14).  The conditioning projection is produced by a convolution kernel, not by in_conv; what that
  kernel's number formats cost is added for the conditioned model ONLY, derived from the formats, S_p = the projection's absolute
  terms: fp32 mode 2^-16 S_p (operands split into bf16 hi + lo, 2^-17 relative each, lo * lo dropped), fp16 mode 2^-10 S_p (input
  rows and weights rounded to half, 2^-11 each).  A wrong row of the conditioning (the up-sampling index) is an error of
  O(|condp|), orders above either.
  Head (`out_conv_kernel`; base 96: `out_conv_rows_kernel`): the model's output against GroupNorm (the reference's group count,
  eps 1e-5), GELU, 3-tap convolution and bias in float64 FROM the last block's tap as read back (fp16 mode: the stored halves
  exactly).  Bound per element: the mode's Stage A bound (fp32: 8.7e-7; fp16: 4.4e-5 where every |u| the element reads is <= 4,
  3.4e-4 otherwise) * sum |w| over the taps that exist at that position, + 8 E_ref (as in Stage B, of the same head in float32 on the
  CPU), + the statistics term.  The statistics term: E_ref's premise -- one expression, two summation orders -- does not cover the
  variance.  The library forms it in one pass, var = s2 / n - mean^2 in float64 from FLOAT32 sums s1, s2 of the stored values (the
  producing convolution's epilogue, per 256-row tile; gn_prepare adds the tiles in float64), the CPU's float32 group_norm in two.  A
  float32 sum of N terms in any order passes a term through at most N - 1 roundings, the square rounds once: with K = min(T, 256)
  + 1, |d mean| <= K u mean|x| and |d var| <= K u mean(x^2) + 2 |mean| |d mean| <= 3 K u mean(x^2).  Where |d var| < var + eps,
  |d rstd| <= (var + eps - |d var|)^-1/2 - rstd and |d u| <= |gamma| (rstd |d mean| + (|x - mean| + |d mean|) |d rstd|); the output
  moves by at most sum |w| max|gelu'| |d u|, max|gelu'| = 1.13.  Two nearly equal values per group (T = 2, one channel per group at
  base 32) make this term the largest; on long clips it is a few 1e-5 at most and every planted defect stays orders above it.
  A head with more than one output channel exists only for multiples of 32 (vqvs_model_create) and runs on the MFMA convolution,
  which is outside these tests: the in_channels = 3 model keeps the one-channel head, served by out_conv_kernel like the others.

`share_of_bound` of a check is the largest |error| / bound over its entries: the GPU file records it per case under
profiles/pointwise_margins.jsonl, and no case may use more than 1.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu
from vq_voice_swap_amd import UNetPredictor
from vq_voice_swap_amd.det_init import det_init_
from vq_voice_swap_amd.unet import pad_blocks

MARGINS = "pointwise_margins.jsonl"
U = 2.0 ** -24
TOPO = dict(channel_mult=(1, 2), depth_mult=1, middle_dilations=(1,))
NUM_LABELS = 4

# ------------------------------------------------------------------------------------------------------------------ Stage A: GELU
FORMS = {"gelu_f": 0, "exact": 1, "poly6": 2, "poly7": 3, "grad": 4}
GELU_GATE = {0: 1e-6, 1: 1e-6, 2: 6e-4, 3: 3.5e-4, 4: 1e-6}  # |error| on [-8, 8]
GELU_GATE_INNER = {3: 5e-5}  # ... and on [-4, 4]
GELU_TAIL = {0: 2.0 ** -22, 1: 2.0 ** -22, 2: 2.0 ** -9, 3: 2.0 ** -12}  # |error| / |v| beyond +-8 (form 4: the absolute gate)
COMMON_HPP = {0: 8.7e-7, 1: 8.7e-7, 2: 5.7e-4, 3: 3.4e-4, "3inner": 4.4e-5}  # what csrc/common.hpp states
FORM01_ULPS = 2
TAILS = (10.0, 100.0, 3.0e4, 65504.0)


def _around(c, n=64):
    """Every float32 within n ulps of c."""
    if c == 0.0:
        k = np.arange(-n, n + 1, dtype=np.int64)
        return (k.astype(np.float64) * 2.0 ** -149).astype(np.float32)
    bits = np.array([c], dtype=np.float32).view(np.int32)[0].astype(np.int64)
    return (bits + np.arange(-n, n + 1, dtype=np.int64)).astype(np.int32).view(np.float32)


def gelu_inputs():
    """float32: 2^20 + 1 evenly spaced values on [-8, 8]; every float32 within 64 ulps of 0, +-4 and +-8; +-{10, 100, 3e4, 65504}; +-0."""
    grid = np.linspace(-8.0, 8.0, 2 ** 20 + 1).astype(np.float32)
    near = [_around(c) for c in (0.0, 4.0, -4.0, 8.0, -8.0)]
    tails = np.array([s * t for t in TAILS for s in (1.0, -1.0)] + [0.0, -0.0], dtype=np.float32)
    return np.concatenate([grid] + near + [tails])


def gelu64(x):
    x = torch.as_tensor(np.asarray(x, dtype=np.float64))
    return (0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))).numpy()


def gelu_want(x, form):
    """The float64 reference of a form on float32 inputs."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    if form != 4:
        return gelu64(x)
    xt = torch.from_numpy(x)
    return (0.5 * (1.0 + torch.erf(xt / math.sqrt(2.0))) + xt * torch.exp(-0.5 * xt * xt) / math.sqrt(2.0 * math.pi)).numpy()


def gelu_gate(x, form):
    """The absolute bound of every entry."""
    a = np.abs(np.asarray(x, dtype=np.float32).astype(np.float64))
    g = np.full(a.shape, GELU_GATE[form])
    if form in GELU_GATE_INNER:
        g[a <= 4.0] = GELU_GATE_INNER[form]
    if form in GELU_TAIL:
        g[a > 8.0] = GELU_TAIL[form] * a[a > 8.0]
    return g


def _fma(a, b, c):
    """float32 fma: the product of two float32 values is exact in float64."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


AS_COEF = (0.0000430638, 0.0002765672, 0.0001520143, 0.0092705272, 0.0422820123, 0.0705230784, 1.0)
POLY6 = (2.81608722e-08, -1.89188380e-06, 5.41903041e-05, -8.78980255e-04, 9.11294959e-03, -6.53883549e-02, 3.98526915e-01)
POLY7 = (-1.301278171e-09, 1.041951057e-07, -3.657111166e-06, 7.485478930e-05, -1.006488756e-03, 9.505392772e-03, -6.588783436e-02,
         3.986733897e-01)


def _horner(coef, z):
    p = np.full(z.shape, np.float32(coef[0]), dtype=np.float32)
    for c in coef[1:]:
        p = _fma(p, z, np.float32(c))
    return p


def gelu_formula(x, form, poly7=POLY7):
    """The formulas of csrc/common.hpp restated in float32 numpy (rcp and exp by numpy's own): what the gates ask is attainable."""
    f = np.float32
    v = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if form in (0, 1, 4):
            z = np.abs(v) * f(0.70710678118654752440)
            p = _horner(AS_COEF, z)
            for _ in range(4):
                p = p * p
            e = np.copysign(f(1.0) - f(1.0) / p, v)
            if form == 0:
                return f(0.5) * v * (f(1.0) + e)
            if form == 1:
                return (v * f(0.5)) * (e + f(1.0))
            Phi = f(0.5) * (f(1.0) + e)
            return _fma(v * f(0.39894228040143267794), np.exp(f(-0.5) * v * v), Phi)
        vc = np.where(np.isnan(v), v, np.clip(v, f(-4.0), f(4.0)))
        p = _horner(POLY6 if form == 2 else poly7, vc * vc)
        return v * _fma(vc, p, f(0.5))


def worst(got, want, bound):
    """(largest |error|, largest |error| / bound, flat index of the latter) over the entries."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    share = err / np.asarray(bound, dtype=np.float64)
    i = int(np.nanargmax(share)) if share.size else 0
    return float(err.max()), float(share.reshape(-1)[i]), i


def rel_rms(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.sqrt(np.mean((got - want) ** 2)) / np.sqrt(np.mean(want ** 2)))


# ------------------------------------------------------------------------------------------------------------------ the models
EMB_BASES = (32, 64, 96, 128, 256, 40)  # 256: E = 1024, time_embed_kernel's limit; 40: a padded width (built at 64)
FILM_B = (1, 31, 32, 33, 65)
STEM_BASES = (32, 64, 96, 128)  # 4, 8, 12 and 16 octets per row
STEM_T = (2, 254, 256, 258, 770)
STEM_B = (1, 3)
EXTRA = {"in3": dict(base=32, in_channels=3), "cond": dict(base=64, cond_channels=64)}
COND_LEN, COND_T = 37, 770
TS_HEAD = (0.0, 1e-7, 1e-3, 0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.999, 1.0, 1.5, -0.3)


def make_model(base, labels=True, **kw):
    """UNetPredictor(base, channel_mult=(1, 2), depth_mult=1, middle_dilations=(1,)[, num_labels=4]) under det_init_, eval()."""
    m = UNetPredictor(base, num_labels=NUM_LABELS if labels else None, **TOPO, **kw)
    det_init_((f"pw.{base}." + k, v) for k, v in m.state_dict().items())
    return m.eval()


def state(model, dtype=torch.float64):
    return {"predictor." + k: v.detach().to(dtype) for k, v in model.state_dict().items()}


def clip_inputs(B, base=None, seed=7700):
    """(ts [B] float32, labels [B] int64, vectors [B, 4 * base] float32 N(0, 0.3^2) or None).  Timesteps: the thirteen listed ones, then
    (2 i + 1) / 40 for clip i -- i / 20 on the odd fortieths, because i / 20 itself repeats 0.75, 0.9, 1 and 1.5 of the list and the
    clips must stay distinct (with the same label, clips 7 and 15 would be indistinguishable); labels i % 4."""
    ts = torch.tensor([TS_HEAD[i] if i < len(TS_HEAD) else (2 * i + 1) / 40.0 for i in range(B)], dtype=torch.float32)
    labels = torch.arange(B, dtype=torch.int64) % NUM_LABELS
    vec = None
    if base is not None:
        vec = 0.3 * torch.randn((B, 4 * base), generator=torch.Generator().manual_seed(seed + base))
    return ts, labels, vec


def wave(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def phys_index(base, n):
    """Physical position of every entry of a real axis of n channels on the handle of width `base` (identity unless padded)."""
    q, qp = pad_blocks(base)
    idx = torch.arange(n)
    return (idx // q) * qp + idx % q


# ------------------------------------------------------------------------------------------------------------------ Stage B
EMB_CAP = 2e-5
EREF_MAX = 1e-5


def embedding(sd, ts, labels=None, vectors=None, clamp_labels_to=None):
    """[B, E] in the dtype of `sd`: ref_cpu.unet_embedding with the argument t * f formed in float32 and widened, and `vectors` in
    place of class_embed[labels] where given.  clamp_labels_to: a planted defect (tests/test_pointwise.py)."""
    w = sd["predictor.time_embed.proj.weight"]
    half = w.shape[1] // 2
    freqs = torch.exp(-math.log(100.0 / 0.1) * torch.arange(0, half, dtype=torch.float32) / (half - 1)) * 100.0
    args = (ts.to(torch.float32)[:, None] * freqs[None]).to(w.dtype)
    emb = F.linear(torch.cat([torch.cos(args), torch.sin(args)], dim=-1), w, sd["predictor.time_embed.proj.bias"])
    emb = F.linear(F.gelu(emb), sd["predictor.time_embed_extra.1.weight"], sd["predictor.time_embed_extra.1.bias"])
    if labels is not None:
        if clamp_labels_to is not None:
            labels = labels.clamp(max=clamp_labels_to)
        emb = emb + F.embedding(labels, sd["predictor.class_embed.weight"])
    if vectors is not None:
        emb = emb + vectors.to(w.dtype)
    return emb


def e_ref(want64, got32):
    """Largest absolute error of the float32 CPU evaluation, floored at u max|want|."""
    want64 = torch.as_tensor(want64).double()
    return max(float((torch.as_tensor(got32).double() - want64).abs().max()), U * float(want64.abs().max()))


def emb_bound(sd64, eref):
    """[E]: min(2e-5, 1e-6 sum_j |w2[r][j]| + 8 E_ref)."""
    return (1e-6 * sd64["predictor.time_embed_extra.1.weight"].abs().sum(dim=1) + 8.0 * eref).clamp(max=EMB_CAP)


def emb_case(model, B=33, path="labels"):
    """dict(ts, labels, vectors, want [B, E] float64, eref, bound [E]) of a path: "labels", "vectors" or "none" (a model without labels)."""
    base = model.base_channels
    ts, labels, vec = clip_inputs(B, base)
    labels, vec = (labels if path == "labels" else None), (vec if path == "vectors" else None)
    sd64 = state(model)
    want = embedding(sd64, ts, labels, vec)
    er = e_ref(want, embedding(state(model, torch.float32), ts, labels, vec))
    return dict(ts=ts, labels=labels, vectors=vec, want=want, eref=er, bound=emb_bound(sd64, er))


# ------------------------------------------------------------------------------------------------------------------ Stage C
def film_blocks(base):
    """[(block name, cout)] in the order of the rows: down, middle, up."""
    specs = ref_cpu.predictor_block_specs(base, **TOPO)
    return [(f"{part}.{i}", s["cout"]) for part, key in (("down_blocks", "down"), ("middle_blocks", "middle"), ("up_blocks", "up"))
            for i, s in enumerate(specs[key])]


def film_index(base):
    """Physical row, in the handle's [R] layout, of every real FiLM row (a | b per block, blocks in order)."""
    q, qp = pad_blocks(base)
    out, row = [], 0
    for _name, cout in film_blocks(base):
        p, cp = phys_index(base, cout), cout // q * qp
        out += [row + p, row + cp + p]
        row += 2 * cp
    return torch.cat(out), row


def film_ref(model, emb, defect=None):
    """(want [B, R], bound [B, R]) in float64 from the embedding [B, E] (real width) as read back.  defect: "swap32" (the (a | b) halves
    of clip 32 swapped) or "emb0" (clip 32 reads clip 0's embedding) -- planted, for tests/test_pointwise.py."""
    sd = state(model)
    Wall = torch.cat([sd[f"predictor.{n}.cond_layers.1.weight"] for n, _ in film_blocks(model.base_channels)])
    ball = torch.cat([sd[f"predictor.{n}.cond_layers.1.bias"] for n, _ in film_blocks(model.base_channels)])
    emb = torch.as_tensor(emb).double().clone()
    if defect == "emb0":
        emb[32] = emb[0]
    g = torch.from_numpy(gelu64(emb.numpy()))
    want = ball + g @ Wall.T
    S = ball.abs() + g.abs() @ Wall.abs().T
    E = Wall.shape[1]
    bound = 1e-6 * Wall.abs().sum(dim=1) + (E / 4 + 6) * U * S
    if defect == "swap32":
        row = 0
        for _n, cout in film_blocks(model.base_channels):
            want[32, row:row + 2 * cout] = torch.cat([want[32, row + cout:row + 2 * cout], want[32, row:row + cout]])
            row += 2 * cout
    return want, bound


# ------------------------------------------------------------------------------------------------------------------ Stage D
PROJ_FORMAT = {"fp32": 2.0 ** -16, "fp16": 2.0 ** -10}  # operand formats of the MFMA convolution (module docstring)
GELU_SLOPE = 1.13  # max |gelu'| (1.1290 at v = 1.4142)
HEAD_GELU = {"fp32": (8.7e-7, 8.7e-7), "fp16": (4.4e-5, 3.4e-4)}  # Stage A bound of the mode's form: (every |u| <= 4, otherwise)


def half_rounding(v):
    """Largest error of rounding v to fp16: 2^-11 |v|, and half the subnormal spacing, 2^-25, below 2^-14."""
    return (2.0 ** -11 * v.abs()).clamp(min=2.0 ** -25)


def stem_ref(model, x, cond=None, defect=None):
    """dict(want, bound32, bound16 [B, C, T]) of the in_conv tap in float64.  defect: "left256" (the left neighbour dropped at
    t = 256) or "right_end" (the last row reads the sample behind it -- the next clip's first -- instead of zero)."""
    sd = state(model)
    w, b = sd["predictor.in_conv.weight"], sd["predictor.in_conv.bias"]
    x = x.double()
    Cin, T = x.shape[1], x.shape[2]
    v = F.conv1d(x, w, b, padding=1)
    if defect == "left256":
        v[:, :, 256] -= torch.einsum("oc,bc->bo", w[:, :, 0], x[:, :, 255])
    if defect == "right_end":
        nxt = torch.roll(x, -1, dims=0)[:, :, 0]
        v[:, :, T - 1] += torch.einsum("oc,bc->bo", w[:, :, 2], nxt)
    S = F.conv1d(x.abs(), w.abs(), b.abs(), padding=1)
    want, condp, Sp = v, torch.zeros_like(v), torch.zeros_like(v)
    if cond is not None:
        wc, bc = sd["predictor.cond_proj.weight"], sd["predictor.cond_proj.bias"]
        condp = F.interpolate(F.conv1d(cond.double(), wc, bc, padding=1), T)
        Sp = F.interpolate(F.conv1d(cond.double().abs(), wc.abs(), bc.abs(), padding=1), T)
        want = v + condp
    b32 = (3 * Cin + 2) * U * (S + Sp)
    return dict(want=want, bound32=b32 + PROJ_FORMAT["fp32"] * Sp,
                bound16=b32 + half_rounding(want) + (half_rounding(condp) if cond is not None else 0.0) + PROJ_FORMAT["fp16"] * Sp)


def head_eval(sd, tap, defect=None):
    """(out [B, Cout, T], u [B, C, T], g = gelu(u)) in the dtype of `sd` from the last block's tap.  defect: "stats256" (GroupNorm
    statistics over the first 256 rows only), "left256", "right_end" (as in stem_ref, on the rows of gelu(u))."""
    w, b = sd["predictor.out.1.weight"], sd["predictor.out.1.bias"]
    h = tap.to(w.dtype)
    gw, gb = sd["predictor.out.0.0.weight"], sd["predictor.out.0.0.bias"]
    groups = ref_cpu.gn_groups(gw.shape[0])
    if defect == "stats256":
        B, C, T = h.shape
        hg = h[:, :, :256].reshape(B, groups, -1)
        mean, var = hg.mean(dim=2), hg.var(dim=2, unbiased=False)
        u = (h.reshape(B, groups, -1) - mean[:, :, None]) / torch.sqrt(var[:, :, None] + 1e-5)
        u = u.reshape(B, C, T) * gw[None, :, None] + gb[None, :, None]
    else:
        u = F.group_norm(h, groups, gw, gb, eps=1e-5)
    g = F.gelu(u)
    out = F.conv1d(g, w, b, padding=1)
    if defect == "left256":
        out[:, :, 256] -= torch.einsum("oc,bc->bo", w[:, :, 0], g[:, :, 255])
    if defect == "right_end":
        out[:, :, -1] += torch.einsum("oc,bc->bo", w[:, :, 2], torch.roll(g, -1, dims=0)[:, :, 0])
    return out, u, g


def gn_stats_term(sd64, tap):
    """[B, C, T]: how far the one-pass float32 statistics can move u (module docstring), inf where they decide nothing."""
    gw = sd64["predictor.out.0.0.weight"]
    B, C, T = tap.shape
    groups = ref_cpu.gn_groups(C)
    hg = tap.double().reshape(B, groups, -1)
    K = min(T, 256) + 1
    mean, var = hg.mean(dim=2, keepdim=True), hg.var(dim=2, unbiased=False, keepdim=True) + 1e-5
    dmean = K * U * hg.abs().mean(dim=2, keepdim=True)
    dvar = 3 * K * U * (hg * hg).mean(dim=2, keepdim=True)
    rstd = var.rsqrt()
    drstd = torch.where(dvar < var, (var - dvar).clamp(min=1e-300).rsqrt() - rstd, torch.full_like(var, float("inf")))
    du = rstd * dmean + ((hg - mean).abs() + dmean) * drstd
    return du.reshape(B, C, T) * gw.abs()[None, :, None]


def head_ref(model, tap, mode, defect=None):
    """dict(want, bound [B, Cout, T], eref) of the model's output in float64 from the last block's tap as read back."""
    sd64 = state(model)
    want, u, g = head_eval(sd64, tap.double(), defect)
    er = e_ref(want, head_eval(state(model, torch.float32), tap.float(), defect)[0])
    w = sd64["predictor.out.1.weight"]
    B, C, T = u.shape
    sumw = F.conv1d(torch.ones(1, C, T, dtype=torch.float64), w.abs(), padding=1)  # [1, Cout, T]: the taps that exist
    umax = F.max_pool1d(u.abs().amax(dim=1, keepdim=True), 3, 1, padding=1)  # [B, 1, T]: every |u| the element reads
    lo, hi = HEAD_GELU[mode]
    bound = torch.where(umax <= 4.0, lo, hi) * sumw + 8.0 * er + F.conv1d(GELU_SLOPE * gn_stats_term(sd64, tap), w.abs(), padding=1)
    return dict(want=want, bound=bound, eref=er)
