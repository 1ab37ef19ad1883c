"""The cases and the float64 reference of tests/test_backward_schedules.py and tests/test_backward_schedules_gpu.py: the guidance
gradient d log p / d x_t through the classifier stem and through the whole EncoderPredictor UNet.

The reference is `oracle.ref_cpu.classifier_cond_fn` / `encoder_predictor_cond_fn` run on a float64 state dict with float64 `x` and
`ts`: ref_cpu is dtype-generic, so this is float64 autograd of the same program text that the reference project's fixtures pin in
float32 (tests/test_backward_schedules.py ties the two together).  The models are the smallest that still reach every form of the
backward kernels (csrc/backward_kernels.hip, `resblock_backward` in csrc/net.cpp):

  clf_f15a     the reference project's own gradient (fixture F15, tag c_a): 8 blocks, T = 4096
  clf_ragged   level lengths 592 / 296 / 148 / 74: two whole 256-row partial-sum tiles and a ragged one, one and a ragged one, single
               partial tiles; avg-pool backward (BW_FROM_HALF) and non-resizing blocks; a head of 37 tokens
  clf_default  the default 27-block topology down to 5 tokens, 10 tiles at the top level
  ep32         whole-UNet backward: concatenating blocks (column slices c0 / Ctot, one gn_bw over the joint partials), nearest x2
               (BW_FROM_DOUBLE), bw_add, enc_head_kernel with 7 of its 64 positions live; the second level is 896 rows = 3.5 tiles
  ep96         octet counts that are no power of two: bw_act's rpp = 256 / opr leaves idle threads, in_conv_bw_rows_kernel runs
"""
import os

import numpy as np
import torch

from oracle import ref_cpu
from vq_voice_swap_amd import Classifier, EncoderPredictor
from vq_voice_swap_amd.det_init import det_init_

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F15A = dict(channel_mult=(1, 2, 2, 4), output_mult=8, depth_mult=1)

CASES = [
    dict(id="clf_f15a", family="clf", labels=5, base=32, kw=F15A, prefix="clf.c_a.", fixture=("f15_custom_classifiers", "c_a")),
    dict(id="clf_ragged", family="clf", labels=5, base=32, kw=dict(channel_mult=(1, 2, 2, 4), output_mult=8, depth_mult=2),
         prefix="bws.clf_ragged.", B=3, T=16 * 37, ts=("linspace", 0.1, 0.9), y=(0, 2, 4), scale=1.0, x_seed=7101),
    dict(id="clf_default", family="clf", labels=5, base=32, kw={}, prefix="bws.clf_default.", B=2, T=512 * 5, ts=(0.1, 0.9), y=(0, 2),
         scale=1.0, x_seed=7102),
    dict(id="ep32", family="ep", base=32, rate=256, latents=40, bottleneck=32, prefix="bws.ep32.", B=3, T=256 * 7,
         ts=("linspace", 0.2, 0.9), y_seed=5, scale=2.0, x_seed=7103),
    dict(id="ep96", family="ep", base=96, rate=256, latents=40, bottleneck=64, prefix="bws.ep96.", B=2, T=256 * 7, ts=(0.3, 0.8),
         y_seed=6, scale=1.0, x_seed=7104),
]
CASE = {c["id"]: c for c in CASES}

# Gates of the GPU file: relative RMS against the reference, the worst clip held to the same figure as the batch.
# fp16, and the logits in both modes: the project's figures (tests/test_classifier.py, tests/test_encoder_predictor.py).
# fp32 gradient: the project's figure 2e-3 is the cap; the gate is `fp32_gate` of the recorded run profiles/backward_schedule_margins.jsonl
# (tests/test_backward_schedules.py checks that it is).
GRAD_GATE_CAP = 2e-3
GRAD_GATE = {"clf": {"fp32": 4e-4, "fp16": 3e-2}, "ep": {"fp32": 4e-4, "fp16": 4e-2}}
LOGIT_GATE = {"fp32": 2e-4, "fp16": 8e-3}
MARGINS = "backward_schedule_margins.jsonl"


def fp32_gate(records, family):
    """3 x the largest fp32 error against the reference (batch or worst clip) that `records` hold for a model family, over all
    schedules and cases, rounded up to one significant digit, never above GRAD_GATE_CAP.  3 x: the kernels are deterministic on fixed
    inputs; what can move a value is the CU count (it regroups conv_ws_kernel's walks) and the compiler version."""
    import math

    errs = [max(r["grad_err"], r["grad_err_worst_clip"]) for r in records
            if r.get("test") == "backward_schedules" and r["prec"] == "fp32" and CASE[r["case"]]["family"] == family]
    v = 3.0 * max(errs)
    e = math.floor(math.log10(v))
    return min(GRAD_GATE_CAP, float(f"{math.ceil(v / 10.0 ** e - 1e-9)}e{e}"))


def make_model(case):
    """The module of a case on the CPU: det_init_ under the case's prefix, eval()."""
    if case["family"] == "clf":
        m = Classifier(case["labels"], base_channels=case["base"], **case["kw"])
    else:
        m = EncoderPredictor(case["base"], case["rate"], num_latents=case["latents"], bottleneck_dim=case["bottleneck"])
    det_init_((case["prefix"] + k, v) for k, v in m.state_dict().items())
    return m.eval()


def n_resblocks(case):
    if case["family"] == "clf":
        kw = case["kw"]
        return len(kw.get("channel_mult", ref_cpu.CHANNEL_MULT)) * (kw.get("depth_mult", ref_cpu.DEPTH_MULT) + 1)
    return sum(len(v) for v in ref_cpu.predictor_block_specs(case["base"]).values())


def inputs(case):
    """(x [B, 1, T] float32, ts [B] float32, y int64 (labels [B] or targets [B, T // rate]), scale)."""
    if "fixture" in case:
        name, tag = case["fixture"]
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        return tuple(torch.from_numpy(z[f"{tag}.{k}"]) for k in ("x", "ts", "labels")) + (1.0,)
    B, T = case["B"], case["T"]
    x = torch.randn((B, 1, T), generator=torch.Generator().manual_seed(case["x_seed"]))
    ts = torch.linspace(case["ts"][1], case["ts"][2], B) if case["ts"][0] == "linspace" else torch.tensor(case["ts"], dtype=torch.float32)
    if case["family"] == "clf":
        y = torch.tensor(case["y"], dtype=torch.int64)
    else:
        y = torch.randint(0, case["latents"], (B, T // case["rate"]), generator=torch.Generator().manual_seed(case["y_seed"]))
    return x, ts, y, case["scale"]


def fixture(case):
    """(grad, logits) of the reference project itself, float32, for a case that has a fixture."""
    name, tag = case["fixture"]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return torch.from_numpy(z[tag + ".grad"]), torch.from_numpy(z[tag + ".logits"])


def oracle(case, dtype=torch.float64, model=None):
    """(grad [B, 1, T], logits) of the CPU oracle with parameters, x and ts in `dtype`."""
    m = model if model is not None else make_model(case)
    sd = {k: v.detach().to(dtype) for k, v in m.state_dict().items()}
    x, ts, y, scale = inputs(case)
    x, ts = x.to(dtype), ts.to(dtype)
    if case["family"] == "clf":
        kw = case["kw"]
        topo = dict(channel_mult=kw["channel_mult"], depth_mult=kw["depth_mult"]) if kw else None
        logits = ref_cpu.classifier(sd, case["base"], x, ts, topology=topo)
        grad = ref_cpu.classifier_cond_fn(sd, case["base"], y, scale, topology=topo)(x, ts)
    else:
        logits = ref_cpu.encoder_predictor(sd, case["base"], x, ts, case["rate"])
        grad = ref_cpu.encoder_predictor_cond_fn(sd, case["base"], case["rate"], y, scale)(x, ts)
    assert grad.dtype == dtype and logits.dtype == dtype
    return grad.detach(), logits.detach()


def rel_rms(got, want):
    """Relative RMS difference over the whole batch, in float64."""
    got, want = got.double(), want.double()
    return ((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt()).item()


def clip_rel_rms(got, want):
    """Relative RMS difference of every clip alone, float64 [B]."""
    got, want = got.double().flatten(1), want.double().flatten(1)
    return (got - want).pow(2).mean(dim=1).sqrt() / want.pow(2).mean(dim=1).sqrt()


def references():
    """{id: (grad, logits)}, what the GPU gradient is held to: the reference project's float32 fixture for clf_f15a, the float64
    oracle for every other case."""
    return {c["id"]: fixture(c) if "fixture" in c else oracle(c) for c in CASES}
