"""The guidance backward has two schedules for the same mathematics (`resblock_backward` in csrc/net.cpp).  The default one multiplies by
GELU' and forms the partial sums S1 = sum du, S2 = sum du * u in conv_mfma_kernel's epilogue (per convolution tile), and evaluates the
mid-block d h1 = P * du2 + Q * h1 + R in conv1^T's prologue.  VQVS_BW_FUSE=0 runs bw_act_kernel after every transposed convolution
instead (same-resolution form, column-slice form on concatenating blocks, partial sums per STAT_TILE rows) and leaves the transposed
convolutions without an epilogue, so that the 2-byte modes route them to conv_ws_kernel; VQVS_BW_AFF2=0 runs the mid-block bw_affine
as a launch of its own, in place.  This file runs all four combinations on the cases of tests/backward_ref.py, in both gate modes:

  * every schedule against the float64 reference (the reference project's own fixture for clf_f15a), over the batch and for the
    worst clip, gradient and logits;
  * a repeat call bitwise equal (a race shows as nondeterminism), and every clip run alone bitwise equal to that clip in the batch;
  * the op table of every handle (`handle.op_info`), which proves that the switches changed the schedule: without it a broken or
    renamed switch would let four identical runs pass;
  * the schedules against each other (fp32 mode: closer to the default schedule than the default schedule is to float64).

The switches are read once per process, so every schedule runs in an interpreter of its own, one after another, each under its own
time limit.  A child that ends in anything but a clean verdict (a signal, a time limit, an unexpected exit status) stops the file: no
further child is started on the GPU and nothing is retried."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import backward_ref as R
from util import record_margin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = R.MARGINS
CHILD_SECONDS = 300
PRECS = ("fp32", "fp16")

SCHEDULES = [("default", {}), ("aff2_0", {"VQVS_BW_AFF2": "0"}), ("fuse_0", {"VQVS_BW_FUSE": "0"}),
             ("both_0", {"VQVS_BW_AFF2": "0", "VQVS_BW_FUSE": "0"})]
SWITCHES = ("VQVS_BW_AFF2", "VQVS_BW_FUSE")

# Gates, relative RMS against the reference, over the batch and for the worst clip alike (tests/backward_ref.py).  fp16 and the logits: the
# project's figures.  fp32 gradient: 3 x the largest error of the recorded run (profiles/backward_schedule_margins.jsonl: 1.008e-4 for
# the classifiers, 1.026e-4 for the EncoderPredictors, both at the worst clip of the default schedule), rounded up: 4e-4, a fifth of the
# project's 2e-3.
GRAD_GATE, LOGIT_GATE = R.GRAD_GATE, R.LOGIT_GATE

SCRIPT = r"""
import collections, json, os, sys
spec = json.loads(sys.argv[1])
ref_path, out_path = sys.argv[2], sys.argv[3]
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import torch
import backward_ref as R
from util import record_margin

def run(m, case, x, ts, y, scale):
    # (gradient, the logits of the same call, the forward output)
    if case["family"] == "clf":
        g, lg = m.log_prob_grad(x, ts, y, scale, return_logits=True)
        return g, lg, m(x, ts)
    g = m.guidance_grad(x, ts, y, scale)
    lg = m(x, ts)
    return g, lg, lg

def main():
    dev = torch.device("cuda:0")
    torch.set_num_threads(8)
    refs = np.load(ref_path)
    failures, grads = [], {{}}
    for case in R.CASES:
        cid, fam = case["id"], case["family"]
        m = R.make_model(case).to(dev)
        x, ts, y, scale = R.inputs(case)
        B, T = x.shape[0], x.shape[2]
        x, ts, y = x.to(dev), ts.to(dev), y.to(dev)
        want_g, want_l = torch.from_numpy(refs[cid + ".grad"]), torch.from_numpy(refs[cid + ".logits"])
        for prec in spec["precs"]:
            tag = f"{{cid}}.{{prec}}"
            m.set_precision(prec)
            g, lg, fwd = run(m, case, x, ts, y, scale)
            g2, lg2, _ = run(m, case, x, ts, y, scale)  # a race shows up as nondeterminism
            alone = [run(m, case, x[i:i + 1], ts[i:i + 1], y[i:i + 1], scale) for i in range(B)]
            torch.cuda.synchronize()
            ops = collections.Counter(kind for kind, _by, _fl in m.handle(dev, B, T).op_info(B, T))
            print("BWS_OPS " + json.dumps(dict(schedule=spec["schedule"], case=cid, prec=prec, ops=dict(ops))), flush=True)
            gc, lc = g.cpu(), lg.cpu()
            assert gc.shape == want_g.shape and lc.shape == want_l.shape, (tag, gc.shape, lc.shape)
            clip = R.clip_rel_rms(gc, want_g)
            worst = int(clip.argmax())
            rec = dict(test="backward_schedules", schedule=spec["schedule"], case=cid, prec=prec, ref="fixture" if "fixture" in case else "float64",
                       grad_err=R.rel_rms(gc, want_g), grad_err_worst_clip=clip[worst].item(), worst_clip=worst, grad_gate=spec["grad_gate"][fam][prec],
                       logit_err=R.rel_rms(lc, want_l), logit_gate=spec["logit_gate"][prec])
            record_margin(spec["margins"], rec)
            print("BWS_RESULT " + json.dumps(rec), flush=True)
            grads[tag] = gc.numpy()
            if not bool(torch.isfinite(gc).all()):
                failures.append(f"{{tag}}: the gradient is not finite")
            if not rec["grad_err"] < rec["grad_gate"]:
                failures.append(f"{{tag}}: gradient over the batch {{rec['grad_err']:.3e}} >= {{rec['grad_gate']:.1e}}")
            if not rec["grad_err_worst_clip"] < rec["grad_gate"]:
                failures.append(f"{{tag}}: gradient of clip {{worst}} {{rec['grad_err_worst_clip']:.3e}} >= {{rec['grad_gate']:.1e}}")
            if not rec["logit_err"] < rec["logit_gate"]:
                failures.append(f"{{tag}}: logits {{rec['logit_err']:.3e}} >= {{rec['logit_gate']:.1e}}")
            if not torch.equal(fwd, lg):
                failures.append(f"{{tag}}: the forward output differs from the logits of the gradient call")
            if not (torch.equal(g2, g) and torch.equal(lg2, lg)):
                failures.append(f"{{tag}}: a repeat call changed {{int((g2 != g).sum())}} gradient samples")
            for i, (g1, l1, _) in enumerate(alone):
                if not (torch.equal(g1[0], g[i]) and torch.equal(l1[0], lg[i])):
                    failures.append(f"{{tag}}: clip {{i}} alone differs bitwise from the batch in {{int((g1[0] != g[i]).sum())}} gradient samples")
        del m
    np.savez(out_path, **grads)
    return failures

failures = main()
for f in failures:
    print("BWS_FAILURE " + f, flush=True)
print("BWS_VERDICT " + ("FAIL" if failures else "OK"), flush=True)
sys.exit(1 if failures else 0)
"""


def _lines(stdout, key):
    return [json.loads(ln[len(key) + 1:]) for ln in stdout.splitlines() if ln.startswith(key + " ")]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{schedule: dict(started, clean, ok, text, results, ops, grads)}: the float64 reference once, on the CPU, handed to the children in
    an .npz; then one child per schedule, in the order of SCHEDULES, stopping at the first that ends without a clean verdict."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.set_num_threads(8)
    tmp = tmp_path_factory.mktemp("backward_schedules")
    ref = {}
    for cid, (g, lg) in R.references().items():
        ref[cid + ".grad"], ref[cid + ".logits"] = g.numpy(), lg.numpy()
    np.savez(tmp / "ref.npz", **ref)
    script = tmp / "child.py"
    script.write_text(SCRIPT.format(root=ROOT))
    out, stopped = {}, None
    for name, switches in SCHEDULES:
        if stopped:
            out[name] = dict(started=False, clean=False, ok=False, text=f"not started: schedule {stopped} ended without a clean verdict")
            continue
        spec = dict(schedule=name, precs=PRECS, grad_gate=GRAD_GATE, logit_gate=LOGIT_GATE, margins=MARGINS)
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(switches)
        grads = tmp / f"grads_{name}.npz"
        try:
            r = subprocess.run([sys.executable, str(script), json.dumps(spec), str(tmp / "ref.npz"), str(grads)], capture_output=True, text=True,
                               env=env, timeout=CHILD_SECONDS)
            rc, so, se = r.returncode, r.stdout, r.stderr
        except subprocess.TimeoutExpired as ex:
            dec = lambda b: b.decode(errors="replace") if isinstance(b, bytes) else (b or "")  # noqa: E731
            rc, so, se = f"no verdict within {CHILD_SECONDS} s", dec(ex.stdout), dec(ex.stderr)
        clean = (rc == 0 and "BWS_VERDICT OK" in so) or (rc == 1 and "BWS_VERDICT FAIL" in so)
        if not clean:
            stopped = name
        out[name] = dict(started=True, clean=clean, ok=rc == 0 and "BWS_VERDICT OK" in so, text=f"exit status {rc}\n{so[-12000:]}\n{se[-4000:]}",
                         results={(r["case"], r["prec"]): r for r in _lines(so, "BWS_RESULT")},
                         ops={(r["case"], r["prec"]): r["ops"] for r in _lines(so, "BWS_OPS")}, grads=grads)
    return out


@pytest.mark.parametrize("schedule", [s for s, _ in SCHEDULES])
def test_schedule_against_reference(schedule, runs):
    """Gradient (batch and worst clip) and logits inside the gates, repeat calls and single-clip calls bitwise equal: the child's verdict."""
    run = runs[schedule]
    print(run["text"])
    assert run["started"], run["text"]
    assert run["ok"], f"{schedule}: {run['text']}"
    assert set(run["results"]) == {(c["id"], p) for c in R.CASES for p in PRECS}


def _need(runs, *names):
    for n in names:
        assert runs[n]["started"] and runs[n]["clean"], f"schedule {n} gave no results: {runs[n]['text'][:300]}"


def test_switches_change_the_op_table(runs):
    """The coverage proof, read from the op table of every handle: VQVS_BW_FUSE=0 adds at least one bw_act per ResBlock (conv2^T's; conv1^T's
    too unless the block resizes, where the default schedule already has one; two on a concatenating block, and one for the
    EncoderPredictor's output convolution), VQVS_BW_AFF2=0 adds exactly one bw_affine per ResBlock, and neither changes the other count."""
    _need(runs, *(s for s, _ in SCHEDULES))
    for case in R.CASES:
        n = R.n_resblocks(case)
        for prec in PRECS:
            k = (case["id"], prec)
            ops = {s: runs[s]["ops"][k] for s, _ in SCHEDULES}
            print(f"[ops] {case['id']} {prec} ({n} ResBlocks): " + "; ".join(
                f"{s}: bw_act {o.get('bw_act', 0)}, bw_affine {o.get('bw_affine', 0)}, conv {o.get('conv', 0)}, {sum(o.values())} ops" for s, o in ops.items()))
            d = ops["default"]
            for s in ("fuse_0", "both_0"):
                assert ops[s].get("bw_act", 0) - d.get("bw_act", 0) >= n, (k, s, ops[s], d)
            for s in ("aff2_0", "both_0"):
                assert ops[s]["bw_affine"] - d["bw_affine"] == n, (k, s, ops[s], d)
            assert ops["aff2_0"].get("bw_act", 0) == d.get("bw_act", 0) and ops["fuse_0"]["bw_affine"] == d["bw_affine"], (k, ops)
            assert all(o["conv"] == d["conv"] and o["gn_bw"] == d["gn_bw"] for o in ops.values()), (k, ops)
    for prec in PRECS:
        assert runs["default"]["ops"][("ep32", prec)].get("bw_act", 0) >= 1  # the nearest-x2 blocks keep the separate kernel


def test_schedules_against_each_other(runs):
    """d: the relative RMS difference of every other schedule's gradient from the default schedule's, over the batch and for the worst clip.
    Recorded in both modes.  fp32 mode: d < e_default, the default schedule's own error against the reference in this run -- both
    schedules form 3-term bf16-split MFMA products with fp32 accumulation and differ only in how the partial sums are grouped and in
    where one fp32 affine is applied, so they must sit closer to each other than either sits to float64.  (fp16 mode: VQVS_BW_FUSE=0
    rounds du to fp16 once more per convolution, d is of the order of the error itself: recorded only.)
    Recorded (profiles/backward_schedule_margins.jsonl): VQVS_BW_AFF2=0 alone gives d = 0 in both modes -- bw_affine_kernel and the AFF2
    prologue evaluate the same fmaf(P, du, fmaf(Q, h1, R)) and round once to the same operand format; VQVS_BW_FUSE=0 gives d = 4.9e-6 ...
    1.5e-5 in the fp32 mode, 0.12 ... 0.21 of e_default, and 1.2e-3 ... 2.4e-3 in the fp16 mode, 0.22 ... 0.57 of e_default."""
    _need(runs, "default")
    base = np.load(runs["default"]["grads"])
    compared, failures = 0, []
    for s, _ in SCHEDULES[1:]:
        if not (runs[s]["started"] and runs[s]["clean"]):
            failures.append(f"schedule {s} gave no results")
            continue
        got = np.load(runs[s]["grads"])
        for case in R.CASES:
            for prec in PRECS:
                tag = f"{case['id']}.{prec}"
                g, g0 = torch.from_numpy(got[tag]), torch.from_numpy(base[tag])
                clip = R.clip_rel_rms(g, g0)
                e0 = runs["default"]["results"][(case["id"], prec)]
                rec = dict(test="backward_schedules.vs_default", schedule=s, case=case["id"], prec=prec, d=R.rel_rms(g, g0),
                           d_worst_clip=clip.max().item(), e_default=e0["grad_err"], e_default_worst_clip=e0["grad_err_worst_clip"],
                           gated=prec == "fp32")
                record_margin(MARGINS, rec)
                compared += 1
                if prec == "fp32" and not rec["d"] < rec["e_default"]:
                    failures.append(f"{s} {tag}: d = {rec['d']:.3e} is not below the default schedule's own error {rec['e_default']:.3e}")
    assert not failures, "\n".join(failures)
    assert compared == 3 * len(R.CASES) * len(PRECS)
