"""The reference of tests/test_backward_schedules_gpu.py, on the CPU: the float64 guidance gradient (tests/backward_ref.py) is the same
program as the float32 oracle that the reference project's fixtures pin, so the two may differ by float32 rounding only.

The bound on that difference is a condition on the reference alone: 2e-5 relative RMS, over the batch and for every clip.  (float32
autograd through at most 27 ResBlocks measures 1e-6 ... 4e-6 here; 2e-5 is two orders below the tightest gate any GPU gradient is
held to, so a float64 reference that passes cannot move a GPU verdict.)  For clf_f15a the float32 oracle must give the reference
project's own gradient and logits (fixture F15, tag c_a) exactly, and the float64 run is held to that fixture at the same 2e-5."""
import pytest
import torch

import backward_ref as R

torch.set_num_threads(8)
REF_TOL = 2e-5


@pytest.fixture(scope="module")
def f64(lib_built):
    return {c["id"]: R.oracle(c, torch.float64) for c in R.CASES}


def test_cases_are_the_shapes_they_claim():
    lens = {"clf_ragged": (3, 592, 12), "clf_default": (2, 2560, 27), "ep32": (3, 1792, None), "ep96": (2, 1792, None)}
    for cid, (B, T, blocks) in lens.items():
        c = R.CASE[cid]
        x, ts, y, _ = R.inputs(c)
        assert tuple(x.shape) == (B, 1, T) and tuple(ts.shape) == (B,) and x.dtype == ts.dtype == torch.float32
        assert y.dtype == torch.int64 and tuple(y.shape) == ((B,) if c["family"] == "clf" else (B, T // 256))
        if blocks:
            assert R.n_resblocks(c) == blocks
    assert R.n_resblocks(R.CASE["clf_f15a"]) == 8 and R.n_resblocks(R.CASE["ep32"]) == R.n_resblocks(R.CASE["ep96"])
    assert R.make_model(R.CASE["clf_ragged"]).downsample_rate == 16 and 592 // 16 == 37
    assert len({c["prefix"] for c in R.CASES}) == len(R.CASES)
    # the seeds are fixed: two draws agree
    assert all(torch.equal(a, b) for c in R.CASES for a, b in zip(R.inputs(c)[:3], R.inputs(c)[:3]))


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES if "fixture" not in c])
def test_float32_oracle_is_within_rounding_of_the_float64_reference(cid, f64):
    case = R.CASE[cid]
    g32, l32 = R.oracle(case, torch.float32)
    g64, l64 = f64[cid]
    assert g64.dtype == torch.float64 and g32.dtype == torch.float32 and bool(torch.isfinite(g64).all()) and g64.abs().max() > 0
    err, clip = R.rel_rms(g32, g64), R.clip_rel_rms(g32, g64)
    print(f"[margin] {cid}: float32 oracle against float64: grad {err:.3e}, worst clip {clip.max().item():.3e}, logits {R.rel_rms(l32, l64):.3e}")
    assert err < REF_TOL and clip.max().item() < REF_TOL, (cid, err, clip.tolist())
    assert R.rel_rms(l32, l64) < REF_TOL


def test_f15a_oracle_is_the_reference_projects_gradient(f64):
    case = R.CASE["clf_f15a"]
    want_g, want_l = R.fixture(case)
    g32, l32 = R.oracle(case, torch.float32)
    assert torch.equal(l32, want_l) and torch.equal(g32, want_g)
    g64, l64 = f64["clf_f15a"]
    err, clip = R.rel_rms(want_g, g64), R.clip_rel_rms(want_g, g64)
    print(f"[margin] clf_f15a: fixture against float64: grad {err:.3e}, worst clip {clip.max().item():.3e}, logits {R.rel_rms(want_l, l64):.3e}")
    assert err < REF_TOL and clip.max().item() < REF_TOL and R.rel_rms(want_l, l64) < REF_TOL


def test_fp32_gates_follow_the_recorded_run():
    """profiles/backward_schedule_margins.jsonl is one whole GPU run of tests/test_backward_schedules_gpu.py (4 schedules x 5 cases x 2
    modes against the reference, 3 x 5 x 2 against the default schedule); the fp32 gradient gates are `fp32_gate` of it, and every
    recorded error sits inside its gate with the factor of three to spare."""
    import json
    import os

    path = os.path.join(os.path.dirname(R.GOLDEN), os.pardir, "profiles", R.MARGINS)
    recs = [json.loads(ln) for ln in open(path)]
    runs = [r for r in recs if r["test"] == "backward_schedules"]
    assert len({(r["schedule"], r["case"], r["prec"]) for r in runs}) == len(runs) == 4 * len(R.CASES) * 2
    assert len([r for r in recs if r["test"] == "backward_schedules.vs_default"]) == 3 * len(R.CASES) * 2
    for family in ("clf", "ep"):
        assert R.GRAD_GATE[family]["fp32"] == R.fp32_gate(recs, family) <= R.GRAD_GATE_CAP, (family, R.fp32_gate(recs, family))
    for r in runs:
        gate = R.GRAD_GATE[R.CASE[r["case"]]["family"]][r["prec"]]
        assert max(r["grad_err"], r["grad_err_worst_clip"]) * (3 if r["prec"] == "fp32" else 1) <= gate and r["logit_err"] < R.LOGIT_GATE[r["prec"]], r
    assert R.fp32_gate([dict(test="backward_schedules", prec="fp32", case="ep32", grad_err=1e-4, grad_err_worst_clip=1.0001e-4)], "ep") == 4e-4
    assert R.fp32_gate([dict(test="backward_schedules", prec="fp32", case="ep32", grad_err=1e-4, grad_err_worst_clip=1e-4)], "ep") == 3e-4
    assert R.fp32_gate([dict(test="backward_schedules", prec="fp32", case="ep32", grad_err=1e-3, grad_err_worst_clip=1e-4)], "ep") == 2e-3
