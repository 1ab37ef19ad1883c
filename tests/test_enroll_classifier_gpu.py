"""Classifier enrolment on the GPU (csrc/enroll_kernels.hip: head_xent_grad_kernel, head_adamw_kernel; `ClassifierEnroller`,
enroll_classifier.py) against the references of tests/enroll_head_ref.py:

  * `vqvs_head_xent_grad` against an extended-precision restatement on the shapes and kinds of `enroll_head_ref`: nll, coef and
    new_mass within the DERIVED bound (the share of it that is used is recorded), top1 exact, the stored logits within one float32
    ulp, the GELU at the project's tolerance, repeat and single-clip calls bitwise;
  * `vqvs_head_adamw` within one float32 ulp of the float64 step on the same float32 state, the untouched row bitwise;
  * after `finish()` the grown classifier's own forward gives the enroller's logits, the old columns bit for bit the un-grown model's;
  * three steps against float64 autograd + torch.optim.AdamW on the float64 stem's features; the loss on a fixed batch over 20 steps;
  * guidance towards an enrolled label: `log_prob_grad` against float64 autograd of the grown classifier -- what the feature is for;
  * the script end to end, each run in a fresh child process.

Every error is printed and recorded (profiles/enroll_classifier_margins.jsonl is one GPU run of this file) before it is gated."""

import numpy as np
import pytest
import torch

import backward_ref as BR
import enroll_head_ref as H
from oracle import ref_cpu
from util import record_margin, run_script
from vq_voice_swap_amd import Classifier, _native
from vq_voice_swap_amd.det_init import det_init_
from vq_voice_swap_amd.enroll import ClassifierEnroller, head_adamw_step, head_xent_grad

pytestmark = pytest.mark.gpu
SHAPE_IDS = ["x".join(str(v) for v in s) for s in H.XENT_SHAPES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.set_num_threads(8)
    return torch.device("cuda:0")


def _cpu(out):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


# ---- vqvs_head_xent_grad -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("shape", H.XENT_SHAPES, ids=SHAPE_IDS)
def test_head_xent_grad_against_float64(shape, kind, dev):
    B, K, n, F = shape
    c = H.make_case(shape, kind)
    feat, w_old, b_old, rows, y = (c[k].to(dev) for k in ("feat", "w_old", "b_old", "rows", "targets"))
    got = _cpu(head_xent_grad(feat, w_old, b_old, rows, y))
    again = _cpu(head_xent_grad(feat, w_old, b_old, rows, y))
    alone = [_cpu(head_xent_grad(feat[i:i + 1], w_old, b_old, rows, y[i:i + 1])) for i in range(B)]
    torch.cuda.synchronize()
    assert all(np.isfinite(got[k]).all() for k in ("nll", "coef", "new_mass", "logits", "act"))
    act_err = float(np.abs(got["act"].astype(np.float64) - H.gelu64(c["feat"].numpy())).max())
    ref = H.head_ref(got["act"], c["w_old"].numpy(), c["b_old"].numpy(), c["rows"].numpy(), c["targets"].numpy(), dtype=H.XL)
    share = H.share_of_bound(got, ref, F, K, n)
    ulp = float(H.ulps_f32(got["logits"], ref["logits"].astype(np.float64)).max())
    lo, hi = c["tie"]
    rec = dict(test="enroll_classifier.xent", shape=list(shape), kind=kind, share_nll=share["nll"], share_coef=share["coef"],
               share_new_mass=share["new_mass"], logits_ulp=ulp, act_err=act_err, nll_max=float(got["nll"].max()),
               new_mass_min=float(got["new_mass"].min()), top1=got["top1"].tolist())
    record_margin(H.MARGINS, rec)
    assert share["nll"] < 1 and share["coef"] < 1 and share["new_mass"] < 1, rec
    assert (got["top1"] == ref["top1"]).all() and got["top1"][0] == 1 and (B == 1 or got["top1"][1] == 0), (got["top1"], ref["top1"])
    assert got["logits"][0, lo] == got["logits"][0, hi] == got["logits"][0].max()  # the duplicated rows tie bitwise
    assert ulp <= 1 and act_err <= H.ACT_TOL, rec
    for k in ("nll", "coef", "new_mass", "logits", "act", "top1"):
        assert np.array_equal(got[k], again[k]), f"{k}: a repeat call differs"
        for i in range(B):
            assert np.array_equal(alone[i][k][0], got[k][i]), f"{k}: clip {i} alone differs from the batch"


def test_head_xent_grad_refuses_a_label_outside_the_grown_model(dev):
    """The binding raises IndexError; the library itself never indexes with such a target: that clip's nll and coef row are NaN, its
    top1 0, and the clips beside it keep their bits."""
    B, K, n, F = shape = (3, 5, 2, 33)
    c = H.make_case(shape, "plain")
    feat, w_old, b_old, rows = (c[k].to(dev) for k in ("feat", "w_old", "b_old", "rows"))
    good = _cpu(head_xent_grad(feat, w_old, b_old, rows, c["targets"].to(dev)))
    for bad in (K + n, -1, 2 ** 40):
        y = c["targets"].clone()
        y[1] = bad
        with pytest.raises(IndexError):
            head_xent_grad(feat, w_old, b_old, rows, y.to(dev))
        y = y.to(dev)
        nll = torch.zeros(B, device=dev, dtype=torch.float64)
        coef = torch.zeros(B, n, device=dev, dtype=torch.float64)
        top1 = torch.full((B,), 7, device=dev, dtype=torch.int64)
        mass = torch.zeros(B, device=dev, dtype=torch.float64)
        _native.check(_native.lib().vqvs_head_xent_grad(feat.data_ptr(), w_old.data_ptr(), b_old.data_ptr(), rows.data_ptr(), y.data_ptr(), None,
                                                        None, nll.data_ptr(), top1.data_ptr(), mass.data_ptr(), coef.data_ptr(), B, F, K, n,
                                                        _native._stream_ptr()))
        nll, coef, top1, mass = nll.cpu().numpy(), coef.cpu().numpy(), top1.cpu().numpy(), mass.cpu().numpy()
        assert np.isnan(nll[1]) and np.isnan(coef[1]).all() and top1[1] == 0 and mass[1] == good["new_mass"][1], bad
        for i in (0, 2):
            assert nll[i] == good["nll"][i] and np.array_equal(coef[i], good["coef"][i]) and top1[i] == good["top1"][i], (bad, i)


# ---- vqvs_head_adamw ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", H.ADAMW_WD)
@pytest.mark.parametrize("shape", H.XENT_SHAPES, ids=SHAPE_IDS)
def test_head_adamw_against_float64(shape, wd, dev):
    """Seven steps from zero moments with a fresh (coef, act) per step, B in {1, 3, 8}: after steps 1 and 7 every stored value is
    within one float32 ulp of the float64 step taken from the float32 state the kernel started that step from.  With n >= 2 the last
    coef column is zero: at weight decay 0 that row and its moments keep their bits through all seven steps."""
    _, _, n, F = shape
    lr, betas, eps = H.HYPER["lr"], H.HYPER["betas"], H.HYPER["eps"]
    hyper = (H.f32(lr), (H.f32(betas[0]), H.f32(betas[1])), H.f32(eps), H.f32(wd))
    worst = 0.0
    for B in H.ADAMW_B:
        g = torch.Generator().manual_seed(9700 + 10 * H.XENT_SHAPES.index(shape) + B)
        rows0 = torch.randn(n, F + 1, generator=g) / np.sqrt(F)
        rows, m, v = rows0.to(dev), torch.zeros(n, F + 1, device=dev), torch.zeros(n, F + 1, device=dev)
        for step in range(1, max(H.ADAMW_STEPS) + 1):
            coef = 2 * torch.rand(B, n, generator=g, dtype=torch.float64) - 1
            if n >= 2:
                coef[:, -1] = 0
            act = torch.from_numpy(H.gelu64(1.5 * torch.randn(B, F, generator=g).numpy())).float()
            before = tuple(t.cpu().numpy().astype(np.float64) for t in (rows, m, v))
            head_adamw_step(rows, m, v, act.to(dev), coef.to(dev), step, lr, betas, eps, wd)
            if step in H.ADAMW_STEPS:
                want = H.adamw_update(*before, H.grad_ref(act.numpy(), coef.numpy()), step, *hyper)
                for name, t, w in zip(("rows", "m", "v"), (rows, m, v), want):
                    ulps = H.ulps_f32(t.cpu().numpy(), w)
                    worst = max(worst, float(ulps.max()))
                    assert ulps.max() <= 1, (name, B, step, float(ulps.max()))
        got = rows.cpu()
        assert not torch.equal(got[0], rows0[0])
        if n >= 2 and wd == 0.0:
            assert torch.equal(got[-1], rows0[-1]), "a row whose coef column is zero moved at weight decay 0"
            assert not m.cpu()[-1].any() and not v.cpu()[-1].any()
        elif n >= 2:
            assert not torch.equal(got[-1], rows0[-1])
    record_margin(H.MARGINS, dict(test="enroll_classifier.adamw", shape=list(shape), weight_decay=wd, worst_ulp=worst))


# ---- ClassifierEnroller on small classifiers ---------------------------------------------------------------------------------------
def _setup(case_id, dev, init, lr=1e-2, precision="fp32", T=None):
    """(case, model on the device, enroller of two new speakers, x_0 [4, 1, T], ts, noise, labels): three clips of the new speakers and
    one replay clip of old speaker 1, fixed (t, noise)."""
    case = BR.CASE[case_id]
    model = BR.make_model(case).to(dev)
    model.set_precision(precision)
    T = T or (case.get("T") or 4096)
    g = torch.Generator().manual_seed(9800 + len(case_id))
    x0 = 0.5 * torch.randn(4, 1, T, generator=g)
    noise = torch.randn(4, 1, T, generator=g)
    ts = torch.tensor([0.15, 0.4, 0.65, 0.9])
    K = case["labels"]
    labels = torch.tensor([K, K + 1, K, 1])
    en = ClassifierEnroller(model, 2, lr=lr, init=init)
    return case, model, en, x0.to(dev), ts, noise.to(dev), labels


def _topology(case):
    kw = case["kw"]
    return dict(channel_mult=kw["channel_mult"], depth_mult=kw["depth_mult"]) if kw else None


def _act64(case, model, x_t, ts):
    """gelu(feat) [B, F] of the float64 stem on float32 (x_t, ts): the oracle's classifier with an identity head."""
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    Fd = model.feature_dim
    sd["out.1.weight"], sd["out.1.bias"] = torch.eye(Fd, dtype=torch.float64), torch.zeros(Fd, dtype=torch.float64)
    return ref_cpu.classifier(sd, case["base"], x_t.cpu().double(), ts.cpu().double(), topology=_topology(case)).numpy()


def _trajectory(case_id, dev, precision, steps=3):
    case, model, en, x0, ts, noise, labels = _setup(case_id, dev, "zeros" if case_id == "clf_f15a" else "mean", precision=precision)
    rows0 = en.rows.cpu().numpy().astype(np.float64)
    head = model.out[1]
    w_old, b_old = head.weight.detach().cpu().double().numpy(), head.bias.detach().cpu().double().numpy()
    x_t = en.losses(x0, labels.to(dev), ts=ts, noise=noise)["x_t"]  # the reference sees the x_t the enroller forms
    # float64 autograd + torch.optim.AdamW on the float64 classifier: its stem is frozen, so its features are formed once
    auto = H.AutogradHead(w_old, b_old, rows0, lr=H.f32(1e-2), betas=(H.f32(0.9), H.f32(0.999)), eps=H.f32(1e-8))
    act64 = _act64(case, model, x_t, ts)
    ref_losses = [auto.step(act64, labels.numpy())[0] for _ in range(steps)]
    want = [auto.rows()]
    losses =[en.step(x0, labels.to(dev), ts=ts, noise=noise)["loss"].item() for _ in range(steps)]
    torch.cuda.synchronize()
    model.check_status()
    got = en.rows.cpu().numpy().astype(np.float64)
    assert en.steps == steps and np.isfinite(got).all()
    return dict(case=case_id, prec=precision, steps=steps, lr=1e-2, traj_err=H.rel_rms(got - rows0, want[-1] - rows0),
                loss_err=max(abs(a - b) / b for a, b in zip(losses, ref_losses)))


@pytest.mark.parametrize("case_id", H.TRAJ_CASES)
def test_three_steps_against_float64(case_id, dev):
    rec = dict(test="enroll.traj", **_trajectory(case_id, dev, "fp32"))
    record_margin(H.MARGINS, rec)
    half = dict(test="enroll_classifier.traj_fp16", **_trajectory(case_id, dev, "fp16"))  # recorded, not gated
    record_margin(H.MARGINS, half)
    assert rec["traj_err"] < H.GATES["traj"] and rec["loss_err"] < 1e-3, rec


def test_new_logits_equal_the_grown_models(dev):
    case, model, en, x0, ts, noise, labels = _setup("clf_ragged", dev, "mean")
    for _ in range(2):
        en.step(x0, labels.to(dev), ts=ts, noise=noise)
    out = en.losses(x0, labels.to(dev), ts=ts, noise=noise)
    x_t, K = out["x_t"], case["labels"]
    before = model(x_t, ts.to(dev)).cpu()
    assert tuple(before.shape) == (4, K) and tuple(out["logits"].shape) == (4, K + 2)
    assert en.finish() is model and model.num_labels == K + 2
    after = model(x_t, ts.to(dev)).cpu()
    torch.cuda.synchronize()
    model.check_status()
    assert tuple(after.shape) == (4, K + 2)
    assert torch.equal(after[:, :K], before), "the old logits changed"
    mine = out["logits"].cpu()
    rec = dict(test="enroll_classifier.logits", new_err=BR.rel_rms(after[:, K:], mine[:, K:]), old_err=BR.rel_rms(before, mine[:, :K]))
    record_margin(H.MARGINS, rec)
    assert rec["new_err"] < BR.LOGIT_GATE["fp32"] and rec["old_err"] < BR.LOGIT_GATE["fp32"], rec


def test_loss_falls_over_twenty_steps(dev):
    case, model, en, x0, ts, noise, labels = _setup("clf_ragged", dev, "zeros")
    head = model.out[1]
    w_old, b_old = head.weight.detach().cpu().double().numpy(), head.bias.detach().cpu().double().numpy()
    first = en.losses(x0, labels.to(dev), ts=ts, noise=noise)
    before = first["nll"].mean().item()
    for _ in range(20):
        en.step(x0, labels.to(dev), ts=ts, noise=noise)
    after = en.losses(x0, labels.to(dev), ts=ts, noise=noise)["nll"].mean().item()
    _, ref_losses = H.trajectory_ref(_act64(case, model, first["x_t"], ts), w_old, b_old, np.zeros((2, model.feature_dim + 1)), labels.numpy(), 21, 1e-2)
    print(f"[margin] NLL on the fixed batch: GPU {before:.6f} -> {after:.6f} after 20 steps; float64 {ref_losses[0]:.6f} -> {ref_losses[20]:.6f}")
    assert after < before and ref_losses[20] < ref_losses[0]


def test_guidance_reaches_a_new_label(dev):
    """After `finish()`, `log_prob_grad` towards the enrolled labels: finite, non-zero, and float64 autograd of the grown classifier."""
    case, model, en, x0, ts4, noise, labels = _setup("clf_ragged", dev, "mean")
    for _ in range(3):
        en.step(x0, labels.to(dev), ts=ts4, noise=noise)
    en.finish()
    K = case["labels"]
    x, ts, _, scale = BR.inputs(case)
    y = torch.tensor([K, K + 1, K])
    grad, logits = model.log_prob_grad(x.to(dev), ts.to(dev), y.to(dev), scale, return_logits=True)
    torch.cuda.synchronize()
    model.check_status()
    grad = grad.cpu()
    assert tuple(logits.shape) == (3, K + 2) and bool(torch.isfinite(grad).all()) and all(bool(grad[i].any()) for i in range(3))
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    want = ref_cpu.classifier_cond_fn(sd, case["base"], y, scale, topology=_topology(case))(x.double(), ts.double())
    clip = BR.clip_rel_rms(grad, want)
    rec = dict(test="enroll_classifier.guidance", case=case["id"], grad_err=BR.rel_rms(grad, want), grad_err_worst_clip=clip.max().item())
    record_margin(H.MARGINS, rec)
    gate = BR.GRAD_GATE["clf"]["fp32"]
    assert rec["grad_err"] < gate and rec["grad_err_worst_clip"] < gate, rec
    other = model.log_prob_grad(x.to(dev), ts.to(dev), torch.tensor([K + 1, K, K + 1]).to(dev), scale).cpu()
    assert not torch.equal(other, grad)  # the label is read, not clamped away


# ---- the script --------------------------------------------------------------------------------------------------------------------
def test_enroll_classifier_script_end_to_end(tmp_path, dev):
    """A det-init classifier of three labels, the synthetic tones as three new speakers and as the replay set: six steps, then a
    resumed run of two; the written checkpoint loads with `Classifier.load`, has six labels, the old rows bitwise, and scores a
    clip under an enrolled label.  Each run is a fresh child process."""
    model = Classifier(3, base_channels=32, channel_mult=(1, 2, 2, 4), output_mult=8, depth_mult=1)
    det_init_((("enrc.script." + k, v) for k, v in model.state_dict().items()))
    ckpt = tmp_path / "clf.pt"
    model.save(str(ckpt))
    out_dir = tmp_path / "added"
    args = ["tones", "--pretrained-path", ckpt, "--output-dir", out_dir, "--save-interval", "3", "--holdout", "2", "--lr", "1e-2", "--seed", "0",
            "--replay-dir", "tones", "--replay-batch", "4", "--curriculum-steps", "4"]
    text = run_script("enroll_classifier.py", args + ["--steps", "6"])
    steps = [ln for ln in text.splitlines() if ln.startswith("step ") and "loss=" in ln]
    assert [ln.split(":")[0] for ln in steps] == [f"step {i}" for i in range(1, 7)] and all(" acc=" in ln and " q" in ln for ln in steps), text
    held = [ln for ln in text.splitlines() if "holdout_nll=" in ln]
    assert [ln.split(":")[0] for ln in held] == ["step 3", "step 6"] and all(ln.endswith("(2 clips)") for ln in held), text
    assert all("holdout_acc=" in ln and 0 < float(ln.split("replay_new_mass=")[1].split(" ")[0]) < 1 for ln in held), text
    assert "resuming" not in text
    text = run_script("enroll_classifier.py", args + ["--steps", "2"])
    steps = [ln for ln in text.splitlines() if ln.startswith("step ") and "loss=" in ln]
    assert "resuming from" in text and [ln.split(":")[0] for ln in steps] == ["step 7", "step 8"], text
    grown = Classifier.load(str(out_dir / "model.pt"))
    w, b = grown.out[1].weight.detach(), grown.out[1].bias.detach()
    assert grown.num_labels == 6 and tuple(w.shape) == (6, 256) and tuple(b.shape) == (6,)
    assert torch.equal(w[:3], model.out[1].weight.detach()) and torch.equal(b[:3], model.out[1].bias.detach()), "the checkpoint's own rows changed"
    assert bool(torch.isfinite(w[3:]).all()) and bool(w[3:].any()) and not torch.equal(w[3], w[4])
    for k, v in model.state_dict().items():
        if not k.startswith("out.1."):
            assert torch.equal(grown.state_dict()[k], v), k
    state = torch.load(str(out_dir / "enroll.pt"), map_location="cpu")
    assert state["steps"] == 8 and state["first_label"] == 3 and tuple(state["rows"].shape) == (3, 257)
    # eval_conversion.py's classifier path: `Classifier.scores` at t = 0 under an enrolled label
    grown.to(dev).eval()
    x = 0.3 * torch.sin(2 * np.pi * 500.0 * torch.arange(4096) / 16000.0).repeat(2, 1, 1).to(dev)
    scores = grown.scores(x, torch.zeros(2, device=dev), torch.tensor([4, 5], device=dev))
    assert tuple(scores["nll"].shape) == (2,) and bool(torch.isfinite(scores["nll"]).all())
    with pytest.raises(IndexError):
        model.to(dev).eval().scores(x, torch.zeros(2, device=dev), torch.tensor([4, 5], device=dev))  # the un-grown checkpoint cannot
