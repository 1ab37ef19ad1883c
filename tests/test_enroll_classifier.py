"""Classifier enrolment, host side (none of this needs a device): the numpy reference of tests/enroll_head_ref.py against float64
autograd + torch.optim.AdamW and against the closed form, what a replay batch and an unreached row do, `Classifier.add_labels`, the
host logic of `ClassifierEnroller` with the native calls stubbed, the declaration, export and refusals of the two entry points,
enroll_classifier.py's command line, label offset, batch layout, hold-out and curriculum, and that the gate of the GPU file follows
from the recorded run."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import enroll_head_ref as H
import enroll_ref
import vq_voice_swap_amd.enroll as enroll
from util import flags_of
from vq_voice_swap_amd import Classifier, _native
from vq_voice_swap_amd.det_init import det_init_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(8)
TINY = dict(base_channels=32, channel_mult=(1, 2), output_mult=2, depth_mult=1)  # F = 64


def _batch(B=8, K=5, n=2, F=64, seed=31, targets=None):
    """(act, w_old, b_old, rows0, targets): random features through the float64 GELU, a random head, rows from N(0, 1 / F)."""
    g = torch.Generator().manual_seed(seed)
    act = H.gelu64(torch.randn(B, F, generator=g).numpy()).astype(np.float32)
    w_old = (torch.randn(K, F, generator=g) / np.sqrt(F)).numpy()
    b_old = (0.1 * torch.randn(K, generator=g)).numpy()
    rows0 = (torch.randn(n, F + 1, generator=g) / np.sqrt(F)).numpy()
    if targets is None:
        targets = [K + (b % n) if b % 4 else b % K for b in range(B)]  # one clip in four is a replay clip
    return act, w_old, b_old, rows0, np.asarray(targets, dtype=np.int64)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_numpy_reference_is_autograd_and_torch_adamw(wd):
    """5 steps: rows, loss and gradient of the numpy restatement against float64 autograd + torch.optim.AdamW on a grown nn.Linear."""
    act, w_old, b_old, rows0, y = _batch()
    auto = H.AutogradHead(w_old, b_old, rows0, lr=1e-2, weight_decay=wd)
    rows, m, v = rows0.astype(np.float64), np.zeros(rows0.shape), np.zeros(rows0.shape)
    for step in range(1, 6):
        loss, grad = auto.step(act, y)
        rows, m, v, r = H.step_ref(act, w_old, b_old, rows, m, v, y, step, 1e-2, weight_decay=wd)
        assert abs(r["nll"].mean() - loss) < 1e-12 and np.abs(H.grad_ref(act, r["coef"]) - grad).max() < 1e-13, step
        assert np.abs(rows - auto.rows()).max() < 1e-12, step
    assert np.abs(rows - rows0).max() > 1e-2  # five steps of lr 1e-2 moved them


def test_reference_is_the_closed_form():
    """d nll_b / d W[K + j, :] = (softmax_b[K + j] - [y_b = K + j]) gelu(feat_b), one clip at a time, against autograd; head_ref in
    extended precision agrees with its float64 self."""
    act, w_old, b_old, rows0, y = _batch()
    K, n = 5, 2
    r = H.head_ref(act, w_old, b_old, rows0, y)
    rx = H.head_ref(act, w_old, b_old, rows0, y, dtype=H.XL)
    assert np.finfo(H.XL).eps <= 2.0 ** -63, "the bound test needs a long double wider than float64"
    for name in ("logits", "nll", "new_mass", "coef"):
        assert np.abs(r[name] - rx[name].astype(np.float64)).max() < 1e-13, name
    assert (r["top1"] == rx["top1"]).all()
    W = torch.tensor(np.concatenate([w_old, rows0[:, :-1]]), dtype=torch.float64, requires_grad=True)
    b = torch.tensor(np.concatenate([b_old, rows0[:, -1]]), dtype=torch.float64, requires_grad=True)
    a = torch.tensor(act, dtype=torch.float64)
    for i in range(len(y)):
        logp = torch.log_softmax(a[i] @ W.t() + b, dim=-1)
        gW, gb = torch.autograd.grad(-logp[y[i]], [W, b])
        p = logp.exp().detach().numpy()
        coef = p[K:] - (np.arange(K, K + n) == y[i])
        assert np.abs(r["coef"][i] - coef).max() < 1e-14 and abs(r["nll"][i] + logp[y[i]].item()) < 1e-13
        assert np.abs(gW[K:].numpy() - coef[:, None] * act[i][None, :].astype(np.float64)).max() < 1e-14
        assert np.abs(gb[K:].numpy() - coef).max() < 1e-14
        assert abs(r["new_mass"][i] - p[K:].sum()) < 1e-14 and r["top1"][i] == int(p.argmax() == y[i])
    # a single float32 rounding of the stored logits, and the bound's terms are what they claim
    E_logit, E_nll, E_coef, E_mass = H.bounds(rx, 64, K, n)
    assert E_logit.shape == (8, 7) and (E_logit >= 8 * H.U * np.abs(r["logits"])).all()  # D = min(64, 1 + 6) = 7
    assert (E_nll > 2 * E_logit.max(axis=1)).all() and (E_coef < E_nll).all() and (E_mass > E_coef).all()


def test_a_replay_batch_only_lowers_the_new_logits():
    act, w_old, b_old, rows0, y = _batch(targets=[b % 5 for b in range(8)])  # every clip an old speaker
    r = H.head_ref(act, w_old, b_old, rows0, y)
    assert (r["coef"] > 0).all() and np.abs(r["coef"].sum(axis=1) - r["new_mass"]).max() < 1e-15  # coef = softmax[K + j]: no indicator
    g = H.grad_ref(act, r["coef"])
    assert (g[:, -1] > 0).all()  # the biases go down
    for i in range(8):  # a clip alone: the step -eta g lowers each of its new logits by eta c (|act|^2 + 1)
        gi = H.grad_ref(act[i:i + 1], r["coef"][i:i + 1])
        assert ((gi[:, :-1] @ act[i].astype(np.float64) + gi[:, -1]) > 0).all()
    rows, _m, _v, _ = H.step_ref(act, w_old, b_old, rows0, np.zeros(rows0.shape), np.zeros(rows0.shape), y, 1, 1e-3)
    after = H.head_ref(act, w_old, b_old, rows.astype(np.float32), y)
    assert after["nll"].mean() < r["nll"].mean() and after["new_mass"].mean() < r["new_mass"].mean()
    assert (after["logits"][:, :5] == r["logits"][:, :5]).all()  # the old logits do not move


def test_a_row_nothing_reaches_is_unchanged():
    """Row 1 of the new rows has a bias of -1e4, so its softmax is exactly 0, and no clip names it: its coef column, its gradient and
    its moments are exactly 0 and at weight decay 0 the row keeps its bits; with weight decay it shrinks."""
    act, w_old, b_old, rows0, y = _batch(targets=[5 if b % 2 else b % 5 for b in range(8)])
    rows0 = rows0.astype(np.float32)
    rows0[1, -1] = -1e4
    zeros = np.zeros(rows0.shape)
    rows, m, v, r = H.step_ref(act, w_old, b_old, rows0, zeros, zeros, y, 1, 1e-2)
    assert (r["coef"][:, 1] == 0).all() and (rows[1] == rows0[1]).all() and not m[1].any() and not v[1].any()
    assert not (rows[0] == rows0[0]).any()
    rows, _, _, _ = H.step_ref(act, w_old, b_old, rows0, zeros, zeros, y, 1, 1e-2, weight_decay=0.01)
    assert np.abs(rows[1] - rows0[1].astype(np.float64) * (1 - 1e-4)).max() < 1e-12 * 1e4 and (rows[1, :-1] != rows0[1, :-1]).all()


def test_reference_loss_falls_over_twenty_steps():
    """B 8, K 5, n 2, F 64, lr 1e-2: the condition the GPU test relies on, for the reference alone."""
    act, w_old, b_old, rows0, y = _batch()
    _, losses = H.trajectory_ref(act, w_old, b_old, rows0, y, 21, 1e-2)
    assert losses[20] < losses[0] and all(b < a for a, b in zip(losses, losses[1:])), losses


def test_cases_are_what_they_claim():
    assert [s[1] + s[2] for s in H.XENT_SHAPES] == [2, 7, 256, 256, 257, 255, 8192]
    for shape in H.XENT_SHAPES[:-1]:
        B, K, n, F = shape
        for kind in H.KINDS:
            c = H.make_case(shape, kind)
            r = H.head_ref(H.gelu64(c["feat"].numpy()).astype(np.float32), c["w_old"], c["b_old"], c["rows"], c["targets"])
            lo, hi = c["tie"]
            assert lo < hi and r["logits"][0, lo] == r["logits"][0, hi] == r["logits"][0].max() and r["top1"][0] == 1
            assert c["targets"].min() >= 0 and c["targets"].max() < K + n
            if B > 1:
                assert r["top1"][1] == 0 and c["targets"][1] == hi  # the later copy of the maximum is not the first index
            if B > 3:
                assert (c["targets"][2:] < K).any() and (c["targets"][2:] >= K).any()
            if kind == "saturated":
                assert 79.9 < np.abs(r["logits"]).max() < 80.1


# ---- Classifier.add_labels ---------------------------------------------------------------------------------------------------------
def _classifier(num_labels=4):
    clf = Classifier(num_labels, **TINY)
    det_init_(("enrc.host." + k, v) for k, v in clf.state_dict().items())
    return clf.eval()


def test_add_labels_keeps_the_old_rows_bitwise(tmp_path):
    clf = _classifier()
    old_w, old_b = clf.out[1].weight.detach().clone(), clf.out[1].bias.detach().clone()
    others = {k: v.clone() for k, v in clf.state_dict().items() if not k.startswith("out.1.")}
    assert old_w.abs().sum() > 0
    clf.add_labels(3)
    w, b = clf.out[1].weight.detach(), clf.out[1].bias.detach()
    assert clf.num_labels == 7 and tuple(w.shape) == (7, 64) and tuple(b.shape) == (7,) and clf.save_kwargs()["num_labels"] == 7
    assert torch.equal(w[:4], old_w) and torch.equal(b[:4], old_b) and not w[4:].any() and not b[4:].any()
    assert all(torch.equal(clf.state_dict()[k], v) for k, v in others.items())
    assert clf._cfg().num_labels == 7 and clf._handle is None
    path = str(tmp_path / "grown.pt")
    clf.save(path)
    back = Classifier.load(path)
    assert back.num_labels == 7 and back.save_kwargs() == clf.save_kwargs()
    assert all(torch.equal(back.state_dict()[k], v) for k, v in clf.state_dict().items())
    for bad in (0, -1, 1.5, 8192):
        with pytest.raises(ValueError):
            clf.add_labels(bad)


# ---- ClassifierEnroller with the native calls stubbed -------------------------------------------------------------------------------
class _StubLib:
    """Stands in for libvqvs_hip.so behind vq_voice_swap_amd.enroll: records the calls, touches nothing."""

    def __init__(self):
        self.calls = []

    def vqvs_ddpm_noise(self, *a):
        self.calls.append(("noise", a))
        return 0

    def vqvs_head_xent_grad(self, *a):
        self.calls.append(("xent", a))
        return 0

    def vqvs_head_adamw(self, *a):
        self.calls.append(("adamw", a))
        return 0


@pytest.fixture
def stubbed(monkeypatch):
    lib = _StubLib()
    monkeypatch.setattr(_native, "lib", lambda: lib)
    monkeypatch.setattr(_native, "require_cuda", lambda *t: None)
    monkeypatch.setattr(_native, "_stream_ptr", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    monkeypatch.setattr(enroll, "randn_clips", lambda n, T, device, seed, clip_offset=0, stream_id=1: torch.zeros(n, 1, T))
    return lib


def test_init_modes():
    clf = _classifier()
    w, b = clf.out[1].weight.detach(), clf.out[1].bias.detach()
    z = enroll.ClassifierEnroller(clf, 3).rows
    assert tuple(z.shape) == (3, 65) and z.dtype == torch.float32 and not z.any()  # "zeros" is the default: a fresh head
    mean = enroll.ClassifierEnroller(clf, 2, init="mean").rows
    assert torch.equal(mean[0], mean[1])
    assert torch.equal(mean[0, :-1], w.double().mean(dim=0).float()) and mean[0, -1] == b.double().mean().float()
    row = enroll.ClassifierEnroller(clf, 2, init=2).rows
    assert torch.equal(row[0, :-1], w[2]) and row[0, -1] == b[2] and torch.equal(row[0], row[1])
    for bad in ("normal", 4, -1, True, 1.0):
        with pytest.raises((ValueError, IndexError)):
            enroll.ClassifierEnroller(clf, 2, init=bad)
    with pytest.raises(ValueError):
        enroll.ClassifierEnroller(torch.nn.Linear(2, 2), 1)
    with pytest.raises(RuntimeError):
        enroll.ClassifierEnroller(_classifier().train(), 1)
    for bad in (0, 1.5, 8190):
        with pytest.raises(ValueError):
            enroll.ClassifierEnroller(clf, bad)
    with pytest.raises(ValueError):
        enroll.ClassifierEnroller(clf, 1, schedule_name="no such schedule")


def test_step_calls_and_resume_round_trip(stubbed, monkeypatch):
    clf = _classifier()
    seen = {}

    def features(x_t, ts):
        seen.update(x_t=tuple(x_t.shape), ts=ts.clone())
        return torch.ones(len(x_t), 64)

    monkeypatch.setattr(clf, "features", features)
    en = enroll.ClassifierEnroller(clf, 3, lr=1e-3, weight_decay=0.5, init="mean")
    x = torch.zeros(2, 1, 256)
    out = en.step(x, torch.tensor([6, 1]), ts=torch.tensor([0.25, 0.75]), seed=4)  # a new speaker and a replay clip
    assert sorted(out) == ["acc", "loss", "new_mass", "nlls", "ts"] and out["ts"].tolist() == [0.25, 0.75] and tuple(out["nlls"].shape) == (2,)
    assert seen["x_t"] == (2, 1, 256) and seen["ts"].tolist() == [0.25, 0.75] and en.steps == 1
    assert [k for k, _ in stubbed.calls] == ["noise", "xent", "adamw"]
    assert stubbed.calls[1][1][11:15] == (2, 64, 4, 3)  # B, F, K, n
    adamw = stubbed.calls[2][1]
    assert adamw[0] == en.rows.data_ptr() and adamw[5:9] == (3, 2, 64, 1) and adamw[9:14] == (1e-3, 0.9, 0.999, 1e-8, 0.5)
    assert clf.num_labels == 4  # the classifier is untouched
    with pytest.raises(IndexError):
        en.step(x, torch.tensor([7, 0]), ts=torch.tensor([0.25, 0.75]))
    with pytest.raises(IndexError):
        en.step(x, torch.tensor([-1, 0]), ts=torch.tensor([0.25, 0.75]))
    with pytest.raises(ValueError):
        en.step(x, torch.tensor([0]), ts=torch.tensor([0.25, 0.75]))
    # resume: rows, moments and the step count survive a round trip through a fresh enroller
    en.rows += 0.125
    en.exp_avg += 0.5
    en.exp_avg_sq += 0.25
    state = en.state_dict()
    fresh = enroll.ClassifierEnroller(clf, 3)
    assert not torch.equal(fresh.rows, en.rows)
    fresh.load_state_dict(state)
    assert torch.equal(fresh.rows, en.rows) and torch.equal(fresh.exp_avg, en.exp_avg) and torch.equal(fresh.exp_avg_sq, en.exp_avg_sq)
    assert fresh.steps == 1 and fresh.first_label == 4
    fresh.step(x, torch.tensor([4, 5]), ts=torch.tensor([0.5, 0.5]))
    assert stubbed.calls[-1][1][8] == 2  # the next step is step 2
    with pytest.raises(ValueError):
        enroll.ClassifierEnroller(clf, 2).load_state_dict(state)
    with pytest.raises(ValueError):
        enroll.ClassifierEnroller(_classifier(5), 3).load_state_dict(state)


def test_finish_and_checkpoint_agree_and_leave_the_old_rows_bitwise():
    clf = _classifier()
    old = {k: v.clone() for k, v in clf.state_dict().items()}
    en = enroll.ClassifierEnroller(clf, 2, init=1)
    en.rows += torch.randn(2, 65, generator=torch.Generator().manual_seed(3))
    ck = en.checkpoint()
    assert clf.num_labels == 4 and ck["kwargs"]["num_labels"] == 6  # the classifier itself is untouched until finish()
    loaded = Classifier.load_dict(ck)
    w, b = loaded.out[1].weight.detach(), loaded.out[1].bias.detach()
    assert loaded.num_labels == 6 and torch.equal(w[:4], old["out.1.weight"]) and torch.equal(b[:4], old["out.1.bias"])
    assert torch.equal(w[4:], en.rows[:, :-1]) and torch.equal(b[4:], en.rows[:, -1])
    out = en.finish()
    assert out is clf and clf.num_labels == 6 and clf.save_kwargs()["num_labels"] == 6
    assert all(torch.equal(clf.state_dict()[k], v) for k, v in loaded.state_dict().items())  # checkpoint() is finish() + save_dict()
    assert all(torch.equal(clf.state_dict()[k], v) for k, v in old.items() if not k.startswith("out.1."))
    assert all(torch.equal(en.checkpoint()["state_dict"][k], v) for k, v in clf.state_dict().items())
    with pytest.raises(RuntimeError):
        en.finish()
    with pytest.raises(RuntimeError):
        en.losses(torch.zeros(1, 1, 256), torch.tensor([0]))


# ---- the entry points ----------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(lib_built):
    header = " ".join(open(os.path.join(ROOT, "include", "vqvs.h")).read().split())
    for name, nargs in (("vqvs_head_xent_grad", 16), ("vqvs_head_adamw", 15)):
        assert name in _native.EXPORTS and hasattr(lib_built, name)
        decl = re.search(r"int " + name + r"\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == nargs == len(getattr(lib_built, name).argtypes), name
    args = [a.strip() for a in re.search(r"int vqvs_head_xent_grad\(([^;]*)\);", header).group(1).split(",")]
    assert args == ["const float* d_feat", "const float* d_w_old", "const float* d_b_old", "const float* d_new", "const int64_t* d_targets",
                    "float* d_act", "float* d_logits", "double* d_nll", "int64_t* d_top1", "double* d_new_mass", "double* d_coef", "int B", "int F",
                    "int K", "int n", "void* stream"]
    args = [a.strip() for a in re.search(r"int vqvs_head_adamw\(([^;]*)\);", header).group(1).split(",")]
    assert args == ["float* d_new", "float* d_m", "float* d_v", "const float* d_act", "const double* d_coef", "int n", "int B", "int F", "int step",
                    "float lr", "float beta1", "float beta2", "float eps", "float weight_decay", "void* stream"]


def test_entry_points_refuse_bad_arguments_without_a_device(lib_built):
    L = lib_built
    buf = C.cast((C.c_double * 64)(), C.c_void_p)
    ok = dict(feat=buf, w_old=buf, b_old=buf, new=buf, targets=buf, act=None, logits=None, nll=buf, top1=None, new_mass=None, coef=buf,
              B=2, F=4, K=3, n=2)

    def xent(**kw):
        a = dict(ok, **kw)
        return L.vqvs_head_xent_grad(a["feat"], a["w_old"], a["b_old"], a["new"], a["targets"], a["act"], a["logits"], a["nll"], a["top1"],
                                     a["new_mass"], a["coef"], a["B"], a["F"], a["K"], a["n"], None)

    for bad in (dict(feat=None), dict(w_old=None), dict(b_old=None), dict(new=None), dict(targets=None), dict(nll=None), dict(coef=None),
                dict(B=0), dict(B=65536), dict(F=0), dict(F=4097), dict(K=0), dict(n=0), dict(K=8192, n=1), dict(K=1, n=8192), dict(K=-1, n=5),
                dict(K=2 ** 31 - 1, n=2)):
        assert xent(**bad) == -1 and L.vqvs_last_error(), bad
    ok2 = dict(new=buf, m=buf, v=buf, act=buf, coef=buf, n=2, B=3, F=8, step=1, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.0)

    def adamw(**kw):
        a = dict(ok2, **kw)
        return L.vqvs_head_adamw(a["new"], a["m"], a["v"], a["act"], a["coef"], a["n"], a["B"], a["F"], a["step"], a["lr"], a["b1"], a["b2"],
                                 a["eps"], a["wd"], None)

    for bad in (dict(new=None), dict(m=None), dict(v=None), dict(act=None), dict(coef=None), dict(n=0), dict(B=0), dict(F=-1), dict(step=0),
                dict(n=8193), dict(B=65536), dict(F=4097), dict(lr=-1.0), dict(lr=float("nan")), dict(eps=-1e-8), dict(wd=-0.1), dict(b1=1.0),
                dict(b2=-0.1), dict(b2=float("inf"))):
        assert adamw(**bad) == -1 and L.vqvs_last_error(), bad


# ---- enroll_classifier.py ------------------------------------------------------------------------------------------------------------
def test_command_line_label_offset_and_curriculum():
    import enroll_classifier as script
    import enroll_speaker

    p = script.arg_parser()
    assert flags_of(p) == sorted(["--lr", "--weight-decay", "--batch-size", "--output-dir", "--pretrained-path", "--save-interval", "--encoding",
                                  "--schedule", "--curriculum-start", "--curriculum-steps", "--steps", "--init", "--seed", "--holdout", "--seconds",
                                  "--precision", "--replay-dir", "--replay-batch", "data_dir"])
    a = p.parse_args(["speakers", "--pretrained-path", "clf.pt"])
    assert (a.lr, a.weight_decay, a.batch_size, a.output_dir, a.encoding, a.schedule) == (1e-4, 0.0, 8, "ckpt_classifier_added", "linear", "exp")
    assert (a.curriculum_start, a.curriculum_steps, a.init, a.replay_dir, a.replay_batch, a.precision) == (30.0, 0, "zeros", None, None, "fp32")
    with pytest.raises(SystemExit):
        p.parse_args(["speakers"])  # --pretrained-path is required
    assert script.parse_init("zeros") == "zeros" and script.parse_init("mean") == "mean" and script.parse_init("7") == 7
    for name in ("split_holdout", "epoch_batches", "load_clips", "model_labels", "local_device"):
        assert getattr(script, name) is getattr(enroll_speaker, name), name  # imported, not copied
    # the reference's sample_timesteps (train_loop.py:563-569): power = start * (1 - frac) + frac while total_steps < curriculum_steps
    assert script.curriculum_power(0, 30.0, 0) == 1.0 and script.curriculum_power(0, 30.0, 100) == 30.0
    assert script.curriculum_power(50, 30.0, 100) == 15.5 and script.curriculum_power(99, 30.0, 100) == 30.0 * (1 - 99 / 100) + 99 / 100
    assert script.curriculum_power(100, 30.0, 100) == 1.0 and script.curriculum_power(10 ** 6, 30.0, 100) == 1.0
    from vq_voice_swap_amd import Diffusion

    assert torch.equal(script.batch_ts(4, 3, 8, 1.0), Diffusion.draw_ts(4, 3, 8))
    assert torch.equal(script.batch_ts(4, 3, 8, 15.5), Diffusion.draw_ts(4, 3, 8) ** 15.5)
    # new clips first, offset by the old count (train_loop.py:450); replay clips behind them under their own labels
    audio, labels = script.compose_batch(torch.zeros(3, 1, 8), torch.tensor([0, 1, 0]), 251, torch.ones(2, 1, 8), torch.tensor([7, 250]))
    assert labels.tolist() == [251, 252, 251, 7, 250] and labels.dtype == torch.int64
    assert not audio[:3].any() and bool((audio[3:] == 1).all())
    assert script.compose_batch(torch.zeros(3, 1, 8), torch.tensor([0, 1, 0]), 251)[1].tolist() == [251, 252, 251]
    with pytest.raises(ValueError):
        script.compose_batch(torch.zeros(3, 1, 8), torch.tensor([0, 1, 0]), 251, torch.ones(2, 1, 16), torch.tensor([7, 250]))


class _FakeEnroller:
    """Stands in for ClassifierEnroller behind enroll_classifier.main: counts steps, remembers what it was shown."""
    seen = []

    def __init__(self, model, num_new, **kw):
        self.steps, self.first_label, self.num_new, self.kw = 0, model.num_labels, num_new, kw

    def step(self, audio, labels, *, ts, seed, clip_offset):
        self.steps += 1
        n = len(audio)
        _FakeEnroller.seen.append(dict(labels=labels.tolist(), ts=ts.clone(), clip_offset=clip_offset, n=n))
        return {"loss": torch.tensor(1.0), "nlls": torch.ones(n), "acc": torch.tensor(0.5), "ts": torch.full((n,), 0.5)}

    def losses(self, audio, labels, *, ts, seed, clip_offset):
        n = len(audio)
        return {"nll": torch.ones(n), "top1": torch.ones(n, dtype=torch.int64), "new_mass": torch.full((n,), 0.25)}

    def checkpoint(self):
        return {}

    def state_dict(self):
        return {"steps": self.steps}

    def load_state_dict(self, state):
        self.steps = state["steps"]


@pytest.fixture
def fake_script(monkeypatch):
    """enroll_classifier with everything native stubbed; returns (script, shown): `shown` lists (dataset kind, indices) of every load."""
    import enroll_classifier as script

    shown = []
    real_load = script.load_clips

    def load_clips(dataset, indices, device):
        shown.append(list(indices))
        return torch.zeros(len(indices), 1, 8), real_load(dataset, indices[:1], device)[1].repeat(len(indices))

    fake_model = types.SimpleNamespace(num_labels=3, check_status=lambda: None)
    fake_model.to = lambda d: fake_model
    fake_model.eval = lambda: fake_model
    fake_model.set_precision = lambda p: fake_model
    saved = {}
    del _FakeEnroller.seen[:]
    monkeypatch.setattr(script, "load_clips", load_clips)
    monkeypatch.setattr(script, "Classifier", types.SimpleNamespace(load=lambda p: fake_model))
    monkeypatch.setattr(script, "ClassifierEnroller", _FakeEnroller)
    monkeypatch.setattr(script, "local_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(script, "atomic_save", lambda state, path: saved.__setitem__(os.path.basename(path), dict(state)))
    monkeypatch.setattr(script.torch, "load", lambda path, map_location=None: saved["enroll.pt"])
    return script, shown, fake_model


def test_held_out_clips_never_reach_a_step(fake_script, tmp_path, capsys):
    """enroll_classifier.main on the synthetic set (30 clips): over more than two passes, and again in a resumed run, no training batch
    holds a held-out index, and the step numbers go on."""
    script, shown, _ = fake_script
    args = ["tones", "--pretrained-path", "x.pt", "--output-dir", str(tmp_path), "--batch-size", "4", "--holdout", "3", "--seed", "2",
            "--save-interval", "5", "--curriculum-steps", "10"]
    script.main(args + ["--steps", "15"])  # 27 training clips: 6 batches per pass, so 2.5 passes
    held, train = script.split_holdout(30, 3, 2)
    assert shown[0] == held and len(shown) == 16
    walked = shown[1:]
    assert all(len(b) == 4 and not set(b) & set(held) for b in walked)
    assert walked[:6] == script.epoch_batches(train, 4, 2, 0) and walked[6:12] == script.epoch_batches(train, 4, 2, 1)
    seen = _FakeEnroller.seen
    assert all(min(s["labels"]) >= 3 and max(s["labels"]) < 6 for s in seen)  # tones: three new speakers behind three old ones
    assert [s["clip_offset"] for s in seen] == [4 * i for i in range(15)]
    for i, s in enumerate(seen):  # the curriculum counts the steps taken before this one
        assert torch.equal(s["ts"], script.batch_ts(4, 2, 4 * i, script.curriculum_power(i, 30.0, 10))), i
    out = capsys.readouterr().out
    assert [ln.split(":")[0] for ln in out.splitlines() if "loss=" in ln] == [f"step {i}" for i in range(1, 16)]
    assert all(" acc=0.5000 " in ln and " q" in ln for ln in out.splitlines() if "loss=" in ln)
    lines = [ln for ln in out.splitlines() if "holdout_nll=" in ln]
    assert [ln.split(":")[0] for ln in lines] == ["step 5", "step 10", "step 15"]
    assert all("holdout_acc=1.0000" in ln and "replay_new_mass" not in ln and ln.endswith("(3 clips)") for ln in lines)
    # a resumed run: the same held-out clips, and it goes on in the pass and at the batch where the first run stopped
    open(os.path.join(tmp_path, "enroll.pt"), "w").close()
    del shown[:]
    script.main(args + ["--steps", "4"])
    assert shown[0] == held and shown[1:] == (script.epoch_batches(train, 4, 2, 2)[3:] + script.epoch_batches(train, 4, 2, 3))[:4]
    out = capsys.readouterr().out
    assert [ln.split(":")[0] for ln in out.splitlines() if "loss=" in ln] == [f"step {i}" for i in range(16, 20)] and "step 19: holdout_nll=" in out
    with pytest.raises(SystemExit):
        script.main(["tones", "--pretrained-path", "x.pt", "--seconds", "1"])


def test_replay_batches_follow_the_new_clips(fake_script, tmp_path, capsys, monkeypatch):
    """--replay-dir: every batch is --batch-size new clips, then --replay-batch replay clips under old labels; the replay set's own
    held-out clips never train; a replay set with more speakers than the checkpoint has labels is refused; one new speaker alone warns."""
    script, shown, fake_model = fake_script
    args = ["tones", "--pretrained-path", "x.pt", "--output-dir", str(tmp_path), "--batch-size", "4", "--holdout", "3", "--seed", "2",
            "--save-interval", "3", "--replay-dir", "tones", "--replay-batch", "2", "--steps", "3"]
    script.main(args)
    held, train = script.split_holdout(30, 3, 2)
    assert shown[0] == held and shown[1] == held  # the new set's and the replay set's held-out clips, by the same rule
    new_loads, replay_loads = shown[2::2][:3], shown[3::2][:3]
    assert new_loads == script.epoch_batches(train, 4, 2, 0)[:3] and replay_loads == script.epoch_batches(train, 2, 3, 0)[:3]
    assert not set(i for b in replay_loads for i in b) & set(held)
    for s in _FakeEnroller.seen:
        assert s["n"] == 6 and all(lab >= 3 for lab in s["labels"][:4]) and all(lab < 3 for lab in s["labels"][4:]), s
    assert [s["clip_offset"] for s in _FakeEnroller.seen] == [0, 6, 12]
    line = [ln for ln in capsys.readouterr().out.splitlines() if "holdout_nll=" in ln]
    assert len(line) == 1 and "replay_new_mass=2.500000e-01" in line[0] and line[0].endswith("(3 clips)")
    fake_model.num_labels = 2
    with pytest.raises(SystemExit, match="3 speakers, the checkpoint has 2 labels"):
        script.main(args)
    # one new speaker and no replay set: a warning, not an error
    fake_model.num_labels = 3
    real_loader = script.create_data_loader
    monkeypatch.setattr(script, "create_data_loader", lambda **kw: (real_loader(**kw)[0], 1))
    script.main(["tones", "--pretrained-path", "x.pt", "--output-dir", str(tmp_path / "one"), "--steps", "1"])
    assert "nothing in the loss bounds its row" in capsys.readouterr().err


def test_gates_follow_the_recorded_run():
    """profiles/enroll_classifier_margins.jsonl is one whole GPU run of tests/test_enroll_classifier_gpu.py; the three-step gate is
    `enroll_ref.gate_of` of it, every recorded share of the derived bound is below 1 and every AdamW value within one ulp."""
    recs = H.recorded()
    traj = [r for r in recs if r["test"] == "enroll.traj"]
    assert sorted(r["case"] for r in traj) == sorted(H.TRAJ_CASES) and all(r["prec"] == "fp32" for r in traj)
    assert H.GATES["traj"] == enroll_ref.gate_of(recs, "traj") <= enroll_ref.GRAD_GATE_CAP, (H.GATES, enroll_ref.gate_of(recs, "traj"))
    assert all(3 * r["traj_err"] <= H.GATES["traj"] for r in traj)
    assert sorted(r["case"] for r in recs if r["test"] == "enroll_classifier.traj_fp16") == sorted(H.TRAJ_CASES)  # recorded, not gated
    xent = [r for r in recs if r["test"] == "enroll_classifier.xent"]
    assert len(xent) == len(H.XENT_SHAPES) * len(H.KINDS)
    assert all(max(r["share_nll"], r["share_coef"], r["share_new_mass"]) < 1 and r["logits_ulp"] <= 1 and r["act_err"] <= H.ACT_TOL for r in xent)
    adamw = [r for r in recs if r["test"] == "enroll_classifier.adamw"]
    assert len(adamw) == len(H.XENT_SHAPES) * len(H.ADAMW_WD) and all(r["worst_ulp"] <= 1 for r in adamw)
