"""Speaker enrolment, host side (none of this needs a device): the numpy AdamW of tests/enroll_ref.py against torch.optim.AdamW, the
autograd reference's own sanity, the declaration and export of the two entry points, the refusals of VQVS_KIND_PREDICTOR_GRAD, the
host logic of `SpeakerEnroller` with the native calls stubbed, enroll_speaker.py's command line and label offset, and that the gates
of the GPU file follow from the recorded run."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import enroll_ref as R
import vq_voice_swap_amd.enroll as enroll
from util import flags_of
from vq_voice_swap_amd import DiffusionModel, _native
from vq_voice_swap_amd.det_init import det_init_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(8)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_numpy_adamw_is_torch_adamw(wd):
    """5 steps on float64 tensors, three rows of which one is named by two clips, one by one and one by none: 1e-12."""
    g = torch.Generator().manual_seed(5)
    rows0 = torch.randn(3, 16, generator=g, dtype=torch.float64)
    row_of_clip = [0, 1, 0]
    p = torch.nn.Parameter(rows0.clone())
    opt = torch.optim.AdamW([p], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    ref = (rows0.numpy().copy(), np.zeros((3, 16)), np.zeros((3, 16)))
    for step in range(1, 6):
        grads = 1e-3 * torch.randn(3, 16, generator=g, dtype=torch.float64)
        table = torch.zeros(3, 16, dtype=torch.float64)
        table.index_add_(0, torch.tensor(row_of_clip), grads)
        p.grad = table / 3  # losses.mean(): every clip's gradient carries 1 / B
        opt.step()
        ref = R.adamw_ref(*ref, grads.numpy(), row_of_clip, step, 1e-2, (0.9, 0.999), 1e-8, wd)
        assert np.abs(ref[0] - p.detach().numpy()).max() < 1e-12, step
    assert (ref[0][2] == rows0.numpy()[2]).all() == (wd == 0.0)  # the unnamed row moves by weight decay alone


def test_reference_gradient_of_an_unnamed_row_is_zero(lib_built):
    case = R.CASE["pg_ragged"]
    r = R.reference(case)
    named = set(case["labels"])
    for row in range(case["num_labels"]):
        assert bool((r["table_grad"][row] == 0).all()) == (row not in named), row
    # the table's gradient is the per-clip gradients summed per row over the batch mean
    table = torch.zeros_like(r["table_grad"])
    for b, lab in enumerate(case["labels"]):
        table[lab] += r["grads"][b] / case["B"]
    assert R.rel_rms(table[sorted(named)], r["table_grad"][sorted(named)]) < 1e-12
    assert r["dfilm"].shape == (case["B"], sum(2 * cout for _, _, cout in R.film_rows(case)))
    # down_blocks.1, channel 5: 1 + a = 0 exactly, and d a there is an ordinary finite number
    block, c = case["zero_film"]
    m = R.make_model(case)
    lin = dict(m.named_modules())[block].cond_layers[1]
    assert not lin.weight[c].any() and lin.bias[c].item() == -1.0
    row = {n: r0 for n, r0, _ in R.film_rows(case)}[block]
    assert bool(torch.isfinite(r["dfilm"][:, row + c]).all()) and r["dfilm"][:, row + c].abs().min() > 0


def test_cases_are_the_shapes_they_claim(lib_built):
    for cid, (B, T, blocks, E) in {"pg32": (3, 1792, 65, 128), "pg_ragged": (2, 592, 14, 128), "pg96": (2, 592, 14, 384)}.items():
        case = R.CASE[cid]
        x_t, ts, eps, cond, labels = R.inputs(case)
        assert tuple(x_t.shape) == tuple(eps.shape) == (B, 1, T) and tuple(ts.shape) == tuple(labels.shape) == (B,)
        assert len(R.film_rows(case)) == blocks and R.make_model(case).class_embed.weight.shape[1] == E
        assert (cond is None) == (case["cond_channels"] is None)
    assert R.inputs(R.CASE["pg32"])[3].shape[2] == 1792 // 256 and R.inputs(R.CASE["pg96"])[3].shape[2] == 5
    assert len(set(R.CASE["pg32"]["labels"])) == 2  # two clips on one row


def test_entry_points_are_declared_and_exported(lib_built):
    header = " ".join(open(os.path.join(ROOT, "include", "vqvs.h")).read().split())
    for name, nargs in (("vqvs_unet_embed_grad", 12), ("vqvs_embed_adamw", 15), ("vqvs_debug_read_dfilm", 3)):
        assert name in _native.EXPORTS and hasattr(lib_built, name)
        decl = re.search(r"int " + name + r"\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == nargs == len(getattr(lib_built, name).argtypes), name
    assert re.search(r"#define VQVS_KIND_PREDICTOR_GRAD 6\b", header) and _native.KIND_PREDICTOR_GRAD == 6
    args = [a.strip() for a in re.search(r"int vqvs_unet_embed_grad\(([^;]*)\);", header).group(1).split(",")]
    assert args == ["vqvs_model* m", "const float* d_x_t", "const float* d_ts", "const float* d_cond", "const float* d_vec", "const float* d_eps",
                    "float* d_mse", "float* d_grad", "float* d_pred", "int B", "int T", "void* stream"]
    args = [a.strip() for a in re.search(r"int vqvs_embed_adamw\(([^;]*)\);", header).group(1).split(",")]
    assert args == ["float* d_rows", "float* d_m", "float* d_v", "const float* d_grad", "const int64_t* d_row_of_clip", "int n", "int B", "int E",
                    "int step", "float lr", "float beta1", "float beta2", "float eps", "float weight_decay", "void* stream"]


def _grad_cfg(**over):
    cfg = R.make_model(R.CASE["pg_ragged"])._cfg()
    cfg.kind, cfg.precision, cfg.max_batch, cfg.max_T = _native.KIND_PREDICTOR_GRAD, _native.PREC_F32, 2, 592
    for k, v in over.items():
        if k == "reserved4":
            cfg.reserved[4] = v
        else:
            setattr(cfg, k, v)
    return cfg


def test_param_count_refuses_what_the_kind_is_not_built_for(lib_built):
    L = lib_built
    good = _grad_cfg()
    n = L.vqvs_param_count(C.byref(good))
    pred = _grad_cfg(kind=_native.KIND_PREDICTOR)
    assert n > 0 and _native.param_table(good) == _native.param_table(pred)  # the predictor's own parameter table
    for over, field in ((dict(precision=_native.PREC_F16), b"precision"), (dict(precision=_native.PREC_BF16), b"precision"),
                        (dict(reserved4=24), b"reserved[4]"), (dict(num_labels=0), b"num_labels"), (dict(out_channels=32), b"out_channels")):
        assert L.vqvs_param_count(C.byref(_grad_cfg(**over))) == -1, over
        assert field in L.vqvs_last_error(), (over, L.vqvs_last_error())
    with_cond = _grad_cfg(cond_channels=32)
    assert L.vqvs_param_count(C.byref(with_cond)) == n + 2  # cond_proj.weight / .bias: conditional or not


def test_entry_points_refuse_bad_arguments_without_a_device(lib_built):
    L = lib_built
    bufs = [(C.c_float * 64)() for _ in range(4)]
    rows, m, v, grad = (C.cast(b, C.c_void_p) for b in bufs)
    idx = C.cast((C.c_int64 * 4)(), C.c_void_p)
    ok = dict(rows=rows, m=m, v=v, grad=grad, idx=idx, n=2, B=3, E=8, step=1, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_embed_adamw(a["rows"], a["m"], a["v"], a["grad"], a["idx"], a["n"], a["B"], a["E"], a["step"], a["lr"], a["b1"], a["b2"],
                                  a["eps"], a["wd"], None)

    for bad in (dict(rows=None), dict(m=None), dict(v=None), dict(grad=None), dict(idx=None), dict(n=0), dict(B=0), dict(E=-1), dict(step=0),
                dict(lr=-1.0), dict(lr=float("nan")), dict(eps=-1e-8), dict(wd=-0.1), dict(b1=1.0), dict(b2=-0.1), dict(b2=float("inf"))):
        assert call(**bad) == -1 and L.vqvs_last_error(), bad
    assert L.vqvs_unet_embed_grad(None, rows, rows, None, rows, rows, rows, rows, None, 1, 64, None) == -1
    assert L.vqvs_debug_read_dfilm(None, 1, rows) == -1


# ---- SpeakerEnroller with the native calls stubbed -------------------------------------------------------------------------------------
class _StubLib:
    """Stands in for libvqvs_hip.so behind vq_voice_swap_amd.enroll: records the calls, touches nothing."""

    def __init__(self):
        self.calls = []

    def vqvs_ddpm_noise(self, *a):
        self.calls.append(("noise", a))
        return 0

    def vqvs_embed_adamw(self, *a):
        self.calls.append(("adamw", a))
        return 0


@pytest.fixture
def stubbed(monkeypatch, lib_built):
    lib = _StubLib()
    lib.vqvs_pad_blocks = lib_built.vqvs_pad_blocks  # (host arithmetic that constructing a model asks the library for)
    monkeypatch.setattr(_native, "lib", lambda: lib)
    monkeypatch.setattr(_native, "require_cuda", lambda *t: None)
    monkeypatch.setattr(_native, "_stream_ptr", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    monkeypatch.setattr(enroll, "randn_clips", lambda n, T, device, seed, clip_offset=0, stream_id=1: torch.zeros(n, 1, T))
    return lib


def _model(num_labels=4):
    model = DiffusionModel("unet", 32, num_labels=num_labels)
    det_init_(("enr.host." + k, v) for k, v in model.state_dict().items())
    return model.eval()


def test_init_modes(lib_built):
    model = _model()
    old = model.predictor.class_embed.weight.detach().clone()
    a = enroll.SpeakerEnroller(model, 3, init="normal", seed=7).rows
    b = enroll.SpeakerEnroller(model, 3, init="normal", seed=7).rows
    c = enroll.SpeakerEnroller(model, 3, init="normal", seed=8).rows
    assert tuple(a.shape) == (3, 128) and a.dtype == torch.float32 and torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(a, torch.randn(3, 128, generator=torch.Generator().manual_seed(7)))  # N(0, 1), a fresh nn.Embedding's law
    mean = enroll.SpeakerEnroller(model, 2, init="mean").rows
    assert torch.equal(mean[0], mean[1]) and torch.allclose(mean[0], old.mean(dim=0), atol=1e-7)
    row = enroll.SpeakerEnroller(model, 2, init=2).rows
    assert torch.equal(row[0], old[2]) and torch.equal(row[1], old[2])
    for bad in ("zeros", 4, -1, True):
        with pytest.raises((ValueError, IndexError)):
            enroll.SpeakerEnroller(model, 2, init=bad)
    with pytest.raises(ValueError):
        enroll.SpeakerEnroller(DiffusionModel("unet", 32), 1)  # no class embedding
    with pytest.raises(RuntimeError):
        enroll.SpeakerEnroller(_model().train(), 1)
    with pytest.raises(ValueError):
        enroll.SpeakerEnroller(model, 0)


def test_step_calls_and_resume_round_trip(stubbed, monkeypatch):
    model = _model()
    seen = {}

    def embedding_grad(x_t, ts, eps, vectors, *, cond=None, return_pred=False):
        seen.update(vectors=vectors.clone(), ts=ts.clone(), cond=cond)
        return torch.tensor([1.0, 3.0]), torch.ones(2, 128)

    monkeypatch.setattr(model.predictor, "embedding_grad", embedding_grad)
    en = enroll.SpeakerEnroller(model, 3, lr=1e-3, weight_decay=0.5, seed=1)
    x = torch.zeros(2, 1, 256)
    out = en.step(x, torch.tensor([2, 0]), ts=torch.tensor([0.25, 0.75]), seed=4)
    assert out["loss"].item() == 2.0 and out["mses"].tolist() == [1.0, 3.0] and out["ts"].tolist() == [0.25, 0.75]
    assert torch.equal(seen["vectors"], en.rows[[2, 0]]) and seen["cond"] is None and en.steps == 1
    assert [k for k, _ in stubbed.calls] == ["noise", "adamw"]
    adamw = stubbed.calls[1][1]
    assert adamw[5:9] == (3, 2, 128, 1) and adamw[9:14] == (1e-3, 0.9, 0.999, 1e-8, 0.5)  # n, B, E, step; lr, betas, eps, weight decay
    with pytest.raises(IndexError):
        en.step(x, torch.tensor([3, 0]), ts=torch.tensor([0.25, 0.75]))
    with pytest.raises(ValueError):
        en.step(x, torch.tensor([0]), ts=torch.tensor([0.25, 0.75]))
    # resume: rows, moments and the step count survive a round trip through a fresh enroller
    en.exp_avg += 0.5
    en.exp_avg_sq += 0.25
    state = en.state_dict()
    fresh = enroll.SpeakerEnroller(model, 3, seed=99)
    assert not torch.equal(fresh.rows, en.rows)
    fresh.load_state_dict(state)
    assert torch.equal(fresh.rows, en.rows) and torch.equal(fresh.exp_avg, en.exp_avg) and torch.equal(fresh.exp_avg_sq, en.exp_avg_sq)
    assert fresh.steps == 1 and fresh.first_label == 4
    fresh.step(x, torch.tensor([1, 1]), ts=torch.tensor([0.5, 0.5]))
    assert stubbed.calls[-1][1][8] == 2  # the next step is step 2
    with pytest.raises(ValueError):
        enroll.SpeakerEnroller(model, 2).load_state_dict(state)
    with pytest.raises(ValueError):
        enroll.SpeakerEnroller(_model(5), 3).load_state_dict(state)


def test_finish_and_checkpoint_leave_the_old_rows_bitwise(lib_built):
    model = _model()
    old = model.predictor.class_embed.weight.detach().clone()
    others = {k: v.clone() for k, v in model.state_dict().items() if k != "predictor.class_embed.weight"}
    en = enroll.SpeakerEnroller(model, 2, init="normal", seed=3)
    ck = en.checkpoint()
    assert model.num_labels == 4 and ck["kwargs"]["num_labels"] == 6  # the model itself is untouched until finish()
    loaded = DiffusionModel.load_dict(ck)
    w = loaded.predictor.class_embed.weight.detach()
    assert loaded.num_labels == loaded.predictor.num_labels == 6 and torch.equal(w[:4], old) and torch.equal(w[4:], en.rows)
    out = en.finish()
    w = model.predictor.class_embed.weight.detach()
    assert out is model and model.num_labels == model.predictor.num_labels == 6 and model.save_kwargs()["num_labels"] == 6
    assert torch.equal(w[:4], old) and torch.equal(w[4:], en.rows)
    assert all(torch.equal(model.state_dict()[k], v) for k, v in others.items())
    assert all(torch.equal(en.checkpoint()["state_dict"][k], v) for k, v in model.state_dict().items())
    with pytest.raises(RuntimeError):
        en.finish()


def test_enroll_speaker_command_line_and_label_offset():
    import enroll_speaker as script

    p = script.arg_parser()
    assert flags_of(p) == sorted(["--lr", "--weight-decay", "--batch-size", "--output-dir", "--pretrained-path", "--save-interval", "--encoding",
                                  "--steps", "--init", "--seed", "--holdout", "--seconds", "data_dir"])
    a = p.parse_args(["speakers", "--pretrained-path", "model.pt"])
    assert (a.lr, a.weight_decay, a.batch_size, a.output_dir, a.save_interval, a.encoding) == (1e-4, 0.0, 8, "ckpt_vqvae_added", 1000, "linear")
    assert "usage" in p.format_help() and "--holdout N" in p.format_help()
    with pytest.raises(SystemExit):
        p.parse_args(["speakers"])  # --pretrained-path is required: there is nothing to enrol into
    assert script.parse_init("normal") == "normal" and script.parse_init("mean") == "mean" and script.parse_init("7") == 7
    assert script.model_labels(torch.tensor([0, 1, 0]), 251).tolist() == [251, 252, 251]  # train_loop.py:450


def test_holdout_split_and_batches():
    import enroll_speaker as script

    held, train = script.split_holdout(30, 7, seed=5)
    assert len(held) == 7 and len(train) == 23 and sorted(held + train) == list(range(30))
    assert script.split_holdout(30, 7, seed=5) == (held, train) and script.split_holdout(30, 7, seed=6)[0] != held
    assert script.split_holdout(30, 0, seed=5) == ([], list(range(30)))
    with pytest.raises(ValueError):
        script.split_holdout(30, 31, seed=5)
    for epoch in range(3):
        batches = script.epoch_batches(train, 4, 5, epoch)
        flat = [i for b in batches for i in b]
        assert len(batches) == 5 and all(len(b) == 4 for b in batches) and len(set(flat)) == 20
        assert not set(flat) & set(held) and set(flat) <= set(train)
        assert batches == script.epoch_batches(train, 4, 5, epoch)
    assert script.epoch_batches(train, 4, 5, 0) != script.epoch_batches(train, 4, 5, 1)


class _FakeEnroller:
    """Stands in for SpeakerEnroller behind enroll_speaker.main: counts steps, remembers what it was shown."""
    saved = None

    def __init__(self, model, num_new, **kw):
        self.steps, self.first_label, self.num_new = 0, model.num_labels, num_new

    def step(self, audio, rows, *, seed, clip_offset):
        self.steps += 1
        n = len(audio)
        return {"loss": torch.tensor(1.0), "mses": torch.ones(n), "ts": torch.full((n,), 0.5)}

    def losses(self, audio, rows, *, ts, seed, clip_offset):
        return (torch.ones(len(audio)),)

    def checkpoint(self):
        return {}

    def state_dict(self):
        return {"steps": self.steps}

    def load_state_dict(self, state):
        self.steps = state["steps"]


def test_held_out_clips_never_reach_a_step(monkeypatch, tmp_path, capsys):
    """enroll_speaker.main on the synthetic set (30 clips) with everything native stubbed: over more than two passes, and again in a
    resumed run, no training batch holds a held-out index; the holdout line names exactly N clips, N below the batch size."""
    import types

    import enroll_speaker as script

    shown = []
    real_load = script.load_clips

    def load_clips(dataset, indices, device):
        shown.append(list(indices))
        return torch.zeros(len(indices), 1, 8), real_load(dataset, indices[:1], device)[1].repeat(len(indices))

    fake_model = types.SimpleNamespace(num_labels=3, predictor=types.SimpleNamespace(check_status=lambda: None))
    fake_model.to = lambda d: fake_model
    fake_model.eval = lambda: fake_model
    saved = {}
    monkeypatch.setattr(script, "load_clips", load_clips)
    monkeypatch.setattr(script, "VQVAE", types.SimpleNamespace(load=lambda p: fake_model))
    monkeypatch.setattr(script, "SpeakerEnroller", _FakeEnroller)
    monkeypatch.setattr(script, "local_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(script, "atomic_save", lambda state, path: saved.__setitem__(os.path.basename(path), dict(state)))
    monkeypatch.setattr(script.torch, "load", lambda path, map_location=None: saved["enroll.pt"])
    args = ["tones", "--pretrained-path", "x.pt", "--output-dir", str(tmp_path), "--batch-size", "4", "--holdout", "3", "--seed", "2",
            "--save-interval", "5"]
    script.main(args + ["--steps", "15"])  # 27 training clips: 6 batches per pass, so 2.5 passes
    held, train = script.split_holdout(30, 3, 2)
    assert shown[0] == held and len(shown) == 16
    walked = shown[1:]
    assert all(len(b) == 4 and not set(b) & set(held) for b in walked)
    assert walked[:6] == script.epoch_batches(train, 4, 2, 0) and walked[6:12] == script.epoch_batches(train, 4, 2, 1)
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if "holdout=" in ln]
    assert [ln.split(":")[0] for ln in lines] == ["step 5", "step 10", "step 15"] and all(ln.endswith("(3 clips)") for ln in lines)
    # a resumed run: the same held-out clips, and it goes on in the pass and at the batch where the first run stopped
    open(os.path.join(tmp_path, "enroll.pt"), "w").close()
    del shown[:]
    script.main(args + ["--steps", "4"])
    assert shown[0] == held and shown[1:] == (script.epoch_batches(train, 4, 2, 2)[3:] + script.epoch_batches(train, 4, 2, 3))[:4]
    assert "step 19: holdout=" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        script.main(["tones", "--pretrained-path", "x.pt", "--seconds", "1"])


def test_gates_follow_the_recorded_run():
    """profiles/enroll_margins.jsonl is one whole GPU run of tests/test_enroll_gpu.py; every gate is `gate_of` of it and every
    recorded error sits inside its gate with the factor of three to spare."""
    recs = R.recorded()
    count = {t: len([r for r in recs if r["test"] == "enroll." + R.GATE_TEST.get(t, t)]) for t in R.GATES}
    assert count == {"grad": len(R.CASES), "dfilm": len(R.CASES), "dfilm_block": len(R.CASES), "adamw": 4, "traj": 1}, count
    assert {r["case"] for r in recs if r["test"] == "enroll.grad"} == set(R.CASE)
    for test, gate in R.GATES.items():
        assert gate == R.gate_of(recs, test) <= R.GRAD_GATE_CAP, (test, gate, R.gate_of(recs, test))
        for r in recs:
            if r["test"] == "enroll." + R.GATE_TEST.get(test, test):
                assert all(3 * r[f] <= gate for f in R.GATE_FIELDS[test]), r
    assert R.gate_of([dict(test="enroll.grad", grad_err=1e-4, grad_err_worst_clip=1.0001e-4)], "grad") == 4e-4
    assert R.gate_of([dict(test="enroll.grad", grad_err=1e-4, grad_err_worst_clip=1e-4)], "grad") == 3e-4
    assert R.gate_of([dict(test="enroll.traj", traj_err=1e-3)], "traj") == 2e-3
