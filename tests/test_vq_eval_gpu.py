"""VQ-VAE evaluation on the device: `vqvs_vq_quantize` against `vqvs_vq_argmin` (bitwise), `dict[idx]` (bitwise), float64 torch
and `torch.bincount` over a shape grid that crosses the kernel's tile edges (32 positions, 128 codes, 64 channels); its
determinism; `VQVAE.losses` end to end against fixture F17 (written by tools/gen_vq_eval_golden.py from the reference); the
generated-noise path; sharding of an evaluation pass; and eval_vqvae.py as a child process.

Measured on MI355X (profiles/vq_eval_margins.jsonl): sq_err vs float64 at most 2.8e-8 over the grid (bound 2.4e-7); F17 in fp32:
all 256 codes equal (7 positions sit below the margin threshold), sq_err per clip at most 1.4e-6 (bounds ~3.0e-4), vq_loss
4.3e-7 (3.0e-4), mses per clip at most 2.4e-7 (bounds ~5.6e-5)."""
import json
import os
import re
from functools import lru_cache

import numpy as np
import pytest
import torch

from vq_voice_swap_amd import VQVAE, StandardVQLoss, _native, code_usage, create_data_loader
from vq_voice_swap_amd.det_init import det_init_

from util import run_script, sample_lines, seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO = 1e-4  # the project's per-forward relative-RMS bound of the fp32 mode (tests/test_parity_gpu.py: FP32_REL)
T16 = 16384
# one f32 subtraction and one f32 square per term: at most 3 * 2^-24 relative error on every (non-negative) term, so on their
# sum; the f64 sum adds nothing visible; one unit of slack
SQERR_REL = 4 * 2.0 ** -24
GRID = [(Cd, T1, K) for Cd in (32, 68, 512) for T1 in (1, 37, 64) for K in (1, 130, 512)]
BATCHES = (1, 3)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def f17(golden):
    return golden("f17_vqvae_losses")


def record(name, value, bound):
    rec = {"test": name, "rel_err": float(value), "bound": float(bound), "fraction_of_bound": float(value / bound)}
    print(f"[margin] {name}: rel err {value:.3e} (bound {bound:.3e})")
    path = os.environ.get("VQVS_VQ_EVAL_MARGINS")  # a .jsonl file to append to (profiles/vq_eval_margins.jsonl is such a run)
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def loss_bound(r, rho=RHO):
    """|loss - ref| / ref <= 2 rho r + (rho r)^2 for a sum of squares |d|^2 whose one side moves by |delta| <= rho |v|, r = |v| / |d|
    (the rule of tests/test_losses_gpu.py; here also with v = z, d = z - e)."""
    return 2 * rho * r + (rho * r) ** 2


def argmin_call(z, d):
    B, Cd, T1 = z.shape
    idx = torch.full((B, T1), -1, device=z.device, dtype=torch.int64)
    _native.check(_native.lib().vqvs_vq_argmin(z.data_ptr(), d.data_ptr(), idx.data_ptr(), B, Cd, T1, d.shape[0], _native._stream_ptr()))
    return idx


def quantize_call(z, d, *, embedded=True, sq_err=True, hist=None):
    B, Cd, T1 = z.shape
    idx = torch.full((B, T1), -1, device=z.device, dtype=torch.int64)
    emb = torch.full_like(z, float("nan")) if embedded else None
    sq = torch.full((B,), float("nan"), device=z.device, dtype=torch.float64) if sq_err else None
    _native.check(_native.lib().vqvs_vq_quantize(z.data_ptr(), d.data_ptr(), idx.data_ptr(), _native._ptr(emb), _native._ptr(sq),
                                                 _native._ptr(hist), B, Cd, T1, d.shape[0], _native._stream_ptr()))
    return idx, emb, sq


@lru_cache(maxsize=None)
def case(B, Cd, T1, K):
    """Inputs of one grid point (shared, never modified): random z and dictionary; where there is room, dictionary row 5 is a
    copy of row 2 (the lower index has to win) and, in clips of more than one position, column 0 IS row 2 (an exact hit)."""
    dev = torch.device("cuda:0")
    z = seeded((B, Cd, T1), 1000 + Cd + T1).to(dev)
    d = seeded((K, Cd), 2000 + Cd + K).to(dev)
    if K > 5:
        d[5] = d[2]
        if T1 > 1:
            z[:, :, 0] = d[2]
    hist0 = (torch.arange(K, device=dev, dtype=torch.int64) * 7 + 3) % 11  # a non-zero start
    hist = hist0.clone()
    idx, emb, sq = quantize_call(z, d, hist=hist)
    torch.cuda.synchronize()
    return z, d, idx, emb, sq, hist0, hist


# ---------------------------------------------------------------- the kernel over the grid
@pytest.mark.parametrize("Cd,T1,K", GRID)
def test_idx_is_bitwise_vq_argmin(dev, Cd, T1, K):
    for B in BATCHES:
        z, d, idx, _, _, _, _ = case(B, Cd, T1, K)
        assert torch.equal(idx, argmin_call(z, d))
        assert int(idx.min()) >= 0 and int(idx.max()) < K
        if K > 5:
            assert not (idx == 5).any()  # duplicated row: the first index wins
            assert T1 == 1 or (idx[:, 0] == 2).all()  # exact hit


@pytest.mark.parametrize("Cd,T1,K", GRID)
def test_embedded_is_an_exact_copy_and_optional(dev, Cd, T1, K):
    for B in BATCHES:
        z, d, idx, emb, sq, _, _ = case(B, Cd, T1, K)
        assert torch.equal(emb, d[idx].permute(0, 2, 1).contiguous())
        # NULL outputs: accepted, and the others do not change
        hist = torch.zeros(K, device=dev, dtype=torch.int64)
        idx2, none, sq2 = quantize_call(z, d, embedded=False, hist=hist)
        assert none is None and torch.equal(idx2, idx) and torch.equal(sq2, sq)
        assert torch.equal(hist, torch.bincount(idx.reshape(-1), minlength=K))
        idx3, emb3, none = quantize_call(z, d, sq_err=False)
        assert none is None and torch.equal(idx3, idx) and torch.equal(emb3, emb)
        idx4, _, _ = quantize_call(z, d, embedded=False, sq_err=False)
        assert torch.equal(idx4, idx)


@pytest.mark.parametrize("Cd,T1,K", GRID)
def test_sq_err_vs_float64(dev, Cd, T1, K):
    worst = 0.0
    for B in BATCHES:
        z, d, idx, emb, sq, _, _ = case(B, Cd, T1, K)
        want = ((z.double() - d[idx].permute(0, 2, 1).double()) ** 2).flatten(1).sum(1)
        assert sq.dtype == torch.float64 and (want > 0).all()
        err = ((sq - want).abs() / want).max().item()
        worst = max(worst, err)
        assert err <= SQERR_REL, (B, Cd, T1, K, err)
    record(f"sq_err Cd={Cd} T1={T1} K={K} vs float64", worst, SQERR_REL)


@pytest.mark.parametrize("Cd,T1,K", [(32, 37, 130), (68, 64, 512), (512, 37, 130)])
def test_sq_err_of_dictionary_rows_is_exactly_zero(dev, Cd, T1, K):
    d = seeded((K, Cd), 31).to(dev)
    pick = (torch.arange(3 * T1, device=dev) * 37 % K).reshape(3, T1)
    z = d[pick].permute(0, 2, 1).contiguous()
    z[1] = seeded((Cd, T1), 32).to(dev)  # clip 1 is ordinary: only clips 0 and 2 are made of dictionary rows
    idx, emb, sq = quantize_call(z, d)
    assert torch.equal(idx[0], pick[0]) and torch.equal(idx[2], pick[2])
    assert sq[0].item() == 0.0 and sq[2].item() == 0.0 and sq[1].item() > 0.0


@pytest.mark.parametrize("Cd,T1,K", GRID)
def test_hist_accumulates(dev, Cd, T1, K):
    for B in BATCHES:
        z, d, idx, _, _, hist0, hist = case(B, Cd, T1, K)
        counts = torch.bincount(idx.reshape(-1), minlength=K)
        assert hist0.any() and torch.equal(hist, hist0 + counts)
        again = hist.clone()
        quantize_call(z, d, embedded=False, sq_err=False, hist=again)
        assert torch.equal(again, hist0 + 2 * counts)  # two calls accumulate
        assert int(counts.sum()) == B * T1


@pytest.mark.parametrize("Cd,T1,K", [(32, 1, 1), (68, 37, 130), (512, 64, 512), (512, 37, 130)])
def test_determinism_and_row_independence(dev, Cd, T1, K):
    z, d, idx, emb, sq, _, _ = case(3, Cd, T1, K)
    idx2, emb2, sq2 = quantize_call(z, d)
    assert torch.equal(idx, idx2) and torch.equal(emb, emb2) and torch.equal(sq, sq2)
    alone = quantize_call(z[2:3].contiguous(), d)
    assert torch.equal(alone[0], idx[2:3]) and torch.equal(alone[1], emb[2:3]) and torch.equal(alone[2], sq[2:3])


def test_vq_module_surface(dev):
    from vq_voice_swap_amd import VQ

    vq = VQ(68, 130).eval().to(dev)
    x = seeded((3, 68, 5, 7), 41).to(dev)  # any trailing shape
    hist = torch.zeros(130, device=dev, dtype=torch.int64)
    q = vq.quantize(x, hist=hist)
    fwd = vq(x)
    assert q["idxs"].shape == (3, 5, 7) and torch.equal(q["idxs"], fwd["idxs"]) and torch.equal(q["idxs"], vq.encode(x))
    assert torch.equal(q["embedded"], fwd["embedded"]) and q["sq_err"].shape == (3,) and q["sq_err"].dtype == torch.float64
    assert torch.equal(hist, torch.bincount(q["idxs"].reshape(-1), minlength=130))
    assert vq.quantize(x, embedded=False)["embedded"] is None
    loss = StandardVQLoss()
    direct, fused = loss(x, q["embedded"], vq.dictionary).item(), loss.from_sq_err(q["sq_err"], x.numel()).item()
    assert abs(direct - fused) <= 1e-6 * fused
    for bad in (torch.zeros(130, device=dev, dtype=torch.int32), torch.zeros(129, device=dev, dtype=torch.int64)):
        with pytest.raises(ValueError):
            vq.quantize(x, hist=bad)


# ---------------------------------------------------------------- end to end (fixture F17)
def det_model(m):
    det_init_(m.state_dict().items())
    m.eval()
    return m


@lru_cache(maxsize=None)
def f17_model(num_labels=5):
    f = np.load(os.path.join(ROOT, "tests", "golden", "f17_vqvae_losses.npz"))
    model = det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=num_labels, dictionary_size=130))
    with torch.no_grad():
        model.vq.dictionary.copy_(torch.from_numpy(f["dictionary"]))
    model.set_precision("fp32")
    return model.to(torch.device("cuda:0"))


def test_losses_vs_reference(f17, dev):
    model = f17_model()
    x = (float(f17["x_scale"]) * seeded((4, 1, T16), int(f17["x_seed"]))).to(dev)
    noise = seeded((4, 1, T16), int(f17["noise_seed"])).to(dev)
    labels, ts = torch.from_numpy(f17["labels"]).to(dev), torch.from_numpy(f17["ts"])
    hist = torch.zeros(130, device=dev, dtype=torch.int64)
    out = model.losses(StandardVQLoss(), x, labels, ts=ts, noise=noise, hist=hist)
    assert set(out) >= {"vq_loss", "mse", "ts", "mses", "idxs", "sq_err"}
    assert torch.equal(out["ts"].cpu(), ts)  # returned unchanged
    # codes: equal wherever the reference's own margin clears the fixture's threshold
    sure = torch.from_numpy(f17["margin"] > float(f17["margin_threshold"]))
    assert sure.float().mean().item() >= 0.95
    got_idx, ref_idx = out["idxs"].cpu(), torch.from_numpy(f17["idxs"])
    assert got_idx.shape == ref_idx.shape and torch.equal(got_idx[sure], ref_idx[sure])
    print(f"codes: {int((got_idx != ref_idx).sum())} of {ref_idx.numel()} differ, {int((~sure).sum())} positions are below the margin threshold")
    # histogram: the fixture's, up to the excluded positions
    assert int(hist.sum()) == ref_idx.numel() and torch.equal(hist.cpu(), torch.bincount(got_idx.reshape(-1), minlength=130))
    assert torch.equal(torch.bincount(got_idx[sure], minlength=130), torch.bincount(ref_idx[sure], minlength=130))
    assert (hist.cpu() - torch.from_numpy(f17["hist"])).abs().sum().item() <= 2 * int((~sure).sum())
    # quantisation error per clip and the loss, within the bound of an encoder output that moved by rho
    sq, want_sq = out["sq_err"].cpu().numpy(), f17["sq_err"]
    err, bound = np.abs(sq - want_sq) / want_sq, loss_bound(f17["r_vq"])
    for b in range(4):
        record(f"F17 sq_err fp32 clip {b}", err[b], bound[b])
    assert (err <= bound).all(), (err, bound)
    vq_err = abs(float(out["vq_loss"]) - float(f17["vq_loss"])) / float(f17["vq_loss"])
    record("F17 vq_loss fp32", vq_err, bound.max() + 2.0 ** -22)  # (+ the reference's own float32 mean)
    assert vq_err <= bound.max() + 2.0 ** -22
    assert float(out["vq_loss"]) == pytest.approx(1.25 * sq.sum() / int(f17["z_numel"]), rel=1e-14)
    # noise-prediction loss per clip
    got, want = out["mses"].cpu().double().numpy(), f17["mses"].astype(np.float64)
    err, bound = np.abs(got - want) / want, loss_bound(f17["r"])
    for b in range(4):
        record(f"F17 mses fp32 clip {b} (t = {f17['ts'][b]:.2f})", err[b], bound[b])
    assert (err <= bound).all(), (err, bound)
    assert float(out["mse"]) == pytest.approx(got.mean(), rel=1e-6)
    u = code_usage(hist)
    assert u["used_codes"] >= 16 and 1.0 <= u["perplexity"] <= u["used_codes"]


def test_generated_noise_path_is_denoising_losses(f17, dev):
    model = f17_model()
    x = (0.3 * seeded((3, 1, T16), 51)).to(dev)
    labels, ts = torch.tensor([1, 4, 0], device=dev), torch.tensor([0.2, 0.5, 0.8])
    out = model.losses(StandardVQLoss(), x, labels, ts=ts, seed=77, clip_offset=5)
    direct = model.diffusion.denoising_losses(x, model.predictor, ts, seed=77, clip_offset=5, cond=out["embedded"], labels=labels)
    assert torch.equal(out["mses"], direct)
    assert torch.equal(out["embedded"], model.vq.embed(out["idxs"])) and torch.equal(out["idxs"], model.encode(x))
    # ts = None: the seeded draw of denoising_losses
    auto = model.losses(StandardVQLoss(), x, labels, seed=77, clip_offset=5)
    assert torch.equal(auto["ts"].cpu(), model.diffusion.draw_ts(3, 77, 5))
    with pytest.raises(RuntimeError):
        model.train().losses(StandardVQLoss(), x, labels)
    model.eval()


# ---------------------------------------------------------------- an evaluation pass, whole and sharded
def test_sharded_pass_equals_one_pass(dev):
    import eval_vqvae

    model = f17_model(3)  # tones: three speakers
    loader, num_labels = create_data_loader("tones", batch_size=2, seed=1)
    assert num_labels == 3
    batches = [b for _, b in zip(range(6), loader)]
    assert len(batches) == 6

    def run(indices):
        state = eval_vqvae.EvalState(130, dev)
        for i in indices:
            state.add_batch(model, batches[i]["samples"][:, None].to(dev), batches[i]["label"].to(dev), 2 * i, 1)
        return state

    one = run(range(6))
    merged = run(range(0, 6, 2)).to_host().merge(run(range(1, 6, 2)).to_host())
    assert merged.num_samples == one.num_samples == 12 and merged.numel == one.numel
    assert torch.equal(merged.hist, one.hist.cpu()) and int(one.hist.sum()) == 12 * 250
    assert merged.sq_err == one.sq_err and float(one.sq_err) > 0  # exact sums: no order in them
    a, b = one.log_dict(), merged.log_dict()
    assert list(a) == list(b) and any(k.startswith("rand_q") for k in a)
    for k in a:
        assert abs(a[k] - b[k]) <= 1e-12 * abs(a[k]), (k, a[k], b[k])


# ---------------------------------------------------------------- the script
LINE = re.compile(r"^(\d+) samples:((?: cond_q[0-3]=\d+\.\d{6})+)((?: rand_q[0-3]=\d+\.\d{6})+) vq_loss=(\d+\.\d{6}) used_codes=(\d+) perplexity=(\d+\.\d{6})$")


def test_eval_vqvae_script(tmp_path, dev):
    model = det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=3))
    ckpt = tmp_path / "vqvae32.pt"
    model.save(str(ckpt))
    args = [ckpt, "tones", "--batch-size", "4", "--seed", "1", "--max-samples", "8"]
    lines = sample_lines(run_script("eval_vqvae.py", args))
    assert len(lines) == 2
    for n, ln in zip((4, 8), lines):
        m = LINE.match(ln)
        assert m, ln
        assert int(m.group(1)) == n
        used, perplexity = int(m.group(5)), float(m.group(6))
        assert 1 <= used <= model.vq.num_codes and 1.0 <= perplexity <= used
    # the same pass, driven directly
    import eval_vqvae

    model.to(dev).set_precision("fp32")
    state = eval_vqvae.EvalState(model.vq.num_codes, dev)
    loader, _ = create_data_loader("tones", batch_size=4, seed=1)
    for i, batch in zip(range(2), loader):
        state.add_batch(model, batch["samples"][:, None].to(dev), batch["label"].to(dev), 4 * i, 1)
    assert lines[-1] == eval_vqvae.format_line(state.num_samples, state.log_dict())
    assert sample_lines(run_script("eval_vqvae.py", args, ranks=2)) == lines[-1:]  # one merged line, the one a single rank ends with
