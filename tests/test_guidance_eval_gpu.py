"""Guidance-model evaluation on the device: `vqvs_xent_score` against a numpy evaluation of the rank rule (counts: equal) and
float64 torch (NLL sums) over a shape grid that crosses a 64-lane wave, a tile edge in L, K below one wave and the L = 1 path; its
determinism and independence of the batch layout; a NaN target logit; `Classifier.scores` / `EncoderPredictor.scores` end to end
against the reference's fixtures F9, F15 and F10 in the fp32 mode; `Diffusion.sample_q_seeded`; and the two scripts as child
processes, on one rank and on two.

The NLL bound: both sides are float64 sums of at most K terms with a few-ulp exp, so a position may differ by
(2K + 16) * 2^-53 * max(1, |nll|), and a clip by the sum of that over its positions.

Measured on MI355X (profiles/guidance_eval_margins.jsonl): NLL vs float64 over the grid at most 13 % of the bound (largest error
4.7e-10, one ulp of a +-1e4 clip's sum of about 2e6); fixtures in fp32: NLL vs float64 of the device's logits at most 4.5e-16, vs the fixture's logits 1.8e-7
(bound 4.2e-7, F9) ... 2.9e-5 (bound 3.5e-3, F10); no position of the 134 left out of the top-1 comparison."""
import json
import os
import re
from functools import lru_cache

import numpy as np
import pytest
import torch

from vq_voice_swap_amd import VQVAE, Classifier, Diffusion, EncoderPredictor, _native, classification_scores, create_data_loader, make_schedule, randn_clips
from vq_voice_swap_amd.det_init import det_init_

from util import run_script, sample_lines, seeded

pytestmark = pytest.mark.gpu

GRID = [(K, L) for K in (1, 2, 7, 96, 251, 512, 8192) for L in (1, 37, 64, 250) if (K, L) != (8192, 250)]
BATCHES = (1, 3)
U = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def record(name, value, bound):
    rec = {"test": name, "err": float(value), "bound": float(bound), "fraction_of_bound": float(value / bound) if bound else 0.0}
    print(f"[margin] {name}: err {value:.3e} (bound {bound:.3e})")
    path = os.environ.get("VQVS_GUIDANCE_EVAL_MARGINS")  # a .jsonl file to append to (profiles/guidance_eval_margins.jsonl is such a run)
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def score_call(logits, targets, *, top1=True, k=None, confusion=None):
    """The C entry point on [B, K, L] logits and [B, L] targets; outputs start as NaN / -1 so that an unwritten one shows."""
    B, K, L = logits.shape
    nll = torch.full((B,), float("nan"), device=logits.device, dtype=torch.float64)
    t1 = torch.full((B,), -1, device=logits.device, dtype=torch.int64) if top1 else None
    tk = torch.full((B,), -1, device=logits.device, dtype=torch.int64) if k is not None else None
    _native.check(_native.lib().vqvs_xent_score(logits.data_ptr(), targets.data_ptr(), nll.data_ptr(), _native._ptr(t1), _native._ptr(tk),
                                                int(k or 0), _native._ptr(confusion), B, K, L, _native._stream_ptr()))
    return nll, t1, tk


def reference(logits: np.ndarray, targets: np.ndarray):
    """The rank rule, the first-index argmax and the float64 NLL with its bound, per position, on the CPU from the same logits."""
    B, K, L = logits.shape
    xy = np.take_along_axis(logits, targets[:, None, :], axis=1)  # [B, 1, L]
    below = np.arange(K)[None, :, None] < targets[:, None, :]
    rank = (logits > xy).sum(1) + ((logits == xy) & below).sum(1)
    rank = np.where(np.isnan(xy[:, 0]), K, rank)
    argmax = np.where(np.isnan(logits), -np.inf, logits).argmax(1)  # numpy's argmax is the first index of the maximum
    lt = torch.from_numpy(logits).double()
    nll = -torch.log_softmax(lt, dim=1).gather(1, torch.from_numpy(targets)[:, None]).squeeze(1).numpy()
    bound = (2 * K + 16) * U * np.maximum(1.0, np.abs(nll))
    return rank, argmax, nll, bound


def confusion_of(targets, argmax, K):
    """[K, K] counts of (target, argmax) pairs, both taken from the CPU reference; the K * K bins themselves are filled on the device
    (at K = 8192 they are 512 MiB)."""
    pairs = torch.from_numpy(targets.reshape(-1).astype(np.int64) * K + argmax.reshape(-1).astype(np.int64)).to("cuda:0")
    return torch.bincount(pairs, minlength=K * K).reshape(K, K)


@lru_cache(maxsize=None)
def case(B, K, L):
    """Inputs of one grid point (shared, never modified) with their CPU reference.  Seeded logits scaled so that several classes
    compete; planted where there is room: position 0 an exact tie of the maximum at an index BELOW the target, position 1 one at
    an index ABOVE it, position 2 a target that is the unique maximum (positions count along L, then along clips); with three
    clips, the middle one holds only +-1e4, where a naive exp overflows (its planted position keeps its plant at that scale)."""
    logits = (2.0 * seeded((B, K, L), 3000 + 7 * K + L)).numpy().copy()
    targets = torch.randint(0, K, (B, L), generator=torch.Generator().manual_seed(4000 + K + L)).numpy()
    if B == 3:
        logits[1] = np.where(logits[1] > 0, np.float32(1e4), np.float32(-1e4))
    planted = {}
    flat = [(p // L, p % L) for p in range(B * L)] if L < 3 else [(0, 0), (0, 1), (0, 2)]
    big = np.float32(3e4)
    if K >= 2 and len(flat) > 0:
        b, l = flat[0]
        targets[b, l] = K - 1
        logits[b, 0, l] = logits[b, K - 1, l] = big
        planted["tie_below"] = (b, l)
    if K >= 2 and len(flat) > 1:
        b, l = flat[1]
        targets[b, l] = 0
        logits[b, 0, l] = logits[b, K - 1, l] = big
        planted["tie_above"] = (b, l)
    if len(flat) > 2:
        b, l = flat[2]
        targets[b, l] = K // 2
        logits[b, K // 2, l] = big
        planted["unique"] = (b, l)
    ref = reference(logits, targets)
    dev = torch.device("cuda:0")
    return torch.from_numpy(logits).to(dev), torch.from_numpy(targets).to(dev), logits, targets, ref, planted


# ---------------------------------------------------------------- the kernel over the grid
@pytest.mark.parametrize("K,L", GRID)
def test_counts_equal_the_rank_rule(dev, K, L):
    for B in BATCHES:
        lg, tg, logits, targets, (rank, argmax, _, _), planted = case(B, K, L)
        # the plants did what they are there for
        if "tie_below" in planted:
            assert rank[planted["tie_below"]] == 1 and argmax[planted["tie_below"]] == 0
        if "tie_above" in planted:
            assert rank[planted["tie_above"]] == 0 and argmax[planted["tie_above"]] == 0
        if "unique" in planted:
            assert rank[planted["unique"]] == 0 and argmax[planted["unique"]] == K // 2
        conf0 = (torch.arange(K * K, device=dev, dtype=torch.int64).reshape(K, K) * 5 + 1) % 7  # a non-zero start
        conf = conf0.clone()
        tops = {}
        for k in sorted({1, min(5, K), K}):
            _, t1, tk = score_call(lg, tg, k=k, confusion=conf if k == 1 else None)
            assert np.array_equal(t1.cpu().numpy(), (rank == 0).sum(1)), (B, K, L)
            assert np.array_equal(tk.cpu().numpy(), (rank < k).sum(1)), (B, K, L, k)
            tops[k] = tk
        assert torch.equal(tops[1], t1)                         # k = 1 is top-1
        assert (tops[K] == L).all()                             # k = K is every position: no NaN here
        assert torch.equal(conf - conf0, confusion_of(targets, argmax, K))
        # NULL outputs: accepted, and the others do not change
        nll, none1, nonek = score_call(lg, tg, top1=False)
        assert none1 is None and nonek is None and torch.equal(nll, score_call(lg, tg, k=1)[0])


@pytest.mark.parametrize("K,L", GRID)
def test_nll_vs_float64(dev, K, L):
    worst = 0.0
    for B in BATCHES:
        lg, tg, _, _, (_, _, nll, bound), _ = case(B, K, L)
        got = score_call(lg, tg)[0].cpu().numpy()
        assert got.dtype == np.float64 and np.isfinite(got).all()
        err, clip_bound = np.abs(got - nll.sum(1)), bound.sum(1)
        b = int(np.argmax(err / clip_bound))
        worst = max(worst, float(err[b] / clip_bound[b]))
        record(f"nll K={K} L={L} B={B} vs float64 (clip nearest its bound)", err[b], clip_bound[b])
        assert (err <= clip_bound).all(), (B, K, L, err, clip_bound)
        if K == 1:
            assert (got == 0.0).all()  # one class: log(1) - 0
    assert worst <= 1.0


SUBSET = [(1, 1), (7, 1), (251, 1), (512, 1), (8192, 1), (2, 37), (96, 37), (251, 64), (512, 250), (8192, 64)]


@pytest.mark.parametrize("K,L", SUBSET)
def test_determinism_and_layout_independence(dev, K, L):
    lg, tg, _, targets, (_, argmax, _, _), _ = case(3, K, L)
    k = min(5, K)
    first = score_call(lg, tg, k=k)
    again = score_call(lg, tg, k=k)
    assert all(torch.equal(a, b) for a, b in zip(first, again))  # bitwise, run to run
    # clip 2 alone, at row 0 of a batch of three, and at row 2
    alone = score_call(lg[2:3].contiguous(), tg[2:3].contiguous(), k=k)
    front = score_call(torch.cat([lg[2:3], lg[0:2]]).contiguous(), torch.cat([tg[2:3], tg[0:2]]).contiguous(), k=k)
    for out, row in ((alone, 0), (front, 0), (first, 2)):
        assert all(torch.equal(out[i][row], first[i][2]) for i in range(3)), (K, L, row)
    # confusion accumulated over two calls is the sum of the two calls made separately
    a, b, both = (torch.zeros(K, K, device=dev, dtype=torch.int64) for _ in range(3))
    score_call(lg[:2].contiguous(), tg[:2].contiguous(), confusion=a)
    score_call(lg[2:].contiguous(), tg[2:].contiguous(), confusion=b)
    score_call(lg[:2].contiguous(), tg[:2].contiguous(), confusion=both)
    score_call(lg[2:].contiguous(), tg[2:].contiguous(), confusion=both)
    assert torch.equal(both, a + b) and int(both.sum()) == 3 * L
    assert torch.equal(both, confusion_of(targets, argmax, K))


@pytest.mark.parametrize("K,L", [(251, 1), (96, 37), (512, 250)])
def test_nan_target_logit(dev, K, L):
    lg, tg, logits, targets, (rank, _, _, _), _ = case(3, K, L)
    clean = score_call(lg, tg, k=K)
    l = L - 1
    y = int(targets[2, l])
    bad = lg.clone()
    bad[2, y, l] = float("nan")
    conf = torch.zeros(K, K, device=dev, dtype=torch.int64)
    nll, t1, tk = score_call(bad, tg, k=K, confusion=conf)
    assert torch.isnan(nll[2]) and torch.equal(nll[:2], clean[0][:2])  # that clip, and no other
    hit = int(rank[2, l] == 0)
    assert torch.equal(t1[:2], clean[1][:2]) and int(t1[2]) == int(clean[1][2]) - hit  # the position counts as incorrect
    assert torch.equal(tk[:2], clean[2][:2]) and int(tk[2]) == L - 1                   # rank K: outside even the top K
    ref = reference(bad.cpu().numpy(), targets)
    assert ref[0][2, l] == K and torch.equal(conf, confusion_of(targets, ref[1], K))


def test_wrapper_surface_and_range_check(dev):
    lg, tg, _, targets, (rank, argmax, nll, _), _ = case(3, 96, 37)
    conf = torch.zeros(96, 96, device=dev, dtype=torch.int64)
    out = classification_scores(lg, tg, topk=5, confusion=conf)
    raw = score_call(lg, tg, k=5)
    assert set(out) == {"nll", "top1", "topk", "positions"} and out["positions"] == 37
    assert torch.equal(out["nll"], raw[0]) and torch.equal(out["top1"], raw[1]) and torch.equal(out["topk"], raw[2])
    assert torch.equal(conf, confusion_of(targets, argmax, 96))
    assert classification_scores(lg, tg)["topk"] is None
    # [B, K] logits with [B] targets are the L = 1 case
    flat = classification_scores(lg[:, :, 0].contiguous(), tg[:, 0].contiguous(), topk=5)
    one = score_call(lg[:, :, :1].contiguous(), tg[:, :1].contiguous(), k=5)
    assert flat["positions"] == 1 and all(torch.equal(flat[n], one[i]) for i, n in enumerate(("nll", "top1", "topk")))
    # targets outside 0..K-1 never reach the kernel
    for value in (96, -1):
        wrong = tg.clone()
        wrong[1, 5] = value
        before = conf.clone()
        with pytest.raises(IndexError):
            classification_scores(lg, wrong, topk=5, confusion=conf)
        assert torch.equal(conf, before)
    for a, b in ((lg, tg.cpu()), (lg.cpu(), tg), (lg.cpu(), tg.cpu())):  # no CPU path, for either argument
        with pytest.raises(_native.NativeError):
            classification_scores(a, b)


# ---------------------------------------------------------------- end to end (fixtures F9, F15, F10), fp32 mode
def det_model(m, prefix=""):
    det_init_((prefix + k, v) for k, v in m.state_dict().items())
    m.eval()
    return m


def fixture_models(golden):
    """(name, model, x, ts, targets, reference logits) built as tests/test_classifier.py and tests/test_encoder_predictor.py do."""
    z = golden("f9_classifier32")
    yield ("F9 classifier32", det_model(Classifier(num_labels=7, base_channels=32)), seeded((2, 1, 64000), int(z["x_seed"])),
           torch.from_numpy(z["ts"]), torch.from_numpy(z["labels"]), z["logits"])
    z = golden("f15_custom_classifiers")
    for tag, kw in (("c_a", dict(channel_mult=(1, 2, 2, 4), output_mult=8, depth_mult=1)),
                    ("c_b", dict(channel_mult=(1, 1, 2, 2, 2, 4), output_mult=4, depth_mult=3))):
        yield (f"F15 {tag}", det_model(Classifier(num_labels=5, base_channels=32, **kw), "clf." + tag + "."), torch.from_numpy(z[tag + ".x"]),
               torch.from_numpy(z[tag + ".ts"]), torch.from_numpy(z[tag + ".labels"]), z[tag + ".logits"])
    z = golden("f10_encpred32")
    yield ("F10 encpred32", det_model(EncoderPredictor(base_channels=32, downsample_rate=256, num_latents=96, bottleneck_dim=64)),
           seeded((2, 1, 16384), int(z["x_seed"])), torch.from_numpy(z["ts"]), torch.from_numpy(z["targets"]), z["logits"])


def test_scores_vs_reference_fixtures(golden, dev):
    from test_guidance_eval import top_two_gap

    for name, model, x, ts, targets, ref_logits in fixture_models(golden):
        model.to(dev).set_precision("fp32")
        x, ts = x.to(dev), ts.to(dev)
        logits_dev = model(x, ts).cpu().numpy()
        as3 = (lambda a: a[:, :, None]) if ref_logits.ndim == 2 else (lambda a: a)
        K, L = ref_logits.shape[1], as3(ref_logits).shape[2]
        eps = float(np.abs(logits_dev - ref_logits).max())  # (gated by the existing tests of the forward)
        gap = top_two_gap(ref_logits).reshape(len(x), L)
        assert (gap < 2e-3).mean() < 0.05  # from the fixture alone: the cap holds with room for a logit error of 1e-3
        sure = gap > 2 * eps
        left_out = 1.0 - sure.mean()
        print(f"{name}: max |logits_dev - logits_ref| = {eps:.3e}; {int((~sure).sum())} of {sure.size} positions ({100 * left_out:.2f} %) have a "
              f"top-two gap within twice that and are left out of the top-1 comparison")
        assert left_out < 0.05, (name, left_out)
        # two sets of targets: the fixture's, and the reference's own prediction (so that hits exist to be compared)
        for what, tg in (("fixture targets", targets.numpy()), ("reference argmax as targets", as3(ref_logits).argmax(1).reshape(targets.shape))):
            tg3 = tg.reshape(len(x), L)
            conf = torch.zeros(K, K, device=dev, dtype=torch.int64)
            out = model.scores(x, ts, torch.from_numpy(tg).to(dev), topk=min(5, K), confusion=conf)
            assert out["positions"] == L and int(conf.sum()) == len(x) * L
            got_nll, got_top1 = out["nll"].cpu().numpy(), out["top1"].cpu().numpy()
            # the device's own logits, evaluated in float64 on the CPU: the bound of the grid test, and equal counts
            rank, argmax, nll, bound = reference(as3(logits_dev), tg3)
            err = np.abs(got_nll - nll.sum(1))
            record(f"{name}, {what}: nll vs float64 of the device's logits (worst clip)", err.max(), bound.sum(1)[err.argmax()])
            assert (err <= bound.sum(1)).all(), (name, err, bound.sum(1))
            assert np.array_equal(got_top1, (rank == 0).sum(1)) and np.array_equal(out["topk"].cpu().numpy(), (rank < min(5, K)).sum(1))
            assert torch.equal(conf, confusion_of(tg3, argmax, K))
            # the fixture's logits: NLL is 2-Lipschitz in the max-norm of the logits
            ref_rank, _, ref_nll, _ = reference(as3(ref_logits), tg3)
            err = np.abs(got_nll - ref_nll.sum(1))
            record(f"{name}, {what}: nll vs the fixture's logits (worst clip)", err.max(), 2 * eps * L)
            assert (err <= 2 * eps * L).all(), (name, err, 2 * eps * L)
            # hits: those of the fixture on every position whose gap clears the logit error; the others may go either way
            sure_hits = ((ref_rank == 0) & sure).sum(1)
            assert (sure_hits <= got_top1).all() and (got_top1 <= sure_hits + (~sure).sum(1)).all(), (name, what, got_top1, sure_hits)
            if what.startswith("reference"):
                assert sure_hits.sum() == sure.sum() > 0
        if isinstance(model, EncoderPredictor):  # `losses` is the per-position mean of the same numbers
            mean = model.losses(x, ts, targets.to(dev)).cpu().double().numpy()
            got = model.scores(x, ts, targets.to(dev))["nll"].cpu().numpy() / L
            assert np.abs(mean - got).max() <= 2.0 ** -20 * np.abs(got).max()  # (`losses` is float32: a few of its ulps)


# ---------------------------------------------------------------- sample_q_seeded
@pytest.mark.parametrize("T", [512, 514])
def test_sample_q_seeded(dev, T):
    B, seed, off = 3, 99, 40
    d = Diffusion(make_schedule("exp"))
    x0 = seeded((B, 1, T), 61).to(dev)
    ts = torch.tensor([0.1, 0.45, 0.8])
    got = d.sample_q_seeded(x0, ts, seed=seed, clip_offset=off)
    assert got.shape == x0.shape and got.dtype == torch.float32
    # eps read back through vqvs_ddpm_noise with the same keys: x_0 = 0 and alpha_bar = 0 leave the noise itself
    lib, eps = _native.lib(), torch.empty_like(x0)
    zeros, alpha0 = torch.zeros_like(x0), torch.zeros(B, device=dev)
    _native.check(lib.vqvs_ddpm_noise(zeros.data_ptr(), B, alpha0.data_ptr(), None, 0, None, eps.data_ptr(), B, T, seed, off, _native._stream_ptr()))
    assert torch.equal(eps, randn_clips(B, T, dev, seed=seed, clip_offset=off, stream_id=2))
    # the same kernel on the read-back noise: bitwise
    alpha = d.schedule(ts).to(dev)
    given = torch.empty_like(x0)
    _native.check(lib.vqvs_ddpm_noise(x0.data_ptr(), B, alpha.data_ptr(), eps.data_ptr(), B, None, given.data_ptr(), B, T, 0, 0, _native._stream_ptr()))
    assert torch.equal(got, given)
    # sqrt(a) x0 + sqrt(1 - a) eps in float64.  In f32: a square root within one ulp (2^-23), a product and a sum of half an ulp
    # (2^-24) each, so at most 2^-22 of |p| + |q| to first order; the bound is the next power of two
    a = alpha.double().reshape(-1, 1, 1)
    p, q = a.sqrt() * x0.double(), (1 - a).sqrt() * eps.double()
    assert ((got.double() - (p + q)).abs() <= 2.0 ** -21 * (p.abs() + q.abs())).all()
    # a clip noised in a batch of 1 and in a batch of 3 at the same global index is bitwise equal
    for b in range(B):
        alone = d.sample_q_seeded(x0[b:b + 1], ts[b:b + 1], seed=seed, clip_offset=off + b)
        assert torch.equal(alone[0], got[b])
    assert not torch.equal(d.sample_q_seeded(x0, ts, seed=seed + 1, clip_offset=off), got)
    with pytest.raises(ValueError):
        d.sample_q_seeded(x0, ts[:2], seed=seed)


# ---------------------------------------------------------------- the scripts
LINE = re.compile(r"^(\d+) samples:((?: nll_q[0-3]=\d+\.\d{6})+)((?: acc_q[0-3]=\d+\.\d{6})+)((?: top(\d+)_q[0-3]=\d+\.\d{6})+) nll=(\d+\.\d{6}) acc=(\d+\.\d{6})$")


def check_lines(lines, positions_per_clip, topk):
    assert len(lines) == 2
    for n, ln in zip((2, 4), lines):
        m = LINE.match(ln)
        assert m, ln
        assert int(m.group(1)) == n and int(m.group(5)) == topk
        hits = float(m.group(7)) * n * positions_per_clip  # acc * positions is a count
        assert abs(hits - round(hits)) <= 1e-6 * n * positions_per_clip and 0 <= round(hits) <= n * positions_per_clip


def in_process(model, diffusion, num_classes, targets_of, dev, confusion=True):
    import eval_classifier

    loader, _ = create_data_loader("tones", batch_size=2, seed=1)
    state = eval_classifier.EvalState(num_classes, dev, 5, confusion=confusion)
    for i, batch in zip(range(2), loader):
        audio = batch["samples"][:, None].to(dev)
        state.add_batch(model, diffusion, audio, targets_of(audio, batch), 2 * i, 1)
    return state, eval_classifier.format_line(state.num_samples, state.log_dict())


def test_eval_classifier_script(tmp_path, dev):
    model = det_model(Classifier(num_labels=3, base_channels=32))
    ckpt, conf_path = tmp_path / "clf32.pt", tmp_path / "confusion.npy"
    model.save(str(ckpt))
    args = [str(ckpt), "tones", "--batch-size", "2", "--seed", "1", "--max-samples", "4"]
    lines = sample_lines(run_script("eval_classifier.py", args + ["--confusion-path", str(conf_path)]))
    check_lines(lines, 1, 3)
    state, line = in_process(model.to(dev), Diffusion(make_schedule("exp")), 3, lambda audio, batch: batch["label"].to(dev), dev)
    assert lines[-1] == line
    conf = np.load(conf_path)
    assert conf.shape == (3, 3) and conf.dtype == np.int64 and conf.sum() == 4 and np.array_equal(conf, state.confusion.cpu().numpy())
    assert int(np.trace(conf)) == state.correct
    two = sample_lines(run_script("eval_classifier.py", args, ranks=2))
    assert two == lines[-1:]  # one merged line, the one a single rank ends with
    # a fixed t: every clip falls into one quartile
    import eval_classifier

    fixed = eval_classifier.EvalState(3, dev, 5)
    loader, _ = create_data_loader("tones", batch_size=2, seed=1)
    batch = next(iter(loader))
    fixed.add_batch(model, Diffusion(make_schedule("exp")), batch["samples"][:, None].to(dev), batch["label"].to(dev), 0, 1, t=0.0)
    assert list(fixed.log_dict()) == ["nll_q0", "acc_q0", "top3_q0", "nll", "acc"] and fixed.num_samples == 2


def test_eval_enc_pred_script(tmp_path, dev):
    vq_vae = det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=3))
    model = det_model(EncoderPredictor(base_channels=32, downsample_rate=256, num_latents=512), "enc_pred.")
    vq_path, ckpt = tmp_path / "vqvae32.pt", tmp_path / "enc_pred32.pt"
    vq_vae.save(str(vq_path))
    model.save(str(ckpt))
    args = ["--vq-vae-path", str(vq_path), str(ckpt), "tones", "--batch-size", "2", "--seed", "1", "--max-samples", "4"]
    lines = sample_lines(run_script("eval_enc_pred.py", args))
    check_lines(lines, 250, 5)
    vq_vae.to(dev)
    state, line = in_process(model.to(dev), vq_vae.diffusion, 512, lambda audio, batch: vq_vae.encode(audio), dev, confusion=False)
    assert lines[-1] == line and state.positions == 1000
    assert sample_lines(run_script("eval_enc_pred.py", args, ranks=2)) == lines[-1:]
