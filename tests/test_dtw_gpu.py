"""MCD-DTW on the device: `vqvs_mel_cepstra` (rows of different lengths, padded with anything), `vqvs_dtw_distance` against the
float64 restatement of tests/dtw_ref.py, `AlignedDistance`, and eval_parallel.py end to end.

The alignment's bound, per pair: |cost - ref| <= 2 (n_ceps + Fa + Fb + 4) 2^-53 ref (dtw_ref.bound_factor), with steps, both and vuv
exactly the reference's -- legitimate because tests/test_dtw.py shows that on these inputs no cell's two cheapest predecessors lie
within 1000 bounds of each other.  Each case's fraction of its bound is recorded (profiles/dtw_margins.jsonl).

Measured on MI355X: all 13 alignment records are bit-equal to the restatement -- cost, counts and both track sums, fraction of the
bound 0 --; the stored cepstra equal the emulated float64 front end exactly in all ten rows; the MCD formed from the stored cepstra
lies within 0.035 of its bound of `vqvs_spectral_distance`'s sum (0 .. 0.035 over six clips)."""
import os
import sys

import numpy as np
import pytest
import torch

from vq_voice_swap_amd import VQVAE, AlignedDistance, PitchDistance, SpectralDistance, _native, dtw_distance
from vq_voice_swap_amd.audio import ChunkWriter
from vq_voice_swap_amd.det_init import det_init_

import dtw_ref as dr
from util import record_margin, seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = "dtw_margins.jsonl"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def bits(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


# ---------------------------------------------------------------- cepstra
def cepstra_call(d, x, lengths, guard=8):
    """The C entry point with outputs NaN-guarded past their ends and `lengths` as DEVICE data (no host check) -> ceps, logmel,
    frames, and whether every guard element is still NaN."""
    B, T = x.shape
    F = T // d.hop + 1
    c = d.constants(x.device)
    ceps = torch.full((B * F * d.n_ceps + guard,), float("nan"), device=x.device)
    mel = torch.full((B * F * d.n_mels + guard,), float("nan"), device=x.device)
    frames = torch.full((B + guard,), -7, device=x.device, dtype=torch.int32)
    n = torch.tensor(lengths, dtype=torch.int32, device=x.device)
    _native.check(_native.lib().vqvs_mel_cepstra(x.data_ptr(), n.data_ptr(), c["window"].data_ptr(), c["twiddle"].data_ptr(), c["fb"].data_ptr(),
                                                 c["dct"].data_ptr(), ceps.data_ptr(), mel.data_ptr(), frames.data_ptr(), B, T, d.n_fft, d.hop,
                                                 d.n_mels, d.n_ceps, d.eps, _native._stream_ptr()))
    clean = bool(ceps[-guard:].isnan().all() and mel[-guard:].isnan().all() and (frames[B:] == -7).all())
    return ceps[:-guard].view(B, F, d.n_ceps), mel[:-guard].view(B, F, d.n_mels), frames[:B], clean


@pytest.mark.parametrize("cfg", [dr.CFG_SMALL, dr.CFG_DEFAULT])
def test_cepstra_of_padded_rows(dev, cfg):
    """Rows of five lengths -- the shortest accepted, an odd one, one frame short of a workgroup's eight, the full row -- padded with
    NaN: finite, zero from the row's own frame count on, nothing written past the arrays, bitwise what the recording alone gives at
    T = its length, and within 1e-4 of the float64 restatement (its float32 roundings are the kernel's; what is left is the FFT
    against the direct DFT, a few float32 ulps of log-mel values below 16 spread over n_mels terms: about 1e-5)."""
    n_fft, hop, n_mels, n_ceps = cfg
    d = SpectralDistance(n_fft=n_fft, hop=hop, n_mels=n_mels, n_ceps=n_ceps)
    T = 25 * hop + 7
    lengths = [n_fft // 2 + 1, n_fft + 13, 7 * hop - 1, 17 * hop, T]
    x = 0.3 * seeded((len(lengths), T), 5)
    padded = x.clone()
    for row, n in enumerate(lengths):
        padded[row, n:] = float("nan")
    ceps, mel, frames, clean = cepstra_call(d, padded.to(dev), lengths)
    assert clean and frames.tolist() == [n // hop + 1 for n in lengths]
    assert torch.isfinite(ceps).all() and torch.isfinite(mel).all()
    want_c, want_m, want_f = dr.cepstra_ref(x.numpy(), lengths, cfg, logmel=True)
    assert want_f.tolist() == frames.tolist()
    for row, n in enumerate(lengths):
        F = n // hop + 1
        assert not ceps[row, F:].any() and not mel[row, F:].any()
        alone = d.cepstra(x[row:row + 1, :n].to(dev).contiguous(), [n], logmel=True)
        assert alone["frames"].tolist() == [F] and alone["ceps"].shape == (1, F, n_ceps)
        assert torch.equal(bits(alone["ceps"][0]), bits(ceps[row, :F])) and torch.equal(bits(alone["logmel"][0]), bits(mel[row, :F]))
        err = max(np.abs(ceps[row].cpu().numpy() - want_c[row]).max(), np.abs(mel[row].cpu().numpy() - want_m[row]).max())
        record_margin(MARGINS, {"test": "cepstra_vs_float64", "cfg": list(cfg), "length": n, "max_abs_err": float(err), "bound": 1e-4})
        assert err <= 1e-4 and np.abs(want_c[row, :F, 1:]).max() > 0.1, (cfg, n, err)
    # the wrapper, zero padding, another batch and another row: the same bits
    zero = torch.where(padded.isnan(), torch.zeros_like(padded), padded)
    got = d.cepstra(zero[[3, 1]].to(dev)[:, None], torch.tensor([lengths[3], lengths[1]]))
    assert "logmel" not in got and torch.equal(bits(got["ceps"]), bits(ceps[[3, 1]])) and got["frames"].tolist() == [frames.tolist()[3], frames.tolist()[1]]
    # lengths are device data: whatever they hold is clamped into n_fft / 2 + 1 .. T and nothing outside the arrays is touched
    wild = [0, -5, T + 100, 2 ** 31 - 1, -2 ** 31]
    ceps_w, _, frames_w, clean = cepstra_call(d, zero.to(dev), wild)
    lo, hi = n_fft // 2 + 1, T
    assert clean and frames_w.tolist() == [lo // hop + 1, lo // hop + 1, hi // hop + 1, hi // hop + 1, lo // hop + 1]
    ceps_c, _, _, _ = cepstra_call(d, zero.to(dev), [lo, lo, hi, hi, lo])
    assert torch.equal(bits(ceps_w), bits(ceps_c))


@pytest.mark.parametrize("cfg", [dr.CFG_SMALL, dr.CFG_DEFAULT])
def test_stored_cepstra_give_the_fused_kernels_mcd(dev, cfg):
    """Equal lengths: the frame-for-frame MCD formed in float64 from the stored cepstra, summed in frame order, against
    `vqvs_spectral_distance`'s own sum: identical float32 cepstra on both sides, so only the rounding order of two float64
    evaluations separates them -- relative 2 (n_ceps + F + 4) 2^-53."""
    n_fft, hop, n_mels, n_ceps = cfg
    d = SpectralDistance(n_fft=n_fft, hop=hop, n_mels=n_mels, n_ceps=n_ceps)
    T = 1119
    a, b = (0.3 * seeded((3, T), 40)).to(dev), (0.3 * seeded((3, T), 41)).to(dev)
    fused = d(a, b)["mcd"].cpu().numpy()
    ca, cb = (d.cepstra(x, [T] * 3)["ceps"].cpu().numpy() for x in (a, b))
    F = T // hop + 1
    bound = dr.bound_factor(n_ceps, F, 0)
    for row in range(3):
        per_frame = np.diagonal(dr.local_cost(ca[row], cb[row])).tolist()
        total = 0.0
        for v in per_frame:
            total = total + v
        frac = abs(total - fused[row]) / (bound * fused[row])
        record_margin(MARGINS, {"test": "stored_cepstra_mcd", "cfg": list(cfg), "row": row, "fraction_of_bound": frac})
        assert fused[row] > 0 and frac <= 1.0, (cfg, row, total, fused[row])


# ---------------------------------------------------------------- alignment
def batch_of(inputs, order, fa_max, fb_max, dev, tracks=True):
    """The pairs `order` of `inputs` as one padded batch; cepstra beyond a pair's counts are NaN and tracks there 1e30: never read."""
    n_ceps = inputs[0][0].shape[1]
    B = len(order)
    ca = torch.full((B, fa_max, n_ceps), float("nan"))
    cb = torch.full((B, fb_max, n_ceps), float("nan"))
    ta, tb = torch.full((B, fa_max), 1e30, dtype=torch.float64), torch.full((B, fb_max), 1e30, dtype=torch.float64)
    fa, fb = [], []
    for row, k in enumerate(order):
        a, b, t, u, _ = inputs[k]
        ca[row, :len(a)], cb[row, :len(b)] = torch.tensor(a), torch.tensor(b)   # (copies: the shared inputs are read-only)
        ta[row, :len(a)], tb[row, :len(b)] = torch.tensor(t), torch.tensor(u)
        fa.append(len(a))
        fb.append(len(b))
    args = [ca.to(dev), fa, cb.to(dev), fb] + ([ta.to(dev), tb.to(dev)] if tracks else [])
    return {k: v.cpu() for k, v in dtw_distance(*args).items()}


def check_against_reference(name, got, row, ref, n_ceps, Fa, Fb):
    bound = dr.bound_factor(n_ceps, Fa, Fb)
    cost = float(got["cost"][row])
    frac = abs(cost - ref["cost"]) / (bound * ref["cost"]) if ref["cost"] else float(cost != 0.0)
    s2_bound = bound * ref["s2"]
    s1_bound = bound * np.sqrt(ref["both"] * ref["s2"])  # sum |l| <= sqrt(n sum l^2)
    s1_err, s2_err = abs(float(got["shift_sum"][row]) - ref["s1"]), abs(float(got["shift_sq_sum"][row]) - ref["s2"])
    record_margin(MARGINS, {"test": name, "shape": [Fa, Fb], "n_ceps": n_ceps, "row": row, "cost": cost, "fraction_of_bound": frac,
                            "bit_equal": cost == ref["cost"], "shift_sum_fraction": s1_err / s1_bound if s1_bound else float(s1_err != 0),
                            "shift_sq_sum_fraction": s2_err / s2_bound if s2_bound else float(s2_err != 0), "margin": ref["margin"]})
    assert frac <= 1.0, (name, Fa, Fb, cost, ref["cost"])
    assert (int(got["steps"][row]), int(got["both"][row]), int(got["vuv"][row])) == (ref["steps"], ref["both"], ref["vuv"]), (name, Fa, Fb)
    assert s1_err <= s1_bound and s2_err <= s2_bound, (name, Fa, Fb, s1_err, s1_bound, s2_err, s2_bound)


@pytest.fixture(scope="module")
def mixed(dev):
    """All nine shapes in one padded batch, the largest first and last; computed once."""
    return batch_of(dr.dtw_inputs(), dr.BATCH_ORDER, 263, 305, dev)


def test_alignment_against_the_reference(mixed):
    inputs = dr.dtw_inputs()
    assert mixed["cost"].dtype == torch.float64 and mixed["steps"].dtype == torch.int32 and mixed["both"].dtype == torch.int64
    for row, k in enumerate(dr.BATCH_ORDER):
        Fa, Fb = dr.SHAPES[k]
        check_against_reference("mixed_batch", mixed, row, inputs[k][4], dr.CFG_SMALL[3], Fa, Fb)
    assert torch.equal(bits(mixed["cost"][0]), bits(mixed["cost"][-1])) and mixed["steps"][0] == mixed["steps"][-1]   # the same pair twice


def test_alignment_is_independent_of_batch_row_and_padding(dev, mixed):
    """Every pair alone at F*_max = its own counts, and two pairs under the kernel's largest rings (F*_max = 2048: the LDS request
    above 64 KiB): bitwise the mixed batch's values."""
    inputs = dr.dtw_inputs()
    for k, (Fa, Fb) in enumerate(dr.SHAPES):
        alone = batch_of(inputs, [k], Fa, Fb, dev)
        row = dr.BATCH_ORDER.index(k)
        for key in ("cost", "steps", "both", "vuv", "shift_sum", "shift_sq_sum"):
            assert torch.equal(bits(alone[key][0]), bits(mixed[key][row])), (Fa, Fb, key)
    wide = batch_of(inputs, [7, 3], 2048, 2048, dev)
    for row, k in enumerate((7, 3)):
        for key in ("cost", "steps", "both", "vuv", "shift_sum", "shift_sq_sum"):
            assert torch.equal(bits(wide[key][row]), bits(mixed[key][dr.BATCH_ORDER.index(k)])), (k, key)


def test_alignment_without_tracks_and_swapped(dev, mixed):
    inputs = dr.dtw_inputs()
    plain = batch_of(inputs, dr.BATCH_ORDER, 263, 305, dev, tracks=False)
    assert sorted(plain) == ["cost", "steps"]
    assert torch.equal(bits(plain["cost"]), bits(mixed["cost"])) and torch.equal(plain["steps"], mixed["steps"])
    swapped = tuple((b, a, u, t, None) for a, b, t, u, _ in inputs)
    back = batch_of(swapped, dr.BATCH_ORDER, 305, 263, dev)
    assert torch.equal(bits(back["cost"]), bits(mixed["cost"])) and torch.equal(back["steps"], mixed["steps"])
    assert torch.equal(back["both"], mixed["both"]) and torch.equal(back["vuv"], mixed["vuv"])
    assert torch.equal(bits(back["shift_sum"]), bits(-mixed["shift_sum"] + 0.0)) and torch.equal(bits(back["shift_sq_sum"]), bits(mixed["shift_sq_sum"]))


def test_alignment_of_a_recording_with_itself(dev):
    """d(a, a): cost exactly 0 and steps = F, for noise and for constant cepstra, where only the tie-break decides."""
    for F in (1, 9, 64, 300):
        noise = torch.from_numpy(dr.noise_cepstra(F, 5, F))[None]
        for c in (noise, torch.ones(1, F, 5)):
            t = torch.from_numpy(dr.noise_track(F, F))[None].to(dev)
            got = dtw_distance(c.to(dev), [F], c.to(dev), [F], t, t)
            assert bits(got["cost"]).tolist() == [0] and got["steps"].tolist() == [F] and got["vuv"].tolist() == [0]
            assert got["both"].tolist() == [int(torch.isfinite(t).sum())] and bits(got["shift_sum"]).tolist() == [0] and bits(got["shift_sq_sum"]).tolist() == [0]
    flat = dtw_distance(torch.ones(1, 4, 5, device=dev), [4], torch.ones(1, 7, 5, device=dev), [7])
    assert flat["cost"].tolist() == [0.0] and flat["steps"].tolist() == [7]


def test_alignment_at_the_longest_side_and_at_the_default_width(dev):
    """2048 frames against 3 and 3 against 2048 (eight rows per thread, rings of 2048 slots), and 13 coefficients."""
    inputs = dr.dtw_inputs(shapes=dr.LONG_SHAPES)
    for k, (Fa, Fb) in enumerate(dr.LONG_SHAPES):
        got = batch_of(inputs, [k], Fa, Fb, dev)
        check_against_reference("long_side", got, 0, inputs[k][4], dr.CFG_SMALL[3], Fa, Fb)
    wide = dr.dtw_inputs(dr.CFG_DEFAULT[3], ((129, 70),))
    check_against_reference("default_width", batch_of(wide, [0, 0], 140, 70, dev), 1, wide[0][4], dr.CFG_DEFAULT[3], 129, 70)


def test_frame_counts_are_clamped_device_data(dev):
    """Counts outside 1..F*_max, handed over as device data: the values of the clamped counts, and nothing else happens."""
    inputs = dr.dtw_inputs()
    a, b = torch.tensor(inputs[5][0])[None].to(dev), torch.tensor(inputs[5][1])[None].to(dev)   # (17, 9)
    ca, cb = a.repeat(4, 1, 1).contiguous(), b.repeat(4, 1, 1).contiguous()
    wild = dtw_distance(ca, torch.tensor([0, 99, -3, 2 ** 31 - 1], dtype=torch.int32, device=dev), cb,
                        torch.tensor([100, -2 ** 31, 9, 0], dtype=torch.int32, device=dev))
    want = dtw_distance(ca, [1, 17, 1, 17], cb, [9, 1, 9, 1])
    assert torch.equal(bits(wild["cost"]), bits(want["cost"])) and torch.equal(wild["steps"], want["steps"])
    assert want["steps"].tolist() == [9, 17, 9, 17]


# ---------------------------------------------------------------- AlignedDistance
def sweep(n, f_lo, f_hi, amp=0.3):
    """A three-harmonic tone gliding from f_lo to f_hi Hz over n samples at 16 kHz."""
    phase = 2 * np.pi * np.cumsum(np.linspace(f_lo, f_hi, n)) / 16000.0
    return (amp * (np.sin(phase) + 0.5 * np.sin(2 * phase) + 0.25 * np.sin(3 * phase)) / 1.75).astype(np.float32)


def test_aligned_distance_of_a_padded_recording(dev):
    """A short pair padded (with NaN) into a batch beside a longer one: its scores, with and without a `PitchDistance`, are bitwise
    those of the pair alone; the sweeps are voiced, so the pitch figures are about something."""
    a_short, b_short, a_long, b_long = sweep(4000, 110, 180), sweep(5500, 130, 210), sweep(9600, 200, 120), sweep(8000, 180, 140)
    A, Bt = torch.full((2, 9600), float("nan")), torch.full((2, 8000), float("nan"))
    A[0, :4000], A[1], Bt[0, :5500], Bt[1] = torch.from_numpy(a_short), torch.from_numpy(a_long), torch.from_numpy(b_short), torch.from_numpy(b_long)
    for pitch in (None, PitchDistance()):
        aligned = AlignedDistance(SpectralDistance(), pitch)
        both = aligned(A.to(dev), [4000, 9600], Bt.to(dev)[:, None], torch.tensor([5500, 8000]))
        alone = aligned(torch.from_numpy(a_short)[None, None].to(dev), [4000], torch.from_numpy(b_short)[None].to(dev), [5500])
        keys = ["cost", "steps", "frames_a", "frames_b"] + (["both", "vuv", "shift_sum", "shift_sq_sum"] if pitch else [])
        assert sorted(both) == sorted(keys) == sorted(alone)
        for key in keys:
            assert torch.equal(bits(both[key][0]), bits(alone[key][0])), key
        assert both["frames_a"].tolist() == [26, 61] and both["frames_b"].tolist() == [35, 51]
        assert (both["steps"] >= torch.maximum(both["frames_a"], both["frames_b"])).all() and torch.isfinite(both["cost"]).all() and (both["cost"] > 0).all()
        if pitch:
            assert (both["both"] > 10).all() and torch.isfinite(both["shift_sum"]).all()
            assert ((both["shift_sum"] / both["both"]).abs() < 24).all()   # (within two octaves: 60 .. 500 Hz are searched)
        same = aligned(A[1:].to(dev), [9600], A[1:].to(dev), [9600])
        assert same["cost"].tolist() == [0.0] and same["steps"].tolist() == [61]


# ---------------------------------------------------------------- the script
PAIRS = (("s1/a.wav", 8000, "t/a.wav", 7000, 1), ("s1/b.wav", 3200, "t/b.wav", 4000, 1), ("s2/a.wav", 1600, "t/c.wav", 2000, 2),
         ("s2/b.wav", 4800, "t/d.wav", 5200, 2))
WINDOW_FLAGS = ["--window-seconds", "0.128", "--overlap-seconds", "0.032", "--sample-steps", "2", "--seed", "9"]


def test_eval_parallel(dev, tmp_path, capsys):
    """A det_init base-32 VQ-VAE and four pairs of unequal lengths: the `--checkpoint` run's merged line equals the line of
    convert_dataset.py followed by `--converted-dir` on its output, character for character, and itself at another --pack-windows."""
    sys.path.insert(0, ROOT)
    import convert_dataset
    import eval_parallel

    model = VQVAE(base_channels=32, pred_name="unet", num_labels=3)
    det_init_(model.state_dict().items())
    ck, data, out = str(tmp_path / "v.pt"), tmp_path / "data", tmp_path / "out"
    model.save(ck)
    for i, (src, n_s, tgt, n_t, _) in enumerate(PAIRS):
        for rel, n, lo, hi in ((src, n_s, 100 + 10 * i, 160 + 10 * i), (tgt, n_t, 140 + 10 * i, 220 + 10 * i)):
            os.makedirs(data / os.path.dirname(rel), exist_ok=True)
            w = ChunkWriter(str(data / rel), 16000)
            w.write(sweep(n, lo, hi))
            w.close()
    table = tmp_path / "pairs.tsv"
    table.write_text("# source, target, label\n" + "".join(f"{s}\t{t}\t{label}\n" for s, _, t, _, label in PAIRS))
    labels = tmp_path / "targets.tsv"
    labels.write_text("s1\t1\ns2\t2\nt\t0\n")   # the sources sort first: file id i is pair i

    def line(*flags):
        capsys.readouterr()
        state = eval_parallel.main([str(table), str(data), "--pitch", *flags])
        lines = [ln for ln in capsys.readouterr().out.splitlines() if " pairs: " in ln]
        assert state.num_pairs == 4 and lines[-1].startswith("4 pairs: mcd_dtw=") and "src_vuv_err_dtw=" in lines[-1]
        return lines[-1], len(lines) - 1

    one, packs_one = line("--checkpoint", ck, *WINDOW_FLAGS, "--pack-windows", "64")
    small, packs_small = line("--checkpoint", ck, *WINDOW_FLAGS, "--pack-windows", "2", "--window-batch", "2")
    assert small == one and (packs_one, packs_small) == (1, 4)
    convert_dataset.main([ck, str(data), str(out), "--label-map", str(labels), *WINDOW_FLAGS, "--pack-windows", "5"])
    files, _ = line("--converted-dir", str(out), "--pack-windows", "3")
    assert files == one
    state = eval_parallel.main([str(table), str(data), "--converted-dir", str(out), "--max-pairs", "2"])
    assert state.num_pairs == 2 and not state.pitch
    log = state.log_dict()
    assert log["mcd_dtw"] > 0 and log["src_mcd_dtw"] > 0 and 1.0 <= log["stretch"] < 2.0
