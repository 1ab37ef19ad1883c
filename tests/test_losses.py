"""Denoising-loss evals, host side: the loss tracker, the data sets, the scripts' flags, and the argument checks of the two
kernels' entry points (none of this needs a device).  Fixture F16 is written by tools/gen_loss_golden.py from the reference."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from vq_voice_swap_amd import LossTracker, create_data_loader
from vq_voice_swap_amd.audio import ChunkWriter, encode_u_law
from vq_voice_swap_amd.dataset import AudioFormatError, SpeakerWindows, ToneDataset

from util import flags_of


@pytest.fixture(scope="module")
def f16(golden):
    return golden("f16_denoising_losses")


def as_row(tracker):
    log = tracker.log_dict()
    return [log.get(f"q{i}", float("nan")) for i in range(4)]


# ---------------------------------------------------------------- tracker (fixture D)
def test_tracker_matches_reference_exactly(f16):
    tracker = LossTracker(avg_size=int(f16["d_avg_size"]))
    for ts, mses, want in zip(f16["d_ts"], f16["d_mses"], f16["d_logs"]):
        tracker.add(torch.from_numpy(ts), torch.from_numpy(mses))
        got = np.array(as_row(tracker), dtype=np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])  # the same floats, not close ones
    assert max(tracker.counts()) == int(f16["d_avg_size"])  # (the window did slide)


def test_tracker_keys_buckets_and_prefix():
    tracker = LossTracker(quantiles=4, avg_size=3, prefix="eval_")
    tracker.add(np.array([0.0, 0.2499, 0.26, 1.0], dtype=np.float32), np.array([1.0, 3.0, 5.0, 7.0], dtype=np.float32))
    assert tracker.log_dict() == {"eval_q0": 2.0, "eval_q1": 5.0, "eval_q3": 7.0}
    assert tracker.quantile_averages() == [2.0, 5.0, None, 7.0]
    tracker.add(torch.tensor([0.1, 0.1]), torch.tensor([9.0, 11.0]))  # window of 3: the 1.0 leaves
    assert tracker.log_dict()["eval_q0"] == pytest.approx((3.0 + 9.0 + 11.0) / 3)
    with pytest.raises(IndexError):
        tracker.add(np.array([1.5]), np.array([0.0]))


def test_tracker_large_window_grows_and_slides():
    rng = np.random.default_rng(0)
    vals = rng.random(5000)
    tracker = LossTracker(quantiles=1, avg_size=3000)
    for part in np.split(vals, 10):
        tracker.add(np.full(part.size, 0.5), part)
    assert tracker.quantile_averages()[0] == float(np.mean(vals[-3000:]))


def test_tracker_merge_of_two_halves_equals_one(f16):
    ts, mses = f16["d_ts"].reshape(-1), f16["d_mses"].reshape(-1)
    one, a, b = (LossTracker(avg_size=1000) for _ in range(3))
    one.add(ts, mses)
    half = ts.size // 2
    a.add(ts[:half], mses[:half])
    b.add(ts[half:], mses[half:])
    assert a.merge(b).log_dict() == one.log_dict()
    assert a.counts() == one.counts()
    with pytest.raises(ValueError):
        a.merge(LossTracker(quantiles=3))


# ---------------------------------------------------------------- tones (fixture C)
def test_tones_match_reference(f16):
    items = [int(i) for i in f16["c_items"]]
    lin, ulaw = ToneDataset("linear"), ToneDataset("ulaw")
    assert len(lin) == 30 and lin.speaker_ids == [300, 500, 1000]
    for k, i in enumerate(items):
        a, u = lin[i], ulaw[i]
        assert a["label"] == int(f16["c_linear_labels"][k]) == u["label"] == int(f16["c_ulaw_labels"][k])
        assert a["samples"].shape == (64000,) and a["samples"].dtype == np.float32
        err = np.abs(a["samples"][:64] - f16["c_linear_head"][k]).max()
        print(f"tones item {i}: max |linear - reference| over the head = {err:.3e}")
        assert err <= 8e-3
        # ulaw: the same samples through the existing codec
        assert np.array_equal(u["samples"], encode_u_law(a["samples"]))
        # ... which the reference's head agrees with to the linear bound times the codec's steepest slope, mu / ln(1 + mu)
        assert np.abs(u["samples"][:64] - f16["c_ulaw_head"][k]).max() <= 8e-3 * 255 / np.log(256)
    # the far end of a clip, where the reference's float32 argument is coarsest: float64 closed form
    n = np.arange(64000, dtype=np.float64)
    want = np.sin(2 * np.pi * 1000 * (n / 16000 + 0.9))
    assert np.abs(lin[29]["samples"] - want).max() <= 1e-6


def test_tones_loader_batches():
    loader, num_labels = create_data_loader("tones", batch_size=4, seed=3)
    assert num_labels == 3
    batches = list(loader)
    assert len(batches) == 7  # 30 items, incomplete batch dropped
    assert batches[0]["samples"].shape == (4, 64000) and batches[0]["samples"].dtype == torch.float32
    assert batches[0]["label"].dtype == torch.int64
    again = list(create_data_loader("tones", batch_size=4, seed=3)[0])
    assert all(torch.equal(x["label"], y["label"]) and torch.equal(x["samples"], y["samples"]) for x, y in zip(batches, again))
    # shards deal out the same batches
    r0 = list(create_data_loader("tones", batch_size=4, seed=3, rank=0, world=2)[0])
    r1 = list(create_data_loader("tones", batch_size=4, seed=3, rank=1, world=2)[0])
    assert len(r0) == 4 and len(r1) == 3
    assert torch.equal(r1[0]["samples"], batches[1]["samples"]) and torch.equal(r0[1]["samples"], batches[2]["samples"])


# ---------------------------------------------------------------- directory data set
def write_wav(path, samples):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    w = ChunkWriter(str(path), 16000)
    w.write(samples)
    w.close()


def ramp(n, start=0):
    """s16-exact samples that name their own position: sample k is (start + k) % 2000 / 2^15 after the reader's decode."""
    return (((start + np.arange(n)) % 2000) / (2 ** 15 - 1) + 1e-6).astype(np.float32)


def test_directory_dataset(tmp_path):
    root = tmp_path / "set"
    write_wav(root / "spk_b" / "ch1" / "long.wav", ramp(9600))    # 0.6 s
    write_wav(root / "spk_a" / "ch7" / "short.wav", ramp(1600))   # 0.1 s: shorter than a window
    write_wav(root / "spk_c" / "mid.wav", ramp(4000))             # directly under the speaker
    (root / "stray.wav").write_bytes(b"")                          # not under a speaker directory: ignored
    ds = SpeakerWindows(str(root), window_duration=0.25, window_spacing=0.1)
    assert ds.speaker_ids == ["spk_a", "spk_b", "spk_c"]
    rows = {(label, os.path.basename(path), off) for label, path, off in ds.data}
    # long: total = int(16000 * (0.6 - 0.05)) = 8800 samples, window 4000, spacing 1600 -> offsets below 4800
    assert rows == {(0, "short.wav", 0), (1, "long.wav", 0), (1, "long.wav", 1600), (1, "long.wav", 3200), (2, "mid.wav", 0)}
    by = {(os.path.basename(p), off): i for i, (_, p, off) in enumerate(ds.data)}
    item = ds[by[("long.wav", 1600)]]
    assert item["label"] == 1 and item["samples"].shape == (4000,)
    assert np.array_equal(np.rint(item["samples"] * 2 ** 15).astype(int), (1600 + np.arange(4000)) % 2000)
    short = ds[by[("short.wav", 0)]]
    assert np.array_equal(np.rint(short["samples"][:1600] * 2 ** 15).astype(int), np.arange(1600) % 2000)
    assert not short["samples"][1600:].any()  # zero-padded
    # the index is cached and reused: a tree whose files are gone still lists the same windows
    index = json.loads((root / "index.json").read_text())
    assert index["spk_b"]["ch1"]["long.wav"] == pytest.approx(0.6)
    os.remove(root / "spk_c" / "mid.wav")
    assert len(SpeakerWindows(str(root), window_duration=0.25, window_spacing=0.1)) == 5
    loader, num_labels = create_data_loader(str(root), batch_size=2, seed=0, window_duration=0.25, window_spacing=0.1)
    assert num_labels == 3 and len(loader) == 2
    # ulaw goes through the reader's codec
    u = SpeakerWindows(str(root), encoding="ulaw", window_duration=0.25, window_spacing=0.1)
    assert np.allclose(u[by[("long.wav", 1600)]]["samples"], encode_u_law(item["samples"]), atol=1e-6)


def test_directory_of_flac_only_is_refused(tmp_path):
    root = tmp_path / "libri"
    os.makedirs(root / "19" / "198")
    (root / "19" / "198" / "19-198-0001.flac").write_bytes(b"fLaC")
    with pytest.raises(AudioFormatError) as e:
        create_data_loader(str(root), batch_size=1)
    assert "FLAC" in str(e.value) and "19-198-0001.flac" in str(e.value)
    assert not (root / "index.json").exists()


# ---------------------------------------------------------------- scripts' flags
def test_eval_diffusion_flags():
    import eval_diffusion

    assert flags_of(eval_diffusion.arg_parser()) == sorted(
        ["--batch-size", "checkpoint_path", "data_dir", "--precision", "--seed", "--max-samples", "--dist-backend"])
    args = eval_diffusion.arg_parser().parse_args(["ckpt.pt", "tones"])
    assert (args.batch_size, args.precision, args.max_samples, args.checkpoint_path, args.data_dir) == (4, "fp32", None, "ckpt.pt", "tones")


def test_voice_search_flags():
    import voice_search_vqvae

    assert flags_of(voice_search_vqvae.arg_parser()) == sorted(
        ["--sample-rate", "--seconds", "--encoding", "--num-timesteps", "--num-seeds", "--batch-size", "--top-k", "--input-file",
         "checkpoint_path", "--precision", "--seed"])
    args = voice_search_vqvae.arg_parser().parse_args(["--input-file", "a.wav", "m.pt"])
    assert (args.sample_rate, args.seconds, args.encoding, args.num_timesteps, args.num_seeds, args.batch_size, args.top_k) == \
        (16000, 4, "linear", 16, 1, 16, 20)
    assert args.precision == "fp32"
    with pytest.raises(SystemExit):
        voice_search_vqvae.arg_parser().parse_args(["m.pt"])  # --input-file is required
    labels, ts = voice_search_vqvae.search_grid(3, 4, "cpu")
    assert labels.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    assert torch.equal(ts, torch.linspace(0, 1, 4).repeat(3))


def test_shim_exports():
    from vq_voice_swap.dataset import create_data_loader as shim_loader
    from vq_voice_swap.loss_tracker import LossTracker as ShimTracker

    assert shim_loader is create_data_loader and ShimTracker is LossTracker


# ---------------------------------------------------------------- entry points
def test_loss_entry_points_refuse_bad_arguments_without_a_device(lib_built):
    L = lib_built
    assert hasattr(L, "vqvs_ddpm_noise") and hasattr(L, "vqvs_ddpm_sqerr")
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p)
    B, T = 4, 8
    ok_noise = dict(x0=p, x0_rows=B, alpha=p, eps=p, eps_rows=B, idx=None, x_t=p, B=B, T=T)

    def noise(**kw):
        a = dict(ok_noise, **kw)
        return L.vqvs_ddpm_noise(a["x0"], a["x0_rows"], a["alpha"], a["eps"], a["eps_rows"], a["idx"], a["x_t"], a["B"], a["T"], 0, 0, None)

    for bad in (dict(x0=None), dict(alpha=None), dict(x_t=None), dict(B=0, x0_rows=0, eps_rows=0), dict(B=-1), dict(T=0),
                dict(x0_rows=2), dict(x0_rows=0), dict(x0_rows=5), dict(eps_rows=2), dict(eps_rows=0), dict(eps_rows=5),
                dict(eps=None, eps_rows=3), dict(B=70000, x0_rows=70000, eps_rows=70000)):
        assert noise(**bad) == -1, bad
    ok_sq = dict(pred=p, eps=p, eps_rows=B, idx=None, loss=p, B=B, T=T)

    def sqerr(**kw):
        a = dict(ok_sq, **kw)
        return L.vqvs_ddpm_sqerr(a["pred"], a["eps"], a["eps_rows"], a["idx"], a["loss"], a["B"], a["T"], 0, 0, None)

    for bad in (dict(pred=None), dict(loss=None), dict(B=0, eps_rows=0), dict(T=0), dict(T=-4), dict(eps_rows=2), dict(eps_rows=0),
                dict(eps_rows=7), dict(eps=None, eps_rows=2)):
        assert sqerr(**bad) == -1, bad
    assert b"eps_rows" in L.vqvs_last_error()
