"""Sample-quality statistics on the host: Frechet distance, class score, merging of moment states (Chan), the two-rank
all_reduce (gloo), the WAV round trip of in-line statistics, and the plumbing of stat_generate.py / stat_compare.py /
sample_diffusion.py's new flags.  No GPU needed."""
import contextlib
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vq_voice_swap_amd import FeatureStats, class_score, frechet_distance, wav_roundtrip
from vq_voice_swap_amd.audio import ChunkReader, ChunkWriter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_spd(rng, n, floor=0.1):
    a = rng.standard_normal((n, n))
    return a @ a.T / n + floor * np.eye(n)


# ---- Frechet distance

def test_frechet_distance_diagonal_closed_form():
    rng = np.random.default_rng(0)
    for n in (1, 5, 64):
        a, b = rng.uniform(0.2, 3.0, n), rng.uniform(0.2, 3.0, n)
        mu1, mu2 = rng.standard_normal(n), rng.standard_normal(n)
        want = np.sum((np.sqrt(a) - np.sqrt(b)) ** 2) + np.sum((mu1 - mu2) ** 2)
        got = frechet_distance(mu1, np.diag(a), mu2, np.diag(b))
        assert abs(got - want) <= 1e-12 * abs(want), (n, got, want)


def test_frechet_distance_symmetric_and_zero_on_identical_inputs():
    rng = np.random.default_rng(1)
    s1, s2 = random_spd(rng, 48), random_spd(rng, 48)
    mu1, mu2 = rng.standard_normal(48), rng.standard_normal(48)
    d12, d21 = frechet_distance(mu1, s1, mu2, s2), frechet_distance(mu2, s2, mu1, s1)
    assert d12 > 0 and abs(d12 - d21) <= 1e-10 * d12
    assert abs(frechet_distance(mu1, s1, mu1, s1)) <= 1e-8 * np.trace(s1)
    # a singular (rank-deficient) covariance is still positive semi-definite: no eps fallback needed, same value either way
    x = rng.standard_normal((10, 48))
    sing = np.cov(x, rowvar=False)
    assert abs(frechet_distance(mu1, sing, mu1, sing)) <= 1e-8 * np.trace(sing)


def test_frechet_distance_matches_scipy_sqrtm():
    linalg = pytest.importorskip("scipy.linalg")
    rng = np.random.default_rng(2)
    for _ in range(4):
        s1, s2 = random_spd(rng, 64), random_spd(rng, 64)
        mu1, mu2 = rng.standard_normal(64), rng.standard_normal(64)
        covmean = linalg.sqrtm(s1.dot(s2))
        covmean = np.real(covmean)
        diff = mu1 - mu2
        want = diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean)
        got = frechet_distance(mu1, s1, mu2, s2)
        assert abs(got - want) <= 1e-9 * abs(want), (got, want)


# ---- class score

def test_class_score():
    assert class_score(np.full((10, 7), 1 / 7)) == pytest.approx(1.0, abs=1e-14)
    for k in (1, 3, 7):
        assert class_score(np.eye(k)) == pytest.approx(float(k), rel=1e-14)
    rng = np.random.default_rng(3)
    p = rng.uniform(0.01, 1.0, (50, 9))
    p /= p.sum(axis=1, keepdims=True)
    kl = p * (np.log(p) - np.log(np.expand_dims(np.mean(p, 0), 0)))  # stat_generate.py:47-52, as the reference writes it
    want = np.exp(np.mean(np.sum(kl, 1)))
    assert class_score(p) == pytest.approx(want, rel=1e-13)
    assert class_score(p.astype(np.float32)) == pytest.approx(class_score(p.astype(np.float32).astype(np.float64)), rel=1e-15)


# ---- moment states

def state_of(chunk, shift):
    d = chunk - shift
    return FeatureStats.from_moments(len(chunk), shift, d.sum(0), d.T @ d, device="cpu")


def rel_fro(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("offset", [0.0, 1e4])
def test_merge_of_chunks_with_different_shifts(offset):
    rng = np.random.default_rng(4)
    x = rng.standard_normal((300, 24)) * rng.uniform(0.5, 3.0, 24) + offset + rng.standard_normal(24)
    cuts = [0, 1, 2, 50, 51, 170, 299, 300]  # 1-row chunks included
    total = FeatureStats(24, device="cpu")
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        shift = x[a] if i % 2 else x[a:b].mean(0) + 3.0  # (every chunk has its own shift)
        total.merge(state_of(x[a:b], shift))
    assert total.n == 300
    assert rel_fro(total.mean(), x.mean(0)) <= 1e-12
    assert rel_fro(total.cov(), np.cov(x, rowvar=False)) <= 1e-12
    # merging into a non-empty state in a different grouping gives the same statistics
    left, right = state_of(x[:120], x[0]), state_of(x[120:], x[200])
    left.merge(right)
    assert rel_fro(left.cov(), np.cov(x, rowvar=False)) <= 1e-12


def test_state_errors_and_probs():
    st = FeatureStats(4, device="cpu")
    with pytest.raises(ValueError):
        st.mean()
    with pytest.raises(ValueError):
        FeatureStats(0, device="cpu")
    with pytest.raises(RuntimeError):  # the accumulation is a device kernel: host features are refused, not summed on the CPU
        st.update(torch.zeros(2, 4))
    a = state_of(np.arange(8.0).reshape(2, 4), np.zeros(4))
    a.add_probs(np.eye(2, 3))
    b = state_of(np.arange(8.0, 16.0).reshape(2, 4), np.ones(4))
    b.add_probs(np.eye(2, 3)[::-1])
    a.merge(b)
    assert a.probs.shape == (4, 3) and np.array_equal(a.probs[2:], np.eye(2, 3)[::-1])


ALL_REDUCE_WORKER = r"""
import sys, numpy as np, torch.distributed as dist
sys.path.insert(0, {root!r})
from vq_voice_swap_amd.stats import FeatureStats
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
rng = np.random.default_rng(5)
x = rng.standard_normal((37, 16)) * 2.0 + 1e3
p = rng.uniform(0.1, 1.0, (37, 5)); p /= p.sum(1, keepdims=True)
lo, hi = (0, 15) if rank == 0 else (15, 37)
d = x[lo:hi] - x[lo]
st = FeatureStats.from_moments(hi - lo, x[lo], d.sum(0), d.T @ d, probs=p[lo:hi], device="cpu")
st.all_reduce()
d = x - x[0]
one = FeatureStats.from_moments(37, x[0], d.sum(0), d.T @ d, probs=p, device="cpu")
rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
assert st.n == 37
assert rel(st.mean(), one.mean()) <= 1e-12 and rel(st.cov(), one.cov()) <= 1e-12, (rel(st.mean(), one.mean()), rel(st.cov(), one.cov()))
assert np.array_equal(st.probs, one.probs.astype(np.float32))
assert abs(st.class_score() - one.class_score()) <= 1e-12 * one.class_score()
print(f"ALL_REDUCE_OK {{rank}}\n", end="", flush=True)  # one write: the two ranks share the pipe, and pieces of two prints can interleave
dist.destroy_process_group()
"""


def test_two_rank_all_reduce_gloo(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(ALL_REDUCE_WORKER.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29547", str(script)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL_REDUCE_OK 0" in r.stdout and "ALL_REDUCE_OK 1" in r.stdout


# ---- the WAV round trip of in-line statistics

@pytest.mark.parametrize("encoding", ["linear", "ulaw"])
def test_wav_roundtrip_is_the_file_route(tmp_path, encoding):
    g = torch.Generator().manual_seed(6)
    x = torch.randn(3, 1, 4096, generator=g) * 0.7  # some samples past +-1: the clip is part of the route
    got = wav_roundtrip(x, encoding)
    for i in range(3):
        path = str(tmp_path / f"c{i}.wav")
        w = ChunkWriter(path, 16000, encoding=encoding)
        w.write(x[i].reshape(-1).numpy())
        w.close()
        back = torch.from_numpy(ChunkReader(path, 16000).read(1 << 20))
        if encoding == "linear":
            assert torch.equal(got[i, 0], back)
        else:  # (torch's and numpy's float32 pow may round apart: one s16 step at most)
            assert (got[i, 0] - back).abs().max().item() <= 1 / 2 ** 15
    with pytest.raises(ValueError):
        wav_roundtrip(x, "mp3")


# ---- C ABI and script plumbing

def test_feature_moments_argument_errors_without_a_device(lib_built):
    L = lib_built
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p)
    assert L.vqvs_feature_moments(None, 4, 8, p, p, p, None) == -1
    assert L.vqvs_feature_moments(p, 4, 8, None, p, p, None) == -1
    assert L.vqvs_feature_moments(p, 4, 8, p, None, p, None) == -1
    assert L.vqvs_feature_moments(p, 4, 8, p, p, None, None) == -1
    assert L.vqvs_feature_moments(p, 4, 0, p, p, p, None) == -1
    assert L.vqvs_feature_moments(p, 4, -3, p, p, p, None) == -1
    assert L.vqvs_feature_moments(p, 4, 8193, p, p, p, None) == -1
    assert L.vqvs_feature_moments(p, 0, 8, p, p, p, None) == -1
    assert L.vqvs_classifier_features(None, p, p, p, None, None, 1, 512, None) == -1


def test_stat_compare_reads_reference_format(tmp_path):
    import stat_compare

    rng = np.random.default_rng(7)
    x, y = rng.standard_normal((40, 6)), rng.standard_normal((30, 6)) + 0.5
    files = []
    for name, z in (("a.npz", x), ("b.npz", y)):  # the reference's dtypes: float32 mean (np.mean of float32 features), float64 cov
        np.savez(tmp_path / name, mean=z.mean(0).astype(np.float32), cov=np.cov(z, rowvar=False), probs=np.zeros((2, 2), np.float32),
                 class_score=1.0)
        files.append(str(tmp_path / name))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        stat_compare.main(files)
    want = frechet_distance(x.mean(0).astype(np.float32), np.cov(x, rowvar=False), y.mean(0).astype(np.float32), np.cov(y, rowvar=False))
    assert float(out.getvalue().strip()) == pytest.approx(want, rel=1e-12)


def test_stat_generate_flags(tmp_path):
    import stat_generate

    args = stat_generate.parse_args(["--checkpoint-path", "clf.pt", "--batch-size", "8", "--num-samples", "100", "--sample-dir",
                                     str(tmp_path), str(tmp_path / "out.npz")])
    assert (args.checkpoint_path, args.batch_size, args.num_samples, args.precision) == ("clf.pt", 8, 100, "fp32")
    err = io.StringIO()
    with pytest.raises(SystemExit), contextlib.redirect_stderr(err):
        stat_generate.parse_args(["--data-dir", str(tmp_path), "out.npz"])
    assert "--data-dir" in err.getvalue()


def test_stat_generate_refuses_lengths_off_the_downsample_grid(tmp_path):
    import stat_generate

    for i, n in enumerate((1024, 1000)):
        w = ChunkWriter(str(tmp_path / f"s{i}.wav"), 16000)
        w.write(np.zeros(n, np.float32))
        w.close()
    with pytest.raises(SystemExit, match="s1.wav"):
        list(stat_generate.batches_of_equal_length(stat_generate.list_samples(str(tmp_path)), 4, 512))


def test_sample_diffusion_stats_flags():
    import sample_diffusion

    ok = sample_diffusion.parse_args(["--num-samples", "2", "--stats-classifier", "c.pt", "--stats-path", "s.npz"])
    assert ok.stats_precision == "fp32"
    assert sample_diffusion.parse_args([]).stats_path is None
    for bad in (["--num-samples", "4", "--stats-path", "s.npz"], ["--num-samples", "4", "--stats-classifier", "c.pt"],
                ["--stats-classifier", "c.pt", "--stats-path", "s.npz"],
                ["--num-samples", "1", "--stats-classifier", "c.pt", "--stats-path", "s.npz"]):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            sample_diffusion.parse_args(bad)
