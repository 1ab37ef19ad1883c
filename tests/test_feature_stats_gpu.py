"""Classifier features and sample-quality statistics on the GPU: `vqvs_classifier_features` against the reference (fixture F9)
and the CPU oracle, its consistency with the forward entry, the f64 moments kernel against numpy, in-line statistics of a
sampling run against stat_generate.py on the WAV files it wrote, and a two-rank stat_generate.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu
from vq_voice_swap_amd import Classifier, DiffusionModel, FeatureStats, frechet_distance
from vq_voice_swap_amd.det_init import det_init_

from util import rel_rms, seeded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def make_classifier():
    clf = Classifier(num_labels=7, base_channels=32)
    det_init_(clf.state_dict().items())
    clf.eval()
    return clf


@pytest.mark.parametrize("precision,tol", [("fp32", 2e-4), ("fp16", 8e-3)])
def test_features_through_the_head_match_reference_logits(golden, precision, tol):
    z = golden("f9_classifier32")
    dev = torch.device("cuda:0")
    clf = make_classifier().to(dev)
    clf.set_precision(precision)
    x = seeded((2, 1, 64000), int(z["x_seed"])).to(dev)
    ts = torch.from_numpy(z["ts"]).to(dev)
    feat = clf.features(x, ts)
    assert feat.shape == (2, 512) and feat.dtype == torch.float32
    with torch.no_grad():
        logits = clf.out(feat).cpu()
    assert rel_rms(logits, torch.from_numpy(z["logits"])) < tol


def test_features_against_the_oracle_stem():
    """out.1 = identity: the oracle's classifier returns gelu(feat), the reference's stem output through the head's GELU."""
    dev = torch.device("cuda:0")
    clf = make_classifier()
    sd = {k: v.detach().clone() for k, v in clf.state_dict().items()}
    Fd = clf.feature_dim
    sd["out.1.weight"] = torch.eye(Fd)
    sd["out.1.bias"] = torch.zeros(Fd)
    x = seeded((2, 1, 64000), 11)
    ts = torch.tensor([0.0, 0.37])
    want = ref_cpu.classifier(sd, 32, x, ts)
    clf = clf.to(dev)
    got = F.gelu(clf.features(x.to(dev), ts.to(dev))).cpu()
    assert rel_rms(got, want) < 1e-5


def test_features_entry_is_consistent_with_forward():
    dev = torch.device("cuda:0")
    clf = make_classifier().to(dev)
    x = seeded((8, 1, 64000), 12).to(dev)
    ts = torch.zeros(8, device=dev)
    feat, logits, probs = clf.features(x, return_logits=True, return_probs=True)  # (ts=None: t = 0)
    assert torch.equal(logits, clf(x, ts))
    assert torch.equal(feat, clf.features(x, ts))
    assert (probs - torch.softmax(logits, dim=-1)).abs().max().item() < 1e-6
    assert (probs.sum(-1) - 1).abs().max().item() < 1e-6
    for B in (1, 3):
        assert torch.equal(clf.features(x[:B]), feat[:B]), B
    # forward and guidance are untouched by the new outputs
    labels = torch.arange(8, device=dev) % 7
    grad, logits2 = clf.log_prob_grad(x, ts, labels, 1.0, return_logits=True)
    assert torch.equal(logits2, logits) and torch.isfinite(grad).all()


def accumulate(x32, dev, batch=64):
    st = FeatureStats(x32.shape[1], dev)
    for b in range(0, x32.shape[0], batch):
        st.update(torch.from_numpy(x32[b:b + batch]).to(dev))
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("F_,offset", [(40, 0.0), (512, 0.0), (4096, 0.0), (40, 1e3), (512, 1e3)])
def test_moments_kernel_against_numpy(F_, offset):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(F_)
    x32 = (rng.standard_normal((1000, F_)) * rng.uniform(0.2, 2.0, F_) + rng.standard_normal(F_) + offset).astype(np.float32)
    st = accumulate(x32, dev)  # batches of 64, the last one 40 rows
    x = x32.astype(np.float64)
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)  # noqa: E731
    assert st.n == 1000
    assert rel(st.mean(), x.mean(0)) <= 1e-12
    cov = st.cov()
    assert np.array_equal(cov, cov.T)
    assert rel(cov, np.cov(x, rowvar=False)) <= 1e-12
    again = accumulate(x32, dev)
    for a, b in zip(st.moments()[1:], again.moments()[1:]):
        assert np.array_equal(a, b)


def test_moments_kernel_small_batches_and_odd_width():
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(9)
    x32 = rng.standard_normal((7, 77)).astype(np.float32)
    st = FeatureStats(77, dev)
    for b in range(7):  # one row per call
        st.update(torch.from_numpy(x32[b:b + 1]).to(dev))
    x = x32.astype(np.float64)
    assert np.linalg.norm(st.cov() - np.cov(x, rowvar=False)) <= 1e-12 * np.linalg.norm(np.cov(x, rowvar=False))


def write_checkpoints(tmp_path):
    m = DiffusionModel("unet", 32)
    det_init_(m.state_dict().items())
    ck = str(tmp_path / "d.pt")
    m.save(ck)
    cck = str(tmp_path / "c.pt")
    make_classifier().save(cck)
    return ck, cck


def test_inline_stats_equal_stat_generate_on_the_written_files(tmp_path):
    import sample_diffusion
    import stat_generate

    ck, cck = write_checkpoints(tmp_path)
    out, a, b = str(tmp_path / "s"), str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    sample_diffusion.main(["--checkpoint-path", ck, "--sample-steps", "3", "--batch-size", "4", "--num-samples", "6", "--sample-path", out,
                           "--seed", "3", "--stats-classifier", cck, "--stats-path", a])
    assert len(os.listdir(out)) == 6
    stat_generate.main(["--checkpoint-path", cck, "--sample-dir", out, b])
    za, zb = np.load(a), np.load(b)
    for k in ("mean", "cov"):
        assert np.abs(za[k] - zb[k]).max() <= 1e-10 * max(np.abs(zb[k]).max(), 1e-30), k
    assert za["probs"].shape == (6, 7)
    assert abs(float(za["class_score"]) - float(zb["class_score"])) <= 1e-12 * float(zb["class_score"])
    key = lambda p: sorted(map(tuple, np.round(p.astype(np.float64), 7)))  # noqa: E731
    assert key(za["probs"]) == key(zb["probs"])
    assert frechet_distance(za["mean"], za["cov"], zb["mean"], zb["cov"]) <= 1e-6 * np.trace(zb["cov"])


def test_stat_generate_two_ranks_equal_one(tmp_path):
    import sample_diffusion

    ck, cck = write_checkpoints(tmp_path)
    out = str(tmp_path / "s")
    sample_diffusion.main(["--checkpoint-path", ck, "--sample-steps", "2", "--batch-size", "5", "--num-samples", "5", "--sample-path", out,
                           "--seed", "4"])
    env = dict(os.environ, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    one, two = str(tmp_path / "one.npz"), str(tmp_path / "two.npz")
    script = os.path.join(ROOT, "stat_generate.py")
    r = subprocess.run([sys.executable, script, "--checkpoint-path", cck, "--batch-size", "2", "--sample-dir", out, one],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29553", script, "--dist-backend", "gloo", "--checkpoint-path", cck, "--batch-size", "2",
                        "--sample-dir", out, two], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("classifier score:") == 1
    z1, z2 = np.load(one), np.load(two)
    for k in ("mean", "cov"):
        assert np.abs(z1[k] - z2[k]).max() <= 1e-12 * max(np.abs(z1[k]).max(), 1e-30), k
    assert np.array_equal(z1["probs"], z2["probs"])
    assert abs(float(z1["class_score"]) - float(z2["class_score"])) <= 1e-12 * float(z1["class_score"])
