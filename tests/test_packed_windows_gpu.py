"""Packed window steps and corpus conversion on the device.  Everything here is bit for bit (`torch.equal`): a recording of a pack is
what the single-recording entry point, loop, model call or script gives for it alone at clip + r."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vq_voice_swap_amd import VQVAE, _native
from vq_voice_swap_amd.audio import ChunkWriter
from vq_voice_swap_amd.det_init import det_init_
from vq_voice_swap_amd.diffusion import Diffusion, make_schedule
from vq_voice_swap_amd.longform import pack_layout, plan_pack

from util import seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, CLIP, STEP = (1 << 32) + 7, (1 << 32) + 5, 3
# (W, H, counts): a 64-lane wave spans two recordings; a 256-thread block does; V = 0; recordings cross chunk (4096) and block
# boundaries with a one-window recording between longer ones; many table entries
SHAPES = [(128, 64, (1, 1, 2, 1, 3)), (512, 256, (1, 3, 2)), (512, 512, (2, 1, 2)), (4352, 2304, (3, 1, 2)),
          (512, 256, tuple(itertools.islice(itertools.cycle((1, 2, 1, 3)), 40)))]
IDS = ["wave-spans-two", "block-spans-two", "no-overlap", "chunks-and-blocks", "forty-recordings"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def scalar(v, dev):
    return torch.tensor([float(v)], dtype=torch.float32, device=dev)


def guarded(size, dev):
    return torch.full((size + 64,), float("nan"), device=dev)


def unguard(buf, size):
    assert torch.isnan(buf[size:]).all(), "the kernel wrote past the end of an output"
    assert torch.isfinite(buf[:size]).all(), "the kernel left elements unwritten (or wrote non-finite values)"
    return buf[:size]


class Pack:
    """The geometry and inputs of one pack; `rows(r)` / `wins(r)` slice a long / a window array down to recording r."""

    def __init__(self, W, H, counts, dev, seed=11):
        self.W, self.H, self.counts, self.R = W, H, list(counts), len(counts)
        self.first, self.offsets, self.total = pack_layout(counts, W, H)
        self.N = self.first[-1]
        self.d_first = torch.tensor(self.first, dtype=torch.int32, device=dev)
        self.x, self.noise, self.prev = (seeded((self.total,), seed + i).to(dev) for i in (0, 2, 4))
        self.eps, self.grad = (seeded((self.N, W), seed + i).to(dev) for i in (1, 3))

    def rows(self, t, r):
        return None if t is None else t[self.offsets[r]:self.offsets[r] + self.counts[r] * self.H + self.W - self.H]

    def wins(self, t, r):
        return None if t is None else t[self.first[r]:self.first[r + 1]]


def call(name, p, geom, x, eps, grad, noise, prev, a, *, flags, eta, noise_scale, clip, want_windows, Np, NW):
    """One call of the single (`geom` = (n,)) or packed (`geom` = (d_first, R)) form of sampler `name` -> (x_to, windows, x0)."""
    L, st, dev = _native.lib(), _native._stream_ptr(), x.device
    out, win = guarded(Np, dev), guarded(NW, dev) if want_windows else None
    x0 = guarded(Np, dev) if name == "dpmpp" else None
    fn = getattr(L, f"vqvs_{name}_step_windows" + ("_packed" if len(geom) == 2 else ""))
    if name == "ddpm":
        rc = fn(x.data_ptr(), eps.data_ptr(), _native._ptr(noise), a[1].data_ptr(), a[2].data_ptr(), out.data_ptr(), _native._ptr(win), *geom,
                p.W, p.H, flags, noise_scale, SEED, clip, STEP, st)
    elif name == "ddim":
        rc = fn(x.data_ptr(), eps.data_ptr(), _native._ptr(grad), _native._ptr(noise), a[1].data_ptr(), a[2].data_ptr(), out.data_ptr(),
                _native._ptr(win), *geom, p.W, p.H, flags, eta, noise_scale, SEED, clip, STEP, st)
    else:
        rc = fn(x.data_ptr(), eps.data_ptr(), _native._ptr(grad), _native._ptr(prev), None if prev is None else a[0].data_ptr(), a[1].data_ptr(),
                a[2].data_ptr(), out.data_ptr(), x0.data_ptr(), _native._ptr(win), *geom, p.W, p.H, flags, st)
    _native.check(rc)
    return unguard(out, Np), None if win is None else unguard(win, NW).view(-1, p.W), None if x0 is None else unguard(x0, Np)


def packed_call(name, p, *, grad=False, noise=False, prev=False, **kw):
    return call(name, p, (p.d_first.data_ptr(), p.R), p.x, p.eps, p.grad if grad else None, p.noise if noise else None,
                p.prev if prev else None, kw.pop("a"), Np=p.total, NW=p.N * p.W, clip=CLIP, **kw)


def single_calls(name, p, *, grad=False, noise=False, prev=False, **kw):
    """The existing entry point, once per recording on that recording's slices at clip + r."""
    a = kw.pop("a")
    outs = []
    for r in range(p.R):
        n = p.counts[r]
        outs.append(call(name, p, (n,), p.rows(p.x, r), p.wins(p.eps, r).contiguous(), p.wins(p.grad, r) if grad else None,
                         p.rows(p.noise, r) if noise else None, p.rows(p.prev, r) if prev else None, a, Np=(n - 1) * p.H + p.W,
                         NW=n * p.W, clip=CLIP + r, **kw))
    return outs


def variants(name):
    """(label, keywords) of every variant of sampler `name` that the packed form is held to."""
    base = dict(flags=0, eta=0.0, noise_scale=1.0, want_windows=True)
    if name == "ddpm":
        for flags, given in itertools.product((0, 2, 3), (False, True)):
            yield f"flags={flags} noise given={given}", dict(base, flags=flags, noise=given)
        yield "noise_scale=0", dict(base, flags=2, noise_scale=0.0)
        yield "no windows", dict(base, flags=2, want_windows=False)
    elif name == "ddim":
        for eta, grad, given in itertools.product((0.0, 0.5, 1.0), (False, True), (False, True)):
            yield f"eta={eta} grad={grad} noise given={given}", dict(base, eta=eta, grad=grad, noise=given, flags=2 if grad == given else 0)
        yield "constrain, eta=1, grad", dict(base, eta=1.0, grad=True, flags=2)
        yield "noise_scale=0", dict(base, eta=1.0, flags=2, noise_scale=0.0)
        yield "no windows", dict(base, eta=0.5, flags=2, want_windows=False)
    else:
        for prev, grad, flags in itertools.product((False, True), (False, True), (0, 2)):
            yield f"history={prev} grad={grad} flags={flags}", dict(base, prev=prev, grad=grad, flags=flags)
        yield "no windows", dict(base, prev=True, flags=2, want_windows=False)


def alphas(dev):
    return scalar(0.22, dev), scalar(0.3, dev), scalar(0.37, dev)  # a_from < a_t < a_to: a usable history


def assert_pack_is_the_singles(p, got, singles, label):
    for r, one in enumerate(singles):
        for what, whole, alone, cut in (("x_to", got[0], one[0], p.rows), ("windows", got[1], one[1], p.wins), ("x0", got[2], one[2], p.rows)):
            assert (whole is None) == (alone is None), (label, what)
            if whole is not None:
                assert torch.equal(cut(whole, r), alone), f"{label}: {what} of recording {r} of {p.counts}"


# ---------------------------------------------------------------- 1. the packed step is the existing step, recording by recording
@pytest.mark.parametrize("name", ["ddpm", "ddim", "dpmpp"])
@pytest.mark.parametrize("W,H,counts", SHAPES, ids=IDS)
def test_packed_step_is_the_single_step_per_recording(dev, name, W, H, counts):
    p = Pack(W, H, counts, dev)
    a = alphas(dev)
    for label, kw in variants(name):
        got = packed_call(name, p, a=a, **kw)
        assert_pack_is_the_singles(p, got, single_calls(name, p, a=a, **kw), f"{name} {label}")


# ---------------------------------------------------------------- 2. R = 1
@pytest.mark.parametrize("name", ["ddpm", "ddim", "dpmpp"])
@pytest.mark.parametrize("W,H,n", [(512, 256, 1), (4352, 2304, 4), (512, 512, 3)])
def test_one_recording_is_the_existing_entry_point(dev, name, W, H, n):
    p = Pack(W, H, (n,), dev, seed=31)
    assert (p.first, p.total) == ([0, n], (n - 1) * H + W)
    a = alphas(dev)
    for label, kw in variants(name):
        got = packed_call(name, p, a=a, **kw)
        assert_pack_is_the_singles(p, got, single_calls(name, p, a=a, **kw), f"{name} {label}")


# ---------------------------------------------------------------- 3. nothing crosses a recording boundary
@pytest.mark.parametrize("name", ["ddpm", "ddim", "dpmpp"])
def test_no_blending_across_a_recording_boundary(dev, name):
    """The last window of recording r and the first of r + 1 are neighbours in the batch: changing eps (and grad) in the one leaves
    every sample of the other, and of every recording but r, as it was -- and does change recording r's overlap and tail."""
    p = Pack(512, 256, (2, 3, 1, 2), dev, seed=41)
    a = alphas(dev)
    kw = dict(a=a, flags=2, eta=0.5, noise_scale=1.0, want_windows=True, grad=name != "ddpm", prev=name == "dpmpp")
    before = packed_call(name, p, **kw)
    for r in range(p.R - 1):
        q = Pack(512, 256, p.counts, dev, seed=41)
        last = q.first[r + 1] - 1
        q.eps[last] += 1.0
        q.grad[last] -= 0.5
        after = packed_call(name, q, **kw)
        for other in range(p.R):
            for whole_b, whole_a, cut in ((before[0], after[0], p.rows), (before[1], after[1], p.wins), (before[2], after[2], p.rows)):
                if whole_b is None:
                    continue
                same = torch.equal(cut(whole_b, other), cut(whole_a, other))
                assert same == (other != r), (name, r, other)


# ---------------------------------------------------------------- 4. the sampling loops
def analytic_predictor(base, rec=None):
    """Depends on the window's own index base + first + row: `base` is the index of a recording's first window in its pack."""

    def predictor(w, ts, first):
        m = w.shape[0]
        index = (base + first + torch.arange(m, device=w.device)).to(torch.float32)
        if rec is not None:
            rec.append((first, m))
        return 0.5 * torch.sin(3 * w) + 0.1 * index.view(m, 1, 1)

    return predictor


def analytic_cond_fn(base):
    def cond_fn(x, ts, first):
        m = x.shape[0]
        index = (base + first + torch.arange(m, device=x.device)).to(torch.float32)
        return torch.tanh(x) * (ts + 0.1 * index).view(m, 1, 1)

    return cond_fn


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("method,kw", [("ddpm_sample_windows", dict(constrain=True)), ("ddpm_sample_windows", dict(sigma_large=True)),
                                       ("ddim_sample_windows", dict(eta=0.5, constrain=True)), ("ddim_sample_windows", dict(eta=0.0)),
                                       ("dpmpp_sample_windows", dict(constrain=True)), ("dpmpp_sample_windows", dict())])
def test_sample_windows_with_counts(dev, method, kw, guided):
    W, H, counts, steps, clip0 = 512, 256, (2, 1, 3), 4, 5
    first, offsets, total = pack_layout(counts, W, H)
    d = Diffusion(make_schedule("exp"))
    x_T = seeded((1, 1, total), 51).to(dev)
    sample = getattr(d, method)
    lengths = [(c - 1) * H + W for c in counts]
    for noise in (None, [seeded((1, 1, total), 60 + i).to(dev) for i in range(steps)]):
        runs = {}
        for wb in (64, 4, 1):
            rec = []
            runs[wb] = sample(x_T, analytic_predictor(0, rec), steps, window=W, hop=H, window_batch=wb, seed=9, clip_offset=clip0, noise=noise,
                              counts=counts, cond_fn=analytic_cond_fn(0) if guided else None, **kw)
            assert runs[wb].shape == (1, 1, total)
            m = min(wb, first[-1])
            assert rec == [(b, min(m, first[-1] - b)) for _ in range(steps) for b in range(0, first[-1], m)]  # slices run across recordings
        assert torch.equal(runs[64], runs[4]) and torch.equal(runs[64], runs[1])
        for r in range(len(counts)):
            sl = slice(offsets[r], offsets[r] + lengths[r])
            alone = sample(x_T[..., sl].contiguous(), analytic_predictor(first[r]), steps, window=W, hop=H, seed=9, clip_offset=clip0 + r,
                           noise=None if noise is None else [z[..., sl].contiguous() for z in noise],
                           cond_fn=analytic_cond_fn(first[r]) if guided else None, **kw)
            assert torch.equal(runs[64][..., sl], alone), (method, kw, guided, r)


def test_counts_must_match_the_state(dev):
    d = Diffusion(make_schedule("exp"))
    _, _, total = pack_layout((2, 1), 16, 12)
    with pytest.raises(ValueError, match="plan_pack"):
        d.ddpm_sample_windows(torch.zeros(1, 1, total + 4, device=dev), analytic_predictor(0), 4, window=16, hop=12, counts=(2, 1))
    with pytest.raises(ValueError):
        d.ddim_sample_windows(torch.zeros(1, 1, total, device=dev), analytic_predictor(0), 4, window=16, hop=12, counts=(2, 0))


# ---------------------------------------------------------------- 5. model level
def det_model(m):
    det_init_(m.state_dict().items())
    m.eval()
    return m


@pytest.fixture(scope="module")
def vqvae(dev):
    model = det_model(VQVAE(base_channels=32, pred_name="unet", num_labels=3)).to(dev)
    model.set_precision("fp32")
    return model


LENGTHS, W5, H5 = (5000, 2048, 300), 2048, 1536


@pytest.fixture(scope="module")
def waves(dev):
    return [(0.3 * seeded((1, 1, n), 71 + i)).clamp(-1, 1).to(dev) for i, n in enumerate(LENGTHS)]


@pytest.fixture(scope="module")
def alone(vqvae, waves, dev):
    """Per-wave `encode_long` codes, computed once; decodes are cached per (sampler, labels) by `decode_alone`."""
    return [vqvae.encode_long(w, W5, H5) for w in waves], {}


def decode_alone(vqvae, alone, sampler, labels):
    codes, cache = alone
    key = (sampler, tuple(labels))
    if key not in cache:
        cache[key] = [vqvae.decode_long(codes[r], torch.tensor([labels[r]], device=codes[r].device), num_samples=LENGTHS[r], window=W5, hop=H5,
                                        steps=3, constrain=True, seed=9, clip_offset=5 + r, sampler=sampler) for r in range(len(LENGTHS))]
    return cache[key]


def test_encode_long_batch(dev, vqvae, waves, alone):
    for wb in (2, 64):
        codes, counts = vqvae.encode_long_batch(waves, W5, H5, window_batch=wb)
        assert counts == [3, 1, 1] == plan_pack(LENGTHS, W5, H5)[0]
        assert codes.shape == (5, W5 // 256) and codes.dtype == torch.int64
        assert torch.equal(codes, torch.cat(alone[0]))


@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp"])
def test_decode_long_batch(dev, vqvae, waves, alone, sampler):
    codes, counts = vqvae.encode_long_batch(waves, W5, H5)
    kw = dict(counts=counts, num_samples=list(LENGTHS), window=W5, hop=H5, steps=3, constrain=True, seed=9, clip_offset=5, sampler=sampler)
    for labels in ([1], [2, 0, 1]):
        want = decode_alone(vqvae, alone, sampler, labels * 3 if len(labels) == 1 else labels)
        for wb in (2, 64):
            got = vqvae.decode_long_batch(codes, torch.tensor(labels, device=dev), window_batch=wb, **kw)
            assert [tuple(g.shape) for g in got] == [(1, 1, n) for n in LENGTHS]
            for r in range(len(LENGTHS)):
                assert torch.equal(got[r], want[r]), (sampler, labels, wb, r)
    per_window = torch.tensor([2, 2, 2, 0, 1], device=dev)  # one label per window says the same as one per recording
    got = vqvae.decode_long_batch(codes, per_window, window_batch=64, **kw)
    assert all(torch.equal(g, w) for g, w in zip(got, decode_alone(vqvae, alone, sampler, [2, 0, 1])))
    # whatever else is in the pack: the last two recordings alone, keyed by their own ids
    got = vqvae.decode_long_batch(codes[3:], torch.tensor([0, 1], device=dev), **dict(kw, counts=counts[1:], num_samples=list(LENGTHS[1:]), clip_offset=6))
    assert all(torch.equal(g, w) for g, w in zip(got, decode_alone(vqvae, alone, sampler, [2, 0, 1])[1:]))
    for bad in (dict(counts=[3, 1]), dict(num_samples=[5000, 2048, 3000]), dict(window=W5 + 4)):
        with pytest.raises(ValueError):
            vqvae.decode_long_batch(codes, torch.tensor([1], device=dev), **dict(kw, **bad))
    with pytest.raises(ValueError):
        vqvae.decode_long_batch(codes, torch.tensor([1, 2], device=dev), **kw)  # neither 1, R nor N labels


# ---------------------------------------------------------------- 6. the script
FILES = (("s1/a.wav", 8000), ("s1/c/b.wav", 3200), ("s2/a.wav", 800), ("s2/b.wav", 4800))  # 0.5 s, 0.2 s, 0.05 s, 0.3 s
WINDOW_FLAGS = ["--window-seconds", "0.128", "--overlap-seconds", "0.032", "--sample-steps", "3"]


def read_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_convert_dataset(dev, vqvae, tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import convert_dataset
    import sample_vqvae

    ck, data = str(tmp_path / "v.pt"), tmp_path / "data"
    vqvae.save(ck)
    sources = {}
    for i, (rel, n) in enumerate(FILES):
        os.makedirs(data / os.path.dirname(rel), exist_ok=True)
        sources[rel] = (0.3 * np.sin(np.arange(n) * (0.05 + 0.01 * i))).astype(np.float32)
        w = ChunkWriter(str(data / rel), 16000)
        w.write(sources[rel])
        w.close()
    rels = sorted(rel for rel, _ in FILES)
    assert rels == [rel for rel, _ in FILES]  # FILES is in id order

    def run(out, *flags):
        totals = convert_dataset.main([ck, str(data), str(tmp_path / out), "--seed", "9", *WINDOW_FLAGS, *flags])
        return [int(t) for t in totals], {rel: read_bytes(tmp_path / out / rel) for rel in rels if os.path.exists(tmp_path / out / rel)}

    totals2, small = run("out2", "--label", "2", "--pack-windows", "2", "--window-batch", "2")
    totals64, large = run("out64", "--label", "2", "--pack-windows", "64")
    assert sorted(small) == rels and small == large  # byte for byte, whatever the packs and the window batch
    windows = plan_pack([n for _, n in FILES], 2048, 1536)[0]
    assert windows == [5, 2, 1, 3]  # of 2048 every 1536
    assert totals2[:4] == totals64[:4] == [4, 0, sum(n for _, n in FILES), sum(windows)]
    assert totals64[4] == 1 and totals2[4] == 4  # 5 | 2 | 1 | 3 under a budget of 2: an oversized file is a pack of its own
    assert "4 files written, 0 skipped" in capsys.readouterr().out

    # two ranks (the packs dealt round-robin, one fresh process each): the same bytes, one line from rank 0
    from bench import free_port

    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    cmd = ["timeout", "-k", "10", "120", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "convert_dataset.py"), ck, str(data), str(tmp_path / "out2r"),
           "--seed", "9", *WINDOW_FLAGS, "--label", "2", "--pack-windows", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("files written") == 1 and "4 files written, 0 skipped" in r.stdout
    assert {rel: read_bytes(tmp_path / "out2r" / rel) for rel in rels} == large

    # the file with id 0 is what the single-file script writes for it
    one = str(tmp_path / "one.wav")
    sample_vqvae.main(["--label", "2", "--input-file", str(data / rels[0]), "--seed", "9", "--whole-file", *WINDOW_FLAGS, ck, one])
    assert read_bytes(one) == large[rels[0]]

    # --label-map: each directory to its label, against decode_long of every file on its own at its global id
    table = tmp_path / "targets.tsv"
    table.write_text("s1\t1\ns2\t0\n")
    _, mapped = run("outmap", "--label-map", str(table), "--pack-windows", "3")
    for i, rel in enumerate(rels):
        wave = torch.from_numpy(convert_dataset.read_wave(str(data / rel), "linear")).view(1, 1, -1).to(dev)
        codes = vqvae.encode_long(wave, 2048, 1536)
        label = torch.tensor([1 if rel.startswith("s1") else 0], device=dev)
        out = vqvae.decode_long(codes, label, num_samples=wave.shape[-1], window=2048, hop=1536, steps=3, constrain=True, seed=9, clip_offset=i)
        want = str(tmp_path / "want.wav")
        w = ChunkWriter(want, 16000)
        w.write(out.clamp(-1, 1).cpu().numpy().flatten())
        w.close()
        assert read_bytes(want) == mapped[rel], rel
    assert mapped[rels[0]] != large[rels[0]]  # label 1, not 2

    # --skip-existing: a finished run rewrites nothing; an interrupted one is completed with the files it would have written
    stamps = {rel: os.stat(tmp_path / "out64" / rel).st_mtime_ns for rel in rels}
    totals, again = run("out64", "--label", "2", "--pack-windows", "64", "--skip-existing")
    assert totals[0] == 0 and again == large
    assert stamps == {rel: os.stat(tmp_path / "out64" / rel).st_mtime_ns for rel in rels}
    os.remove(tmp_path / "out64" / rels[1])
    os.remove(tmp_path / "out64" / rels[2])
    totals, resumed = run("out64", "--label", "2", "--pack-windows", "64", "--skip-existing")
    assert totals[0] == 2 and resumed == large
    assert all(stamps[rel] == os.stat(tmp_path / "out64" / rel).st_mtime_ns for rel in (rels[0], rels[3]))
