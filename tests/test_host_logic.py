"""CPU-side checks: the C-ABI library loads and exports every declared symbol, the parameter table equals
the reference's state-dict layout, checkpoints round-trip, error behaviour, sharding logic (gloo, world 2)."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from vq_voice_swap_amd import DiffusionModel, VQVAE, _native
from vq_voice_swap_amd.sampler import shard_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(lib_built):
    header = open(os.path.join(ROOT, "include", "vqvs.h")).read()
    declared = set(re.findall(r"\b(vqvs_[a-z0-9_]+)\s*\(", header))
    declared -= {"vqvs_model", "vqvs_cfg"}
    assert declared, "no declarations found"
    for sym in sorted(declared):
        assert hasattr(lib_built, sym), f"libvqvs_hip.so does not export {sym}"
    assert set(_native.EXPORTS) <= declared | {"vqvs_last_error", "vqvs_version"}
    assert b"gfx950" in lib_built.vqvs_version()


def test_param_table_is_the_reference_state_dict(lib_built):
    m = DiffusionModel("unet", 32, num_labels=3, dropout=0.1)
    sd = m.predictor.state_dict()
    table = _native.param_table(m.predictor._cfg())
    assert [n for n, _ in table] and set(n for n, _ in table) == set(sd.keys())
    assert all(tuple(sd[n].shape) == s for n, s in table)
    assert "down_blocks.0.post_cond.2.weight" in sd  # dropout checkpoints keep the conv at index 2 (unet.py:295-300)
    v = VQVAE(base_channels=32, pred_name="unet", num_labels=5)
    keys = list(v.state_dict().keys())
    assert "vq.dictionary" in keys and "vq.usage_count" in keys and "encoder.blocks.25.pre_cond.2.weight" in keys
    assert v.cond_channels == 512 and v.save_kwargs()["enc_name"] == "unet"


def test_open_topology_param_tables(lib_built):
    """channel_mult / depth_mult / middle_dilations / out_dilations other than the defaults (reference unet.py:17-30, 188-196): the
    library's parameter table is the module's state dict (whose keys and shapes are the reference's, fixture F14 is made with
    them), the downsample rate follows the level count, and what cannot be built is refused with the reason."""
    from vq_voice_swap_amd import UNetEncoder, UNetPredictor

    for kw in (dict(channel_mult=(1, 2, 2, 4), middle_dilations=(1, 6), depth_mult=1, num_labels=3),
               dict(channel_mult=(1, 1, 2), middle_dilations=(), depth_mult=3),
               dict(channel_mult=(1, 4, 8, 8, 16), middle_dilations=(2, 32, 5), depth_mult=2, cond_channels=64)):
        m = UNetPredictor(32, **kw)
        sd = m.state_dict()
        table = _native.param_table(m._cfg())
        assert len(table) == len(sd) and set(n for n, _ in table) == set(sd.keys()), kw
        assert all(tuple(sd[n].shape) == s for n, s in table)
        assert m.downsample_rate == 2 ** (len(kw["channel_mult"]) - 1)
    for kw in (dict(channel_mult=(1, 2, 4), out_dilations=(2, 8), depth_mult=1, out_channels=64),
               dict(channel_mult=(1, 1, 2, 2, 4, 4), out_dilations=(), depth_mult=3, out_channels=96)):
        m = UNetEncoder(32, **kw)
        sd = m.state_dict()
        table = _native.param_table(m._cfg())
        assert len(table) == len(sd) and set(n for n, _ in table) == set(sd.keys()), kw
        assert all(tuple(sd[n].shape) == s for n, s in table)
    # the default topology does not set the fields at all (old cfg structs keep working)
    assert UNetPredictor(32)._cfg().topology_set == 0 and UNetEncoder(32)._cfg().topology_set == 0
    for bad in (dict(channel_mult=(1, 1.5)), dict(channel_mult=(1, 64)), dict(depth_mult=0), dict(middle_dilations=(64,)), dict(channel_mult=(2, 2)),
                dict(channel_mult=tuple([1] * 13))):
        with pytest.raises(ValueError):
            UNetPredictor(32, **bad)  # widths not multiples of 32 / beyond 1024 / depth / dilation range / head width / level count
    cfg = UNetPredictor(32)._cfg()
    cfg.topology_set, cfg.n_levels = 1, 0
    assert lib_built.vqvs_param_count(cfg) < 0 and b"n_levels" in lib_built.vqvs_last_error()
    # the builder's limits hold for every caller of the C ABI, not only behind the Python wrappers (include/vqvs.h, vqvs_cfg):
    # a predictor whose first level is wider than base_channels (the output head is built for base_channels) ...
    cfg = UNetPredictor(32)._cfg()
    cfg.set_topology((2, 2), 2, ())
    assert lib_built.vqvs_param_count(cfg) < 0 and b"channel_mult[0]" in lib_built.vqvs_last_error()
    # ... and a classifier whose final width is neither <= 64 nor a multiple of 64 (attention heads of 64 channels)
    cfg = _native.Cfg()
    cfg.kind, cfg.base_channels, cfg.in_channels, cfg.out_channels, cfg.num_labels = _native.KIND_CLASSIFIER, 32, 1, 1, 5
    cfg.set_topology((1, 3), 2, ())
    assert lib_built.vqvs_param_count(cfg) < 0 and b"multiple of 64" in lib_built.vqvs_last_error()
    cfg.set_topology((1, 4), 2, ())
    assert lib_built.vqvs_param_count(cfg) > 0


def test_checkpoint_roundtrip(tmp_path, lib_built):
    m = DiffusionModel("unet", 32, num_labels=4)
    p = str(tmp_path / "m.pt")
    m.save(p)
    state = torch.load(p, map_location="cpu")
    assert set(state.keys()) == {"kwargs", "state_dict"}  # reference format, base.py:74-82
    m2 = DiffusionModel.load(p)
    for (k1, v1), (k2, v2) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
    # old checkpoints stored dropout as a 1-tuple (diffusion_model.py:30-31)
    assert DiffusionModel("unet", 32, dropout=(0.0,)).dropout == 0.0


def test_errors_mirror_the_reference(lib_built):
    m = DiffusionModel("unet", 32, num_labels=4)
    x, ts = torch.zeros(1, 1, 256), torch.zeros(1)
    with pytest.raises(AssertionError, match="must provide labels"):
        m.predictor(x, ts)
    with pytest.raises(AssertionError, match="must provide cond"):
        m.predictor(x, ts, cond=torch.zeros(1, 512, 1), labels=torch.zeros(1).long())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predictor(x, ts, labels=torch.zeros(1).long())
    with pytest.raises(ValueError, match="unknown schedule"):
        DiffusionModel("unet", 32, schedule_name="nope")
    with pytest.raises(ValueError, match="unknown predictor"):
        DiffusionModel("nope", 32)
    cfg = _native.Cfg()
    cfg.kind, cfg.base_channels, cfg.in_channels, cfg.out_channels = 0, 48, 1, 1
    with pytest.raises(ValueError):
        _native.param_table(cfg) and _native.check(-1)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        _native.lib()


def test_shard_ranges_cover_exactly():
    for n in (0, 1, 7, 64, 511, 512):
        for w in (1, 2, 3, 8):
            spans = [shard_range(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [e - b for b, e in spans]
            assert max(sizes) - min(sizes) <= 1


WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, {root!r})
from vq_voice_swap_amd.sampler import sample_clips, shard_range
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
T, n_total = 512, 5
def fake(begin, end, seed):   # a "sampler" whose output depends only on the GLOBAL clip index
    return torch.stack([torch.full((1, T), float(seed * 1000 + i)) for i in range(begin, end)]) if end > begin else torch.empty(0, 1, T)
out = sample_clips(None, n_total, T, steps=3, seed=7, sample_fn=fake)
if rank == 0:
    assert out.shape == (n_total, 1, T), out.shape
    assert [int(v) for v in out[:, 0, 0].tolist()] == [7000 + i for i in range(n_total)]
    print("GATHER_OK")
else:
    assert out is None
dist.destroy_process_group()
"""


def test_two_rank_gather_gloo(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(WORKER.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29531", str(script)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "GATHER_OK" in r.stdout


def test_plain_c_client_of_the_abi(tmp_path, lib_built):
    """examples/abi_info.c: the header is self-contained C and the host-side entry points work without torch."""
    import numpy as np

    exe = str(tmp_path / "abi_info")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "abi_info.c"),
                    "-ldl", "-o", exe], check=True)
    out = subprocess.run([exe, _native.LIB_PATH, "32"], check=True, capture_output=True, text=True).stdout
    cfg = _native.Cfg()
    cfg.kind, cfg.base_channels, cfg.in_channels, cfg.out_channels, cfg.max_batch, cfg.max_T = 0, 32, 1, 1, 1, 256
    table = _native.param_table(cfg)
    assert f"{len(table)} parameters" in out and "time_embed.proj.weight" in out
    assert f"total {sum(int(np.prod(s)) for _, s in table)} float32 values" in out


def _run_bench(args, env_extra, timeout=300):
    import subprocess

    env = dict(os.environ, VQVS_BENCH_BACKEND="gloo", OMP_NUM_THREADS="2", **env_extra)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=timeout)


def test_bench_gpus_n_launches_n_ranks():
    """`python bench.py --gpus 2` with no torchrun environment must start two ranks itself (re-exec under
    torch.distributed.run) and only report when the process group really has two ranks.  Run here up to process-group
    initialisation on gloo (`--init-only`); on a GPU box the same path continues into the RCCL benchmark."""
    r = _run_bench(["--gpus", "2", "--init-only"], {})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out == {"init_only": True, "world_size": 2, "backend": "gloo", "allreduce_ok": True}


def test_bench_refuses_world_size_mismatch():
    """Launched with 2 ranks but asked to report 3 GPUs: no JSON line, non-zero exit."""
    import subprocess

    from bench import free_port

    env = dict(os.environ, VQVS_BENCH_BACKEND="gloo", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "3", "--init-only"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")], r.stdout
    assert "refusing to report" in r.stderr


def test_bench_dump_outputs_sample(tmp_path, monkeypatch):
    """--dump-outputs: float32 clips as they are while they fit the budget, else a fixed, seeded sample of whole clips in clip order."""
    import numpy as np

    import bench

    x = torch.randn(10, 1, 100, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "all"), x)
    y = np.load(tmp_path / "all" / "x0.npy")
    assert y.dtype == np.float32 and np.array_equal(y, x.float().numpy())
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 100 * 4)
    samples = []
    for tag in ("a", "b"):
        bench.dump_outputs(str(tmp_path / tag), x)
        samples.append(np.load(tmp_path / tag / "x0.npy"))
        assert os.path.getsize(tmp_path / tag / "x0.npy") <= 3 * 100 * 4 + 128
    assert samples[0].shape == (3, 1, 100) and np.array_equal(samples[0], samples[1])
    rows = [int(np.flatnonzero((y == s).all(axis=(1, 2)))[0]) for s in samples[0]]
    assert rows == sorted(set(rows))


def test_weight_snapshot_token_and_copies(lib_built):
    """The device snapshot key follows in-place parameter updates (the reference reads live parameters), and
    modules deep-copy / pickle without a handle; index validation raises like nn.Embedding."""
    import copy
    import pickle

    m = DiffusionModel("unet", 32)
    p = m.predictor
    t0 = p._weights_token()
    assert p._weights_token() == t0
    with torch.no_grad():
        p.out[1].bias.add_(1.0)
    t1 = p._weights_token()
    assert t1 != t0
    src = DiffusionModel("unet", 32)
    m.load_from_pretrained(src)
    assert p._weights_token() != t1
    c = copy.deepcopy(m)
    assert c.predictor._handle is None and torch.equal(c.predictor.out[1].bias, p.out[1].bias)
    assert pickle.loads(pickle.dumps(p)).base_channels == 32
    with pytest.raises(IndexError):
        _native.check_index_range(torch.tensor([0, 5]), 5, "labels")
    with pytest.raises(IndexError):
        _native.check_index_range(torch.tensor([-1]), 5, "labels")
    _native.check_index_range(torch.tensor([0, 4]), 5, "labels")
    # eval-only guard: dropout in training mode is refused, not silently ignored
    d = DiffusionModel("unet", 32, dropout=0.1)
    d.train()
    with pytest.raises(RuntimeError, match="dropout"):
        d.predictor._check_inference_only(torch.zeros(1))


def test_padded_width_parameter_tables(lib_built):
    """Widths that are not multiples of 32 (the reference takes any, unet.py:17-30): the handle is built at the padded physical width
    (csrc/net.cpp pad_map) and the module's real-width parameters are spread into its table block by block -- every value kept, every
    pad position zero, FiLM's (a | b) halves and concatenated inputs included."""
    from vq_voice_swap_amd import UNetEncoder, UNetPredictor
    from vq_voice_swap_amd.unet import pad_blocks, pad_state, physical_base

    assert [physical_base(b) for b in (48, 40, 24, 20, 16, 8, 100, 36, 96, 150)] == [64, 64, 32, 32, 32, 32, 128, 64, 96, 256]
    m = UNetPredictor(48, channel_mult=(1, 2, 2), middle_dilations=(4,), depth_mult=1, num_labels=3, cond_channels=64)
    cfg = m._cfg()
    assert (cfg.base_channels, cfg.reserved[4]) == (64, 48) and m.base_channels == 48
    table, sd = _native.param_table(cfg), m.state_dict()
    assert set(n for n, _ in table) == set(sd.keys())
    q, qp = pad_blocks(48)
    ps = pad_state(sd, table, q, qp)
    for n, shape in table:
        assert tuple(ps[n].shape) == shape, n
        assert torch.equal(ps[n].abs().sum().double(), sd[n].detach().abs().sum().double()) or abs(float(ps[n].abs().sum() - sd[n].abs().sum())) < 1e-3, n
    w, pw = sd["up_blocks.0.pre_cond.2.weight"].detach(), ps["up_blocks.0.pre_cond.2.weight"]  # [96][96 + 96 concatenated][3] -> [128][256][3]
    assert torch.equal(pw[4 * 5 + 1, 4 * 40 + 2], w[3 * 5 + 1, 3 * 40 + 2]) and float(pw[3::4].abs().sum()) == 0.0 and float(pw[:, 3::4].abs().sum()) == 0.0
    f, pf = sd["down_blocks.0.cond_layers.1.weight"].detach(), ps["down_blocks.0.cond_layers.1.weight"]  # FiLM rows (a | b), columns = the embedding
    assert torch.equal(pf[64 + 4 * 2 + 1, 4 * 7], f[48 + 3 * 2 + 1, 3 * 7])
    e = UNetEncoder(40, channel_mult=(1, 2, 4), depth_mult=1, out_channels=64)
    assert (e._cfg().base_channels, e._cfg().reserved[4]) == (64, 40)
    assert UNetPredictor(64)._cfg().reserved[4] == 0 and UNetPredictor(96)._cfg().reserved[4] == 0
    with pytest.raises(ValueError, match="builds up to 256"):
        UNetPredictor(300)


def test_few_step_promotion_finds_the_native_modules(lib_built):
    """Diffusion.ddpm_sample promotes a guided run of fewer than FEW_GUIDED_STEPS steps to the fp32 mode: it has to find the native
    modules behind whatever callables it is given -- the module itself, UNetPredictor.condition's partial, a bound method, the
    guidance closures of Classifier / EncoderPredictor -- and nothing behind a plain function."""
    from vq_voice_swap_amd import Classifier, EncoderPredictor, UNetPredictor
    from vq_voice_swap_amd.diffusion import FEW_GUIDED_STEPS, _native_modules

    p = UNetPredictor(32, num_labels=3)
    clf = Classifier(num_labels=3, base_channels=32)
    ep = EncoderPredictor(base_channels=32, downsample_rate=256, num_latents=8, bottleneck_dim=32)
    assert FEW_GUIDED_STEPS == 10
    assert _native_modules(p) == [p]
    assert _native_modules(p.condition(labels=torch.zeros(1, dtype=torch.long))) == [p]
    assert _native_modules(p.forward) == [p]
    assert _native_modules(clf.guidance_fn(torch.zeros(1, dtype=torch.long), 2.0)) == [clf]
    assert _native_modules(ep.guidance_fn(torch.zeros(1, 4, dtype=torch.long), 1.0)) == [ep]
    assert _native_modules(lambda x, ts: x) == []


def test_the_four_sampling_loops_walk_one_sequence(monkeypatch):
    """`ddpm_sample`, `ddim_sample` and their window forms on CPU tensors, with the device check and the kernel seams (`_step`,
    `_ddim_step`, `_keep_`, `longform._*_step_windows`, `longform.keep_windows_`) replaced by recording stubs: every loop walks steps
    start_step .. steps - 1, shows the predictor row i of the t table, passes no noise on the last step (and none at eta = 0) and
    noise_scale 0 there alone, re-applies the keep region with index i + 1 at the alpha_bar stepped to, and checks `source` / `keep`
    once.  A guided run of 3 steps in a 2-byte mode enters the fp32 override once and runs its 3 steps once, inside it."""
    import contextlib
    import warnings

    from vq_voice_swap_amd import diffusion as dmod, longform
    from vq_voice_swap_amd.diffusion import Diffusion, make_schedule

    steps, n, W, H = 5, 3, 8, 4
    Np = (n - 1) * H + W
    d = Diffusion(make_schedule("exp"))
    log = []
    monkeypatch.delenv("VQVS_FEW_STEP_PROMOTE", raising=False)
    monkeypatch.setattr(_native, "require_cuda", lambda *tensors: None)
    monkeypatch.setattr(_native, "_stream_ptr", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    real_check = dmod.check_keep_args
    monkeypatch.setattr(dmod, "check_keep_args", lambda *a: (log.append(("check",)), real_check(*a))[1])

    def clip_step(x_t, eps, a_t, a_to, ts, **kw):
        assert torch.equal(eps, 0.5 * x_t)
        log.append(("step", kw["step_index"], a_t, a_to, kw["noise"], kw["noise_scale"], kw["cond_fn"]))
        return x_t + 1

    def windows_step(rule, x, eps, grad, nz, a_t, a_to, x_to, next_windows, n_, window, hop, noise_scale, seed, clip_offset, step_index, st):
        assert (n_, window, hop, seed, clip_offset) == (n, W, H, 7, 3) and torch.equal(eps, 0.5 * longform.gather_windows(x, W, H))
        log.append(("step", step_index, a_t, a_to, nz, noise_scale, None))
        x_to.copy_(x + 1)
        next_windows.copy_(longform.gather_windows(x_to, W, H))

    def guided_fill(rule, xw, e, tables, i, b0, cond_fn, eps, grad, st):
        eps[b0:b0 + xw.shape[0]].copy_(e)
        cond_fn(xw, tables[3][i, :xw.shape[0]], first=b0)

    def keep_stub(*args, **kw):
        assert (kw["seed"], kw["clip_offset"]) == (7, 3)
        if args[-2] is None:  # (x, [windows,] source, keep, alpha) at a later start: the call writes EVERY sample of a state that is
            args[0].copy_(args[-3])  # uninitialised memory until then
        log.append(("keep", kw["index"], args[-1]))

    monkeypatch.setattr(d, "_step", clip_step)
    monkeypatch.setattr(d, "_ddim_step", clip_step)
    monkeypatch.setattr(d, "_keep_", keep_stub)
    monkeypatch.setattr(longform, "_ddpm_step_windows", windows_step)
    monkeypatch.setattr(longform, "_ddim_step_windows", windows_step)
    monkeypatch.setattr(longform, "keep_windows_", keep_stub)

    def predictor(x, ts, first=0):
        log.append(("pred", ts.clone(), first))
        return 0.5 * x

    clips, long = dict(x=torch.zeros(2, 1, 8), firsts=[0]), dict(x=torch.zeros(1, 1, Np), firsts=[0, 2], window=W, hop=H, window_batch=2)
    loops = [("ddpm_sample", d.ddpm_sample, clips, {}, True), ("ddim_sample", d.ddim_sample, clips, dict(eta=0.0), False),
             ("ddim_sample", d.ddim_sample, clips, dict(eta=0.5), True),
             ("ddpm_sample_windows", lambda *a, **kw: longform.ddpm_sample_windows(d, *a, **kw), long, {}, True),
             ("ddim_sample_windows", lambda *a, **kw: longform.ddim_sample_windows(d, *a, **kw), long, dict(eta=0.0), False),
             ("ddim_sample_windows", lambda *a, **kw: longform.ddim_sample_windows(d, *a, **kw), long, dict(eta=0.5), True)]
    ts_all, a_t_all, a_to_all, _ = d.step_tables(steps, 2, None, torch.device("cpu"))  # two rows: the clips, or the windows of a slice
    for name, call, group, rule_kw, noisy in loops:
        x_T = group["x"]
        layout_kw = {k: v for k, v in group.items() if k not in ("x", "firsts")}
        noise = [torch.full_like(x_T, float(i)) for i in range(steps)]
        source, keep = torch.ones_like(x_T), torch.zeros_like(x_T, dtype=torch.bool)
        keep[..., 3:6] = True
        for start in (0, 2):
            del log[:]
            out = call(x_T, predictor, steps, noise=noise, seed=7, clip_offset=3, source=source, keep=keep, start_step=start,
                       **layout_kw, **rule_kw)
            assert out.shape == x_T.shape, name
            assert log[0] == ("check",) and [e[0] for e in log].count("check") == 1, name
            assert log[1][:2] == ("keep", start) and torch.equal(log[1][2], a_t_all[start]), name  # the start state, at a_t[start]
            per_step = len(group["firsts"]) + 2
            assert len(log) == 2 + per_step * (steps - start), (name, len(log))
            for k, i in enumerate(range(start, steps)):
                entries = log[2 + per_step * k:2 + per_step * (k + 1)]
                preds, step, kept = entries[:-2], entries[-2], entries[-1]
                for first, p in zip(group["firsts"], preds):
                    assert p[0] == "pred" and p[2] == first and torch.equal(p[1], ts_all[i, :p[1].numel()]), (name, i)
                last = i + 1 == steps
                assert step[:2] == ("step", i) and torch.equal(step[2], a_t_all[i]) and torch.equal(step[3], a_to_all[i]), (name, i)
                assert step[5] == (0.0 if last else 1.0), (name, i)
                if last or not noisy:
                    assert step[4] is None, (name, i)
                else:
                    assert torch.equal(step[4].reshape(-1), noise[i].reshape(-1)), (name, i)
                assert kept[:2] == ("keep", i + 1) and torch.equal(kept[2], a_to_all[i]), (name, i)

    # a guided run of 3 steps in a 2-byte mode: one entry into the fp32 override, the loop run once, inside it
    class HalfPredictor:
        precision, entered, inside = "fp16", 0, False

        @contextlib.contextmanager
        def precision_override(self, mode):
            assert mode == "fp32"
            self.entered, self.inside = self.entered + 1, True
            try:
                yield
            finally:
                self.inside = False

        def check_status(self):
            log.append(("status", self.inside))

        def __call__(self, x, ts, first=0):
            assert self.inside
            return predictor(x, ts, first)

    def cond_fn(x, ts, first=0):
        log.append(("cond", first))
        return 0.1 * x

    monkeypatch.setattr(longform, "_ddpm_fill", guided_fill)
    for name, call, group, rule_kw, _ in loops:
        half = HalfPredictor()
        layout_kw = {k: v for k, v in group.items() if k not in ("x", "firsts")}
        del log[:]
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            call(group["x"], half, 3, cond_fn=cond_fn, seed=7, clip_offset=3, **layout_kw, **rule_kw)
        promoted = [w for w in rec if "run in the fp32" in str(w.message)]
        assert len(promoted) == 1 and promoted[0].category is RuntimeWarning and name + ":" in str(promoted[0].message), name
        assert promoted[0].filename == __file__, (name, promoted[0].filename)  # the warning points at the caller of the entry point
        assert half.entered == 1 and not half.inside, name
        assert [e[1] for e in log if e[0] == "step"] == [0, 1, 2] and [e[0] for e in log].count("check") == 1, name
        assert log[-1] == ("status", True), name  # the final guard runs on the promoted handle
        if group is long:
            assert [e for e in log if e[0] == "cond"] == [("cond", 0), ("cond", 2)] * 3, name
        else:
            assert all(e[6] is cond_fn for e in log if e[0] == "step"), name
