"""Packed window steps and corpus conversion, host side: exports, declarations and argument checks of the three
`vqvs_*_step_windows_packed` entry points; `plan_pack`; the pack / rank / label-map bookkeeping of convert_dataset.py; the script's
flags; `counts=` against the keywords that are not built for a pack.  Nothing here needs a device."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

from vq_voice_swap_amd import _native
from vq_voice_swap_amd.corpus import deal_packs, list_files, make_packs, read_label_map
from vq_voice_swap_amd.diffusion import Diffusion, make_schedule
from vq_voice_swap_amd.longform import MAX_WINDOWS, pack_layout, plan_pack, plan_windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOM = ["const int32_t* d_first", "int R", "int W", "int H"]
DDPM_ARGS = ["const float* d_x", "const float* d_eps", "const float* d_noise", "const float* d_alpha_t", "const float* d_alpha_prev",
             "float* d_x_prev", "float* d_windows", *GEOM, "uint32_t flags", "float noise_scale", "uint64_t seed", "uint64_t clip",
             "uint32_t step_index", "void* stream"]
DDIM_ARGS = ["const float* d_x", "const float* d_eps", "const float* d_grad", "const float* d_noise", "const float* d_alpha_t",
             "const float* d_alpha_to", "float* d_x_to", "float* d_windows", *GEOM, "uint32_t flags", "float eta", "float noise_scale",
             "uint64_t seed", "uint64_t clip", "uint32_t step_index", "void* stream"]
DPMPP_ARGS = ["const float* d_x", "const float* d_eps", "const float* d_grad", "const float* d_x0_prev", "const float* d_alpha_from",
              "const float* d_alpha_t", "const float* d_alpha_to", "float* d_x_to", "float* d_x0_out", "float* d_windows", *GEOM,
              "uint32_t flags", "void* stream"]


def host_buffers(count, floats=64):
    bufs = [(C.c_float * floats)() for _ in range(count)]
    return bufs, [C.cast(b, C.c_void_p) for b in bufs]


# ---------------------------------------------------------------- 1. exports, declarations, refusals
def test_symbols_are_exported_and_declared(lib_built):
    header = open(os.path.join(ROOT, "include", "vqvs.h")).read()
    for name, want in (("vqvs_ddpm_step_windows_packed", DDPM_ARGS), ("vqvs_ddim_step_windows_packed", DDIM_ARGS),
                       ("vqvs_dpmpp_step_windows_packed", DPMPP_ARGS)):
        assert name in _native.EXPORTS and hasattr(lib_built, name)
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl, f"include/vqvs.h does not declare {name}"
        assert [a.strip() for a in " ".join(decl.group(1).split()).split(",")] == want
        assert len(getattr(lib_built, name).argtypes) == len(want)


# what every packed entry point refuses on (R, d_first, W, H): the rules of the single-recording form on W and H, R for n
BAD_GEOMETRY = (dict(R=0), dict(R=-1), dict(R=65536), dict(first=None),
                dict(W=18, H=12), dict(W=16, H=10), dict(W=0, H=0), dict(W=16, H=0), dict(W=-16, H=-12), dict(W=16, H=-4),
                dict(W=12, H=16), dict(W=28, H=12))


def test_ddpm_packed_refuses_bad_arguments_without_a_device(lib_built):
    """VQVS_ERR_ARG with host-only pointers, which a call that reached the device would fault on."""
    L = lib_built
    keep, (x, eps, noise, a_t, a_prev, out, win, first) = host_buffers(8)
    ok = dict(x=x, eps=eps, noise=noise, a_t=a_t, a_prev=a_prev, out=out, win=None, first=first, R=2, W=16, H=12, flags=2)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_ddpm_step_windows_packed(a["x"], a["eps"], a["noise"], a["a_t"], a["a_prev"], a["out"], a["win"], a["first"], a["R"],
                                               a["W"], a["H"], a["flags"], 1.0, 1, 2, 3, None)

    inside = C.c_void_p(x.value + 16)
    for bad in (dict(x=None), dict(eps=None), dict(a_t=None), dict(a_prev=None), dict(out=None), *BAD_GEOMETRY,
                dict(out=x), dict(out=inside), dict(noise=None, x=None), dict(win=win, R=0)):
        assert call(**bad) == -1, bad
        assert L.vqvs_last_error(), bad
    assert call(R=65536) == -1 and b"65535" in L.vqvs_last_error()
    assert call(R=0) == -1 and b"R=0" in L.vqvs_last_error()
    assert call(first=None) == -1 and b"first" in L.vqvs_last_error()
    assert call(W=28, H=12) == -1 and b"overlap" in L.vqvs_last_error()
    assert call(x=None) == -1 and b"non-NULL" in L.vqvs_last_error()


def test_ddim_packed_refuses_bad_arguments_without_a_device(lib_built):
    L = lib_built
    keep, (x, eps, grad, noise, a_t, a_to, out, win, first) = host_buffers(9)
    ok = dict(x=x, eps=eps, grad=grad, noise=noise, a_t=a_t, a_to=a_to, out=out, win=None, first=first, R=2, W=16, H=12, flags=2, eta=0.5)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_ddim_step_windows_packed(a["x"], a["eps"], a["grad"], a["noise"], a["a_t"], a["a_to"], a["out"], a["win"], a["first"],
                                               a["R"], a["W"], a["H"], a["flags"], a["eta"], 1.0, 1, 2, 3, None)

    inside = C.c_void_p(x.value + 16)
    for bad in (dict(x=None), dict(eps=None), dict(a_t=None), dict(a_to=None), dict(out=None), *BAD_GEOMETRY,
                dict(out=x), dict(out=inside), dict(out=grad), dict(out=first), dict(win=eps), dict(win=out),
                dict(eta=-1.0), dict(eta=float("nan")), dict(flags=1), dict(flags=3), dict(flags=16), dict(flags=6, eta=0.0),
                dict(flags=4, eta=0.5),
                dict(noise=None, grad=None, x=None), dict(win=win, R=0)):
        assert call(**bad) == -1, bad
        assert L.vqvs_last_error(), bad
    assert call(R=65536) == -1 and b"65535" in L.vqvs_last_error()
    assert call(first=None) == -1 and b"first" in L.vqvs_last_error()
    assert call(eta=-1.0) == -1 and b"eta" in L.vqvs_last_error()
    assert call(win=out) == -1 and b"overlap" in L.vqvs_last_error()


def test_dpmpp_packed_refuses_bad_arguments_without_a_device(lib_built):
    L = lib_built
    keep, (x, eps, grad, prev, a_from, a_t, a_to, out, x0, win, first) = host_buffers(11)
    ok = dict(x=x, eps=eps, grad=grad, prev=prev, a_from=a_from, a_t=a_t, a_to=a_to, out=out, x0=x0, win=None, first=first, R=2, W=16, H=12,
              flags=2)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vqvs_dpmpp_step_windows_packed(a["x"], a["eps"], a["grad"], a["prev"], a["a_from"], a["a_t"], a["a_to"], a["out"], a["x0"],
                                                a["win"], a["first"], a["R"], a["W"], a["H"], a["flags"], None)

    inside = C.c_void_p(prev.value + 16)
    for bad in (dict(x=None), dict(eps=None), dict(a_t=None), dict(a_to=None), dict(out=None), *BAD_GEOMETRY,
                dict(flags=1), dict(flags=4), dict(flags=16),
                dict(out=x), dict(out=grad), dict(out=prev), dict(out=x0), dict(out=first), dict(x0=inside), dict(x0=eps),
                dict(x0=prev, out=prev),
                dict(win=eps), dict(win=out), dict(win=x0), dict(win=prev), dict(win=prev, x0=prev),
                dict(grad=None, prev=None, a_from=None, x0=None, x=None), dict(win=win, R=0)):
        assert call(**bad) == -1, bad
        assert L.vqvs_last_error(), bad
    assert call(R=65536) == -1 and b"65535" in L.vqvs_last_error()
    assert call(flags=4) == -1 and b"flags" in L.vqvs_last_error()
    assert call(x0=inside) == -1 and b"x0_prev" in L.vqvs_last_error()


# ---------------------------------------------------------------- 2. plan_pack
@pytest.mark.parametrize("W,H", [(128, 64), (512, 256), (512, 512), (4352, 2304), (64000, 57600)])
def test_plan_pack_offsets_and_total(W, H):
    lengths = [1, W, W + 1, 3 * W, 5 * H + 7, 2 * H + (W - H), 2 * H + (W - H) + 1]
    counts, offsets, total = plan_pack(lengths, W, H)
    assert counts == [plan_windows(n, W, H)[0] for n in lengths]
    V, first = W - H, [0]
    for c in counts:
        first.append(first[-1] + c)
    assert offsets == [first[r] * H + r * V for r in range(len(lengths))]
    assert total == first[-1] * H + len(lengths) * V
    assert all(o % 4 == 0 for o in offsets)  # a quad never straddles two recordings
    for r, n in enumerate(lengths):  # every recording's padded row fits in front of the next one
        end = offsets[r + 1] if r + 1 < len(lengths) else total
        assert end - offsets[r] == plan_windows(n, W, H)[1] >= n


def test_plan_pack_refuses_what_the_kernel_cannot_index():
    assert sum(plan_pack([16] * MAX_WINDOWS, 16, 16)[0]) == MAX_WINDOWS
    with pytest.raises(ValueError):
        plan_pack([16] * (MAX_WINDOWS + 1), 16, 16)  # N > 65535
    W = 1 << 20
    assert plan_pack([W * 1023] * 2, W, W)[2] == 2046 * W
    with pytest.raises(ValueError):
        plan_pack([W * 1024] * 2, W, W)  # 2^31 samples
    for bad in ([], [0], [16, -1]):
        with pytest.raises(ValueError):
            plan_pack(bad, 16, 16)
    with pytest.raises(ValueError):
        plan_pack([100], 18, 12)


# ---------------------------------------------------------------- 3. packs, ranks, label map
WINDOWS = [1, 2, 1, 9, 1, 1, 3, 2, 2, 1, 1, 7, 1]


@pytest.mark.parametrize("budget", [2, 7, 10 ** 6])
def test_make_packs(budget):
    packs = make_packs(WINDOWS, budget)
    assert [i for p in packs for i in p] == list(range(len(WINDOWS)))  # the order is kept and a file's id is its place in the list
    for p in packs:
        assert p == list(range(p[0], p[0] + len(p)))  # consecutive ids: recording r of a pack is keyed first id + r
        assert sum(WINDOWS[i] for i in p) <= budget or len(p) == 1  # an oversized file is a pack of its own
    for a, b in zip(packs, packs[1:]):  # greedy: the next file did not fit
        assert sum(WINDOWS[i] for i in a) + WINDOWS[b[0]] > budget
    if budget == 10 ** 6:
        assert len(packs) == 1


def test_make_packs_with_ids_left_out():
    ids = [0, 1, 2, 5, 6, 9]  # files 3, 4, 7, 8 exist already (--skip-existing) or could not be read
    packs = make_packs([1] * len(ids), 100, ids)
    assert packs == [[0, 1, 2], [5, 6], [9]]  # a gap ends a pack: the ids of those that remain do not move
    for bad in (dict(windows=[1, 0], budget=4), dict(windows=[1, 1], budget=0), dict(windows=[1, 1], budget=4, ids=[3, 3]),
                dict(windows=[1, 1], budget=4, ids=[1])):
        with pytest.raises(ValueError):
            make_packs(**bad)


@pytest.mark.parametrize("world", [1, 2, 3, 8, 32])
def test_deal_packs_is_a_partition(world):
    packs = make_packs(WINDOWS, 3)
    dealt = [deal_packs(packs, rank, world) for rank in range(world)]
    assert sorted(tuple(p) for d in dealt for p in d) == sorted(tuple(p) for p in packs)
    assert sum(len(d) for d in dealt) == len(packs)
    assert max(len(d) for d in dealt) - min(len(d) for d in dealt) <= 1
    with pytest.raises(ValueError):
        deal_packs(packs, world, world)


def test_list_files_is_sorted_by_relative_path():
    index = {"b": {"x.wav": 1.0, "sub": {"a.wav": 2.0}}, "a": {"z.wav": 0.5, "c": {"d": {"e.wav": 3.0}}}}
    files = list_files(index)
    assert [f[0] for f in files] == sorted(f[0] for f in files)
    assert dict(files) == {os.path.join("a", "c", "d", "e.wav"): 3.0, os.path.join("a", "z.wav"): 0.5,
                           os.path.join("b", "sub", "a.wav"): 2.0, os.path.join("b", "x.wav"): 1.0}


def test_read_label_map(tmp_path):
    path = tmp_path / "map.tsv"
    path.write_text("# targets\nspk1\t2\n\nspk 2\t0\r\n")
    assert read_label_map(str(path)) == {"spk1": 2, "spk 2": 0}
    assert read_label_map(str(path), ["spk1"]) == {"spk1": 2, "spk 2": 0}
    with pytest.raises(ValueError, match="spk3"):
        read_label_map(str(path), ["spk1", "spk3"])  # an unmapped directory
    for text in ("spk1 2\n", "spk1\t2\t3\n", "\t2\n", "spk1\ttwo\n", "spk1\t-1\n", "spk1\t1.5\n", "spk1\t\n", "spk1\t1\nspk1\t2\n"):
        path.write_text(text)
        with pytest.raises(ValueError):
            read_label_map(str(path))


# ---------------------------------------------------------------- 4. the script's flags
def test_convert_dataset_flags(tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import convert_dataset

    flags = {o for a in convert_dataset.arg_parser()._actions for o in a.option_strings} - {"-h", "--help"}
    assert flags == {"--label", "--label-map", "--sampler", "--eta", "--sample-steps", "--window-seconds", "--overlap-seconds",
                     "--window-batch", "--pack-windows", "--enc-pred-path", "--enc-pred-scale", "--encoding", "--precision", "--seed",
                     "--max-files", "--skip-existing"}
    args = convert_dataset.parse_args(["m.pt", "data", "out", "--label", "7"])
    assert (args.checkpoint_path, args.data_dir, args.out_dir, args.label, args.label_map) == ("m.pt", "data", "out", 7, None)
    assert (args.pack_windows, args.window_batch, args.seed, args.sampler, args.eta, args.skip_existing) == (512, 64, 0, "ddpm", 0.0, False)
    args = convert_dataset.parse_args(["m.pt", "data", "out", "--label-map", "t.tsv", "--sampler", "dpmpp", "--sample-steps", "25",
                                       "--precision", "fp16", "--skip-existing", "--max-files", "3"])
    assert (args.label, args.label_map, args.sampler, args.sample_steps, args.precision) == (None, "t.tsv", "dpmpp", 25, "fp16")
    for bad in (["m.pt", "data", "out"], ["m.pt", "data", "out", "--label", "1", "--label-map", "t.tsv"],
                ["m.pt", "data", "out", "--label", "1", "--eta", "0.5"], ["m.pt", "data", "out", "--label", "1", "--pack-windows", "0"],
                ["m.pt", "data", "--label", "1"]):
        with pytest.raises(SystemExit):
            convert_dataset.parse_args(bad)
    capsys.readouterr()


def test_unmapped_directory_ends_the_run_before_any_device_work(tmp_path):
    """The plan -- files, labels, packs -- is made on the host: a file under a directory the map does not name is reported there."""
    sys.path.insert(0, ROOT)
    import convert_dataset
    from vq_voice_swap_amd.audio import ChunkWriter

    data = tmp_path / "data"
    for rel, n in (("s1/a.wav", 800), ("s1/c/b.wav", 4000), ("s2/a.wav", 300)):
        os.makedirs(data / os.path.dirname(rel), exist_ok=True)
        w = ChunkWriter(str(data / rel), 16000)
        w.write(torch.zeros(n).numpy())
        w.close()
    table = tmp_path / "t.tsv"
    table.write_text("s1\t1\n")
    argv = ["m.pt", str(data), str(tmp_path / "out"), "--label-map", str(table), "--window-seconds", "0.128", "--overlap-seconds", "0.032"]
    with pytest.raises(SystemExit, match="s2"):
        convert_dataset.main(argv)
    table.write_text("s1\t1\ns2\t0\n")
    files, labels, packs = convert_dataset.plan(convert_dataset.parse_args(argv + ["--pack-windows", "2"]), 2048, 1536)
    assert [f[0] for f in files] == [os.path.join("s1", "a.wav"), os.path.join("s1", "c", "b.wav"), os.path.join("s2", "a.wav")]
    assert labels == [1, 1, 0]
    assert packs == [[0], [1], [2]]  # 1, 3 and 1 windows under a budget of 2


# ---------------------------------------------------------------- 5. counts= and what is not built for a pack
@pytest.mark.parametrize("method", ["ddpm_sample_windows", "ddim_sample_windows", "dpmpp_sample_windows"])
def test_counts_refuses_source_keep_and_start_step(method):
    W, H, counts = 16, 12, (2, 1)
    _, _, total = plan_pack([28, 16], W, H)
    x = torch.zeros(1, 1, total)
    sample = getattr(Diffusion(make_schedule("exp")), method)

    def predictor(w, ts, first):
        raise AssertionError("the run must be refused before the predictor is called")

    for bad in (dict(source=x), dict(source=x, keep=torch.ones(1, 1, total, dtype=torch.bool)), dict(keep=torch.ones(1, 1, total, dtype=torch.bool)),
                dict(source=x, start_step=1), dict(start_step=1)):
        with pytest.raises(ValueError, match="pack"):
            sample(x, predictor, 4, window=W, hop=H, counts=counts, **bad)


# ---------------------------------------------------------------- 6. one layout: what the kernels are told, and a pack of one
class RecordingLib:
    """Stands in for the library: every entry point is there, records (name, arguments) and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args)) or 0


GEOMETRY_AT = {"ddpm": 7, "ddim": 8, "dpmpp": 10, "keep": 6}  # the index of the first geometry argument (include/vqvs.h)


@pytest.mark.parametrize("counts", [None, (2, 1), (3,)])
def test_the_layout_picks_the_entry_point_and_its_geometry(counts, monkeypatch):
    """One step and one keep call of each rule through `_Windows`, the library replaced by a recorder: one recording (no `counts`) is
    told to the `..._windows` entry points as n, a pack -- of one recording too -- to the `..._windows_packed` ones as (d_first, R)."""
    from vq_voice_swap_amd import _native, longform
    from vq_voice_swap_amd.diffusion import _Ddim, _Ddpm, _Dpmpp

    lib = RecordingLib()
    monkeypatch.setattr(_native, "lib", lambda: lib)
    monkeypatch.setattr(_native, "_stream_ptr", lambda: 0)
    W, H, n = 16, 12, 3
    _, _, total = pack_layout(counts or [n], W, H)
    d = Diffusion(make_schedule("exp"))
    x = torch.zeros(1, 1, total)
    source, keep = torch.ones_like(x), torch.ones_like(x, dtype=torch.uint8)
    for name, rule, fill, step in (("ddpm", _Ddpm(False, False), longform._ddpm_fill, longform._ddpm_step_windows),
                                   ("ddim", _Ddim(0.5, False), longform._ddim_fill, longform._ddim_step_windows),
                                   ("dpmpp", _Dpmpp(False), longform._ddim_fill, longform._dpmpp_step_windows)):
        del lib.calls[:]
        layout = longform._Windows(rule, None, None, W, H, 2, fill, step, counts=counts)
        tables = d.step_tables(2, layout.rows(x), None, x.device)
        assert (layout.n, layout.Np, layout.mb) == (n, total, 2)
        state = layout.start(x, None, None, tables[1][0], start_step=0, seed=7, clip_offset=3)
        layout.st = 0  # (what `predict` leaves: the step's stream)
        state = layout.step(state, None, None, tables, 0, noise_scale=1.0, seed=7, clip_offset=3)
        layout.keep(state, source, keep, tables[2][0], index=1, seed=7, clip_offset=3)
        (step_name, step_args), (keep_name, keep_args) = lib.calls
        suffix, geom = ("", (n,)) if counts is None else ("_packed", (layout.first.data_ptr(), len(counts)))
        assert step_name == f"vqvs_{name}_step_windows{suffix}" and keep_name == f"vqvs_keep_region_windows{suffix}"
        for args, at in ((step_args, GEOMETRY_AT[name]), (keep_args, GEOMETRY_AT["keep"])):
            assert args[at:at + len(geom) + 2] == geom + (W, H), (name, args)
        if counts is not None:
            assert layout.first.dtype == torch.int32 and layout.first.tolist() == pack_layout(counts, W, H)[0]


def test_a_pack_of_one_is_the_single_layout(monkeypatch):
    """`_Windows` without `counts` and with `counts=(n,)`: the same n, Np, offsets and slice size, and the same window batch gathered
    from the same x_T (only the entry points differ, above)."""
    from vq_voice_swap_amd import _native, longform

    monkeypatch.setattr(_native, "require_cuda", lambda *tensors: None)
    W, H, n = 16, 12, 3
    x = torch.arange((n - 1) * H + W, dtype=torch.float32).view(1, 1, -1)
    layouts = [longform._Windows(type("Rule", (), dict(name="ddim", flags=0))(), None, None, W, H, 2, None, None, counts=counts) for counts in (None, (n,))]
    states = []
    for layout in layouts:
        assert layout.rows(x) == 2 == layout.mb
        assert (layout.n, layout.Np, layout.offsets, list(layout.counts)) == (n, x.shape[2], [0], [n])
        states.append(layout.start(x, None, None, None, start_step=0, seed=0, clip_offset=0))
    assert isinstance(layouts[0].geom, int) and layouts[0].geom == n and layouts[1].geom is layouts[1] and layouts[1].R == 1
    assert torch.equal(layouts[0].windows, layouts[1].windows) and torch.equal(states[0], states[1])
    assert torch.equal(layouts[0].windows, longform.gather_windows(x, W, H))
