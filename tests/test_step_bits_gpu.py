"""Every output bit of the nine reverse-step entry points against a recorded table (tests/step_bits.json).

The DDPM, DDIM and DPM-Solver++(2M) steps each run on a batch of clips, on one long row seen through overlapping windows and on a
pack of such rows (csrc/sampler_kernels.hip: one rule per sampler, one kernel per layout).  A change that is meant to leave the
arithmetic alone -- moving a body between kernels, merging two kernels, another launch path -- must leave every output bit as it
was.  The table holds, per case, the SHA-256 of the raw bytes of every output array (`x_to`, and `windows` and `x0_out` where the
form has them); the test passes when every hash equals the recorded one.

The table is written by `python tests/test_step_bits_gpu.py --record` on a GPU machine, against the library that is to be held, and
never by the test.

Inputs come from a CPU torch.Generator seeded from the case id: x, eps, the explicit noise and the history ~ N(0, 1), grad ~ 0.1 N(0, 1),
drawn in float64 and rounded to float32, and the alphas from ExpSchedule in float64, rounded likewise (a float64 draw goes through no
instruction-set specific code, so the inputs are the same bits on every host).  Outputs start at -7 everywhere.

Shapes, the smallest at which each path can go wrong:
  clips (B, T)        (1, 1); (2, 5): a tail quad; (2, 8) with every array offset by one float: DPM-Solver++'s one-by-one path at
                      T % 4 == 0; (2, 4099): two sum chunks (4096) and a tail; (2, 4100): two chunks, T % 4 == 0
  windows (n, W, H)   (1, 8, 4); (3, 8, 4): V = H, every interior quad in two windows; (2, 512, 256); (3, 512, 512): no overlap;
                      (2, 4352, 2304): two chunks per window
  packs (W, H, counts) (8, 4, [1, 3, 1]); (512, 256, [2, 1, 3]); (4352, 2304, [1, 2]): recording boundaries, per-recording partials
Times (t_from, t, t_to): (0.8, 0.7, 0.6) early; (0.3, 0.2, 0.1) late, where the clamp of CONSTRAIN binds only partly; (0.2, 0.1, 0.0)
the last step, alpha_to = 1.  Row b of a batch of clips takes its times 0.01 b lower, so rows have their own scalars.
Axes: DDPM {0, SIGMA_LARGE, CONSTRAIN, both} x noise {given, drawn, noise_scale = 0}; DDIM eta {0, 0.5, 1} x CONSTRAIN x guided x
noise {given, drawn}, and INVERT at eta 0 (clips and windows; stepped from t_to back to t, since at eta 0 the flag alone changes
nothing); DPM-Solver++ history {none, given, given with x0_out == x0_prev} x CONSTRAIN x guided, and one case with x0_out = NULL.
The small shapes take the full product; the two-chunk shapes one guided CONSTRAIN case and one plain case per sampler."""
import ctypes as C
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_bits.json")
SIGMA_LARGE, CONSTRAIN, INVERT = 1, 2, 4
TIMES = {"early": (0.8, 0.7, 0.6), "late": (0.3, 0.2, 0.1), "last": (0.2, 0.1, 0.0)}
# (layout, shape id, shape, every array offset by one float, full product)
SHAPES = [
    ("clips", "1x1", (1, 1), False, True), ("clips", "2x5", (2, 5), False, True), ("clips", "2x8off1", (2, 8), True, True),
    ("clips", "2x4099", (2, 4099), False, False), ("clips", "2x4100", (2, 4100), False, False),
    ("windows", "1x8x4", (1, 8, 4), False, True), ("windows", "3x8x4", (3, 8, 4), False, True),
    ("windows", "2x512x256", (2, 512, 256), False, True), ("windows", "3x512x512", (3, 512, 512), False, True),
    ("windows", "2x4352x2304", (2, 4352, 2304), False, False),
    ("pack", "8x4_1-3-1", (8, 4, (1, 3, 1)), False, True), ("pack", "512x256_2-1-3", (512, 256, (2, 1, 3)), False, True),
    ("pack", "4352x2304_1-2", (4352, 2304, (1, 2)), False, False),
]


def _axes(rule, layout, full):
    """The (axis id, settings) of one sampler at one shape."""
    out = []
    if rule == "ddpm":
        for flags in (0, SIGMA_LARGE, CONSTRAIN, SIGMA_LARGE | CONSTRAIN) if full else (CONSTRAIN, 0):
            for noise in ("given", "drawn", "off") if full else ("drawn",):
                out.append((f"f{flags}.{noise}", dict(flags=flags, noise=noise)))
    elif rule == "ddim":
        if not full:
            return [("e0.5.f2.g1.drawn", dict(eta=0.5, flags=CONSTRAIN, guided=True, noise="drawn")),
                    ("e0.5.f0.g0.drawn", dict(eta=0.5, flags=0, guided=False, noise="drawn"))]
        for eta in (0.0, 0.5, 1.0):
            for flags in (0, CONSTRAIN):
                for guided in (False, True):
                    for noise in ("given", "drawn"):
                        out.append((f"e{eta}.f{flags}.g{int(guided)}.{noise}", dict(eta=eta, flags=flags, guided=guided, noise=noise)))
        if layout != "pack":
            for guided in (False, True):
                out.append((f"e0.0.f{INVERT}.g{int(guided)}.drawn", dict(eta=0.0, flags=INVERT, guided=guided, noise="drawn", back=True)))
    else:
        if not full:
            return [("given.f2.g1", dict(hist="given", flags=CONSTRAIN, guided=True)), ("given.f0.g0", dict(hist="given", flags=0, guided=False))]
        for hist in ("none", "given", "inplace"):
            for flags in (0, CONSTRAIN):
                for guided in (False, True):
                    out.append((f"{hist}.f{flags}.g{int(guided)}", dict(hist=hist, flags=flags, guided=guided)))
        out.append(("given.f0.g0.nox0out", dict(hist="given", flags=0, guided=False, x0_out=False)))
    return out


def _cases():
    groups = {}
    for rule in ("ddpm", "ddim", "dpmpp"):
        for layout, sid, shape, off1, full in SHAPES:
            cases = groups.setdefault(f"{rule}.{layout}.{sid}", [])
            for tid in TIMES:
                for aid, ax in _axes(rule, layout, full):
                    cases.append(dict(ax, id=f"{rule}.{layout}.{sid}.{tid}.{aid}", rule=rule, layout=layout, shape=shape, off1=off1, times=tid))
    return groups


GROUPS = _cases()
CASE_IDS = [c["id"] for g in GROUPS.values() for c in g]


def run_case(case):
    """{output name: its array on the host} of one case, run through the C entry point."""
    from vq_voice_swap_amd import _native
    from vq_voice_swap_amd.diffusion import ExpSchedule

    L = _native.lib()
    dev = torch.device("cuda:0")
    digest = hashlib.sha256(case["id"].encode()).digest()
    g = torch.Generator().manual_seed(int.from_bytes(digest[:7], "little"))
    seed, clip, step = int.from_bytes(digest[8:16], "little"), int.from_bytes(digest[16:20], "little"), digest[20]
    off = 1 if case["off1"] else 0
    rule, layout, shape = case["rule"], case["layout"], case["shape"]

    def put(v):  # a float32 device array holding v, one float past its allocation's start when the case is misaligned
        buf = torch.empty(v.numel() + off, dtype=torch.float32, device=dev)
        buf[off:].copy_(v.reshape(-1))
        return buf[off:]

    def randn(n, scale=1.0):
        return put((torch.randn(n, generator=g, dtype=torch.float64) * scale).float())

    def blank(n):
        return put(torch.full((n,), -7.0))

    first = None
    if layout == "clips":
        B, T = shape
        rows, n_long, n_win, dims = B, B * T, B * T, (B, T)
    elif layout == "windows":
        n, W, H = shape
        rows, n_long, n_win, dims = 1, (n - 1) * H + W, n * W, (n, W, H)
    else:
        W, H, counts = shape
        rows, n_long, n_win, dims = 1, sum(counts) * H + len(counts) * (W - H), sum(counts) * W, (len(counts), W, H)
        first = torch.tensor([sum(counts[:i]) for i in range(len(counts) + 1)], dtype=torch.int32, device=dev)
    t_from, t, t_to = TIMES[case["times"]]
    if case.get("back"):
        t, t_to = t_to, t
    lower = 0.01 * torch.arange(rows, dtype=torch.float64)
    a_from, a_t, a_to = (put(ExpSchedule()(ti - lower).float()) for ti in (t_from, t, t_to))

    x, eps = randn(n_long), randn(n_win)
    grad = randn(n_win, 0.1) if case.get("guided") else None
    noise = randn(n_long) if case.get("noise") == "given" else None
    outs = {"x_to": blank(n_long)}
    if layout != "clips":
        outs["windows"] = blank(n_win)
    p = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    geom = ([p(first)] if first is not None else []) + list(dims)
    st = _native._stream_ptr()
    tail_out = [p(outs.get("windows"))] if layout != "clips" else []
    if rule == "dpmpp":
        hist = randn(n_long) if case["hist"] != "none" else None
        if case.get("x0_out", True):
            outs["x0_out"] = hist if case["hist"] == "inplace" else blank(n_long)
        args = [p(x), p(eps), p(grad), p(hist), p(a_from) if hist is not None else None, p(a_t), p(a_to), p(outs["x_to"]), p(outs.get("x0_out"))]
        args += tail_out + geom + [case["flags"], st]
    else:
        scale = {"given": 1.0, "drawn": 0.75, "off": 0.0}[case["noise"]]
        draw = [C.c_float(scale), seed, clip, step, st]
        if rule == "ddpm":
            args = [p(x), p(eps), p(noise), p(a_t), p(a_to), p(outs["x_to"])] + tail_out + geom + [case["flags"]] + draw
        else:
            args = [p(x), p(eps), p(grad), p(noise), p(a_t), p(a_to), p(outs["x_to"])] + tail_out + geom + [case["flags"], C.c_float(case["eta"])] + draw
    fn = getattr(L, f"vqvs_{rule}_step" + {"clips": "", "windows": "_windows", "pack": "_windows_packed"}[layout])
    _native.check(fn(*args))
    return {k: v.cpu().numpy() for k, v in outs.items()}


def bits(case):
    return {k: hashlib.sha256(v.tobytes()).hexdigest() for k, v in run_case(case).items()}


@pytest.fixture(scope="module")
def recorded():
    with open(TABLE) as f:
        table = json.load(f)
    assert sorted(table) == sorted(CASE_IDS), "tests/step_bits.json does not hold the case list of this file"
    return table


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_step_bits(group, recorded):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    wrong = []
    for case in GROUPS[group]:
        got, want = bits(case), recorded[case["id"]]
        assert sorted(got) == sorted(want), (case["id"], sorted(got), sorted(want))
        wrong += [f"{case['id']}:{k}" for k in got if got[k] != want[k]]
    assert not wrong, f"{len(wrong)} output arrays of {group} differ from the recorded bits: {wrong[:8]}"


def record():
    assert torch.cuda.is_available(), "recording needs an MI355X"
    table = {}
    for group in sorted(GROUPS):
        for case in GROUPS[group]:
            table[case["id"]] = bits(case)
        print(f"{group}: {len(GROUPS[group])} cases", flush=True)
    with open(TABLE, "w") as f:
        json.dump(table, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"wrote {TABLE}: {len(table)} cases, {sum(len(v) for v in table.values())} arrays")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_step_bits_gpu.py --record")
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
    record()
