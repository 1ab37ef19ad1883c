"""conv_ws_kernel's persistent workgroups walk a contiguous range of tiles that may cross clip boundaries, and the producers read
each clip's GroupNorm/FiLM (scale, shift) table from a ring of LDS slots (clip & (ss_ring - 1)) that the planner sizes from the
steps per clip, spc = ntx * nty * nchunks.  The ring rule has its case boundaries at spc = 2 and spc = 5 (the load cursor runs
WS_LOOKAHEAD = 5 chunks ahead of a chunk another wave still stages), so this file pins spc in {1, 2, 3, 4, 5, 6, 8} with every
workgroup walking at least five consecutive clips -- spc == 4 by five routes -- crossed with who builds the tables (producer waves
copy them / consumer waves build them from a fused GroupNorm), the walk direction, FiLM, and both gate modes.

Per case: parity against the CPU oracle at the ResBlock gates (batch and per clip), a repeat run that must be bitwise equal, and
every clip bitwise equal to the same clip run in a batch of two (a batch of two cannot span three clips in any workgroup: one
borrowed (scale, shift) row changes bits).  The VQVS_WS_TRACE lines of the process prove that the intended (spc, table builder)
class ran with >= 5 clips per workgroup, and that every traced ring is larger than the clip span of its lookahead.

The switches are read once per process, so each case runs in its own interpreter, one after another, each under its own time
limit.  A case whose interpreter ends in anything but a clean verdict (a signal, a time limit, an unexpected exit status) stops the
file: no further case is started on the GPU."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GATE = {"fp32": 2e-4, "fp16": 4e-3}  # the ResBlock gates of test_scale_gpu.py / test_switches_gpu.py; per clip: 5x
MIN_CLIPS_PER_WG = 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


SCRIPT = r"""
import json, os, sys
case = json.loads(sys.argv[1])
trace_path = sys.argv[2]
# the library writes its VQVS_WS_TRACE lines to file descriptor 2: keep them in a file this process can read back
sys.stderr.flush()
_saved = os.dup(2)
_tf = open(trace_path, "w")
os.dup2(_tf.fileno(), 2)
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import torch
from oracle import ref_cpu
from vq_voice_swap_amd.unet import ResBlockModule
from vq_voice_swap_amd.det_init import det_init_
from util import gate, rel_rms, seeded

def parse_trace():
    plans = []
    for line in open(trace_path):
        if line.startswith("conv_ws: "):
            kv = dict(t.split("=", 1) for t in line.split()[1:])
            plans.append({{k: (v if k == "prec" else int(v)) for k, v in kv.items()}})
    return plans

def main():
    dev = torch.device("cuda:0")
    torch.set_num_threads(8)
    cin, cout, dil, L, B, emb = (case[k] for k in ("cin", "cout", "dil", "L", "B", "emb"))
    name, seed = case["id"], case["seed"]
    m = ResBlockModule(cin, emb, cout if cout != cin else None, 1.0, dil)
    det_init_((f"walk.{{name}}." + k, v) for k, v in m.block.state_dict().items())
    x = seeded((B, cin, L), 9000 + seed)
    e = seeded((B, emb), 9500 + seed) if emb else None
    sd = {{"b." + k: v.detach() for k, v in m.block.state_dict().items()}}
    want = ref_cpu.res_block(x, sd, "b", dict(cin=cin, cout=cout, scale=1.0, dil=dil), e)
    xd, ed = x.to(dev), None if e is None else e.to(dev)
    results, failures = [], []
    for prec in case["precs"]:
        tol = case["gates"][prec]
        m.set_precision(prec)
        got = m(xd, ed).cpu()
        again = m(xd, ed).cpu()  # a race shows up as nondeterminism
        pairs = []
        for i in range(0, B, 2):  # every clip again, in a batch of (at most) two
            pairs.append(m(xd[i:i + 2].contiguous(), None if ed is None else ed[i:i + 2].contiguous()))
        small = torch.cat(pairs).cpu()
        err = rel_rms(got, want)
        clip_err = (got - want).pow(2).mean(dim=(1, 2)).sqrt() / want.pow(2).mean(dim=(1, 2)).sqrt()
        worst = int(clip_err.argmax())
        diff_small = (got != small).flatten(1).any(dim=1)
        diff_again = (got != again).flatten(1).any(dim=1)
        r = dict(id=name, prec=prec, err=err, gate=tol, per_clip=clip_err[worst].item(), per_clip_gate=5 * tol, worst_clip=worst,
                 clips_differ_from_pairs=int(diff_small.sum()), clips_differ_on_repeat=int(diff_again.sum()),
                 first_differing_clip=int(diff_small.nonzero()[0]) if diff_small.any() else None)
        print("WALK_RESULT " + json.dumps(r), flush=True)
        results.append(r)
        for what, fn in (("batch", lambda: gate(f"ws_walk.{{name}}.{{prec}}", got, want, tol, relative=True)),
                         ("worst clip", lambda: gate(f"ws_walk.{{name}}.{{prec}}.worst_clip", got[worst], want[worst], 5 * tol, relative=True))):
            try:
                fn()
            except AssertionError as ex:
                failures.append(f"{{prec}}: {{what}} parity: {{ex}}")
        if diff_again.any():
            failures.append(f"{{prec}}: a repeat run changed {{int(diff_again.sum())}} clips")
        if diff_small.any():
            failures.append(f"{{prec}}: {{int(diff_small.sum())}} clips differ bitwise from the batch-of-two run, first {{r['first_differing_clip']}}")
    torch.cuda.synchronize()
    # coverage guard: the intended plans ran, each workgroup walking at least five clips, with a ring the lookahead cannot wrap
    plans = parse_trace()
    print("WALK_PLANS " + json.dumps(plans), flush=True)
    big = [p for p in plans if p["B"] == B]
    for prec, spc, gn in case["expect"]:
        hit = [p for p in big if p["prec"] == prec and p["spc"] == spc and p["gn"] == gn]
        if "rev" in case:
            hit = [p for p in hit if p["rev"] in case["rev"]]
        if not hit:
            failures.append(f"coverage: no traced plan with prec={{prec}} spc={{spc}} gn={{gn}} at B={{B}}")
        for p in hit:
            clips = p["ntiles"] / p["grid"] / (p["ntx"] * p["nty"])
            if clips < case["min_clips"]:
                failures.append(f"coverage: prec={{prec}} spc={{spc}}: only {{clips:.2f}} clips per workgroup")
            if case.get("mid_clip") and p["ntiles"] % p["grid"] == 0 and (p["ntiles"] // p["grid"]) % (p["ntx"] * p["nty"]) == 0:
                failures.append(f"coverage: prec={{prec}} spc={{spc}}: every workgroup starts on a clip boundary")
    for p in plans:
        span = (p["spc"] - 1 + p["la"]) // p["spc"]  # clip boundaries between the last chunk of a clip and the cursor la chunks on
        if p["ss_ring"] & (p["ss_ring"] - 1) or p["ss_ring"] <= span:
            failures.append(f"ring: spc={{p['spc']}} lookahead={{p['la']}} spans {{span}} clips but ss_ring={{p['ss_ring']}} ({{p['prec']}}, gn={{p['gn']}})")
    return failures

code = 2
try:
    failures = main()
    for f in failures:
        print("WALK_FAILURE " + f, flush=True)
    print("WALK_VERDICT " + ("FAIL" if failures else "OK"), flush=True)
    code = 1 if failures else 0
finally:
    os.dup2(_saved, 2)
    _tf.close()
    try:
        sys.stderr.write(open(trace_path).read())
    except OSError:
        pass
sys.exit(code)
"""

GRID8 = {"VQVS_WS_GRID": "8"}  # 8 workgroups: 45 ... 48 clips are then 5.6 ... 6 clips per workgroup, and the CPU oracle stays cheap
GN0 = {"VQVS_WS_GN": "0"}  # the producers copy the tables at every width
REV0 = {"VQVS_WS_REV": "0"}  # every launch walks forward (the default alternates: conv 1 forward, conv 2 from the far end)


def C(id, cin, cout, dil, L, B, emb, env, expect, *, precs=("fp16", "fp32"), timeout=300, mid_clip=False, rev=None):
    d = dict(id=id, cin=cin, cout=cout, dil=dil, L=L, B=B, emb=emb, env=env, expect=expect, precs=list(precs), mid_clip=mid_clip, timeout=timeout)
    if rev is not None:
        d["rev"] = rev
    return d


# expect: (mode, spc, 1 = tables built by the consumers / 0 = copied by the producers) of a plan that must be traced at the case's B.
# Geometry (fp16 storage: 256 staged rows, tile_rows = 256 - 2 * dilation, conv 1 has dilation 1; an identity skip is CT / 32 more
# chunks of conv 2, a 1x1 skip conv cin / 32; fp32 storage: 128 x 128 tiles of 128 - 2 * dilation rows at 128 channels, the identity
# skip is added in the epilogue; 32 output channels run on conv_mfma_kernel in the fp32 mode, so only fp16 plans are expected there).
CASES = [
    # ---- 32 channels: never fused (the planner wants Ctot % 64 == 0)
    C("c32_L200_film", 32, 32, 1, 200, 48, 128, GRID8, [("fp16", 1, 0), ("fp16", 2, 0)]),  # conv 1: 1 chunk, 1 tile; conv 2: + skip chunk
    C("c32_L200_fwd", 32, 32, 2, 200, 48, None, {**GRID8, **REV0}, [("fp16", 1, 0), ("fp16", 2, 0)], rev=[0]),
    C("c32_L600", 32, 32, 1, 600, 48, None, GRID8, [("fp16", 3, 0), ("fp16", 6, 0)]),  # ntx = 3
    C("c32_L900_midclip_film", 32, 32, 1, 900, 45, 128, GRID8, [("fp16", 4, 0), ("fp16", 8, 0)], mid_clip=True),  # conv 1: ntx = 4; 22.5 tiles per workgroup
    C("c32_L900_fwd", 32, 32, 2, 900, 48, None, {**GRID8, **REV0}, [("fp16", 4, 0), ("fp16", 8, 0)], rev=[0]),
    C("c32_L400", 32, 32, 1, 400, 48, None, GRID8, [("fp16", 2, 0), ("fp16", 4, 0)]),  # conv 2: ntx = 2 with the skip chunk, reversed
    C("c32_L400_fwd_film", 32, 32, 1, 400, 45, 128, {**GRID8, **REV0}, [("fp16", 2, 0), ("fp16", 4, 0)], mid_clip=True, rev=[0]),
    C("c96to32_L200", 96, 32, 1, 200, 48, None, GRID8, [("fp16", 3, 0), ("fp16", 4, 0)]),  # conv 1: 3 chunks; conv 2: 1 + 3 (1x1 skip conv)
    C("c160to32_L200_film", 160, 32, 2, 200, 48, 128, GRID8, [("fp16", 5, 0), ("fp16", 6, 0)]),  # 5 chunks; 1 + 5
    # ---- 64 channels and up: fused by default (fp16), producer-built with VQVS_WS_GN=0 and in the fp32 mode
    C("c64_L400", 64, 64, 1, 400, 48, None, GRID8, [("fp16", 4, 1), ("fp16", 8, 1), ("fp32", 4, 0)]),  # ntx = 2, 2 (+ 2) chunks
    C("c64_L400_gn0_film", 64, 64, 2, 400, 45, 128, {**GRID8, **GN0}, [("fp16", 4, 0), ("fp16", 8, 0), ("fp32", 4, 0)], mid_clip=True),
    C("c64_L400_gn0_fwd", 64, 64, 1, 400, 48, None, {**GRID8, **GN0, **REV0}, [("fp16", 4, 0), ("fp16", 8, 0), ("fp32", 4, 0)], rev=[0]),
    C("c128_L200_film", 128, 128, 1, 200, 48, 128, GRID8, [("fp16", 4, 1), ("fp16", 8, 1), ("fp32", 8, 0)]),  # n = 4, ntx = 1 (fp32: two 126-row tiles)
    C("c128_L200_gn0", 128, 128, 2, 200, 48, None, {**GRID8, **GN0}, [("fp16", 4, 0), ("fp16", 8, 0), ("fp32", 8, 0)]),
    C("c128_L120_film", 128, 128, 1, 120, 48, 128, GRID8, [("fp32", 4, 0), ("fp16", 4, 1)]),  # fp32: the 128-row x 128-channel geometry, both convolutions
    C("c128_L120_fwd", 128, 128, 2, 120, 48, None, {**GRID8, **REV0}, [("fp32", 4, 0), ("fp16", 4, 1)], rev=[0]),
    C("c32to64_L200", 32, 64, 1, 200, 48, None, GRID8, [("fp16", 3, 1), ("fp32", 3, 0)]),  # conv 2: 2 + 1 chunks (conv 1 is one chunk at CT = 64: declined)
    C("c32to64_L200_gn0_film", 32, 64, 2, 200, 48, 128, {**GRID8, **GN0}, [("fp16", 3, 0), ("fp32", 3, 0)]),
    C("c96to64_L200_film", 96, 64, 1, 200, 48, 128, GRID8, [("fp16", 3, 0), ("fp16", 5, 1), ("fp32", 3, 0), ("fp32", 5, 0)]),  # conv 2: 2 + 3
    C("c64to128_L120", 64, 128, 1, 120, 48, None, GRID8, [("fp16", 2, 1), ("fp16", 6, 1), ("fp32", 2, 0), ("fp32", 6, 0)]),  # conv 2: 4 + 2
    C("c64to128_L120_gn0_film", 64, 128, 2, 120, 48, 128, {**GRID8, **GN0}, [("fp16", 2, 0), ("fp16", 6, 0), ("fp32", 2, 0), ("fp32", 6, 0)]),
    # ---- no switch set: one workgroup per CU, 1408 clips = 5.5 clips per workgroup (every second one starts in the middle of a clip)
    C("c32_L900_default_film", 32, 32, 1, 900, 1408, 128, {}, [("fp16", 4, 0), ("fp16", 8, 0)], timeout=900, mid_clip=True),
    C("c32_L400_default", 32, 32, 2, 400, 1408, None, {}, [("fp16", 2, 0), ("fp16", 4, 0)], timeout=900, mid_clip=True),
]

_stopped = []  # set by the first case that did not end in a clean verdict


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_ws_walk(case, dev, tmp_path):
    if _stopped:
        pytest.fail(f"not started: case {_stopped[0]} ended without a clean verdict, nothing further runs on the GPU")
    script = tmp_path / "walk.py"
    script.write_text(SCRIPT.format(root=ROOT))
    spec = dict(case, seed=CASES.index(case), gates=GATE, min_clips=MIN_CLIPS_PER_WG)
    env = {k: v for k, v in os.environ.items() if k not in ("VQVS_WS_GRID", "VQVS_WS_GN", "VQVS_WS_REV", "VQVS_WS_TRACE")}
    env.update(case["env"], VQVS_WS_TRACE="1")
    try:
        r = subprocess.run([sys.executable, str(script), json.dumps(spec), str(tmp_path / "trace.txt")], capture_output=True, text=True, env=env,
                           timeout=case["timeout"])
    except subprocess.TimeoutExpired as ex:
        _stopped.append(case["id"])
        pytest.fail(f"{case['id']}: no verdict within {case['timeout']} s\n{(ex.stdout or b'')[-4000:]}\n{(ex.stderr or b'')[-4000:]}")
    print(r.stdout[-6000:])
    clean = (r.returncode == 0 and "WALK_VERDICT OK" in r.stdout) or (r.returncode == 1 and "WALK_VERDICT FAIL" in r.stdout)
    if not clean:
        _stopped.append(case["id"])
    assert r.returncode == 0 and "WALK_VERDICT OK" in r.stdout, f"{case['id']}: exit status {r.returncode}\n{r.stdout[-6000:]}\n{r.stderr[-6000:]}"
