"""Randomised ResBlock parity sweep (HIP vs oracle): random channel counts, lengths (incl. tile-boundary cases),
dilations, resizes, FiLM on/off, batch sizes, all three precision modes.  Developer tool; tests/ hold the fixed cases.
    python tools/fuzz_resblock.py [seed] [cases] [big|walk]   ("big": every fourth case is a long, many-clip launch;
    "walk": every fourth case has few steps per clip and many clips -- L in 255 .. 1100 at widths 32 / 64 / 96 / 128, six clips per
    workgroup (VQVS_WS_GRID is honoured, so a small grid keeps the oracle cheap) -- the band where the (scale, shift) ring rule of
    conv_ws_kernel has its case boundaries; those cases are also checked per clip and, bitwise, against batches of two;
    tests/test_ws_walk_gpu.py pins the seeded list)"""
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: a process-level HIP switch, before the runtime starts
import os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from oracle import ref_cpu
from vq_voice_swap_amd.unet import ResBlockModule
from vq_voice_swap_amd.det_init import det_init_
from util import rel_rms, seeded

dev = torch.device("cuda:0")
rng = random.Random(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
N = int(sys.argv[2]) if len(sys.argv) > 2 else 40
BIG = len(sys.argv) > 3 and sys.argv[3] == "big"
WALK = len(sys.argv) > 3 and sys.argv[3] == "walk"
WALK_GRID = int(os.environ.get("VQVS_WS_GRID", "0")) or 256  # workgroups per launch (default: one per CU of an MI355X)
worst = {"fp32": 0.0, "fp16": 0.0, "bf16": 0.0}
bad = 0
for i in range(N):
    cin = rng.choice([32, 64, 96, 128, 192, 256, 384, 512])
    scale = rng.choice([1.0, 1.0, 1.0, 0.5, 2.0])
    cout = cin if scale != 1.0 else rng.choice([cin, 32, 64, 128, 256, 512])
    dil = 2 if scale == 2.0 else rng.choice([1, 2, 2, 4, 8, 16, 32])
    emb = rng.choice([None, 128, 256])
    L = rng.choice([2, 6, 64, 126, 250, 252, 254, 256, 258, 500, 508, 510, 1000, 1024, rng.randrange(2, 1500) * 2])
    B = rng.choice([1, 2, 3, 5])
    if scale == 0.5 and L < 4:  # (one output row per channel and clip: torch's group_norm -- the oracle, and the reference -- refuses it)
        L = 4
    if BIG and i % 4 == 0:  # many tiles per workgroup and workgroups that cross clip boundaries (the (scale, shift) ring)
        L = rng.choice([4000, 6002, 8190, 12000])
        B = rng.choice([24, 37, 48])
        cin = rng.choice([64, 128])
        cout = cin if scale != 1.0 else rng.choice([cin, 64, 128])
    walk = WALK and i % 4 == 0
    if walk:  # few steps per clip, every workgroup walks six clips (and starts in the middle of one when B is not a multiple of the grid)
        scale = 1.0
        cin = rng.choice([32, 64, 96, 128])
        cout = rng.choice([cin, 32, 64, 128])
        dil = rng.choice([1, 2, 4])
        L = rng.randrange(255, 1101)
        B = 6 * WALK_GRID - rng.choice([0, 1, 3])
    m = ResBlockModule(cin, emb, cout if cout != cin else None, scale, dil)
    det_init_((f"fz{i}." + k, v) for k, v in m.block.state_dict().items())
    x = seeded((B, cin, L), 5000 + i)
    e = seeded((B, emb), 6000 + i) if emb else None
    sd = {"b." + k: v.detach() for k, v in m.block.state_dict().items()}
    want = ref_cpu.res_block(x, sd, "b", dict(cin=cin, cout=cout, scale=scale, dil=dil), e)
    for prec, tol in (("fp32", 2e-4), ("fp16", 4e-3), ("bf16", 3e-2)):
        m.set_precision(prec)
        got = m(x.to(dev), None if e is None else e.to(dev)).cpu()
        err = rel_rms(got, want) if got.shape == want.shape else float("inf")
        if walk and got.shape == want.shape:  # one clip's wrong table must not hide in the batch RMS, and a clip's bits must not depend on the batch
            per_clip = ((got - want).pow(2).mean(dim=(1, 2)).sqrt() / want.pow(2).mean(dim=(1, 2)).sqrt()).max().item()
            pairs = torch.cat([m(x[j:j + 2].to(dev), None if e is None else e[j:j + 2].to(dev)) for j in range(0, B, 2)]).cpu()
            if not per_clip < 5 * tol or not torch.equal(got, pairs):
                bad += 1
                print("MISMATCH (walk)", prec, dict(cin=cin, cout=cout, dil=dil, emb=emb, L=L, B=B), "per clip", per_clip, "clips differing from the batch-of-two run",
                      int((got != pairs).flatten(1).any(dim=1).sum()), flush=True)
        worst[prec] = max(worst[prec], err)
        if not err < tol:
            bad += 1
            print("MISMATCH", prec, dict(cin=cin, cout=cout, scale=scale, dil=dil, emb=emb, L=L, B=B), err, flush=True)
print("cases", N, "worst", worst, "bad", bad)
