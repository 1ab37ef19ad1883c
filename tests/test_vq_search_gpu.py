"""The VQ code search on the device against the float64 nearest-code reference of tests/vq_ref.py: `vqvs_vq_argmin` under the
search rule over every case (random grid across the tile edges, every (tile, code group, j) slot, the tie geometries,
cancellation and scale, a NaN position), `vqvs_vq_quantize` on the same cases (codes bitwise the argmin call's, embedding an
exact copy, counts, sq_err against float64), the Python surface, three calls sharing one stream's scratch buffer, and
`vqvs_vq_embed` over its own grid with a guarded output buffer.  The reference runs on the host, once per case.

The gate is the derived bound E of vq_ref.py; what the kernel uses of it is recorded, not gated (VQVS_VQ_SEARCH_MARGINS names a
.jsonl file to append to; profiles/vq_search_margins.jsonl is such a run).  Measured on MI355X, per family, the largest
fraction of the bound used and the positions that differ from the float64 argmin: grid 0 and 0 of 3503; every slot 0 and 0 of
1544; ties 0 and 0 of 20; cancellation 0 and 0 of 768; nan 0 and 0 of 32 -- the kernel returned the float64 nearest code at every
position of every case, including the 3 positions that the rule leaves undecided."""
import json
import os

import numpy as np
import pytest
import torch

from vq_voice_swap_amd import VQ, _native

from test_vq_eval_gpu import SQERR_REL, argmin_call, quantize_call
from util import seeded
from vq_ref import CASES, Reference, reference

pytestmark = pytest.mark.gpu

IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def record(case, fraction, differ, positions):
    rec = {"case": case.name, "family": case.family, "fraction_of_bound": float(fraction), "differ_from_best64": int(differ), "positions": int(positions)}
    print(f"[margin] {case.name}: {fraction:.3e} of the bound used, {differ} of {positions} positions differ from the float64 argmin")
    path = os.environ.get("VQVS_VQ_SEARCH_MARGINS")  # a .jsonl file to append to (profiles/vq_search_margins.jsonl is such a run)
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def on_device(case, dev):
    return case.z.to(dev), case.d.to(dev)


# ---------------------------------------------------------------- the search against the float64 reference
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_argmin_obeys_the_search_rule(dev, i):
    case, ref = CASES[i], reference(i)
    z, d = on_device(case, dev)
    g = argmin_call(z, d).cpu().numpy()
    fraction, differ = ref.margins(np.clip(g, 0, case.K - 1))
    record(case, fraction, differ, g.size)
    bad = ref.violations(g)
    assert bad == [], (case.name, bad[:8], len(bad))
    if case.expected is not None:
        assert np.array_equal(g, case.expected), (case.name, np.argwhere(g != case.expected)[:8].tolist())
    for b, t in case.nan_at:
        assert g[b, t] == 0, (case.name, b, t, int(g[b, t]))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_quantize_on_the_same_cases(dev, i):
    case = CASES[i]
    z, d = on_device(case, dev)
    hist0 = (torch.arange(case.K, device=dev, dtype=torch.int64) * 5 + 1) % 7  # a non-zero start
    hist = hist0.clone()
    idx, emb, sq = quantize_call(z, d, hist=hist)
    assert torch.equal(idx, argmin_call(z, d))  # bitwise the argmin call's
    assert torch.equal(emb, d[idx].permute(0, 2, 1).contiguous())  # an exact copy of the chosen rows
    assert torch.equal(hist - hist0, torch.bincount(idx.reshape(-1), minlength=case.K))
    want = ((z.double() - d[idx].permute(0, 2, 1).double()) ** 2).flatten(1).sum(1)
    ok = ~torch.isnan(want)  # (a clip that holds a NaN has a NaN sum: nothing to compare)
    assert bool(ok.all()) == (not case.nan_at) and bool(torch.isnan(sq[~ok]).all())
    err = (sq[ok] - want[ok]).abs()
    assert (err <= SQERR_REL * want[ok]).all(), (case.name, (err / want[ok]).max().item())


# ---------------------------------------------------------------- the Python surface
@pytest.mark.parametrize("name,trailing", [("every slot Cd=68 K=130 reversed", (10, 13)), ("grid Cd=512 K=512 T1=33 B=3", (33,)),
                                           ("grid Cd=60 K=127 T1=70 B=1", (2, 5, 7))])
def test_vq_module_returns_the_same_codes(dev, name, trailing):
    i = IDS.index(name)
    case, ref = CASES[i], reference(i)
    z, d = on_device(case, dev)
    raw = argmin_call(z, d)
    vq = VQ(case.Cd, case.K).eval().to(dev)
    with torch.no_grad():
        vq.dictionary.copy_(d)
    x = z.reshape(case.B, case.Cd, *trailing)
    enc, q, fwd = vq.encode(x), vq.quantize(x), vq(x)
    assert enc.shape == (case.B, *trailing) and enc.dtype == torch.int64
    assert torch.equal(enc.reshape(case.B, -1), raw) and torch.equal(q["idxs"], enc) and torch.equal(fwd["idxs"], enc)
    assert torch.equal(fwd["embedded"], q["embedded"]) and torch.equal(fwd["embedded"], vq.embed(enc))
    assert ref.violations(enc.reshape(case.B, -1).cpu().numpy()) == []
    if case.expected is not None:
        assert np.array_equal(enc.reshape(case.B, -1).cpu().numpy(), case.expected)


# ---------------------------------------------------------------- one stream, one scratch buffer, no synchronisation
def test_calls_that_share_a_scratch_buffer(dev):
    """argmin (K = 512 norms), quantize (tile sums and K = 130 norms, laid out differently in the same buffer), argmin again:
    queued on one stream with nothing between them, each returns what it returns alone."""
    ia, ib = IDS.index("cancellation Cd=68 K=130 T1=64 scale 1e3"), IDS.index("cancellation Cd=68 K=130 T1=64 offset 3.0")
    za, zb = CASES[ia].z.to(dev), CASES[ib].z.to(dev)
    dict_a, dict_b = seeded((512, 68), 9101, 1e3).to(dev), CASES[ib].d.to(dev)  # norms of A ~ 7e7, of B ~ 7e2: a stale one is fatal
    hist0 = torch.zeros(130, device=dev, dtype=torch.int64)

    torch.cuda.synchronize()
    alone_a = argmin_call(za, dict_a)
    torch.cuda.synchronize()
    hist_alone = hist0.clone()
    alone_b = quantize_call(zb, dict_b, hist=hist_alone)
    torch.cuda.synchronize()

    hist = hist0.clone()
    first = argmin_call(za, dict_a)
    second = quantize_call(zb, dict_b, hist=hist)
    third = argmin_call(za, dict_a)
    torch.cuda.synchronize()
    assert torch.equal(first, alone_a) and torch.equal(third, alone_a)
    assert all(torch.equal(x, y) for x, y in zip(second, alone_b)) and torch.equal(hist, hist_alone)
    # and both are right, not merely equal
    assert Reference(za.cpu(), dict_a.cpu()).violations(alone_a.cpu().numpy()) == []
    assert reference(ib).violations(alone_b[0].cpu().numpy()) == []


# ---------------------------------------------------------------- the gather
GUARD = 64
SENTINEL = -12345.0


@pytest.mark.parametrize("Cd", [1, 3, 4, 68])
@pytest.mark.parametrize("T1", [1, 255, 256, 257])
def test_embed_is_an_exact_gather_inside_its_buffer(dev, Cd, T1):
    for K in (1, 130):
        d = seeded((K, Cd), 300 + Cd + K).to(dev)
        for B in (1, 3):
            idx = torch.randint(0, K, (B, T1), generator=torch.Generator().manual_seed(400 + T1 + B)).to(dev)
            if B * T1 >= 2:
                idx[0, 0], idx[-1, -1] = 0, K - 1  # both ends of the dictionary in one call
                calls = [idx]
            else:
                calls = [torch.zeros_like(idx), torch.full_like(idx, K - 1)]  # one position: one call per end
            assert min(int(ix.min()) for ix in calls) == 0 and max(int(ix.max()) for ix in calls) == K - 1
            for ix in calls:
                n = B * Cd * T1
                buf = torch.full((GUARD + n + GUARD,), SENTINEL, device=dev, dtype=torch.float32)
                out = buf[GUARD:GUARD + n]
                _native.check(_native.lib().vqvs_vq_embed(ix.data_ptr(), d.data_ptr(), out.data_ptr(), B, Cd, T1, K, _native._stream_ptr()))
                assert torch.equal(out.reshape(B, Cd, T1), d[ix].permute(0, 2, 1).contiguous()), (Cd, T1, K, B)
                assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all(), (Cd, T1, K, B)
