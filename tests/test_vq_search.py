"""The VQ code search, host side: the float64 nearest-code reference of tests/vq_ref.py against the oracle on fixture F7, the
cases' own conditions (pairwise covering, the cap on what the search rule leaves undecided, the exact families), an honest
float32 implementation that passes the rule on every case, five defective ones that the rule rejects, and the argument checks
of `vqvs_vq_embed` / `vqvs_vq_argmin` on the built library (none of this needs a device).  The kernels themselves meet the
same cases in tests/test_vq_search_gpu.py."""
import ctypes as C
from itertools import combinations

import numpy as np
import pytest
import torch

from oracle import ref_cpu
from vq_voice_swap_amd import _native

import vq_ref
from util import seeded
from vq_ref import CASES, EXACT_FAMILIES, FAMILIES, MUTANTS, UNDECIDED_CAP, Reference, reference

IDS = [c.name for c in CASES]


# ---------------------------------------------------------------- the reference against the oracle (fixture F7)
def test_best64_agrees_with_the_oracle_on_f7(golden):
    z7 = golden("f7_encoder_vq32")
    dic = seeded((512, 512), 77, 0.35)
    z = torch.from_numpy(z7["z"]).float()
    ref = Reference(z, dic)
    oracle = ref_cpu.vq_encode(dic, z).numpy()
    # the oracle is the same formula in float32 (a bmm and two sums of 512 terms): it obeys the rule everywhere ...
    assert ref.violations(oracle) == []
    # ... and equals best64 wherever the fixture's recorded top-2 gap clears the bound on two distances
    sure = z7["gap"].astype(np.float64) > 2 * ref.E.max(axis=-1)
    assert sure.mean() >= 0.9, sure.mean()
    assert np.array_equal(oracle[sure], ref.best[sure])
    # wherever the rule leaves nothing open, too, whatever the recorded gap says
    decided = ~ref.undecided()
    assert np.array_equal(oracle[decided], ref.best[decided])
    print(f"F7: {int((~sure).sum())} of {sure.size} positions below the bound, {int((~decided).sum())} undecided, "
          f"{int((oracle != ref.best).sum())} differ from best64")
    # the margin set: dictionary rows plus 1e-3 noise
    idx_m = torch.from_numpy(z7["margin_idx"])
    zm = ref_cpu.vq_embed(dic, idx_m) + 1e-3 * seeded((2, 512, 250), int(z7["margin_noise_seed"]))
    ref_m = Reference(zm, dic)
    assert np.array_equal(ref_m.best, idx_m.numpy()) and not ref_m.undecided().any()


def test_dist64_is_the_plain_sum_of_squared_differences():
    z, d = seeded((2, 8, 3), 1), seeded((5, 8), 2)
    D, S = vq_ref.dist64(z, d), vq_ref.mag64(z, d)
    assert D.shape == S.shape == (2, 3, 5) and D.dtype == np.float64
    for b in range(2):
        for t in range(3):
            for k in range(5):
                x, e = z[b, :, t].double(), d[k].double()
                assert D[b, t, k] == pytest.approx(float(((x - e) ** 2).sum()), rel=1e-15)
                assert S[b, t, k] == pytest.approx(float(((x.abs() + e.abs()) ** 2).sum()), rel=1e-15)
    assert np.array_equal(vq_ref.err_bound(z, d), 11 * 2.0 ** -24 * S)
    # first index on ties, and the smallest index among equal rows
    d2 = d.clone()
    d2[3] = d2[1]
    zz = d2[[3, 1]].t()[None].contiguous()
    assert vq_ref.best64(zz, d2).tolist() == [[1, 1]]
    assert vq_ref.first_equal_row(d2).tolist() == [0, 1, 2, 1, 4]
    r = Reference(zz, d2)
    assert r.violations(np.array([[1, 1]])) == [] and [v[3] for v in r.violations(np.array([[3, 1]]))] == ["a later copy of an equal row"]
    assert not r.undecided().any()  # the copy does not make the position undecided


# ---------------------------------------------------------------- the cases' own conditions
def test_cases_cover_every_pair_of_the_grid_and_the_listed_families():
    grid = [(c.Cd, c.K, c.T1, c.B) for c in CASES if c.family == "grid"]
    factors = (vq_ref.GRID_CD, vq_ref.GRID_K, vq_ref.GRID_T1, vq_ref.GRID_B)
    assert len(grid) == len(set(grid)) == len(vq_ref.GRID_CD) * len(vq_ref.GRID_K)
    for a, b in combinations(range(4), 2):
        assert {(g[a], g[b]) for g in grid} == {(u, v) for u in factors[a] for v in factors[b]}, (a, b)
    assert {c.family for c in CASES} == set(FAMILIES)
    assert sorted((c.Cd, c.K, c.T1) for c in CASES if c.family == "every slot") == sorted([(4, 130, 130), (68, 130, 130), (68, 512, 512)] * 2)
    assert sorted((c.Cd, c.K) for c in CASES if c.family == "ties") == [(4, 257), (68, 257)]
    assert sorted({(c.Cd, c.K, c.T1) for c in CASES if c.family == "cancellation"}) == [(32, 512, 64), (68, 130, 64)]
    assert sum(c.family == "cancellation" for c in CASES) == 6 and not any(c.Cd == 512 for c in CASES if c.family == "cancellation")
    for c in CASES:
        assert c.z.dtype == torch.float32 and c.d.dtype == torch.float32 and c.B * c.T1 <= 600
        assert (c.expected is not None) == (c.family in EXACT_FAMILIES)
        assert bool(torch.isnan(c.z).any()) == (c.family == "nan") and not torch.isnan(c.d).any()
    (nan,) = [c for c in CASES if c.family == "nan"]
    assert int(torch.isnan(nan.z).sum()) == 1 and nan.T1 == 32 and nan.nan_at == ((0, 13),)
    # the tie geometries are what their names say (16 codes per thread, 128 per tile)
    d = [c for c in CASES if c.family == "ties"][0].d
    for first, copies in vq_ref.TIE_COPIES.items():
        for k in copies:
            assert torch.equal(d[k], d[first]) and first < k
    slot = lambda k: (k // 128, (k % 128) // 16, k % 16)  # noqa: E731  (tile, code group, j)
    assert slot(2)[:2] == slot(5)[:2]
    assert slot(3)[0] == slot(40)[0] and slot(3)[1] != slot(40)[1]
    assert slot(7)[0] != slot(135)[0] and slot(7)[1:] == slot(135)[1:]
    assert slot(120)[0] < slot(130)[0] and slot(120)[1] > slot(130)[1]
    assert slot(256) == (2, 0, 0) and 257 - 256 == 1


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_rule_leaves_little_open(i):
    """A condition on the cases, not a measurement: nothing undecided in the exact families, at most 2 % of a case's positions
    elsewhere (a seed changes, never the cap)."""
    case, ref = CASES[i], reference(i)
    und = ref.undecided()
    share = und.mean()
    print(f"{case.name}: {int(und.sum())} of {und.size} positions undecided")
    if case.family in EXACT_FAMILIES:
        assert not und.any()
        assert np.array_equal(ref.best, case.expected)  # the float64 argmin IS the constructed answer
    else:
        assert share <= UNDECIDED_CAP, (case.name, share)
    if case.family == "nan":
        assert [tuple(p) for p in np.argwhere(ref.nan)] == list(case.nan_at) and ref.best[0, 13] == 0


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_an_honest_float32_search_passes_the_rule(i):
    """The rule is satisfiable and the bound honest: numpy's float32 matmul, norms and bracket order obey it on every case."""
    case, ref = CASES[i], reference(i)
    g = vq_ref.search_f32(case.z, case.d)
    assert ref.violations(g) == []
    if case.expected is not None:
        assert np.array_equal(g, case.expected)
    for b, t in case.nan_at:
        assert g[b, t] == 0


@pytest.mark.parametrize("name", list(MUTANTS))
def test_the_rule_rejects_a_defective_search(name):
    """Each defect the issue lists, applied to the float32 model, is rejected by at least one case."""
    rejected = {}
    for i, case in enumerate(CASES):
        bad = reference(i).violations(vq_ref.mutant_answer(name, case))
        if bad:
            rejected.setdefault(case.family, []).append((case.name, len(bad)))
    print(f"{name}: rejected by {sum(len(v) for v in rejected.values())} cases in families {sorted(rejected)}")
    assert rejected, name
    want = {"partial last tile ignored": "every slot", "channels past the last full 64-channel chunk ignored": "grid",
            "last index on ties": "ties", "norms of a different dictionary": "grid", "slot k % 128 == 37 never chosen": "every slot"}
    assert want[name] in rejected, (name, sorted(rejected))  # the family built for this defect sees it


# ---------------------------------------------------------------- the entry points refuse bad sizes without a device
def test_embed_and_argmin_refuse_bad_arguments_without_a_device(lib_built):
    L = lib_built
    buf = (C.c_double * 16)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(a=p, b=p, c=p, B=2, Cd=8, T1=4, K=3)

    def call(fn, **kw):
        a = dict(ok, **kw)
        return fn(a["a"], a["b"], a["c"], a["B"], a["Cd"], a["T1"], a["K"], None)

    sizes = (dict(B=0), dict(B=-1), dict(Cd=0), dict(Cd=-4), dict(T1=0), dict(T1=-1), dict(K=0), dict(K=-2), dict(B=65536), dict(B=1 << 30))
    for bad in sizes + (dict(a=None), dict(b=None), dict(c=None), dict(Cd=65536), dict(Cd=1 << 30)):
        assert call(L.vqvs_vq_embed, **bad) == -1, bad
        assert L.vqvs_last_error(), bad
    for bad in sizes + (dict(a=None), dict(b=None), dict(c=None), dict(Cd=6)):
        assert call(L.vqvs_vq_argmin, **bad) == -1, bad
        assert L.vqvs_last_error(), bad
    assert call(L.vqvs_vq_embed, K=0) == -1 and b"K=0" in L.vqvs_last_error()
    assert call(L.vqvs_vq_embed, B=65536) == -1 and b"65536" in L.vqvs_last_error()
    assert call(L.vqvs_vq_embed, Cd=65536) == -1 and b"65536" in L.vqvs_last_error()
    assert call(L.vqvs_vq_embed, a=None) == -1 and b"non-NULL" in L.vqvs_last_error()
    assert call(L.vqvs_vq_argmin, B=65536) == -1 and b"65536" in L.vqvs_last_error()
    assert call(L.vqvs_vq_argmin, T1=0) == -1 and b"T1=0" in L.vqvs_last_error()
