"""The numpy reference of the counter-based normal generator (tests/philox_ref.py) on its own: the published Philox4x32-10
known-answer vectors, the moments of its normals, and that every word of (seed, quad, clip, step, stream) reaches the draw.
tests/test_rng_gpu.py holds the compiled kernels to this reference; nothing here needs the library or a GPU."""
import itertools

import numpy as np

import philox_ref

# counter, key, output: the known-answer vectors of the Random123 distribution (kat_vectors, "philox4x32 10")
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_known_answer_vectors():
    for counter, key, want in KAT:
        got = tuple(int(w) for w in philox_ref.philox4x32_10(counter, key))
        assert got == want, ([hex(w) for w in got], [hex(w) for w in want])
        # the vectors pin the round count too
        assert tuple(int(w) for w in philox_ref.philox4x32_10(counter, key, rounds=9)) != want
    # vectorised over counter and key: the same words as one at a time
    c = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    key = [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    got = philox_ref.philox4x32_10(c, key)
    assert [tuple(int(w[j]) for w in got) for j in range(3)] == [k[2] for k in KAT]


def test_uniform_edges_are_the_float32_definition():
    top, f = np.uint64(0xFFFFFFFF), np.float32
    u = philox_ref.uniforms4([np.array([0, 0xFF, 0x100, top], dtype=np.uint64)] * 4)
    assert all(x.dtype == np.float32 for x in u)
    # (0, 1]: the smallest value is 2^-25; 16777215.5 is no float32 and rounds (to even) to 2^24, so the largest is 1
    assert u[0].tolist() == [f(2.0 ** -25), f(2.0 ** -25), f(1.5 * 2.0 ** -24), f(1.0)] and u[2].tolist() == u[0].tolist()
    # [0, 1): 0 up to 1 - 2^-24
    assert u[1].tolist() == [0.0, 0.0, f(2.0 ** -24), f(1.0 - 2.0 ** -24)] and u[3].tolist() == u[1].tolist()


def test_reference_normals_have_standard_moments():
    """2^20 quads (n = 2^22 values) of one clip, the draw behind the figures quoted with the reference: seed 5, clip 3, stream 1.
    Mean and variance are within 5 / sqrt(n) = 2.4e-3 of 0 and 1 (measured 1.8e-4 and 2.1e-4).  The fourth moment's estimator
    has variance E z^8 - (E z^4)^2 = 96 over n: 5 / sqrt(n) on m4 - 3 itself would be a band of half a standard error that a
    perfect generator misses three times in five (this draw measures 3.0055), so the same 5 / sqrt(n) is applied to the
    standardised (m4 - 3) / sqrt(96), as it is -- with unit variance -- to the mean."""
    nq = 1 << 20
    z = philox_ref.normal4(5, np.arange(nq, dtype=np.uint64), 3, 0, philox_ref.STREAM_XT)
    assert z.shape == (nq, 4) and z.dtype == np.float64
    assert np.isfinite(z).all()
    n = z.size
    mean, var, m4 = z.mean(), z.var(), (z ** 4).mean()
    print(f"[moments] n = {n}: mean {mean:.3e}, var - 1 {var - 1:.3e}, m4 - 3 {m4 - 3:.3e}; 5 / sqrt(n) = {5 / n ** 0.5:.3e}")
    assert abs(mean) <= 5 / n ** 0.5
    assert abs(var - 1) <= 5 / n ** 0.5
    assert abs(m4 - 3) / 96 ** 0.5 <= 5 / n ** 0.5
    # the four components of a quad are four draws, not two: no pair is correlated
    corr = np.corrcoef(z.T)
    assert np.abs(corr - np.eye(4)).max() <= 5 / nq ** 0.5
    # randn lays the quads out along the row and cuts the tail
    row = philox_ref.randn(2, 4099, 5, 2, philox_ref.STREAM_XT)
    assert row.shape == (2, 4099) and np.array_equal(row[1], z[:1025].reshape(-1)[:4099])


BASE = dict(seed=(7 << 32) | 5, quad=11, clip=(2 << 32) | 3, step=4, stream=1)
CHANGES = {
    "seed low word": dict(seed=(7 << 32) | 6),
    "seed high word": dict(seed=(8 << 32) | 5),
    "quad": dict(quad=12),
    "clip low word": dict(clip=(2 << 32) | 4),
    "clip high word": dict(clip=((2 << 32) | 3) + (1 << 32)),
    "step": dict(step=5),
    "stream": dict(stream=2),
}


def test_every_word_reaches_the_draw():
    base = philox_ref.normal4(**BASE)
    assert base.shape == (4,)
    draws = {"base": base}
    for name, change in CHANGES.items():
        draws[name] = philox_ref.normal4(**dict(BASE, **change))
    # all eight draws differ from each other in every component (equal components of two draws have probability ~2^-24)
    for (na, a), (nb, b) in itertools.combinations(draws.items(), 2):
        assert (a != b).all(), (na, nb, a, b)
    # ... also from zero: a dropped high word is the same as a zero one
    assert (philox_ref.normal4(5, 0, 0, 0, 0) != philox_ref.normal4(5 | (1 << 32), 0, 0, 0, 0)).all()
    assert (philox_ref.normal4(5, 0, 0, 0, 0) != philox_ref.normal4(5, 0, 1 << 32, 0, 0)).all()
    # rows of randn: consecutive clips, steps and streams are different draws
    a = philox_ref.randn(2, 9, 5, 0, 0, step=0)
    assert not np.array_equal(a[0], a[1])
    assert not np.array_equal(a, philox_ref.randn(2, 9, 5, 0, 0, step=1))
    assert not np.array_equal(a, philox_ref.randn(2, 9, 5, 0, 1, step=0))
    assert np.array_equal(a[1], philox_ref.randn(1, 9, 5, 1, 0)[0])


def test_stream_word_does_not_collide_across_high_clip_words():
    words = {}
    for stream, hi in itertools.product((0, 1, 2), range(4)):
        w = int(philox_ref.counter_words(0, hi << 32, 0, stream)[3])
        assert w == stream ^ (hi << 8)
        assert w not in words, (stream, hi, words[w])
        words[w] = (stream, hi)
    assert len(words) == 12
