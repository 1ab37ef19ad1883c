"""The counter-based normal generator of the library (csrc/philox.hpp), restated in numpy from the published algorithm: the
reference that tests/test_rng.py pins to the Philox known-answer vectors and tests/test_rng_gpu.py compares the kernels with.
It does not import the library.

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011): ten rounds of
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),
the key bumped by (W0, W1) after every round.

The generator's use of it:
    counter = (quad index within the clip, low word of the GLOBAL clip index, step index, stream id ^ (high clip word << 8))
    key     = (low seed word, high seed word)
    stream ids: 0 = the reverse step's noise, 1 = x_T, 2 = the forward process' epsilon
The four output words become four uniforms IN FLOAT32 -- words 0 and 2 on (0, 1] as ((c >> 8) + 0.5) * 2^-24, words 1 and 3 on
[0, 1) as (c >> 8) * 2^-24; the float32 rounding of the "+ 0.5" above 2^23 is part of the definition, and makes u = 1 (a radius
of 0) possible -- and two Box-Muller pairs, (r cos, r sin) with r = sqrt(-2 ln u) and the angle 2 pi u', evaluated here in float64.
Sample 4 q + j of a clip is component j of quad q.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)  # round multipliers
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)  # key increments (golden ratio, sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)
S32, S8 = np.uint64(32), np.uint64(8)
STREAM_STEP, STREAM_XT, STREAM_LOSS = 0, 1, 2


def _u64(v):
    """Python ints (up to 2^64 - 1) or integer arrays as uint64 arrays."""
    if isinstance(v, (int, np.integer)):
        return np.asarray(int(v) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    return np.asarray(v).astype(np.uint64)


def philox4x32_10(counter_words, key_words, rounds=10):
    """Four counter words and two key words (uint64 arrays masked to 32 bits, broadcast against each other) -> four output words."""
    c = [_u64(v) & MASK for v in counter_words]
    k0, k1 = (_u64(v) & MASK for v in key_words)
    for _ in range(rounds):
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [((p1 >> S32) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> S32) ^ c[3] ^ k1) & MASK, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def counter_words(quad, clip, step, stream):
    clip = _u64(clip)
    return [_u64(quad), clip & MASK, _u64(step), (_u64(stream) ^ ((clip >> S32) << S8)) & MASK]


def uniforms4(words):
    """The generator's four float32 uniforms: (0, 1], [0, 1), (0, 1], [0, 1)."""
    f, scale = np.float32, np.float32(1.0 / 16777216.0)
    mant = [(w >> S8).astype(f) for w in words]  # 24 bits: exact in float32
    return [(mant[0] + f(0.5)) * scale, mant[1] * scale, (mant[2] + f(0.5)) * scale, mant[3] * scale]


def normal4(seed, quad, clip, step, stream):
    """float64 [..., 4]: the four normals of quad `quad` of clip `clip` (arguments broadcast against each other)."""
    seed = _u64(seed)
    u = uniforms4(philox4x32_10(counter_words(quad, clip, step, stream), (seed & MASK, seed >> S32)))
    assert all(x.dtype == np.float32 for x in u)
    out = []
    for ur, ua in ((u[0], u[1]), (u[2], u[3])):
        r = np.sqrt(-2.0 * np.log(ur.astype(np.float64)))
        a = 2.0 * np.pi * ua.astype(np.float64)
        out += [r * np.cos(a), r * np.sin(a)]
    return np.stack(np.broadcast_arrays(*out), axis=-1)


def randn(B, T, seed, clip_offset, stream, step=0):
    """float64 [B, T]: row b is clip clip_offset + b; a tail of T % 4 samples takes the leading components of the last quad."""
    quads = np.arange((T + 3) // 4, dtype=np.uint64)[None, :]
    clips = np.asarray([(int(clip_offset) + b) & 0xFFFFFFFFFFFFFFFF for b in range(B)], dtype=np.uint64)[:, None]
    return normal4(seed, quads, clips, step, stream).reshape(B, -1)[:, :T]
