"""Host restatement of the keyed noise generator (csrc/ddpm.h: randn_keyed_value / randn_keyed_kernel), numpy only.

Written from the algorithm of the paper (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
SC 2011 -- Philox4x32-10) and from the contract that include/diffsbdd_hip.h states for dsbdd_randn_keyed:

  value(seed, draw_index, stream_id, global sample id gs, element index e inside the sample's [rows][n_cols] block)
    key     = (seed & 0xffffffff, seed >> 32)
    counter = (gs & 0xffffffff, e, draw_index & 0xffffffff, (draw_index >> 32) ^ (stream_id * 0x9E3779B1) ^ (gs >> 32))
    w       = philox4x32_10(counter, key)
    u1      = ((w[0] >> 8) + 1) / 2^24   in (0, 1]       u2 = (w[1] >> 8) / 2^24   in [0, 1)
    z       = sqrt(-2 ln u1) * cos(2 pi u2)              (2 pi rounded to float32)

Two arithmetic modes: float32 rounds every operation to float32 (what the kernel does, up to its logf / cosf); float64
evaluates the same formula in double from the same exact uniforms and the same float32-rounded 2 pi, so the two modes
differ by rounding alone.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0 = np.uint64(0xD2511F53)
PHILOX_M1 = np.uint64(0xCD9E8D57)
PHILOX_W0 = np.uint64(0x9E3779B9)     # key increments ("Weyl" constants: golden ratio, sqrt(3) - 1)
PHILOX_W1 = np.uint64(0xBB67AE85)
STREAM_MUL = np.uint64(0x9E3779B1)    # odd: stream_id -> stream_id * STREAM_MUL mod 2^32 is a bijection
TWO_PI_F32 = np.float32(6.28318530717958647692)
# |z| <= sqrt(-2 ln 2^-24): the tail the 24-bit u1 allows
MAX_ABS = float(np.sqrt(48.0 * np.log(2.0)))


def _u64(v):
    """Python ints (of any sign, reduced mod 2^64) or integer arrays -> uint64 array."""
    if isinstance(v, (int, np.integer)):
        return np.uint64(int(v) & 0xFFFFFFFFFFFFFFFF)
    a = np.asarray(v)
    if a.dtype == np.uint64:
        return a
    if a.dtype == object:
        return np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in a.reshape(-1)], dtype=np.uint64).reshape(a.shape)
    return a.astype(np.int64).view(np.uint64) if a.dtype.kind == "i" else a.astype(np.uint64)


def philox4x32_10(ctr, key):
    """ctr: 4 words, key: 2 words (scalars or broadcastable integer arrays, each < 2^32) -> tuple of 4 uint64 arrays
    holding the 32-bit output words.  uint64 arithmetic masked to 32 bits."""
    c0, c1, c2, c3 = (_u64(c) & M32 for c in ctr)
    k0, k1 = (_u64(k) & M32 for k in key)
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0 = PHILOX_M0 * c0            # 32 x 32 -> 64 bit products: no overflow in uint64
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def counter_words(seed, draw_index, stream_id, gs, elem):
    """The (counter[4], key[2]) that the generator feeds to Philox for one value.  seed, draw_index, gs: 64 bit;
    stream_id, elem: 32 bit.  Arrays broadcast."""
    seed, draw, gs = _u64(seed), _u64(draw_index), _u64(gs)
    stream, elem = _u64(stream_id) & M32, _u64(elem) & M32
    s32 = np.uint64(32)
    c3 = (draw >> s32) ^ ((stream * STREAM_MUL) & M32) ^ (gs >> s32)
    return (gs & M32, elem, draw & M32, c3), (seed & M32, seed >> s32)


def uniforms(w0, w1):
    """The two 24-bit uniforms as exact float64: u1 in (0, 1], u2 in [0, 1)."""
    u1 = ((_u64(w0) >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (_u64(w1) >> np.uint64(8)).astype(np.float64) / 16777216.0
    return u1, u2


def box_muller(w0, w1, dtype=np.float32):
    """One normal from output words 0 and 1, in float32 (every operation rounded) or float64 arithmetic."""
    dtype = np.dtype(dtype)
    u1, u2 = uniforms(w0, w1)            # exact in either format (24 bits)
    if dtype == np.float32:
        u1, u2 = u1.astype(np.float32), u2.astype(np.float32)
        r = np.sqrt(np.float32(-2.0) * np.log(u1), dtype=np.float32)
        return (r * np.cos(TWO_PI_F32 * u2, dtype=np.float32)).astype(np.float32)
    if dtype == np.float64:
        return np.sqrt(-2.0 * np.log(u1)) * np.cos(np.float64(TWO_PI_F32) * u2)
    raise ValueError("dtype must be float32 or float64")


def randn_keyed(seed, draw_index, stream_id, sample_ids, sizes, n_cols, dtype=np.float32, sample_offset=0):
    """The [sum(sizes)][n_cols] block dsbdd_randn_keyed writes for a batch whose sample b has sizes[b] rows.
    Global sample id of sample b: sample_ids[b] when sample_ids is not None, else b + sample_offset."""
    sizes = [int(s) for s in sizes]
    n_cols = int(n_cols)
    if sample_ids is None:
        gs_of = [(b + int(sample_offset)) & 0xFFFFFFFFFFFFFFFF for b in range(len(sizes))]
    else:
        gs_of = [int(s) & 0xFFFFFFFFFFFFFFFF for s in sample_ids]
        assert len(gs_of) == len(sizes)
    gs = np.repeat(np.array(gs_of, dtype=np.uint64), [s * n_cols for s in sizes])
    elem = np.concatenate([np.arange(s * n_cols, dtype=np.uint64) for s in sizes] + [np.zeros(0, dtype=np.uint64)])
    ctr, key = counter_words(seed, draw_index, stream_id, gs, elem)
    w = philox4x32_10(ctr, key)
    return box_muller(w[0], w[1], dtype).reshape(sum(sizes), n_cols)
