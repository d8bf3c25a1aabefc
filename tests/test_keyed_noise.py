"""The keyed noise generator on the host (oracle/keyed_noise.py, a numpy restatement of csrc/ddpm.h: Philox4x32-10 +
Box-Muller): published known answers of the block function, the distribution and the independence of the streams it
produces (thresholds from theory: every statistic is a fixed function of fixed keys, so the tests are deterministic), and
the key domain that include/diffsbdd_hip.h states.  tests/test_gpu_noise_and_steps.py compares the kernel with this
restatement element by element; here the restatement itself is pinned."""
import math

import numpy as np
import torch

from oracle import keyed_noise as kn

# the block every distribution test works on: seed 7, draw 3, stream 0, 64 samples x 400 rows x 13 columns
SEED, DRAW, STREAM = 7, 3, 0
B, ROWS, COLS = 64, 400, 13
N = B * ROWS * COLS

_cache = {}


def block(seed=SEED, draw=DRAW, stream=STREAM, dtype=np.float32):
    key = (seed, draw, stream, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = kn.randn_keyed(seed, draw, stream, None, [ROWS] * B, COLS, dtype)
    return _cache[key]


def corr(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


# ---- 1. the block function -----------------------------------------------------------------------------------------------
KNOWN_ANSWERS = [   # Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, output
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox4x32_10_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        got = tuple(int(w) for w in kn.philox4x32_10(ctr, key))
        assert got == want, ([hex(g) for g in got], [hex(w) for w in want])
    # vectorised: the three vectors in one call
    ctr = [np.array([k[0][i] for k in KNOWN_ANSWERS], dtype=np.uint64) for i in range(4)]
    key = [np.array([k[1][i] for k in KNOWN_ANSWERS], dtype=np.uint64) for i in range(2)]
    got = np.stack(kn.philox4x32_10(ctr, key), 1)
    assert got.tolist() == [list(k[2]) for k in KNOWN_ANSWERS]


def _philox_scalar(c, k):
    """Philox4x32-10 once more, on Python ints (an implementation that shares no code with the restatement)."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def _value_scalar(seed, draw, stream, gs, elem):
    """The header's contract for one value, in Python ints and the math module (double)."""
    ctr = [gs & 0xFFFFFFFF, elem, draw & 0xFFFFFFFF,
           (draw >> 32) ^ ((stream * 0x9E3779B1) & 0xFFFFFFFF) ^ (gs >> 32)]
    w = _philox_scalar(ctr, [seed & 0xFFFFFFFF, seed >> 32])
    u1 = ((w[0] >> 8) + 1) / 16777216.0
    u2 = (w[1] >> 8) / 16777216.0
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(float(np.float32(2.0 * math.pi)) * u2)


def test_randn_keyed_is_the_header_contract_value_by_value():
    """Every input of the key reaches the counter where the header says (which word, which half), words 0 and 1 feed u1
    and u2 in that order, and the element index is row_in_sample * n_cols + col with rows counted inside the sample."""
    assert _philox_scalar(KNOWN_ANSWERS[2][0], KNOWN_ANSWERS[2][1]) == list(KNOWN_ANSWERS[2][2])
    sizes, n_cols = [3, 0, 2, 5], 7
    cases = [dict(seed=7, draw=3, stream=0, ids=None, off=0),
             dict(seed=(0xDEADBEEF << 32) | 7, draw=(5 << 32) | 3, stream=0xFFFFFFFF, ids=None, off=(1 << 32) - 2),
             dict(seed=(1 << 64) - 1, draw=(1 << 64) - 1, stream=1, ids=[9, (3 << 32) | 1, 0, (1 << 63) - 1], off=0)]
    for c in cases:
        got64 = kn.randn_keyed(c["seed"], c["draw"], c["stream"], c["ids"], sizes, n_cols, np.float64, c["off"])
        got32 = kn.randn_keyed(c["seed"], c["draw"], c["stream"], c["ids"], sizes, n_cols, np.float32, c["off"])
        assert got64.shape == got32.shape == (sum(sizes), n_cols)
        assert got64.dtype == np.float64 and got32.dtype == np.float32
        want, row = np.empty_like(got64), 0
        for b, n in enumerate(sizes):
            gs = c["ids"][b] if c["ids"] is not None else b + c["off"]
            for r in range(n):
                for col in range(n_cols):
                    want[row, col] = _value_scalar(c["seed"], c["draw"], c["stream"], gs, r * n_cols + col)
                row += 1
        # same formula in double: libm against numpy, a few ulp of double at most
        assert np.abs(got64 - want).max() <= 1e-13, np.abs(got64 - want).max()
        # the float32 mode differs from the float64 mode by rounding only
        assert np.abs(got32.astype(np.float64) - got64).max() <= 4e-6


def test_box_muller_ends_of_the_uniform_ranges():
    """u1 = ((w0 >> 8) + 1) / 2^24 lies in (0, 1]: the smallest word gives the largest finite |z| = sqrt(48 ln 2), the
    largest gives exactly 0; u2 = (w1 >> 8) / 2^24 lies in [0, 1): the low 8 bits of either word are unused."""
    u1, u2 = kn.uniforms(np.array([0, 255, 256, 0xFFFFFFFF]), np.array([0, 255, 256, 0xFFFFFFFF]))
    assert u1.tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0]
    assert u2.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]
    for dt in (np.float32, np.float64):
        z = kn.box_muller(np.array([0, 0xFFFFFFFF, 0]), np.array([0, 12345, 0x80000000]), dt)
        assert np.isfinite(z).all()
        assert abs(float(z[0]) - math.sqrt(48.0 * math.log(2.0))) <= 1e-6 and float(z[1]) == 0.0
        assert abs(float(z[2]) + math.sqrt(48.0 * math.log(2.0))) <= 1e-5        # cos(pi) = -1
    assert abs(kn.MAX_ABS - math.sqrt(48.0 * math.log(2.0))) < 1e-15


# ---- 2. distribution of the restatement ---------------------------------------------------------------------------------
def test_moments_and_tail():
    z = block().astype(np.float64).reshape(-1)
    assert z.size == N == 332800
    assert np.isfinite(z).all() and np.abs(z).max() <= kn.MAX_ABS
    mean, std, m4 = z.mean(), z.std(), (z ** 4).mean()
    print(f"  mean {mean * math.sqrt(N):+.2f} sigma, std {(std - 1) * math.sqrt(2 * N):+.2f} sigma, "
          f"E z^4 - 3 = {m4 - 3:+.4f} (bound {4 * math.sqrt(96 / N):.4f})")
    assert abs(mean) <= 4 / math.sqrt(N)
    assert abs(std - 1.0) <= 4 / math.sqrt(2 * N)
    assert abs(m4 - 3.0) <= 4 * math.sqrt(96 / N)           # var(z^4) = E z^8 - 9 = 96
    z64 = block(dtype=np.float64).reshape(-1)
    assert np.isfinite(z64).all() and np.abs(z64).max() <= kn.MAX_ABS


def test_kolmogorov_smirnov_against_the_normal_cdf():
    z = torch.from_numpy(np.sort(block().astype(np.float64).reshape(-1)))
    cdf = 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))
    i = torch.arange(1, N + 1, dtype=torch.float64)
    d = float(torch.maximum(i / N - cdf, cdf - (i - 1) / N).max())
    print(f"  sqrt(N) D = {math.sqrt(N) * d:.3f}")
    assert math.sqrt(N) * d <= 1.95                          # 0.1 % point of the Kolmogorov distribution


def test_no_correlation_inside_a_sample_or_between_samples():
    z = block().astype(np.float64).reshape(B, ROWS * COLS)
    r1 = corr(z[:, :-1], z[:, 1:])                           # lag 1 over the element index, pairs inside a sample
    print(f"  lag-1 |r| sqrt(N) = {abs(r1) * math.sqrt(N):.2f}")
    assert abs(r1) * math.sqrt(N) <= 4
    c = np.corrcoef(z)
    off = np.abs(c[np.triu_indices(B, 1)])
    assert off.size == 2016
    print(f"  largest sample-against-sample |r| sqrt(5200) = {off.max() * math.sqrt(ROWS * COLS):.2f}")
    assert off.max() * math.sqrt(ROWS * COLS) <= math.sqrt(2 * math.log(2016)) + 1.5


VARIANTS = {"draw 4": dict(draw=4), "stream 1": dict(stream=1), "seed 8": dict(seed=8),
            "seed 7 + 2^32": dict(seed=7 + 2 ** 32), "draw 3 + 2^32": dict(draw=3 + 2 ** 32)}


def test_every_key_input_gives_an_unrelated_block():
    base = block()
    blocks = {"base": base}
    for name, kw in VARIANTS.items():
        v = block(**kw)
        r = corr(base, v)
        print(f"  {name}: |r| sqrt(N) = {abs(r) * math.sqrt(N):.2f}")
        assert abs(r) * math.sqrt(N) <= 4, name
        blocks[name] = v
    # no two of the six blocks share one equal element, in the float32 values and in the float64 mode (where a value
    # is determined by its pair of uniforms)
    names = list(blocks)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            kw_a, kw_b = VARIANTS.get(a, {}), VARIANTS.get(b, {})
            assert not (blocks[a] == blocks[b]).any(), (a, b)
            assert not (block(dtype=np.float64, **kw_a) == block(dtype=np.float64, **kw_b)).any(), (a, b)


# ---- 3. the key domain ---------------------------------------------------------------------------------------------------
def test_counter_mapping_is_injective_inside_the_domain():
    """include/diffsbdd_hip.h: distinct (seed, draw, stream, sample id, element) give distinct (counter, key) as long as
    draw_index < 2^32 and sample id < 2^32.  Checked on the grid of the edge values of every input (all combinations) and
    on the argument that makes it general: in the domain word 3 is stream_id * 0x9E3779B1 mod 2^32 alone, an odd
    multiplier, and the other five words are the remaining inputs verbatim."""
    seeds = [0, 1, 7, 2 ** 32 - 1, 2 ** 32, 7 + 2 ** 32, 2 ** 63, 2 ** 64 - 1]
    draws = [0, 1, 3, 2 ** 31, 2 ** 32 - 1]
    streams = [0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    ids = [0, 1, 63, 2 ** 31, 2 ** 32 - 1]
    elems = [0, 1, 12, 2 ** 16, 2 ** 32 - 1]
    g = np.meshgrid(*(np.array(v, dtype=np.uint64) for v in (seeds, draws, streams, ids, elems)), indexing="ij")
    ctr, key = kn.counter_words(*(a.reshape(-1) for a in g))
    words = np.stack([*ctr, *key], 1)
    assert words.max() < 2 ** 32
    assert len(np.unique(words, axis=0)) == len(seeds) * len(draws) * len(streams) * len(ids) * len(elems)
    # the verbatim words, and word 3 as a function of the stream alone
    flat = [a.reshape(-1) for a in g]
    assert (ctr[0] == flat[3]).all() and (ctr[1] == flat[4]).all() and (ctr[2] == flat[1]).all()
    assert (key[0] == (flat[0] & kn.M32)).all() and (key[1] == (flat[0] >> np.uint64(32))).all()
    assert (ctr[3] == (flat[2] * kn.STREAM_MUL) & kn.M32).all()
    assert int(kn.STREAM_MUL) % 2 == 1                       # odd => a bijection of the 32-bit stream ids
    s = np.arange(1 << 16, dtype=np.uint64) * np.uint64(65537)         # 65 536 stream ids spread over the 32 bits
    assert len(np.unique(kn.counter_words(0, 0, s, 0, 0)[0][3])) == s.size
    # distinct outputs too, on a slice of that grid
    sizes = [2] * 3
    seen = set()
    for seed in (7, 7 + 2 ** 32):
        for draw in (3, 2 ** 32 - 1):
            for stream in (0, 1, 0xFFFFFFFF):
                z = kn.randn_keyed(seed, draw, stream, [0, 63, 2 ** 32 - 1], sizes, 13, np.float64)
                seen.update(z.reshape(-1).tolist())
    assert len(seen) == 2 * 2 * 3 * 6 * 13


def test_documented_alias_outside_the_domain():
    """Word 3 of the counter is draw_hi ^ stream_id * 0x9E3779B1 ^ gs_hi, so the high halves of the draw index and of the
    sample id alias: (draw + 2^32, gs) and (draw, gs + 2^32) are one stream.  Harmless where the project works (draws
    and sample ids below 2^32) and stated next to dsbdd_randn_keyed."""
    sizes, cols = [5, 3], 13
    a = kn.randn_keyed(SEED, DRAW + 2 ** 32, 0, [11, 12], sizes, cols)
    b = kn.randn_keyed(SEED, DRAW, 0, [11 + 2 ** 32, 12 + 2 ** 32], sizes, cols)
    c = kn.randn_keyed(SEED, DRAW, 0, [11, 12], sizes, cols)
    assert np.array_equal(a, b) and not (a == c).any()
    wa = kn.counter_words(SEED, DRAW + 2 ** 32, 0, 11, 4)
    wb = kn.counter_words(SEED, DRAW, 0, 11 + 2 ** 32, 4)
    assert [int(w) for w in wa[0] + wa[1]] == [int(w) for w in wb[0] + wb[1]]
    # the stream id can cancel a high half as well: stream * 0x9E3779B1 = 1 (mod 2^32) for the multiplier's inverse
    inv = pow(0x9E3779B1, -1, 2 ** 32)
    wc = kn.counter_words(SEED, DRAW + 2 ** 32, inv, 11, 4)
    wd = kn.counter_words(SEED, DRAW, 0, 11, 4)
    assert [int(w) for w in wc[0] + wc[1]] == [int(w) for w in wd[0] + wd[1]]
    # both halves of the seed are the key: no alias there
    assert not (kn.randn_keyed(SEED + 2 ** 32, DRAW, 0, [11, 12], sizes, cols) == c).any()
