"""The node chain's second row split (csrc/chain_split.h ChainDeal, DSBDD_OPT_CHAIN_DEAL; DESIGN.md §5 "Min-max deal") as
compiled: dsbdd_chain_deal_host runs the kernel's own text on the host.  No GPU.

Checked on the 722 listed cases of tests/_chain_split_cases (H = 256 and 128), on the five LARGE row counts and on the six
node-chain launches of a headline call at grid 256:
  * coverage: every 16-row tile of [0, ceil(Mw / 16)) lies in exactly one piece of 1 - 6 tiles.  The policy's 32-bit sums
    (tiles x at most 240 units) hold for every row count the entry points accept, so all five LARGE counts are covered;
    FIRST_ROWS_32BIT_CANNOT_HOLD is where tiles x 240 would pass 2^32, far behind the 8 388 608 rows the launch takes;
  * no straddle: no piece has a problem's start (rounded down to a tile) or end (rounded up) in its interior;
  * slowest load, by chain_range's own rule (a piece multiplies ALL its tiles for every projection it touches): at most the
    old split's on every listed case, at most the issue's no-straddle min-max figures on the six benchmark launches;
  * brute force: on small cases the bottleneck equals the optimum of the restricted problem (contiguous ranges, none across
    a cut, at most `grid` of them), computed here by a dynamic programme over the segments.
The fallback is a pure function of the counts (8 x segments > grid and tiles >= 3 x grid: the old split's forced path deals
the launch, which cuts at the same boundaries) and is part of every check: its pieces must be the old split's."""
import ctypes as C

import numpy as np
import pytest

from diffsbdd_amd import _lib
from tests import _chain_split_cases as cs

# tiles x 240 units (H = 128, node MLP and three 512-column projections) reaches 2^32 at 17 895 698 tiles
FIRST_ROWS_32BIT_CANNOT_HOLD = ((2**32 + 239) // 240 - 1) * 16 + 1
ROWS_MAX = 8 << 20                                   # what launch_node_chain and the entry points accept

# the six node-chain launches of a headline call (crossdock_fullatom_cond x 64: levels of 1 472 / 3 639 / 11 545 / 18 764
# rows, 286 ghost rows in front of the ghost stages' lists) and the issue's bound on their slowest workgroup
BENCH = [((3639 + 286, 256, True, [(512, 3639, 286), (512, 1472, 286), (512, None, 0)]), 2304),
         ((11545 + 286, 256, True, [(512, 3639, 286), (512, 1472, 286), (512, None, 0)]), 5120),
         ((18764 + 286, 256, True, [(512, 3639, 286), (512, 1472, 286), (512, None, 0)]), 7680),
         ((18764, 256, True, [(512, 3639, 0), (512, 1472, 0), (512, None, 0)]), 7168),
         ((11545, 256, True, [(512, 3639, 0), (512, 1472, 0), (512, None, 0)]), 5120),
         ((3639, 256, True, [(512, 3639, 0), (512, 1472, 0)]), 1792)]


def deal_split(lib, M, grid, do_mlp, projs, H=256):
    """dsbdd_chain_deal_host: (pieces int32 [n][3] = (workgroup, first row, tiles), header (Mw, B, grid, Vs, fallback))."""
    n = len(projs)
    arr = lambda v: (C.c_int32 * 3)(*(list(v) + [0] * (3 - n)))
    pn, pf = arr([p[0] for p in projs]), arr([p[2] for p in projs])
    pc = arr([cs.ALL_ROWS if p[1] is None else p[1] for p in projs])
    header = (C.c_uint32 * 5)()
    args = (M, int(do_mlp), n, pn, pf, pc, H, grid, header)
    count = lib.dsbdd_chain_deal_host(*args, None, 0)
    assert count >= 0, count
    pieces = np.zeros((count, 3), dtype=np.int32)
    assert lib.dsbdd_chain_deal_host(*args, pieces.ctypes.data_as(C.c_void_p), count) == count
    return pieces, tuple(int(x) for x in header)


def problems(M, projs, H):
    """[(first, end, weight)] as chain_range sees them: first as given, the count clamped as the split clamps it."""
    out = []
    for n, cnt, first in projs:
        fst = min(M, first)
        c = max(min(M - fst, cs.ALL_ROWS if cnt is None else cnt), 0)
        out.append((first, first + c, n * 16 // H))
    return out


def piece_load(r0, take, do_mlp, probs):
    """Executed load of a piece by chain_range's rule: the node MLP and every projection it touches, on ALL its tiles."""
    load = 48 if do_mlp else 0
    for lo, end, w in probs:
        if not (r0 >= end or r0 + 16 * take <= lo):
            load += w
    return 16 * take * load


def slowest(flat, grid, do_mlp, probs):
    loads = np.zeros(grid, dtype=np.int64)
    for wg, r0, take in flat.tolist():
        loads[wg] += piece_load(r0, take, do_mlp, probs)
    return int(loads.max()) if len(flat) else 0


def cuts_in_tiles(n_tiles, probs, empty=True):
    """Starts (rounded down to a tile) and ends (rounded up) of the problems.  empty: also of a problem without rows, whose
    projection chain_range still runs on the tile around its first row."""
    cuts = {0, n_tiles}
    for lo, end, _ in probs:
        if lo >> 4 < n_tiles and (empty or end > lo):
            cuts.add(lo >> 4)
            cuts.add(min(n_tiles, (end + 15) >> 4))
    return sorted(cuts)


def check_cover_and_straddle(flat, Mw, probs, what):
    n_tiles = (Mw + 15) // 16
    if len(flat) == 0:
        assert Mw == 0, what
        return
    r0, take = flat[:, 1].astype(np.int64), flat[:, 2].astype(np.int64)
    assert (r0 % 16 == 0).all() and (take >= 1).all() and (take <= 6).all(), what
    t0 = r0 // 16
    seen = np.zeros(n_tiles + 1, dtype=np.int64)
    assert t0.min() >= 0 and (t0 + take).max() <= n_tiles, what
    np.add.at(seen, t0, 1)
    np.add.at(seen, t0 + take, -1)
    assert (np.cumsum(seen)[:n_tiles] == 1).all(), what
    for c in cuts_in_tiles(n_tiles, probs, empty=False):
        assert not ((t0 < c) & (c < t0 + take)).any(), (what, c)


def restricted_optimum(n_tiles, do_mlp, probs, G):
    """min over (ranges per segment, at most G in all) of the slowest range: ranges are runs of tiles inside one segment."""
    cuts = cuts_in_tiles(n_tiles, probs)
    segs = [(b - a, piece_load(16 * a, 1, do_mlp, probs)) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    INF = float("inf")
    best = [0] + [INF] * G                            # best[n]: slowest range with exactly n ranges so far
    for T, c in segs:
        nxt = [INF] * (G + 1)
        for used, worst in enumerate(best):
            if worst == INF:
                continue
            for n in range(1, min(T, G - used) + 1):
                nxt[used + n] = min(nxt[used + n], max(worst, c * -(-T // n)))
        best = nxt
    return min(best), len(segs)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("H", cs.HS)
def test_listed_cases_cover_do_not_straddle_and_are_no_slower_than_the_old_split(lib, H):
    n_fallback = n_better = 0
    for case in cs.listed_cases():
        M, grid, do_mlp, projs = case
        what = (case, H)
        probs = problems(M, projs, H)
        flat, (Mw, B, G, Vs, fallback) = deal_split(lib, *case, H=H)
        old_flat, old_header = cs.host_split(lib, *case, H=H)
        assert Mw == old_header[0] and G == (grid if Mw else 0), what  # the same rows have work
        check_cover_and_straddle(flat, Mw, probs, what)
        new, old = slowest(flat, grid, do_mlp, probs), slowest(old_flat, grid, do_mlp, probs)
        print(what, "slowest executed: deal", new, "old", old, "fallback", fallback)
        assert new <= old, what
        if fallback:
            assert old_header[4] and np.array_equal(flat, old_flat) and Vs == old_header[3], what
        elif Vs <= grid:
            assert new == B, what                                      # one range per workgroup
        n_fallback += fallback
        n_better += new < old
    # neither branch is vacuous: the narrow grids of the small random cases fall back, and at least the three NAMED launches
    # whose ranges straddle under the old split (ghost rows in front, 11 545 and 3 639 rows) come out ahead
    assert 0 < n_fallback < len(cs.listed_cases()) and n_better >= 3


@pytest.mark.parametrize("H", cs.HS)
def test_large_row_counts_are_covered_up_to_the_launch_limit(lib, H):
    assert cs.LARGE[-1][0] == ROWS_MAX < FIRST_ROWS_32BIT_CANNOT_HOLD
    assert (FIRST_ROWS_32BIT_CANNOT_HOLD + 15) // 16 * 240 >= 2**32 > (FIRST_ROWS_32BIT_CANNOT_HOLD - 1 + 15) // 16 * 240
    for case in cs.LARGE:
        M, grid, do_mlp, projs = case
        probs = problems(M, projs, H)
        flat, (Mw, B, G, Vs, fallback) = deal_split(lib, *case, H=H)
        assert Mw == M and not fallback and Vs <= grid
        check_cover_and_straddle(flat, Mw, probs, (case, H))
        assert slowest(flat, grid, do_mlp, probs) == B
    h5 = (C.c_uint32 * 5)()
    assert lib.dsbdd_chain_deal_host(ROWS_MAX + 1, 1, 0, None, None, None, H, 256, h5, None, 0) == _lib.ERR_ARG


def test_benchmark_launches_meet_the_no_straddle_min_max(lib):
    for case, bound in BENCH:
        M, grid, do_mlp, projs = case
        probs = problems(M, projs, 256)
        flat, (Mw, B, G, Vs, fallback) = deal_split(lib, *case)
        old_flat, _ = cs.host_split(lib, *case)
        check_cover_and_straddle(flat, Mw, probs, case)
        new, old = slowest(flat, grid, do_mlp, probs), slowest(old_flat, grid, do_mlp, probs)
        print(case, "tiles", (Mw + 15) // 16, "ranges", Vs, "slowest executed: deal", new, "old", old, "bound", bound)
        assert not fallback and new == B and new <= bound and new <= old, case


@pytest.mark.parametrize("H", cs.HS)
def test_small_cases_reach_the_optimum_of_the_restricted_problem(lib, H):
    n = n_search = 0
    for case in cs.small_random_cases() + cs.edge_host_cases():
        M, grid, do_mlp, projs = case
        if grid > 8 or (M + 15) // 16 > 100:
            continue
        probs = problems(M, projs, H)
        flat, (Mw, B, G, Vs, fallback) = deal_split(lib, *case, H=H)
        if Mw == 0:
            assert len(flat) == 0
            continue
        n_tiles = (Mw + 15) // 16
        # the fallback is a pure function of the counts
        n_segs = restricted_optimum(n_tiles, do_mlp, probs, 1000)[1]
        assert fallback == (8 * n_segs > grid and n_tiles >= 3 * grid), (case, H)
        n += 1
        if fallback:
            assert np.array_equal(flat, cs.host_split(lib, *case, H=H)[0]), (case, H)
        elif n_tiles <= grid or n_segs > grid:
            assert Vs == n_tiles and (flat[:, 2] == 1).all(), (case, H)   # every tile a range of its own, in rounds
            assert flat[:, 0].tolist() == sorted(t % grid for t in range(n_tiles)), (case, H)
        else:
            best, _ = restricted_optimum(n_tiles, do_mlp, probs, grid)
            assert B == best == slowest(flat, grid, do_mlp, probs) and Vs <= grid, (case, H, B, best)
            n_search += 1
    assert n > 150 and n_search > 20, (n, n_search)


def test_argument_checks_are_those_of_the_split_entry_point(lib):
    z3, h5 = (C.c_int32 * 3)(), (C.c_uint32 * 5)()
    ok = dict(M=32, n_proj=0, H=256, grid=1, header=h5, pieces=z3, cap=1)
    assert lib.dsbdd_chain_deal_host(32, 1, 0, z3, z3, z3, 256, 1, h5, z3, 1) == 1
    for bad in (dict(header=None), dict(pieces=None), dict(grid=0), dict(H=100), dict(H=0), dict(n_proj=4),
                dict(n_proj=-1), dict(M=ROWS_MAX + 1), dict(cap=-1)):
        a = {**ok, **bad}
        assert lib.dsbdd_chain_deal_host(a["M"], 1, a["n_proj"], z3, z3, z3, a["H"], a["grid"], a["header"], a["pieces"],
                                         a["cap"]) == _lib.ERR_ARG, bad
