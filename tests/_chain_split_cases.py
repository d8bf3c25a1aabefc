"""Cases of the node chain's row split (csrc/chain_split.h), shared by the recorder of tests/golden/chain_split_parent.npz
and the tests that compare against it.  A case is (M, grid, do_mlp, [(N columns, count or None = all that follow, first)]);
M is what the kernel has after min(M, *m_count)."""
import ctypes as C
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_split_parent.npz")
ALL_ROWS = 2**31 - 1              # kChainAllRows: "the problem covers all rows that follow"
HS = (256, 128)                   # every case is recorded with both weights (48 : N * 16 / H)

NAMED = [(19776, 256, True, [(512, 3639, 0), (512, 1472, 0), (512, None, 0)]),        # all rows, full chain
         (18764 + 286, 256, True, [(512, 3639, 286), (512, 1472, 286), (512, None, 0)]),  # ghost rows in front
         (11545, 256, True, [(512, 3639, 0), (512, 1472, 0)]), (3639, 256, True, [(512, 3639, 0), (512, 1472, 0)]),
         (19776, 256, False, [(512, None, 0)]), (1888, 256, True, [(512, None, 0)]), (5, 256, True, []),
         (40000, 256, True, [(512, None, 0)])]

# (M, *m_count or None, grid, do_mlp, projections): the smallest shapes that reach every path of the split
EDGE = [(32, None, 1, True, []),                                        # plain path, one workgroup
        (47, None, 1, True, []),                                        # forced path, smallest (3 tiles on 1 workgroup)
        (368, None, 8, True, []),                                       # 23 tiles: just below the forced threshold
        (376, None, 8, True, []),                                       # 24 tiles: just at it
        (400, None, 8, True, [(512, 100, 32), (512, None, 0)]),         # ghost-row offset
        (2000, None, 8, True, [(512, 700, 96), (512, 300, 96), (512, None, 0)]),   # 3 projections, 4 ranges per workgroup
        (400, None, 8, False, [(512, None, 0)]),                        # projections only
        (1, None, 8, False, [(512, 0, 0)]),                             # nothing to do
        (100, None, 8, False, []),                                      # nothing to do
        (5, None, 256, True, []),                                       # far fewer rows than workgroups
        (400, 300, 8, True, [(512, None, 0)]),                          # *m_count bites
        (400, None, 8, True, [(512, 1000, 100)]),                       # a *count larger than the rows that remain
        (400, None, 8, True, [(512, 50, 500), (512, None, 0)])]         # a first beyond M

LARGE = [(600000, 256, True, [(512, 3639, 0), (512, 1472, 0), (512, None, 0)]),
         (1000000, 256, True, [(512, 3639, 0), (512, 1472, 0), (512, None, 0)]),
         (2000000, 256, True, [(512, 3639, 0), (512, 1472, 0), (512, None, 0)]),
         (4000000, 256, True, [(512, 3639, 0), (512, 1472, 0), (512, None, 0)]),
         (8388608, 256, True, [(512, 3639, 0), (512, 1472, 0), (512, None, 0)])]


def _random(seed, n, m_hi, grids):
    """The generator of test_node_chain_row_split_covers_every_tile_once_and_balances_cost."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        M = int(rng.randint(1, m_hi))
        projs = [(int(rng.choice([128, 256, 512, 768])), None if rng.rand() < 0.3 else int(rng.randint(0, M + 50)),
                  int(rng.choice([0, 0, rng.randint(0, M + 1)]))) for _ in range(rng.randint(0, 4))]
        out.append((M, int(rng.choice(grids)), bool(rng.rand() < 0.7) or not projs, projs))
    return out


def random_cases():
    return _random(0, 40, 30000, [8, 104, 256, 304])


def small_random_cases():
    return _random(5, 300, 1500, [1, 2, 3, 8])


def edge_host_cases():
    return [(M if mc is None else min(M, mc), grid, do_mlp, projs) for M, mc, grid, do_mlp, projs in EDGE]


def listed_cases():
    """The cases whose piece lists the fixture holds, in its order."""
    return NAMED + random_cases() + small_random_cases() + edge_host_cases()


def case_row(M, grid, do_mlp, projs, H):
    """One case as 14 int32: M, grid, H, do_mlp, n_proj, then (N, count, first) per projection slot."""
    row = [M, grid, H, int(do_mlp), len(projs)]
    for q in range(3):
        n, cnt, first = projs[q] if q < len(projs) else (0, 0, 0)
        row += [n, ALL_ROWS if cnt is None else cnt, first]
    return row


def digest(pieces):
    return hashlib.sha256(np.ascontiguousarray(pieces, dtype="<i4").tobytes()).hexdigest()


def host_split(lib, M, grid, do_mlp, projs, H=256):
    """dsbdd_chain_split_host: the compiled split for every workgroup.  Returns (pieces int32 [n][3] = (workgroup, first
    row, tiles), header (Mw, total, V, Vs, forced))."""
    n = len(projs)
    arr = lambda v: (C.c_int32 * 3)(*(list(v) + [0] * (3 - n)))
    pn, pf = arr([p[0] for p in projs]), arr([p[2] for p in projs])
    pc = arr([ALL_ROWS if p[1] is None else p[1] for p in projs])
    header = (C.c_uint32 * 5)()
    args = (M, int(do_mlp), n, pn, pf, pc, H, grid, header)
    count = lib.dsbdd_chain_split_host(*args, None, 0)
    assert count >= 0, count
    pieces = np.zeros((count, 3), dtype=np.int32)
    assert lib.dsbdd_chain_split_host(*args, pieces.ctypes.data_as(C.c_void_p), count) == count
    return pieces, tuple(int(x) for x in header)


def per_workgroup(pieces, grid):
    """[[(r0, tiles), ...] per workgroup] of a flat piece list."""
    out = [[] for _ in range(grid)]
    for wg, r0, take in pieces.tolist():
        out[wg].append((r0, take))
    return out
