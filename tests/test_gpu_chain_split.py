"""The node chain's row split on the device (-m gpu): dsbdd_chain_split_probe runs csrc/chain_split.h in a launch of `grid`
workgroups that read the device scalars through node_chain_kernel's own lines.  Its output must equal, exactly, what the
same text computes on the host (dsbdd_chain_split_host) and what the commit before chain_split.h computed
(tests/golden/chain_split_parent.npz) -- at the smallest shapes that reach every path, with both weights (H = 256, 128)."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib
from tests import _chain_split_cases as cs

pytestmark = pytest.mark.gpu


def probe(lib, M, m_count, grid, do_mlp, projs, H):
    """One probe launch.  m_count and every count that is not None are DEVICE scalars.  Returns (pieces, header)."""
    n = len(projs)
    scal = torch.tensor([0 if m_count is None else m_count] + [0 if p[1] is None else p[1] for p in projs],
                        dtype=torch.int32, device="cuda")
    at = lambda k: scal.data_ptr() + 4 * k
    arr = lambda v: (C.c_int32 * 3)(*(list(v) + [0] * (3 - n)))
    counts = (C.c_void_p * 3)(*[None if p[1] is None else at(1 + q) for q, p in enumerate(projs)])
    cap = (M + 15) // 16 + 1                      # every piece holds a tile of its own
    header = torch.zeros(5, dtype=torch.int32, device="cuda")
    pieces = torch.full((cap, 3), -1, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    _lib.check(lib.dsbdd_chain_split_probe(None, M, None if m_count is None else at(0), int(do_mlp), n,
                                           arr([p[0] for p in projs]), arr([p[2] for p in projs]), counts, H, grid,
                                           header.data_ptr(), pieces.data_ptr(), cap, count.data_ptr()),
               "dsbdd_chain_split_probe")
    torch.cuda.synchronize()
    k = int(count.item())
    assert 0 <= k <= cap, (k, cap)
    return pieces[:k].cpu().numpy(), tuple(int(v) for v in header.cpu().numpy().view(np.uint32))


@pytest.fixture(scope="module")
def golden():
    z = np.load(cs.GOLDEN)
    return {k: z[k] for k in ("header", "piece_off", "pieces")}


def check(lib, golden, index, M, m_count, grid, do_mlp, projs, H):
    dev_pieces, dev_header = probe(lib, M, m_count, grid, do_mlp, projs, H)
    host_pieces, host_header = cs.host_split(lib, M if m_count is None else min(M, m_count), grid, do_mlp, projs, H=H)
    what = (M, m_count, grid, do_mlp, projs, H)
    assert dev_header == host_header == tuple(golden["header"][index]), what
    assert np.array_equal(dev_pieces, host_pieces), what
    assert np.array_equal(dev_pieces, golden["pieces"][golden["piece_off"][index]:golden["piece_off"][index + 1]]), what
    return dev_header


@pytest.mark.parametrize("hi", range(len(cs.HS)))
def test_probe_equals_host_and_parent_on_every_path(golden, hi):
    lib, n_listed = _lib.load(), len(cs.listed_cases())
    first = n_listed - len(cs.EDGE)               # the edge list closes the fixture's cases
    headers = [check(lib, golden, hi * n_listed + first + k, *case, cs.HS[hi]) for k, case in enumerate(cs.EDGE)]
    forced = [h[4] for h in headers]
    assert forced[:4] == [0, 1, 0, 1]                                   # either side of the threshold, at grid 1 and 8
    assert headers[5][3] == 4 * 8 and forced[5]                         # four ranges per workgroup
    assert headers[7] == headers[8] == (0, 0, 0, 0, 0)                  # nothing to do
    assert headers[10][0] == 300                                        # *m_count bites


@pytest.mark.parametrize("hi", range(len(cs.HS)))
def test_probe_equals_host_and_parent_on_small_random_problems(golden, hi):
    lib, n_listed = _lib.load(), len(cs.listed_cases())
    first = len(cs.NAMED) + len(cs.random_cases())
    n_forced = 0
    for k, (M, grid, do_mlp, projs) in enumerate(cs.small_random_cases()):
        n_forced += check(lib, golden, hi * n_listed + first + k, M, None, grid, do_mlp, projs, cs.HS[hi])[4]
    assert n_forced > 200


def test_probe_argument_checks():
    lib = _lib.load()
    one = torch.zeros(16, dtype=torch.int32, device="cuda")
    p, z3 = one.data_ptr(), (C.c_int32 * 3)()
    c3, h5 = (C.c_void_p * 3)(), (C.c_uint32 * 5)()
    ok = dict(M=32, n_proj=0, H=256, grid=1, header=p, pieces=p, cap=1, count=p)
    for bad in (dict(header=None), dict(pieces=None), dict(count=None), dict(grid=0), dict(H=100), dict(H=0),
                dict(n_proj=4), dict(n_proj=-1), dict(M=(8 << 20) + 1), dict(cap=-1)):
        a = {**ok, **bad}
        assert lib.dsbdd_chain_split_probe(None, a["M"], None, 1, a["n_proj"], z3, z3, c3, a["H"], a["grid"], a["header"],
                                           a["pieces"], a["cap"], a["count"]) == _lib.ERR_ARG, bad
        if "count" not in bad:
            assert lib.dsbdd_chain_split_host(a["M"], 1, a["n_proj"], z3, z3, z3, a["H"], a["grid"], a["header"] and h5,
                                              a["pieces"] and z3, a["cap"]) == _lib.ERR_ARG, bad
