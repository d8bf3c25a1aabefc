"""The node chain's second row split on the device (csrc/chain_split.h ChainDeal, DSBDD_OPT_CHAIN_DEAL; -m gpu).

(1) dsbdd_chain_deal_probe runs the policy in a launch of `grid` workgroups that read the device scalars through
node_chain_kernel's own lines; its header and pieces must equal, exactly, what the same text computes on the host
(dsbdd_chain_deal_host) -- at the edge list of tests/_chain_split_cases and its small random cases, H = 256 and 128.
(2) Every output element of node_chain_kernel is one fmaf chain over k that does not depend on the row split, so a
ligand-output call leaves the same bits with the option at 0 and at 1: eps of the ligand and the hidden state of every row,
on the ragged batch of test_gpu_cone_shell.py (ghost rows in front of the lists, two samples sharing a pocket) and on 16
identical pockets of the H = 256 architecture (4 944 rows: more than one 16-row tile per workgroup on 256 CUs)."""
import ctypes as C

import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib
from oracle import weights as W
from tests import _chain_split_cases as cs
from tests import test_gpu_cone_shell as cone
from tests.test_chain_deal import deal_split

pytestmark = pytest.mark.gpu
OPT_CHAIN_DEAL = 7
cone.PROBLEMS.setdefault("identical16", [(286, 23, 1.5, 0.0, 0)] * 16)      # every sample has sample 0's pocket


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
    _lib.check(lib.dsbdd_chain_deal_probe(None, M, None if m_count is None else at(0), int(do_mlp), n,
                                          arr([p[0] for p in projs]), arr([p[2] for p in projs]), counts, H, grid,
                                          header.data_ptr(), pieces.data_ptr(), cap, count.data_ptr()),
               "dsbdd_chain_deal_probe")
    torch.cuda.synchronize()
    k = int(count.item())
    assert 0 <= k <= cap, (k, cap)
    return pieces[:k].cpu().numpy(), tuple(int(v) for v in header.cpu().numpy().view(np.uint32))


def check(lib, M, m_count, grid, do_mlp, projs, H):
    dev_pieces, dev_header = probe(lib, M, m_count, grid, do_mlp, projs, H)
    host_pieces, host_header = deal_split(lib, M if m_count is None else min(M, m_count), grid, do_mlp, projs, H=H)
    what = (M, m_count, grid, do_mlp, projs, H)
    assert dev_header == host_header, what
    assert np.array_equal(dev_pieces, host_pieces), what
    return dev_header


@pytest.mark.parametrize("H", cs.HS)
def test_probe_equals_host_on_every_path(H):
    lib = _lib.load()
    headers = [check(lib, *case, H) for case in cs.EDGE]
    fallback = [h[4] for h in headers]
    # (47 rows on 1 workgroup, 2 000 rows on 8 with three projections: ChainSplit's forced path deals them)
    assert fallback[1] == 1 and fallback[5] == 1 and fallback[0] == fallback[2] == fallback[9] == 0
    assert headers[7] == headers[8] == (0, 0, 0, 0, 0)                  # nothing to do
    assert headers[10][0] == 300                                        # *m_count bites
    assert headers[9][3] == 1                                           # 5 rows: one tile, one range


@pytest.mark.parametrize("H", cs.HS)
def test_probe_equals_host_on_small_random_problems(H):
    lib = _lib.load()
    headers = [check(lib, M, None, grid, do_mlp, projs, H) for M, grid, do_mlp, projs in cs.small_random_cases()]
    n_fallback = sum(h[4] for h in headers)
    assert 0 < n_fallback < len(headers)                                # both the policy's own paths and its fallback


def test_probe_argument_checks():
    lib = _lib.load()
    one = torch.zeros(16, dtype=torch.int32, device="cuda")
    p, z3, c3 = one.data_ptr(), (C.c_int32 * 3)(), (C.c_void_p * 3)()
    ok = dict(M=32, n_proj=0, H=256, grid=1, header=p, pieces=p, cap=1, count=p)
    for bad in (dict(header=None), dict(pieces=None), dict(count=None), dict(grid=0), dict(H=100), dict(H=0),
                dict(n_proj=4), dict(n_proj=-1), dict(M=(8 << 20) + 1), dict(cap=-1)):
        a = {**ok, **bad}
        assert lib.dsbdd_chain_deal_probe(None, a["M"], None, 1, a["n_proj"], z3, z3, c3, a["H"], a["grid"], a["header"],
                                          a["pieces"], a["cap"], a["count"]) == _lib.ERR_ARG, bad


def ligand_call(kind, sel, deal):
    """One ligand-output call with frame, cone and shell: bits of eps_lig and of the node features the call leaves."""
    batch = cone.select(kind, sel)
    m, eng, a, cap = cone.engine_for(batch, True)
    eng.set_option(OPT_CHAIN_DEAL, deal)
    assert eng.get_option(OPT_CHAIN_DEAL) == deal
    eps, _, status = m.forward_async(*a, batch=len(sel), edge_cap=cap, want_pocket=False)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    n = a[0].shape[0] + a[1].shape[0]
    H = W.arch_cfg(cone.ARCH)[0]["hidden_nf"]
    res = {"eps": eps.detach().cpu().contiguous().view(torch.int32), "plan": eng.last_plan(), "rows": n,
           "h": eng._read(eng.buffer_ptr(_lib.BUF_H), n * H, np.uint32).copy()}
    eng.clear_pocket_frame()
    return res


@pytest.mark.parametrize("kind,n_samples,rows", [("ragged", 4, 969), ("identical16", 16, 4944)])
def test_ligand_output_call_is_bit_identical_with_the_option_at_0_and_1(kind, n_samples, rows):
    sel = list(range(n_samples))
    off, on = ligand_call(kind, sel, 0), ligand_call(kind, sel, 1)
    assert off["rows"] == on["rows"] == rows
    assert (off["plan"][0], off["plan"][1]) == (on["plan"][0], on["plan"][1]) == cone.PLAN
    assert np.count_nonzero(off["h"]) > 0 and off["eps"].abs().sum() > 0
    assert torch.equal(on["eps"], off["eps"])
    assert np.array_equal(on["h"], off["h"])


def test_option_defaults_to_1():
    cfg, _ = W.arch_cfg(cone.ARCH)
    eng = cone.make_dynamics(cfg, W.random_state_dict(cfg, 0)).engine()
    assert eng.get_option(OPT_CHAIN_DEAL) == 1
