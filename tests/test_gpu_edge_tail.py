"""Quarter items of the fused edge kernels (csrc/edge_wave.h "quarter items", DSBDD_OPT_TAIL; -m gpu).

The tiles of a message launch's last, partly filled round are evaluated as 32-edge quarter items, split over the
column tiles of a workgroup's four waves.  The split keeps every output's fmaf chain and every sum's operands, so
there is no tolerance in this file: every comparison is torch.equal / an integer-view equality against the same engine
with the option at 0.  Problems: the "ragged" and "shapes" batches of test_gpu_cone_shell.py (B = 4, 150-286 pocket
atoms, 0-23 ligand atoms, H = 256), about 130 tiles of 128 edges per all-rows launch.  Values n > 1 of the option put
n in place of the resident workgroups in the rule: a large n (ALL) makes every tile of every launch a quarter item, a
small n makes a launch hold whole rounds followed by quarter items (test_mixed_launch asserts that from the edge list).
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import weights as W
from tests._golden import GOLDEN_DIR
from tests.test_gpu_cone_shell import ARCH, PLAN, engine_for, select
from tests.test_gpu_fullsize import _make_ddpm, dev, make_dynamics

pytestmark = pytest.mark.gpu
OPT_TAIL = 6
MIXED_NS = (24, 40, 64, 104)            # 3 / 5 / 8 / 13 workgroups per XCD in the rule
ALL = 1 << 16                           # 8192 per XCD: every launch of this file is at most a quarter of a round


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def split_plan(slots, n):
    """The kernel's rule on the host: per XCD (first tile, tiles, tiles split into quarter items) of a launch over
    `slots` list entries with n in place of the resident workgroups."""
    ntiles = (slots + 127) // 128
    tq, tr = divmod(ntiles, 8)
    S = max(n >> 3, 1)
    plan, cbase = [], 0
    for x in range(8):
        csize = tq + (1 if x < tr else 0)
        R = csize % S
        nsplit = R if 4 * R <= S else (R - S // 2 if 2 * R > S and 4 * R <= 3 * S else 0)
        plan.append((cbase, csize, nsplit))
        cbase += csize
    return plan


@functools.lru_cache(maxsize=None)
def plain(tail, attention):
    """One all-rows call (no frame, pocket output wanted) with the per-block trace: eps, trace, the raw row list."""
    from diffsbdd_amd import _lib
    from diffsbdd_amd.engine import edge_capacity
    cfg = dict(W.arch_cfg(ARCH)[0], attention=attention)
    batch = select("ragged", [0, 1, 2, 3])
    m = make_dynamics(cfg, W.random_state_dict(cfg, 0))
    eng = m.engine()
    a = [batch[k].to(dev()).contiguous() for k in ("xl", "xp", "t", "ml", "mp")]
    cap = edge_capacity(a[3], a[4], 4)
    eng.set_option(OPT_TAIL, tail)
    assert eng.get_option(OPT_TAIL) == tail
    n = a[0].shape[0] + a[1].shape[0]
    eng.ensure_workspace(a[0].shape[0], a[1].shape[0], 4, cap)
    th, tx = eng.set_trace(n)
    eps_l, eps_p, status = m.forward_async(*a, batch=4, edge_cap=cap)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    slots = eng.edge_slots(n)
    rows = eng._read(eng.buffer_ptr(_lib.BUF_EDGE_ROW), slots, np.int32)
    out = {"eps_l": bits(eps_l), "eps_p": bits(eps_p), "h": bits(th), "x": bits(tx), "rows": rows, "slots": slots}
    eng.clear_trace()
    return out


def same_call(got, want):
    return all(torch.equal(got[k], want[k]) for k in ("eps_l", "eps_p", "h", "x"))


@pytest.mark.parametrize("attention", [True, False])
def test_all_rows_call_bitwise(attention):
    """Plain all-rows call, option 1 and every tile a quarter item against 0: eps of both node sets and every
    block's h / x."""
    off = plain(0, attention)
    assert all(nsplit == csize > 0 for _, csize, nsplit in split_plan(off["slots"], ALL))
    assert off["h"].abs().sum() > 0
    for tail in (1, ALL):
        assert same_call(plain(tail, attention), off), tail
    if attention:                        # the gates do something: the two configurations are different networks
        assert not torch.equal(off["eps_l"], plain(0, False)["eps_l"])


def test_mixed_launch():
    """Small n: whole items followed by quarter items in one launch.  From the raw row list (padding entries -1) and
    the rule: over the n of MIXED_NS there is an XCD range with both kinds; a row whose edges straddle the boundary
    tile from a whole item into a quarter item (its head slot is written by the quarter item) and from a quarter item
    into the next XCD's first whole item (the reverse); the list's last tile has inactive slots and is split."""
    off = plain(0, True)
    rows, slots = off["rows"], off["slots"]
    seen = {"mixed": 0, "whole->quarter": 0, "quarter->whole": 0, "split last tile": 0}
    straddles = lambda e: 0 < e < slots and rows[e] >= 0 and rows[e - 1] == rows[e]
    for n in MIXED_NS:
        plan = split_plan(slots, n)
        print(f"n = {n}: {slots} slots, (first tile, tiles, split) per XCD {plan}")
        for x, (cbase, csize, nsplit) in enumerate(plan):
            if nsplit == 0:
                continue
            seen["mixed"] += csize > nsplit
            seen["whole->quarter"] += csize > nsplit and straddles(128 * (cbase + csize - nsplit))
            seen["quarter->whole"] += x < 7 and plan[x + 1][1] > plan[x + 1][2] and straddles(128 * (cbase + csize))
            seen["split last tile"] += x == 7 or all(c == 0 for _, c, _ in plan[x + 1:])
        assert same_call(plain(n, True), off), n
    print(seen)
    assert slots % 128 != 0 or rows[-1] < 0                      # inactive slots in the list's last tile
    assert all(v > 0 for v in seen.values()), seen


def pruned(kind, sel, tail, shell=True, xl=None):
    """Ligand-output call with frame, cone and shell (three calls, asserted bit-identical): eps, the node features
    the call leaves behind (the shell rows' hidden state after their stages, see test_gpu_cone_shell.py), the plan."""
    from diffsbdd_amd import _lib
    batch = select(kind, sel)
    if xl is not None:
        batch = dict(batch, xl=xl)
    m, eng, a, cap = engine_for(batch, shell)
    eng.set_option(OPT_TAIL, tail)
    B = len(sel)
    outs = [m.forward_async(*a, batch=B, edge_cap=cap, want_pocket=False) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(int(o[2].item()) == 0 for o in outs)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][0], outs[2][0])
    n = a[0].shape[0] + a[1].shape[0]
    H = W.arch_cfg(ARCH)[0]["hidden_nf"]
    res = {"eps": bits(outs[0][0]), "plan": eng.last_plan(),
           "h": eng._read(eng.buffer_ptr(_lib.BUF_H), n * H, np.uint32).copy()}
    eng.clear_pocket_frame()
    return res


@pytest.mark.parametrize("kind,sel", [("ragged", [0, 1, 2, 3]), ("shapes", [0, 1, 2, 3]), ("shapes", [1])])
def test_pruned_frame_cone_shell_bitwise(kind, sel):
    """Pruned call with frame, cone and shell on -- block 0's two-list launch, the shell instantiation with its message
    store, the level prefixes -- with option 1, every tile split and two small n (mixed launches) against option 0:
    eps and the hidden state of every row, the shell rows among them.  ("shapes", [1]): a ligand that touches nothing,
    so both shell lists (the second list of stages 1 and 2) are empty."""
    off = pruned(kind, sel, 0)
    assert (off["plan"][0], off["plan"][1]) == PLAN
    assert np.count_nonzero(off["h"]) > 0
    for tail in (1, ALL, 24, 64):
        on = pruned(kind, sel, tail)
        assert (on["plan"][0], on["plan"][1]) == PLAN
        assert torch.equal(on["eps"], off["eps"]), tail
        assert np.array_equal(on["h"], off["h"]), tail


def test_shell_off_with_quarter_items():
    """The same with OPT_SHELL = 0 (the default instantiation on the cone's stages 1 and 2)."""
    off = pruned("ragged", [0, 1, 2, 3], 0, shell=False)
    for tail in (ALL, 40):
        on = pruned("ragged", [0, 1, 2, 3], tail, shell=False)
        assert torch.equal(on["eps"], off["eps"]) and np.array_equal(on["h"], off["h"]), tail


def test_graph_replay_after_the_ligand_moved():
    """A captured graph replayed after the ligand moved (edge counts, and with them the split, change on the device)
    equals the eager call, and both equal option 0."""
    batch = select("shapes", [0, 1, 2, 3])
    moved = batch["xl"].clone()
    moved[:, :3] += torch.tensor([2.5, -1.0, 1.5])
    for tail in (ALL, 40):
        m, eng, a, cap = engine_for(batch, True)
        eng.set_option(OPT_TAIL, tail)
        for _ in range(2):
            m.forward_async(*a, batch=4, edge_cap=cap, want_pocket=False)
        a[0].copy_(moved.to(a[0].device))
        replayed = bits(m.forward_async(*a, batch=4, edge_cap=cap, want_pocket=False)[0])
        assert eng.graph_stats()[0] >= 1                         # it was a replay
        eng.clear_pocket_frame()
        assert torch.equal(replayed, pruned("shapes", [0, 1, 2, 3], tail, xl=moved)["eps"]), tail
        assert torch.equal(replayed, pruned("shapes", [0, 1, 2, 3], 0, xl=moved)["eps"]), tail


def test_chain_of_four_steps_bitwise():
    """A 4-step chain (all ligand atoms anchored, bench.py's state model): ligand, pocket and masks, every tile split and
    a small n against 0."""
    from diffsbdd_amd.pocket import prepare_pocket
    B, T, n_l = 3, 4, 14
    cfg, _ = W.arch_cfg(ARCH)
    z = np.load(os.path.join(GOLDEN_DIR, "pocket_3rfm.npz"))
    pocket = prepare_pocket(z["fa_x"], z["fa_types"], cfg["residue_nf"], repeats=B)
    g = torch.Generator().manual_seed(2)
    ligand = {"x": torch.from_numpy(z["ligand_x"]).float().repeat(B, 1),
              "one_hot": torch.nn.functional.one_hot(torch.randint(0, cfg["atom_nf"], (B * n_l,), generator=g),
                                                     cfg["atom_nf"]).float(),
              "size": torch.full((B,), n_l), "mask": torch.repeat_interleave(torch.arange(B), n_l)}
    model = _make_ddpm(ARCH, W.random_state_dict(cfg, 0))
    model.cone_mode = 2
    out = {}
    for tail in (0, ALL, 40):
        model.dynamics.engine().set_option(OPT_TAIL, tail)
        model.seed(7, sample_offset=0)
        res = model.inpaint({k: v.clone() for k, v in ligand.items()}, {k: v.clone() for k, v in pocket.items()},
                            torch.ones(B * n_l), resamplings=1, timesteps=T)
        assert (model.dynamics.engine().last_plan()[0], model.dynamics.engine().last_plan()[1]) == PLAN
        out[tail] = [r.cpu() for r in res]
    assert len(out[0]) == 4 and out[0][0].abs().sum() > 0
    for tail in (ALL, 40):
        for got, want in zip(out[tail], out[0]):
            assert got.dtype == want.dtype and torch.equal(got, want), tail


def test_option_keeps_the_workspace_layout():
    """Same capacities, option 0 / 1 / n: the same workspace size and the same offset of every named buffer."""
    from diffsbdd_amd import _lib
    cfg, _ = W.arch_cfg(ARCH)
    layouts = []
    for tail in (0, 1, 40):
        m = make_dynamics(cfg, W.random_state_dict(cfg, 0))
        eng = m.engine()
        eng.set_option(OPT_TAIL, tail)
        eng.ensure_workspace(60, 900, 4, 40000)
        nbytes = eng.lib.dsbdd_engine_workspace_bytes(eng.handle, *eng.caps)
        base = (eng.workspace.data_ptr() + 255) & ~255
        layouts.append((nbytes, [eng.buffer_ptr(b) - base for b in range(_lib.BUF_LEVEL_STATS + 1)]))
    assert layouts[0][0] > 0 and layouts[0] == layouts[1] == layouts[2]
