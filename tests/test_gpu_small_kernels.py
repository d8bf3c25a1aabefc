"""The small kernels around the matrix kernels of a sampling call (-m gpu), through the C ABI:

  levels_kernel (csrc/level_list.h)       hop levels, per-level counts, level-ordered list and shell degrees against a numpy
                                           breadth-first search over the natural-order list of the same call -- with the
                                           sample's levels and edges in LDS, and once with a pocket too large for that
  scan_kernel (csrc/radius_graph.h)       row_ptr of the main list and of the second list (pocket frame) against numpy's
                                           padded prefix sums of the degrees
  lig_head_kernel (csrc/lig_head.h)       eps_lig of one ligand-output-only call: the bytes the parent commit produced
                                           (tests/golden/small_kernels_parent.json) and a float64 evaluation of the head on
                                           the call's own h; a NaN input coordinate still sets the status bit
  cond_step_keyed_kernel (csrc/ddpm.h)    z_lig / xh_pocket after one keyed reverse step, with and without the RePaint
                                           branch: the parent's bytes (its float64 restatement: test_gpu_noise_and_steps.py)

The parent's bytes are SHA-256 digests plus a few rows, recorded by tests/golden/make_golden_small_kernels.py from a build
of the parent commit; they are never regenerated from the code under test."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle import weights as W
from tests._golden import GOLDEN_DIR
from tests.test_gpu_fullsize import _hop_levels
from tests.test_gpu_parity import _random_problem, dev, make_dynamics

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(GOLDEN_DIR, "small_kernels_parent.json")
OPT_CONE, OPT_SHELL = 1, 5
LIST2_DEG, LIST2_ROW_PTR = 0, 1            # dsbdd_engine_list2_read
LDS_ROWS, LDS_EDGES = 2048, 8192           # csrc/level_list.h kLvlRows / kLvlEdges: what levels_kernel holds in LDS

# ligand / pocket sizes per sample.  "ragged": the problem of test_folded_scans_are_bitwise_the_scan_kernels (a sample without
# ligand atoms, one without pocket atoms, a one-atom ligand); "frame": the same ligands on pockets that all exist, for the
# call with a pocket frame; "big": one pocket whose edges do not fit levels_kernel's LDS (the walk over global memory)
LEVEL_PROBLEMS = {
    "ragged": ([23, 0, 9, 40, 1], [36, 50, 0, 20, 44], False),
    "frame": ([23, 0, 9, 40, 1], [36, 50, 30, 20, 44], True),
    "big": ([12, 5], [700, 40], False),
}


def align32(v):
    return (v + 31) // 32 * 32


def padded_ptr(deg, groups):
    """row_ptr [N + 1] of a list whose segments `groups` (arrays of node ids, in list order) each start at a multiple of
    32: a row's first slot = its segment's base + the edges of the segment's earlier rows; [N] = the padded total."""
    ptr = np.zeros(len(deg) + 1, dtype=np.int64)
    base = 0
    for rows in groups:
        d = deg[rows]
        ptr[rows] = base + np.cumsum(d) - d
        base += align32(int(d.sum()))
    ptr[-1] = base
    return ptr, base


def list2_read(eng, which, n):
    from diffsbdd_amd import _lib
    out = np.zeros(n, dtype=np.int32)
    _lib.check(eng.lib.dsbdd_engine_list2_read(eng.handle, C.c_int(which), C.c_void_p(out.ctypes.data), C.c_int64(n)),
               "dsbdd_engine_list2_read")
    return out


def check_level_structures(eng, ml, mp, B, frame, shell=None):
    """Everything levels_kernel / scan_kernel produce for the last ligand-output-only call of `eng`, against numpy."""
    from diffsbdd_amd import _lib
    n_l, N = len(ml), len(ml) + len(mp)
    batch_of = np.concatenate([ml.numpy(), mp.numpy()])
    is_lig = np.arange(N) < n_l
    torch.cuda.synchronize()
    lv = eng.last_levels(N)
    deg = lv["deg"].astype(np.int64)
    rp = eng._read(eng.buffer_ptr(_lib.BUF_ROW_PTR), N + 1, np.int32).astype(np.int64)
    # ---- scan: the natural-order list's row_ptr = padded prefix sums of deg over (ligand rows of b ..., pocket rows of b ...)
    segs = [np.nonzero(is_lig & (batch_of == b))[0] for b in range(B)] + \
           [np.nonzero(~is_lig & (batch_of == b))[0] for b in range(B)]
    want_rp, total = padded_ptr(deg, segs)
    assert np.array_equal(rp, want_rp)
    row = eng._read(eng.buffer_ptr(_lib.BUF_EDGE_ROW), total, np.int32).astype(np.int64)
    col = eng._read(eng.buffer_ptr(_lib.BUF_EDGE_COL), total, np.int32).astype(np.int64)
    for i in range(N):
        assert (row[rp[i]:rp[i] + deg[i]] == i).all(), i
    assert int((row >= 0).sum()) == int(deg.sum())                    # everything else is padding
    keep = row >= 0
    row, col = row[keep], col[keep]
    if frame:   # the second list: the edges with a ligand endpoint, same layout
        deg2 = list2_read(eng, LIST2_DEG, N).astype(np.int64)
        want_deg2 = np.where(is_lig, deg, np.bincount(row[col < n_l], minlength=N))
        assert np.array_equal(deg2, want_deg2)
        assert np.array_equal(list2_read(eng, LIST2_ROW_PTR, N + 1), padded_ptr(deg2, segs)[0])
    # ---- levels: breadth-first search over that list
    lvl = _hop_levels(row, col, n_l, N)
    assert np.array_equal(lv["level"], lvl)
    assert np.array_equal(lv["count"], [(lvl <= r).sum() for r in range(5)])
    assert np.array_equal(lv["order"], np.argsort(lvl, kind="stable"))          # nodes by (level, id)
    # the level-ordered list: one 32-aligned segment per (level, sample), behind the ghost slots of a canonical pocket
    groups = [np.nonzero((lvl == L) & (batch_of == b))[0] for L in range(5) for b in range(B)]
    want_ptr, _ = padded_ptr(deg, groups)
    gs = lv["ghost_slots"]
    assert np.array_equal(lv["row_ptr"], want_ptr[:N] + gs)
    ends = [gs + sum(align32(int(deg[g].sum())) for g in groups[:(L + 1) * B]) for L in range(5)]
    assert np.array_equal(lv["end"], ends)
    if shell is not None:   # a row of level 2 / 3: its edges from columns of a lower level
        want = np.bincount(row[lvl[col] < lvl[row]], minlength=N)
        sel = (lvl == 2) | (lvl == 3)
        assert sel.any() and np.array_equal(shell["deg"][sel], want[sel])
    return lvl, deg, batch_of


@pytest.mark.parametrize("kind", list(LEVEL_PROBLEMS))
def test_levels_and_scans_vs_numpy(kind):
    """small_cond, one ligand-output-only call (t shared by the batch).  "ragged" holds a sample without ligand atoms
    -- every pocket row of it at the top level -- and pocket rows more than three hops from the ligand; "frame" adds the
    pocket frame with the cone options on (the second list of the radius graph; this architecture builds no shell lists,
    the H = 256 test below does); "big" takes levels_kernel's walk over global memory."""
    from diffsbdd_amd.engine import edge_capacity
    n_lig, n_poc, frame = LEVEL_PROBLEMS[kind]
    cfg, _ = W.arch_cfg("small_cond")
    xl, xp, _, ml, mp = _random_problem(cfg, n_lig, n_poc, seed=17)
    B, d = len(n_lig), dev()
    m = make_dynamics(cfg, W.random_state_dict(cfg, 4))
    eng = m.engine()
    a = [v.to(d).contiguous() for v in (xl, xp, torch.full((1,), 0.4), ml, mp)]
    cap = edge_capacity(a[3], a[4], B)
    if frame:
        eng.set_option(OPT_CONE, 2)
        eng.set_option(OPT_SHELL, 1)
        eng.set_pocket_frame(a[1][:, :3].contiguous(), a[4], torch.tensor(n_poc).to(d), a[0].shape[0], B, cap)
    _, _, st = m.forward_async(*a, batch=B, edge_cap=cap, want_pocket=False)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    lvl, deg, batch_of = check_level_structures(eng, ml, mp, B, frame)
    poc = np.arange(len(lvl)) >= len(ml)
    seg_edges = [int(deg[poc & (batch_of == b)].sum()) for b in range(B)]
    if kind == "big":
        assert align32(seg_edges[0]) > LDS_EDGES and n_poc[0] <= LDS_ROWS    # the bound that sends sample 0 to global memory
    else:
        assert max(align32(s) for s in seg_edges) <= LDS_EDGES
        assert (lvl[poc & (batch_of == 1)] == 4).all()                       # the sample without ligand atoms
    assert all((lvl == L).any() for L in range(5))                           # ... and rows more than three hops out
    if frame:
        eng.clear_pocket_frame()


def test_levels_and_shell_degrees_h256():
    """The same on the full-atom architecture (hidden_nf 256) with a pocket frame, the forward cone and the shell lists on:
    the ragged batch of test_gpu_cone_shell.py (samples 0 and 3 share a pocket, sample 2 has no ligand atoms)."""
    from tests.test_gpu_cone_shell import engine_for, read_shell, select
    batch = select("ragged", [0, 1, 2, 3])
    m, eng, a, cap = engine_for(batch, True)
    B = len(batch["sizes_p"])
    _, _, st = m.forward_async(*a, batch=B, edge_cap=cap, want_pocket=False)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    n = a[0].shape[0] + a[1].shape[0]
    lvl, _, _ = check_level_structures(eng, batch["ml"], batch["mp"], B, True, shell=read_shell(eng, n))
    assert (lvl == 2).any() and (lvl == 3).any()
    eng.clear_pocket_frame()


# ---- the parent's bytes -----------------------------------------------------------------------------------------------
HEAD_ARCHS = ["small_cond", "crossdock_fullatom_cond"]
HEAD_SIZES = ([23, 1, 9], [36, 50, 20])            # B = 3, ragged
STEP_CASES = [("anf10_rnf10", 10, 10), ("anf10_rnf20", 10, 20)]     # (full-atom and small, C-alpha) feature widths
STEP_SIZES = ([23, 0, 9], [36, 50, 20])
GOLDEN_ROWS = 4


def head_call(arch, nan_row=None):
    """One ligand-output-only call: (eps_lig, status, h and x as the call left them, the inputs), numpy / CPU."""
    from diffsbdd_amd import _lib
    cfg, _ = W.arch_cfg(arch)
    sd = W.random_state_dict(cfg, 4)
    xl, xp, _, ml, mp = _random_problem(cfg, *HEAD_SIZES, seed=23)
    if nan_row is not None:
        xl = xl.clone()
        xl[nan_row, 1] = float("nan")
    m = make_dynamics(cfg, sd)
    B, N = len(HEAD_SIZES[0]), len(ml) + len(mp)
    eps, _, st = m.forward_async(xl, xp, torch.full((1,), 0.4), ml, mp, want_pocket=False, batch=B)
    torch.cuda.synchronize()
    eng, H = m.engine(), cfg["hidden_nf"]
    h = eng._read(eng.buffer_ptr(_lib.BUF_H), N * H, np.float32).reshape(N, H)
    x = eng._read(eng.buffer_ptr(_lib.BUF_X), N * 3, np.float32).reshape(N, 3)
    return eps.cpu().numpy(), int(st.item()), h, x, xl, cfg, sd


def step_call(anf, rnf, repaint):
    """One keyed reverse step (repaint 0: update only, 1: + RePaint iteration, 2: + the jump back) -> (z_lig, xh_pocket)."""
    from diffsbdd_amd import _lib
    lib = _lib.load()
    lsz, psz = STEP_SIZES
    g = torch.Generator().manual_seed(100 * anf + rnf + repaint)
    dl, dp, nl, npk, B, d = 3 + anf, 3 + rnf, sum(lsz), sum(psz), len(lsz), dev()
    ml = torch.repeat_interleave(torch.arange(B), torch.tensor(lsz)).to(d)
    mp = torch.repeat_interleave(torch.arange(B), torch.tensor(psz)).to(d)
    centre = (torch.rand(B, 3, generator=g) - 0.5) * 60.0
    rnd = lambda n, c: torch.randn(n, c, generator=g)
    z = torch.cat([centre[ml.cpu()] + rnd(nl, 3) * 3.0, rnd(nl, anf)], 1).to(d)
    poc = torch.cat([centre[mp.cpu()] + rnd(npk, 3) * 9.0, rnd(npk, rnf)], 1).to(d)
    eps, xh0 = rnd(nl, dl).to(d), torch.cat([centre[ml.cpu()] + rnd(nl, 3) * 3.0, rnd(nl, anf)], 1).to(d)
    fixed = (torch.rand(nl, generator=g) < 0.5).float().to(d)
    com0 = (centre + rnd(B, 3) * 0.5).to(d)
    scratch, t_word = torch.zeros_like(z), torch.zeros(1, device=d)
    p = lambda t: t.data_ptr()
    _lib.check(lib.dsbdd_cond_step_keyed(
        None, p(z), p(poc), p(eps), p(scratch), p(xh0), p(com0), p(fixed), p(ml), p(mp), nl, npk, B, anf, rnf,
        0.98437, 0.07911, 0.12345, repaint, 0.95312, 0.30273, 0.15891, 1, C.c_uint64((0xABCD << 32) | 7), C.c_uint64(6),
        1000, None, p(t_word), 0.37), "dsbdd_cond_step_keyed")
    torch.cuda.synchronize()
    return z.cpu().numpy(), poc.cpu().numpy()


def parent_cases():
    """name -> float32 array: everything the golden file records (the recording script calls this on the parent's build)."""
    out = {}
    for arch in HEAD_ARCHS:
        out[f"eps_lig/{arch}"] = head_call(arch)[0]
    for name, anf, rnf in STEP_CASES:
        for repaint in (0, 1, 2):
            z, poc = step_call(anf, rnf, repaint)
            out[f"step/{name}/repaint{repaint}/z_lig"] = z
            out[f"step/{name}/repaint{repaint}/xh_pocket"] = poc
    return out


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return {"shape": list(a.shape), "sha256": hashlib.sha256(a.tobytes()).hexdigest(),
            "rows": [[float(v) for v in r] for r in a[:GOLDEN_ROWS]]}


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def assert_parent_bytes(name, got):
    want, have = golden()[name], digest(got)
    assert have["shape"] == want["shape"], name
    # the first rows value by value (a readable failure), then every byte
    assert np.array_equal(np.array(have["rows"], dtype=np.float32), np.array(want["rows"], dtype=np.float32)), name
    assert have["sha256"] == want["sha256"], name


@pytest.mark.parametrize("arch", HEAD_ARCHS)
def test_lig_head_is_the_parents_bytes_and_float64(arch):
    """eps_lig of one call: bit for bit the parent's; the head itself -- embedding_out, the atom decoder, x - x_in -- in
    float64 on the h and x the call left behind, 1e-5 absolute."""
    eps, status, h, x, xl, cfg, sd = head_call(arch)
    assert status == 0
    assert_parent_bytes(f"eps_lig/{arch}", eps)
    n_l, J = len(xl), cfg["joint_nf"]
    f64 = lambda k: sd[k].double().numpy()
    hout = h[:n_l].astype(np.float64) @ f64("egnn.embedding_out.weight")[:J].T + f64("egnn.embedding_out.bias")[:J]
    mid = hout @ f64("atom_decoder.0.weight").T + f64("atom_decoder.0.bias")
    mid = mid / (1.0 + np.exp(-mid))
    eps_h = mid @ f64("atom_decoder.2.weight").T + f64("atom_decoder.2.bias")
    err_h = np.abs(eps[:, 3:] - eps_h).max()
    err_x = np.abs(eps[:, :3] - (x[:n_l].astype(np.float64) - xl[:, :3].double().numpy())).max()
    print(f"lig_head {arch}: max |err| features {err_h:.3e} coordinates {err_x:.3e}")
    assert err_h < 1e-5 and err_x < 1e-5


def test_lig_head_nan_coordinate_sets_the_status_bit():
    _, status, _, _, _, _, _ = head_call("small_cond", nan_row=5)
    assert status & 1


@pytest.mark.parametrize("repaint", [0, 1, 2])
@pytest.mark.parametrize("name,anf,rnf", STEP_CASES)
def test_keyed_step_is_the_parents_bytes(name, anf, rnf, repaint):
    z, poc = step_call(anf, rnf, repaint)
    assert np.isfinite(z).all() and np.isfinite(poc).all()
    assert_parent_bytes(f"step/{name}/repaint{repaint}/z_lig", z)
    assert_parent_bytes(f"step/{name}/repaint{repaint}/xh_pocket", poc)
