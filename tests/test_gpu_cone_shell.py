"""Shell stages of the forward cone (csrc/forward.h "Shell", DSBDD_OPT_SHELL; -m gpu).

In the ascending stages g = 1, 2 of the cone the rows of level g + 1 run only their edges from columns of level <= g
(the stage's shell list) and take the messages of their other edges from the canonical pocket's ghost rows.  Everything
here runs on the 3rfm full-atom fixture cut to sub-pockets of 286 / 201 / 150 atoms, H = 256, four samples, single
forward calls or three chained ones, with the cone pinned on (OPT_CONE = 2) and the frame at the raw pocket coordinates.

One case of the issue cannot be built: "a shell row of degree 0 in the shell list".  A row has level g + 1 exactly
when one of its columns has level g (levels_kernel relaxes over the row's own edges), so every shell row has at least
one edge in its list; test_shell_shapes asserts that fact instead.  The completion kernel still handles the degree-0
row (it never reads agg for it).

Run time on one MI355X: 4.2 s for the file (measured; two oracle evaluations of 4-sample batches dominate).
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import egnn_oracle as eo
from oracle import weights as W
from tests._golden import GOLDEN_DIR
from tests.test_gpu_fullsize import _hop_levels, dev, excess, make_dynamics, oracle_threads

pytestmark = pytest.mark.gpu
ARCH = "crossdock_fullatom_cond"
OPT_CONE, OPT_SHELL = 1, 5
(SHELL_STATS, SHELL_COUNT, SHELL_ROW, SHELL_COL, SHELL_PTR, SHELL_DEG) = range(6)       # dsbdd_engine_shell_read
PLAN = ([1, 2, 3, 3, 2, 1], [1, 1, 1, 0, 0, 0])
GOLDEN = os.path.join(GOLDEN_DIR, "cone_shell_parent_chain.npz")

# (pocket atoms, ligand atoms, ligand spread in Angstrom, ligand offset, representative) per sample
PROBLEMS = {
    # the layout of test_ligand_only_call_with_ragged_and_empty_samples: samples 0 and 3 share one representative
    "ragged": [(286, 23, 1.5, 0.0, 0), (201, 9, 1.5, 0.0, 1), (150, 0, 1.5, 0.0, 2), (286, 14, 1.5, 0.0, 0)],
    # sample 1: a ligand 100 A away touches nothing (every pocket row level 4, empty lists); sample 2: no ligand atoms;
    # sample 3: 23 atoms spread over the 150-atom pocket reach every pocket row within two hops (level 3 empty)
    "shapes": [(286, 23, 1.5, 0.0, 0), (201, 9, 1.5, 100.0, 1), (150, 0, 1.5, 0.0, 2), (150, 23, 2.5, 0.0, 2)],
}


@functools.lru_cache(maxsize=None)
def problem(kind):
    """CPU tensors of one batch: (xl, xp, t, ml, mp), raw frame coordinates, pocket sizes, representatives."""
    cfg, dd = W.arch_cfg(ARCH)
    z = np.load(os.path.join(GOLDEN_DIR, "pocket_3rfm.npz"))
    g = torch.Generator().manual_seed(11)
    P = torch.from_numpy(z["fa_x"]).float()
    types = torch.from_numpy(z["fa_types"]).long()
    center = P.mean(0)
    order = (P - center).norm(dim=1).argsort()
    xs, raws, hs, mp, ml, xl = [], [], [], [], [], []
    for b, (n_p, n_l, spread, far, _) in enumerate(PROBLEMS[kind]):
        idx = order[:n_p].sort().values
        shift = torch.randn(3, generator=g) * 3
        xs.append(P[idx] - center + shift)
        raws.append(P[idx] - center)
        hs.append(torch.nn.functional.one_hot(types[idx], cfg["residue_nf"]).float() / dd["norm_values"][1])
        mp.append(torch.full((n_p,), b))
        ml.append(torch.full((n_l,), b))
        xl.append(shift + far + torch.randn(n_l, 3, generator=g) * spread)
    ml_all, mp_all = torch.cat(ml), torch.cat(mp)
    xp_all = torch.cat([torch.cat(xs), torch.cat(hs)], 1)
    xl_all = torch.cat([torch.cat(xl), torch.randn(len(ml_all), cfg["atom_nf"], generator=g) * 0.5], 1)
    return {"xl": xl_all, "xp": xp_all, "t": torch.full((1,), 0.4), "ml": ml_all, "mp": mp_all,
            "raw": torch.cat(raws), "sizes_p": [s[0] for s in PROBLEMS[kind]], "rep": [s[4] for s in PROBLEMS[kind]]}


def select(kind, sel):
    """The samples `sel` of a problem as a batch of their own (masks and representatives renumbered)."""
    p = problem(kind)
    B = len(p["sizes_p"])
    sel_t = torch.tensor(sel)
    keep_l, keep_p = torch.isin(p["ml"], sel_t), torch.isin(p["mp"], sel_t)
    remap = torch.full((B,), -1, dtype=torch.long)
    remap[sel_t] = torch.arange(len(sel))
    rep = [int(remap[p["rep"][s]]) if p["rep"][s] in sel else int(remap[s]) for s in sel]
    return {"xl": p["xl"][keep_l], "xp": p["xp"][keep_p], "t": p["t"], "ml": remap[p["ml"][keep_l]],
            "mp": remap[p["mp"][keep_p]], "raw": p["raw"][keep_p], "sizes_p": [p["sizes_p"][s] for s in sel],
            "rep": rep, "lig_rows": keep_l}


def read_shell(eng, n_nodes):
    """The shell lists and their counters of the last call (dsbdd_engine_shell_read), as numpy arrays."""
    import ctypes
    from diffsbdd_amd import _lib

    def rd(which, n, dt, lst=0):
        out = np.zeros(n, dtype=dt)
        _lib.check(eng.lib.dsbdd_engine_shell_read(eng.handle, ctypes.c_int(which), ctypes.c_int(lst),
                                                   ctypes.c_void_p(out.ctypes.data), ctypes.c_int64(n)),
                   "dsbdd_engine_shell_read")
        return out

    stats = rd(SHELL_STATS, 8, np.uint64).astype(np.int64)
    cnt = rd(SHELL_COUNT, 2, np.int32)
    out = {"stats": stats, "slots": cnt, "ptr": rd(SHELL_PTR, n_nodes, np.int32),
           "deg": rd(SHELL_DEG, n_nodes, np.int32), "row": [], "col": []}
    for s in range(2):
        out["row"].append(rd(SHELL_ROW, int(cnt[s]), np.int32, s))
        out["col"].append(rd(SHELL_COL, int(cnt[s]), np.int32, s))
    return out


def engine_for(batch, shell, cone=2):
    """(module, engine, device args, edge capacity) with the frame at the batch's raw pocket coordinates."""
    from diffsbdd_amd.engine import edge_capacity
    cfg, _ = W.arch_cfg(ARCH)
    d = dev()
    m = make_dynamics(cfg, W.random_state_dict(cfg, 0))
    eng = m.engine()
    a = [batch[k].to(d).contiguous() for k in ("xl", "xp", "t", "ml", "mp")]
    B = len(batch["sizes_p"])
    cap = edge_capacity(a[3], a[4], B)
    eng.set_option(OPT_CONE, cone)
    if shell is not None:            # (None: a build without the option -- the recording of the parent's outputs)
        eng.set_option(OPT_SHELL, int(shell))
    eng.set_pocket_frame(batch["raw"].to(d), a[4], torch.tensor(batch["sizes_p"]).to(d), a[0].shape[0], B, cap,
                         representative=batch["rep"])
    return m, eng, a, cap


def run(batch, shell, want_lists=False):
    """Three calls (eager, captured, replayed; asserted bit-identical): ligand eps, edges, levels, plan, shell read-out."""
    m, eng, a, cap = engine_for(batch, shell)
    B = len(batch["sizes_p"])
    outs = [m.forward_async(*a, batch=B, edge_cap=cap, want_pocket=False) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(int(o[2].item()) == 0 for o in outs)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][0], outs[2][0])
    n = a[0].shape[0] + a[1].shape[0]
    er, ec = eng.last_edges(n)
    from diffsbdd_amd import _lib
    H = W.arch_cfg(ARCH)[0]["hidden_nf"]
    res = {"eps": outs[0][0].cpu(), "edges": torch.stack([er, ec]), "plan": eng.last_plan(),
           "level": eng.last_levels(n)["level"], "shell": read_shell(eng, n) if want_lists else None,
           # the node features as the call left them: a row holds the h of the last stage that evaluated it
           "h": eng._read(eng.buffer_ptr(_lib.BUF_H), n * H, np.float32).reshape(n, H).copy()}
    eng.clear_pocket_frame()
    return res


@functools.lru_cache(maxsize=None)
def reference(kind):
    """Per problem, once: the engine with the path on and off, the host BFS, the oracle on the engine's edge list."""
    batch = select(kind, [0, 1, 2, 3])
    on, off = run(batch, True, want_lists=True), run(batch, False)
    cfg, _ = W.arch_cfg(ARCH)
    n_l = len(batch["ml"])
    N = n_l + len(batch["mp"])
    row, col = on["edges"][0].numpy(), on["edges"][1].numpy()
    lvl = _hop_levels(row, col, n_l, N)
    trace = []
    with oracle_threads():
        o_l, _, _ = eo.dynamics_forward(W.random_state_dict(cfg, 0), cfg, batch["xl"], batch["xp"], batch["t"],
                                        batch["ml"], batch["mp"], edges=on["edges"], trace=trace)
    return {"batch": batch, "on": on, "off": off, "oracle": o_l, "lvl": lvl, "row": row, "col": col, "n_lig": n_l, "N": N,
            "trace_h": [h.numpy() for h, _ in trace]}


def host_shell_list(ref, g):
    """Stage g's shell list from the host BFS: (rows with -1 pads, columns, canonical (row, col) pairs, per-sample edges)."""
    lvl, row, col, n_l, N = ref["lvl"], ref["row"], ref["col"], ref["n_lig"], ref["N"]
    batch_of = np.concatenate([ref["batch"]["ml"].numpy(), ref["batch"]["mp"].numpy()])
    deg = np.bincount(row, minlength=N)
    ptr = np.concatenate([[0], np.cumsum(deg)])
    rows, cols, canon, per_sample, spans = [], [], [], [], {}
    for b in range(len(ref["batch"]["sizes_p"])):
        n_b = 0
        for i in np.nonzero((batch_of == b) & (lvl == g + 1))[0]:
            c = col[ptr[i]:ptr[i + 1]]
            own = c[lvl[c] <= g]
            canon += [(i, j) for j in c[lvl[c] > g]]
            assert (c[lvl[c] > g] >= n_l).all()                  # canonical references are pocket columns
            spans[i] = (len(rows), len(own))
            rows += [i] * len(own); cols += list(own); n_b += len(own)
        per_sample.append(n_b)
        pad = -len(rows) % 32
        rows += [-1] * pad; cols += [0] * pad
    return np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), canon, per_sample, spans


def check_counters(ref):
    """The engine's shell counters against the host lists; returns the host lists of stages 1 and 2."""
    sh = ref["on"]["shell"]
    calls = int(sh["stats"][6])
    assert calls == 3                                            # every call of run() built the lists
    lists = []
    for g in (1, 2):
        rows, cols, canon, per_sample, spans = host_shell_list(ref, g)
        s = g - 1
        assert int(sh["slots"][s]) == len(rows)
        assert sh["stats"][3 * s] == calls * int((rows >= 0).sum())
        assert sh["stats"][3 * s + 1] == calls * len(rows)
        assert sh["stats"][3 * s + 2] == calls * len(canon)
        lists.append((rows, cols, canon, per_sample, spans))
    return lists


@pytest.mark.parametrize("kind", ["ragged", "shapes"])
def test_shell_vs_oracle_and_switch(kind):
    """Ligand eps with the path on: against the float64-checked oracle (1e-4) and against the same engine with
    OPT_SHELL = 0 (2e-5: the tolerance between the pruned and the all-rows call); the cone's plan; both lists non-empty
    by the engine's own counters, so the comparison cannot pass with the path silently off."""
    ref = reference(kind)
    assert (ref["on"]["plan"][0], ref["on"]["plan"][1]) == PLAN and (ref["off"]["plan"][0], ref["off"]["plan"][1]) == PLAN
    lists = check_counters(ref)
    assert all((rows >= 0).sum() > 0 and len(canon) > 0 for rows, _, canon, _, _ in lists)
    # timed launches: whole prefixes of the largest radius only -- the shell stage of radius 3 is not one of them
    assert ref["on"]["plan"][2] == 3
    d_oracle, d_switch = excess(ref["on"]["eps"], ref["oracle"]), (ref["on"]["eps"] - ref["off"]["eps"]).abs().max().item()
    print(f"[{kind}] excess over 1e-4 vs oracle {d_oracle:.2e} (off: {excess(ref['off']['eps'], ref['oracle']):.2e}); "
          f"on vs off {d_switch:.2e}; shell edges {[int((l[0] >= 0).sum()) for l in lists]}, "
          f"canonical references {[len(l[2]) for l in lists]}")
    assert d_oracle <= 0                                         # 1e-4
    assert d_switch < 2e-5


@pytest.mark.parametrize("kind", ["ragged", "shapes"])
def test_shell_rows_hidden_state(kind):
    """The shell rows themselves.  The ligand output is too far downstream (and too well normalised) to show a wrong
    canonical gather, so this compares the node features the call leaves behind: with radii [1,2,3,3,2,1] a row of level
    3 holds its h after stage 3, a row of level 2 after stage 4, rows of level <= 1 after stage 5 -- all downstream of
    the shell stages 1 and 2, whose shell rows are exactly the levels 2 and 3.  Against the oracle's per-block trace
    (1e-4 relative to max(1, max |h|), the bound of the per-block trace test of test_gpu_fullsize.py) and against the
    same engine with OPT_SHELL = 0 (2e-5 on the same scale, this file's on / off tolerance).  A build whose ghost tiles
    do not store their messages shows 2.8e-3 on the level-3 rows, 28 x and 138 x the bounds (profiles/r7_shell.md)."""
    ref = reference(kind)
    h_on, h_off, lvl = ref["on"]["h"], ref["off"]["h"], ref["lvl"]
    for level, blk in ((3, 3), (2, 4), (1, 5), (0, 5)):
        rows = lvl == level
        if not rows.any():
            continue
        want = ref["trace_h"][blk][rows]
        scale = max(1.0, float(np.abs(want).max()))
        d_oracle = float(np.abs(h_on[:len(lvl)][rows] - want).max()) / scale
        d_off = float(np.abs(h_off[:len(lvl)][rows] - want).max()) / scale
        d_switch = float(np.abs(h_on[:len(lvl)][rows] - h_off[:len(lvl)][rows]).max()) / scale
        print(f"[{kind}] level {level} ({int(rows.sum())} rows, h after block {blk}, max |h| {scale:.3g}): "
              f"on vs oracle {d_oracle:.2e} (off {d_off:.2e}), on vs off {d_switch:.2e}")
        assert d_oracle < 1e-4, (level, d_oracle)
        assert d_switch < 2e-5, (level, d_switch)


def test_shell_shapes():
    """The shapes at which the path can go wrong, in one batch ("shapes"), each asserted from the host BFS and the
    engine's counters: a shell row whose list segment crosses a 32-edge tile boundary, a sample whose ligand touches
    nothing (empty lists), a sample without ligand atoms, a sample with an empty level 3 (no shell rows in stage 2).
    The parity with the oracle of this batch is test_shell_vs_oracle_and_switch[shapes]."""
    ref = reference("shapes")
    lists = check_counters(ref)
    lvl, n_l = ref["lvl"], ref["n_lig"]
    batch_of = np.concatenate([ref["batch"]["ml"].numpy(), ref["batch"]["mp"].numpy()])
    for rows, _, _, per_sample, spans in lists:
        assert any(pos // 32 != (pos + d - 1) // 32 for pos, d in spans.values())       # a row across two wave tiles
        assert min(d for _, d in spans.values()) >= 1            # (no shell row without an edge in its list: see the module docstring)
        assert per_sample[1] == 0 and per_sample[2] == 0         # out of contact / no ligand atoms: empty segments
    poc = lambda b: lvl[(batch_of == b) & (np.arange(len(lvl)) >= n_l)]
    assert (ref["batch"]["ml"] == 1).sum() == 9 and (poc(1) == 4).all()                  # a ligand that touches nothing
    assert (ref["batch"]["ml"] == 2).sum() == 0 and (poc(2) == 4).all()                  # no ligand atoms
    assert (poc(3) == 2).any() and not (poc(3) == 3).any() and lists[1][3][3] == 0       # level 3 empty
    assert lists[0][3][3] > 0 and lists[0][3][0] > 0 and lists[1][3][0] > 0


@pytest.mark.parametrize("kind", ["ragged", "shapes"])
def test_shell_lists_vs_host_bfs(kind):
    """The lists themselves: rows / columns / padding of stages 1 and 2 equal {level(row) = g + 1, level(col) <= g} in
    (sample, row, natural column) order with 32-aligned sample segments; the rest of the rows' edges -- the canonical
    references, pocket columns of level >= g + 1 -- are counted by the engine (check_counters), and both parts together
    are the rows' whole edge sets by construction of host_shell_list."""
    ref = reference(kind)
    sh = ref["on"]["shell"]
    assert np.array_equal(ref["on"]["level"], ref["lvl"])
    for g, (rows, cols, canon, _, spans) in zip((1, 2), check_counters(ref)):
        assert np.array_equal(sh["row"][g - 1], rows)
        assert np.array_equal(sh["col"][g - 1][rows >= 0], cols[rows >= 0])
        for i, (pos, d) in spans.items():
            assert sh["ptr"][i] == pos and sh["deg"][i] == d
        deg = np.bincount(ref["row"], minlength=ref["N"])
        assert (rows >= 0).sum() + len(canon) == deg[ref["lvl"] == g + 1].sum()


def test_shell_bitwise():
    """With the path on: a sample alone = the same sample inside the ragged batch (also the one whose lists are empty),
    B = 4 = 2 x B = 2, and a captured graph replayed after the ligand moved (rows change level) = the eager call.
    (Two runs of the same call: asserted inside run() for every call of this file.)"""
    full = reference("shapes")["on"]["eps"]
    p = problem("shapes")
    for sel in ([0], [1], [3], [0, 1], [2, 3]):
        part = run(select("shapes", sel), True)
        assert (part["plan"][0], part["plan"][1]) == PLAN
        assert torch.equal(part["eps"], full[torch.isin(p["ml"], torch.tensor(sel))]), sel
    # the same device tensors, ligand moved between the captured call and the replay
    batch = select("shapes", [0, 1, 2, 3])
    moved = batch["xl"].clone()
    moved[:, :3] += torch.tensor([2.5, -1.0, 1.5])
    m, eng, a, cap = engine_for(batch, True)
    for _ in range(2):
        m.forward_async(*a, batch=4, edge_cap=cap, want_pocket=False)
    a[0].copy_(moved.to(a[0].device))
    replayed = m.forward_async(*a, batch=4, edge_cap=cap, want_pocket=False)[0].cpu()
    assert eng.graph_stats()[0] >= 1                             # it was a replay
    eng.clear_pocket_frame()
    eager = run(dict(batch, xl=moved), True)
    assert not np.array_equal(eager["level"], reference("shapes")["lvl"])                # rows did change level
    assert torch.equal(replayed, eager["eps"])


def test_shell_chain_pocket_differs_by_a_translation_only():
    """What a chain returns for the POCKET with the path on against off.  The pocket's features never change and its
    coordinates are only ever translated: every reverse step subtracts the ligand's centre of mass from both node sets.
    The ligand differs between on and off in rounding, so the returned pocket is not bit-identical; what holds is that
    the features are, and that the coordinates differ by one translation per sample.  Bounds (T = 4 steps, all ligand
    atoms anchored, bench.py's state model): |translation| <= T x 2e-5 (this file's on / off tolerance per call), and
    around it each coordinate within 2 (T + 2) ulp of the largest coordinate (each run rounds a coordinate once per step
    and twice at the ends)."""
    from diffsbdd_amd.pocket import prepare_pocket
    from tests.test_gpu_fullsize import _make_ddpm
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
    for shell in (1, 0):
        model.dynamics.engine().set_option(OPT_SHELL, shell)
        model.seed(7, sample_offset=0)
        o_l, o_p, _, pm = model.inpaint({k: v.clone() for k, v in ligand.items()}, {k: v.clone() for k, v in pocket.items()},
                                        torch.ones(B * n_l), resamplings=1, timesteps=T)
        assert (model.dynamics.engine().last_plan()[0], model.dynamics.engine().last_plan()[1]) == PLAN
        out[shell] = (o_l.cpu(), o_p.cpu(), pm.cpu())
    (l1, p1, pm), (l0, p0, _) = out[1], out[0]
    assert torch.equal(p1[:, 3:], p0[:, 3:])                               # features: identical
    d = (p1[:, :3] - p0[:, :3]).double()
    ulp = float(p0[:, :3].abs().max()) * 2.0 ** -23
    worst_t = worst_r = 0.0
    for b in range(B):
        db = d[pm == b]
        worst_t = max(worst_t, float(db.mean(0).abs().max()))
        worst_r = max(worst_r, float((db - db.mean(0)).abs().max()))
    print(f"pocket on vs off: translation {worst_t:.2e}, residual {worst_r:.2e} ({worst_r / ulp:.1f} ulp); "
          f"ligand {float((l1 - l0).abs().max()):.2e}")
    assert worst_t <= T * 2e-5
    assert worst_r <= 2 * (T + 2) * ulp


def chain_outputs(shell):
    """Three chained calls on the ragged batch: the ligand moves along its own eps between calls."""
    batch = select("ragged", [0, 1, 2, 3])
    m, eng, a, cap = engine_for(batch, shell)
    outs = []
    for _ in range(3):
        eps, _, status = m.forward_async(*a, batch=4, edge_cap=cap, want_pocket=False)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        outs.append(eps.cpu().numpy().copy())
        a[0][:, :3] -= 0.5 * eps[:, :3]
    assert (eng.last_plan()[0], eng.last_plan()[1]) == PLAN
    eng.clear_pocket_frame()
    return np.stack(outs)


def test_shell_off_is_the_parent():
    """OPT_SHELL = 0: the outputs of a small chain are bit-identical to those of the commit before the option existed,
    recorded on an MI355X from a build of that commit's sources (tests/golden/cone_shell_parent_chain.npz, written by
    chain_outputs(None))."""
    want = np.load(GOLDEN)["eps"]
    got = chain_outputs(False)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
