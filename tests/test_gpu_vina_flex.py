"""GPU: dsbdd_vina_torsions, dsbdd_vina_intra and dsbdd_vina_flex (csrc/vina_torsion.h, vina_intra.h, vina_flex.h) through the
C ABI against their numpy restatements in diffsbdd_amd/vina.py -- integers EQUAL, floats inside the forward bound
`vina.intra_error_bound` evaluates --, the returned rows against separate launches on the returned pose bit for bit, the
geometry the pose must keep, one step replayed from the device's own rows, the one-torsion known answer, `dofs`, the edge
rows, bitwise reproducibility, and the front ends.  Outputs live in guarded sentinel buffers."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib, vina as V
from diffsbdd_amd.molecules import Molecule, write_sdf
from tests import _vina_cases as C
from tests import _vina_flex_cases as F
from tests import _vina_min_cases as MC
from tests import test_gpu_vina_kernels as K
from tests.test_gpu_vina_grad import _crystal, bits, launch_grad
from tests.test_gpu_vina_minimize import at_pose, launch_min

pytestmark = pytest.mark.gpu

DEV = K.DEV
FLEX_NAMES = ("atom", "mol", "flag", "grad", "mol_grad", "intra_atom", "intra_mol", "intra_flag", "intra_grad", "x", "pose",
              "energies", "stat", "theta", "tau")
INT_NAMES = ("flag", "intra_flag", "stat")
PER_ATOM = ("atom", "grad", "intra_atom", "intra_grad", "x")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return (t if t.numel() else torch.zeros(4, dtype=t.dtype, device=DEV)).data_ptr()


def launch_torsions(b):
    """dsbdd_vina_torsions on a batch of numpy inputs -> VinaTorsions of arrays (pair_mask rows nothing was written to hold
    the sentinel)."""
    t = {k: torch.as_tensor(np.ascontiguousarray(b[k]), device=DEV) for k in C.TYPE_KEYS}
    N, B = len(b["atom_type"]), len(b["mol_off"]) - 1
    shapes = ((B, V.TOR_INT), (B * V.MAX_TORSIONS, 2), (B * V.MAX_TORSIONS, V.MASK_WORDS), (N, V.MASK_WORDS))
    bufs = [K._guarded(*s) for s in shapes]
    rc = _lib.load().dsbdd_vina_torsions(_stream(), t["order"].data_ptr(), _ptr(t["atom_type"]), t["mol_off"].data_ptr(), B,
                                         len(b["class_elem"]), t["class_elem"].data_ptr(), b["order"].shape[1],
                                         *(buf[K.GUARD:].data_ptr() for buf in bufs))
    _lib.check(rc, "dsbdd_vina_torsions")
    torch.cuda.synchronize()
    assert all(K._intact(buf, s[0]) for buf, s in zip(bufs, shapes))
    K._unchanged(t, b, C.TYPE_KEYS)
    ints, ends, sides, mask = (buf.cpu().numpy()[K.GUARD:K.GUARD + s[0]] for buf, s in zip(bufs, shapes))
    return V.VinaTorsions(ints, ends.reshape(B, V.MAX_TORSIONS, 2), sides.reshape(B, V.MAX_TORSIONS, V.MASK_WORDS), mask,
                          np.asarray(b["mol_off"], np.int32))


def launch_intra(b, pair_mask=None):
    """dsbdd_vina_intra -> (atom [N,5], mol [B,8], flag [B], grad [N,3])."""
    pair_mask = b["tree"].pair_mask if pair_mask is None else pair_mask
    t = {k: torch.as_tensor(np.ascontiguousarray(b[k]), device=DEV) for k in ("lig_x", "lig_code", "mol_off")}
    pm = torch.as_tensor(np.ascontiguousarray(pair_mask), device=DEV)
    N, B = len(b["lig_x"]), len(b["mol_off"]) - 1
    shapes = ((N, V.ATOM_OUT), (B, V.MOL_OUT), (B, 0), (N, V.ATOM_GRAD))
    bufs = [K._guarded(*s) for s in shapes]
    rc = _lib.load().dsbdd_vina_intra(_stream(), _ptr(t["lig_x"]), _ptr(t["lig_code"]), t["mol_off"].data_ptr(), B, _ptr(pm),
                                      *(buf[K.GUARD:].data_ptr() for buf in bufs))
    _lib.check(rc, "dsbdd_vina_intra")
    torch.cuda.synchronize()
    assert all(K._intact(buf, s[0]) for buf, s in zip(bufs, shapes))
    K._unchanged(t, b, ("lig_x", "lig_code", "mol_off"))
    out = [buf.cpu().numpy()[K.GUARD:K.GUARD + s[0]] for buf, s in zip(bufs, shapes)]
    return out[0].view(np.float32), out[1].view(np.float32), out[2], out[3].view(np.float32)


def launch_flex(b, dofs=3, step=V.MIN_STEP, tol=V.MIN_TOL, max_evals=F.MAX_EVALS, tree=None):
    """dsbdd_vina_flex on a batch of numpy inputs with its tree -> dict of FLEX_NAMES."""
    tree = b["tree"] if tree is None else tree
    t = {k: torch.as_tensor(np.ascontiguousarray(b[k]), device=DEV) for k in C.SCORE_KEYS}
    tr = [torch.as_tensor(np.ascontiguousarray(v), device=DEV) for v in (tree.ints, tree.ends, tree.sides, tree.pair_mask)]
    N, B = len(b["lig_x"]), len(b["mol_off"]) - 1
    shapes = ((N, V.ATOM_OUT), (B, V.MOL_OUT), (B, 0), (N, V.ATOM_GRAD), (B, V.MOL_GRAD), (N, V.ATOM_OUT), (B, V.MOL_OUT), (B, 0),
              (N, V.ATOM_GRAD), (N, 3), (B, V.MOL_POSE), (B, V.MOL_FLEX), (B, V.MOL_STAT), (B, V.MAX_TORSIONS), (B, V.MAX_TORSIONS))
    bufs = [K._guarded(*s) for s in shapes]
    rc = _lib.load().dsbdd_vina_flex(_stream(), _ptr(t["lig_x"]), _ptr(t["lig_code"]), _ptr(t["mol_off"]), B, _ptr(t["mol_group"]),
                                     _ptr(t["mol_int"]), _ptr(t["poc_x"]), _ptr(t["poc_code"]), _ptr(t["group_off"]),
                                     len(b["group_off"]) - 1, *(_ptr(v) for v in tr), int(dofs), float(step), float(tol),
                                     int(max_evals), *(buf[K.GUARD:].data_ptr() for buf in bufs))
    _lib.check(rc, "dsbdd_vina_flex")
    torch.cuda.synchronize()
    assert all(K._intact(buf, s[0]) for buf, s in zip(bufs, shapes))          # nothing written before or after the outputs
    K._unchanged(t, b, C.SCORE_KEYS)
    got = [buf.cpu().numpy()[K.GUARD:K.GUARD + s[0]] for buf, s in zip(bufs, shapes)]
    return {name: (a if name in INT_NAMES else a.view(np.float32)) for name, a in zip(FLEX_NAMES, got)}


@functools.lru_cache(maxsize=None)
def relaxed():
    """`flex_batch()` relaxed with a budget of 24 evaluations: one launch, shared by the tests that read it."""
    return launch_flex(F.flex_batch())


def _inside(got, want, bound, what):
    return K._inside(got, want, bound, what)


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_torsion_tree_equals_the_restatement():
    for b in (F.torsion_batch(), C.type_batch(), {k: F.flex_batch()[k] for k in C.TYPE_KEYS}):
        want = V._vina_torsions_host(*(b[k] for k in C.TYPE_KEYS), fill=K.SENTINEL)
        got = launch_torsions(b)
        for name in ("ints", "ends", "sides", "pair_mask"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), (name, np.argwhere(getattr(got, name) != getattr(want, name))[:4])
        _, mol_int = K.launch_type(b)
        assert np.array_equal(got.found, mol_int[:, V.I_ROT])                # what dsbdd_vina_type counts on the same input
    tb = F.torsion_batch()
    got = launch_torsions(tb)
    assert got.ints[:, :2].tolist() == [[1, 1], [2, 2], [0, 0], [1, 1], [2, 2], [3, 3], [32, 37], [32, 125], [0, 125], [0, 0]]
    small = dict(tb, order=np.ascontiguousarray(tb["order"][:, :20, :20]))   # a smaller n_max: chain40 is longer, hence rigid
    want = V._vina_torsions_host(*(small[k] for k in C.TYPE_KEYS), fill=K.SENTINEL)
    got = launch_torsions(small)
    assert all(np.array_equal(getattr(got, n), getattr(want, n)) for n in ("ints", "ends", "sides", "pair_mask"))
    assert got.ints[6].tolist() == [0, 17, 0, 0]


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_intra_within_the_bound_reproducible_and_independent_of_the_batch():
    b = F.flex_batch()
    B, off = len(b["mol_off"]) - 1, b["mol_off"]
    want, margin, atom_bound, mol_bound, grad_bound = V._vina_intra_host(b["lig_x"], b["lig_code"], off, b["tree"].pair_mask, eps=V.EPS32)
    assert margin > C.MARGIN
    atom, mol, flag, grad = launch_intra(b)
    assert np.array_equal(flag, want.flag) and flag.sum() == 1 and flag[b["nan_mol"]] == 1
    fa = _inside(atom, want.atom, atom_bound, "intra atoms")
    fm = _inside(mol[:, :6], want.mol[:, :6], mol_bound, "intra molecules")
    fg = _inside(grad, want.grad, grad_bound, "intra gradient")
    live = flag == 0
    assert (mol[live, 6:] == 0).all() and np.isnan(mol[b["nan_mol"]]).all()
    for m in (b["rigid"], b["empty_mol"], b["empty_group"], b["untyped_mol"]):      # exact zeros without a rotor or a pair
        assert not mol[m].any() and not atom[off[m]:off[m + 1]].any() and not grad[off[m]:off[m + 1]].any(), m
    assert mol[b["folded"], 2] > 0 and mol[b["crystal"], 5] != 0 and mol[b["untyped_atom"], 1] > 0
    assert not atom[off[b["untyped_atom"]] + 2].any()
    print("largest error / bound (profiles/vina_intra_error.md): atoms %.3e, molecules %.3e, gradient %.3e" % (fa.max(), fm.max(), fg.max()))
    # twice, each alone, permuted
    again = launch_intra(b)
    assert all(np.array_equal(bits(u), bits(v)) for u, v in zip((atom, mol, flag, grad), again))
    for m in (b["crystal"], b["folded"], b["nan_mol"]):
        one, rows = F.sub_batch(b, [m])
        a1, m1, f1, g1 = launch_intra(one)
        assert np.array_equal(bits(a1), bits(atom[rows])) and np.array_equal(bits(m1[0]), bits(mol[m])) and f1[0] == flag[m]
        assert np.array_equal(bits(g1), bits(grad[rows])), m
    order = list(range(B))[::-1]
    rev, rows = F.sub_batch(b, order)
    ar, mr, fr, gr = launch_intra(rev)
    assert np.array_equal(bits(ar), bits(atom[rows])) and np.array_equal(bits(mr), bits(mol[order])) and np.array_equal(bits(gr), bits(grad[rows]))


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_returned_rows_are_those_of_separate_launches_on_the_returned_pose():
    b = F.flex_batch()
    got = relaxed()
    B = len(b["mol_off"]) - 1
    live = np.arange(B) != b["nan_mol"]
    there = at_pose(b, got["x"])
    for name, w in zip(FLEX_NAMES[:5], launch_grad(there)):
        assert np.array_equal(bits(got[name]), bits(w)), name
    for name, w in zip(FLEX_NAMES[5:9], launch_intra(there)):
        assert np.array_equal(bits(got[name]), bits(w)), name
    E = got["energies"]
    inter0, intra0 = launch_grad(b)[1][:, V.M_INTER], launch_intra(b)[1][:, V.M_INTER]
    assert np.array_equal(bits(E[:, V.E_START]), bits(inter0)) and np.array_equal(bits(E[:, V.X_INTRA_START]), bits(intra0))
    assert np.array_equal(bits(E[:, V.E_FINAL]), bits(got["mol"][:, V.M_INTER]))
    assert np.array_equal(bits(E[:, V.X_INTRA_FINAL]), bits(got["intra_mol"][:, V.M_INTER]))
    total = lambda a, c: (a.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert np.array_equal(bits(E[live, V.X_E_START]), bits(total(inter0, intra0)[live]))
    assert np.array_equal(bits(E[live, V.X_E_FINAL]), bits(total(got["mol"][:, V.M_INTER], got["intra_mol"][:, V.M_INTER])[live]))
    assert (E[live, V.X_E_FINAL] <= E[live, V.X_E_START]).all()
    assert (got["stat"][live, V.S_EVALS] <= F.MAX_EVALS + 1).all() and got["stat"][:, V.S_ACCEPTED].max() >= 5
    for m in (b["shifted"], b["folded"], b["decane"]):
        assert E[m, V.X_E_FINAL] < E[m, V.X_E_START], m


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_the_pose_keeps_every_rigid_distance_and_is_the_stored_pose():
    b = F.flex_batch()
    got = relaxed()
    off = b["mol_off"]
    used = [0.0, 0.0]
    for m in (b["crystal"], b["shifted"], b["folded"], b["decane"], b["untyped_atom"], b["rigid"]):
        rows = slice(off[m], off[m + 1])
        x0, x = b["lig_x"][rows], got["x"][rows]
        rotors = V.valid_torsions(b["tree"], m, len(x0))
        keep = F.distance_pairs(*b["graphs"][m], rotors)
        tol = F.distance_tolerance(x0, x, len(rotors))
        err = np.abs(F.distances(x) - F.distances(x0))[keep].max()
        assert err <= tol, (m, err, tol)
        theta = np.asarray([got["theta"][m, r[3]] for r in rotors], np.float64)
        again = V.torsion_coordinates(x0, rotors, theta, got["pose"][m, V.P_SHIFT].astype(np.float64), got["pose"][m, V.P_QUAT].astype(np.float64))
        gap = np.abs(again.astype(np.float64) - x).max()
        assert gap <= F.pose_tolerance(x), (m, gap)
        used = [max(used[0], err / tol), max(used[1], gap / F.pose_tolerance(x))]
    print("largest fraction of the distance tolerance, of the pose tolerance:", used)
    assert np.abs(got["theta"][b["folded"]]).max() > 1e-3 and np.abs(got["theta"][b["shifted"]]).max() > 1e-3      # torsions did turn
    assert not got["theta"][b["rigid"]].any() and not got["theta"][b["folded"], 4:].any()


def replay_step(one, tree, dofs, step):
    """The first trial of the one-molecule batch `one`, built on the host from the device's own rows at the input pose
    (dsbdd_vina_score_grad, dsbdd_vina_intra) by `flex_geometry`, `flex_slope`, `flex_step` and `torsion_coordinates` with the
    rotors `valid_torsions` keeps.  -> (xt float32, theta, rotors, tau, E at the input)."""
    x0 = one["lig_x"]
    _, mol0, _, g0, mg0 = launch_grad(one)
    _, imol0, _, ig0 = launch_intra(one, tree.pair_mask)
    rotors = V.valid_torsions(tree, 0, len(x0), dofs)
    Fn, M = mg0[0, V.G_NET].astype(np.float64), mg0[0, V.G_MOMENT].astype(np.float64)
    c, rho2, rho_max, tau, reach, rho2k = V.flex_geometry(x0, rotors, g0.astype(np.float64) + ig0.astype(np.float64))
    u = V.flex_slope(Fn, M, rho2, rho_max, tau, reach, rho2k, dofs)
    t, q, theta = V.flex_step(np.zeros(3), [1.0, 0, 0, 0], np.zeros(len(rotors)), Fn, M, tau, c, rho2, rho2k, float(np.float32(step)) / u, dofs)
    return V.torsion_coordinates(x0, rotors, theta, t, q), theta, rotors, tau, float(mol0[0, V.M_INTER]) + float(imol0[0, V.M_INTER])


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_one_step_replayed_from_the_device_rows():
    b = F.flex_batch()
    cases = [F.sub_batch(b, [m])[0] for m in (b["shifted"], b["folded"])] + [dict(F.one_torsion(90.0), tree=F.one_torsion_tree()),
                                                                             dict(F.one_torsion(20.0), tree=F.one_torsion_tree())]
    seen = set()
    for k, one in enumerate(cases):
        dofs = 3 if k < 2 else 2
        step = V.MIN_STEP if k < 3 else 2.0                                  # the last case, 7 degrees from its well, steps 80 degrees: rejected
        x0 = one["lig_x"]
        xt, theta, rotors, tau, E0 = replay_step(one, one["tree"], dofs, step)
        L = float(np.float32(step))
        moved = np.sqrt(((xt.astype(np.float64) - x0) ** 2).sum(1)).max()
        # no atom moves more than L, plus the two roundings: each end of the displacement is a float32 point, off the float64 one
        # by at most half an ulp <= EPS32 |x| per component, sqrt(3) EPS32 |x|max per point
        assert 0 < moved <= L + 2 * np.sqrt(3.0) * V.EPS32 * max(np.abs(xt).max(), np.abs(x0).max())
        trial = at_pose(one, xt)
        mol1, imol1 = launch_grad(trial)[1], launch_intra(trial)[1]
        E1 = float(mol1[0, V.M_INTER]) + float(imol1[0, V.M_INTER])
        bound = sum(V.error_bound(*(v[key] for key in C.SCORE_KEYS))[1][0, V.M_INTER] +
                    V.intra_error_bound(v["lig_x"], v["lig_code"], v["mol_off"], one["tree"].pair_mask)[1][0, V.M_INTER] for v in (one, trial))
        print(f"case {k}: E = {E0!r}, E' = {E1!r}, twice the summed bounds {2 * bound:.3e}")
        got = launch_flex(one, dofs=dofs, step=step, max_evals=2)
        accepted = bool(got["stat"][0, V.S_ACCEPTED])
        if abs(E1 - E0) > 2 * bound:                                         # the decision does not hang on a rounding: it must match
            assert accepted == (E1 < E0), k
            seen.add(accepted)
        assert got["stat"][0].tolist() == [0, 2 if accepted else 3, int(accepted), 0], k
        assert np.array_equal(bits(got["energies"][0, V.X_E_START]), bits(np.float32(E0)))
        if accepted:
            assert (np.abs(got["x"].astype(np.float64) - xt) <= MC.ulp32(xt)).all(), k
            assert got["energies"][0, V.E_STEP] == np.float32(step)
            assert (np.abs(got["theta"][0, [r[3] for r in rotors]].astype(np.float64) - theta) <= MC.ulp32(theta)).all(), k      # one rounding
        else:
            assert np.array_equal(bits(got["x"]), bits(x0)), k
            assert got["energies"][0, V.E_STEP] == 0 and got["pose"][0, :7].tolist() == [0, 0, 0, 1, 0, 0, 0] and not got["theta"].any()
            slots = [r[3] for r in rotors]                                  # the torques of the input pose: one float32 rounding
            assert (np.abs(got["tau"][0, slots].astype(np.float64) - tau) <= MC.ulp32(tau)).all(), k
    assert seen == {True, False}


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_one_torsion_known_answer_on_the_device():
    wells = F.one_torsion_wells()
    parts = [F.one_torsion(90.0), F.one_torsion(30.0)]
    b = dict(parts[0])
    b["lig_x"], b["lig_code"] = np.concatenate([p["lig_x"] for p in parts]), np.concatenate([p["lig_code"] for p in parts])
    b["mol_off"], b["mol_group"] = np.asarray([0, 4, 8], np.int32), np.zeros(2, np.int32)
    b["mol_int"] = np.concatenate([p["mol_int"] for p in parts])
    one = F.one_torsion_tree()
    tree = V.VinaTorsions(*(np.concatenate([v, v]) for v in (one.ints, one.ends, one.sides, one.pair_mask)), b["mol_off"])
    got = launch_flex(b, dofs=2, max_evals=V.MIN_EVALS, tree=tree)
    for k, well in enumerate((wells[1], wells[0])):
        x = got["x"][4 * k:4 * k + 4]
        arc = np.deg2rad(abs(F.dihedral_deg(x) - well)) * F.RADIUS
        print(f"start {(90.0, 30.0)[k]}: dihedral {F.dihedral_deg(x):.4f}, well {well:.4f}, stat {got['stat'][k].tolist()}")
        assert V.STATUS[got["stat"][k, V.S_STATUS]] == "converged" and arc <= 2 * V.MIN_TOL, (k, arc)
        assert np.array_equal(bits(x[:3]), bits(b["lig_x"][4 * k:4 * k + 3])) and got["intra_mol"][k, 5] == 0


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_dofs_switch_blocks_off():
    b = F.flex_batch()
    sel = [b["shifted"], b["folded"], b["decane"]]
    part, _ = F.sub_batch(b, sel)
    off = part["mol_off"]
    rigid = launch_flex(part, dofs=1)
    assert not rigid["theta"].any() and rigid["stat"][:, V.S_ACCEPTED].max() >= 1
    pose = rigid["pose"].copy()
    for m in range(3):                                                      # x = t + R(q) x0: as the rigid suite checks it, about the origin
        x0, x = part["lig_x"][off[m]:off[m + 1]], rigid["x"][off[m]:off[m + 1]]
        assert np.abs(F.distances(x) - F.distances(x0)).max() <= MC.distance_tolerance(np.concatenate([x, x0]))
        again = V.torsion_coordinates(x0, [], [], pose[m, V.P_SHIFT].astype(np.float64), pose[m, V.P_QUAT].astype(np.float64))
        assert np.abs(again.astype(np.float64) - x).max() <= F.pose_tolerance(x)
    tors = launch_flex(part, dofs=2)
    assert tors["pose"][:, :7].tolist() == [[0, 0, 0, 1, 0, 0, 0]] * 3 and np.abs(tors["theta"]).max() > 1e-3
    for m in range(3):
        n = off[m + 1] - off[m]
        outside = ~np.any([r[2] for r in V.valid_torsions(part["tree"], m, n)], axis=0)
        rows = np.arange(off[m], off[m + 1])[outside]
        assert outside.any() and np.array_equal(bits(tors["x"][rows]), bits(part["lig_x"][rows])), m
        assert tors["energies"][m, V.X_E_FINAL] <= tors["energies"][m, V.X_E_START]


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_edge_rows():
    b = F.flex_batch()
    got = relaxed()
    off, stat, E = b["mol_off"], got["stat"], got["energies"]
    for m in (b["empty_mol"], b["empty_group"], b["bad_group"], b["untyped_mol"]):      # the rows the rigid suite expects
        rows = slice(off[m], off[m + 1])
        assert stat[m].tolist() == [2, 1, 0, 0] and np.array_equal(bits(got["x"][rows]), bits(b["lig_x"][rows])), m
        assert got["pose"][m, :7].tolist() == [0, 0, 0, 1, 0, 0, 0] and not E[m].any() and not got["grad"][rows].any()
        assert not got["theta"][m].any() and not got["tau"][m].any()
    m = b["rigid"]                                                          # zero rotors: a rigid relaxation, no intramolecular term
    rows = slice(off[m], off[m + 1])
    assert stat[m, V.S_STATUS] in (0, 1) and 2 <= stat[m, V.S_EVALS] <= F.MAX_EVALS + 1 and E[m, V.X_E_FINAL] <= E[m, V.X_E_START]
    assert not got["theta"][m].any() and not got["tau"][m].any() and E[m, V.X_INTRA_FINAL] == 0 and E[m, V.X_INTRA_START] == 0
    assert np.abs(F.distances(got["x"][rows]) - F.distances(b["lig_x"][rows])).max() <= MC.distance_tolerance(got["x"][rows])
    m = b["nan_mol"]
    rows = slice(off[m], off[m + 1])
    assert stat[m].tolist() == [3, 0, 0, 0] and got["flag"][m] == 1 and got["intra_flag"][m] == 1 and got["flag"].sum() == 1
    assert np.array_equal(bits(got["x"][rows]), bits(b["lig_x"][rows]))
    for name in ("atom", "grad", "intra_atom", "intra_grad"):
        assert np.isnan(got[name][rows]).all(), name
    for name in ("mol", "mol_grad", "intra_mol", "pose", "energies", "theta", "tau"):
        assert np.isnan(got[name][m]).all(), name
    # 33 or more rotors, and a molecule longer than n_max: the first 32 turn, the long one is a rigid body
    rng = np.random.RandomState(8)
    chain40 = F.chain_coordinates(np.deg2rad(rng.choice([60.0, -60.0, 180.0], 37)))
    t = F.type_inputs([C.chain(40), C.chain(40)], n_max=40)
    short = dict(t, order=np.ascontiguousarray(t["order"][:, :30, :30]))     # n_max 30 < 40: molecule 1's tree comes from here
    tree_a, tree_b = launch_torsions(t), launch_torsions(short)
    tree = V.VinaTorsions(*(np.concatenate([u[:1] if u.shape[0] == 2 else u[:40], v[1:] if v.shape[0] == 2 else v[40:]])
                            for u, v in zip((tree_a.ints, tree_a.ends, tree_a.sides, tree_a.pair_mask),
                                            (tree_b.ints, tree_b.ends, tree_b.sides, tree_b.pair_mask))), t["mol_off"])
    assert tree.ints[:, :2].tolist() == [[32, 37], [0, 27]]
    code, mol_int = V._vina_type_host(*(t[k] for k in C.TYPE_KEYS))
    pocket = F._pocket_around(chain40.astype(np.float64), rng, 30)
    long = {"lig_x": np.concatenate([chain40, chain40]), "lig_code": code, "mol_off": t["mol_off"], "mol_group": np.zeros(2, np.int32),
            "mol_int": mol_int, "poc_x": pocket, "poc_code": np.full(30, 17, np.int32), "group_off": np.asarray([0, 30], np.int32)}
    out = launch_flex(long, tree=tree)
    assert np.abs(out["theta"][0, :32]).max() > 1e-3 and not out["theta"][1].any() and out["energies"][1, V.X_INTRA_FINAL] == 0
    x0, x = chain40, out["x"][40:]
    assert np.abs(F.distances(x) - F.distances(x0)).max() <= MC.distance_tolerance(np.concatenate([x, x0]))      # rigid
    keep = F.distance_pairs(*C.chain(40), V.valid_torsions(tree, 0, 40))
    assert np.abs(F.distances(out["x"][:40]) - F.distances(x0))[keep].max() <= F.distance_tolerance(x0, out["x"][:40])
    # a rotor with an end out of range, built on the host: dropped, the others turn
    one, _ = F.sub_batch(b, [b["folded"]])
    bad = V.VinaTorsions(one["tree"].ints.copy(), one["tree"].ends.copy(), one["tree"].sides.copy(), one["tree"].pair_mask, one["mol_off"])
    bad.ends[0, 1] = (3, 700)
    bad.ends[0, 2] = (-5, 4)
    bad.sides[0, 0, 3] = -1                                                 # side bits far above n
    bad.ints[0, 0] = 99                                                     # clamped to 32; slots 4.. hold -1 ends and are dropped
    out = launch_flex(one, tree=bad)
    assert [r[3] for r in V.valid_torsions(bad, 0, 7)] == [0, 3]
    # one step of the device on the malformed tree against that step built from the device's own rows with the rotors the
    # restatement's check keeps: the same slots turn, by the same angles (one float32 rounding), to the same coordinates
    xt, theta, rotors, _, _ = replay_step(one, bad, 3, V.MIN_STEP)
    step1 = launch_flex(one, tree=bad, max_evals=2)
    assert step1["stat"][0].tolist() == [0, 2, 1, 0] and np.nonzero(step1["theta"][0])[0].tolist() == [0, 3] == [r[3] for r in rotors]
    assert (np.abs(step1["theta"][0, [0, 3]].astype(np.float64) - theta) <= MC.ulp32(theta)).all()
    assert (np.abs(step1["x"].astype(np.float64) - xt) <= MC.ulp32(xt)).all()
    assert out["theta"][0, 1] == 0 and out["theta"][0, 2] == 0 and not out["theta"][0, 4:].any()
    assert np.abs(out["theta"][0, [0, 3]]).max() > 1e-3 and out["energies"][0, V.X_E_FINAL] < out["energies"][0, V.X_E_START]
    assert np.isfinite(out["x"]).all()


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_bitwise_reproducible_and_independent_of_the_batch():
    b = F.flex_batch()
    B = len(b["mol_off"]) - 1
    first, again = relaxed(), launch_flex(b)
    assert all(np.array_equal(bits(first[k]), bits(again[k])) for k in FLEX_NAMES)
    for m in (b["shifted"], b["decane"]):                                   # each alone
        one, rows = F.sub_batch(b, [m])
        got = launch_flex(one)
        for name in FLEX_NAMES:
            want = first[name][rows] if name in PER_ATOM else first[name][m:m + 1]
            assert np.array_equal(bits(got[name]), bits(want)), (m, name)
    order = np.random.RandomState(4).permutation(B).tolist()
    perm, rows = F.sub_batch(b, order)
    got = launch_flex(perm)
    for name in FLEX_NAMES:
        want = first[name][rows] if name in PER_ATOM else first[name][order]
        assert np.array_equal(bits(got[name]), bits(want)), name


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_front_end_on_the_displaced_fixture_and_without_atoms():
    z = C.fixture()
    x, at, mask, pockets, decoder, orders = _crystal(z, "5ndu")
    moved = MC.rigid_motion(z["5ndu_crystal_x"])
    xm = torch.as_tensor(moved, device=DEV)
    keep = xm.clone()
    plain = V.vina_minimize(xm, at, mask, pockets, decoder, orders=orders, max_evals=40)
    st = V.vina_minimize(xm, at, mask, pockets, decoder, orders=orders, max_evals=40, torsions=True)
    assert type(plain) is V.VinaMinimized and isinstance(st, V.VinaFlexed) and torch.equal(xm, keep)
    assert tuple(st.energies.shape) == (1, 8) and tuple(st.theta.shape) == (1, 32) and int(st.n_torsions[0]) == 10 == int(st.torsions_found[0])
    ref = V.vina_gradient(st.x, at, mask, pockets, decoder, orders=orders)
    assert torch.equal(ref.mol.view(torch.int32), st.mol.view(torch.int32)) and torch.equal(ref.grad.view(torch.int32), st.grad.view(torch.int32))
    own = V.vina_intra(st.x, at, mask, decoder, orders=orders)
    assert torch.equal(own.mol.view(torch.int32), st.intra_out.mol.view(torch.int32)) and torch.equal(own.intra, st.intra)
    start = V.vina_score(xm, at, mask, pockets, decoder, orders=orders)
    assert torch.equal(start.inter, st.inter_start) and torch.equal(V.vina_intra(xm, at, mask, decoder, orders=orders).intra, st.intra_start)
    assert float(st.energies[0, V.X_E_FINAL]) <= float(st.energies[0, V.X_E_START]) and float(st.rmsd[0]) > 0
    print(f"5ndu displaced: E {float(st.energies[0, 6]):.4f} -> {float(st.energies[0, 7]):.4f} with torsions; "
          f"inter {float(plain.inter_start[0]):.4f} -> {float(plain.inter[0]):.4f} rigid")
    rec, = st.molecules()
    assert isinstance(rec, V.MolVinaFlex) and rec.n_torsions == 10 and rec.intra == float(st.intra[0]) and rec.theta.shape == (32,)
    assert {"intra", "intra_start", "n_torsions", "torsions_found"} <= set(rec.as_dict())
    # without the keyword: today's launches, today's bits
    direct = launch_min({"lig_x": moved, "lig_code": plain.lig_code.cpu().numpy(), "mol_off": np.asarray([0, len(x)], np.int32),
                         "mol_group": np.zeros(1, np.int32), "mol_int": plain.mol_int.cpu().numpy(), "poc_x": pockets.x.cpu().numpy(),
                         "poc_code": pockets.code.cpu().numpy(), "group_off": pockets.group_off.cpu().numpy()}, max_evals=40)
    for name, t in (("x", plain.x), ("mol", plain.mol), ("energies", plain.energies), ("stat", plain.stat), ("pose", plain.pose)):
        assert np.array_equal(bits(direct[name]), bits(t.cpu().numpy())), name
    with pytest.raises(ValueError, match="dofs"):
        V.vina_minimize(xm, at, mask, pockets, decoder, orders=orders, torsions=True, dofs=4)
    # N = 0
    empty = lambda: (torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV))
    none = V.vina_minimize(*empty(), pockets, "crossdock", batch=0, torsions=True)
    assert tuple(none.x.shape) == (0, 3) and tuple(none.energies.shape) == (0, 8) and none.molecules() == []
    hollow = V.vina_minimize(*empty(), pockets, "crossdock", batch=3, torsions=True)
    assert hollow.stat.cpu().tolist() == [[2, 1, 0, 0]] * 3 and not hollow.energies.cpu().numpy().any() and len(hollow.molecules()) == 3
    assert V.minimize_molecules([], pockets, torsions=True) == [] and V.intra_molecules([]) == []
    # the tree and the intramolecular term through their own front ends, on the same ligand
    el, bonds = C.fixture_ligand(z, "5ndu")
    tree = V.ligand_torsions(xm, at, mask, decoder, orders=orders)
    host = V._vina_torsions_host(orders.cpu().numpy(), at.cpu().numpy(), [0, len(x)], V.class_table(decoder))
    for name in ("ints", "ends", "sides", "pair_mask"):
        assert np.array_equal(getattr(tree, name).cpu().numpy(), getattr(host, name)), name
        assert torch.equal(getattr(tree, name), getattr(st.intra_out.torsions, name)), name
    assert tree.kept.cpu().tolist() == [10] and tree.found.cpu().tolist() == [10]
    rec, = V.intra_molecules([(moved, el, bonds)], device=DEV, bonds="file")
    assert isinstance(rec, V.MolVinaIntra) and rec.n_torsions == 10 and rec.torsions_found == 10 and rec.nonfinite == 0
    assert np.float32(rec.intra) == np.float32(float(st.intra_start[0])) and rec.grad.shape == (len(x), 3) and rec.atom.shape == (len(x), 5)
    with pytest.raises(_lib.HipLibraryError):
        V.ligand_torsions(xm.cpu(), at.cpu(), mask.cpu(), decoder, orders=orders.cpu())


def test_generator_and_command_line_with_torsions(tmp_path, capsys):
    from tests.test_gpu_ligand_design import generator
    from tests.test_gpu_vina import _fixture_pdb
    from tests.test_ligand_design import PDB
    pdb = tmp_path / "c.pdb"
    pdb.write_text(PDB)
    gen, _ = generator("small_cond")
    residues = gen.select_pocket_residues(str(pdb), ref_ligand="A:100")
    job = [(residues, 2, torch.tensor([9, 14]))]
    (mols,) = gen.generate_for_pockets(job, timesteps=4, seed=5, sample_ids=torch.arange(2),
                                       vina={"minimize": {"max_evals": 30, "torsions": True}})
    out = gen.vina_minimize(str(pdb), mols, ref_ligand="A:100", scope="pocket", max_evals=30, torsions=True)
    for m, o in zip(mols, out):
        rec = m.vina_min
        assert isinstance(rec, V.MolVinaFlex) and rec.inter_start == m.vina.inter and rec.evals <= 31 and rec.theta.shape == (32,)
        assert rec.n_torsions == min(rec.torsions_found, 32) and rec.torsions_found == m.vina.n_rot
        assert np.array_equal(o["x"], rec.x) and o["intra"] == rec.intra and np.array_equal(o["theta"], rec.theta)
    # the command line
    z = C.fixture()
    pdb, sdf, csv, sdf_out = tmp_path / "p.pdb", tmp_path / "l.sdf", tmp_path / "scores.csv", tmp_path / "relaxed.sdf"
    _fixture_pdb(pdb, z, "5ndu")
    el, bonds = C.fixture_ligand(z, "5ndu")
    bonds = [(max(i, j), min(i, j), o) for i, j, o in bonds]
    write_sdf(str(sdf), [Molecule(MC.rigid_motion(z["5ndu_crystal_x"]), el, bonds)])
    rows = V.main(["--pdbfile", str(pdb), "--sdf", str(sdf), "--bonds", "file", "--out", str(csv), "--minimize", str(sdf_out),
                   "--torsions", "--max_evals", "40", "--device", DEV])
    err = capsys.readouterr().err
    assert V.VINA_FLEX_COVERAGE in err and V.VINA_MIN_COVERAGE not in err
    lines = csv.read_text().splitlines()
    assert lines[0].split(",") == ["source", "index"] + list(V.FLEX_CSV_COLUMNS) and lines[0].endswith("intra,intra_start,n_torsions")
    cells = dict(zip(lines[0].split(","), lines[1].split(",")))
    rec = rows[0][2]
    assert float(cells["intra"]) == rec.intra and float(cells["intra_start"]) == rec.intra_start and int(cells["n_torsions"]) == 10
    (xyz, elements, bd), = V.read_sdf_records(str(sdf_out))
    assert elements == el and np.abs(xyz - rec.x).max() <= 0.5e-4 + 1e-6
    plain = V.main(["--pdbfile", str(pdb), "--sdf", str(sdf), "--bonds", "file", "--out", str(tmp_path / "m.csv"), "--minimize",
                    str(tmp_path / "m.sdf"), "--max_evals", "40", "--device", DEV])
    assert (tmp_path / "m.csv").read_text().splitlines()[0].split(",") == ["source", "index"] + list(V.MIN_CSV_COLUMNS)
    assert type(plain[0][2]) is V.MolVinaMin
