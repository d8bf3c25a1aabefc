"""The rigid-body minimiser's float64 restatement `vina._vina_minimize_host` (the specification of dsbdd_vina_minimize): the
one-atom cases against the wells of the pair energy, monotone and rigid on the scoring batch, the budget, the degenerate
molecules, and the C entry's and the front ends' argument checks.  No GPU."""
import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib, vina as V
from tests import _vina_cases as C
from tests import _vina_min_cases as MC


def _host(b, **settings):
    return V._vina_minimize_host(*(b[k] for k in C.SCORE_KEYS), **settings)


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_one_atom_on_a_line_ends_in_the_well_it_started_in():
    d_in, d_out = MC.well(-0.5, 0.5), MC.well(2.0, 4.0)
    assert 0.002 < d_in < 0.004 and abs(d_out - 3.0) < 1e-3                   # near 0.0029; the outer well is gauss2's, at d = 3
    d = np.linspace(d_in, d_out, 2001)
    assert MC.pair_energy(d).max() > max(MC.pair_energy(2.2), MC.pair_energy(0.7))     # a barrier between r0 = 4.5 and 6.0
    for r0 in MC.STARTS:
        st = _host(MC.one_atom(r0))
        r = float(np.linalg.norm(st.x[0].astype(np.float64)))
        print(f"r0 = {r0}: r_final = {r:.5f}, target {MC.target(r0):.5f}, stat {st.stat[0].tolist()}, energies {st.energies[0].tolist()}")
        assert st.stat[0, V.S_STATUS] == 1 and st.stat[0, V.S_EVALS] <= V.MIN_EVALS
        assert abs(r - MC.target(r0)) <= 2 * MC.TOL, (r0, r)
        assert st.energies[0, V.E_FINAL] < st.energies[0, V.E_START]
        # one atom: no moment arm, the quaternion's rotation moves nothing, the atom stays on the line
        off_line = np.linalg.norm(np.cross(st.x[0].astype(np.float64), MC.AXIS))
        assert off_line <= 1e-5                                               # float32 roundings of a 3 ... 7 A vector, some steps
    assert MC.target(4.5) == MC.target(3.0) == pytest.approx(3.8029, abs=2e-4) and MC.target(6.0) == pytest.approx(6.8, abs=1e-3)
    # the three as one batch: the same results, molecule by molecule
    st = _host(MC.one_atom_batch())
    for k, r0 in enumerate(MC.STARTS):
        one = _host(MC.one_atom(r0))
        assert np.array_equal(st.x[k], one.x[0]) and np.array_equal(st.stat[k], one.stat[0]) and np.array_equal(st.pose[k], one.pose[0])


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_monotone_and_rigid_on_the_scoring_batch():
    b = C.score_batch()
    st, trace = MC.min_reference()
    B = len(b["mol_off"]) - 1
    live = np.asarray([m != b["nan_mol"] for m in range(B)])
    assert (st.energies[live, V.E_FINAL] <= st.energies[live, V.E_START]).all()
    assert (st.stat[:, V.S_ACCEPTED] <= st.stat[:, V.S_EVALS]).all() and (st.stat[:, 3] == 0).all()
    assert [sum(1 for k, _ in trace if k == m) for m in range(B)] == [int(v) if m != b["nan_mol"] else 1
                                                                       for m, v in enumerate(st.stat[:, V.S_EVALS])]
    moved = st.stat[:, V.S_ACCEPTED] > 0
    assert moved.sum() >= 10 and (st.energies[moved, V.E_FINAL] < st.energies[moved, V.E_START]).all()
    assert (st.energies[moved, V.E_STEP] > 0).all() and (st.energies[~moved & live, V.E_STEP] == 0).all()
    # the accepted energies of a molecule descend strictly (float32), whatever was tried in between
    for m in np.nonzero(moved)[0]:
        e, best, count = [v for k, v in trace if k == m], None, -1
        for v in e:
            if best is None or v < best:
                best, count = v, count + 1
        assert count == st.stat[m, V.S_ACCEPTED] and np.float32(st.energies[m, V.E_FINAL]) == best, m
    # the returned rows are those of the gradient's restatement at the returned coordinates
    at = dict(b)
    at["lig_x"] = st.x
    g = V._vina_grad_host(*(at[k] for k in C.SCORE_KEYS))
    assert np.allclose(g.mol[live], st.mol[live], rtol=1e-12, atol=1e-12) and np.allclose(g.grad, st.grad, rtol=1e-9, atol=1e-12, equal_nan=True)
    assert np.array_equal(np.float32(g.mol[live, V.M_INTER]), np.float32(st.energies[live, V.E_FINAL]))
    # rigid: x from the pose, distances preserved; the molecule with the NaN keeps its input
    used = MC.check_rigid(b["lig_x"], st.x, st.pose, b["mol_off"], skip=(b["nan_mol"],))
    print("largest fraction of the pose tolerance, of the distance tolerance:", used)
    assert st.x.dtype == np.float32 and np.isfinite(np.delete(st.x, np.r_[b["mol_off"][9]:b["mol_off"][10]], 0)).all()
    # with the float64 pose the coordinates are reproduced exactly: they are a function of x0 and the pose alone
    off = b["mol_off"]
    for m in np.nonzero(live)[0]:
        lo, hi = off[m], off[m + 1]
        assert np.array_equal(st.x[lo:hi], V.pose_coordinates(b["lig_x"][lo:hi], st.pose[m, V.P_SHIFT], st.pose[m, V.P_QUAT])), m
    rmsd = st.rmsd
    assert rmsd.shape == (B,) and (rmsd[moved] > 0).all() and (rmsd[~moved & live] == 0).all() and np.isnan(rmsd[b["nan_mol"]])
    assert np.allclose(st.score_start[live], st.energies[live, V.E_START] * st.mol_grad[live, V.G_ROT])


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_budget():
    b = C.score_batch()
    st = _host(b, max_evals=1)
    live = np.arange(16) != b["nan_mol"]
    assert np.isin(st.stat[live, V.S_STATUS], (0, 2)).all() and (st.stat[live, V.S_EVALS] == 1).all() and not st.stat[:, V.S_ACCEPTED].any()
    assert (st.stat[live, V.S_STATUS] == 0).sum() == 11
    assert np.array_equal(st.x.view(np.int32), b["lig_x"].view(np.int32))
    assert np.array_equal(st.pose[live][:, :7], np.tile([0, 0, 0, 1, 0, 0, 0], (15, 1))) and (st.pose[live, V.P_RHO2] >= 1).all()
    assert np.array_equal(st.energies[live, V.E_START], st.energies[live, V.E_FINAL])
    g = V._vina_grad_host(*(b[k] for k in C.SCORE_KEYS))
    assert np.allclose(st.mol[live], g.mol[live], rtol=1e-12, atol=1e-12)
    # a budget of two: one trial; rejected, it is evaluated away again (3 evaluations), accepted, it stands (2)
    two = _host(b, max_evals=2)
    tried = two.stat[:, V.S_STATUS] == 0
    assert tried.sum() == 11 and np.array_equal(two.stat[tried, V.S_EVALS], 3 - two.stat[tried, V.S_ACCEPTED])
    # the defaults suffice for every molecule
    full, _ = MC.min_reference()
    print("status, evals, accepted:", full.stat[:, :3].tolist())
    assert np.isin(full.stat[:, V.S_STATUS], (1, 2, 3)).all() and full.stat[:, V.S_EVALS].max() <= V.MIN_EVALS
    assert (full.stat[:, V.S_STATUS] == 1).sum() == 11 and full.stat[:, V.S_EVALS].max() > 50


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_conventions_of_the_degenerate_molecules():
    b = C.score_batch()
    st, _ = MC.min_reference()
    off = b["mol_off"]
    for m in (b["empty_mol"], 0, b["untyped_mol"], 10):                       # no atoms, empty group, all untyped, group id out of range
        rows = slice(off[m], off[m + 1])
        assert st.stat[m].tolist() == [2, 1, 0, 0], m
        assert np.array_equal(st.x[rows].view(np.int32), b["lig_x"][rows].view(np.int32)), m
        assert not st.grad[rows].any() and not st.mol[m].any() and st.energies[m].tolist() == [0, 0, 0, 0] and st.flag[m] == 0
        assert st.pose[m, :7].tolist() == [0, 0, 0, 1, 0, 0, 0]
    m = b["nan_mol"]
    rows = slice(off[m], off[m + 1])
    assert st.stat[m].tolist() == [3, 0, 0, 0] and st.flag[m] == 1
    assert np.array_equal(st.x[rows].view(np.int32), b["lig_x"][rows].view(np.int32))
    assert np.isnan(st.pose[m]).all() and np.isnan(st.energies[m]).all() and np.isnan(st.grad[rows]).all() and np.isnan(st.mol[m, :7]).all()
    assert st.flag.sum() == 1


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_c_entry_refuses_bad_arguments_without_a_launch():
    lib = _lib.load()
    buf, other = np.zeros(64, np.int32), np.zeros(64, np.int32)
    p, x_out = buf.ctypes.data, other.ctypes.data
    good = [None, p, p, p, 1, p, p, p, p, p, 1, p, p, p, p, p, 0.25, 1e-3, 200, x_out, p, p, p]
    assert len(_lib.SIGNATURES["dsbdd_vina_minimize"][1]) == 23 and _lib.ABI_VERSION == 6 == lib.dsbdd_abi_version()
    assert lib.dsbdd_vina_minimize(*(good[:4] + [0] + good[5:])) == _lib.OK                    # batch 0: nothing launched
    assert lib.dsbdd_vina_minimize(*(good[:4] + [-1] + good[5:])) == _lib.ERR_ARG
    assert lib.dsbdd_vina_minimize(*(good[:10] + [-1] + good[11:])) == _lib.ERR_ARG
    for k in (1, 2, 3, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 19, 20, 21, 22):
        args = list(good)
        args[k] = None
        assert lib.dsbdd_vina_minimize(*args) == _lib.ERR_ARG and b"null" in lib.dsbdd_last_error(), k
    for k, bad in ((16, 0.0), (16, -0.25), (16, float("nan")), (16, float("inf")), (17, 0.0), (17, -1e-3), (17, float("nan")),
                   (17, float("inf")), (18, 0), (18, -1), (18, V.MAX_EVALS + 1)):
        args = list(good)
        args[k] = bad
        assert lib.dsbdd_vina_minimize(*(args[:4] + [0] + args[5:])) == _lib.ERR_ARG, (k, bad)   # refused before batch 0 returns
    assert b"max_evals" in lib.dsbdd_last_error()
    assert lib.dsbdd_vina_minimize(*(good[:4] + [0] + good[5:18] + [V.MAX_EVALS] + good[19:])) == _lib.OK
    aliased = list(good)
    aliased[19] = p
    assert lib.dsbdd_vina_minimize(*aliased) == _lib.ERR_ARG and b"alias" in lib.dsbdd_last_error()
    assert lib.dsbdd_vina_minimize(*(aliased[:4] + [0] + aliased[5:])) == _lib.OK              # batch 0: nothing is read or written
    assert not buf.any() and not other.any()


def test_front_end_argument_handling(tmp_path):
    x, t, m = torch.zeros((2, 3)), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    pocket = V.TypedPocket(np.zeros((1, 3), np.float32), np.asarray([1], np.int32))
    with pytest.raises(_lib.HipLibraryError, match="vina_minimize"):
        V.vina_minimize(x, t, m, [pocket], "crossdock")
    with pytest.raises(_lib.HipLibraryError, match="minimize_molecules"):
        V.minimize_molecules([(np.zeros((1, 3)), ["C"])], [pocket], device="cpu")
    for bad in (dict(step=0), dict(tol=float("nan")), dict(max_evals=0), dict(max_evals=V.MAX_EVALS + 1), dict(max_evals=2.5)):
        with pytest.raises(ValueError):
            V._settings(**{**dict(step=0.25, tol=1e-3, max_evals=200), **bad})
    assert V._settings(0.25, 1e-3, 200) == (0.25, float(np.float32(1e-3)), 200)
    a = V.parse_args(["--pdbfile", "p.pdb", "--sdf", "a.sdf", "--minimize", "r.sdf", "--step", "0.5", "--max_evals", "50"])
    assert (a.minimize, a.step, a.tol, a.max_evals) == ("r.sdf", 0.5, V.MIN_TOL, 50)
    assert V.parse_args(["--pdbfile", "p.pdb", "--sdf", "a.sdf"]).minimize is None
    for word in ("rigid", "no torsions", "protein is rigid", "local", "steepest descent", "not BFGS", "no intramolecular", "smina", "qvina"):
        assert word in V.VINA_MIN_COVERAGE, word
    rec = V.MolVinaMin(np.asarray([0, 0, 0, 0, 0, -4, -2, 0], np.float32), np.asarray([2, 0, 1, 0], np.int32), np.zeros((2, 5), np.float32),
                       np.asarray([17, 17], np.int32), 0, np.zeros((2, 3), np.float32), np.asarray([0, 0, 0, 0, 0, 0, 0, 0.5], np.float32),
                       np.ones((2, 3), np.float32), np.asarray([0, 0, 0, 1, 0, 0, 0, 1], np.float32), np.asarray([-3, -4, 0.125, 0.5], np.float32),
                       np.asarray([1, 40, 12, 0], np.int32), 0.75)
    assert (rec.status, rec.evals, rec.accepted, rec.inter_start, rec.score_start, rec.score) == (1, 40, 12, -3.0, -1.5, -2.0)
    d = rec.as_dict()
    assert set(V.MIN_CSV_COLUMNS) <= set(d) and V.MIN_CSV_COLUMNS[:len(V.CSV_COLUMNS)] == V.CSV_COLUMNS
    assert V.MIN_CSV_COLUMNS[len(V.CSV_COLUMNS):] == ("inter_start", "score_start", "status", "evals", "rmsd") and d["rmsd"] == 0.75
    out = tmp_path / "m.csv"
    V.write_csv(str(out), [("a.sdf", 3, rec)], V.MIN_CSV_COLUMNS)
    lines = out.read_text().splitlines()
    assert lines[0].split(",") == ["source", "index"] + list(V.MIN_CSV_COLUMNS) and lines[1].endswith(",-3.0,-1.5,1,40,0.75")
    from diffsbdd_amd.generate import LigandGenerator
    assert LigandGenerator._vina_options(True) == {} and LigandGenerator._vina_options({"minimize": False}) == {}
    assert LigandGenerator._vina_options({"minimize": True}) == {"minimize": {}}
    assert LigandGenerator._vina_options({"minimize": {"max_evals": 50}, "residues": [1]}) == {"minimize": {"max_evals": 50}, "residues": [1]}
    with pytest.raises(ValueError, match="minimize"):
        LigandGenerator._vina_options({"minimize": {"steps": 3}})
