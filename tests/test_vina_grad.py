"""Host logic of the Vina-type gradient (diffsbdd_amd/vina.py): the float64 restatement `_vina_grad_host` of
dsbdd_vina_score_grad against central finite differences of an energy written on its own, at hand values, at the
conventions of the non-smooth points, its net force and moment, the derived error bound against a plain float32 evaluation,
and the C entry's argument checks.  No GPU."""
import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib, vina as V
from tests import _vina_cases as C
from tests import _vina_grad_cases as GC

W = np.asarray(V.WEIGHTS, np.float64)


def _slope(d, hyd, hb):
    """sum_k w_k T_k'(d), written out from the formulas of the header."""
    c = (d - 3.0) / 2.0
    s = W[0] * (-8.0 * d * np.exp(-4.0 * d * d)) + W[1] * (-c * np.exp(-c * c))
    s += W[2] * (2.0 * d if d < 0 else 0.0)
    s += W[3] * (-1.0 if hyd and 0.5 < d < 1.5 else 0.0)
    s += W[4] * (-1.0 / 0.7 if hb and -0.7 < d < 0 else 0.0)
    return s


def _one(lig_x, lig_code, poc_x, poc_code, n_rot=0, **kw):
    """The restatement on one molecule and one group."""
    n, m = len(lig_code), len(poc_code)
    return V._vina_grad_host(np.asarray(lig_x, np.float32).reshape(n, 3), lig_code, [0, n], [0], [[n, 0, n_rot, 0]],
                             np.asarray(poc_x, np.float32).reshape(m, 3), poc_code, [0, m], **kw)


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_against_finite_differences():
    """Central differences (h = 1e-4 A) of `_vina_grad_cases.frozen_energy` against `_vina_grad_host` on score_batch(0): every
    atom of the molecules of at most 65 atoms, 40 seeded atoms of the 300-atom one.  Tolerance per atom and component:
    h^2 / 6 times the bound of the third derivative along the axis (`third_derivative_bound`) + the rounding of the two
    energies, (n + 8) 2^-53 sum |weighted terms| / h (n terms summed, a few roundings each), + the same for the analytic
    sum.  Recorded: 12 209 counted pairs, the nearest kink 6.2e-4 A away, no pair at r = 0; largest |difference| / tolerance
    0.35."""
    b = C.score_batch(0)
    st = GC.grad_reference(0, appended=False)[0]
    h, eps64 = GC.H, 2.0 ** -53
    rng = np.random.RandomState(11)
    n_pairs, nearest, worst, checked = 0, np.inf, 0.0, 0
    for m in range(len(b["mol_off"]) - 1):
        lo, hi = int(b["mol_off"][m]), int(b["mol_off"][m + 1])
        if st.flag[m] or hi == lo:
            continue
        x, q, ri, rj, counted, hyd, hb, r32 = GC.molecule_pairs(b, m)
        assert not (counted & (r32 == 0)).any()
        x64, q64 = x.astype(np.float64), q.astype(np.float64)
        e0, size, d = GC.frozen_energy(x64, q64, ri, rj, counted, hyd, hb)
        n_pairs += int(counted.sum())
        nearest = min(nearest, GC.kink_distance(d, counted, hyd, hb))
        atoms = np.arange(hi - lo) if hi - lo <= 65 else np.sort(rng.choice(hi - lo, 40, replace=False))
        r = d + ri[:, None] + rj[None, :]
        third = GC.third_derivative_bound(r, d, counted, hyd, hb)
        n_i = counted.sum(1)
        slope_size = np.abs(np.where(counted[..., None], V.pair_slopes(d, hyd, hb) * W, 0.0)).sum((1, 2))
        tol = h * h / 6 * third + (n_i + 8) * eps64 * size / h + (n_i + 8) * eps64 * slope_size
        for k in range(3):
            step = np.zeros(3)
            step[k] = h
            up = GC.frozen_energy(x64[atoms] + step, q64, ri[atoms], rj, counted[atoms], hyd[atoms], hb[atoms])[0]
            dn = GC.frozen_energy(x64[atoms] - step, q64, ri[atoms], rj, counted[atoms], hyd[atoms], hb[atoms])[0]
            diff = np.abs((up - dn) / (2 * h) - st.grad[lo:hi][atoms, k])
            live = tol[atoms] > 0
            assert np.all(diff <= tol[atoms]), (m, k, float((diff - tol[atoms]).max()))
            if live.any():
                worst = max(worst, float((diff[live] / tol[atoms][live]).max()))
            checked += len(atoms)
    print(f"counted pairs {n_pairs}, nearest kink {nearest:.3e} A, atoms x components {checked}, largest diff / tol {worst:.3f}")
    assert n_pairs == 12209 and nearest >= 2 * h and checked > 3 * 300       # the precondition: no kink inside a step
    assert np.nanmax(np.abs(st.grad)) > 0.1 and worst > 1e-3                     # neither side is trivially zero


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_gradient_at_hand_values():
    for d in (-0.5, 0.25, 1.0, 2.0):
        for hyd in (False, True):
            for hb in (False, True):
                ci, cj = V.C_C | 16 * hyd | V.DONOR * hb, V.C_C | 16 * hyd | V.ACCEPTOR * hb
                for side in (1.0, -1.0):
                    r = float(np.float32(d + 3.8))
                    st = _one([[0, 0, 0]], [ci], [[side * r, 0, 0]], [cj])
                    want = _slope(r - 1.9 - 1.9, hyd, hb) * -side                  # u = (x_i - x_j) / r = -side on the x axis
                    assert st.grad[0, 0] == pytest.approx(want, rel=1e-12, abs=1e-15), (d, hyd, hb, side)
                    assert st.grad[0, 1] == 0 and st.grad[0, 2] == 0
    # the signs: inside the repulsive wall the atom is pushed away from the pocket atom, in the attractive well pulled to it
    assert _one([[0, 0, 0]], [17], [[3.3, 0, 0]], [17]).grad[0, 0] > 0 > _one([[0, 0, 0]], [17], [[-3.3, 0, 0]], [17]).grad[0, 0]
    assert _one([[0, 0, 0]], [17], [[4.8, 0, 0]], [17]).grad[0, 0] < 0
    # off the axis the row is the slope times the unit vector; N_rot only enters the factor
    st = _one([[1, 2, 3]], [17], [[3, 5, 9]], [17], n_rot=4)
    u = np.asarray([-2.0, -3.0, -6.0]) / 7.0
    assert np.allclose(st.grad[0], _slope(7.0 - 3.8, True, False) * u, rtol=1e-12, atol=0)
    assert st.rot_factor[0] == 1.0 / (1.0 + 4 * V.ROT_WEIGHT) and st.max_norm[0] == pytest.approx(abs(_slope(3.2, True, False)), rel=1e-12)
    assert np.allclose(st.score_grad, st.grad / (1.0 + 4 * V.ROT_WEIGHT), rtol=1e-15)


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_conventions_at_the_points_without_a_derivative():
    # an atom exactly on a pocket atom: its terms as ever, nothing from that pair in the gradient
    poc = [[1, 2, 3], [4.5, 2, 3]]
    both, far = _one([[1, 2, 3]], [17], poc, [17, 17]), _one([[1, 2, 3]], [17], poc[1:], [17])
    score_both, _ = V._vina_score_host(np.asarray([[1, 2, 3]], np.float32), [17], [0, 1], [0], [[1, 0, 0, 0]],
                                       np.asarray(poc, np.float32), [17, 17], [0, 2])
    assert np.array_equal(both.atom, score_both.atom) and both.atom[0, 2] == pytest.approx(3.8 ** 2 + 0.09, rel=1e-6)
    assert np.array_equal(both.grad, far.grad) and both.grad[0, 0] != 0
    assert not _one([[1, 2, 3]], [17], poc[:1], [17]).grad.any()
    # the batch: untyped atoms, an empty group, a group id out of range, a molecule that is not finite, the coincident atom
    b = GC.grad_batch()
    st, grad_bound, mol_bound = GC.grad_reference()
    off = b["mol_off"]
    rows = lambda m: slice(off[m], off[m + 1])
    for m in (0, b["empty_mol"], b["untyped_mol"], 10):
        assert not st.grad[rows(m)].any() and not st.mol_grad[m, :7].any(), m
        assert st.mol_grad[m, 7] == 1.0 / (1.0 + V.ROT_WEIGHT * b["mol_int"][m, 2])
    untyped = ((b["lig_code"] & 15) == 0) | ((b["lig_code"] & 15) > 10)       # class 0 and the classes outside the list
    live_rows = np.ones(len(untyped), bool)
    live_rows[rows(b["nan_mol"])] = False
    assert untyped.sum() > 20 and not st.grad[untyped & live_rows].any()
    assert st.flag[b["nan_mol"]] == 1 and np.isnan(st.grad[rows(b["nan_mol"])]).all() and np.isnan(st.mol_grad[b["nan_mol"]]).all()
    assert np.isnan(grad_bound[rows(b["nan_mol"])]).all() and not np.isnan(st.grad[live_rows]).any()
    m, a, on = b["coincident"]
    x, q, ri, rj, counted, hyd, hb, r32 = GC.molecule_pairs(b, m)
    assert r32[a, on] == 0 and counted[a, on] and np.isfinite(st.grad[rows(m)]).all() and st.grad[rows(m)][a].any()
    assert st.atom[rows(m)][a, 2] >= 3.8 ** 2 * (1 - 1e-6)                  # the pair's repulsion is in the terms
    # d exactly at a kink, from representable coordinates: F / F pairs (radii 1.5 + 1.5) at r = 3.5, 4.5 and 3.0
    F, eps = V.C_F | V.HYDROPHOBIC, 2.0 ** -20
    smooth = lambda d: W[0] * (-8 * d * np.exp(-4 * d * d)) + W[1] * (-(d - 3) / 2 * np.exp(-((d - 3) / 2) ** 2))
    g = lambda r, ci=F, cj=F: -_one([[0, 0, 0]], [ci], [[r, 0, 0]], [cj]).grad[0, 0]          # = the slope (u = -1)
    assert g(3.5) == pytest.approx(smooth(0.5), rel=1e-12)                    # d = 0.5: the branch `1`, slope 0
    assert g(3.5 + eps) == pytest.approx(smooth(0.5 + eps) - W[3], rel=1e-9)  # just above: the ramp, -1
    assert g(4.5 - eps) == pytest.approx(smooth(1.5 - eps) - W[3], rel=1e-9)
    assert g(4.5) == pytest.approx(smooth(1.5), rel=1e-12)                    # d = 1.5: the branch `0`
    don, acc = V.C_F | V.DONOR, V.C_F | V.ACCEPTOR
    assert g(3.0, don, acc) == pytest.approx(smooth(0.0), rel=1e-12)          # d = 0: hbond' = 0 and repulsion' = 0
    assert g(3.0 - eps, don, acc) == pytest.approx(smooth(-eps) - W[4] / 0.7 + W[2] * 2 * -eps, rel=1e-9)
    # no float32 r gives d = -0.7 exactly (-0.7 + 3 is not a float32): the rule at the point itself on the function, the two
    # sides of it through the restatement
    assert V.pair_slopes(np.asarray([-0.7, 0.5, 1.5, 0.0]))[:, 2:].tolist() == [[2 * -0.7, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    lo, hi = float(np.float32(2.3)) - 4 * eps, float(np.float32(2.3)) + 4 * eps
    assert g(lo, don, acc) == pytest.approx(smooth(lo - 3) + W[2] * 2 * (lo - 3), rel=1e-9)
    assert g(hi, don, acc) == pytest.approx(smooth(hi - 3) + W[2] * 2 * (hi - 3) - W[4] / 0.7, rel=1e-9)
    low = V.VINA_GRAD_COVERAGE.lower()
    for word in ("inter", "ligand heavy atoms only", "rigid protein", "typing", "constants", "8 a cutoff", "kinks", "smina", "minimiser"):
        assert word in low, word


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_net_moment_and_translation():
    b = GC.grad_batch()
    st = GC.grad_reference()[0]
    off = b["mol_off"]
    seen = 0
    for m in range(len(off) - 1):
        if st.flag[m] or off[m + 1] == off[m]:
            continue
        x, g = b["lig_x"][off[m]:off[m + 1]].astype(np.float64), st.grad[off[m]:off[m + 1]]
        net, moment = g.sum(0), np.cross(x - x.mean(0), g).sum(0)
        scale = np.abs(g).sum(0).max() * max(np.abs(x - x.mean(0)).max(), 1.0)
        assert np.all(np.abs(st.net[m] - net) <= 1e-12 * np.abs(g).sum(0)), m
        assert np.all(np.abs(st.moment[m] - moment) <= 1e-12 * scale), m
        assert st.max_norm[m] == pytest.approx(np.sqrt((g * g).sum(1)).max(), rel=1e-12)
        seen += bool(g.any())
    assert seen >= 10
    # every coordinate of a group translated by an offset that is exact in float32: the gradient does not move
    rng = np.random.RandomState(3)
    lig, poc = rng.randint(0, 16 * 1024, (10, 3)) / 1024.0, rng.randint(0, 16 * 1024, (40, 3)) / 1024.0
    ci, cj = rng.choice(C._CODES[:16], 10), rng.choice(C._CODES[:16], 40)
    shift = np.asarray([8.0, -4.0, 16.0])
    assert np.array_equal((lig + shift).astype(np.float32).astype(np.float64) - shift, lig)
    here, there = _one(lig, ci, poc, cj, n_rot=2), _one(lig + shift, ci, poc + shift, cj, n_rot=2)
    assert np.abs(here.grad).max() > 0.01
    assert np.all(np.abs(here.grad - there.grad) <= 1e-12 * np.abs(here.grad).max())
    assert np.all(np.abs(here.mol_grad - there.mol_grad) <= 1e-12 * np.abs(here.mol_grad).max() * 32)


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_grad_error_bound_holds_plain_float32_and_scales_with_eps():
    """Recorded: the restatement evaluated in float32 (numpy) uses at most 0.087 of the bound per atom and 0.082 per molecule
    (0.21 on the rotor factor) on this batch; the kernel's own fractions are in profiles/vina_grad_error.md."""
    b = C.score_batch()
    st, grad_bound, mol_bound = GC.grad_reference(0, appended=False)
    assert st.kink_margin > GC.KINK_MARGIN                                   # no jump term is switched on
    live = st.flag == 0
    assert live.sum() == 15 and np.isnan(mol_bound[b["nan_mol"]]).all()
    assert (mol_bound[live] >= 0).all() and (mol_bound[live, 7] > 0).all() and (mol_bound[b["empty_mol"], :7] == 0).all()
    gb2, mb2 = V.grad_error_bound(*(b[k] for k in C.SCORE_KEYS), eps=2 * V.EPS32)
    ok = np.isfinite(gb2)
    assert np.allclose(gb2[ok], 2 * grad_bound[ok], rtol=1e-5) and np.allclose(mb2[live], 2 * mol_bound[live], rtol=1e-5)
    st32 = V._vina_grad_host(*(b[k] for k in C.SCORE_KEYS), dtype=np.float32)
    assert st32.grad.dtype == np.float32 and st32.mol_grad.dtype == np.float32
    with np.errstate(invalid="ignore", divide="ignore"):
        fa = np.abs(st32.grad.astype(np.float64) - st.grad) / grad_bound
        fm = np.abs(st32.mol_grad.astype(np.float64) - st.mol_grad) / mol_bound
    print("float32 restatement / bound: atoms", np.nanmax(fa, 0), "molecules", np.nanmax(fm, 0))
    assert np.nanmax(fa) <= 1.0 and np.nanmax(fm) <= 1.0
    assert np.nanmax(fa) > 1e-3 and np.nanmax(fm[:, :7]) > 1e-3              # within three decades: not vacuous
    # a pair inside dd of a kink switches the jump on: two hydrophobic fluorines at d = 0.5 exactly
    one = dict(lig_x=np.zeros((1, 3), np.float32), lig_code=[V.C_F | 16], mol_off=[0, 1], mol_group=[0], mol_int=[[1, 0, 0, 0]],
               poc_x=np.asarray([[3.5, 0, 0]], np.float32), poc_code=[V.C_F | 16], group_off=[0, 1])
    gb, _ = V.grad_error_bound(*(one[k] for k in C.SCORE_KEYS))
    assert gb[0, 0] > abs(V.WEIGHTS[3]) and gb[0, 1] == 0


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_c_entry_refuses_bad_arguments_without_a_launch():
    lib = _lib.load()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    good = [None, p, p, p, 1, p, p, p, p, p, 1, p, p, p, p, p]
    assert len(_lib.SIGNATURES["dsbdd_vina_score_grad"][1]) == 16 and _lib.ABI_VERSION == 6 == lib.dsbdd_abi_version()
    assert lib.dsbdd_vina_score_grad(*(good[:4] + [0] + good[5:])) == _lib.OK                  # batch 0: nothing launched
    assert lib.dsbdd_vina_score_grad(*(good[:4] + [-1] + good[5:])) == _lib.ERR_ARG
    assert lib.dsbdd_vina_score_grad(*(good[:10] + [-1] + good[11:])) == _lib.ERR_ARG
    for k in (1, 2, 3, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15):
        args = list(good)
        args[k] = None
        assert lib.dsbdd_vina_score_grad(*args) == _lib.ERR_ARG and b"null" in lib.dsbdd_last_error(), k
    assert not buf.any()


def test_front_end_argument_handling(tmp_path):
    x, t, m = torch.zeros((2, 3)), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    pocket = V.TypedPocket(np.zeros((1, 3), np.float32), np.asarray([1], np.int32))
    with pytest.raises(_lib.HipLibraryError, match="vina_gradient"):
        V.vina_gradient(x, t, m, [pocket], "crossdock")
    with pytest.raises(_lib.HipLibraryError):
        V.vina_energy(x.requires_grad_(), t, m, [pocket], "crossdock")
    with pytest.raises(_lib.HipLibraryError, match="gradient_molecules"):
        V.gradient_molecules([(np.zeros((1, 3)), ["C"])], [pocket], device="cpu")
    a = V.parse_args(["--pdbfile", "p.pdb", "--sdf", "a.sdf", "--grad_out", "g.csv"])
    assert a.grad_out == "g.csv" and V.parse_args(["--pdbfile", "p.pdb", "--sdf", "a.sdf"]).grad_out is None
    rec = V.MolVinaGrad(np.zeros(8, np.float32), np.asarray([2, 0, 1, 0], np.int32), np.zeros((2, 5), np.float32),
                        np.asarray([17, 17], np.int32), 0, np.asarray([[3, 0, 4], [0, 0, 0]], np.float32),
                        np.asarray([3, 0, 4, 0, 0, 0, 5, 0.5], np.float32))
    assert rec.max_norm == 5.0 and rec.rot_factor == 0.5 and rec.score_grad[0].tolist() == [1.5, 0, 2] and rec.net.tolist() == [3, 0, 4]
    assert set(V.CSV_COLUMNS) <= set(rec.as_dict())
    out = tmp_path / "g.csv"
    V.write_grad_csv(str(out), [("a.sdf", 7, rec)])
    lines = out.read_text().splitlines()
    assert lines[0].split(",") == list(V.GRAD_CSV_COLUMNS) == ["source", "index", "atom", "gx", "gy", "gz", "norm"]
    assert lines[1] == "a.sdf,7,0,3.0,0.0,4.0,5.0" and lines[2] == "a.sdf,7,1,0.0,0.0,0.0,0.0" and len(lines) == 3
