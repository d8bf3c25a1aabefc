"""CPU: the torsion tree, the intramolecular term and the flexible minimiser as diffsbdd_amd/vina.py restates them
(`torsion_tree`, `_vina_torsions_host`, `_vina_intra_host`, `torsion_coordinates`, `flex_geometry`, `flex_step`,
`_vina_flex_host`): the tree on hand-built graphs and the crystal fixture, the invariants of the coordinates, the projected
gradient against central finite differences of an independently written energy, and the one-torsion known answer."""
import itertools

import numpy as np
import pytest

from diffsbdd_amd import _lib, vina as V
from tests import _vina_cases as C
from tests import _vina_flex_cases as F


def _sides(rotors):
    return [np.nonzero(r[2])[0].tolist() for r in rotors]


# ---- the tree -----------------------------------------------------------------------------------------------------------------
def test_tree_of_hand_built_graphs():
    rotors, found, pairs = F.tree_of(*F.GRAPHS["chain4"])
    assert found == 1 and [(r[0], r[1]) for r in rotors] == [(1, 2)] and _sides(rotors) == [[2, 3]]      # the tie: the side of atom 2
    assert not pairs.any()                                                  # 0 and 3 are exactly 3 bonds apart
    rotors, found, pairs = F.tree_of(*F.GRAPHS["chain5"])
    assert found == 2 and [(r[0], r[1]) for r in rotors] == [(2, 1), (2, 3)] and _sides(rotors) == [[0, 1], [3, 4]]
    assert np.argwhere(pairs).tolist() == [[0, 4], [4, 0]]
    rotors, found, pairs = F.tree_of(*F.GRAPHS["benzene"])
    assert found == 0 and rotors == [] and not pairs.any()
    rotors, found, pairs = F.tree_of(*F.GRAPHS["biphenyl"])
    assert found == 1 and (rotors[0][0], rotors[0][1]) == (0, 6) and _sides(rotors) == [list(range(6, 12))]      # 6 against 6: atom 6's
    assert not pairs[1, 7] and not pairs[0, 8]                              # 1-0-6-7 and 0-6-7-8: 3 bonds
    # of the 36 pairs across the bond 1 is bonded, 4 are 2 bonds apart (0-7, 0-11, 6-1, 6-5) and 8 are 3 bonds apart
    assert pairs[2, 8] and pairs[3, 9] and not pairs[2, 3] and pairs.sum() == 2 * (36 - 1 - 4 - 8)
    rotors, found, pairs = F.tree_of(*F.GRAPHS["tailed_ring"])
    assert found == 2 and [(r[0], r[1]) for r in rotors] == [(0, 6), (6, 7)] and _sides(rotors) == [[6, 7, 8], [7, 8]]
    assert pairs[8, 3] and pairs[8, 2] and not pairs[8, 0] and not pairs[6, 2] and pairs[6, 3]      # 6-0-1-2: 3 bonds; 6 to 3: 4
    rotors, found, pairs = F.tree_of(*F.GRAPHS["fragments"])
    assert found == 3 and _sides(rotors) == [[2, 3], [4, 5], [7, 8]]
    assert pairs[2, 5] and pairs[3, 8] and not pairs[0, 1] and pairs[0, 4] and not pairs[0, 6]      # unconnected pairs count once a rotor parts them
    rotors, found, pairs = F.tree_of(*F.GRAPHS["chain40"])
    assert found == 37 and len(rotors) == 32 and [(r[0], r[1]) for r in rotors[:2]] == [(2, 1), (3, 2)]
    # rotor k is the bond (k + 2, k + 1); the tie at the middle bond (20, 19) goes to the side of atom 20
    assert _sides(rotors)[17] == list(range(0, 19)) and _sides(rotors)[18] == list(range(20, 40)) and _sides(rotors)[19] == list(range(21, 40))
    assert not pairs[36:, 36:].any() and pairs[39, 30]                      # the rotors past the 32nd part nothing
    assert F.tree_of(*F.GRAPHS["chain5"], keep=0)[0] == [] and not F.tree_of(*F.GRAPHS["chain5"], keep=0)[2].any()


def test_sides_are_nested_or_disjoint_and_masks_symmetric():
    z = C.fixture()
    graphs = list(F.GRAPHS.values()) + [C.fixture_ligand(z, str(n)) for n in z["names"]] + [C.chain(128)]
    for el, bonds in graphs:
        rotors, found, pairs = F.tree_of(el, bonds)
        assert np.array_equal(pairs, pairs.T) and not pairs.diagonal().any()
        for a, b in itertools.combinations(rotors, 2):
            both = a[2] & b[2]
            assert not both.any() or np.array_equal(both, a[2]) or np.array_equal(both, b[2])
        for p, m, side in rotors:
            assert side[m] and not side[p] and 2 * side.sum() <= len(el)
        if not rotors:
            assert not pairs.any()


def test_rotors_found_equal_the_typing_count_on_the_fixture_and_the_ragged_batch():
    z = C.fixture()
    sizes = {}
    for name in z["names"]:
        el, bonds = C.fixture_ligand(z, str(name))
        rotors, found, _ = F.tree_of(el, bonds)
        assert found == int(z[f"{name}_n_rot"]) == C.type_host(el, bonds)[1]
        sizes[str(name)] = (len(el), found)
    assert sizes["5ndu"][0] == 49 and sizes["3rfm"][1] == 0
    for b in (C.type_batch(), F.torsion_batch()):
        tree = V._vina_torsions_host(*(b[k] for k in C.TYPE_KEYS), fill=-7)
        _, mol_int = V._vina_type_host(*(b[k] for k in C.TYPE_KEYS))
        assert np.array_equal(tree.found, mol_int[:, V.I_ROT])
        assert ((tree.kept == np.minimum(tree.found, 32)) | (np.diff(b.get("true_off", b["mol_off"])) > 128)).all()
    tb = F.torsion_batch()
    tree = V._vina_torsions_host(*(tb[k] for k in C.TYPE_KEYS))
    assert tree.ints[:, :2].tolist() == [[1, 1], [2, 2], [0, 0], [1, 1], [2, 2], [3, 3], [32, 37], [32, 125], [0, 125], [0, 0]]
    off = tb["mol_off"]
    assert not tree.pair_mask[off[8]:off[9]].any() and (tree.ends[8] == -1).all()      # longer than n_max: rigid
    assert (tree.ends[6, :32] >= 0).all() and (tree.ends[0, 1:] == -1).all() and not tree.sides[0, 1:].any()
    # masks round-trip
    bits = np.random.RandomState(0).rand(5, 77) < 0.5
    assert np.array_equal(V.unpack_masks(V.pack_masks(bits), 77), bits) and V.pack_masks(bits).dtype == np.int32


# ---- the intramolecular term --------------------------------------------------------------------------------------------------
def test_intra_restatement_on_the_batch():
    b = F.flex_batch()
    st, margin, atom_bound, mol_bound, grad_bound = V._vina_intra_host(b["lig_x"], b["lig_code"], b["mol_off"], b["tree"].pair_mask,
                                                                       eps=V.EPS32)
    off = b["mol_off"]
    rows = lambda m: slice(off[m], off[m + 1])
    assert margin > C.MARGIN
    assert st.flag.tolist() == [int(m == b["nan_mol"]) for m in range(len(off) - 1)]
    for m in (b["rigid"], b["empty_mol"], b["empty_group"], b["untyped_mol"]):      # no rotor / no atoms / no pair beyond 3 bonds / untyped
        assert not st.mol[m].any() and not st.atom[rows(m)].any() and not st.grad[rows(m)].any(), m
    assert np.isnan(st.mol[b["nan_mol"]]).all() and np.isnan(st.grad[rows(b["nan_mol"])]).all()
    assert st.mol[b["folded"], 2] > 0 and st.mol[b["crystal"], 0] > 0              # true clashes in the folded chain
    live = [m for m in range(len(off) - 1) if m != b["nan_mol"]]
    for m in live:                                                          # every pair once; internal forces cancel
        assert st.mol[m, :5] == pytest.approx(st.atom[rows(m)].sum(0) / 2, rel=1e-12, abs=1e-300)
        assert np.abs(st.grad[rows(m)].sum(0)).max() <= 1e-12
        assert st.mol[m, 5] == pytest.approx(float((np.asarray(V.WEIGHTS) * st.mol[m, :5]).sum()), rel=1e-12, abs=1e-300)
    untyped = off[b["untyped_atom"]] + 2
    assert not st.atom[untyped].any() and st.atom[untyped + 3].any()
    assert np.isfinite(mol_bound[live]).all() and (mol_bound[live] >= 0).all()
    assert atom_bound.shape == (off[-1], 5) and grad_bound.shape == (off[-1], 3) and mol_bound.shape == (len(off) - 1, 6)


# ---- coordinates ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain40", "tailed_ring", "5ndu"])
def test_coordinates_keep_every_rigid_distance(name):
    rng = np.random.RandomState(3)
    if name == "5ndu":
        z = C.fixture()
        el, bonds = C.fixture_ligand(z, "5ndu")
        x0 = z["5ndu_crystal_x"].astype(np.float32)
    else:
        el, bonds = F.GRAPHS[name]
        x0 = (rng.normal(size=(len(el), 3)) * 3.0 + [20.0, -35.0, 50.0]).astype(np.float32)      # any points: only rigidity is tested
    rotors, _, _ = F.tree_of(el, bonds)
    theta = rng.uniform(-np.pi, np.pi, len(rotors))
    x = V.torsion_coordinates(x0, rotors, theta)
    keep = F.distance_pairs(el, bonds, rotors)
    tol = F.distance_tolerance(x0, x, len(rotors))
    assert keep.any() and np.abs(F.distances(x) - F.distances(x0))[keep].max() <= tol
    assert np.abs(x.astype(np.float64) - x0).max() > 0.1                    # and the pose did change
    # any list order gives the same geometry
    order = rng.permutation(len(rotors))
    xp = V.torsion_coordinates(x0, [rotors[k] for k in order], theta[order])
    assert np.abs(xp.astype(np.float64) - x.astype(np.float64)).max() <= tol
    # theta = 0: the input's bits, through a frame as well
    same = V.torsion_coordinates(x0, rotors, np.zeros(len(rotors)))
    assert np.array_equal(same.view(np.int32), x0.view(np.int32))
    q = np.asarray([0.8, 0.36, -0.48, 0.0])                                 # a unit quaternion
    framed = V.torsion_coordinates(x0, rotors, theta, [1.0, 2.0, 3.0], q).astype(np.float64)
    assert np.abs(framed - (V._torsion_frame(x0, rotors, theta) @ V.pose_frame(q).T + [1.0, 2.0, 3.0])).max() <= tol
    assert np.abs(F.distances(framed) - F.distances(x0))[keep].max() <= F.distance_tolerance(x0, framed, len(rotors))


# ---- the projected gradient -----------------------------------------------------------------------------------------------------
def _rotation(w):
    angle = float(np.linalg.norm(w))
    if angle == 0.0:
        return np.eye(3)
    k = np.asarray(w) / angle
    K = np.asarray([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _energy64(x, code, q, qcode, pairs):
    """inter + intra in float64 by its own loops over pairs (the cutoff on the float64 distance: the case keeps every pair
    0.3 A away from it)."""
    radius = {1: 1.9, 2: 1.8, 3: 1.7}

    def term(r, ci, cj):
        if r >= V.CUTOFF:
            return 0.0
        d = r - radius[ci & 15] - radius[cj & 15]
        e = V.WEIGHTS[0] * np.exp(-(d / 0.5) ** 2) + V.WEIGHTS[1] * np.exp(-((d - 3.0) / 2.0) ** 2)
        return e + (V.WEIGHTS[2] * d * d if d < 0 else 0.0)
    total = 0.0
    for i in range(len(x)):
        for j in range(len(q)):
            total += term(float(np.linalg.norm(x[i] - q[j])), int(code[i]), int(qcode[j]))
        for j in range(i + 1, len(x)):
            if pairs[i, j]:
                total += term(float(np.linalg.norm(x[i] - x[j])), int(code[i]), int(code[j]))
    return total


def test_force_moment_and_torques_against_finite_differences():
    """A folded heptane of class-only codes (no hydrophobic or hbond term: no kink but the repulsion's, which is C1) among
    six pocket atoms, every pair inside the cutoff: F, M and tau of the restatement are the derivatives of an independently
    written float64 energy in the translation, the rotation vector about the centroid and the torsion angles."""
    el, bonds = C.chain(7)
    rotors, _, pairs = F.tree_of(el, bonds)
    x0 = F.chain_coordinates(np.deg2rad([62.0, -58.0, 55.0, 64.0])).astype(np.float32)
    for seed in range(100):                                                 # the first seeded pocket with no pair near the cutoff
        q = F._pocket_around(x0.astype(np.float64), np.random.RandomState(seed), 6, lo=3.3, hi=4.2)
        if np.abs(F.distances(np.concatenate([x0, q])) - V.CUTOFF).min() > 0.3:
            break
    code, qcode = np.asarray([1, 1, 2, 1, 3, 1, 1], np.int32), np.asarray([1, 2, 3, 1, 1, 2], np.int32)
    assert len(rotors) == 4 and pairs.sum() > 0
    assert np.abs(F.distances(np.concatenate([x0, q])) - V.CUTOFF).min() > 0.3      # no pair crosses the cutoff under a nudge
    masks = V.pack_masks(pairs)
    args = (x0, code, [0, 7], [0], np.zeros((1, 4), np.int32), q, qcode, [0, 6])
    g = V._vina_grad_host(*args)
    gi, _ = V._vina_intra_host(x0, code, [0, 7], masks)
    assert gi.mol[0, 5] != 0.0
    c, rho2, rho_max, tau, _, _ = V.flex_geometry(x0, rotors, g.grad + gi.grad)
    x64 = x0.astype(np.float64)

    def energy(shift, w, theta):
        y = V._torsion_frame(x0, rotors, theta)
        cy = y.mean(0)
        return _energy64(cy + (y - cy) @ _rotation(w).T + shift, code, q.astype(np.float64), qcode, pairs)
    assert energy(np.zeros(3), np.zeros(3), np.zeros(4)) == pytest.approx(float(g.mol[0, 5] + gi.mol[0, 5]), rel=1e-12)
    assert np.abs(c - x64.mean(0)).max() < 1e-12
    h = 1e-5

    def slope(k, block):
        lo, hi = [np.zeros(3), np.zeros(3), np.zeros(4)], [np.zeros(3), np.zeros(3), np.zeros(4)]
        lo[block][k], hi[block][k] = -h, h
        return (energy(*hi) - energy(*lo)) / (2 * h)
    fd_F = np.asarray([slope(k, 0) for k in range(3)])
    fd_M = np.asarray([slope(k, 1) for k in range(3)])
    fd_tau = np.asarray([slope(k, 2) for k in range(4)])
    scale = max(np.abs(fd_F).max(), np.abs(fd_M).max(), np.abs(fd_tau).max())
    assert scale > 1e-3
    # central differences of a smooth function: h^2 |E'''| / 6 ~ 1e-10 |E'''|, and 1e-16 |E| / h ~ 1e-11 of rounding
    assert np.abs(fd_F - g.mol_grad[0, V.G_NET]).max() < 1e-7 * max(scale, 1.0)
    assert np.abs(fd_M - g.mol_grad[0, V.G_MOMENT]).max() < 1e-7 * max(scale, 1.0)
    assert np.abs(fd_tau - tau).max() < 1e-7 * max(scale, 1.0)
    assert np.abs(tau).min() > 0


# ---- the iteration --------------------------------------------------------------------------------------------------------------
def test_flex_step_moves_no_atom_further_than_the_step():
    b = F.flex_batch()
    for m in (b["shifted"], b["folded"], b["decane"]):
        one, _ = F.sub_batch(b, [m])
        x0 = one["lig_x"]
        rotors = V.valid_torsions(one["tree"], 0, len(x0))
        g = V._vina_grad_host(*(one[k] for k in C.SCORE_KEYS))
        gi, _ = V._vina_intra_host(x0, one["lig_code"], one["mol_off"], one["tree"].pair_mask)
        Fn, M = g.mol_grad[0, V.G_NET], g.mol_grad[0, V.G_MOMENT]
        c, rho2, rho_max, tau, reach, rho2k = V.flex_geometry(x0, rotors, g.grad + gi.grad)
        for dofs in (1, 2, 3):
            kept = rotors if dofs & 2 else []
            u = V.flex_slope(Fn, M, rho2, rho_max, tau[:len(kept)], reach, rho2k, dofs)
            for L in (0.25, 1.0):
                t, q, theta = V.flex_step(np.zeros(3), [1.0, 0, 0, 0], np.zeros(len(kept)), Fn, M, tau[:len(kept)], c, rho2,
                                          rho2k[:len(kept)], L / u, dofs)
                x = V.torsion_coordinates(x0, kept, theta, t, q)
                moved = np.sqrt(((x.astype(np.float64) - x0) ** 2).sum(1))
                assert 0.2 * L < moved.max() <= L + 2 * np.sqrt(3.0) * V.EPS32 * np.abs(x0).max(), (m, dofs, L, moved.max())
                if dofs == 1:
                    assert np.allclose(theta, 0)
                if dofs == 2:
                    outside = ~np.any([r[2] for r in rotors], axis=0)
                    assert np.array_equal(x[outside].view(np.int32), x0[outside].view(np.int32))


@pytest.mark.parametrize("start, well", [(90.0, 1), (30.0, 0)])
def test_one_torsion_case_converges_to_the_well_downhill(start, well):
    wells = F.one_torsion_wells()
    assert wells[0] == pytest.approx(13.023, abs=2e-3) and wells[1] == pytest.approx(106.977, abs=2e-3)
    pair_at_well = V.WEIGHTS[0] * np.exp(-(F.WELL / 0.5) ** 2) + V.WEIGHTS[1] * np.exp(-((F.WELL - 3) / 2) ** 2)
    assert pair_at_well == pytest.approx(-0.036124, abs=2e-6)
    barrier = F.one_torsion_energy(np.deg2rad(60.0)) - F.one_torsion_energy(np.deg2rad(wells[0]))
    assert barrier == pytest.approx(0.29 + 0.036, abs=0.02)
    b = F.one_torsion(start)
    out = V._vina_flex_host(*(b[k] for k in C.SCORE_KEYS), F.one_torsion_tree(), dofs=2)
    assert V.STATUS[out.stat[0, V.S_STATUS]] == "converged" and out.stat[0, V.S_ACCEPTED] > 3
    assert np.array_equal(out.x[:3].view(np.int32), b["lig_x"][:3].view(np.int32))      # dofs = 2: only C3 is in the side
    arc = np.deg2rad(abs(F.dihedral_deg(out.x) - wells[well])) * F.RADIUS
    assert arc <= 2 * V.MIN_TOL, (F.dihedral_deg(out.x), wells[well])
    assert out.intra_out.mol[0, 5] == 0.0 and out.energies[0, V.X_E_FINAL] < out.energies[0, V.X_E_START]
    assert out.theta[0, 0] == pytest.approx(np.deg2rad(F.dihedral_deg(out.x) - start), abs=1e-5) and not out.theta[0, 1:].any()


def test_flex_restatement_on_edge_rows_and_the_abi():
    b = F.flex_batch()
    edge = [b["rigid"], b["empty_mol"], b["empty_group"], b["bad_group"], b["untyped_mol"], b["nan_mol"], b["folded"]]
    one, rows = F.sub_batch(b, edge)
    out = V._vina_flex_host(*(one[k] for k in C.SCORE_KEYS), one["tree"], max_evals=F.MAX_EVALS)
    status = [V.STATUS[s] for s in out.stat[:, V.S_STATUS]]
    assert status[1:6] == ["no gradient"] * 4 + ["nonfinite"] and status[0] in ("budget", "converged") and status[6] == "budget"
    assert out.stat[1:5, V.S_EVALS].tolist() == [1] * 4 and out.stat[5].tolist() == [3, 0, 0, 0]
    assert not out.theta[:5].any() and np.isnan(out.theta[5]).all() and np.isnan(out.energies[5]).all()
    assert np.abs(out.theta[6, :4]).max() > 1e-3 and out.energies[6, V.X_E_FINAL] < out.energies[6, V.X_E_START]
    assert F.MAX_EVALS <= out.stat[6, V.S_EVALS] <= F.MAX_EVALS + 1
    # without the keyword nothing of the rigid restatement moved: the same function, the same defaults
    rigid = V._vina_minimize_host(*(one[k] for k in C.SCORE_KEYS), max_evals=F.MAX_EVALS)
    assert rigid.energies.shape[1] == 4 and out.energies.shape[1] == 8
    # the three entries are declared, bound and exported; the ABI version stands
    lib = _lib.load()
    for name in ("dsbdd_vina_torsions", "dsbdd_vina_intra", "dsbdd_vina_flex"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.dsbdd_abi_version() == 6
    for text in (V.VINA_FLEX_COVERAGE, V.VINA_INTRA_COVERAGE):
        assert "NOT" in text and "smina" in text
    with pytest.raises(ValueError, match="dofs"):
        V._vina_flex_host(*(one[k] for k in C.SCORE_KEYS), one["tree"], dofs=0)
