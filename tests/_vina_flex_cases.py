"""Inputs shared by tests/test_vina_flex.py and tests/test_gpu_vina_flex.py: hand-built graphs with coordinates, the
one-torsion known answer, the typed batches of the torsion, intramolecular and flexible-minimiser kernels, and the tolerances
they are judged by.  References are computed once per process and must not be modified."""
import functools

import numpy as np

from diffsbdd_amd import vina as V
from tests import _vina_cases as C

BOND, ANGLE = 1.53, np.deg2rad(111.0)
MAX_EVALS = 24


# ---- graphs -------------------------------------------------------------------------------------------------------------------
def tailed_ring():
    """Cyclohexane with a 3-atom tail on atom 0: atoms 6, 7, 8."""
    return C.join(C.ring(6), C.chain(3), links=[(6, 0, 1)])


def fragments():
    """Butane and pentane side by side, not connected."""
    return C.join(C.chain(4), C.chain(5))


GRAPHS = {"chain4": C.chain(4), "chain5": C.chain(5), "benzene": C.benzene(), "biphenyl": C.GRAPHS["biphenyl"],
          "tailed_ring": tailed_ring(), "fragments": fragments(), "chain40": C.chain(40)}


def tree_of(elements, bonds, keep=V.MAX_TORSIONS):
    """`V.torsion_tree` of a hand-built graph."""
    n = len(elements)
    low = V.orders_from_bonds(n, bonds).astype(np.int64)
    return V.torsion_tree([V.class_of(e) for e in elements], low + low.T, keep)


def type_inputs(mols, n_max=C.N_MAX):
    """The typing kernel's inputs of a list of (elements, bonds) with the crossdock decoder."""
    sizes = [len(m[0]) for m in mols]
    order = np.zeros((len(mols), n_max, n_max), np.int8)
    for b, (el, bonds) in enumerate(mols):
        order[b] = V.orders_from_bonds(len(el), bonds, n_max)
    return {"order": order, "atom_type": np.asarray([C.DECODER.index(e) for m in mols for e in m[0]], np.int32),
            "mol_off": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), "class_elem": V.class_table(C.DECODER)}


def torsion_batch():
    """The graphs of the issue's table, a 128-atom chain, a 140-atom chain (longer than n_max) and an empty molecule."""
    return type_inputs(list(GRAPHS.values()) + [C.chain(128), C.chain(140), ([], [])])


# ---- coordinates ----------------------------------------------------------------------------------------------------------------
def chain_coordinates(dihedrals, bond=BOND, angle=ANGLE):
    """float32 [len(dihedrals) + 3, 3]: a chain with the given bond length and angle; atom k + 3 is placed at dihedral
    dihedrals[k] (rad) about the bond (k + 1, k + 2)."""
    x = [np.asarray([bond * np.cos(angle), bond * np.sin(angle), 0.0]), np.zeros(3), np.asarray([bond, 0.0, 0.0])]
    for phi in dihedrals:
        a, b, c = x[-3], x[-2], x[-1]
        bc = (c - b) / np.linalg.norm(c - b)
        nrm = np.cross(b - a, bc)
        nrm /= np.linalg.norm(nrm)
        m = np.cross(nrm, bc)
        d = np.asarray([-bond * np.cos(angle), bond * np.sin(angle) * np.cos(phi), bond * np.sin(angle) * np.sin(phi)])
        x.append(c + d[0] * bc + d[1] * m + d[2] * nrm)
    return np.asarray(x, np.float64).astype(np.float32)


def distance_pairs(elements, bonds, rotors):
    """bool [n, n]: the pairs whose distance no torsion changes: bonded, 1-3, and both atoms in the same rigid piece (no
    rotor has exactly one of them in its side, and they are connected)."""
    n = len(elements)
    adj = np.zeros((n, n), bool)
    for i, j, _ in bonds:
        adj[i, j] = adj[j, i] = True
    near = adj | ((adj.astype(int) @ adj.astype(int)) > 0)
    reach = adj | np.eye(n, dtype=bool)
    for _ in range(n):
        reach = (reach.astype(int) @ reach.astype(int)) > 0
    cut = np.zeros((n, n), bool)
    for rotor in rotors:
        cut |= rotor[2][:, None] != rotor[2][None, :]
    return (near | (reach & ~cut)) & ~np.eye(n, dtype=bool)


def distances(x):
    x = np.asarray(x, np.float64)
    return np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))


def distance_tolerance(x0, x, n_rotors=V.MAX_TORSIONS):
    """How far a distance that the pose keeps may differ between the float32 input and the float32 result.  Both ends are
    rounded to float32 once: 2 atoms x sqrt(3) x half an ulp at the largest |coordinate| of either set, eps32 |x|max each.
    Between the roundings the coordinates are float64: every rotation (at most `n_rotors`, and the frame) multiplies and adds
    numbers no larger than the extent, a few eps64 each; 64 eps64 (n_rotors + 1) |x|max covers them with room to spare, and is
    2^-23 of the first part."""
    top = max(float(np.abs(np.asarray(x0, np.float64)).max()), float(np.abs(np.asarray(x, np.float64)).max()), 1.0)
    return 2 * np.sqrt(3.0) * V.EPS32 * top + 64 * V.EPS64 * (n_rotors + 1) * top


def pose_tolerance(x):
    """How far coordinates recomputed from the STORED float32 pose (t, q, theta) may be from the device's, which used the
    float64 pose: a float32 rounding of t moves an atom by eps32 |t|, of q turns it by 2 eps32 (4 components, |dq| <= eps32
    each) about the origin of y, of a theta by eps32 |theta| <= 4 eps32 about its axis, at most 32 of them: together
    (|t| + 2 |x| + 32 * 4 |x|) eps32 <= 131 eps32 |x|max with |x|max the largest world coordinate (the lever arms are no
    longer), plus one float32 rounding of the result."""
    top = max(float(np.abs(np.asarray(x, np.float64)).max()), 1.0)
    return 132 * V.EPS32 * top


# ---- the one-torsion known answer ----------------------------------------------------------------------------------------------
WELL = 0.002874                        # the inner well of the C-C pair (class-only codes), surface distance in A
RADIUS = BOND * np.sin(ANGLE)          # of C3's circle about the axis C1 -> C2: 1.4284 A


def one_torsion(phi_deg):
    """The inputs of the scoring kernels for butane at dihedral phi and one pocket carbon: C1 at the origin, C2 on +x, C0 in
    the xy plane, C3 on its circle; the pocket atom Q in the circle's plane, 3.8 + WELL - 0.6 A outside the circle at 60
    degrees.  All codes are 1 (class C, no flags)."""
    x = chain_coordinates([np.deg2rad(phi_deg)])
    centre = np.asarray([BOND - BOND * np.cos(ANGLE), 0.0, 0.0])
    out = np.asarray([0.0, np.cos(np.pi / 3), np.sin(np.pi / 3)])
    q = centre + (RADIUS + 3.8 + WELL - 0.6) * out
    return {"lig_x": x, "lig_code": np.ones(4, np.int32), "mol_off": np.asarray([0, 4], np.int32),
            "mol_group": np.zeros(1, np.int32), "mol_int": np.asarray([[4, 0, 1, 0]], np.int32),
            "poc_x": q[None].astype(np.float32), "poc_code": np.ones(1, np.int32), "group_off": np.asarray([0, 1], np.int32)}


def one_torsion_tree():
    t = type_inputs([C.chain(4)])
    return V._vina_torsions_host(*(t[k] for k in C.TYPE_KEYS))


def one_torsion_energy(phi):
    """inter (float64) of the case with C3 at dihedral phi (rad, array), by its own arithmetic: three gaussian-type terms of
    four C-C pairs."""
    b = one_torsion(0.0)
    q = b["poc_x"][0].astype(np.float64)
    fixed = b["lig_x"][:3].astype(np.float64)
    centre = np.asarray([BOND - BOND * np.cos(ANGLE), 0.0, 0.0])
    phi = np.asarray(phi, np.float64)
    c3 = centre + RADIUS * np.stack([0 * phi, np.cos(phi), np.sin(phi)], -1)
    total = np.zeros(phi.shape)
    for pos in [fixed[0], fixed[1], fixed[2], c3]:
        d = np.sqrt(((pos - q) ** 2).sum(-1)) - 3.8
        total = total + V.WEIGHTS[0] * np.exp(-(d / 0.5) ** 2) + V.WEIGHTS[1] * np.exp(-((d - 3) / 2) ** 2) + \
            V.WEIGHTS[2] * np.where(d < 0, d * d, 0.0)
    return total


def one_torsion_wells():
    """The two minima of the scan in degrees (grid of 1e-4 degree around each, after a coarse scan)."""
    coarse = np.deg2rad(np.arange(0.0, 120.0, 0.01))
    e = one_torsion_energy(coarse)
    wells = []
    for lo, hi in ((0.0, 60.0), (60.0, 120.0)):
        sel = (coarse >= np.deg2rad(lo)) & (coarse < np.deg2rad(hi))
        k = np.deg2rad(np.rad2deg(coarse[sel][np.argmin(e[sel])]) + np.arange(-0.02, 0.02, 1e-5))
        wells.append(float(np.rad2deg(k[np.argmin(one_torsion_energy(k))])))
    return wells


def dihedral_deg(x):
    """The dihedral 0-1-2-3 of four points, in degrees."""
    x = np.asarray(x, np.float64)
    b0, b1, b2 = x[0] - x[1], x[2] - x[1], x[3] - x[2]
    b1 = b1 / np.linalg.norm(b1)
    v, w = b0 - (b0 @ b1) * b1, b2 - (b2 @ b1) * b1
    return float(np.rad2deg(np.arctan2(np.cross(b1, v) @ w, v @ w)))


# ---- the typed batch of the intramolecular and flexible kernels -------------------------------------------------------------------
def _pocket_around(x, rng, count, lo=3.4, hi=6.5):
    """`count` pocket atoms scattered around the ligand coordinates x, none closer than `lo` to a ligand atom, every one
    within `hi` of one."""
    out = []
    while len(out) < count:
        p = x[rng.randint(len(x))] + rng.normal(size=3) * 3.0
        d = np.sqrt(((x - p) ** 2).sum(1))
        if d.min() > lo and d.min() < hi:
            out.append(p)
    return np.asarray(out, np.float32)


@functools.lru_cache(maxsize=None)
def flex_batch():
    """dict: the typing inputs, the scoring inputs (codes and mol_int by `_vina_type_host`, the tree by
    `_vina_torsions_host`) and notes.  Molecules: the 5ndu ligand at its crystal and at its `shifted` pose (group 0: its
    pocket behind 800 further atoms, 1087 in all: more than one tile), a folded heptane with intramolecular clashes and a folded decane (group 1, 40 atoms), benzene
    (no rotor), methylborane + tail (an untyped atom), a molecule with a NaN coordinate, an empty molecule, butane on an
    empty group and on a group id out of range (it has no intramolecular pair: its ends are 3 bonds apart), a pentane of untyped atoms."""
    rng = np.random.RandomState(11)
    z = C.fixture()
    el, bonds = C.fixture_ligand(z, "5ndu")
    folded7 = chain_coordinates(np.deg2rad([55.0, -50.0, 48.0, 62.0]))
    folded10 = chain_coordinates(np.deg2rad([60.0, 65.0, -70.0, 58.0, 175.0, -60.0, 62.0]))
    hexagon = np.asarray([[1.39 * np.cos(k * np.pi / 3), 1.39 * np.sin(k * np.pi / 3), 0.0] for k in range(6)], np.float32)
    borane = (["C", "C", "B", "C", "C", "C"], [(1, 0, 1), (2, 1, 1), (3, 2, 1), (4, 3, 1), (5, 4, 1)])
    nan6 = chain_coordinates(np.deg2rad([60.0, 60.0, 60.0]))
    nan6[2, 1] = np.nan
    mols = [((el, bonds), z["5ndu_crystal_x"], 0), ((el, bonds), z["5ndu_shifted_x"], 0), (C.chain(7), folded7, 1),
            (C.chain(10), folded10, 1), (C.benzene(), hexagon, 1), (borane, chain_coordinates(np.deg2rad([50.0, -55.0, 60.0])), 1),
            (C.chain(6), nan6, 1), (([], []), np.zeros((0, 3), np.float32), 1),
            (C.chain(4), chain_coordinates([1.0]), 2), (C.chain(4), chain_coordinates([2.0]), 9),
            ((["B"] * 5, C.chain(5)[1]), chain_coordinates([1.0, -1.0]), 1)]
    for k in (2, 3, 4, 5, 6, 10):                                                # group 1's molecules sit in its pocket's frame
        mols[k] = (mols[k][0], (np.asarray(mols[k][1], np.float64) + [30.0, -20.0, 10.0]).astype(np.float32), mols[k][2])
    t = type_inputs([m[0] for m in mols])
    code, mol_int = V._vina_type_host(*(t[k] for k in C.TYPE_KEYS))
    tree = V._vina_torsions_host(*(t[k] for k in C.TYPE_KEYS))
    near = np.concatenate([np.asarray(mols[k][1], np.float64) for k in (2, 3, 5)])
    pocket1 = _pocket_around(near, rng, 40)
    # group 0: 800 more atoms around the 5ndu ligand (none closer than 4.5 A) ahead of its 287 pocket atoms, so that the group is
    # longer than one tile of 1024 and both tiles hold counted pairs
    codes = np.asarray([1, 17, 2, 34, 66, 67], np.int32)
    filler = _pocket_around(z["5ndu_crystal_x"].astype(np.float64), rng, 800, lo=4.5, hi=12.0)
    poc_x = [np.concatenate([filler, z["5ndu_poc_x"].astype(np.float32)]), pocket1, np.zeros((0, 3), np.float32)]
    poc_code = [np.concatenate([rng.choice(codes, 800), z["5ndu_poc_code"].astype(np.int32)]), rng.choice(codes, 40), np.zeros(0, np.int32)]
    b = dict(t)
    b.update(lig_x=np.concatenate([np.asarray(m[1], np.float32).reshape(-1, 3) for m in mols]), lig_code=code,
             mol_group=np.asarray([m[2] for m in mols], np.int32), mol_int=mol_int, poc_x=np.concatenate(poc_x),
             poc_code=np.concatenate(poc_code), group_off=np.concatenate([[0], np.cumsum([len(p) for p in poc_x])]).astype(np.int32),
             tree=tree, graphs=[m[0] for m in mols], crystal=0, shifted=1, folded=2, decane=3, rigid=4, untyped_atom=5, nan_mol=6,
             empty_mol=7, empty_group=8, bad_group=9, untyped_mol=10)
    return b


def sub_batch(b, molecules):
    """`C.sub_batch` that carries the tree's rows along."""
    out, rows = C.sub_batch(b, molecules)
    tree, sel = b["tree"], list(molecules)
    out["tree"] = V.VinaTorsions(tree.ints[sel], tree.ends[sel], tree.sides[sel], tree.pair_mask[rows], out["mol_off"])
    out["graphs"] = [b["graphs"][m] for m in sel]
    return out, rows
