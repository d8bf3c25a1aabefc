"""Inputs shared by tests/test_pose.py and tests/test_gpu_pose.py: the crystal fixture (tests/golden/pose_crystal.npz),
the exact tie / threshold cases, and one ragged batch built to hit every path of pose_check_kernel."""
import os

import numpy as np

from diffsbdd_amd import pose

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_crystal.npz")

# Exact cases: small integer coordinates and radii 1.75 (Cl), so every operation is exact.  With tol 0.5 the clash limit of
# two such atoms is 1.75 + 1.75 - 0.5 = 3.0 exactly.
EXACT_POCKET_X = np.asarray([[3, 0, 0], [-3, 0, 0], [0, 4, 0]], np.float32)
EXACT_POCKET_R = np.asarray([1.75, 1.75, 1.75], np.float32)
# ligand A at the origin: d = 3, 3, 4 -> nearest 0 (tie with 1), no clash (3 == limit), contacts 2 (4 == cutoff is none)
# ligand B at (1, 0, 0):  d = 2, 4, sqrt(17) -> one clash, one contact (4 == cutoff is none), nearest 0
EXACT_A = np.asarray([[0, 0, 0]], np.float32)
EXACT_B = np.asarray([[1, 0, 0]], np.float32)
EXACT_R = np.asarray([1.75], np.float32)
EXACT_A_ATOM = [0, 2, 0, int(np.float32(3.0).view(np.int32))]
EXACT_B_ATOM = [1, 1, 0, int(np.float32(2.0).view(np.int32))]

_RADII = np.asarray(sorted(set(pose.VDW_RADII.values())) + [pose.DEFAULT_RADIUS], np.float32)


def fixture_cases():
    """[(label, (lig_x, lig_el), (poc_x, poc_el), tol, atom int32 [n,3] = clashes, contacts, nearest, dmin float64 [n])]"""
    z = np.load(GOLDEN)
    out = []
    for name in z["names"]:
        for variant in ("crystal", "shifted"):
            for tol in z["tols"]:
                key = f"{name}_{variant}_tol{tol}"
                out.append((key, (z[f"{name}_{variant}_x"], [str(s) for s in z[f"{name}_lig_el"]]),
                            (z[f"{name}_poc_x"], [str(s) for s in z[f"{name}_poc_el"]]), float(tol), z[key + "_atom"],
                            z[key + "_dmin"]))
    return out, float(z["contact"])


def ball_residues(seed, n_atoms, radius=60.0):
    """A synthetic "pocket" for the sampler tests: `n_atoms` atoms (C, N, O, S) uniform in a ball, one pseudo-residue per
    atom (full-atom featurisation reads element and position only).

    Why not the example pockets: a network with random weights does not denoise, so a reverse chain ends about
    1 / alpha_T = 45 times wider than it started (small_cond: polynomial_2, precision 5e-4) -- its atoms land tens of
    Angstrom from the pocket centre, where a 12 A crystal pocket has no atom to clash with (measured: no clash and no contact
    in 8 samples for any cut of 3rfm / 5ndu and 4 to 20 steps).  A ball of 60 A with one atom per 150 cubic Angstrom puts
    protein atoms where the samples go: about one clash per five ligand atoms."""
    rng = np.random.RandomState(seed)
    v = rng.normal(size=(n_atoms, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    x = (v * radius * rng.uniform(0, 1, (n_atoms, 1)) ** (1.0 / 3.0)).astype(np.float32)
    elements = rng.choice(["C", "C", "N", "O", "S"], n_atoms)
    return [dict(chain="A", resseq=i + 1, icode=" ", resname="ALA", hetero=False,
                 atoms=[("X", str(e), tuple(float(c) for c in p))]) for i, (p, e) in enumerate(zip(x, elements))]


def ragged_batch(seed=0):
    """dict of the kernel's inputs (numpy).  Molecule sizes 0, 1, 63, 64, 65, 129 (> 2 rounds of the 4 waves) and 300 (more
    atoms than the workgroup has threads); group sizes 0, 1, 63, 64, 65 and 1025 (one LDS tile + 1); several molecules on one
    group; an unreferenced group; unsorted mol_group; the exact tie / threshold cases; one molecule with a NaN and an inf
    coordinate.  16 molecules, 712 ligand atoms."""
    rng = np.random.RandomState(seed)
    group_sizes = [0, 1, 63, 64, 65, 1025, len(EXACT_POCKET_X), 10]          # group 6: exact cases, group 7: unreferenced
    mols = [(0, 5), (1, 2), (63, 5), (64, 4), (65, 3), (129, 5), (300, 5), (7, 0), (9, 1), ("A", 6), ("B", 6), ("nan", 5),
            (20, 2), (33, 3), (2, 4), (12, 1)]
    # a group's atoms fill a box with one atom per 60 cubic Angstrom, its ligands the same box: about two pocket atoms
    # inside an atom's clash limit (3 - 3.5 A), so atoms with several clashes, with contacts only and with neither all occur
    boxes = [max(60.0 * m, 60.0) ** (1.0 / 3.0) for m in group_sizes]
    poc_x, poc_r = [], []
    for g, m in enumerate(group_sizes):
        if g == 6:
            poc_x.append(EXACT_POCKET_X)
            poc_r.append(EXACT_POCKET_R)
        else:
            poc_x.append(rng.uniform(0, boxes[g], (m, 3)).astype(np.float32))
            poc_r.append(rng.choice(_RADII, m).astype(np.float32))
    lig_x, lig_r, groups = [], [], []
    for size, g in mols:
        if size == "A" or size == "B":
            x, r = (EXACT_A if size == "A" else EXACT_B), EXACT_R
        elif size == "nan":
            x = rng.uniform(0, boxes[g], (5, 3)).astype(np.float32)
            x[1, 2], x[3, 0] = np.nan, np.inf
            r = rng.choice(_RADII, 5).astype(np.float32)
        else:
            x = rng.uniform(0, boxes[g], (size, 3)).astype(np.float32)
            r = rng.choice(_RADII, size).astype(np.float32)
        if size == 300:                               # its first atom sits next to the one pocket atom of the second LDS tile
            x[0] = poc_x[5][1024] + np.asarray([0.25, 0, 0], np.float32)
        lig_x.append(x)
        lig_r.append(r)
        groups.append(g)
    return {"lig_x": np.concatenate(lig_x), "lig_r": np.concatenate(lig_r),
            "mol_off": np.concatenate([[0], np.cumsum([len(x) for x in lig_x])]).astype(np.int32),
            "mol_group": np.asarray(groups, np.int32), "poc_x": np.concatenate(poc_x), "poc_r": np.concatenate(poc_r),
            "group_off": np.concatenate([[0], np.cumsum(group_sizes)]).astype(np.int32),
            "exact": {9: EXACT_A_ATOM, 10: EXACT_B_ATOM}, "nan_mol": 11}
