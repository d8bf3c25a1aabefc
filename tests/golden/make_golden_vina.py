#!/usr/bin/env python
"""Fixture of the Vina-type score (diffsbdd_amd/vina.py), made where the reference's example complexes exist:

    python tests/golden/make_golden_vina.py

  vina_crystal.npz   the two example complexes of the reference (example/3rfm.pdb + 3rfm_B_CFF.sdf, example/5ndu.pdb +
                     5ndu_C_8V2.sdf), read as DATA with this package's own readers: heavy-atom ligand coordinates, elements
                     and the SDF's bond list, the heavy atoms of the residues within 8 A with residue and atom names, a copy
                     of each ligand shifted 1.5 A towards its nearest pocket atom, and for each the atom codes, N_rot, the
                     five terms (per atom and per molecule), inter and the score.  Arrays only.

The stored values come from the dense float64 statement in THIS script -- its own typing rules on adjacency matrices, its own
list of residue atom flags, its own pair terms -- not from a call into diffsbdd_amd/vina.py, so the tests compare two
independent statements of the definitions.

Margin condition, asserted here in float64 for every stored case: no ligand-pocket pair lies within 1e-4 A of the 8 A cutoff,
so a float32 distance puts every pair on the same side of it.  A case that misses the condition is perturbed (seeded,
1e-3 A) until it holds.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from diffsbdd_amd import pocket as pocket_io  # noqa: E402
from oracle.ref_shim import REF_ROOT  # noqa: E402

COMPLEXES = (("3rfm", "3rfm.pdb", "3rfm_B_CFF.sdf"), ("5ndu", "5ndu.pdb", "5ndu_C_8V2.sdf"))
MARGIN = 1e-4
SHIFT = 1.5
CUTOFF = 8.0
ELEMENTS = ["", "C", "N", "O", "P", "S", "F", "Cl", "Br", "I"]                       # class id = index
RADII = np.asarray([0.0, 1.9, 1.8, 1.7, 2.1, 2.0, 1.5, 1.8, 2.0, 2.2, 1.2])
W = np.asarray([-0.035579, -0.005156, 0.840245, -0.035069, -0.587439])
HYD, DON, ACC = 16, 32, 64

# the protein side, written out: hydrophobic carbons (bonded to carbon only), donors, acceptors
HYDROPHOBIC_CARBONS = {
    "ALA": "CB", "VAL": "CB CG1 CG2", "LEU": "CB CG CD1 CD2", "ILE": "CB CG1 CG2 CD1", "PHE": "CB CG CD1 CD2 CE1 CE2 CZ",
    "TRP": "CB CG CD2 CE3 CZ2 CZ3 CH2", "TYR": "CB CG CD1 CD2 CE1 CE2", "MET": "CB", "PRO": "CB CG", "LYS": "CB CG CD",
    "ARG": "CB CG", "GLU": "CB CG", "GLN": "CB CG", "ASP": "CB", "ASN": "CB", "HIS": "CB", "THR": "CG2", "CYS": "", "SER": "",
    "GLY": ""}
SIDE_DONORS = {"ARG": "NE NH1 NH2", "ASN": "ND2", "GLN": "NE2", "HIS": "ND1 NE2", "LYS": "NZ", "SER": "OG", "THR": "OG1",
               "TYR": "OH", "TRP": "NE1"}
SIDE_ACCEPTOR_N = {"HIS": "ND1 NE2"}


def pocket_code(resname, atom, element):
    cls = ELEMENTS.index(element)
    assert resname in HYDROPHOBIC_CARBONS and 1 <= cls <= 5, (resname, atom, element)
    code = cls
    if element == "C" and atom in HYDROPHOBIC_CARBONS[resname].split():
        code |= HYD
    if (atom == "N" and resname != "PRO") or atom in SIDE_DONORS.get(resname, "").split():
        code |= DON
    if element == "O" or atom in SIDE_ACCEPTOR_N.get(resname, "").split():
        code |= ACC
    return code


def read_ligand(sdf):
    """(xyz, elements, bonds) of the first record, heavy atoms only; the bond block by the counts line's columns."""
    xyz = pocket_io.read_sdf_coords(sdf)
    with open(sdf) as f:
        lines = f.read().splitlines()
    n, nb = len(xyz), int(lines[3][3:6])
    elements = [l[31:34].strip().capitalize() for l in lines[4:4 + n]]                # the files write CL
    bonds = [(int(l[0:3]) - 1, int(l[3:6]) - 1, int(l[6:9])) for l in lines[4 + n:4 + n + nb]]
    keep = [k for k, e in enumerate(elements) if e not in ("H", "D")]
    index = {a: k for k, a in enumerate(keep)}
    bonds = [(index[i], index[j], o) for i, j, o in bonds if i in index and j in index]
    assert all(o in (1, 2, 3) for _, _, o in bonds)
    return xyz[keep], [elements[k] for k in keep], np.asarray(bonds, np.int32).reshape(-1, 3)


def type_ligand(elements, bonds):
    """Codes and N_rot from matrices: A = orders, reachability by repeated squaring of the boolean adjacency."""
    n = len(elements)
    cls = np.asarray([ELEMENTS.index(e) if e in ELEMENTS[1:] else 0 for e in elements])
    A = np.zeros((n, n), np.int64)
    for i, j, o in bonds:
        A[i, j] = A[j, i] = o
    s, top, deg = A.sum(1), A.max(1), (A > 0).sum(1)
    hetero = ((A > 0) @ (cls != 1).astype(np.int64)) > 0
    code = cls.copy()
    code[(cls == 1) & ~hetero] |= HYD
    code[np.isin(cls, (6, 7, 8, 9))] |= HYD
    code[(cls == 2) & (s < 3)] |= DON
    code[(cls == 2) & (s == 3) & (top >= 2)] |= ACC
    code[cls == 3] |= ACC
    code[(cls == 3) & (s < 2)] |= DON

    def connected(adj, a, c):
        reach = np.eye(n, dtype=bool) | adj
        for _ in range(max(int(np.ceil(np.log2(max(n, 2)))), 1)):
            reach = reach | ((reach.astype(np.int64) @ reach.astype(np.int64)) > 0)
        return bool(reach[a, c])

    n_rot = 0
    for i, j, o in bonds:
        if o == 1 and deg[i] >= 2 and deg[j] >= 2:
            cut = A > 0
            cut[i, j] = cut[j, i] = False
            n_rot += not connected(cut, i, j)
    return code.astype(np.int32), int(n_rot)


def brute_force(lig_x, lig_code, poc_x, poc_code, n_rot):
    """float64 dense statement -> (atom [n,5], terms [5], inter, score, smallest |r - 8|)."""
    x, q = np.asarray(lig_x, np.float64), np.asarray(poc_x, np.float64)
    r = np.sqrt(((x[:, None, :] - q[None, :, :]) ** 2).sum(-1))
    ci, cj = np.asarray(lig_code)[:, None], np.asarray(poc_code)[None, :]
    d = r - RADII[ci & 15] - RADII[cj & 15]
    on = (r < CUTOFF) & ((ci & 15) != 0) & ((cj & 15) != 0)
    both_hyd = (ci & cj & HYD) != 0
    hb = (((ci & DON) != 0) & ((cj & ACC) != 0)) | (((ci & ACC) != 0) & ((cj & DON) != 0))
    f = np.zeros(r.shape + (5,))
    f[..., 0] = np.exp(-(d / 0.5) ** 2)
    f[..., 1] = np.exp(-((d - 3.0) / 2.0) ** 2)
    f[..., 2] = np.where(d < 0, d ** 2, 0.0)
    f[..., 3] = np.where(both_hyd, np.clip(1.5 - d, 0.0, 1.0), 0.0)
    f[..., 4] = np.where(hb, np.clip(-d / 0.7, 0.0, 1.0), 0.0)
    f *= on[..., None]
    atom = f.sum(1)
    terms = f.sum((0, 1))
    inter = float(W @ terms)
    return atom, terms, inter, inter / (1.0 + 0.05846 * n_rot), float(np.abs(r - CUTOFF).min())


def settled(lig_x, poc_x, seed):
    """`lig_x` (float32), perturbed until the margin condition holds."""
    rng = np.random.RandomState(seed)
    x = np.asarray(lig_x, np.float32)
    for _ in range(100):
        r = np.sqrt(((x[:, None, :].astype(np.float64) - poc_x[None, :, :]) ** 2).sum(-1))
        if np.abs(r - CUTOFF).min() > MARGIN:
            return x
        x = (lig_x + rng.uniform(-1e-3, 1e-3, lig_x.shape)).astype(np.float32)
    raise RuntimeError("no perturbation satisfies the margin condition")


def main():
    out = {"margin": np.float64(MARGIN), "names": np.asarray([c[0] for c in COMPLEXES])}
    for k, (name, pdb, sdf) in enumerate(COMPLEXES):
        pdb, sdf = os.path.join(REF_ROOT, "example", pdb), os.path.join(REF_ROOT, "example", sdf)
        lig_x, lig_el, bonds = read_ligand(sdf)
        residues = pocket_io.pocket_residues_from_ligand(pocket_io.read_pdb_residues(pdb), pocket_io.read_sdf_coords(sdf))
        atoms = [(r["resname"], a[0], a[1], a[2]) for r in residues for a in r["atoms"] if a[1] not in ("H", "D")]
        poc_x = np.asarray([a[3] for a in atoms], np.float32)
        poc_code = np.asarray([pocket_code(a[0], a[1], a[2]) for a in atoms], np.int32)
        lig_code, n_rot = type_ligand(lig_el, bonds)
        d = np.sqrt(((lig_x[:, None, :].astype(np.float64) - poc_x[None, :, :]) ** 2).sum(-1))
        i, j = np.unravel_index(d.argmin(), d.shape)
        step = (poc_x[j].astype(np.float64) - lig_x[i]) / d[i, j] * SHIFT
        ligands = {"crystal": settled(lig_x, poc_x, 10 * k), "shifted": settled((lig_x + step).astype(np.float32), poc_x, 10 * k + 1)}
        out[f"{name}_lig_el"], out[f"{name}_lig_bonds"] = np.asarray(lig_el), bonds
        out[f"{name}_lig_code"], out[f"{name}_n_rot"] = lig_code, np.int32(n_rot)
        out[f"{name}_poc_x"], out[f"{name}_poc_code"] = poc_x, poc_code
        out[f"{name}_poc_res"], out[f"{name}_poc_atom"] = np.asarray([a[0] for a in atoms]), np.asarray([a[1] for a in atoms])
        for variant, x in ligands.items():
            atom, terms, inter, score, margin = brute_force(x, lig_code, poc_x, poc_code, n_rot)
            assert margin > MARGIN
            out[f"{name}_{variant}_x"], out[f"{name}_{variant}_atom"], out[f"{name}_{variant}_terms"] = x, atom, terms
            out[f"{name}_{variant}_inter"], out[f"{name}_{variant}_score"] = np.float64(inter), np.float64(score)
            print(f"{name} {variant}: {len(x)} ligand / {len(poc_x)} pocket heavy atoms, N_rot {n_rot}, terms "
                  f"{np.round(terms, 4).tolist()}, score {score:.4f} kcal/mol, margin {margin:.2e}")
    path = os.path.join(HERE, "vina_crystal.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
