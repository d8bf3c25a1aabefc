#!/usr/bin/env python
"""Fixture of the pose checks (diffsbdd_amd/pose.py), made where the reference's example complexes exist:

    python tests/golden/make_golden_pose.py

  pose_crystal.npz   the two example complexes of the reference (example/3rfm.pdb + 3rfm_B_CFF.sdf, example/5ndu.pdb +
                     5ndu_C_8V2.sdf), read as DATA with this package's own readers (pocket.py, ligand_io.py): heavy-atom
                     ligand coordinates and element symbols, the heavy atoms of the residues within 8 A, a copy of each
                     ligand shifted 1.5 A towards its nearest pocket atom, and for every (complex, ligand, tol) case the
                     FLOAT64 brute-force result (distance matrix in double, then counts and nearest).  Arrays only.

Margin condition, asserted here in float64 for every stored case: no pair lies within 1e-4 A of a threshold it is compared
with (r_i + r_j - tol for both tol values, the contact cutoff), and an atom's two smallest distances differ by more than
1e-4 A -- so float32 counts and nearest indices can be demanded EQUAL to these.  A case that misses the condition is
perturbed (seeded, 1e-3 A) until it holds.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from diffsbdd_amd import pose  # noqa: E402
from diffsbdd_amd import pocket as pocket_io  # noqa: E402
from oracle.ref_shim import REF_ROOT  # noqa: E402

COMPLEXES = (("3rfm", "3rfm.pdb", "3rfm_B_CFF.sdf"), ("5ndu", "5ndu.pdb", "5ndu_C_8V2.sdf"))
TOLS = (0.5, 0.0)
CONTACT = pose.CONTACT_CUTOFF
MARGIN = 1e-4
SHIFT = 1.5


def read_ligand(sdf):
    """(xyz, element symbols) of the first record.  The example files' counts lines carry no version tag, which
    `ligand_io.read_sdf_molecules` insists on: coordinates through `pocket.read_sdf_coords`, the symbols from the same
    atom lines and columns as `ligand_io` reads them."""
    xyz = pocket_io.read_sdf_coords(sdf)
    with open(sdf) as f:
        lines = f.read().splitlines()
    return xyz, [l[31:34].strip() for l in lines[4:4 + len(xyz)]]


def brute_force(lig_x, lig_r, poc_x, poc_r, tol, contact=CONTACT):
    """float64: -> (atom int32 [n,3] = clashes, contacts, nearest; dmin float64 [n]; smallest distance to any threshold
    or between an atom's two nearest)."""
    x, q = np.asarray(lig_x, np.float64), np.asarray(poc_x, np.float64)
    d = np.sqrt(((x[:, None, :] - q[None, :, :]) ** 2).sum(-1))
    limit = np.asarray(lig_r, np.float64)[:, None] + np.asarray(poc_r, np.float64)[None, :] - tol
    atom = np.stack([(d < limit).sum(1), (d < contact).sum(1), d.argmin(1)], 1).astype(np.int32)
    two = np.sort(d, 1)[:, :2]
    margin = min(np.abs(d - limit).min(), np.abs(d - contact).min(), (two[:, 1] - two[:, 0]).min())
    return atom, d.min(1), float(margin)


def settled(lig_x, lig_r, poc_x, poc_r, seed):
    """`lig_x` (float32), perturbed until every tol's case holds the margin condition."""
    rng = np.random.RandomState(seed)
    x = np.asarray(lig_x, np.float32)
    for _ in range(100):
        if all(brute_force(x, lig_r, poc_x, poc_r, tol)[2] > MARGIN for tol in TOLS):
            return x
        x = (lig_x + rng.uniform(-1e-3, 1e-3, lig_x.shape)).astype(np.float32)
    raise RuntimeError("no perturbation satisfies the margin condition")


def main():
    out = {"tols": np.asarray(TOLS, np.float64), "contact": np.float64(CONTACT), "margin": np.float64(MARGIN),
           "names": np.asarray([c[0] for c in COMPLEXES])}
    for k, (name, pdb, sdf) in enumerate(COMPLEXES):
        pdb, sdf = os.path.join(REF_ROOT, "example", pdb), os.path.join(REF_ROOT, "example", sdf)
        xyz, elements = read_ligand(sdf)
        lig_x, lig_r, keep = pose.heavy_atoms(xyz, elements)
        lig_el = [elements[i] for i in keep]
        residues = pocket_io.pocket_residues_from_ligand(pocket_io.read_pdb_residues(pdb), pocket_io.read_sdf_coords(sdf))
        poc_x, poc_r = pose.pocket_atoms(residues)
        poc_el = [a[1] for r in residues for a in r["atoms"] if a[1] not in pose.HYDROGENS]
        assert np.array_equal(pose.radii_of(poc_el), poc_r)
        packaged = np.load(os.path.join(ROOT, "diffsbdd_amd", "data", f"pocket_{name}.npz"))
        assert np.array_equal(poc_x, packaged["fa_x"]), f"{name}: pocket differs from the packaged fa_x"
        # the ligand moved 1.5 A along the line from its atom nearest to the pocket towards that pocket atom
        d = np.sqrt(((lig_x[:, None, :].astype(np.float64) - poc_x[None, :, :]) ** 2).sum(-1))
        i, j = np.unravel_index(d.argmin(), d.shape)
        step = (poc_x[j].astype(np.float64) - lig_x[i]) / d[i, j] * SHIFT
        ligands = {"crystal": settled(lig_x, lig_r, poc_x, poc_r, 10 * k),
                   "shifted": settled((lig_x + step).astype(np.float32), lig_r, poc_x, poc_r, 10 * k + 1)}
        out[f"{name}_lig_el"], out[f"{name}_poc_el"] = np.asarray(lig_el), np.asarray(poc_el)
        out[f"{name}_poc_x"] = poc_x
        for variant, x in ligands.items():
            out[f"{name}_{variant}_x"] = x
            for tol in TOLS:
                atom, dmin, margin = brute_force(x, lig_r, poc_x, poc_r, tol)
                assert margin > MARGIN
                out[f"{name}_{variant}_tol{tol}_atom"], out[f"{name}_{variant}_tol{tol}_dmin"] = atom, dmin
                print(f"{name} {variant} tol {tol}: {len(x)} ligand / {len(poc_x)} pocket heavy atoms, clash pairs "
                      f"{atom[:, 0].sum()}, contact pairs {atom[:, 1].sum()}, smallest distance {dmin.min():.4f}, "
                      f"margin {margin:.2e}")
    path = os.path.join(HERE, "pose_crystal.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
