"""Pose checks on the device: does a ligand sit in its pocket without running into the protein?

For every ligand heavy atom the kernel `dsbdd_pose_check` (csrc/pose_check.h) counts the pocket heavy atoms it clashes
with and those it is in contact with, and finds the nearest one; for every molecule it gives the totals.  One launch on
the device tensors the samplers return, before a molecule is built, so the samplers and the test-set driver can reject
a pose that clashes the way they reject an over-valent molecule.

Definitions (float32, every operation rounded on its own; `_pose_check_host` restates them in numpy and is the
specification the kernel is tested against bit for bit -- it is not a fallback, the public entry points refuse CPU tensors):

    d       = sqrt((dx dx + dy dy) + dz dz)
    clash   iff d < (r_i + r_j) - tol          strict; r = van-der-Waals radius (VDW_RADII)
    contact iff d < contact                     strict

`CLASH_TOLERANCE` = 0.5 A is the overlap allowance of PoseCheck's clash count (Harris et al. 2023: a clash is a pair closer
than the sum of the van-der-Waals radii minus 0.5 A); `CONTACT_CUTOFF` = 4.0 A is the customary heavy-atom distance cutoff
for a ligand-protein contact.  Both are conventions, not fitted values, and parameters of every entry point.

  python -m diffsbdd_amd.pose --pdbfile P.pdb --sdf L.sdf [L2.sdf ...] [--scope protein|pocket] [--ref_ligand ...]
                              [--tol 0.5] [--contact 4.0] [--out pose.csv]
"""
from __future__ import annotations

import argparse
import ctypes
import sys
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, _pairs
from ._pairs import HYDROGENS, _default_groups, _checked_groups, _np, _ptr, _symbol, select_residues  # noqa: F401

# van-der-Waals radii in Angstrom: Bondi (1964); B from Mantina et al. (2009)
VDW_RADII = {"C": 1.70, "N": 1.55, "O": 1.52, "F": 1.47, "P": 1.80, "S": 1.80, "Cl": 1.75, "Br": 1.85, "I": 1.98,
             "B": 1.92, "Se": 1.90}
DEFAULT_RADIUS = 2.00                 # every other element
CLASH_TOLERANCE = 0.5
CONTACT_CUTOFF = 4.0

# columns of PoseStats.atom / PoseStats.mol (csrc/pose_check.h)
A_CLASH, A_CONTACT, A_NEAREST, A_DIST_BITS = range(4)
M_ATOMS, M_CLASH_PAIRS, M_CLASH_ATOMS, M_CONTACT_PAIRS, M_CONTACT_ATOMS, M_NONFINITE, M_DIST_BITS = range(7)
ATOM_OUT, MOL_OUT = 4, 8
_INF_BITS = int(np.float32(np.inf).view(np.int32))

POSE_COVERAGE = (
    "pose checks: PRESENT = clash pairs, clashing atoms, contact pairs, atoms in contact, nearest protein atom and smallest "
    "distance of every ligand, computed by one GPU kernel from heavy-atom coordinates; heavy atoms only (no hydrogens on "
    "either side), fixed van-der-Waals radii per element (Bondi; 2.0 A for elements outside the table), rigid protein, no "
    "ligand-internal clashes; "
    "CHECKED ATOMS = only the residues given: the samplers and the test-set driver check the pocket selection they sample "
    "in, `python -m diffsbdd_amd.pose` checks every ATOM residue of the file by default (--scope protein) or the residues "
    "within 8 A of --ref_ligand (--scope pocket) -- a clash with a residue outside the selection is not seen; "
    "DEFINED AS = clash: distance < r_i + r_j - tol (tol 0.5 A, the clash definition of PoseCheck), contact: distance < "
    "4.0 A; "
    "NOT = a docking score, an energy or a strain measure, and NOT comparable with PoseBusters or PoseCheck numbers "
    "(different atoms, radii and hydrogens); ABSENT = RDKit/UFF relaxation and external docking (refused).")


def radii_of(symbols):
    """van-der-Waals radii float32 [n] of element symbols; `DEFAULT_RADIUS` for an element outside `VDW_RADII`."""
    return np.asarray([VDW_RADII.get(_symbol(s), DEFAULT_RADIUS) for s in symbols], np.float32)


def heavy_atoms(xyz, symbols):
    """(xyz float32 [n,3], radii float32 [n], kept indices) of the atoms that are not hydrogens."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    if len(symbols) != len(xyz):
        raise ValueError(f"{len(xyz)} coordinates for {len(symbols)} elements")
    keep = np.asarray([k for k, s in enumerate(symbols) if _symbol(s) not in HYDROGENS], np.int64)
    return xyz[keep], radii_of([symbols[k] for k in keep]), keep


def pocket_atoms(residues):
    """Residue dicts of `pocket.read_pdb_residues` -> (xyz float32 [M,3], radii float32 [M]): heavy atoms only, in file
    order."""
    xyz, symbols = [], []
    for res in residues:
        for _, elem, pos in res["atoms"]:
            xyz.append(pos)
            symbols.append(elem)
    x, r, _ = heavy_atoms(np.asarray(xyz, np.float32).reshape(-1, 3), symbols)
    return x, r


def _check_thresholds(tol, contact):
    tol, contact = float(tol), float(contact)
    if not (np.isfinite(tol) and tol >= 0.0 and np.isfinite(contact) and contact >= 0.0):
        raise ValueError(f"tol = {tol} and contact = {contact} must be finite and not negative")
    return tol, contact


# ---- results -------------------------------------------------------------------------------------------------------------
def _totals(atom, finite):
    """int32 [8] of one molecule from its atoms' records: the per-molecule output of the kernel."""
    atom = np.asarray(atom, np.int32).reshape(-1, ATOM_OUT)
    d = np.ascontiguousarray(atom[:, A_DIST_BITS]).view(np.float32)
    out = np.zeros(MOL_OUT, np.int32)
    out[M_ATOMS] = len(atom)
    out[M_CLASH_PAIRS], out[M_CLASH_ATOMS] = atom[:, A_CLASH].sum(), (atom[:, A_CLASH] > 0).sum()
    out[M_CONTACT_PAIRS], out[M_CONTACT_ATOMS] = atom[:, A_CONTACT].sum(), (atom[:, A_CONTACT] > 0).sum()
    out[M_NONFINITE] = int(not np.all(finite))
    out[M_DIST_BITS] = np.float32(d.min() if len(d) else np.inf).view(np.int32)
    return out


@dataclass
class MolPose:
    """The pose record of one molecule (host arrays): what the samplers attach to a `Molecule` as `m.pose`."""
    mol: np.ndarray          # int32 [8]: n_atoms, clash pairs, clash atoms, contact pairs, contact atoms, nonfinite, bits of the smallest d, 0
    atom: np.ndarray         # int32 [n, 4]: clashing pocket atoms, pocket atoms in contact, nearest pocket atom (-1: none), bits of its d
    finite: np.ndarray       # bool [n]: the atom's coordinates are finite
    tol: float = CLASH_TOLERANCE
    contact: float = CONTACT_CUTOFF

    n_atoms = property(lambda self: int(self.mol[M_ATOMS]))
    clash_pairs = property(lambda self: int(self.mol[M_CLASH_PAIRS]))
    clash_atoms = property(lambda self: int(self.mol[M_CLASH_ATOMS]))
    contact_pairs = property(lambda self: int(self.mol[M_CONTACT_PAIRS]))
    contact_atoms = property(lambda self: int(self.mol[M_CONTACT_ATOMS]))
    nonfinite = property(lambda self: int(self.mol[M_NONFINITE]))
    min_distance = property(lambda self: float(self.mol[M_DIST_BITS:M_DIST_BITS + 1].view(np.float32)[0]))
    nearest = property(lambda self: self.atom[:, A_NEAREST])
    atom_clashes = property(lambda self: self.atom[:, A_CLASH])
    atom_contacts = property(lambda self: self.atom[:, A_CONTACT])
    atom_distance = property(lambda self: np.ascontiguousarray(self.atom[:, A_DIST_BITS]).view(np.float32))

    def subset(self, keep):
        """The record of the atoms `keep` alone (a fragment): per-atom rows carried along, totals recomputed from them."""
        keep = np.asarray(keep, np.int64).reshape(-1)
        atom, finite = self.atom[keep].copy(), self.finite[keep].copy()
        return MolPose(_totals(atom, finite), atom, finite, self.tol, self.contact)

    def as_dict(self):
        return {"n_atoms": self.n_atoms, "clash_pairs": self.clash_pairs, "clash_atoms": self.clash_atoms,
                "contact_pairs": self.contact_pairs, "contact_atoms": self.contact_atoms, "nonfinite": self.nonfinite,
                "min_distance": self.min_distance}


@dataclass
class PoseStats:
    """The two outputs of `dsbdd_pose_check` (device tensors from `pose_check`, numpy arrays from `_pose_check_host`)."""
    atom: object             # int32 [N, 4]
    mol: object              # int32 [B, 8]
    mol_off: object          # int32 [B + 1]
    x: object = None         # the coordinates [N, 3] the records belong to (`subset` reads which are finite)
    tol: float = CLASH_TOLERANCE
    contact: float = CONTACT_CUTOFF

    def _bits(self, column):
        if torch.is_tensor(column):
            return column.contiguous().view(torch.float32)
        return np.ascontiguousarray(column).view(np.float32)

    n_atoms = property(lambda self: self.mol[:, M_ATOMS])
    clash_pairs = property(lambda self: self.mol[:, M_CLASH_PAIRS])
    clash_atoms = property(lambda self: self.mol[:, M_CLASH_ATOMS])
    contact_pairs = property(lambda self: self.mol[:, M_CONTACT_PAIRS])
    contact_atoms = property(lambda self: self.mol[:, M_CONTACT_ATOMS])
    nonfinite = property(lambda self: self.mol[:, M_NONFINITE])
    min_distance = property(lambda self: self._bits(self.mol[:, M_DIST_BITS]))
    nearest = property(lambda self: self.atom[:, A_NEAREST])
    atom_clashes = property(lambda self: self.atom[:, A_CLASH])
    atom_contacts = property(lambda self: self.atom[:, A_CONTACT])
    atom_distance = property(lambda self: self._bits(self.atom[:, A_DIST_BITS]))

    def _finite(self, atom, rows=None):
        if self.x is None:
            return np.ones(len(atom), bool)
        x = _np(self.x).reshape(-1, 3)
        return np.isfinite(x if rows is None else x[rows]).all(1)

    def subset(self, rows):
        """`MolPose` of the atom rows `rows` (indices into the batch): a fragment's totals are sums over its atoms."""
        rows = np.asarray(_np(rows), np.int64).reshape(-1)
        atom = _np(self.atom)[rows].copy()
        finite = self._finite(atom, rows)
        return MolPose(_totals(atom, finite), atom, finite, self.tol, self.contact)

    def molecules(self):
        """One `MolPose` per molecule, in order (one copy of each tensor to the host)."""
        atom, mol, off = _np(self.atom), _np(self.mol), _np(self.mol_off)
        finite = self._finite(atom)
        return [MolPose(mol[b].copy(), atom[off[b]:off[b + 1]].copy(), finite[off[b]:off[b + 1]].copy(), self.tol,
                        self.contact) for b in range(len(mol))]


# ---- the device path -------------------------------------------------------------------------------------------------------
class PocketAtoms(_pairs.PocketGroups):
    """`_pairs.PocketGroups` with the van-der-Waals radii r [M] float32; `upload` takes (xyz [m,3], radii [m]) per group."""
    COLUMN, DTYPE, WHAT = "r", np.float32, "radius"


def radius_table(atom_decoder):
    """float32 [n_types]: the radius of every class of a sampler's atom decoder."""
    if any(_symbol(s) in HYDROGENS for s in atom_decoder):
        raise ValueError("the atom decoder holds hydrogens: pose checks are defined on heavy atoms (drop them and pass radii)")
    return radii_of(atom_decoder)


def pose_check(x, atom_type_or_radii, lig_mask, pockets, mol_group=None, batch=None, tol=CLASH_TOLERANCE,
               contact=CONTACT_CUTOFF, info=None):
    """One launch of `dsbdd_pose_check` on device tensors.

    x [N,3] float32 (Angstrom) and lig_mask [N] sorted sample ids as the samplers return them; `atom_type_or_radii` [N]:
    a floating tensor of van-der-Waals radii, or integer class ids of `info["atom_decoder"]` (`info`: a dataset name, its
    dict, or the decoder list).  `pockets`: a `PocketAtoms` (uploaded before), or a list of (xyz, radii) host arrays, one
    per group.  `mol_group` [B]: the group of every molecule (host integers or a device tensor, any order); default:
    molecule b uses group b when there are B groups, group 0 when there is one.  `batch` keeps molecules without atoms
    in the list.  -> PoseStats of device tensors."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.HipLibraryError("pose_check needs device tensors (HIP path; no CPU fallback)")
    tol, contact = _check_thresholds(tol, contact)
    lib = _lib.load()
    dev = x.device
    if not isinstance(pockets, PocketAtoms):
        pockets = PocketAtoms.upload(pockets, dev)
    x = x.detach().to(torch.float32).reshape(-1, 3).contiguous()
    N = int(x.shape[0])
    v = atom_type_or_radii
    if torch.is_tensor(v) and v.is_floating_point():
        radii = v.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    elif not torch.is_tensor(v) and np.asarray(v).dtype.kind == "f":
        radii = torch.as_tensor(np.asarray(v, np.float32).reshape(-1), device=dev)
    else:
        if info is None:
            raise ValueError("integer atom types need `info` (the dataset whose atom decoder they index)")
        if isinstance(info, str):
            from .chem_tables import dataset_info
            info = dataset_info(info)
        table = torch.as_tensor(radius_table(info["atom_decoder"] if isinstance(info, dict) else list(info)), device=dev)
        radii = table[torch.as_tensor(v, device=dev).to(torch.int64).reshape(-1)].contiguous()
    if radii.shape[0] != N or lig_mask.shape[0] != N:
        raise ValueError(f"{N} coordinates, {radii.shape[0]} radii / types, {lig_mask.shape[0]} mask entries")
    B = _pairs._n_molecules(lig_mask, batch)
    off = _pairs.mol_offsets(lig_mask, B, dev)
    G = pockets.n_groups
    groups = _pairs.device_groups(mol_group, B, G, dev)
    i32 = dict(dtype=torch.int32, device=dev)
    out = PoseStats(torch.zeros((N, ATOM_OUT), **i32), torch.zeros((B, MOL_OUT), **i32), off, x, tol, contact)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.dsbdd_pose_check(stream, _ptr(x), _ptr(radii), off.data_ptr(), B, _ptr(groups), _ptr(pockets.x), _ptr(pockets.r),
                              pockets.group_off.data_ptr(), G, tol, contact, _ptr(out.atom), _ptr(out.mol))
    _lib.check(rc, "dsbdd_pose_check")
    return out


def as_ligands(molecules):
    """An SDF path, or a list of `Molecule` objects / (xyz, elements) pairs -> list of (xyz, radii, kept indices), heavy
    atoms only.  Elements outside `VDW_RADII` are kept with `DEFAULT_RADIUS`."""
    if isinstance(molecules, (str, bytes)) or hasattr(molecules, "__fspath__"):
        from .ligand_io import read_sdf_molecules
        molecules = read_sdf_molecules(molecules)
    return [heavy_atoms(*((m.positions, m.symbols) if hasattr(m, "symbols") else m)) for m in molecules]


def _pack(ligands):
    """list of (xyz, radii, ...) -> (x [N,3] float32, r [N] float32, lig_mask [N] int64) on the host."""
    x, mask, _ = _pairs.pack_ligands(ligands)
    r = np.concatenate([np.asarray(l[1], np.float32).reshape(-1) for l in ligands]) if ligands else np.zeros(0, np.float32)
    return x, r, mask


def check_molecules(molecules, pockets, mol_group=None, device="cuda", tol=CLASH_TOLERANCE, contact=CONTACT_CUTOFF):
    """Pose records of written molecules (`as_ligands` forms) against `pockets` (a `PocketAtoms` or a list of (xyz, radii)):
    upload, one launch.  -> list of `MolPose`."""
    ligands = as_ligands(molecules)
    x, r, mask = _pack(ligands)
    dev = pockets.x.device if isinstance(pockets, PocketAtoms) else torch.device(device)
    st = pose_check(torch.as_tensor(x, device=dev), torch.as_tensor(r, device=dev), torch.as_tensor(mask, device=dev), pockets,
                    mol_group, batch=len(ligands), tol=tol, contact=contact)
    return st.molecules()


# ---- the host restatement (specification and test oracle) ---------------------------------------------------------------
def _pose_check_host(lig_x, lig_r, mol_off, mol_group, poc_x, poc_r, group_off, tol=CLASH_TOLERANCE, contact=CONTACT_CUTOFF):
    """`dsbdd_pose_check` in numpy: the same arguments, the same two outputs bit for bit (PoseStats of arrays).  float32
    throughout, one rounding per operation, in the kernel's order."""
    tol, contact = _check_thresholds(tol, contact)
    x = np.asarray(_np(lig_x), np.float32).reshape(-1, 3)
    r = np.asarray(_np(lig_r), np.float32).reshape(-1)
    q = np.asarray(_np(poc_x), np.float32).reshape(-1, 3)
    qr = np.asarray(_np(poc_r), np.float32).reshape(-1)
    off = np.asarray(_np(mol_off), np.int64).reshape(-1)
    goff = np.asarray(_np(group_off), np.int64).reshape(-1)
    B, G = len(off) - 1, len(goff) - 1
    if off[0] < 0 or np.any(np.diff(off) < 0) or off[-1] != len(x) or len(r) != len(x):
        raise ValueError("mol_off must ascend to the number of ligand rows")
    if goff[0] < 0 or np.any(np.diff(goff) < 0) or goff[-1] != len(q) or len(qr) != len(q):
        raise ValueError("group_off must ascend to the number of pocket rows")
    groups = _checked_groups(mol_group, B, G)
    tol32, contact32, inf = np.float32(tol), np.float32(contact), np.float32(np.inf)
    atom = np.zeros((len(x), ATOM_OUT), np.int32)
    atom[:, A_NEAREST], atom[:, A_DIST_BITS] = -1, _INF_BITS
    mol = np.zeros((B, MOL_OUT), np.int32)
    for b in range(B):
        lo, hi = int(off[b]), int(off[b + 1])
        glo, ghi = int(goff[groups[b]]), int(goff[groups[b] + 1])
        p, pr, t, tr = x[lo:hi], r[lo:hi], q[glo:ghi], qr[glo:ghi]
        best = np.full(hi - lo, inf, np.float32)
        if hi > lo and ghi > glo:
            with np.errstate(invalid="ignore", over="ignore"):
                dx = p[:, None, 0] - t[None, :, 0]
                dy = p[:, None, 1] - t[None, :, 1]
                dz = p[:, None, 2] - t[None, :, 2]
                d = np.sqrt((dx * dx + dy * dy) + dz * dz)
                limit = (pr[:, None] + tr[None, :]) - tol32
                atom[lo:hi, A_CLASH] = (d < limit).sum(1)
                atom[lo:hi, A_CONTACT] = (d < contact32).sum(1)
                dm = np.where(d < inf, d, inf)                      # NaN and +inf never are "the nearest"
            assert d.dtype == np.float32 and limit.dtype == np.float32
            best = dm.min(1)
            atom[lo:hi, A_NEAREST] = np.where(best < inf, dm.argmin(1), -1)      # argmin: the first of equal distances
            atom[lo:hi, A_DIST_BITS] = best.view(np.int32)
        mol[b] = _totals(atom[lo:hi], np.isfinite(p).all(1))
    return PoseStats(atom, mol, off.astype(np.int32), x, tol, contact)


def _check_molecules_host(molecules, pockets, mol_group=None, tol=CLASH_TOLERANCE, contact=CONTACT_CUTOFF):
    """`check_molecules` through `_pose_check_host` (tests): `pockets` a list of (xyz, radii).  -> PoseStats of arrays."""
    ligands = as_ligands(molecules)
    x, r, mask = _pack(ligands)
    sizes = np.bincount(mask, minlength=len(ligands))
    off = np.concatenate([[0], np.cumsum(sizes)])
    px = [np.asarray(p[0], np.float32).reshape(-1, 3) for p in pockets]
    goff = np.concatenate([[0], np.cumsum([len(a) for a in px])])
    if mol_group is None:
        mol_group = _default_groups(len(ligands), len(px))
    return _pose_check_host(x, r, off, mol_group, np.concatenate(px) if px else np.zeros((0, 3), np.float32),
                            np.concatenate([np.asarray(p[1], np.float32).reshape(-1) for p in pockets]) if px
                            else np.zeros(0, np.float32), goff, tol, contact)


# ---- acceptance filter -----------------------------------------------------------------------------------------------------
def pose_filter(max_clash_pairs=0, min_contact_fraction=None):
    """Predicate on a `Molecule` that carries a `pose` attribute (the samplers' `pose=` option): passes when the pose is
    finite, has at most `max_clash_pairs` clash pairs and, when `min_contact_fraction` is given, at least that share of
    its atoms in contact with the pocket.  None (no molecule) does not pass; a molecule without `pose` raises."""
    def passes(m):
        if m is None:
            return False
        pose = getattr(m, "pose", None)
        if pose is None:
            raise ValueError("pose_filter: the molecule carries no pose record (sample with pose=True)")
        if pose.nonfinite or pose.clash_pairs > max_clash_pairs:
            return False
        if min_contact_fraction is not None:
            return pose.n_atoms > 0 and pose.contact_atoms >= min_contact_fraction * pose.n_atoms
        return True
    return passes


def summarize_poses(molecules):
    """{'n', 'mean_clash_pairs', 'share_clash_free'} of the molecules that carry a pose record."""
    poses = [m.pose for m in molecules if m is not None and getattr(m, "pose", None) is not None]
    n = len(poses)
    return {"n": n, "mean_clash_pairs": float(np.mean([p.clash_pairs for p in poses])) if n else 0.0,
            "share_clash_free": float(np.mean([p.clash_pairs == 0 for p in poses])) if n else 0.0}


# ---- command line --------------------------------------------------------------------------------------------------------
CSV_COLUMNS = ("n_atoms", "clash_pairs", "clash_atoms", "contact_pairs", "contact_atoms", "nonfinite", "min_distance")


def write_csv(path, rows):
    """rows: (source, index, MolPose or its dict); `path` None writes to stdout."""
    _pairs.write_csv(path, rows, CSV_COLUMNS)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Clash and contact counts of written ligands against a protein (one row per molecule)")
    _pairs.add_complex_arguments(p)
    p.add_argument("--tol", type=float, default=CLASH_TOLERANCE)
    p.add_argument("--contact", type=float, default=CONTACT_CUTOFF)
    a = _pairs.parse_complex_arguments(p, argv)
    try:
        _check_thresholds(a.tol, a.contact)
    except ValueError as exc:
        p.error(str(exc))
    return a


def main(argv=None):
    a = parse_args(argv)
    print(POSE_COVERAGE, file=sys.stderr)
    pockets = PocketAtoms.upload([pocket_atoms(select_residues(a.pdbfile, a.scope, a.ref_ligand))], torch.device(a.device))
    rows = []
    for path in a.sdf:
        rows += [(path, k, rec) for k, rec in enumerate(check_molecules(path, pockets, tol=a.tol, contact=a.contact))]
    write_csv(a.out, rows)
    return rows


if __name__ == "__main__":
    main()
