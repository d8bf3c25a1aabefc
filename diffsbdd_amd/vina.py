"""Vina-type interaction score of ligand poses on the device, with atom typing.

Two launches on the tensors the samplers return (csrc/vina_score.h): `dsbdd_vina_type` types the ligand heavy atoms from
the bond-order matrices `molecules.bond_orders` leaves on the device (hydrophobic, donor, acceptor, rotors), then
`dsbdd_vina_score` sums the five pair terms of Trott & Olson, J. Comput. Chem. 31 (2010) 455 over the ligand-pocket heavy
atom pairs within 8 A.  Nothing crosses the host between the sampler and the score.

Definitions (`_vina_type_host` and `_vina_score_host` restate them in numpy, the second in float64; they are the
specification the kernels are tested against, not a fallback -- the public entry points refuse CPU tensors):

    pair counts iff r < CUTOFF (8.0 A, strict), r the float32 distance of `pose.pose_check`
    d           = r - R_i - R_j                                     R: XS_RADII by class
    gauss1      = exp(-(d / 0.5)^2)             gauss2 = exp(-((d - 3) / 2)^2)
    repulsion   = d^2 if d < 0, else 0
    hydrophobic = 1 if d <= 0.5, 1.5 - d if 0.5 < d < 1.5, else 0   both atoms hydrophobic
    hbond       = 1 if d <= -0.7, -d / 0.7 if -0.7 < d < 0, else 0  one atom donor, the other acceptor; once per pair
    inter       = sum_k WEIGHTS[k] T_k                              T_k: the sum of term k over the molecule's pairs
    score       = inter / (1 + ROT_WEIGHT N_rot)                    kcal/mol

Atom code (one int32): bits 0-3 the class (CLASSES), bit 4 hydrophobic, bit 5 donor, bit 6 acceptor.  Ligand typing, with
s = the sum of bond orders at the atom and a heteroatom neighbour = any neighbour that is not carbon (untyped included):
C hydrophobic iff it has no heteroatom neighbour; F, Cl, Br, I hydrophobic; N donor iff s < 3, acceptor iff s = 3 with a
bond of order >= 2; O acceptor, donor iff s < 2; S, P none; metal donor.  N_rot: single bonds outside rings whose two ends
both have heavy degree >= 2.  Pocket atoms: RESIDUE_TABLE (the 20 standard residues typed by the same rules from their
covalent topology), by element outside it.

  python -m diffsbdd_amd.vina --pdbfile P.pdb --sdf L.sdf [L2.sdf ...] [--scope protein|pocket --ref_ligand ...]
                              [--bonds distance|file] [--dataset crossdock] [--out scores.csv]
"""
from __future__ import annotations

import argparse
import ctypes
import sys
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, _pairs
from ._pairs import HYDROGENS, _n_molecules, _np, _ptr, _symbol, select_residues

# ---- constants -------------------------------------------------------------------------------------------------------------
CLASSES = ("", "C", "N", "O", "P", "S", "F", "Cl", "Br", "I", "metal")           # class id = index; 0 = untyped
C_NONE, C_C, C_N, C_O, C_P, C_S, C_F, C_CL, C_BR, C_I, C_METAL = range(11)
CLASS_MASK, HYDROPHOBIC, DONOR, ACCEPTOR = 15, 16, 32, 64
METALS = ("Zn", "Mg", "Ca", "Mn", "Fe", "Co", "Ni", "Cu")
WATER = ("HOH", "WAT")
XS_RADII = {"C": 1.9, "N": 1.8, "O": 1.7, "P": 2.1, "S": 2.0, "F": 1.5, "Cl": 1.8, "Br": 2.0, "I": 2.2, "metal": 1.2}
WEIGHTS = (-0.035579, -0.005156, 0.840245, -0.035069, -0.587439)                # gauss1, gauss2, repulsion, hydrophobic, hbond
ROT_WEIGHT = 0.05846
CUTOFF = 8.0
TERMS = ("gauss1", "gauss2", "repulsion", "hydrophobic", "hbond")
TILE = 1024                           # pocket atoms per LDS tile of vina_score_kernel (kPairTile, csrc/pair_sweep.h)
ATOM_OUT, MOL_OUT, MOL_INT = 5, 8, 4  # columns of the kernels' outputs
M_INTER, M_SCORE = 5, 6
I_TYPED, I_UNTYPED, I_ROT = 0, 1, 2
EPS32 = 2.0 ** -24
_RADIUS = np.asarray([0.0] + [XS_RADII[c] for c in CLASSES[1:]], np.float64)
_LIPSCHITZ = (1.716, 0.429, None, 1.0, 1.0 / 0.7)                                # of the five terms in d (repulsion: 2 |d| + 2 dd)

VINA_COVERAGE = (
    "Vina-type score: PRESENT = the five intermolecular terms of Trott & Olson (J. Comput. Chem. 31, 2010, 455) -- gauss1, "
    "gauss2, repulsion, hydrophobic, hbond -- summed by one GPU kernel over ligand-pocket heavy-atom pairs closer than 8 A, "
    "their weighted sum `inter` and score = inter / (1 + 0.05846 N_rot) in kcal/mol, per molecule and per atom, after one "
    "GPU typing kernel on the bond-order matrices; "
    "DEFINED AS = surface distance d = r - R_i - R_j with the radii C 1.9, N 1.8, O 1.7, P 2.1, S 2.0, F 1.5, Cl 1.8, "
    "Br 2.0, I 2.2, metal 1.2 A; carbon hydrophobic iff bonded to no heteroatom, halogens hydrophobic; N donor iff it has an "
    "implicit hydrogen (sum of bond orders < 3), acceptor iff that sum is 3 with a double or triple bond; O acceptor, donor "
    "iff its sum of bond orders < 2; N_rot = single bonds outside rings between atoms of heavy degree >= 2 (amide and "
    "conjugated bonds are NOT excluded); protein atoms typed from a table of the 20 standard residues (HIS ND1/NE2 donor "
    "and acceptor: tautomer unknown), by element alone outside it, B, Se and other elements untyped (no pair term); "
    "NOT = the output of smina or AutoDock Vina and NOT comparable with published docking scores: no hydrogens, no "
    "protonation states or charges, no PDBQT typing, no intramolecular term, no search or pose optimisation -- it scores the "
    "pose as given, against a rigid protein, and only the residues given (an atom outside the selection is not seen); "
    "ligand bonds are perceived from distances (the tables of the samplers) unless given (--bonds file); "
    "ABSENT = the external docking binaries (refused).")


def class_of(symbol):
    """Class id of an element symbol; 0 (untyped) for B, Se and every element outside CLASSES and METALS."""
    s = _symbol(symbol)
    if s in METALS:
        return C_METAL
    return CLASSES.index(s) if s in CLASSES[1:10] else C_NONE


def class_table(atom_decoder):
    """int32 [n_types]: the class of every type of a sampler's atom decoder (the kernels' `class_elem`)."""
    return np.asarray([class_of(s) for s in atom_decoder], np.int32)


def _decoder(info):
    if isinstance(info, str):
        from .chem_tables import dataset_info
        info = dataset_info(info)
    return list(info["atom_decoder"] if isinstance(info, dict) else info), info


# ---- typing: the host restatement (specification and test oracle) -----------------------------------------------------------
def _bond_in_ring(nbrs, a, c):
    """Are a and c connected when the bond between them is left out?"""
    seen, front = {a}, [a]
    while front:
        nxt = []
        for u in front:
            for v in nbrs[u]:
                if u == a and v == c:
                    continue
                if v == c:
                    return True
                if v not in seen:
                    seen.add(v)
                    nxt.append(v)
        front = nxt
    return False


def type_graph(classes, sym):
    """Codes and rotors of one molecule: `classes` int [n] class ids, `sym` int [n,n] symmetric bond orders (values outside
    1..3 are no bond).  -> (codes int32 [n], n_rot)."""
    classes = np.asarray(classes, np.int64).reshape(-1)
    n = len(classes)
    sym = np.asarray(sym, np.int64).reshape(n, n)
    sym = np.where((sym >= 1) & (sym <= 3), sym, 0)
    classes = np.where((classes >= 0) & (classes <= C_METAL), classes, C_NONE)
    bonded = sym > 0
    s, top, deg = sym.sum(1), sym.max(1) if n else sym.sum(1), bonded.sum(1)
    hetero = (bonded & (classes != C_C)[None, :]).any(1)
    codes = classes.astype(np.int32).copy()
    for a in range(n):
        k = classes[a]
        if k == C_C:
            codes[a] |= 0 if hetero[a] else HYDROPHOBIC
        elif k in (C_F, C_CL, C_BR, C_I):
            codes[a] |= HYDROPHOBIC
        elif k == C_N:
            codes[a] |= (DONOR if s[a] < 3 else 0) | (ACCEPTOR if s[a] == 3 and top[a] >= 2 else 0)
        elif k == C_O:
            codes[a] |= ACCEPTOR | (DONOR if s[a] < 2 else 0)
        elif k == C_METAL:
            codes[a] |= DONOR
    nbrs = [np.nonzero(bonded[a])[0].tolist() for a in range(n)]
    n_rot = 0
    for a in range(n):
        for c in nbrs[a]:
            if c < a and sym[a, c] == 1 and deg[a] >= 2 and deg[c] >= 2 and not _bond_in_ring(nbrs, a, c):
                n_rot += 1
    return codes, n_rot


def orders_from_bonds(n, bonds, n_max=None):
    """int8 [n_max, n_max] strictly lower triangular (what `dsbdd_bond_orders` writes) of a bond list (i, j, order)."""
    n_max = max(n, 1) if n_max is None else n_max
    o = np.zeros((n_max, n_max), np.int8)
    for i, j, order in bonds:
        i, j = (int(i), int(j)) if i > j else (int(j), int(i))
        if i == j or not (0 <= j and i < n):
            raise ValueError(f"bond ({i}, {j}) of a molecule with {n} atoms")
        if i < n_max:
            o[i, j] = order
    return o


def _vina_type_host(order, atom_type, mol_off, class_elem, fill=0):
    """`dsbdd_vina_type` in numpy (integers): order int8 [B, n_max, n_max], atom_type [N], mol_off [B+1], class_elem
    [n_types] -> (lig_code int32 [N], mol_int int32 [B, 4]).  Rows that belong to no valid molecule keep `fill`."""
    order = np.asarray(_np(order))
    B, n_max = order.shape[0], order.shape[1]
    at = np.asarray(_np(atom_type), np.int64).reshape(-1)
    off = np.asarray(_np(mol_off), np.int64).reshape(-1)
    table = np.asarray(_np(class_elem), np.int64).reshape(-1)
    if len(off) != B + 1:
        raise ValueError(f"{len(off)} offsets for {B} molecules")
    code = np.full(len(at), fill, np.int32)
    mol = np.zeros((B, MOL_INT), np.int32)
    n_total = off[B]
    for b in range(B):
        lo, hi = int(off[b]), int(off[b + 1])
        size = hi - lo if (lo >= 0 and hi >= lo and hi <= n_total) else 0
        n = min(size, n_max)
        t = at[lo:lo + n]
        ok = (t >= 0) & (t < len(table))
        classes = np.where(ok, table[np.where(ok, t, 0)], C_NONE)
        classes = np.where((classes >= 0) & (classes <= C_METAL), classes, C_NONE)
        low = np.tril(order[b, :n, :n].astype(np.int64), -1)
        codes, n_rot = type_graph(classes, low + low.T)
        code[lo:lo + n] = codes
        code[lo + n:lo + size] = 0
        mol[b] = (int((classes != C_NONE).sum()), int((classes == C_NONE).sum()), n_rot, 0)
    return code, mol


# ---- the residue table --------------------------------------------------------------------------------------------------------
_BACKBONE = (("N", "CA", 1), ("CA", "C", 1), ("C", "O", 2))
_SIDE_CHAINS = {        # heavy-atom bonds beyond the backbone; a carboxylate is written with two double bonds (no hydrogen on either O)
    "GLY": (),
    "ALA": (("CA", "CB", 1),),
    "SER": (("CA", "CB", 1), ("CB", "OG", 1)),
    "CYS": (("CA", "CB", 1), ("CB", "SG", 1)),
    "VAL": (("CA", "CB", 1), ("CB", "CG1", 1), ("CB", "CG2", 1)),
    "THR": (("CA", "CB", 1), ("CB", "OG1", 1), ("CB", "CG2", 1)),
    "PRO": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "CD", 1), ("CD", "N", 1)),
    "ILE": (("CA", "CB", 1), ("CB", "CG1", 1), ("CB", "CG2", 1), ("CG1", "CD1", 1)),
    "LEU": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "CD1", 1), ("CG", "CD2", 1)),
    "ASP": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "OD1", 2), ("CG", "OD2", 2)),
    "ASN": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "OD1", 2), ("CG", "ND2", 1)),
    "GLU": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "CD", 1), ("CD", "OE1", 2), ("CD", "OE2", 2)),
    "GLN": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "CD", 1), ("CD", "OE1", 2), ("CD", "NE2", 1)),
    "LYS": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "CD", 1), ("CD", "CE", 1), ("CE", "NZ", 1)),
    "MET": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "SD", 1), ("SD", "CE", 1)),
    "HIS": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "ND1", 1), ("CG", "CD2", 2), ("ND1", "CE1", 2), ("CD2", "NE2", 1),
            ("CE1", "NE2", 1)),
    "PHE": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "CD1", 2), ("CG", "CD2", 1), ("CD1", "CE1", 1), ("CD2", "CE2", 2),
            ("CE1", "CZ", 2), ("CE2", "CZ", 1)),
    "ARG": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "CD", 1), ("CD", "NE", 1), ("NE", "CZ", 1), ("CZ", "NH1", 2),
            ("CZ", "NH2", 1)),
    "TYR": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "CD1", 2), ("CG", "CD2", 1), ("CD1", "CE1", 1), ("CD2", "CE2", 2),
            ("CE1", "CZ", 2), ("CE2", "CZ", 1), ("CZ", "OH", 1)),
    "TRP": (("CA", "CB", 1), ("CB", "CG", 1), ("CG", "CD1", 2), ("CG", "CD2", 1), ("CD1", "NE1", 1), ("NE1", "CE2", 1),
            ("CD2", "CE2", 2), ("CD2", "CE3", 1), ("CE2", "CZ2", 1), ("CE3", "CZ3", 2), ("CZ2", "CH2", 2), ("CZ3", "CH2", 1)),
}
# the tautomer of a histidine is not known from heavy atoms: both ring nitrogens may give and take a hydrogen bond
_OVERRIDES = {("HIS", "ND1"): C_N | DONOR | ACCEPTOR, ("HIS", "NE2"): C_N | DONOR | ACCEPTOR}


def _residue_table():
    """{resname: {atom name: code}} from the covalent topology, by `type_graph`: the residue inside a chain (its N bonded
    to the carbonyl carbon before it, its C to the nitrogen after it), element = first letter of the atom name."""
    table = {}
    for res, side in _SIDE_CHAINS.items():
        names = []
        for i, j, _ in _BACKBONE + side:
            names += [x for x in (i, j) if x not in names]
        index = {x: k for k, x in enumerate(names)}
        n = len(names)
        classes = [class_of(x[0]) for x in names] + [C_C, C_N]                     # + the neighbours along the chain
        sym = np.zeros((n + 2, n + 2), np.int64)
        for i, j, o in _BACKBONE + side + (("N", n, 1), ("C", n + 1, 1)):
            a, c = index.get(i, i), index.get(j, j)
            sym[a, c] = sym[c, a] = o
        codes, _ = type_graph(classes, sym)
        table[res] = {x: int(_OVERRIDES.get((res, x), codes[index[x]])) for x in names}
    return table


RESIDUE_TABLE = _residue_table()
OXT_CODE = C_O | ACCEPTOR             # the chain's last carboxylate oxygen, in every residue
_ELEMENT_FLAGS = {C_O: ACCEPTOR, C_F: HYDROPHOBIC, C_CL: HYDROPHOBIC, C_BR: HYDROPHOBIC, C_I: HYDROPHOBIC, C_METAL: DONOR}


def code_by_element(symbol):
    """The code of an atom typed by its element alone: C not hydrophobic, N no flags, O acceptor, halogens hydrophobic,
    metals donor, everything else untyped."""
    k = class_of(symbol)
    return k | _ELEMENT_FLAGS.get(k, 0)


@dataclass
class TypedPocket:
    """Heavy atoms of a residue list on the host: x float32 [M,3], code int32 [M], and how many of them were typed by
    element alone (`untemplated`: residue or atom name outside RESIDUE_TABLE)."""
    x: np.ndarray
    code: np.ndarray
    untemplated: int = 0


def type_pocket(residues):
    """Residue dicts of `pocket.read_pdb_residues` -> TypedPocket: heavy atoms in file order, water and hydrogens dropped."""
    xyz, codes, untemplated = [], [], 0
    for res in residues:
        name = str(res["resname"]).strip().upper()
        if name in WATER:
            continue
        entry = RESIDUE_TABLE.get(name)
        for atom, elem, pos in res["atoms"]:
            if _symbol(elem) in HYDROGENS:
                continue
            atom = str(atom).strip()
            if entry is not None and atom in entry:
                code = entry[atom]
            elif entry is not None and atom == "OXT":
                code = OXT_CODE
            else:
                code = code_by_element(elem)
                untemplated += 1
            xyz.append(pos)
            codes.append(code)
    return TypedPocket(np.asarray(xyz, np.float32).reshape(-1, 3), np.asarray(codes, np.int32), untemplated)


class VinaPocket(_pairs.PocketGroups):
    """`_pairs.PocketGroups` with the atom codes code [M] int32 and, per group, how many atoms were typed by element alone
    (`untemplated`)."""
    COLUMN, DTYPE, WHAT = "code", np.int32, "code"

    def __init__(self, x, code, offsets, untemplated=()):
        super().__init__(x, code, offsets)
        self.untemplated = list(untemplated)

    @classmethod
    def upload(cls, pockets, device):
        """`pockets`: list of `TypedPocket` or (xyz [m,3], code [m]) host arrays, one per group."""
        pockets = list(pockets)
        return super().upload([(p.x, p.code) if isinstance(p, TypedPocket) else p for p in pockets], device,
                              [getattr(p, "untemplated", 0) for p in pockets])

    @classmethod
    def concat(cls, parts):
        parts = list(parts)
        return super().concat(parts, sum((p.untemplated for p in parts), []))


# ---- results -------------------------------------------------------------------------------------------------------------------
def _score_of(terms, n_rot):
    """(inter, score) in float64 of float terms [..., 5] and rotor counts."""
    terms = np.asarray(terms, np.float64)
    inter = (terms * np.asarray(WEIGHTS, np.float64)).sum(-1)
    return inter, inter / (1.0 + ROT_WEIGHT * np.maximum(np.asarray(n_rot, np.float64), 0.0))


@dataclass
class MolVina:
    """The score record of one molecule (host arrays): what the samplers attach to a `Molecule` as `m.vina`."""
    mol: np.ndarray          # float32 [8]: the five term sums, inter, score, 0
    ints: np.ndarray         # int32 [4]: typed atoms, untyped atoms, N_rot, 0
    atom: np.ndarray         # float32 [n, 5]: the unweighted terms of every atom
    code: np.ndarray         # int32 [n]: atom codes
    nonfinite: int = 0

    terms = property(lambda self: self.mol[:ATOM_OUT])
    inter = property(lambda self: float(self.mol[M_INTER]))
    score = property(lambda self: float(self.mol[M_SCORE]))
    n_rot = property(lambda self: int(self.ints[I_ROT]))
    untyped = property(lambda self: int(self.ints[I_UNTYPED]))
    n_atoms = property(lambda self: len(self.code))

    def subset(self, keep, bonds=()):
        """The record of the atoms `keep` alone (a fragment with the bonds `bonds`, renumbered): per-atom rows carried
        along, sums recomputed from them in float64, rotors counted on the fragment's own graph."""
        keep = np.asarray(keep, np.int64).reshape(-1)
        atom, code = self.atom[keep].copy(), self.code[keep].copy()
        low = orders_from_bonds(len(keep), bonds).astype(np.int64)
        _, n_rot = type_graph(code & CLASS_MASK, low + low.T)
        typed = int(((code & CLASS_MASK) != 0).sum())
        mol = np.zeros(MOL_OUT, np.float32)
        mol[:ATOM_OUT] = atom.astype(np.float64).sum(0)
        mol[M_INTER], mol[M_SCORE] = _score_of(atom.astype(np.float64).sum(0), n_rot)
        if self.nonfinite:
            mol[:M_SCORE + 1] = np.nan
        return MolVina(mol, np.asarray([typed, len(keep) - typed, n_rot, 0], np.int32), atom, code, self.nonfinite)

    def as_dict(self):
        out = {"n_atoms": self.n_atoms, "untyped": self.untyped, "n_rot": self.n_rot, "nonfinite": int(self.nonfinite)}
        out.update({t: float(v) for t, v in zip(TERMS, self.terms)})
        out.update(inter=self.inter, score=self.score)
        return out


@dataclass
class VinaScores:
    """The outputs of the two kernels (device tensors from `vina_score`, numpy arrays from `_vina_score_host`)."""
    atom: object             # float [N, 5]
    mol: object              # float [B, 8]
    mol_int: object          # int32 [B, 4]
    flag: object             # int32 [B]
    lig_code: object         # int32 [N]
    mol_off: object          # int32 [B + 1]

    terms = property(lambda self: self.mol[:, :ATOM_OUT])
    inter = property(lambda self: self.mol[:, M_INTER])
    score = property(lambda self: self.mol[:, M_SCORE])
    n_rot = property(lambda self: self.mol_int[:, I_ROT])
    untyped = property(lambda self: self.mol_int[:, I_UNTYPED])
    nonfinite = property(lambda self: self.flag)

    def molecules(self):
        """One `MolVina` per molecule, in order (one copy of each tensor to the host)."""
        atom, mol, ints, flag, code, off = (_np(v) for v in (self.atom, self.mol, self.mol_int, self.flag, self.lig_code,
                                                             self.mol_off))
        return [MolVina(mol[b].copy(), ints[b].copy(), atom[off[b]:off[b + 1]].copy(), code[off[b]:off[b + 1]].copy(),
                        int(flag[b])) for b in range(len(mol))]


# ---- the device path ---------------------------------------------------------------------------------------------------------
def type_ligands(x, atom_type, lig_mask, info, orders=None, batch=None):
    """Atom codes and rotor counts of a batch on the device: `molecules.bond_orders` (unless `orders` int8 [B, n_max, n_max]
    is given, n_max <= 128) then one launch of `dsbdd_vina_type`.  x [N,3], atom_type [N] class ids of `info`'s atom
    decoder (`info`: a dataset name, its dict, or -- with `orders` -- the decoder list), lig_mask [N] sorted sample ids.
    A molecule longer than 128 atoms is typed as its first 128.  -> (lig_code int32 [N], mol_int int32 [B, 4] = typed atoms,
    untyped atoms, N_rot, 0, mol_off int32 [B+1])."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.HipLibraryError("type_ligands needs device tensors (HIP path; no CPU fallback)")
    lib = _lib.load()
    dev = x.device
    decoder, info = _decoder(info)
    x = x.detach().to(torch.float32).reshape(-1, 3).contiguous()
    N = int(x.shape[0])
    at = torch.as_tensor(atom_type, device=dev).to(torch.int32).reshape(-1).contiguous()
    lig_mask = torch.as_tensor(lig_mask, device=dev).reshape(-1)
    if at.shape[0] != N or lig_mask.shape[0] != N:
        raise ValueError(f"{N} coordinates, {at.shape[0]} types, {lig_mask.shape[0]} mask entries")
    B = _n_molecules(lig_mask, batch)
    off = _pairs.mol_offsets(lig_mask, B, dev)
    i32 = dict(dtype=torch.int32, device=dev)
    code, mol_int = torch.zeros(N, **i32), torch.zeros((B, MOL_INT), **i32)
    if B == 0:
        return code, mol_int, off
    if orders is None and N == 0:
        orders = torch.zeros((B, 1, 1), dtype=torch.int8, device=dev)
    if orders is None:
        if not isinstance(info, dict) or "bonds1" not in info:
            raise ValueError("bond perception needs the dataset (its name or dict), not the decoder alone")
        from .molecules import bond_orders
        orders, _ = bond_orders(x, at, lig_mask, info, batch=B)
        if orders.shape[1] > _lib.MOL_MAX_ATOMS:                    # the block of the first 128 atoms of every molecule
            orders = orders[:, :_lib.MOL_MAX_ATOMS, :_lib.MOL_MAX_ATOMS].contiguous()
    else:
        orders = torch.as_tensor(orders, device=dev).to(torch.int8).contiguous()
    if orders.dim() != 3 or orders.shape[0] != B or orders.shape[1] != orders.shape[2] or \
            not 1 <= orders.shape[1] <= _lib.MOL_MAX_ATOMS:
        raise ValueError(f"orders must be [{B}, n_max, n_max] with n_max in [1, {_lib.MOL_MAX_ATOMS}], got {tuple(orders.shape)}")
    table = torch.as_tensor(class_table(decoder), device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.dsbdd_vina_type(stream, orders.data_ptr(), _ptr(at), off.data_ptr(), B, len(decoder), table.data_ptr(),
                             int(orders.shape[1]), _ptr(code), mol_int.data_ptr())
    _lib.check(rc, "dsbdd_vina_type")
    return code, mol_int, off


def vina_score(x, atom_type, lig_mask, pockets, info, mol_group=None, batch=None, orders=None):
    """The score of a batch on device tensors: bond orders (unless given), `dsbdd_vina_type`, `dsbdd_vina_score`; no
    read-back inside.  x, atom_type, lig_mask, info, orders, batch as for `type_ligands`; `pockets`: a `VinaPocket`
    (uploaded before) or a list of `TypedPocket` / (xyz, code) host arrays, one per group; `mol_group` [B] as for
    `pose.pose_check`.  -> VinaScores of device tensors."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.HipLibraryError("vina_score needs device tensors (HIP path; no CPU fallback)")
    lib = _lib.load()
    dev = x.device
    if not isinstance(pockets, VinaPocket):
        pockets = VinaPocket.upload(pockets, dev)
    x = x.detach().to(torch.float32).reshape(-1, 3).contiguous()
    N = int(x.shape[0])
    lig_mask = torch.as_tensor(lig_mask, device=dev).reshape(-1)
    B = _n_molecules(lig_mask, batch)
    G = pockets.n_groups
    groups = _pairs.device_groups(mol_group, B, G, dev)
    code, mol_int, off = type_ligands(x, atom_type, lig_mask, info, orders=orders, batch=B)
    f32 = dict(dtype=torch.float32, device=dev)
    out = VinaScores(torch.zeros((N, ATOM_OUT), **f32), torch.zeros((B, MOL_OUT), **f32), mol_int,
                     torch.zeros(B, dtype=torch.int32, device=dev), code, off)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.dsbdd_vina_score(stream, _ptr(x), _ptr(code), off.data_ptr(), B, _ptr(groups), _ptr(mol_int), _ptr(pockets.x),
                              _ptr(pockets.code), pockets.group_off.data_ptr(), G, _ptr(out.atom), _ptr(out.mol), _ptr(out.flag))
    _lib.check(rc, "dsbdd_vina_score")
    return out


# ---- written molecules -------------------------------------------------------------------------------------------------------
def read_sdf_records(path):
    """Every record of an SDF file -> list of (xyz float32 [n,3], element symbols, bonds [(i, j, order)], 0-based).  A
    small reader of its own: atom and bond blocks by the counts line's columns, with or without a version tag; bond type 4
    (aromatic) is refused -- the typing rules need Kekule orders."""
    out = []
    for k, rec in enumerate(_pairs.sdf_records(path)):
        if len(rec) < 4:
            raise ValueError(f"{path}: record {k} has no counts line")
        n_atoms, n_bonds = int(rec[3][0:3]), int(rec[3][3:6])
        if len(rec) < 4 + n_atoms + n_bonds:
            raise ValueError(f"{path}: record {k} announces {n_atoms} atoms and {n_bonds} bonds and holds {len(rec) - 4} lines")
        xyz = np.asarray([[float(l[0:10]), float(l[10:20]), float(l[20:30])] for l in rec[4:4 + n_atoms]],
                         np.float32).reshape(-1, 3)
        elements = [l[31:34].strip() for l in rec[4:4 + n_atoms]]
        bonds = []
        for l in rec[4 + n_atoms:4 + n_atoms + n_bonds]:
            i, j, o = int(l[0:3]) - 1, int(l[3:6]) - 1, int(l[6:9])
            if o not in (1, 2, 3):
                raise ValueError(f"{path}: record {k} has a bond of type {o}; orders 1, 2, 3 are read (write Kekule bonds)")
            bonds.append((i, j, o))
        out.append((xyz, elements, bonds))
    return out


def as_ligands(molecules):
    """An SDF path, or a list of `Molecule` objects / (xyz, elements[, bonds]) tuples -> list of (xyz float32 [n,3],
    elements, bonds) over heavy atoms: hydrogens and their bonds dropped, the rest renumbered."""
    if isinstance(molecules, (str, bytes)) or hasattr(molecules, "__fspath__"):
        molecules = read_sdf_records(molecules)
    out = []
    for m in molecules:
        xyz, elements, bonds = (m.positions, m.symbols, m.bonds) if hasattr(m, "symbols") else \
            (m[0], m[1], m[2] if len(m) > 2 else None)
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        if len(elements) != len(xyz):
            raise ValueError(f"{len(xyz)} coordinates for {len(elements)} elements")
        keep = [k for k, s in enumerate(elements) if _symbol(s) not in HYDROGENS]
        index = {a: k for k, a in enumerate(keep)}
        if bonds is not None:
            bonds = [(index[i], index[j], int(o)) for i, j, o in bonds if i in index and j in index]
        out.append((xyz[keep], [_symbol(elements[k]) for k in keep], bonds))
    return out


def score_molecules(molecules, pockets, info="crossdock", mol_group=None, device="cuda", bonds="distance"):
    """Score records of written molecules (`as_ligands` forms) against `pockets` (a `VinaPocket` or a list of typed
    pockets): upload, then the launches of `vina_score`.  bonds 'distance': perceived from the coordinates with the
    tables of the dataset `info`, as for generated molecules (every element must be in its decoder); 'file': the bond
    lists the molecules carry.  -> list of `MolVina`."""
    if bonds not in ("distance", "file"):
        raise ValueError("bonds must be 'distance' or 'file'")
    ligands = as_ligands(molecules)
    dev = pockets.x.device if isinstance(pockets, VinaPocket) else torch.device(device)
    if dev.type != "cuda":
        raise _lib.HipLibraryError("score_molecules needs a HIP device (no CPU fallback)")
    x, mask, sizes = _pairs.pack_ligands(ligands)
    symbols = [s for l in ligands for s in l[1]]
    orders = None
    if bonds == "file":
        if any(l[2] is None for l in ligands):
            raise ValueError("bonds='file' needs molecules that carry a bond list")
        decoder = sorted(set(symbols)) or ["C"]
        if max(sizes, default=0) > _lib.MOL_MAX_ATOMS:
            raise ValueError(f"a molecule has more than {_lib.MOL_MAX_ATOMS} heavy atoms")
        n_max = max(max(sizes, default=0), 1)
        orders = np.stack([orders_from_bonds(n, l[2], n_max) for n, l in zip(sizes, ligands)]) if ligands else \
            np.zeros((0, 1, 1), np.int8)
        info = decoder
    else:
        decoder, info = _decoder(info)
    missing = sorted(set(symbols) - set(decoder))
    if missing:
        raise ValueError(f"elements {missing} are outside the atom decoder of the dataset: bonds cannot be perceived from "
                         "distances (bonds='file' reads them from the molecules)")
    at = np.asarray([decoder.index(s) for s in symbols], np.int64)
    st = vina_score(torch.as_tensor(x, device=dev), torch.as_tensor(at, device=dev), torch.as_tensor(mask, device=dev), pockets,
                    info, mol_group, batch=len(ligands), orders=None if orders is None else torch.as_tensor(orders, device=dev))
    return st.molecules()


def objective(generator, residues, bonds="distance"):
    """A callable on a `Molecule` for `LigandGenerator.optimize_ligands`, larger = better: minus the score of the molecule
    against the heavy atoms of `residues` (typed and uploaded once).  A molecule that carries `m.vina` (sampled with
    vina=True against the same residues) is not scored again; a pose that is not finite ranks last."""
    pockets = VinaPocket.upload([type_pocket(residues)], generator.device)

    def value(m):
        rec = getattr(m, "vina", None)
        if rec is None:
            rec, = score_molecules([m], pockets, generator.dataset_info, bonds=bonds)
        return -rec.score if np.isfinite(rec.score) else float("-inf")
    return value


# ---- the float64 restatement (specification and test oracle) -------------------------------------------------------------------
def pair_terms(d, hydrophobic=True, hbond=True):
    """The five terms at surface distances `d` (any shape) in d's dtype -> [..., 5]."""
    d = np.asarray(d)
    one, zero = d.dtype.type(1), d.dtype.type(0)
    half, c07, c15, c3 = d.dtype.type(0.5), d.dtype.type(0.7), d.dtype.type(1.5), d.dtype.type(3)
    a, c = d / half, (d - c3) / d.dtype.type(2)
    out = np.stack([np.exp(-(a * a)), np.exp(-(c * c)), np.where(d < 0, d * d, zero),
                    np.where(d <= half, one, np.where(d < c15, c15 - d, zero)),
                    np.where(d <= -c07, one, np.where(d < 0, -d / c07, zero))], -1)
    out[..., 3] = np.where(hydrophobic, out[..., 3], zero)
    out[..., 4] = np.where(hbond, out[..., 4], zero)
    return out


def _molecule_pairs(x, code, q, qcode, dtype):
    """Dense pair quantities of one molecule against one group: r [n, m] (dtype), counted, hydrophobic and hbond masks."""
    code, qcode = np.asarray(code, np.int64), np.asarray(qcode, np.int64)
    ki, kj = code & CLASS_MASK, qcode & CLASS_MASK
    ki, kj = np.where(ki <= C_METAL, ki, 0), np.where(kj <= C_METAL, kj, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        xd, qd = x.astype(dtype), q.astype(dtype)
        dx, dy, dz = (xd[:, None, k] - qd[None, :, k] for k in range(3))
        r = np.sqrt((dx * dx + dy * dy) + dz * dz)
        # the pair counts iff the FLOAT32 distance is below the cutoff, whatever dtype evaluates the terms
        x32, q32 = x.astype(np.float32), q.astype(np.float32)
        e = [x32[:, None, k] - q32[None, :, k] for k in range(3)]
        r32 = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        counted = (r32 < np.float32(CUTOFF)) & (ki[:, None] != 0) & (kj[None, :] != 0)
    hyd = ((code[:, None] & qcode[None, :] & HYDROPHOBIC) != 0)
    hb = (((code[:, None] & DONOR) != 0) & ((qcode[None, :] & ACCEPTOR) != 0)) | \
         (((code[:, None] & ACCEPTOR) != 0) & ((qcode[None, :] & DONOR) != 0))
    d = r - _RADIUS[ki].astype(dtype)[:, None] - _RADIUS[kj].astype(dtype)[None, :]
    return r, r32, d, counted, hyd, hb


def _vina_score_host(lig_x, lig_code, mol_off, mol_group, mol_int, poc_x, poc_code, group_off, dtype=np.float64, eps=None):
    """`dsbdd_vina_score` in numpy: the same arguments, float32 coordinates, all arithmetic in `dtype` (float64: the
    specification).  -> (VinaScores of arrays in `dtype`, the batch's smallest |r - 8| over typed pairs).  With `eps` also
    the forward error bound of every output (see `error_bound`): (..., atom_bound [N, 5], mol_bound [B, 7])."""
    x = np.asarray(_np(lig_x), np.float32).reshape(-1, 3)
    code = np.asarray(_np(lig_code), np.int32).reshape(-1)
    q = np.asarray(_np(poc_x), np.float32).reshape(-1, 3)
    qcode = np.asarray(_np(poc_code), np.int32).reshape(-1)
    off = np.asarray(_np(mol_off), np.int64).reshape(-1)
    goff = np.asarray(_np(group_off), np.int64).reshape(-1)
    ints = np.asarray(_np(mol_int), np.int32).reshape(-1, MOL_INT)
    groups = np.asarray(_np(mol_group), np.int64).reshape(-1)
    B, G = len(off) - 1, len(goff) - 1
    if len(code) != len(x) or len(qcode) != len(q) or len(groups) != B or len(ints) != B:
        raise ValueError("one code per atom, one group and one mol_int row per molecule")
    atom = np.zeros((len(x), ATOM_OUT), dtype)
    mol = np.zeros((B, MOL_OUT), dtype)
    flag = np.zeros(B, np.int32)
    atom_bound, mol_bound = np.zeros((len(x), ATOM_OUT)), np.zeros((B, M_SCORE + 1))
    margin = np.inf
    w = np.asarray(WEIGHTS, dtype)
    for b in range(B):
        lo, hi = int(off[b]), int(off[b + 1])
        if not (lo >= 0 and hi >= lo and hi <= off[B]):
            lo = hi = 0
        g = int(groups[b])
        glo, ghi = (int(goff[g]), int(goff[g + 1])) if 0 <= g < G else (0, 0)
        if not (glo >= 0 and ghi >= glo and ghi <= goff[G]):
            glo = ghi = 0
        n_rot = max(int(ints[b, I_ROT]), 0)
        if not np.isfinite(x[lo:hi]).all():
            flag[b], atom[lo:hi], mol[b, :M_SCORE + 1] = 1, np.nan, np.nan
            atom_bound[lo:hi], mol_bound[b] = np.nan, np.nan
            continue
        if hi == lo or ghi == glo:
            continue
        r, r32, d, counted, hyd, hb = _molecule_pairs(x[lo:hi], code[lo:hi], q[glo:ghi], qcode[glo:ghi], dtype)
        typed = ((code[lo:hi, None] & CLASS_MASK) != 0) & ((qcode[None, glo:ghi] & CLASS_MASK) != 0)
        with np.errstate(invalid="ignore"):
            near = np.abs(r32.astype(np.float64) - CUTOFF)[typed & np.isfinite(r32)]
        if near.size:
            margin = min(margin, float(near.min()))
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.where(counted[..., None], pair_terms(d, hyd, hb), dtype(0))
        atom[lo:hi] = f.sum(1)
        mol[b, :ATOM_OUT] = f.sum((0, 1))
        mol[b, M_INTER] = (w * mol[b, :ATOM_OUT]).sum()
        mol[b, M_SCORE] = mol[b, M_INTER] / dtype(1.0 + ROT_WEIGHT * n_rot)
        if eps is not None:
            rr, dd = np.where(counted, r, 0).astype(np.float64), np.where(counted, d, 0).astype(np.float64)
            ff = np.abs(f.astype(np.float64))
            delta = np.where(counted, 4 * eps * rr + 16 * eps, 0.0)
            arg = np.stack([(dd / 0.5) ** 2, ((dd - 3) / 2) ** 2, 0 * dd, 0 * dd, 0 * dd], -1)
            lip = np.stack([np.full_like(dd, _LIPSCHITZ[0]), np.full_like(dd, _LIPSCHITZ[1]), 2 * np.abs(dd) + 2 * delta,
                            np.where(hyd, _LIPSCHITZ[3], 0.0), np.where(hb, _LIPSCHITZ[4], 0.0)], -1)
            pair = lip * delta[..., None] + (4 + arg) * eps * ff
            n_atom, n_mol = counted.sum(1).astype(np.float64), float(counted.sum())
            atom_bound[lo:hi] = pair.sum(1) + n_atom[:, None] * eps * ff.sum(1)
            mol_bound[b, :ATOM_OUT] = pair.sum((0, 1)) + n_mol * eps * ff.sum((0, 1))
            mol_bound[b, M_INTER] = (np.abs(np.asarray(WEIGHTS)) * mol_bound[b, :ATOM_OUT]).sum()
            mol_bound[b, M_SCORE] = mol_bound[b, M_INTER] / (1.0 + ROT_WEIGHT * n_rot) + 2 * eps * abs(float(mol[b, M_SCORE]))
    out = VinaScores(atom, mol, ints, flag, code, off.astype(np.int32))
    return (out, margin) if eps is None else (out, margin, atom_bound, mol_bound)


def error_bound(lig_x, lig_code, mol_off, mol_group, mol_int, poc_x, poc_code, group_off, eps=EPS32):
    """Forward error bound of a float32 evaluation against the float64 restatement, evaluated in float64:
    per counted pair dd = 4 eps r + 16 eps (the roundings of r and of the two subtractions of radii) and
    |df| <= L_k dd + (4 + |a|) eps |f| (L_k the Lipschitz constant of term k in d: 1.716, 0.429, 2 |d| + 2 dd, 1, 1 / 0.7;
    a the argument of the exponential, 0 for the other terms); per sum of n pair terms + n eps sum |f|; inter: sum |w_k|
    bound_k; score: that / (1 + 0.05846 N_rot) + 2 eps |score|.  -> (atom_bound [N, 5], mol_bound [B, 7]); NaN where the
    molecule is not finite."""
    _, _, atom_bound, mol_bound = _vina_score_host(lig_x, lig_code, mol_off, mol_group, mol_int, poc_x, poc_code, group_off,
                                                   eps=float(eps))
    return atom_bound, mol_bound


# ---- command line ----------------------------------------------------------------------------------------------------------
CSV_COLUMNS = ("n_atoms", "untyped", "n_rot", "nonfinite") + TERMS + ("inter", "score")


def write_csv(path, rows):
    """rows: (source, index, MolVina or its dict); `path` None writes to stdout."""
    _pairs.write_csv(path, rows, CSV_COLUMNS)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Vina-type interaction score of written ligand poses against a protein "
                                            "(one row per molecule; not smina output)")
    _pairs.add_complex_arguments(p)
    p.add_argument("--bonds", choices=("distance", "file"), default="distance",
                   help="distance: perceive bonds as for generated molecules; file: read the SDF bond block")
    p.add_argument("--dataset", default="crossdock", help="the dataset whose bond-length tables --bonds distance uses")
    return _pairs.parse_complex_arguments(p, argv)


def main(argv=None):
    a = parse_args(argv)
    print(VINA_COVERAGE, file=sys.stderr)
    typed = type_pocket(select_residues(a.pdbfile, a.scope, a.ref_ligand))
    print(f"[vina] {len(typed.code)} protein heavy atoms, {typed.untemplated} typed by element alone", file=sys.stderr)
    pockets = VinaPocket.upload([typed], torch.device(a.device))
    rows = []
    for path in a.sdf:
        rows += [(path, k, rec) for k, rec in enumerate(score_molecules(path, pockets, a.dataset, bonds=a.bonds))]
    write_csv(a.out, rows)
    return rows


if __name__ == "__main__":
    main()
