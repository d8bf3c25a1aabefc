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

Gradient (`vina_gradient`, `vina_energy`; one launch of `dsbdd_vina_score_grad`, csrc/vina_grad.h, in place of
`dsbdd_vina_score`: the same sweep writes the score's outputs bit for bit and the gradient; `_vina_grad_host` restates it):

    u           = (x_i - x_j) / r              the three float32 differences the distance is formed from, over r
    gauss1'     = -8 d exp(-4 d^2)             gauss2' = -c exp(-c^2), c = (d - 3) / 2
    repulsion'  = 2 d if d < 0, else 0
    hydrophobic'= -1 if 0.5 < d < 1.5, else 0  hbond' = -1 / 0.7 if -0.7 < d < 0, else 0     one-sided as the terms are
    g_i         = sum_j (sum_k WEIGHTS[k] T_k'(d_ij)) u_ij          d inter / d x_i, kcal/mol/A; a pair with r = 0 adds 0
    d score / d x_i = g_i / (1 + ROT_WEIGHT N_rot)                  typing (codes, N_rot) is constant in x

Minimiser (`vina_minimize`; one launch of `dsbdd_vina_minimize`, csrc/vina_minimize.h: one workgroup per molecule iterates the
gradient's sweep, every decision on the device; `_vina_minimize_host` states the iteration): the ligand moves as a rigid
body, pose (T, q) from (0, identity), x_i = float32((c0 + T) + R(q) (x0_i - c0)) always from the input x0; steepest descent in
the metric u = |F| + rho_max |M| / rho^2 with a backtracking step L (0.25 A, halved on a trial that does not lower `inter`,
doubled back after one that does) until L < 0.001 A or 200 evaluations.  Rigid ligand, rigid protein, local: VINA_MIN_COVERAGE.

  python -m diffsbdd_amd.vina --pdbfile P.pdb --sdf L.sdf [L2.sdf ...] [--scope protein|pocket --ref_ligand ...]
                              [--bonds distance|file] [--dataset crossdock] [--out scores.csv] [--grad_out atoms.csv]
                              [--minimize relaxed.sdf [--torsions] [--step 0.25] [--tol 0.001] [--max_evals 200]]

Torsion tree, intramolecular term and flexible minimiser (`ligand_torsions`, `vina_intra`, `vina_minimize(torsions=True)`;
csrc/vina_torsion.h, csrc/vina_intra.h, csrc/vina_flex.h; `torsion_tree`, `_vina_intra_host`, `_vina_flex_host` restate
them): the rotors that N_rot counts, at most 32 kept, each with the smaller side of the molecule as its moving side; intra =
the five terms over the ligand's own pairs more than 3 bonds apart that a kept rotor separates; the flexible minimiser is
the rigid one with the torsion angles as further coordinates and E = inter + intra.  VINA_INTRA_COVERAGE, VINA_FLEX_COVERAGE.
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
ATOM_GRAD, MOL_GRAD = 3, 8            # columns of the gradient outputs of dsbdd_vina_score_grad
G_NET, G_MOMENT, G_MAX, G_ROT = slice(0, 3), slice(3, 6), 6, 7
MOL_POSE, MOL_MIN, MOL_STAT = 8, 4, 4  # columns of the minimiser's outputs (dsbdd_vina_minimize)
P_SHIFT, P_QUAT, P_RHO2 = slice(0, 3), slice(3, 7), 7
E_START, E_FINAL, E_STEP, E_SLOPE = range(4)
S_STATUS, S_EVALS, S_ACCEPTED = range(3)
STATUS = ("budget", "converged", "no gradient", "nonfinite")
MIN_STEP, MIN_TOL, MIN_EVALS, MAX_EVALS = 0.25, 1e-3, 200, 4096
MAX_TORSIONS, TOR_INT, MASK_WORDS = 32, 4, 4   # rotors kept per molecule, columns of tor_int, int32 words of a 128-bit mask
T_KEPT, T_FOUND = 0, 1
MOL_FLEX = 8                           # columns of the flexible minimiser's energies (dsbdd_vina_flex): E_START ... E_SLOPE as above, then
X_INTRA_START, X_INTRA_FINAL, X_E_START, X_E_FINAL = range(4, 8)
DOF_RIGID, DOF_TORSIONS = 1, 2         # bits of `dofs`
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

VINA_GRAD_COVERAGE = (
    "Vina-type gradient: PRESENT = the analytic gradient of the intermolecular term `inter` of the Vina-type score with "
    "respect to the coordinates of the ligand heavy atoms only, in kcal/mol/A, from the GPU sweep that also scores (the score's "
    "outputs come out unchanged), per atom, with its sum, its moment about the ligand's centroid, its largest norm and the "
    "factor 1 / (1 + 0.05846 N_rot) that turns it into the gradient of `score`, and as a torch autograd function of the "
    "coordinates; "
    "DEFINED AS = the sum over the pairs counted at the given pose of the terms' derivatives in the surface distance times "
    "the unit vector from the pocket atom to the ligand atom; a ligand atom exactly on a pocket atom adds nothing; at the "
    "kinks of the piecewise-linear terms the derivative is that of the branch the term takes there; "
    "NOT = a gradient with respect to protein coordinates (rigid protein); NOT a gradient of the typing: atom codes and "
    "N_rot are constants, so a bond made or broken by moving atoms is not seen; NOT smooth: it is discontinuous where the score "
    "is, at the 8 A cutoff (a jump of the score that the gradient ignores) and at the kinks of the repulsion, hydrophobic and "
    "hbond terms; NOT smina's minimiser and not a minimiser at all: no search, no line search, no pose is changed; "
    "no intramolecular term.")

VINA_MIN_COVERAGE = (
    "Vina-type minimiser: PRESENT = a rigid-body relaxation of every given pose under the intermolecular term `inter` of the "
    "Vina-type score, one GPU launch per batch (one workgroup per molecule, every evaluation and decision on the device): the "
    "pose moves by a translation and a rotation about its centroid, and the score, its terms and its gradient are reported at "
    "the returned pose together with the score at the start, the number of evaluations, a status and the RMSD moved; "
    "DEFINED AS = steepest descent in a scaled metric (the net force and the moment about the centroid divided by the "
    "ligand's mean squared radius) with a backtracking step: from 0.25 A (--step) the step halves when a trial does not lower "
    "`inter` and doubles back after one that does, until it falls below 0.001 A (--tol) or 200 evaluations (--max_evals) "
    "are spent; "
    "NOT = a docking run: the ligand is rigid (no torsions), the protein is rigid, the search is local (one start, the "
    "nearest minimum downhill, no global search, no multiple starts), steepest descent and not BFGS, no intramolecular "
    "term; NOT the output of smina or qvina and NOT comparable with their minimised or docked scores; typing is done once, "
    "on the input pose.")

VINA_INTRA_COVERAGE = (
    "Vina-type intramolecular term: PRESENT = the torsion tree of every ligand (one GPU kernel on the bond-order matrices: "
    "the rotatable bonds that N_rot counts, at most 32 kept in ascending order of their atom indices, each with the smaller "
    "side of the molecule as its moving side) and the five pair terms of the Vina-type score with their analytic gradient "
    "summed by one GPU kernel over the ligand's own heavy-atom pairs closer than 8 A that are more than 3 bonds apart (or "
    "not connected) and separated by a kept rotatable bond, per atom and per molecule, `intra` = the weighted sum, every "
    "pair once, not divided by the rotor factor; "
    "NOT = a minimiser: this entry changes no pose and turns no torsion (the flexible minimiser does, the rigid-body "
    "minimiser does not read this term); NOT the intramolecular energy smina or Vina print (heavy atoms only, amide and conjugated bonds rotate, typing "
    "and the tree fixed on the bond orders given); a molecule without rotatable bonds, or longer than 128 atoms, has no "
    "pair and an intramolecular term of exactly 0.")

VINA_FLEX_COVERAGE = (
    "Vina-type flexible minimiser: PRESENT = a relaxation of every given pose over its translation, its rotation and its "
    "rotatable bonds (the torsion tree of the intramolecular term: at most 32 rotors, each turning the smaller side of the "
    "molecule) under E = inter + intra of the Vina-type score, one GPU launch per batch after the typing and the tree (one "
    "workgroup per molecule, every evaluation and decision on the device); `inter`, `score` and their gradient are reported "
    "at the returned pose as the rigid minimiser reports them, `intra` beside them, with both at the start, the torsion "
    "angles, a status and the RMSD moved; bond lengths, angles and rings keep the input's geometry; "
    "DEFINED AS = steepest descent in a scaled metric (net force, moment about the centroid over the mean squared radius, "
    "and per rotor the torque about its axis over the mean squared distance of its side from the axis) with the backtracking "
    "step of the rigid minimiser: no atom moves more than the step (0.25 A, halved on a trial that does not lower E, doubled "
    "back after one that does) until it falls below 0.001 A or 200 evaluations are spent; `dofs` switches the rigid body "
    "(bit 0) or the torsions (bit 1) off; "
    "NOT = BFGS; NOT a docking run: a local search from one start, the nearest minimum downhill, a rigid protein, heavy atoms "
    "only (no hydrogens, no charges), typing and the torsion tree fixed on the input pose, amide and conjugated bonds "
    "rotate, rotors beyond the first 32 and every rotor of a molecule longer than 128 atoms stay rigid; NOT the output of "
    "smina or qvina and NOT comparable with their minimised or docked scores.")


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


@dataclass
class MolVinaGrad(MolVina):
    """`MolVina` with the gradient of `inter` of one molecule (host arrays)."""
    grad: np.ndarray = None       # float32 [n, 3]: d inter / d x_i, kcal/mol/A
    mol_grad: np.ndarray = None   # float32 [8]: net (3), moment about the centroid (3), max |g_i|, 1 / (1 + ROT_WEIGHT N_rot)

    net = property(lambda self: self.mol_grad[G_NET])
    moment = property(lambda self: self.mol_grad[G_MOMENT])
    max_norm = property(lambda self: float(self.mol_grad[G_MAX]))
    rot_factor = property(lambda self: float(self.mol_grad[G_ROT]))
    score_grad = property(lambda self: self.mol_grad[G_ROT] * self.grad)

    def as_dict(self):
        out = super().as_dict()
        out.update(max_norm=self.max_norm, rot_factor=self.rot_factor, net=[float(v) for v in self.net],
                   moment=[float(v) for v in self.moment])
        return out


@dataclass
class VinaGradients(VinaScores):
    """`VinaScores` with the outputs of the fused launch (device tensors from `vina_gradient`, numpy arrays from
    `_vina_grad_host`)."""
    grad: object = None      # float [N, 3]: d inter / d x_i
    mol_grad: object = None  # float [B, 8]
    kink_margin: float = float("inf")   # `_vina_grad_host` only: the smallest |d - kink| over the pairs a kink of hydrophobic' / hbond' applies to

    net = property(lambda self: self.mol_grad[:, G_NET])
    moment = property(lambda self: self.mol_grad[:, G_MOMENT])
    max_norm = property(lambda self: self.mol_grad[:, G_MAX])
    rot_factor = property(lambda self: self.mol_grad[:, G_ROT])

    @property
    def atom_mol(self):
        """[N] the molecule of every atom (from `mol_off`; no read-back)."""
        off = self.mol_off
        if torch.is_tensor(off):
            return torch.repeat_interleave(torch.arange(len(off) - 1, device=off.device), (off[1:] - off[:-1]).long(),
                                           output_size=int(self.grad.shape[0]))
        return np.repeat(np.arange(len(off) - 1), np.diff(off))

    @property
    def score_grad(self):
        """[N, 3] d score / d x_i = rot_factor[mol] grad."""
        return self.rot_factor[self.atom_mol][:, None] * self.grad

    def molecules(self):
        """One `MolVinaGrad` per molecule, in order (one copy of each tensor to the host)."""
        grad, mol_grad, off = _np(self.grad), _np(self.mol_grad), _np(self.mol_off)
        return [MolVinaGrad(m.mol, m.ints, m.atom, m.code, m.nonfinite, grad[off[b]:off[b + 1]].copy(), mol_grad[b].copy())
                for b, m in enumerate(VinaScores.molecules(self))]


@dataclass
class MolVinaMin(MolVinaGrad):
    """`MolVinaGrad` at the pose the minimiser returned for one molecule (host arrays), with that pose."""
    x: np.ndarray = None          # float32 [n, 3]: the returned coordinates
    pose: np.ndarray = None       # float [8]: T (3), q (4, w first), rho^2
    energies: np.ndarray = None   # float [4]: inter at the start, at the end, the last accepted step (0 if none), u at the end
    stat: np.ndarray = None       # int32 [4]: status (index into STATUS), evaluations, accepted steps, 0
    rmsd: float = 0.0             # heavy-atom RMSD between the input and the returned coordinates

    status = property(lambda self: int(self.stat[S_STATUS]))
    evals = property(lambda self: int(self.stat[S_EVALS]))
    accepted = property(lambda self: int(self.stat[S_ACCEPTED]))
    inter_start = property(lambda self: float(self.energies[E_START]))
    score_start = property(lambda self: float(self.energies[E_START]) * self.rot_factor)

    def as_dict(self):
        out = super().as_dict()
        out.update(inter_start=self.inter_start, score_start=self.score_start, status=self.status, evals=self.evals,
                   accepted=self.accepted, rmsd=float(self.rmsd))
        return out


@dataclass
class VinaMinimized(VinaGradients):
    """`VinaGradients` at the poses the minimiser returned (device tensors from `vina_minimize`, numpy arrays from
    `_vina_minimize_host`), with the poses."""
    x: object = None         # float32 [N, 3]: the returned coordinates
    pose: object = None      # float [B, 8]: T (3), q (4, w first), rho^2
    energies: object = None  # float [B, 4]: inter at the start, at the end, the last accepted step (0 if none), u at the end
    stat: object = None      # int32 [B, 4]: status (index into STATUS), evaluations, accepted steps, 0
    x_in: object = None      # float32 [N, 3]: the input coordinates

    status = property(lambda self: self.stat[:, S_STATUS])
    evals = property(lambda self: self.stat[:, S_EVALS])
    accepted = property(lambda self: self.stat[:, S_ACCEPTED])
    inter_start = property(lambda self: self.energies[:, E_START])
    score_start = property(lambda self: self.energies[:, E_START] * self.rot_factor)

    @property
    def rmsd(self):
        """[B] the heavy-atom RMSD between input and returned coordinates (0 for a molecule without atoms; torch on the
        device for device tensors, no read-back)."""
        off, mol = self.mol_off, self.atom_mol
        if torch.is_tensor(self.x):
            d2 = ((self.x.double() - self.x_in.double()) ** 2).sum(1)
            total = torch.zeros(len(off) - 1, dtype=torch.float64, device=d2.device).index_add_(0, mol, d2)
            return torch.sqrt(total / (off[1:] - off[:-1]).clamp(min=1).double())
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = ((self.x.astype(np.float64) - self.x_in.astype(np.float64)) ** 2).sum(1)
        total = np.zeros(len(off) - 1)
        np.add.at(total, mol, d2)
        return np.sqrt(total / np.maximum(np.diff(off), 1))

    def molecules(self):
        """One `MolVinaMin` per molecule, in order (one copy of each tensor to the host)."""
        x, pose, energies, stat, rmsd, off = (_np(v) for v in (self.x, self.pose, self.energies, self.stat, self.rmsd,
                                                               self.mol_off))
        return [MolVinaMin(m.mol, m.ints, m.atom, m.code, m.nonfinite, m.grad, m.mol_grad, x[off[b]:off[b + 1]].copy(),
                           pose[b].copy(), energies[b].copy(), stat[b].copy(), float(rmsd[b]))
                for b, m in enumerate(VinaGradients.molecules(self))]


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
    if orders is None:
        orders = _perceived_orders(x, at, lig_mask, info, B)
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


def _perceived_orders(x, at, lig_mask, info, B):
    """The bond-order matrices `type_ligands` types from when none are given: `molecules.bond_orders` with the tables of the
    dataset `info` (its dict), cut to the block of the first 128 atoms of every molecule; [B, 1, 1] zeros without atoms."""
    if x.shape[0] == 0:
        return torch.zeros((B, 1, 1), dtype=torch.int8, device=x.device)
    if not isinstance(info, dict) or "bonds1" not in info:
        raise ValueError("bond perception needs the dataset (its name or dict), not the decoder alone")
    from .molecules import bond_orders
    orders, _ = bond_orders(x, at, lig_mask, info, batch=B)
    if orders.shape[1] > _lib.MOL_MAX_ATOMS:                        # the block of the first 128 atoms of every molecule
        orders = orders[:, :_lib.MOL_MAX_ATOMS, :_lib.MOL_MAX_ATOMS].contiguous()
    return orders


def perceive_orders(x, atom_type, lig_mask, info, batch=None):
    """The `orders` that `vina_score`, `vina_gradient` and `vina_minimize` perceive for themselves when none are given, for a
    caller that runs more than one of them on a batch: int8 [B, n_max, n_max] on the device.  Arguments as for `type_ligands`."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.HipLibraryError("perceive_orders needs device tensors (HIP path; no CPU fallback)")
    x = x.detach().to(torch.float32).reshape(-1, 3).contiguous()
    at = torch.as_tensor(atom_type, device=x.device).to(torch.int32).reshape(-1).contiguous()
    lig_mask = torch.as_tensor(lig_mask, device=x.device).reshape(-1)
    return _perceived_orders(x, at, lig_mask, _decoder(info)[1], _n_molecules(lig_mask, batch))


def vina_score(x, atom_type, lig_mask, pockets, info, mol_group=None, batch=None, orders=None):
    """The score of a batch on device tensors: bond orders (unless given), `dsbdd_vina_type`, `dsbdd_vina_score`; no
    read-back inside.  x, atom_type, lig_mask, info, orders, batch as for `type_ligands`; `pockets`: a `VinaPocket`
    (uploaded before) or a list of `TypedPocket` / (xyz, code) host arrays, one per group; `mol_group` [B] as for
    `pose.pose_check`.  -> VinaScores of device tensors."""
    return _scored("vina_score", VinaScores, x, atom_type, lig_mask, pockets, info, mol_group, batch, orders)


def _scored(what, kind, x, atom_type, lig_mask, pockets, info, mol_group, batch, orders, settings=None):
    """The launches behind `vina_score` (kind VinaScores: `dsbdd_vina_score`), `vina_gradient` (kind VinaGradients:
    `dsbdd_vina_score_grad`, two more outputs) and `vina_minimize` (kind VinaMinimized: `dsbdd_vina_minimize` with
    `settings` = (step, tol, max_evals), four more) after the typing all share."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.HipLibraryError(f"{what} needs device tensors (HIP path; no CPU fallback)")
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
    out = kind(torch.zeros((N, ATOM_OUT), **f32), torch.zeros((B, MOL_OUT), **f32), mol_int,
               torch.zeros(B, dtype=torch.int32, device=dev), code, off)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    args = (stream, _ptr(x), _ptr(code), off.data_ptr(), B, _ptr(groups), _ptr(mol_int), _ptr(pockets.x), _ptr(pockets.code),
            pockets.group_off.data_ptr(), G, _ptr(out.atom), _ptr(out.mol), _ptr(out.flag))
    if kind is VinaScores:
        rc = lib.dsbdd_vina_score(*args)
    else:
        out.grad, out.mol_grad = torch.zeros((N, ATOM_GRAD), **f32), torch.zeros((B, MOL_GRAD), **f32)
        if kind is VinaGradients:
            rc = lib.dsbdd_vina_score_grad(*args, _ptr(out.grad), _ptr(out.mol_grad))
        else:
            step, tol, max_evals = settings
            out.x_in, out.x = x, x.clone()                             # x_out must not alias the input
            out.pose, out.energies = torch.zeros((B, MOL_POSE), **f32), torch.zeros((B, MOL_MIN), **f32)
            out.stat = torch.zeros((B, MOL_STAT), dtype=torch.int32, device=dev)
            # without atoms both pointers are stand-ins (`_ptr`); held here together, so that they are two addresses
            x_arg, x_out_arg = (x, out.x) if N else (torch.zeros(4, **f32), torch.zeros(4, **f32))
            rc = lib.dsbdd_vina_minimize(stream, x_arg.data_ptr(), *args[2:], _ptr(out.grad), _ptr(out.mol_grad), float(step),
                                         float(tol), int(max_evals), x_out_arg.data_ptr(), _ptr(out.pose), _ptr(out.energies),
                                         _ptr(out.stat))
    _lib.check(rc, {VinaScores: "dsbdd_vina_score", VinaGradients: "dsbdd_vina_score_grad"}.get(kind, "dsbdd_vina_minimize"))
    return out


def vina_gradient(x, atom_type, lig_mask, pockets, info, mol_group=None, batch=None, orders=None):
    """The score of a batch and the gradient of its `inter` term with respect to x, on device tensors: the launches of
    `vina_score` with `dsbdd_vina_score_grad` in place of `dsbdd_vina_score` (one sweep writes both; the score's outputs
    are bit for bit those of `vina_score`).  Arguments as for `vina_score`.  -> VinaGradients of device tensors: `grad`
    [N,3] = d inter / d x_i in kcal/mol/A (0 for untyped atoms), `mol_grad` [B,8] with the properties `net`, `moment` (about
    the centroid), `max_norm`, `rot_factor`, and `score_grad` = rot_factor[mol] grad.  See `VINA_GRAD_COVERAGE`."""
    return _scored("vina_gradient", VinaGradients, x, atom_type, lig_mask, pockets, info, mol_group, batch, orders)


def _settings(step, tol, max_evals):
    """(step, tol, max_evals) as the C entry takes them (float32, float32, int), refused here as it refuses them."""
    step, tol = float(np.float32(step)), float(np.float32(tol))
    if not (np.isfinite(step) and step > 0 and np.isfinite(tol) and tol > 0):
        raise ValueError("step and tol must be finite and positive")
    if int(max_evals) != max_evals or not 1 <= int(max_evals) <= MAX_EVALS:
        raise ValueError(f"max_evals must be an integer in [1, {MAX_EVALS}]")
    return step, tol, int(max_evals)


def vina_minimize(x, atom_type, lig_mask, pockets, info, mol_group=None, batch=None, orders=None, step=MIN_STEP, tol=MIN_TOL,
                  max_evals=MIN_EVALS, torsions=False, dofs=DOF_RIGID | DOF_TORSIONS):
    """Rigid-body relaxation of every pose of a batch under `inter`, on device tensors: the typing of `vina_score` (once, on
    the input pose), then one launch of `dsbdd_vina_minimize` (csrc/vina_minimize.h; one workgroup per molecule iterates
    the sweep of `vina_gradient`, every decision on the device); no read-back inside.  Arguments as for `vina_score`;
    `step` the first and largest step (A; no atom moves further in one trial), `tol` the step below which it stops,
    `max_evals` the evaluation budget (1 ... 4096).  x is not written.  -> VinaMinimized of device tensors: the fields of
    `vina_gradient` at the returned pose (bit for bit what `vina_gradient` gives on `x`), `x` [N,3], `pose` [B,8], `energies`
    [B,4], `stat` [B,4] and the properties `status` (index into STATUS), `evals`, `accepted`, `inter_start`, `score_start`,
    `rmsd`.  `_vina_minimize_host` states the iteration; see `VINA_MIN_COVERAGE` for what this is not.
    torsions=True: the flexible relaxation instead (`dsbdd_vina_torsions`, then one launch of `dsbdd_vina_flex`,
    csrc/vina_flex.h): the rotatable bonds turn as well and the objective is inter + intra; `dofs` bit 0 = the rigid body,
    bit 1 = the torsions.  -> VinaFlexed: the same fields (`inter`, `score`, the gradient stay the intermolecular ones;
    `energies` [B,8]) and `intra`, `intra_start`, `theta` [B,32], `tau`, `n_torsions`, `torsions_found`, `intra_out`.
    `_vina_flex_host` states that iteration; see `VINA_FLEX_COVERAGE`.  Without the keyword nothing changes."""
    if torsions:
        return _flexed(x, atom_type, lig_mask, pockets, info, mol_group, batch, orders, _settings(step, tol, max_evals), dofs)
    return _scored("vina_minimize", VinaMinimized, x, atom_type, lig_mask, pockets, info, mol_group, batch, orders,
                   _settings(step, tol, max_evals))


def _chain(grad_out, grad, rot_factor, mol, which):
    """d (sum_b grad_out[b] E_b) / d x from the saved gradient of `inter`: E = score carries the rotor factor."""
    scale = grad_out[mol] * rot_factor[mol] if which == "score" else grad_out[mol]
    return scale[:, None] * grad


class VinaScoreFunction(torch.autograd.Function):
    """`score` or `inter` [B] as a differentiable function of the ligand coordinates x (the only input with a gradient):
    forward = one fused launch (`vina_gradient`), which saves d inter / d x and the rotor factors; backward = the chain rule
    on them in plain torch.  Once differentiable: the saved gradient is a constant, a second derivative is refused.  A
    molecule with a coordinate that is not finite has a NaN energy and NaN gradient rows."""

    @staticmethod
    def forward(ctx, x, atom_type, lig_mask, pockets, info, mol_group, batch, orders, which):
        if which not in ("score", "inter"):
            raise ValueError("which must be 'score' or 'inter'")
        st = vina_gradient(x, atom_type, lig_mask, pockets, info, mol_group, batch, orders)
        ctx.save_for_backward(st.grad, st.rot_factor.contiguous(), st.atom_mol)
        ctx.which, ctx.x_shape, ctx.x_dtype = which, x.shape, x.dtype
        return (st.score if which == "score" else st.inter).clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        grad, rot_factor, mol = ctx.saved_tensors
        gx = _chain(grad_out.to(torch.float32), grad, rot_factor, mol, ctx.which)
        return (gx.reshape(ctx.x_shape).to(ctx.x_dtype),) + (None,) * 8


def vina_energy(x, atom_type, lig_mask, pockets, info, mol_group=None, batch=None, orders=None, which="score"):
    """`score` (which='score') or `inter` (which='inter') of every molecule, float32 [B] on the device, differentiable in x
    through `VinaScoreFunction`: `vina_energy(x, ...).sum().backward()` leaves d score / d x in `x.grad`.  The other
    arguments as for `vina_score`; none of them receives a gradient."""
    return VinaScoreFunction.apply(x, atom_type, lig_mask, pockets, info, mol_group, batch, orders, which)


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
    return _molecule_records(vina_score, "score_molecules", molecules, pockets, info, mol_group, device, bonds)


def gradient_molecules(molecules, pockets, info="crossdock", mol_group=None, device="cuda", bonds="distance"):
    """`score_molecules` through the launches of `vina_gradient`: the same arguments, the same score records, and the
    gradient of `inter` with them.  -> list of `MolVinaGrad`."""
    return _molecule_records(vina_gradient, "gradient_molecules", molecules, pockets, info, mol_group, device, bonds)


def minimize_molecules(molecules, pockets, info="crossdock", mol_group=None, device="cuda", bonds="distance", step=MIN_STEP,
                       tol=MIN_TOL, max_evals=MIN_EVALS, torsions=False, dofs=DOF_RIGID | DOF_TORSIONS):
    """`gradient_molecules` through the launches of `vina_minimize`: the same arguments and the minimiser's settings.
    -> list of `MolVinaMin`: the records of `gradient_molecules` at the returned pose, with its coordinates `x`; with
    torsions=True list of `MolVinaFlex` (the flexible relaxation)."""
    def entry(*args, **kwargs):
        return vina_minimize(*args, step=step, tol=tol, max_evals=max_evals, torsions=torsions, dofs=dofs, **kwargs)
    return _molecule_records(entry, "minimize_molecules", molecules, pockets, info, mol_group, device, bonds)


def _molecule_records(entry, what, molecules, pockets, info, mol_group, device, bonds):
    if bonds not in ("distance", "file"):
        raise ValueError("bonds must be 'distance' or 'file'")
    ligands = as_ligands(molecules)
    dev = pockets.x.device if isinstance(pockets, VinaPocket) else torch.device(device)
    if dev.type != "cuda":
        raise _lib.HipLibraryError(f"{what} needs a HIP device (no CPU fallback)")
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
    st = entry(torch.as_tensor(x, device=dev), torch.as_tensor(at, device=dev), torch.as_tensor(mask, device=dev), pockets,
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


def _vina_score_host(lig_x, lig_code, mol_off, mol_group, mol_int, poc_x, poc_code, group_off, dtype=np.float64, eps=None,
                     pair_mask=None):
    """`dsbdd_vina_score` in numpy: the same arguments, float32 coordinates, all arithmetic in `dtype` (float64: the
    specification).  -> (VinaScores of arrays in `dtype`, the batch's smallest |r - 8| over typed pairs).  With `eps` also
    the forward error bound of every output (see `error_bound`): (..., atom_bound [N, 5], mol_bound [B, 7]).  `pair_mask`
    (int32 [N, 4], `_vina_intra_host` alone): only the pairs (i, j) with bit j of atom i's 128-bit mask set are counted."""
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
        if pair_mask is not None:
            listed = unpack_masks(pair_mask[lo:hi], ghi - glo)
            counted, typed = counted & listed, typed & listed
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


# ---- the gradient: float64 restatement and error bound -----------------------------------------------------------------------------
_CURVATURE = (8.0, 0.5, 2.0)          # sup |T_k''| of gauss1, gauss2 and (where d < 0) repulsion
_KINKS = ((0.5, 1.5), (-0.7, 0.0))    # of hydrophobic', hbond': where the piecewise-constant derivative jumps
_JUMPS = (1.0, 1.0 / 0.7)
EPS64 = 2.0 ** -53


def pair_slopes(d, hydrophobic=True, hbond=True):
    """The derivatives of the five terms in the surface distance at `d` (any shape) in d's dtype -> [..., 5], one-sided at
    the kinks as `pair_terms` is: at d = 0.5, 1.5, -0.7, 0 the value of the constant branch the term takes there."""
    d = np.asarray(d)
    t = d.dtype.type
    zero = t(0)
    a, c = d / t(0.5), (d - t(3)) / t(2)
    out = np.stack([t(-8) * d * np.exp(-(a * a)), -c * np.exp(-(c * c)), np.where(d < 0, t(2) * d, zero),
                    np.where((d > t(0.5)) & (d < t(1.5)), t(-1), zero),
                    np.where((d > t(-0.7)) & (d < 0), t(-1) / t(0.7), zero)], -1)
    out[..., 3] = np.where(hydrophobic, out[..., 3], zero)
    out[..., 4] = np.where(hbond, out[..., 4], zero)
    return out


def _vina_grad_host(lig_x, lig_code, mol_off, mol_group, mol_int, poc_x, poc_code, group_off, dtype=np.float64, eps=None,
                    pair_mask=None):
    """`dsbdd_vina_score_grad` in numpy: the arguments of `_vina_score_host`, float32 coordinates, the counted pairs decided
    by the float32 distance (and a pair whose float32 distance is 0 adds nothing to the gradient), everything else in
    `dtype` from differences and a root formed in `dtype` (float64: the specification; its differences of float32
    coordinates are exact).  -> VinaGradients of arrays in `dtype`: the fields of `_vina_score_host`'s result, grad [N, 3],
    mol_grad [B, 8].  With `eps` also the forward error bound of `grad_error_bound`: (result, grad_bound [N, 3],
    mol_grad_bound [B, 8]), and the smallest distance |d - kink| over the pairs a kink of hydrophobic' / hbond' applies to
    as `result.kink_margin`.  `pair_mask` as for `_vina_score_host`."""
    st, _ = _vina_score_host(lig_x, lig_code, mol_off, mol_group, mol_int, poc_x, poc_code, group_off, dtype=dtype,
                             pair_mask=pair_mask)
    x = np.asarray(_np(lig_x), np.float32).reshape(-1, 3)
    q = np.asarray(_np(poc_x), np.float32).reshape(-1, 3)
    code, qcode = st.lig_code, np.asarray(_np(poc_code), np.int32).reshape(-1)
    off, goff = st.mol_off.astype(np.int64), np.asarray(_np(group_off), np.int64).reshape(-1)
    groups = np.asarray(_np(mol_group), np.int64).reshape(-1)
    B, G = len(off) - 1, len(goff) - 1
    grad, mol_grad = np.zeros((len(x), ATOM_GRAD), dtype), np.zeros((B, MOL_GRAD), dtype)
    grad_bound, mol_bound = np.zeros((len(x), ATOM_GRAD)), np.zeros((B, MOL_GRAD))
    kink_margin = np.inf
    w = np.asarray(WEIGHTS, dtype)
    aw = np.abs(np.asarray(WEIGHTS, np.float64))
    for b in range(B):
        lo, hi = int(off[b]), int(off[b + 1])
        if not (lo >= 0 and hi >= lo and hi <= off[B]):
            lo = hi = 0
        g = int(groups[b])
        glo, ghi = (int(goff[g]), int(goff[g + 1])) if 0 <= g < G else (0, 0)
        if not (glo >= 0 and ghi >= glo and ghi <= goff[G]):
            glo = ghi = 0
        if st.flag[b]:
            grad[lo:hi], mol_grad[b], grad_bound[lo:hi], mol_bound[b] = np.nan, np.nan, np.nan, np.nan
            continue
        n, n_rot = hi - lo, max(int(st.mol_int[b, I_ROT]), 0)
        mol_grad[b, G_ROT] = dtype(1.0) / dtype(1.0 + ROT_WEIGHT * n_rot)
        if eps is not None:
            mol_bound[b, G_ROT] = 3 * eps * float(mol_grad[b, G_ROT])
        if n == 0 or ghi == glo:
            continue
        r, r32, d, counted, hyd, hb = _molecule_pairs(x[lo:hi], code[lo:hi], q[glo:ghi], qcode[glo:ghi], dtype)
        if pair_mask is not None:
            counted = counted & unpack_masks(pair_mask[lo:hi], ghi - glo)
        live = counted & (r32 > 0)                                              # coincident atoms have no direction
        xd = x[lo:hi].astype(dtype)
        e = xd[:, None, :] - q[glo:ghi].astype(dtype)[None, :, :]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            slopes = np.where(live[..., None], pair_slopes(d, hyd, hb), dtype(0)) * w          # [n, m, 5] weighted
            S = slopes.sum(-1)
            u = np.where(live[..., None], e / np.where(live, r, dtype(1))[..., None], dtype(0))
        f = S[..., None] * u                                                    # [n, m, 3]
        gm = f.sum(1)
        grad[lo:hi] = gm
        c = xd.sum(0) / dtype(n)
        y = xd - c
        norms = np.sqrt((gm[:, 0] * gm[:, 0] + gm[:, 1] * gm[:, 1]) + gm[:, 2] * gm[:, 2])
        mol_grad[b, G_NET], mol_grad[b, G_MOMENT], mol_grad[b, G_MAX] = gm.sum(0), np.cross(y, gm).sum(0), norms.max()
        if eps is None:
            continue
        rr, dd = np.where(live, r, 0.0).astype(np.float64), np.where(live, d, 0.0).astype(np.float64)
        delta = np.where(live, 4 * eps * rr + 16 * eps, 0.0)
        arg = np.stack([(dd / 0.5) ** 2, ((dd - 3) / 2) ** 2], -1)
        sl = np.abs(slopes.astype(np.float64))
        # the slope: curvature times the error of d, the jumps of the piecewise-constant derivatives inside it, evaluation
        lip = aw[0] * _CURVATURE[0] + aw[1] * _CURVATURE[1] + np.where(dd <= delta, aw[2] * _CURVATURE[2], 0.0)
        jump = np.zeros_like(dd)
        for flagged, kinks, size, weight in ((hyd, _KINKS[0], _JUMPS[0], aw[3]), (hb, _KINKS[1], _JUMPS[1], aw[4])):
            near = np.minimum(np.abs(dd - kinks[0]), np.abs(dd - kinks[1]))
            jump += np.where(live & flagged & (near <= delta), weight * size, 0.0)
            if (live & flagged).any():
                kink_margin = min(kink_margin, float(near[live & flagged].min()))
        evaluation = eps * ((10 + 3 * arg[..., 0]) * sl[..., 0] + (10 + 3 * arg[..., 1]) * sl[..., 1] + 6 * sl[..., 2:].sum(-1))
        dS = np.where(live, lip * delta + jump + evaluation, 0.0)
        au, af = np.abs(u.astype(np.float64)), np.abs(f.astype(np.float64))
        pair = dS[..., None] * au + 7 * eps * af
        n_atom = live.sum(1).astype(np.float64)
        ab = pair.sum(1) + n_atom[:, None] * eps * af.sum(1)
        grad_bound[lo:hi] = ab
        ag, ay, ax = np.abs(gm.astype(np.float64)), np.abs(y.astype(np.float64)), np.abs(xd.astype(np.float64))
        mol_bound[b, G_NET] = ab.sum(0) + n * eps * ag.sum(0)
        dy = (n + 1) * eps * ax.mean(0)[None, :] + eps * ay
        ac = np.abs(c.astype(np.float64))
        for k in range(3):
            i, j = (k + 1) % 3, (k + 2) % 3
            mol_bound[b, 3 + k] = (dy[:, i] * ag[:, j] + ay[:, i] * ab[:, j] + dy[:, j] * ag[:, i] + ay[:, j] * ab[:, i]).sum() + \
                (n + 2) * eps * (ay[:, i] * ag[:, j] + ay[:, j] * ag[:, i]).sum() + \
                (n + 4) * EPS64 * ((ax[:, i] + ac[i]) * ag[:, j] + (ax[:, j] + ac[j]) * ag[:, i]).sum()
        mol_bound[b, G_MAX] = float(np.sqrt((ab * ab).sum(1)).max()) + 3 * eps * float(norms.max())
    out = VinaGradients(st.atom, st.mol, st.mol_int, st.flag, st.lig_code, st.mol_off, grad, mol_grad, kink_margin)
    return out if eps is None else (out, grad_bound, mol_bound)


def grad_error_bound(lig_x, lig_code, mol_off, mol_group, mol_int, poc_x, poc_code, group_off, eps=EPS32):
    """Forward error bound of a float32 evaluation of the gradient (and so of the kernel, which rounds less: it works in
    float64 from the float32 r on) against the float64 restatement `_vina_grad_host`, evaluated in float64, first order in
    eps.  -> (grad_bound [N, 3], mol_grad_bound [B, 8]); NaN where the molecule is not finite.  Derivation, per counted
    pair with r > 0, f = S u its contribution, S = sum_k w_k T_k'(d):

    d:  dd = 4 eps r + 16 eps, as in `error_bound` (3.5 eps r from the five roundings of r^2 and the root, 16 eps from the
        two subtractions of radii at |values| <= 8).
    S:  |dT_k'| <= sup |T_k''| dd with sup |T''| = 8 (gauss1: |64 d^2 - 8| exp(-4 d^2) peaks at d = 0), 0.5 (gauss2:
        |4 c^2 - 2| exp(-c^2) / 4 peaks at c = 0), 2 (repulsion, where d < 0; counted where d <= dd, since beyond that both
        sides evaluate the branch 0 exactly).  hydrophobic' and hbond' are piecewise constant: a flagged pair
        with |d - kink| <= dd (kinks 0.5 and 1.5, -0.7 and 0) may sit on the other branch, which adds the full jump, 1 or
        1 / 0.7; every other pair adds 0.  The repulsion's kink at d = 0 is a jump of at most 2 dd of a continuous
        derivative: the Lipschitz term above covers it.  Evaluation in float32: a gaussian derivative -8 d E or -c E has
        the relative error of c (eps), of its square (3 eps, on the argument: 3 |arg| eps on E), of the exponential
        (2 eps), of the product (eps) and of the weight (eps) <= (6 + 3 |arg|) eps; the other terms one or two roundings,
        <= 2 eps; the sum of the five, four additions: 4 eps sum_k |w_k T_k'|.  Together
        dS = sum_k |w_k| sup|T_k''| dd + jumps + eps sum_k ((6 + 3 |arg_k|) or 2, + 4) |w_k T_k'|.
    u:  each float32 difference carries eps (one rounding of an exact difference), r carries 3.5 eps, the division eps:
        |du_k| <= 6 eps |u_k| including the second-order terms.
    f:  |df_k| <= dS |u_k| + 6 eps |S u_k| + eps |S u_k| (the product).
    g_i: the sum of the n_i pair terms adds n_i eps sum_j |f_jk| (a float32 running sum; for the kernel, whose sums are
        float64, the float32 carry between tiles: one rounding per tile that holds a counted pair, at most n_i of them,
        and the stored value's own).
    net: sum_i bound(g_i) + n eps sum_i |g_ik| (n atoms; a float32 sum, the kernel's one final rounding).
    moment: with y = x - c, c the mean: |dc_k| <= (n + 1) eps mean_i |x_ik| (a float32 mean), |dy_ik| <= |dc_k| + eps
        |y_ik|; a component y_a g_b - y_b g_a has the error |dy_a| |g_b| + |y_a| bound(g_b) + (a <-> b), its two
        products and the difference 2 eps (|y_a g_b| + |y_b g_a|), and the sum over atoms n eps of the same.  The kernel
        forms sum x_i x g_i - c x sum g_i in float64 instead: the cancellation between the two is exact algebra, its
        roundings are (n + 4) 2^-53 sum_i (|x_ia| + |c_a|) |g_ib| + (a <-> b), the only float64 term kept (it does not
        shrink with y; everywhere else float64 roundings are 2^-29 of a float32 term already counted in full).
    max_norm: |max_i |g_i| - max_i |g_i|'| <= max_i |dg_i| <= max_i |bound(g_i)|_2, and 3 eps max |g_i| for the norm's
        own evaluation and the store.
    rot_factor: a product, a sum, a division: 3 eps |value|."""
    _, grad_bound, mol_bound = _vina_grad_host(lig_x, lig_code, mol_off, mol_group, mol_int, poc_x, poc_code, group_off,
                                               eps=float(eps))
    return grad_bound, mol_bound


# ---- the minimiser: float64 restatement ------------------------------------------------------------------------------------------
def pose_frame(q):
    """R(q) float64 [3, 3] of a unit quaternion (w first), by the formula the kernel uses."""
    w, x, y, z = (float(v) for v in q)
    return np.asarray([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                       [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                       [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]], np.float64)


def pose_coordinates(x0, shift, q):
    """float32((c0 + T) + R(q) s) of the float32 input coordinates x0 [n, 3] (c0 their float64 mean, s = x0 - c0): formed
    in float64, rounded once."""
    x64 = np.asarray(x0, np.float32).reshape(-1, 3).astype(np.float64)
    if not len(x64):
        return x64.astype(np.float32)
    c0 = x64.sum(0) / len(x64)
    s, R = x64 - c0, pose_frame(q)
    origin = c0 + np.asarray(shift, np.float64)
    return np.stack([origin[k] + ((R[k, 0] * s[:, 0] + R[k, 1] * s[:, 1]) + R[k, 2] * s[:, 2]) for k in range(3)], 1).astype(np.float32)


def pose_step(shift, q, F, M, rho2, alpha):
    """The trial pose of one step: T' = T - alpha F, q' = normalise(dq q) with dq the rotation by -alpha M / rho^2 (a
    rotation about the current centroid in world axes; the identity if that vector is 0).  float64."""
    shift, q = np.asarray(shift, np.float64), np.asarray(q, np.float64)
    th = -(alpha * np.asarray(M, np.float64)) / rho2
    angle = float(np.sqrt((th[0] * th[0] + th[1] * th[1]) + th[2] * th[2]))
    dq = np.asarray([1.0, 0.0, 0.0, 0.0])
    if angle > 0.0:
        dq = np.concatenate([[np.cos(0.5 * angle)], (np.sin(0.5 * angle) / angle) * th])
    r = np.asarray([dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2] - dq[3] * q[3],
                    dq[0] * q[1] + dq[1] * q[0] + dq[2] * q[3] - dq[3] * q[2],
                    dq[0] * q[2] - dq[1] * q[3] + dq[2] * q[0] + dq[3] * q[1],
                    dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1] + dq[3] * q[0]])
    return shift - alpha * np.asarray(F, np.float64), r / np.sqrt((r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3]))


def _norm3(v):
    return float(np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))


def _minimize_one(evaluate, x0, step, tol, max_evals):
    """The iteration on one molecule.  `evaluate(x float32 [n, 3])` -> (E float32, F float64 [3], M float64 [3], record):
    inter, the net gradient and its moment about the centroid, rounded to float32 before they are used.  -> (x float32,
    pose [8], energies [4], stat [4], the record of the returned pose)."""
    x0 = np.asarray(x0, np.float32).reshape(-1, 3)
    n = len(x0)
    s = x0.astype(np.float64) - (x0.astype(np.float64).sum(0) / n if n else 0.0)
    rho2 = max(float((s * s).sum() / n), 1.0) if n else 1.0
    rho_max = float(np.sqrt((s * s).sum(1).max())) if n else 0.0
    shift, q = np.zeros(3), np.asarray([1.0, 0.0, 0.0, 0.0])
    x = pose_coordinates(x0, shift, q)
    E, F, M, kept = evaluate(x)                                                  # 1
    evals, accepted, E_start, L, last_L, rejected = 1, 0, E, step, 0.0, False
    while True:
        u = _norm3(F) + rho_max * _norm3(M) / rho2                               # 2
        if not u > 0.0:
            status = 2
            break
        moved = False
        while True:                                                              # 3
            if L < tol:
                status = 1
                break
            if evals >= max_evals:
                status = 0
                break
            trial = pose_step(shift, q, F, M, rho2, L / u)
            xt = pose_coordinates(x0, *trial)
            Et, Ft, Mt, rec = evaluate(xt)
            evals += 1
            if Et < E:                                                           # float32, strict
                (shift, q), x, E, F, M, kept = trial, xt, Et, Ft, Mt, rec
                last_L, L, accepted, rejected, moved = L, min(2.0 * L, step), accepted + 1, False, True
                break
            L, rejected = 0.5 * L, True
        if not moved:
            break
    if rejected:                                                                 # 4: the rows describe the returned pose
        E, F, M, kept = evaluate(x)
        evals += 1
    pose = np.concatenate([shift, q, [rho2]])
    return x, pose, np.asarray([E_start, E, last_L, u], np.float64), np.asarray([status, evals, accepted, 0], np.int32), kept


def _vina_minimize_host(lig_x, lig_code, mol_off, mol_group, mol_int, poc_x, poc_code, group_off, step=MIN_STEP, tol=MIN_TOL,
                        max_evals=MIN_EVALS, trace=None):
    """`dsbdd_vina_minimize` in numpy, the specification of its iteration: the arguments of `_vina_grad_host` and the three
    settings (step and tol rounded to float32 as the C entry takes them).  Per molecule, with x0 its float32 input
    coordinates, c0 their mean, s = x0 - c0, rho^2 = max(sum |s|^2 / n, 1), rho_max = max |s| and the pose (T, q) from (0,
    identity), all float64; an evaluation is `_vina_grad_host` in float64 on the float32-rounded coordinates
    `pose_coordinates(x0, T, q)`, and E = inter, F = net, M = moment are rounded to float32 before any decision:
      1. evaluate the input pose; E_start = E, L = step
      2. u = |F| + rho_max |M| / rho^2; unless u > 0 stop, status 2
      3. L < tol: stop, status 1; max_evals evaluations made: stop, status 0; else the trial `pose_step` with alpha = L / u
         (no atom moves more than L); evaluate; E' < E (float32, strict): take it, L = min(2 L, step), go to 2; else
         L = L / 2, repeat 3
      4. after a stop on a rejected trial the accepted pose is evaluated once more (counted; the only evaluation beyond
         max_evals)
    A molecule with a coordinate that is not finite: status 3, x the input, NaN in its other floats, the flag.  Only the pocket
    atoms inside the ligand's bounding box widened by 8.5 A are handed to an evaluation (no other can be within the cutoff).
    -> VinaMinimized of arrays: the fields of `_vina_grad_host` (float64) at the returned pose, x float32 [N, 3] (rows of
    no molecule: the input), pose [B, 8] and energies [B, 4] float64, stat int32 [B, 4], x_in; the inherited `kink_margin` is
    not evaluated here (it stays inf: `_vina_grad_host` forms it only with its error bound, on `x` if it is wanted).  `trace`: a list that
    receives (molecule, E float32) for every evaluation, in order."""
    step, tol, max_evals = _settings(step, tol, max_evals)
    x_in = np.asarray(_np(lig_x), np.float32).reshape(-1, 3)
    code = np.asarray(_np(lig_code), np.int32).reshape(-1)
    q_all = np.asarray(_np(poc_x), np.float32).reshape(-1, 3)
    qcode = np.asarray(_np(poc_code), np.int32).reshape(-1)
    off = np.asarray(_np(mol_off), np.int64).reshape(-1)
    goff = np.asarray(_np(group_off), np.int64).reshape(-1)
    ints = np.asarray(_np(mol_int), np.int32).reshape(-1, MOL_INT)
    groups = np.asarray(_np(mol_group), np.int64).reshape(-1)
    B, G, N = len(off) - 1, len(goff) - 1, len(x_in)
    if len(code) != N or len(qcode) != len(q_all) or len(groups) != B or len(ints) != B:
        raise ValueError("one code per atom, one group and one mol_int row per molecule")
    out = VinaMinimized(np.zeros((N, ATOM_OUT)), np.zeros((B, MOL_OUT)), ints, np.zeros(B, np.int32), code, off.astype(np.int32),
                        np.zeros((N, ATOM_GRAD)), np.zeros((B, MOL_GRAD)), float("inf"), x_in.copy(), np.zeros((B, MOL_POSE)),
                        np.zeros((B, MOL_MIN)), np.zeros((B, MOL_STAT), np.int32), x_in)
    for b in range(B):
        lo, hi = int(off[b]), int(off[b + 1])
        if not (lo >= 0 and hi >= lo and hi <= off[B]):
            lo = hi = 0
        g = int(groups[b])
        glo, ghi = (int(goff[g]), int(goff[g + 1])) if 0 <= g < G else (0, 0)
        if not (glo >= 0 and ghi >= glo and ghi <= goff[G]):
            glo = ghi = 0
        x0, c, one = x_in[lo:hi], code[lo:hi], np.asarray([0, hi - lo], np.int64)
        qg, qc = q_all[glo:ghi], qcode[glo:ghi]

        def evaluate(x):
            near = np.ones(len(qg), bool)
            if len(x) and len(qg) and np.isfinite(x).all():
                low, high = x.astype(np.float64).min(0) - (CUTOFF + 0.5), x.astype(np.float64).max(0) + (CUTOFF + 0.5)
                near = ((qg >= low) & (qg <= high)).all(1)
            st = _vina_grad_host(x, c, one, [0], ints[b:b + 1], qg[near], qc[near], [0, int(near.sum())])
            E = np.float32(st.mol[0, M_INTER])
            if trace is not None:
                trace.append((b, E))
            return E, st.mol_grad[0, G_NET].astype(np.float32).astype(np.float64), \
                st.mol_grad[0, G_MOMENT].astype(np.float32).astype(np.float64), st

        if not np.isfinite(x0).all():
            st = evaluate(x0)[3]
            pose, energies, stat = np.full(MOL_POSE, np.nan), np.full(MOL_MIN, np.nan), np.asarray([3, 0, 0, 0], np.int32)
        else:
            x, pose, energies, stat, st = _minimize_one(evaluate, x0, step, tol, max_evals)
            out.x[lo:hi] = x
        out.atom[lo:hi], out.grad[lo:hi] = st.atom, st.grad
        out.mol[b], out.flag[b], out.mol_grad[b] = st.mol[0], st.flag[0], st.mol_grad[0]
        out.pose[b], out.energies[b], out.stat[b] = pose, energies, stat
    return out


# ---- torsion tree and intramolecular term ------------------------------------------------------------------------------------
def pack_masks(bits):
    """bool [..., k <= 128] -> int32 [..., 4]: atom 32 w + b is bit b of word w (the kernels' 128-bit masks)."""
    bits = np.asarray(bits, bool)
    full = np.zeros(bits.shape[:-1] + (32 * MASK_WORDS,), bool)
    full[..., :bits.shape[-1]] = bits
    return np.ascontiguousarray(np.packbits(full, axis=-1, bitorder="little")).view("<u4").astype(np.uint32).view(np.int32)


def unpack_masks(words, n):
    """int32 [k, 4] -> bool [k, n]: the first n bits of every mask; a bit at or above 128 is not set."""
    words = np.ascontiguousarray(np.asarray(_np(words), np.int32).reshape(-1, MASK_WORDS))
    bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little").astype(bool)
    out = np.zeros((len(words), n), bool)
    out[:, :min(n, bits.shape[1])] = bits[:, :n]
    return out


def torsion_tree(classes, sym, keep=MAX_TORSIONS):
    """The torsion tree of one molecule: `classes`, `sym` as for `type_graph`; `keep` = how many rotors are kept (0 for a
    molecule that is to stay rigid).  -> (rotors, found, pairs): `rotors` the kept ones in ascending (a, c) as (fixed end
    p, moving end m, side bool [n]); `found` the number of all rotors (= `type_graph`'s n_rot); `pairs` bool [n, n], the
    pairs of the intramolecular term.
    Rotor: a single bond (a, c), c < a, both ends of heavy degree >= 2, in no ring.  Side: cut the bond; of the two
    components its ends fall into, the one with fewer atoms, on a tie the one of a (the higher index).  Any two sides are
    nested or disjoint (two sides of at most half a component each cannot overlap without one containing the other).
    pairs[i, j]: i != j, both typed, more than 3 bonds apart or not connected, and exactly one of them in the side of some
    kept rotor."""
    classes = np.asarray(classes, np.int64).reshape(-1)
    n = len(classes)
    sym = np.asarray(sym, np.int64).reshape(n, n)
    sym = np.where((sym >= 1) & (sym <= 3), sym, 0)
    classes = np.where((classes >= 0) & (classes <= C_METAL), classes, C_NONE)
    bonded = sym > 0
    deg = bonded.sum(1)
    nbrs = [np.nonzero(bonded[a])[0].tolist() for a in range(n)]
    bonds = [(a, c) for a in range(n) for c in nbrs[a]
             if c < a and sym[a, c] == 1 and deg[a] >= 2 and deg[c] >= 2 and not _bond_in_ring(nbrs, a, c)]

    def component(a, c):                                                        # of a, the bond (a, c) left out
        seen, front = {a}, [a]
        while front:
            nxt = [v for u in front for v in nbrs[u] if not (u == a and v == c)]
            front = list(set(nxt) - seen)
            seen |= set(front)
        return seen

    rotors = []
    for a, c in bonds[:max(int(keep), 0)]:
        of_a, of_c = component(a, c), component(c, a)
        side = np.zeros(n, bool)
        if len(of_a) <= len(of_c):
            side[list(of_a)] = True
            rotors.append((c, a, side))
        else:
            side[list(of_c)] = True
            rotors.append((a, c, side))
    cut = np.zeros((n, n), bool)
    for _, _, side in rotors:
        cut |= side[:, None] != side[None, :]
    step = bonded | np.eye(n, dtype=bool)
    near = step.copy()
    for _ in range(2):
        near = (near.astype(np.int64) @ step.astype(np.int64)) > 0
    typed = classes != C_NONE
    return rotors, len(bonds), cut & ~near & typed[:, None] & typed[None, :]


@dataclass
class VinaTorsions:
    """The outputs of `dsbdd_vina_torsions` (device tensors from `ligand_torsions`, numpy arrays from `_vina_torsions_host`)."""
    ints: object             # int32 [B, 4]: rotors kept, rotors found, 0, 0
    ends: object             # int32 [B, 32, 2]: fixed end, moving end; -1 past the kept
    sides: object            # int32 [B, 32, 4]: the moving side as a 128-bit mask; 0 past the kept
    pair_mask: object        # int32 [N, 4]: the partners of every atom in the intramolecular term
    mol_off: object          # int32 [B + 1]

    kept = property(lambda self: self.ints[:, T_KEPT])
    found = property(lambda self: self.ints[:, T_FOUND])


def _vina_torsions_host(order, atom_type, mol_off, class_elem, fill=0):
    """`dsbdd_vina_torsions` in numpy (integers; exact, the specification): the arguments of `_vina_type_host`.
    -> VinaTorsions of arrays.  A molecule longer than n_max keeps no rotor (`found` is counted on its first n_max atoms, as
    `_vina_type_host` counts N_rot) and the masks of all its atoms are 0; rows of `pair_mask` that belong to no valid molecule
    keep `fill`."""
    order = np.asarray(_np(order))
    B, n_max = order.shape[0], order.shape[1]
    at = np.asarray(_np(atom_type), np.int64).reshape(-1)
    off = np.asarray(_np(mol_off), np.int64).reshape(-1)
    table = np.asarray(_np(class_elem), np.int64).reshape(-1)
    if len(off) != B + 1:
        raise ValueError(f"{len(off)} offsets for {B} molecules")
    out = VinaTorsions(np.zeros((B, TOR_INT), np.int32), np.full((B, MAX_TORSIONS, 2), -1, np.int32),
                       np.zeros((B, MAX_TORSIONS, MASK_WORDS), np.int32), np.full((len(at), MASK_WORDS), fill, np.int32),
                       off.astype(np.int32))
    n_total = off[B]
    for b in range(B):
        lo, hi = int(off[b]), int(off[b + 1])
        size = hi - lo if (lo >= 0 and hi >= lo and hi <= n_total) else 0
        n = min(size, n_max)
        t = at[lo:lo + n]
        ok = (t >= 0) & (t < len(table))
        classes = np.where(ok, table[np.where(ok, t, 0)], C_NONE)
        low = np.tril(order[b, :n, :n].astype(np.int64), -1)
        rotors, found, pairs = torsion_tree(classes, low + low.T, 0 if size > n_max else MAX_TORSIONS)
        out.ints[b, :2] = len(rotors), found
        for k, (p, m, side) in enumerate(rotors):
            out.ends[b, k] = p, m
            out.sides[b, k] = pack_masks(side)
        out.pair_mask[lo:lo + size] = 0
        if n:
            out.pair_mask[lo:lo + n] = pack_masks(pairs)
    return out


def ligand_torsions(x, atom_type, lig_mask, info, orders=None, batch=None):
    """The torsion tree and the intramolecular pair masks of a batch on the device: one launch of `dsbdd_vina_torsions`
    (csrc/vina_torsion.h) on the inputs of `type_ligands` (the same arguments; x is read only to perceive `orders` when none
    are given).  -> VinaTorsions of device tensors.  `_vina_torsions_host` / `torsion_tree` state what it computes."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.HipLibraryError("ligand_torsions needs device tensors (HIP path; no CPU fallback)")
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
    out = VinaTorsions(torch.zeros((B, TOR_INT), **i32), torch.full((B, MAX_TORSIONS, 2), -1, **i32),
                       torch.zeros((B, MAX_TORSIONS, MASK_WORDS), **i32), torch.zeros((N, MASK_WORDS), **i32), off)
    if B == 0:
        return out
    orders = _perceived_orders(x, at, lig_mask, info, B) if orders is None else \
        torch.as_tensor(orders, device=dev).to(torch.int8).contiguous()
    if orders.dim() != 3 or orders.shape[0] != B or orders.shape[1] != orders.shape[2] or \
            not 1 <= orders.shape[1] <= _lib.MOL_MAX_ATOMS:
        raise ValueError(f"orders must be [{B}, n_max, n_max] with n_max in [1, {_lib.MOL_MAX_ATOMS}], got {tuple(orders.shape)}")
    table = torch.as_tensor(class_table(decoder), device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.dsbdd_vina_torsions(stream, orders.data_ptr(), _ptr(at), off.data_ptr(), B, len(decoder), table.data_ptr(),
                                 int(orders.shape[1]), out.ints.data_ptr(), out.ends.data_ptr(), out.sides.data_ptr(),
                                 _ptr(out.pair_mask))
    _lib.check(rc, "dsbdd_vina_torsions")
    return out


@dataclass
class MolVinaIntra:
    """The intramolecular record of one molecule (host arrays)."""
    mol: np.ndarray          # float32 [8]: the five term sums (every pair once), intra, 0, 0
    atom: np.ndarray         # float32 [n, 5]: the unweighted terms of every atom over its partners
    grad: np.ndarray         # float32 [n, 3]: d intra / d x_i, kcal/mol/A
    n_torsions: int = 0      # rotors kept
    torsions_found: int = 0
    nonfinite: int = 0

    terms = property(lambda self: self.mol[:ATOM_OUT])
    intra = property(lambda self: float(self.mol[M_INTER]))


@dataclass
class VinaIntra:
    """The outputs of `dsbdd_vina_intra` (device tensors from `vina_intra`, numpy arrays from `_vina_intra_host`)."""
    atom: object             # float [N, 5]
    mol: object              # float [B, 8]: the five sums with every pair counted once, intra, 0, 0
    flag: object             # int32 [B]
    grad: object             # float [N, 3]: d intra / d x_i
    mol_off: object          # int32 [B + 1]
    torsions: object = None  # VinaTorsions (`vina_intra` only)

    terms = property(lambda self: self.mol[:, :ATOM_OUT])
    intra = property(lambda self: self.mol[:, M_INTER])
    nonfinite = property(lambda self: self.flag)

    def molecules(self):
        """One `MolVinaIntra` per molecule, in order (one copy of each tensor to the host)."""
        atom, mol, flag, grad, off = (_np(v) for v in (self.atom, self.mol, self.flag, self.grad, self.mol_off))
        ints = np.zeros((len(mol), TOR_INT), np.int32) if self.torsions is None else _np(self.torsions.ints)
        return [MolVinaIntra(mol[b].copy(), atom[off[b]:off[b + 1]].copy(), grad[off[b]:off[b + 1]].copy(), int(ints[b, T_KEPT]),
                             int(ints[b, T_FOUND]), int(flag[b])) for b in range(len(mol))]


def _intra_as_groups(lig_x, lig_code, mol_off):
    """The arguments of `_vina_score_host` that make every molecule its own pocket group."""
    off = np.asarray(_np(mol_off), np.int64).reshape(-1)
    B = len(off) - 1
    return (lig_x, lig_code, off, np.arange(B), np.zeros((B, MOL_INT), np.int32), lig_x, lig_code, off)


def _vina_intra_host(lig_x, lig_code, mol_off, pair_mask, dtype=np.float64, eps=None):
    """`dsbdd_vina_intra` in numpy: `_vina_grad_host` with every molecule as its own pocket group, over the pairs listed in
    `pair_mask` (int32 [N, 4]) alone; float32 coordinates, the counted pairs decided by the float32 distance, everything
    else in `dtype` (float64: the specification).  Per molecule the five sums are HALF the sums over the atoms (every
    pair is met from both ends), intra = sum_k WEIGHTS[k] T_k, columns 6 and 7 are 0.  -> (VinaIntra of arrays in `dtype`,
    the smallest |r - 8| over the listed pairs).  With `eps` also the bounds of `intra_error_bound`: (..., atom_bound
    [N, 5], mol_bound [B, 6], grad_bound [N, 3])."""
    mask = np.asarray(_np(pair_mask), np.int32).reshape(-1, MASK_WORDS)
    args = _intra_as_groups(lig_x, lig_code, mol_off)
    if eps is None:
        g = _vina_grad_host(*args, dtype=dtype, pair_mask=mask)
        _, margin = _vina_score_host(*args, dtype=dtype, pair_mask=mask)
    else:
        g, grad_bound, _ = _vina_grad_host(*args, dtype=dtype, eps=eps, pair_mask=mask)
        _, margin, atom_bound, mol_bound = _vina_score_host(*args, dtype=dtype, eps=eps, pair_mask=mask)
    mol = g.mol.copy()
    mol[:, :ATOM_OUT] *= dtype(0.5)
    mol[:, M_INTER] = (mol[:, :ATOM_OUT] * np.asarray(WEIGHTS, dtype)).sum(1)
    mol[:, M_SCORE:] = np.where(np.isnan(mol[:, M_INTER:M_INTER + 1]), dtype(np.nan), dtype(0))
    out = VinaIntra(g.atom, mol, g.flag, g.grad, g.mol_off)
    if eps is None:
        return out, margin
    half = 0.5 * mol_bound[:, :M_INTER + 1] + eps * np.abs(mol[:, :M_INTER + 1].astype(np.float64))
    return out, margin, atom_bound, half, grad_bound


def intra_error_bound(lig_x, lig_code, mol_off, pair_mask, eps=EPS32):
    """Forward error bound of a float32 evaluation of the intramolecular term (and so of the kernel, which rounds less: float64
    from the float32 r on) against `_vina_intra_host` in float64.  The pairs are ligand-ligand, the arithmetic per pair is
    that of `dsbdd_vina_score_grad` with the partner's float32 coordinates and code in the pocket atom's place, so the
    derivations of `error_bound` (terms) and `grad_error_bound` (gradient) hold pair for pair: per atom they are taken
    over as they stand, the sums running over the atom's listed partners.  Per molecule the value is half the sum over all
    ordered pairs: half the bound of that sum (the halving is exact), plus eps |value| for the one rounding of the stored
    float32 that the halved value gets on its own; intra: sum_k |w_k| bound_k, halved the same way, plus eps |intra|.
    -> (atom_bound [N, 5], mol_bound [B, 6], grad_bound [N, 3]); NaN where the molecule is not finite."""
    return _vina_intra_host(lig_x, lig_code, mol_off, pair_mask, eps=float(eps))[2:]


def vina_intra(x, atom_type, lig_mask, info, batch=None, orders=None):
    """The intramolecular term of a batch and its gradient with respect to x, on device tensors: bond orders (unless
    given), `dsbdd_vina_type`, `dsbdd_vina_torsions`, `dsbdd_vina_intra`; no read-back inside.  Arguments as for
    `type_ligands`.  -> VinaIntra of device tensors, with the tree as `.torsions`.  A molecule without rotors (or longer
    than 128 atoms) has no pair and gives exact zeros.  See `VINA_INTRA_COVERAGE`."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.HipLibraryError("vina_intra needs device tensors (HIP path; no CPU fallback)")
    lib = _lib.load()
    dev = x.device
    x = x.detach().to(torch.float32).reshape(-1, 3).contiguous()
    N = int(x.shape[0])
    lig_mask = torch.as_tensor(lig_mask, device=dev).reshape(-1)
    B = _n_molecules(lig_mask, batch)
    if orders is None and B:
        orders = perceive_orders(x, atom_type, lig_mask, info, batch=B)
    code, _, off = type_ligands(x, atom_type, lig_mask, info, orders=orders, batch=B)
    tree = ligand_torsions(x, atom_type, lig_mask, info, orders=orders, batch=B)
    f32 = dict(dtype=torch.float32, device=dev)
    out = VinaIntra(torch.zeros((N, ATOM_OUT), **f32), torch.zeros((B, MOL_OUT), **f32),
                    torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros((N, ATOM_GRAD), **f32), off, tree)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.dsbdd_vina_intra(stream, _ptr(x), _ptr(code), off.data_ptr(), B, _ptr(tree.pair_mask), _ptr(out.atom),
                              _ptr(out.mol), _ptr(out.flag), _ptr(out.grad))
    _lib.check(rc, "dsbdd_vina_intra")
    return out


def intra_molecules(molecules, info="crossdock", device="cuda", bonds="distance"):
    """Intramolecular records of written molecules (`as_ligands` forms) through the launches of `vina_intra`; `info`,
    `device` and `bonds` as for `score_molecules`.  -> list of `MolVinaIntra`."""
    def entry(x, at, mask, pockets, info, mol_group, batch=None, orders=None):
        return vina_intra(x, at, mask, info, batch=batch, orders=orders)
    return _molecule_records(entry, "intra_molecules", molecules, None, info, None, device, bonds)


# ---- the flexible minimiser ---------------------------------------------------------------------------------------------------
@dataclass
class MolVinaFlex(MolVinaMin):
    """`MolVinaMin` at the pose the flexible minimiser returned (host arrays): `inter`, `score` and the gradient stay the
    intermolecular ones, the intramolecular term is reported beside them.  `energies` float [8]: inter at the start, at the
    end, the last accepted step, u at the end, intra at the start, at the end, E = inter + intra at the start, at the end."""
    intra_rec: MolVinaIntra = None    # the intramolecular record at the returned pose
    theta: np.ndarray = None          # float32 [32]: the torsion angles (rad) in the slots of the tree; 0 where no rotor stands
    tau: np.ndarray = None            # float32 [32]: d E / d theta_k at the returned pose

    intra = property(lambda self: self.intra_rec.intra)
    intra_start = property(lambda self: float(self.energies[X_INTRA_START]))
    n_torsions = property(lambda self: self.intra_rec.n_torsions)
    torsions_found = property(lambda self: self.intra_rec.torsions_found)

    def as_dict(self):
        out = super().as_dict()
        out.update(intra=self.intra, intra_start=self.intra_start, n_torsions=self.n_torsions, torsions_found=self.torsions_found)
        return out


@dataclass
class VinaFlexed(VinaMinimized):
    """`VinaMinimized` at the poses the flexible minimiser returned (device tensors from `vina_minimize(torsions=True)`,
    numpy arrays from `_vina_flex_host`); `energies` is [B, 8] (see `MolVinaFlex`)."""
    intra_out: object = None  # VinaIntra at the returned poses, with the tree as `.torsions`
    theta: object = None      # float [B, 32]
    tau: object = None        # float [B, 32]

    intra = property(lambda self: self.intra_out.intra)
    intra_start = property(lambda self: self.energies[:, X_INTRA_START])
    n_torsions = property(lambda self: self.intra_out.torsions.kept)
    torsions_found = property(lambda self: self.intra_out.torsions.found)

    def molecules(self):
        """One `MolVinaFlex` per molecule, in order (one copy of each tensor to the host)."""
        theta, tau = _np(self.theta), _np(self.tau)
        return [MolVinaFlex(m.mol, m.ints, m.atom, m.code, m.nonfinite, m.grad, m.mol_grad, m.x, m.pose, m.energies, m.stat,
                            m.rmsd, r, theta[b].copy(), tau[b].copy())
                for b, (m, r) in enumerate(zip(VinaMinimized.molecules(self), self.intra_out.molecules()))]


def valid_torsions(tree, b, n, dofs=DOF_RIGID | DOF_TORSIONS):
    """The rotors of molecule b (n atoms) of a `VinaTorsions` of arrays that `dsbdd_vina_flex` turns, as it checks them: none
    without the torsion bit of `dofs` or with n > 128; the kept count clamped to [0, 32]; a rotor whose ends are not two
    different atoms of the molecule dropped; side bits at or above n cleared.  -> list of (p, m, side bool [n], slot)."""
    if not (dofs & DOF_TORSIONS) or n > _lib.MOL_MAX_ATOMS:
        return []
    kept = min(max(int(_np(tree.ints)[b, T_KEPT]), 0), MAX_TORSIONS)
    ends, sides = _np(tree.ends)[b], _np(tree.sides)[b]
    out = []
    for k in range(kept):
        p, m = int(ends[k, 0]), int(ends[k, 1])
        if 0 <= p < n and 0 <= m < n and p != m:
            out.append((p, m, unpack_masks(sides[k:k + 1], n)[0], k))
    return out


def _torsion_frame(x0, torsions, theta):
    """y float64 [n, 3]: the input with every side turned, in list order, by the formula the kernel uses."""
    y = np.asarray(x0, np.float32).reshape(-1, 3).astype(np.float64)
    for rotor, angle in zip(torsions, theta):
        p, m, side = rotor[:3]
        angle = float(angle)
        o = y[m].copy()
        ax = o - y[p]
        length = float(np.sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]))
        if angle == 0.0 or not length > 0.0:
            continue
        ax = ax / length
        cs, sn = np.cos(angle), np.sin(angle)
        v = y[side] - o
        along = ((ax[0] * v[:, 0] + ax[1] * v[:, 1]) + ax[2] * v[:, 2]) * (1.0 - cs)
        cr = np.stack([ax[(k + 1) % 3] * v[:, (k + 2) % 3] - ax[(k + 2) % 3] * v[:, (k + 1) % 3] for k in range(3)], 1)
        y[side] = o + ((v * cs + cr * sn) + ax[None, :] * along[:, None])
    return y


def torsion_coordinates(x0, torsions, theta, shift=(0.0, 0.0, 0.0), q=(1.0, 0.0, 0.0, 0.0)):
    """float32(t + R(q) y) of the float32 input coordinates x0 [n, 3]: y = x0 in float64, then for every rotor of `torsions`
    ((p, m, side bool [n], ...) tuples) in list order the atoms of its side turn by its `theta` about the line from y[p]
    through y[m] as it stands (a rotor with theta = 0 or coinciding ends is skipped); rounded once.  The sides being nested
    or disjoint, the result does not depend on the list order beyond the float64 roundings."""
    y = _torsion_frame(x0, torsions, theta)
    R, t = pose_frame(q), np.asarray(shift, np.float64)
    return np.stack([t[k] + ((R[k, 0] * y[:, 0] + R[k, 1] * y[:, 1]) + R[k, 2] * y[:, 2]) for k in range(3)], 1).astype(np.float32)


def flex_geometry(x, torsions, grad):
    """The scales and torques of an accepted pose: x float32 [n, 3] its coordinates, `grad` [n, 3] = g^inter + g^intra.
    -> (c [3], rho2, rho_max, tau [K], reach [K], rho2k [K]) in float64: c the mean of x, rho^2 = max(mean |x - c|^2, 1),
    rho_max = max |x - c|; per rotor a = the unit vector from x[p] to x[m], tau = a . sum_{i in S} (x_i - x[m]) x grad_i,
    reach = the largest distance of an atom of S from the axis, rho2k = max(mean over S of that distance squared, 1); a
    rotor whose ends coincide has tau = reach = 0."""
    x = np.asarray(x, np.float32).reshape(-1, 3).astype(np.float64)
    g = np.asarray(grad, np.float64).reshape(-1, 3)
    n, K = len(x), len(torsions)
    c = x.sum(0) / n if n else np.zeros(3)
    s2 = ((x - c) ** 2).sum(1)
    rho2 = max(float(s2.sum() / n), 1.0) if n else 1.0
    rho_max = float(np.sqrt(s2.max())) if n else 0.0
    tau, reach, rho2k = np.zeros(K), np.zeros(K), np.ones(K)
    for k, rotor in enumerate(torsions):
        p, m, side = rotor[:3]
        ax = x[m] - x[p]
        length = _norm3(ax)
        if not length > 0.0 or not side.any():
            continue
        ax = ax / length
        v = x[side] - x[m]
        tau[k] = float((np.cross(v, g[side]) @ ax).sum())
        d2 = (np.cross(v, ax) ** 2).sum(1)
        reach[k], rho2k[k] = float(np.sqrt(d2.max())), max(float(d2.sum() / len(d2)), 1.0)
    return c, rho2, rho_max, tau, reach, rho2k


def flex_slope(F, M, rho2, rho_max, tau, reach, rho2k, dofs=DOF_RIGID | DOF_TORSIONS):
    """u = |F| + rho_max |M| / rho^2 + sum_k reach_k |tau_k| / rho2k_k, a switched-off block left out."""
    u = _norm3(F) + rho_max * _norm3(M) / rho2 if dofs & DOF_RIGID else 0.0
    for k in range(len(tau)):
        u += reach[k] * abs(tau[k]) / rho2k[k]
    return u


def flex_step(shift, q, theta, F, M, tau, c, rho2, rho2k, alpha, dofs=DOF_RIGID | DOF_TORSIONS):
    """The trial of one step from the accepted pose (t, q, theta) whose coordinates have the mean c: with the rigid bit of
    `dofs` the rotation dq by -alpha M / rho^2 about c and the translation -alpha F, q' = normalise(dq q), t' = c + R(dq)(t - c)
    - alpha F (else t, q as they are); theta' = theta - alpha tau / rho2k (`tau` holds only the rotors that turn).  float64.
    -> (t', q', theta')."""
    shift, q = np.asarray(shift, np.float64), np.asarray(q, np.float64)
    theta = np.asarray(theta, np.float64) - (alpha * np.asarray(tau, np.float64)) / np.asarray(rho2k, np.float64)
    if not dofs & DOF_RIGID:
        return shift.copy(), q.copy(), theta
    th = -(alpha * np.asarray(M, np.float64)) / rho2
    angle = float(np.sqrt((th[0] * th[0] + th[1] * th[1]) + th[2] * th[2]))
    dq = np.asarray([1.0, 0.0, 0.0, 0.0])
    if angle > 0.0:
        dq = np.concatenate([[np.cos(0.5 * angle)], (np.sin(0.5 * angle) / angle) * th])
    _, q1 = pose_step(np.zeros(3), q, np.zeros(3), M, rho2, alpha)
    R, s, c = pose_frame(dq), shift - np.asarray(c, np.float64), np.asarray(c, np.float64)
    t1 = np.asarray([(c[k] + ((R[k, 0] * s[0] + R[k, 1] * s[1]) + R[k, 2] * s[2])) - alpha * float(F[k]) for k in range(3)])
    return t1, q1, theta


def _flex_one(evaluate, x0, torsions, step, tol, max_evals, dofs):
    """The iteration on one molecule.  `evaluate(x float32 [n, 3])` -> (inter float32, intra float32, F [3], M [3], g [n, 3],
    record): the two energies as stored, the net gradient and its moment about the centroid rounded to float32, the sum of
    the two float32 gradients.  -> (x, pose [8], energies [8], stat [4], theta [K], tau [K], record of the returned pose)."""
    x0 = np.asarray(x0, np.float32).reshape(-1, 3)
    K = len(torsions)
    shift, q, theta = np.zeros(3), np.asarray([1.0, 0.0, 0.0, 0.0]), np.zeros(K)
    x = torsion_coordinates(x0, torsions, theta, shift, q)
    inter, intra, F, M, g, kept = evaluate(x)
    E = float(inter) + float(intra)
    evals, accepted, E_start, L, last_L, rejected = 1, 0, E, step, 0.0, False
    inter_start, intra_start = inter, intra
    while True:
        c, rho2, rho_max, tau, reach, rho2k = flex_geometry(x, torsions, g)
        u = flex_slope(F, M, rho2, rho_max, tau, reach, rho2k, dofs)
        if not u > 0.0:
            status = 2
            break
        moved = False
        while True:
            if L < tol:
                status = 1
                break
            if evals >= max_evals:
                status = 0
                break
            trial = flex_step(shift, q, theta, F, M, tau, c, rho2, rho2k, L / u, dofs)
            xt = torsion_coordinates(x0, torsions, trial[2], trial[0], trial[1])
            it, at, Ft, Mt, gt, rec = evaluate(xt)
            evals += 1
            if float(it) + float(at) < E:
                (shift, q, theta), x, E, F, M, g, kept = trial, xt, float(it) + float(at), Ft, Mt, gt, rec
                last_L, L, accepted, rejected, moved = L, min(2.0 * L, step), accepted + 1, False, True
                break
            L, rejected = 0.5 * L, True
        if not moved:
            break
    if rejected:
        kept = evaluate(x)[5]
        evals += 1
    pose = np.concatenate([shift, q, [rho2]])
    inter_final, intra_final = float(np.float32(kept[0].mol[0, M_INTER])), float(np.float32(kept[1].mol[0, M_INTER]))
    energies = np.asarray([inter_start, inter_final, last_L, u, intra_start, intra_final, E_start, E], np.float64)
    return x, pose, energies, np.asarray([status, evals, accepted, 0], np.int32), theta, tau, kept


def _vina_flex_host(lig_x, lig_code, mol_off, mol_group, mol_int, poc_x, poc_code, group_off, tree, dofs=DOF_RIGID | DOF_TORSIONS,
                    step=MIN_STEP, tol=MIN_TOL, max_evals=MIN_EVALS, trace=None):
    """`dsbdd_vina_flex` in numpy, the specification of its iteration: the arguments of `_vina_minimize_host`, `tree` a
    `VinaTorsions` of arrays (what `_vina_torsions_host` returns), `dofs` bit 0 = the rigid body, bit 1 = the torsions.  Per
    molecule, with the rotors `valid_torsions` keeps and the pose (t, q, theta) from (0, identity, 0), all float64:
    an evaluation is `_vina_grad_host` and `_vina_intra_host` in float64 on the float32-rounded coordinates
    `torsion_coordinates(x0, rotors, theta, t, q)`; inter, intra, F = net, M = moment and the two gradients are rounded to
    float32 before any use, and E = inter + intra is their float64 sum:
      1. evaluate the input pose; E_start = E, L = step
      2. at the accepted pose `flex_geometry`, u = `flex_slope`; unless u > 0 stop, status 2
      3. L < tol: stop, status 1; max_evals evaluations made: stop, status 0; else the trial `flex_step` with alpha = L / u
         (no atom moves more than L); evaluate; E' < E (strict): take it, L = min(2 L, step), go to 2; else L = L / 2, repeat 3
      4. after a stop on a rejected trial the accepted pose is evaluated once more (counted; the only evaluation beyond
         max_evals)
    A molecule with a coordinate that is not finite: status 3, x the input, NaN in its other floats, both flags.
    -> VinaFlexed of arrays: the fields of `_vina_minimize_host`, energies [B, 8], `intra_out` (a VinaIntra in float64 with
    the tree), theta and tau [B, 32] in the slots of the tree.  `trace`: a list that receives (molecule, E) per evaluation."""
    step, tol, max_evals = _settings(step, tol, max_evals)
    if dofs not in (1, 2, 3):
        raise ValueError("dofs must be 1, 2 or 3")
    x_in = np.asarray(_np(lig_x), np.float32).reshape(-1, 3)
    code = np.asarray(_np(lig_code), np.int32).reshape(-1)
    q_all = np.asarray(_np(poc_x), np.float32).reshape(-1, 3)
    qcode = np.asarray(_np(poc_code), np.int32).reshape(-1)
    off = np.asarray(_np(mol_off), np.int64).reshape(-1)
    goff = np.asarray(_np(group_off), np.int64).reshape(-1)
    ints = np.asarray(_np(mol_int), np.int32).reshape(-1, MOL_INT)
    groups = np.asarray(_np(mol_group), np.int64).reshape(-1)
    pair_mask = np.asarray(_np(tree.pair_mask), np.int32).reshape(-1, MASK_WORDS)
    B, G, N = len(off) - 1, len(goff) - 1, len(x_in)
    if len(code) != N or len(qcode) != len(q_all) or len(groups) != B or len(ints) != B or len(pair_mask) != N:
        raise ValueError("one code and one pair mask per atom, one group and one mol_int row per molecule")
    intra = VinaIntra(np.zeros((N, ATOM_OUT)), np.zeros((B, MOL_OUT)), np.zeros(B, np.int32), np.zeros((N, ATOM_GRAD)),
                      off.astype(np.int32), tree)
    out = VinaFlexed(np.zeros((N, ATOM_OUT)), np.zeros((B, MOL_OUT)), ints, np.zeros(B, np.int32), code, off.astype(np.int32),
                     np.zeros((N, ATOM_GRAD)), np.zeros((B, MOL_GRAD)), float("inf"), x_in.copy(), np.zeros((B, MOL_POSE)),
                     np.zeros((B, MOL_FLEX)), np.zeros((B, MOL_STAT), np.int32), x_in, intra, np.zeros((B, MAX_TORSIONS)),
                     np.zeros((B, MAX_TORSIONS)))
    for b in range(B):
        lo, hi = int(off[b]), int(off[b + 1])
        if not (lo >= 0 and hi >= lo and hi <= off[B]):
            lo = hi = 0
        g = int(groups[b])
        glo, ghi = (int(goff[g]), int(goff[g + 1])) if 0 <= g < G else (0, 0)
        if not (glo >= 0 and ghi >= glo and ghi <= goff[G]):
            glo = ghi = 0
        x0, c, one = x_in[lo:hi], code[lo:hi], np.asarray([0, hi - lo], np.int64)
        qg, qc, pm = q_all[glo:ghi], qcode[glo:ghi], pair_mask[lo:hi]
        rotors = valid_torsions(tree, b, hi - lo, dofs)

        def evaluate(x):
            near = np.ones(len(qg), bool)
            if len(x) and len(qg) and np.isfinite(x).all():
                low, high = x.astype(np.float64).min(0) - (CUTOFF + 0.5), x.astype(np.float64).max(0) + (CUTOFF + 0.5)
                near = ((qg >= low) & (qg <= high)).all(1)
            st = _vina_grad_host(x, c, one, [0], ints[b:b + 1], qg[near], qc[near], [0, int(near.sum())])
            si, _ = _vina_intra_host(x, c, one, pm)
            inter, intra_e = np.float32(st.mol[0, M_INTER]), np.float32(si.mol[0, M_INTER])
            if trace is not None:
                trace.append((b, float(inter) + float(intra_e)))
            r32 = lambda v: np.asarray(v).astype(np.float32).astype(np.float64)
            return inter, intra_e, r32(st.mol_grad[0, G_NET]), r32(st.mol_grad[0, G_MOMENT]), r32(st.grad) + r32(si.grad), (st, si)

        if not np.isfinite(x0).all():
            st, si = evaluate(x0)[5]
            pose, energies, stat = np.full(MOL_POSE, np.nan), np.full(MOL_FLEX, np.nan), np.asarray([3, 0, 0, 0], np.int32)
            out.theta[b], out.tau[b] = np.nan, np.nan
        else:
            x, pose, energies, stat, theta, tau, (st, si) = _flex_one(evaluate, x0, rotors, step, tol, max_evals, dofs)
            out.x[lo:hi] = x
            for k, rotor in enumerate(rotors):
                out.theta[b, rotor[3]], out.tau[b, rotor[3]] = theta[k], tau[k]
        out.atom[lo:hi], out.grad[lo:hi] = st.atom, st.grad
        out.mol[b], out.flag[b], out.mol_grad[b] = st.mol[0], st.flag[0], st.mol_grad[0]
        intra.atom[lo:hi], intra.grad[lo:hi], intra.mol[b], intra.flag[b] = si.atom, si.grad, si.mol[0], si.flag[0]
        out.pose[b], out.energies[b], out.stat[b] = pose, energies, stat
    return out


def _flexed(x, atom_type, lig_mask, pockets, info, mol_group, batch, orders, settings, dofs):
    """The launches behind `vina_minimize(torsions=True)`: bond orders (unless given), `dsbdd_vina_type`,
    `dsbdd_vina_torsions`, then `dsbdd_vina_flex`."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise _lib.HipLibraryError("vina_minimize needs device tensors (HIP path; no CPU fallback)")
    if dofs not in (1, 2, 3):
        raise ValueError("dofs must be 1 (rigid body), 2 (torsions) or 3 (both)")
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
    if orders is None and B:
        orders = perceive_orders(x, atom_type, lig_mask, info, batch=B)
    code, mol_int, off = type_ligands(x, atom_type, lig_mask, info, orders=orders, batch=B)
    tree = ligand_torsions(x, atom_type, lig_mask, info, orders=orders, batch=B)
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    intra = VinaIntra(torch.zeros((N, ATOM_OUT), **f32), torch.zeros((B, MOL_OUT), **f32), torch.zeros(B, **i32),
                      torch.zeros((N, ATOM_GRAD), **f32), off, tree)
    out = VinaFlexed(torch.zeros((N, ATOM_OUT), **f32), torch.zeros((B, MOL_OUT), **f32), mol_int, torch.zeros(B, **i32), code, off,
                     torch.zeros((N, ATOM_GRAD), **f32), torch.zeros((B, MOL_GRAD), **f32), float("inf"), x.clone(),
                     torch.zeros((B, MOL_POSE), **f32), torch.zeros((B, MOL_FLEX), **f32), torch.zeros((B, MOL_STAT), **i32), x,
                     intra, torch.zeros((B, MAX_TORSIONS), **f32), torch.zeros((B, MAX_TORSIONS), **f32))
    step, tol, max_evals = settings
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    # without atoms both pointers are stand-ins (`_ptr`); held here together, so that they are two addresses
    x_arg, x_out_arg = (x, out.x) if N else (torch.zeros(4, **f32), torch.zeros(4, **f32))
    rc = lib.dsbdd_vina_flex(stream, x_arg.data_ptr(), _ptr(code), off.data_ptr(), B, _ptr(groups), _ptr(mol_int), _ptr(pockets.x),
                             _ptr(pockets.code), pockets.group_off.data_ptr(), G, _ptr(tree.ints), _ptr(tree.ends),
                             _ptr(tree.sides), _ptr(tree.pair_mask), int(dofs), float(step), float(tol), int(max_evals),
                             _ptr(out.atom), _ptr(out.mol), _ptr(out.flag), _ptr(out.grad), _ptr(out.mol_grad), _ptr(intra.atom),
                             _ptr(intra.mol), _ptr(intra.flag), _ptr(intra.grad), x_out_arg.data_ptr(), _ptr(out.pose),
                             _ptr(out.energies), _ptr(out.stat), _ptr(out.theta), _ptr(out.tau))
    _lib.check(rc, "dsbdd_vina_flex")
    return out


# ---- command line ----------------------------------------------------------------------------------------------------------
CSV_COLUMNS = ("n_atoms", "untyped", "n_rot", "nonfinite") + TERMS + ("inter", "score")
MIN_CSV_COLUMNS = CSV_COLUMNS + ("inter_start", "score_start", "status", "evals", "rmsd")      # with --minimize
FLEX_CSV_COLUMNS = MIN_CSV_COLUMNS + ("intra", "intra_start", "n_torsions")                    # with --minimize --torsions


def write_csv(path, rows, columns=CSV_COLUMNS):
    """rows: (source, index, MolVina or its dict); `path` None writes to stdout."""
    _pairs.write_csv(path, rows, columns)


def write_minimized_sdf(path, sources, rows):
    """The relaxed molecules of `rows` = (source, index, MolVinaMin) as one SDF file, in row order: the heavy atoms and bonds
    of record `index` of the SDF file `source` (`sources`: {path: `as_ligands(path)`}) at the returned coordinates."""
    from .molecules import Molecule, write_sdf
    mols, names = [], []
    for source, k, rec in rows:
        _, elements, bonds = sources[source][k]
        # `to_sdf_block` writes a bond (i, j) as "j i": handed over reversed, the bond block repeats the source's columns
        mols.append(Molecule(np.asarray(rec.x, np.float32), list(elements), [(j, i, o) for i, j, o in bonds or []]))
        names.append(f"{source}:{k} status={STATUS[rec.status]} score={rec.score:.4f} score_start={rec.score_start:.4f}")
    write_sdf(path, mols, names)


GRAD_CSV_COLUMNS = ("source", "index", "atom", "gx", "gy", "gz", "norm")


def write_grad_csv(path, rows):
    """rows: (source, index, MolVinaGrad) -> one line per heavy atom: source, molecule index, atom index, the gradient of
    `inter` (kcal/mol/A, floats by repr) and its norm."""
    lines = [",".join(GRAD_CSV_COLUMNS)]
    for source, k, rec in rows:
        for a, g in enumerate(np.asarray(rec.grad, np.float64)):
            lines.append(",".join([str(source), str(k), str(a)] + [repr(float(v)) for v in g] +
                                  [repr(float(np.sqrt((g * g).sum())))]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Vina-type interaction score of written ligand poses against a protein "
                                            "(one row per molecule; not smina output)")
    _pairs.add_complex_arguments(p)
    p.add_argument("--bonds", choices=("distance", "file"), default="distance",
                   help="distance: perceive bonds as for generated molecules; file: read the SDF bond block")
    p.add_argument("--dataset", default="crossdock", help="the dataset whose bond-length tables --bonds distance uses")
    p.add_argument("--grad_out", default=None,
                   help="also write the gradient of `inter` with respect to the ligand coordinates, one row per heavy atom "
                        "(kcal/mol/A; the scores then come from the same launch, unchanged)")
    p.add_argument("--minimize", default=None, metavar="OUT.sdf",
                   help="relax every pose as a rigid body under `inter` on the device first (rigid ligand, rigid protein, a "
                        "local search; not smina or qvina output): the relaxed molecules go to this file, the rows of --out "
                        "(and of --grad_out) describe them and gain the columns inter_start, score_start, status, evals, rmsd")
    p.add_argument("--torsions", action="store_true",
                   help="--minimize: turn the rotatable bonds as well, under inter + intra (a local search, not smina or qvina "
                        "output); the rows gain the columns intra, intra_start, n_torsions")
    p.add_argument("--step", type=float, default=MIN_STEP, help="--minimize: the first and largest step, A")
    p.add_argument("--tol", type=float, default=MIN_TOL, help="--minimize: stop when the step falls below this, A")
    p.add_argument("--max_evals", type=int, default=MIN_EVALS, help=f"--minimize: evaluation budget per molecule (1 ... {MAX_EVALS})")
    return _pairs.parse_complex_arguments(p, argv)


def main(argv=None):
    a = parse_args(argv)
    print(VINA_COVERAGE, file=sys.stderr)
    typed = type_pocket(select_residues(a.pdbfile, a.scope, a.ref_ligand))
    print(f"[vina] {len(typed.code)} protein heavy atoms, {typed.untemplated} typed by element alone", file=sys.stderr)
    pockets = VinaPocket.upload([typed], torch.device(a.device))
    records_of = score_molecules
    if a.grad_out is not None:
        print(VINA_GRAD_COVERAGE, file=sys.stderr)
        records_of = gradient_molecules
    if a.torsions and a.minimize is None:
        raise SystemExit("--torsions needs --minimize OUT.sdf")
    if a.minimize is not None:
        print(VINA_FLEX_COVERAGE if a.torsions else VINA_MIN_COVERAGE, file=sys.stderr)
        step, tol, max_evals = _settings(a.step, a.tol, a.max_evals)

        def records_of(path, *args, **kwargs):
            return minimize_molecules(path, *args, step=step, tol=tol, max_evals=max_evals, torsions=a.torsions, **kwargs)
    rows = []
    for path in a.sdf:
        rows += [(path, k, rec) for k, rec in enumerate(records_of(path, pockets, a.dataset, bonds=a.bonds))]
    write_csv(a.out, rows, CSV_COLUMNS if a.minimize is None else FLEX_CSV_COLUMNS if a.torsions else MIN_CSV_COLUMNS)
    if a.grad_out is not None:
        write_grad_csv(a.grad_out, rows)
    if a.minimize is not None:
        write_minimized_sdf(a.minimize, {path: as_ligands(path) for path in a.sdf}, rows)
    return rows


if __name__ == "__main__":
    main()
