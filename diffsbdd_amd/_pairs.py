"""The batch front end of the two ligand-pocket pair kernels (csrc/pair_sweep.h), shared by pose.py and vina.py: ligand rows
cut into molecules (`mol_offsets`), pocket rows cut into groups (`PocketGroups`), one group id per molecule
(`device_groups`); and what the two command lines share: residue selection, SDF record splitter, CSV writer, flags."""
from __future__ import annotations

import sys

import numpy as np
import torch

HYDROGENS = ("H", "D")                # dropped on both sides


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _symbol(s):
    s = str(s).strip()
    return s[:1].upper() + s[1:].lower()


def _ptr(t):
    """data pointer of a tensor; an empty one gets a one-element stand-in (the C entry refuses null)."""
    return (t if t.numel() else torch.zeros(4, dtype=t.dtype, device=t.device)).data_ptr()


# ---- molecules and their groups ----------------------------------------------------------------------------------------------
def _n_molecules(lig_mask, batch):
    return int(batch) if batch is not None else (int(lig_mask.max()) + 1 if len(lig_mask) else 0)


def _default_groups(n_mols, n_groups):
    if n_groups == 1:
        return np.zeros(n_mols, np.int64)
    if n_groups == n_mols:
        return np.arange(n_mols, dtype=np.int64)
    raise ValueError(f"mol_group is needed: {n_mols} molecules and {n_groups} pocket groups")


def _checked_groups(mol_group, n_mols, n_groups):
    g = np.asarray(_np(mol_group), np.int64).reshape(-1)
    if len(g) != n_mols:
        raise ValueError(f"{len(g)} group ids for {n_mols} molecules")
    if len(g) and (g.min() < 0 or g.max() >= n_groups):
        raise ValueError(f"mol_group outside [0, {n_groups})")
    return g


def mol_offsets(lig_mask, B, dev):
    """int32 [B + 1] on the device: the first row of every molecule of the sorted sample ids `lig_mask`."""
    sizes = torch.bincount(lig_mask.to(dev), minlength=B)
    off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    off[1:] = torch.cumsum(sizes, 0).to(torch.int32)
    return off


def device_groups(mol_group, B, G, dev):
    """int32 [B] on the device: the group of every molecule (None: group b of B, or the one group).  Host integers are
    range-checked here; a device tensor only has its count checked: the kernel range-checks its values."""
    if mol_group is None:
        mol_group = _default_groups(B, G)
    if torch.is_tensor(mol_group) and mol_group.is_cuda:
        if mol_group.numel() != B:
            raise ValueError(f"{mol_group.numel()} group ids for {B} molecules")
        return mol_group.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    return torch.as_tensor(_checked_groups(mol_group, B, G).astype(np.int32), device=dev)


def pack_ligands(ligands):
    """list of (xyz, ...) -> (x [N,3] float32, lig_mask [N] int64, sizes) on the host."""
    xs = [np.asarray(l[0], np.float32).reshape(-1, 3) for l in ligands]
    sizes = [len(a) for a in xs]
    x = np.concatenate(xs) if xs else np.zeros((0, 3), np.float32)
    return x, np.repeat(np.arange(len(xs), dtype=np.int64), sizes), sizes


class PocketGroups:
    """Pocket heavy atoms on the device, one group per pocket: x [M,3] float32, one per-atom column (a subclass names it
    and gives its dtype: COLUMN, DTYPE, WHAT), group_off int32 [G+1] (`offsets`: the same on the host).  Upload once, use
    for many batches."""
    COLUMN, DTYPE, WHAT = None, None, None

    def __init__(self, x, column, offsets):
        self.x = x
        setattr(self, self.COLUMN, column)
        self.offsets = np.asarray(offsets, np.int64).reshape(-1)
        if self.offsets[0] != 0 or np.any(np.diff(self.offsets) < 0) or self.offsets[-1] != x.shape[0] or \
                column.shape[0] != x.shape[0] or self.offsets[-1] >= 2 ** 31:
            raise ValueError(f"{type(self).__name__}: offsets must ascend from 0 to the number of rows")
        self.group_off = torch.as_tensor(self.offsets.astype(np.int32), device=x.device)

    n_groups = property(lambda self: len(self.offsets) - 1)
    column = property(lambda self: getattr(self, self.COLUMN))

    @classmethod
    def upload(cls, pockets, device, *extra):
        """`pockets`: list of (xyz [m,3], column [m]) host arrays, one per group; `extra`: a subclass's own constructor arguments."""
        pockets = list(pockets)
        x, _, sizes = pack_ligands(pockets)
        cs = [np.asarray(p[1], cls.DTYPE).reshape(-1) for p in pockets]
        if [len(c) for c in cs] != sizes:
            raise ValueError(f"a pocket needs one {cls.WHAT} per atom")
        c = np.concatenate(cs) if cs else np.zeros(0, cls.DTYPE)
        return cls(torch.as_tensor(x, device=device), torch.as_tensor(c, device=device), np.concatenate([[0], np.cumsum(sizes)]),
                   *extra)

    @classmethod
    def concat(cls, parts, *extra):
        """The groups of several of these one after the other (a copy on the device, no upload of atoms)."""
        parts = list(parts)
        if len(parts) == 1:
            return parts[0]
        sizes = np.concatenate([np.diff(p.offsets) for p in parts])
        return cls(torch.cat([p.x for p in parts]), torch.cat([p.column for p in parts]), np.concatenate([[0], np.cumsum(sizes)]),
                   *extra)


# ---- written complexes: files and the command lines ----------------------------------------------------------------------------
def sdf_records(path):
    """The records of an SDF file as lists of lines: the text up to a `$$$$` line; a last block without one counts."""
    with open(path) as f:
        lines = f.read().splitlines()
    records, cur = [], []
    for line in lines:
        if line.startswith("$$$$"):
            records.append(cur)
            cur = []
        else:
            cur.append(line)
    if any(l.strip() for l in cur):
        records.append(cur)
    return records


def select_residues(pdb_file, scope="protein", ref_ligand=None):
    """The protein atoms to check: every ATOM residue of the file (`protein`), or the residues within 8 A of `ref_ligand`
    (an SDF path or `<chain>:<resi>` of the file) as `generate_ligands` selects them (`pocket`)."""
    from . import pocket as pocket_io
    if scope == "protein":
        return pocket_io.read_pdb_residues(pdb_file)
    if scope != "pocket":
        raise ValueError("scope must be 'protein' or 'pocket'")
    if ref_ligand is None:
        raise ValueError("scope 'pocket' needs ref_ligand")
    residues = pocket_io.read_pdb_residues(pdb_file, hetero=True)
    skip = None
    if str(ref_ligand).endswith(".sdf"):
        lig_xyz = pocket_io.read_sdf_coords(ref_ligand)
    else:
        from .ligand_io import ligand_atoms_from_pdb
        lig_xyz, _ = ligand_atoms_from_pdb(residues, ref_ligand)
        skip = int(str(ref_ligand).split(":")[1])
    return pocket_io.pocket_residues_from_ligand([r for r in residues if r["resseq"] != skip], lig_xyz)


def write_csv(path, rows, columns):
    """rows: (source, index, a record with `as_dict` or its dict); floats by repr; `path` None writes to stdout."""
    lines = [",".join(("source", "index") + tuple(columns))]
    for source, k, rec in rows:
        rec = rec.as_dict() if hasattr(rec, "as_dict") else rec
        lines.append(",".join([str(source), str(k)] + [repr(rec[c]) if isinstance(rec[c], float) else str(rec[c])
                                                       for c in columns]))
    if path is None:
        sys.stdout.write("\n".join(lines) + "\n")
        return
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def add_complex_arguments(parser):
    """The flags both command lines take: the protein, the ligand files, the residue selection, output and device."""
    parser.add_argument("--pdbfile", required=True)
    parser.add_argument("--sdf", nargs="+", required=True)
    parser.add_argument("--scope", choices=("protein", "pocket"), default="protein")
    parser.add_argument("--ref_ligand", default=None, help="SDF file or <chain>:<resi>: the pocket of --scope pocket")
    parser.add_argument("--out", default=None)
    parser.add_argument("--device", default="cuda")


def parse_complex_arguments(parser, argv):
    """parse_args + the one rule between the shared flags."""
    a = parser.parse_args(argv)
    if a.scope == "pocket" and a.ref_ligand is None:
        parser.error("--scope pocket needs --ref_ligand")
    return a
