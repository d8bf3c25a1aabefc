"""Ligands as INPUT: what substructure inpainting and diversification need before the DDPM call.

The reference's `inpaint.py` and `optimize.py` read ligands with RDKit (`Chem.SDMolSupplier(file, sanitize=False)`,
inpaint.py:19-33, optimize.py:22-62) or take named atoms of a HETATM group through BioPython (inpaint.py:47-60), and
build the packed `ligand` / `lig_fixed` batch with Python loops on the host (inpaint.py:114-141).  This module is the
same layer without either library:

  * `read_sdf_molecules`     V2000 SDF -> coordinates + element symbols, every record, nothing sanitised or stripped;
  * `ligand_atoms_from_pdb`  named atoms of `<chain>:<resi>` in FILE order (inpaint.py:57);
  * `encode_elements`        symbols -> class ids, with an error that names the offending atom;
  * `inpaint_sizes`          the ligand-size rule of inpaint.py:107-112;
  * `plan_ligand_pack` / `pack_ligands`   the packed batch in one HIP launch (`dsbdd_pack_ligands`,
    csrc/ligand_pack.h); templates may be device tensors, e.g. the output of the previous chain.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._pairs import sdf_records


# --------------------------------------------------------------------------- files
def read_sdf_molecules(path):
    """Every record of a V2000 SDF file -> list of (xyz float32 [n,3], element symbols list[str]).

    Like `Chem.SDMolSupplier(path, sanitize=False)` read for positions and symbols: no sanitisation, hydrogens stay,
    bonds and properties are ignored.  A record is the text up to a `$$$$` line; the counts line is its fourth."""
    out = []
    for k, rec in enumerate(sdf_records(path)):
        if len(rec) < 4 or "V2000" not in rec[3]:
            raise ValueError(f"{path}: record {k} is not a V2000 mol block")
        n_atoms = int(rec[3][0:3])
        if len(rec) < 4 + n_atoms:
            raise ValueError(f"{path}: record {k} announces {n_atoms} atoms and holds {len(rec) - 4} lines")
        xyz = np.empty((n_atoms, 3), np.float32)
        elements = []
        for a, l in enumerate(rec[4:4 + n_atoms]):
            xyz[a] = (float(l[0:10]), float(l[10:20]), float(l[20:30]))
            elements.append(l[31:34].strip())
        out.append((xyz, elements))
    return out


def ligand_atoms_from_pdb(residues, ligand_id, atom_names=None):
    """Atoms of the group `<chain>:<resi>` among `pocket.read_pdb_residues(..., hetero=True)` ->
    (xyz float32 [n,3], element symbols).  With `atom_names` only the atoms whose name is in that SET are returned, in
    the order of the FILE, not of the argument (inpaint.py:57); a name the group does not have raises ValueError."""
    chain, resi = str(ligand_id).split(":")
    hit = [r for r in residues if r["chain"] == chain and r["resseq"] == int(resi)]
    if len(hit) > 1:                         # a HETATM group and a residue can share a number
        hit = [r for r in hit if r.get("hetero")] or hit
    if len(hit) != 1:
        raise ValueError(f"{ligand_id}: {len(hit)} groups of the PDB file match")
    atoms = hit[0]["atoms"]
    if atom_names is not None:
        wanted = set(atom_names)
        missing = wanted - {a[0] for a in atoms}
        if missing:
            raise ValueError(f"{ligand_id} has no atom named {sorted(missing)}")
        atoms = [a for a in atoms if a[0] in wanted]
    return (np.asarray([a[2] for a in atoms], np.float32).reshape(-1, 3), [a[1] for a in atoms])


def encode_elements(elements, atom_encoder):
    """Element symbols -> int32 class ids.  The reference indexes the encoder directly and dies with a bare KeyError
    (for example on an explicit hydrogen of an unsanitised SDF); here the error names the element and the atom."""
    out = np.empty(len(elements), np.int32)
    for i, e in enumerate(elements):
        if e not in atom_encoder:
            raise ValueError(f"atom {i}: element {e!r} is not in the atom encoder {sorted(atom_encoder)} "
                             "(remove explicit hydrogens / unsupported elements from the input ligand)")
        out[i] = atom_encoder[e]
    return out


def as_templates(molecules, atom_encoder):
    """`molecules`: an SDF path, or a list whose items are `Molecule` objects or (xyz, elements) pairs ->
    list of (xyz float32 [n,3], int32 class ids [n])."""
    if isinstance(molecules, (str, bytes)) or hasattr(molecules, "__fspath__"):
        molecules = read_sdf_molecules(molecules)
    out = []
    for m in molecules:
        xyz, elements = (m.positions, m.symbols) if hasattr(m, "symbols") else m
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        if len(elements) != len(xyz):
            raise ValueError(f"{len(xyz)} coordinates for {len(elements)} elements")
        out.append((xyz, encode_elements(list(elements), atom_encoder)))
    return out


# --------------------------------------------------------------------------- sizes
def inpaint_sizes(size_distribution, pocket_size, n_fixed, add_n_nodes=None):
    """Ligand sizes of an inpainting batch (inpaint.py:107-112): drawn from p(n_lig | n_pocket) and raised to the
    size of the fixed substructure, or exactly `n_fixed + add_n_nodes`.  -> int64 [len(pocket_size)] on the host."""
    n = len(pocket_size)
    if add_n_nodes is None:
        drawn = size_distribution.sample_conditional(n1=None, n2=pocket_size)
        return torch.clamp(torch.as_tensor(drawn, dtype=torch.int64).cpu(), min=int(n_fixed))
    if int(add_n_nodes) < 0:
        raise ValueError("add_n_nodes must not be negative")
    return torch.ones(n, dtype=torch.int64) * int(n_fixed) + int(add_n_nodes)


# --------------------------------------------------------------------------- packed batch
PackPlan = namedtuple("PackPlan", "buffer n_tmpl tmpl_rows batch n_rows tmpl_ptr slot_tmpl slot_size slot_off")


def plan_ligand_pack(tmpl_sizes, slot_tmpl, slot_sizes):
    """Host side of the packer: everything integer it needs, checked, in ONE int32 buffer
    `[tmpl_ptr (n_tmpl+1) | slot_tmpl (B) | slot_size (B) | slot_off (B+1)]` (the named fields are views of it).
    Slot b holds template slot_tmpl[b] in its first rows and has slot_sizes[b] >= max(len(template), 1) rows; its
    first row is slot_off[b], and n_rows = slot_off[B] is the N of the batch."""
    tmpl_sizes = np.asarray(tmpl_sizes, np.int64).reshape(-1)
    slot_tmpl = np.asarray(slot_tmpl, np.int64).reshape(-1)
    slot_sizes = np.asarray(slot_sizes, np.int64).reshape(-1)
    n_tmpl, B = len(tmpl_sizes), len(slot_sizes)
    if B < 1 or len(slot_tmpl) != B:
        raise ValueError(f"{len(slot_tmpl)} template ids for {B} slots (need one per slot, at least one slot)")
    if (tmpl_sizes < 0).any():
        raise ValueError("negative template size")
    if ((slot_tmpl < 0) | (slot_tmpl >= n_tmpl)).any():
        raise ValueError(f"template id outside [0, {n_tmpl})")
    short = np.nonzero(slot_sizes < np.maximum(tmpl_sizes[slot_tmpl], 1))[0]
    if len(short):
        b = int(short[0])
        raise ValueError(f"slot {b}: {int(slot_sizes[b])} rows for a template of {int(tmpl_sizes[slot_tmpl[b]])} atoms "
                         "(a slot needs at least one row and at least its template's)")
    if int(tmpl_sizes.sum()) >= 2 ** 29 or int(slot_sizes.sum()) >= 2 ** 29:
        raise ValueError("batch too large for 32-bit row indices")
    buf = np.zeros((n_tmpl + 1) + B + B + (B + 1), np.int32)
    o1, o2, o3 = n_tmpl + 1, n_tmpl + 1 + B, n_tmpl + 1 + 2 * B
    buf[1:o1] = np.cumsum(tmpl_sizes)
    buf[o1:o2] = slot_tmpl
    buf[o2:o3] = slot_sizes
    buf[o3 + 1:] = np.cumsum(slot_sizes)
    return PackPlan(buf, n_tmpl, int(buf[o1 - 1]), B, int(buf[-1]), buf[:o1], buf[o1:o2], buf[o2:o3], buf[o3:])


def pack_ligands(tmpl_x, tmpl_type, tmpl_sizes, slot_tmpl, slot_sizes, atom_nf):
    """The packed ligand batch of the design front ends, in one launch on the current stream.

    tmpl_x [M,3] float32 and tmpl_type [M] integer class ids are DEVICE tensors holding the templates one after the
    other (`tmpl_sizes`: their lengths, host integers) -- a set read from files and uploaded once, or the output of
    an earlier chain used as it lies on the device.  `slot_tmpl` / `slot_sizes` (host integers) give every batch slot
    its template and its number of rows.  Returns (ligand, lig_fixed): ligand = {'x' [N,3], 'one_hot' [N,atom_nf]
    float32, 'size' int64 [B], 'mask' int64 [N]} with the template in the first rows of every slot and zeros after,
    lig_fixed int64 [N] = 1 on the template rows.  The integers travel as one small buffer (one asynchronous copy);
    nothing is read back."""
    if not (torch.is_tensor(tmpl_x) and tmpl_x.is_cuda and torch.is_tensor(tmpl_type) and tmpl_type.is_cuda):
        raise _lib.HipLibraryError("pack_ligands needs device tensors (HIP path; no CPU fallback)")
    plan = plan_ligand_pack(tmpl_sizes, slot_tmpl, slot_sizes)
    dev = tmpl_x.device
    tmpl_x = tmpl_x.detach().to(torch.float32).reshape(-1, 3).contiguous()
    tmpl_type = tmpl_type.detach().to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if tmpl_x.shape[0] != plan.tmpl_rows or tmpl_type.shape[0] != plan.tmpl_rows:
        raise ValueError(f"templates hold {tmpl_x.shape[0]} coordinates / {tmpl_type.shape[0]} types, "
                         f"their sizes add up to {plan.tmpl_rows}")
    lib = _lib.load()
    ints = torch.from_numpy(plan.buffer).pin_memory().to(dev, non_blocking=True)
    N, B = plan.n_rows, plan.batch
    x = torch.empty((N, 3), dtype=torch.float32, device=dev)
    one_hot = torch.empty((N, int(atom_nf)), dtype=torch.float32, device=dev)
    fixed = torch.empty(N, dtype=torch.int64, device=dev)
    mask = torch.empty(N, dtype=torch.int64, device=dev)
    size = torch.empty(B, dtype=torch.int64, device=dev)
    p0 = ints.data_ptr()
    o1, o2, o3 = plan.n_tmpl + 1, plan.n_tmpl + 1 + B, plan.n_tmpl + 1 + 2 * B
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.dsbdd_pack_ligands(stream, tmpl_x.data_ptr() if plan.tmpl_rows else None,
                                tmpl_type.data_ptr() if plan.tmpl_rows else None, p0, plan.n_tmpl, plan.tmpl_rows,
                                p0 + 4 * o1, p0 + 4 * o2, p0 + 4 * o3, B, N, int(atom_nf),
                                x.data_ptr(), one_hot.data_ptr(), fixed.data_ptr(), mask.data_ptr(), size.data_ptr())
    _lib.check(rc, "dsbdd_pack_ligands")
    return {"x": x, "one_hot": one_hot, "size": size, "mask": mask}, fixed


def upload_templates(templates, device):
    """list of (xyz, class ids) -> (tmpl_x [M,3] float32, tmpl_type [M] int32 on `device`, sizes list)."""
    sizes = [len(t) for _, t in templates]
    if sum(sizes) == 0:
        return (torch.zeros((0, 3), dtype=torch.float32, device=device),
                torch.zeros(0, dtype=torch.int32, device=device), sizes)
    x = torch.from_numpy(np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c, _ in templates]))
    t = torch.from_numpy(np.concatenate([np.asarray(t, np.int32) for _, t in templates]))
    return x.to(device), t.to(device), sizes
