"""Molecule-set metrics on the device: validity, connectivity, uniqueness, novelty, per-pocket diversity and the KL
divergence of the atom-type distribution of a set of generated molecules.

Counterpart of the reference's `BasicMolecularMetrics` (analysis/metrics.py:42-133), `CategoricalDistribution` (:11-32)
and `MoleculeProperties.calculate_diversity`, without RDKit: everything per molecule comes from two launches on the
device tensors the samplers return -- `dsbdd_bond_orders` and `dsbdd_mol_graph_stats` (csrc/mol_metrics.h: valences,
fragments, a graph key that does not depend on the atom order, a 2048-bit fingerprint, type counts) -- and the pair
distances from `dsbdd_fp_diversity`.  Only the small per-molecule records come to the host, never the order matrices.

`_graph_stats_host` / `_fp_diversity_host` restate both kernels in numpy (uint64 / float64).  They are the specification
the kernels are tested against bit for bit, not a fallback: the public entry points refuse CPU tensors.

  python -m diffsbdd_amd.metrics --sdf A.sdf [B.sdf ...] --dataset crossdock [--train_npz train.npz] [--out metrics.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .chem_tables import MAX_VALENCE, dataset_info
from .molecules import bond_orders

MAX_ATOMS = _lib.MOL_MAX_ATOMS
FP_WORDS = _lib.FP_WORDS
FP_BITS = 32 * FP_WORDS
# columns of GraphStats.stats
N_ATOMS, N_BONDS, N_OVER_VALENCE, N_FRAGMENTS, LARGEST_SIZE, LARGEST_LABEL = range(6)
KL_EPS = 1e-10          # CategoricalDistribution.EPS

METRICS_COVERAGE = (
    "molecule-set metrics vs the reference (analysis/metrics.py, lightning_modules.py:449-485): "
    "PRESENT = validity, connectivity, uniqueness, novelty, per-pocket diversity, kl_div_atom_types, computed per molecule "
    "by GPU kernels from the distance-table bonds; "
    "APPROXIMATED = validity: a sample is valid when it has an atom and no atom exceeds its element's valence, all "
    "fragments included (RDKit's SanitizeMol is absent; the approximation of sanitize stated for process_molecule); "
    "DEFINED DIFFERENTLY = molecule identity is a 64-bit colour-refinement graph key over elements and bond orders "
    "instead of a canonical SMILES (equal keys mean refinement-equivalent, not proven isomorphic; uniqueness is computed "
    "without a reference set too), and diversity uses 2048-bit radius-2 atom-environment fingerprints (ECFP-like) instead "
    "of RDKFingerprint: diversity values are comparable between runs of this package, NOT with the reference's numbers; "
    "kl_div_atom_types sums over the types the reference distribution holds (the reference's formula gives nan when one "
    "is empty); "
    "ABSENT = QED, SA, logP, Lipinski, smina docking score, kl_div_residue_types.")


@dataclass
class GraphStats:
    """Per-atom and per-molecule results of `graph_stats` (device tensors; numpy arrays from the host restatement)."""
    valence: object          # [N] int32 sum of bond orders
    label: object            # [N] int32 smallest atom index (within the molecule) of the atom's fragment
    stats: object            # [B, 8] int32: n_atoms, n_bonds, atoms over valence, fragments, largest size, largest label, 0, 0
    keys: object             # [B, 2] int64 bit patterns of the uint64 keys: largest fragment, whole sample
    fingerprint: object      # [B, 64] int32 bit patterns: 2048 bits of the largest fragment
    type_counts: object      # [B, n_types] int32
    sizes: object            # [B] int64

    def keys_u64(self):
        """[B, 2] uint64 on the host."""
        return np.ascontiguousarray(_np(self.keys)).view(np.uint64)


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def max_valence_table(info):
    """int32 [n_types]: `MAX_VALENCE` of every decoder entry, -1 (not checked) for one without (crossdock_full's 'others')."""
    return np.asarray([MAX_VALENCE.get(s, -1) for s in info["atom_decoder"]], np.int32)


def _n_molecules(lig_mask, batch):
    return int(batch) if batch is not None else (int(lig_mask.max()) + 1 if len(lig_mask) else 0)


# ---- the device path ---------------------------------------------------------------------------------------------------
def mol_graph_stats(orders, atom_type, mol_off, max_valence, bond_orders_in_key=True):
    """`dsbdd_mol_graph_stats` on device tensors: orders int8 [B, n_max, n_max] (what `bond_orders` returns), atom_type
    int32 [N], mol_off int32 [B+1], max_valence int32 [n_types].  -> GraphStats without `sizes`."""
    if not orders.is_cuda:
        raise _lib.HipLibraryError("mol_graph_stats needs device tensors (HIP path; no CPU fallback)")
    lib = _lib.load()
    dev = orders.device
    B, n_max = int(orders.shape[0]), int(orders.shape[1])
    N, T = int(atom_type.numel()), int(max_valence.numel())
    i32 = dict(dtype=torch.int32, device=dev)
    out = GraphStats(torch.zeros(N, **i32), torch.zeros(N, **i32), torch.zeros((B, _lib.MOL_STATS), **i32),
                     torch.zeros((B, 2), dtype=torch.int64, device=dev), torch.zeros((B, FP_WORDS), **i32),
                     torch.zeros((B, T), **i32), None)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.dsbdd_mol_graph_stats(stream, orders.data_ptr(), atom_type.data_ptr(), mol_off.data_ptr(), B, T,
                                   max_valence.data_ptr(), n_max, int(bool(bond_orders_in_key)), out.valence.data_ptr(),
                                   out.label.data_ptr(), out.stats.data_ptr(), out.keys.data_ptr(),
                                   out.fingerprint.data_ptr(), out.type_counts.data_ptr())
    _lib.check(rc, "dsbdd_mol_graph_stats")
    return out


def graph_stats(x, atom_type, lig_mask, info, batch=None, bond_orders_in_key=True):
    """Graph statistics of a batch of point clouds: `bond_orders` then `dsbdd_mol_graph_stats`, both on the device.

    x [N,3] float32 (Angstrom), atom_type [N] class ids of `info["atom_decoder"]`, lig_mask [N] sorted sample ids;
    `batch` keeps samples without atoms in the list.  -> GraphStats of device tensors."""
    if not x.is_cuda:
        raise _lib.HipLibraryError("graph_stats needs device tensors (HIP path; no CPU fallback)")
    if isinstance(info, str):
        info = dataset_info(info)
    dev = x.device
    B = _n_molecules(lig_mask, batch)
    sizes = torch.bincount(lig_mask.to(dev), minlength=B)
    n_max = max(int(sizes.max().item()) if B else 0, 1)
    if n_max > MAX_ATOMS:
        raise ValueError(f"graph_stats: a molecule of {n_max} atoms exceeds the supported {MAX_ATOMS}")
    at = atom_type.to(device=dev, dtype=torch.int32).contiguous()
    off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
    off[1:] = torch.cumsum(sizes, 0).to(torch.int32)
    if B == 0:
        orders = torch.zeros((0, 1, 1), dtype=torch.int8, device=dev)
    else:
        orders, _ = bond_orders(x, at, lig_mask, info, n_max=n_max, batch=B)
    maxv = torch.as_tensor(max_valence_table(info), device=dev)
    out = mol_graph_stats(orders, at, off, maxv, bond_orders_in_key)
    out.sizes = sizes
    return out


def fp_diversity(fingerprint, group_off):
    """`dsbdd_fp_diversity`: fingerprint [M, 64] int32 device tensor, group_off [G+1] row offsets (any integer sequence).
    -> (sum of pair distances float64 [G], number of pairs int64 [G]) as device tensors."""
    if not fingerprint.is_cuda:
        raise _lib.HipLibraryError("fp_diversity needs device tensors (HIP path; no CPU fallback)")
    lib = _lib.load()
    dev = fingerprint.device
    fp = fingerprint.contiguous()
    off_host = np.asarray(_np(group_off), np.int64)
    if len(off_host) < 1 or off_host[0] < 0 or np.any(np.diff(off_host) < 0) or off_host[-1] > fp.shape[0] or \
            fp.dim() != 2 or fp.shape[1] != FP_WORDS:
        raise ValueError("fp_diversity: group_off must ascend within the [M, 64] fingerprint rows")
    G = len(off_host) - 1
    off = torch.as_tensor(off_host.astype(np.int32), device=dev)
    total = torch.zeros(G, dtype=torch.float64, device=dev)
    pairs = torch.zeros(G, dtype=torch.int64, device=dev)
    if fp.shape[0] == 0:
        return total, pairs
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.dsbdd_fp_diversity(stream, fp.data_ptr(), off.data_ptr(), G, total.data_ptr(), pairs.data_ptr())
    _lib.check(rc, "dsbdd_fp_diversity")
    return total, pairs


# ---- the host restatements (specification and test oracle) ----------------------------------------------------------------
_U = np.uint64


def _mix(x):
    """splitmix64 (increment + finaliser) on uint64 arrays, wrapping."""
    x = np.asarray(x, np.uint64) + _U(0x9E3779B97F4A7C15)
    x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
    return x ^ (x >> _U(31))


def _bond_orders_host(x, atom_type, mol_off, info, n_max):
    """bond_orders_kernel in float32 numpy: -> int8 [B, n_max, n_max], strictly lower triangular."""
    x = np.asarray(x, np.float32)
    B = len(mol_off) - 1
    out = np.zeros((B, n_max, n_max), np.int8)
    m1, m2, m3 = (np.float32(m) for m in info["margins"])
    for b in range(B):
        lo, n = int(mol_off[b]), min(int(mol_off[b + 1] - mol_off[b]), n_max)
        if n < 2:
            continue
        p, t = x[lo:lo + n], np.asarray(atom_type[lo:lo + n], np.int64)
        d = p[:, None, :] - p[None, :, :]
        sq = d * d
        dist = np.float32(100.0) * np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])
        o = np.zeros((n, n), np.int8)
        for order, (key, m) in enumerate((("bonds1", m1), ("bonds2", m2), ("bonds3", m3)), 1):
            o[dist < np.asarray(info[key], np.float32)[t[:, None], t[None, :]] + m] = order
        out[b, :n, :n] = np.tril(o, -1)
    return out


def _molecule_host(order, types, n_types, max_valence, bond_orders_in_key):
    """mol_graph_kernel for one molecule: order [n, n] strictly lower triangular, types [n]."""
    n = len(types)
    low = np.tril(np.maximum(np.asarray(order, np.int64), 0), -1)
    A = low + low.T
    nb = A > 0
    val, deg = A.sum(1), nb.sum(1)
    t = np.asarray(types, np.int64)
    lim = np.where((t >= 0) & (t < n_types), np.asarray(max_valence, np.int64)[np.clip(t, 0, n_types - 1)], -1)
    n_over = int(((lim >= 0) & (val > lim)).sum())
    counts = np.bincount(t[(t >= 0) & (t < n_types)], minlength=n_types).astype(np.int32)
    fp = np.zeros(FP_WORDS, np.uint32)
    if n == 0:
        empty = _mix(np.zeros(1, np.uint64))[0]
        return (val.astype(np.int32), np.zeros(0, np.int32), [0, 0, 0, 0, 0, -1, 0, 0], (empty, empty), fp, counts)
    # all BFS at once: dist[a, b]
    dist = np.full((n, n), -1, np.int64)
    np.fill_diagonal(dist, 0)
    frontier = np.eye(n, dtype=bool)
    c = _mix(t.astype(np.uint64) + _U(1))
    d = 0
    while True:
        new = ((frontier.astype(np.int64) @ nb.astype(np.int64)) > 0) & (dist < 0)
        if not new.any():
            break
        d += 1
        dist[new] = d
        shell = new.sum(1).astype(np.uint64)
        grow = shell > 0
        c[grow] = _mix(c[grow] ^ ((_U(d) << _U(32)) | shell[grow]))
        frontier = new
    reach = dist >= 0
    label = reach.argmax(1).astype(np.int32)
    fsize = reach.sum(1)
    roots = np.nonzero(label == np.arange(n))[0]
    big = min(roots, key=lambda a: (-fsize[a], a))          # the rule of Molecule.fragments
    big_size = int(fsize[big])
    in_big = label == big
    w = (A if bond_orders_in_key else nb).astype(np.uint64)

    def refine(col, weights, r):
        s = np.where(nb, _mix(_U(4) * col[None, :] + weights), _U(0)).sum(1, dtype=np.uint64)
        return _mix(col ^ _mix(s + _U(r)))

    key_frag = None
    for r in range(n):
        c = refine(c, w, r)
        if r + 1 == big_size:
            key_frag = _mix(_mix(c[in_big]).sum(dtype=np.uint64) ^ _U(big_size))
    key_whole = _mix(_mix(c).sum(dtype=np.uint64) ^ _U(n))
    f = _mix(t.astype(np.uint64) + _U(1) + (deg.astype(np.uint64) << _U(16)) + (val.astype(np.uint64) << _U(32)))
    for r in range(3):
        bits = (f[in_big] & _U(FP_BITS - 1)).astype(np.int64)
        np.bitwise_or.at(fp, bits >> 5, (np.uint32(1) << (bits & 31).astype(np.uint32)))
        if r < 2:
            f = refine(f, A.astype(np.uint64), r + 1)
    stats = [n, int(deg.sum()) // 2, n_over, len(roots), big_size, int(big), 0, 0]
    return val.astype(np.int32), label, stats, (key_frag, key_whole), fp, counts


def _mol_graph_stats_host(orders, atom_type, mol_off, max_valence, bond_orders_in_key=True):
    """`dsbdd_mol_graph_stats` in numpy: the same outputs, bit for bit (GraphStats of arrays, without `sizes`)."""
    orders, atom_type, mol_off = _np(orders), _np(atom_type), _np(mol_off)
    max_valence = _np(max_valence)
    B, n_max, T = orders.shape[0], orders.shape[1], len(max_valence)
    valence, label = np.zeros(len(atom_type), np.int32), np.zeros(len(atom_type), np.int32)
    stats, keys = np.zeros((B, _lib.MOL_STATS), np.int32), np.zeros((B, 2), np.uint64)
    fp, counts = np.zeros((B, FP_WORDS), np.uint32), np.zeros((B, T), np.int32)
    with np.errstate(over="ignore"):
        for b in range(B):
            lo, n = int(mol_off[b]), max(min(int(mol_off[b + 1] - mol_off[b]), n_max), 0)
            v, l, stats[b], keys[b], fp[b], counts[b] = _molecule_host(orders[b, :n, :n], atom_type[lo:lo + n], T,
                                                                       max_valence, bond_orders_in_key)
            valence[lo:lo + n], label[lo:lo + n] = v, l
    return GraphStats(valence, label, stats, keys.view(np.int64), fp.view(np.int32), counts, None)


def _graph_stats_host(x, atom_type, lig_mask, info, batch=None, bond_orders_in_key=True):
    """`graph_stats` in numpy (float32 bond perception, uint64 keys)."""
    if isinstance(info, str):
        info = dataset_info(info)
    x, atom_type, lig_mask = _np(x), _np(atom_type).astype(np.int32), _np(lig_mask).astype(np.int64)
    B = _n_molecules(lig_mask, batch)
    sizes = np.bincount(lig_mask, minlength=B).astype(np.int64)
    n_max = max(int(sizes.max()) if B else 0, 1)
    if n_max > MAX_ATOMS:
        raise ValueError(f"graph_stats: a molecule of {n_max} atoms exceeds the supported {MAX_ATOMS}")
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    orders = _bond_orders_host(x, atom_type, off, info, n_max)
    out = _mol_graph_stats_host(orders, atom_type, off, max_valence_table(info), bond_orders_in_key)
    out.sizes = sizes
    return out


def _fp_diversity_host(fingerprint, group_off):
    """`dsbdd_fp_diversity` in numpy: exact integer popcounts, float64 distances and sums."""
    fp = np.ascontiguousarray(_np(fingerprint)).view(np.uint32).reshape(-1, FP_WORDS)
    off = np.asarray(_np(group_off), np.int64)
    bits = np.unpackbits(fp.view(np.uint8), axis=1).astype(np.int64)
    total, pairs = np.zeros(len(off) - 1, np.float64), np.zeros(len(off) - 1, np.int64)
    for g in range(len(off) - 1):
        f = bits[off[g]:off[g + 1]]
        m = len(f)
        pairs[g] = m * (m - 1) // 2
        if m < 2:
            continue
        inter = f @ f.T
        pop = f.sum(1)
        union = pop[:, None] + pop[None, :] - inter
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(union > 0, 1.0 - inter.astype(np.float64) / union.astype(np.float64), 0.0)
        total[g] = d[np.tril_indices(m, -1)].sum()
    return total, pairs


# ---- the metrics of a set ----------------------------------------------------------------------------------------------------
def kl_div_atom_types(reference_counts, sample_counts):
    """`CategoricalDistribution.kl_divergence` (analysis/metrics.py:23-32) from two histograms, float64:
    -sum p log(q / p + EPS), p the reference's distribution, q the sample's.  Types the reference never holds (p = 0)
    contribute nothing (the reference's expression is nan there); a sample without atoms has q = 0."""
    p = np.asarray(reference_counts, np.float64)
    q = np.asarray(sample_counts, np.float64)
    p = p / p.sum()
    q = q / q.sum() if q.sum() > 0 else np.zeros_like(q)
    held = p > 0
    return float(-np.sum(p[held] * np.log(q[held] / p[held] + KL_EPS)))


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


class MoleculeSetMetrics:
    """The chain of `BasicMolecularMetrics.evaluate_rdmols` plus diversity and the atom-type KL divergence.

    reference_keys: uint64 keys of the training ligands (`reference_from_dataset`) -- novelty is None without them;
    reference_type_counts: their atom-type histogram -- kl_div_atom_types is -1 without it."""

    def __init__(self, info, reference_keys=None, reference_type_counts=None, connectivity_thresh=1.0, _host=False):
        self.info = dataset_info(info) if isinstance(info, str) else info
        self.reference_keys = None if reference_keys is None else np.unique(np.asarray(reference_keys, np.uint64))
        self.reference_type_counts = None if reference_type_counts is None else \
            np.asarray(reference_type_counts, np.float64)
        self.connectivity_thresh = connectivity_thresh
        self._host = _host          # drive the numpy restatements (tests): not a product path

    def _summary(self, st, keys, sel):
        """Counts and ratios of the samples `sel` (indices)."""
        st, keys = st[sel], keys[sel]
        valid = (st[:, N_ATOMS] >= 1) & (st[:, N_OVER_VALENCE] == 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = st[:, LARGEST_SIZE].astype(np.float64) / st[:, N_ATOMS].astype(np.float64)
        connected = valid & (share >= self.connectivity_thresh)
        unique = np.unique(keys[connected, 0])
        out = {"n": int(len(sel)), "n_valid": int(valid.sum()), "n_connected": int(connected.sum()),
               "n_unique": int(len(unique))}
        out["validity"] = _ratio(out["n_valid"], out["n"])
        out["connectivity"] = _ratio(out["n_connected"], out["n_valid"])
        out["uniqueness"] = _ratio(out["n_unique"], out["n_connected"])
        if self.reference_keys is None:
            out["n_novel"], out["novelty"] = None, None
        else:
            out["n_novel"] = int((~np.isin(unique, self.reference_keys)).sum())
            out["novelty"] = _ratio(out["n_novel"], out["n_unique"])
        return out, sel[connected]

    def evaluate(self, x, atom_type, lig_mask, groups=None, batch=None, per_group=False):
        """x [N,3], atom_type [N], lig_mask [N] as the samplers return them (device tensors); groups [B]: the pocket of
        every sample (any integer labels; None = one group).  -> dict of counts and ratios; `per_group` adds a list
        with the same summary of every group."""
        stats_fn = _graph_stats_host if self._host else graph_stats
        div_fn = _fp_diversity_host if self._host else fp_diversity
        gs = stats_fn(x, atom_type, lig_mask, self.info, batch=batch)
        st, keys = _np(gs.stats), gs.keys_u64()
        B = st.shape[0]
        groups = np.zeros(B, np.int64) if groups is None else np.asarray(_np(groups), np.int64).reshape(-1)
        if len(groups) != B:
            raise ValueError(f"{len(groups)} group labels for {B} samples")
        out, _ = self._summary(st, keys, np.arange(B))
        labels = np.unique(groups)
        rows, off, per = [], [0], []
        for g in labels:
            summary, conn = self._summary(st, keys, np.nonzero(groups == g)[0])
            rows.append(conn)
            off.append(off[-1] + len(conn))
            per.append({"group": int(g), **summary})
        rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        fp = gs.fingerprint
        fp = fp[torch.as_tensor(rows, device=fp.device)] if torch.is_tensor(fp) else fp[rows]
        total, pairs = (_np(v) for v in div_fn(fp, off))
        for k, rec in enumerate(per):
            rec["diversity"] = float(total[k] / pairs[k]) if pairs[k] > 0 else 0.0
        out["n_groups"] = int(len(labels))
        out["diversity"] = float(np.mean([rec["diversity"] for rec in per])) if per else 0.0
        out["kl_div_atom_types"] = -1 if self.reference_type_counts is None else \
            kl_div_atom_types(self.reference_type_counts, _np(gs.type_counts).sum(0))
        if per_group:
            out["groups"] = per
        return out


def reference_from_dataset(dataset, info, chunk=4096, device=None):
    """Sorted unique uint64 keys (largest fragment) and the atom-type counts int64 [n_types] of the ligands of a
    `ProcessedDataset`, with the same two launches as for generated samples, `chunk` ligands at a time."""
    if isinstance(info, str):
        info = dataset_info(info)
    dev = torch.device(device) if device is not None else \
        (dataset.device if dataset.device.type == "cuda" else torch.device("cuda"))
    xs, hs = dataset.items["lig_coords"], dataset.items["lig_one_hot"]
    keys, counts = [], np.zeros(len(info["atom_decoder"]), np.int64)
    for lo in range(0, len(xs), int(chunk)):
        part_x, part_h = xs[lo:lo + chunk], hs[lo:lo + chunk]
        mask = torch.repeat_interleave(torch.arange(len(part_x)), torch.tensor([len(v) for v in part_x]))
        gs = graph_stats(torch.cat(part_x, 0).float().to(dev), torch.cat(part_h, 0).argmax(1).to(dev), mask.to(dev), info,
                         batch=len(part_x))
        keys.append(gs.keys_u64()[:, 0])
        counts += _np(gs.type_counts).sum(0)
    return (np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.uint64)), counts


# ---- command line ------------------------------------------------------------------------------------------------------------
def sdf_batch(sources, info):
    """SDF files, or lists of `Molecule` objects / (xyz, elements) pairs -> (x [N,3] float32, atom_type [N] int32,
    lig_mask [N] int64, groups [B]) on the host; one group per source.  Only atoms and coordinates are read
    (ligand_io): bonds are re-derived as for generated samples."""
    from .ligand_io import as_templates
    xs, ts, mask, groups = [], [], [], []
    for g, source in enumerate(sources):
        for xyz, types in as_templates(source, info["atom_encoder"]):
            mask.append(np.full(len(types), len(groups), np.int64))
            xs.append(xyz)
            ts.append(types)
            groups.append(g)
    cat = lambda v, dt, shape: np.concatenate(v).astype(dt) if v else np.zeros(shape, dt)
    return cat(xs, np.float32, (0, 3)), cat(ts, np.int32, 0), cat(mask, np.int64, 0), np.asarray(groups, np.int64)


def summarize(sources, info, names=None, device="cuda", reference_keys=None, reference_type_counts=None,
              connectivity_thresh=1.0):
    """The metrics of groups of written molecules (`sdf_batch` sources; `names` labels them): overall plus one record per
    group, with METRICS_COVERAGE under "coverage" -- the content of the CLIs' metrics.json."""
    if isinstance(info, str):
        info = dataset_info(info)
    x, t, mask, groups = sdf_batch(sources, info)
    dev = torch.device(device)
    metrics = MoleculeSetMetrics(info, reference_keys, reference_type_counts, connectivity_thresh)
    result = metrics.evaluate(torch.as_tensor(x, device=dev), torch.as_tensor(t, device=dev),
                              torch.as_tensor(mask, device=dev), groups=groups, batch=len(groups), per_group=True)
    if names is not None:
        for rec in result["groups"]:
            rec["name"] = str(names[rec["group"]])
    result["coverage"] = METRICS_COVERAGE
    return result


def write_summary(path, result, prefix="[metrics] "):
    """Prints METRICS_COVERAGE and the overall figures, writes everything to `path` (when given)."""
    print(prefix + METRICS_COVERAGE)
    print(json.dumps({k: v for k, v in result.items() if k not in ("groups", "coverage")}))
    if path:
        with open(path, "w") as f:
            json.dump(result, f, indent=1)


def main(argv=None):
    p = argparse.ArgumentParser(description="Molecule-set metrics of SDF files (one group per file)")
    p.add_argument("--sdf", nargs="+", required=True)
    p.add_argument("--dataset", default="crossdock")
    p.add_argument("--train_npz", default=None, help="processed training split: adds novelty and kl_div_atom_types")
    p.add_argument("--connectivity_thresh", type=float, default=1.0)
    p.add_argument("--out", default=None)
    p.add_argument("--device", default="cuda")
    args = p.parse_args(argv)
    info = dataset_info(args.dataset)
    ref_keys = ref_counts = None
    if args.train_npz is not None:
        from .dataset import ProcessedDataset
        ref_keys, ref_counts = reference_from_dataset(ProcessedDataset(args.train_npz, center=False), info,
                                                      device=args.device)
    result = summarize(args.sdf, info, args.sdf, args.device, ref_keys, ref_counts, args.connectivity_thresh)
    write_summary(args.out, result, prefix="")
    return result


if __name__ == "__main__":
    main()
