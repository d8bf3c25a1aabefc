"""The processed-complex files of the reference (`ProcessedLigandPocketDataset`, dataset.py:7-70) without a DataLoader:
the whole split is uploaded once and a batch is assembled by torch indexing on the device.

File format (process_crossdock.py / process_bindingmoad.py of the reference): `names`, `receptors`, `lig_coords`,
`lig_one_hot`, `lig_mask`, `pocket_coords`, `pocket_one_hot`, `pocket_mask`; complexes are split where a mask changes and
every complex is centred on the joint mean of its ligand and pocket nodes.

`collate(indices)` returns what `LigandPocketDDPM.get_ligand_and_pocket` expects from `collate_fn`; the batch masks are
int64 here (the reference builds float masks and casts them in get_ligand_and_pocket).
"""
from __future__ import annotations

import numpy as np
import torch

_LIG = ("lig_coords", "lig_one_hot")
_POCKET = ("pocket_coords", "pocket_one_hot")


def epoch_permutation(n, seed, epoch):
    """The shuffling of one epoch: a function of (seed, epoch) alone, so a resumed run continues the same order."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(epoch)) % (2 ** 63))
    return torch.randperm(n, generator=g)


class ProcessedDataset:
    def __init__(self, npz_path, center=True, transform=None, device="cpu"):
        self.transform = transform
        self.device = torch.device(device)
        with np.load(npz_path, allow_pickle=False) as f:
            keys = list(f.keys())
            data = {}
            for k in keys:
                try:
                    data[k] = f[k]
                except ValueError:                      # object arrays of names: the reference's files store them pickled
                    with np.load(npz_path, allow_pickle=True) as fp:
                        data[k] = fp[k]
        for k in _LIG + _POCKET + ("lig_mask", "pocket_mask", "names"):
            if k not in data:
                raise KeyError(f"{npz_path}: no '{k}' (not a processed ligand-pocket file)")
        self.names = list(data["names"])
        self.receptors = list(data["receptors"]) if "receptors" in data else None
        self.items = {}
        for side, mask_key in (("lig", "lig_mask"), ("pocket", "pocket_mask")):
            sections = np.where(np.diff(data[mask_key]))[0] + 1
            for k, v in data.items():
                if k.startswith(side + "_"):
                    self.items[k] = [torch.from_numpy(np.ascontiguousarray(x)) for x in np.split(v, sections)]
        self.num_lig_atoms = torch.tensor([len(x) for x in self.items["lig_mask"]])
        self.num_pocket_nodes = torch.tensor([len(x) for x in self.items["pocket_mask"]])
        if len(self.num_lig_atoms) != len(self.names) or len(self.num_pocket_nodes) != len(self.names):
            raise ValueError(f"{npz_path}: {len(self.names)} names, {len(self.num_lig_atoms)} ligands, "
                             f"{len(self.num_pocket_nodes)} pockets")
        if center:
            lc, pc = self.items["lig_coords"], self.items["pocket_coords"]
            for i in range(len(lc)):                    # dataset.py:35-41, same arithmetic
                mean = (lc[i].sum(0) + pc[i].sum(0)) / (len(lc[i]) + len(pc[i]))
                lc[i] = lc[i] - mean
                pc[i] = pc[i] - mean
        # the device copy: flat arrays + first row of every complex
        self._flat = {k: torch.cat(self.items[k], 0).to(self.device) for k in _LIG + _POCKET}
        self._ptr, self._size, self._size_host = {}, {}, {}
        for side, sizes in (("lig", self.num_lig_atoms), ("pocket", self.num_pocket_nodes)):
            self._size_host[side] = sizes.clone()
            self._size[side] = sizes.to(self.device)
            self._ptr[side] = (torch.cumsum(sizes, 0) - sizes).to(self.device)

    def __len__(self):
        return len(self.names)

    def __getitem__(self, idx):
        data = {k: v[idx] for k, v in self.items.items()}
        data["names"] = self.names[idx]
        if self.receptors is not None:
            data["receptors"] = self.receptors[idx]
        data["num_lig_atoms"] = self.num_lig_atoms[idx]
        data["num_pocket_nodes"] = self.num_pocket_nodes[idx]
        if self.transform is not None:
            data = self.transform(data)
        return data

    @staticmethod
    def collate_items(batch):
        """dataset.py:52-70 on a list of items (the host path: used when a transform is set)."""
        out = {}
        for prop in batch[0].keys():
            if prop in ("names", "receptors"):
                out[prop] = [x[prop] for x in batch]
            elif prop in ("num_lig_atoms", "num_pocket_nodes", "num_virtual_atoms"):
                out[prop] = torch.tensor([int(x[prop]) for x in batch])
            elif "mask" in prop:
                out[prop] = torch.cat([torch.full((len(x[prop]),), i, dtype=torch.int64) for i, x in enumerate(batch)], 0)
            else:
                out[prop] = torch.cat([x[prop] for x in batch], 0)
        return out

    def collate(self, indices):
        idx_host = torch.as_tensor(indices, dtype=torch.int64).cpu()
        if self.transform is not None:
            out = self.collate_items([self[int(i)] for i in idx_host])
            return {k: (v.to(self.device) if torch.is_tensor(v) else v) for k, v in out.items()}
        idx = idx_host.to(self.device)
        B = idx.numel()
        out = {"names": [self.names[int(i)] for i in idx_host]}
        if self.receptors is not None:
            out["receptors"] = [self.receptors[int(i)] for i in idx_host]
        arange_b = torch.arange(B, device=self.device)
        for side, keys, nkey in (("lig", _LIG, "num_lig_atoms"), ("pocket", _POCKET, "num_pocket_nodes")):
            total = int(self._size_host[side][idx_host].sum())         # host arithmetic: no device read-back
            sizes = self._size[side][idx]
            mask = torch.repeat_interleave(arange_b, sizes, output_size=total)
            first = torch.cumsum(sizes, 0) - sizes
            rows = self._ptr[side][idx][mask] + (torch.arange(total, device=self.device) - first[mask])
            for k in keys:
                out[k] = self._flat[k][rows]
            out[side + "_mask"] = mask
            out[nkey] = sizes
        return out
