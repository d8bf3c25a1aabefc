"""De-novo ligand generation driver: PDB in, molecules out.

Host-side mirror of `LigandPocketDDPM.__init__` / `prepare_pocket` /
`generate_ligands` (/root/reference/lightning_modules.py:31-186, :714-752,
:754-872) on top of the HIP sampling path, without Lightning, BioPython, RDKit
or OpenBabel:

  * `LigandGenerator.from_checkpoint(path)` reads a reference training
    checkpoint (Lightning format: `hyper_parameters` + `state_dict` with the
    `ddpm.` prefix) and builds the drop-in modules with the same keyword
    arguments the reference passes (`lightning_modules.py:137-173`);
  * `generate_ligands(...)` keeps the reference's signature and tensor logic:
    pocket selection, size sampling, conditional sampling or joint inpainting,
    moving the result back to the pocket frame, molecule building.

Ligands as input (`ligand_io.py`) carry the reference's two other workflows: `inpaint_ligands` /
`inpaint_for_pockets` (inpaint.py: a fixed substructure, the rest designed) and `diversify_ligands` /
`optimize_ligands` (optimize.py: partial noising + denoising of a population, selection by a caller-supplied
objective) -- and `score_ligands` (score.py: the model's own likelihood bound of given molecules, the built-in objective).
Their packed batches are written by one HIP launch (`ligand_io.pack_ligands`).

Molecules are built with the distance-table bonds of `molecules.py` (the
reference's `use_openbabel=False` path); `sanitize` / `relax_iter` need RDKit and
are refused here (convert with `Molecule.to_rdkit()` where RDKit exists).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from . import ligand_io
from . import pocket as pocket_io
from .chem_tables import dataset_info
from .conditional_model import ConditionalDDPM, SimpleConditionalDDPM
from .dynamics import EGNNDynamics
from .en_diffusion import EnVariationalDiffusion, num_nodes_to_batch_mask, seg_mean
from .molecules import Molecule, build_molecules

_DDPM_BY_MODE = {"joint": EnVariationalDiffusion,
                 "pocket_conditioning": ConditionalDDPM,
                 "pocket_conditioning_simple": SimpleConditionalDDPM}


def _get(ns, key, default=None):
    """Hyper-parameters are argparse.Namespace objects or dicts, depending on
    how the checkpoint was written."""
    if isinstance(ns, dict):
        return ns.get(key, default)
    return getattr(ns, key, default)


def load_checkpoint(path, trusted=False):
    """-> (hyper_parameters dict, state_dict).  The file is unpickled with
    `weights_only=True` plus the few plain-data classes Lightning stores; pass
    trusted=True to fall back to a full unpickle for files you wrote yourself."""
    safe = [argparse.Namespace]
    try:
        import numpy.core.multiarray as _ncm  # numpy < 2 name, kept as alias in numpy 2
        safe += [_ncm._reconstruct, np.ndarray, np.dtype]
        safe += [type(np.dtype(np.float64)), type(np.dtype(np.int64)), type(np.dtype(np.float32))]
    except Exception:   # pragma: no cover
        pass
    try:
        with torch.serialization.safe_globals(safe):
            ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:
        if not trusted:
            raise
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
    if "state_dict" not in ckpt or "hyper_parameters" not in ckpt:
        raise ValueError(f"{path}: not a Lightning checkpoint (need 'state_dict' and 'hyper_parameters')")
    return ckpt["hyper_parameters"], ckpt["state_dict"]


class LigandGenerator:
    """Sampling-only counterpart of the reference's LightningModule."""

    _RDKIT_REFUSAL = ("sanitize / relax_iter are RDKit operations; take the returned molecules' "
                      ".to_rdkit() and apply the reference's process_molecule where RDKit is installed")

    def __init__(self, dataset, egnn_params, diffusion_params, mode, node_histogram,
                 pocket_representation="CA", virtual_nodes=False, device="cuda"):
        if mode not in _DDPM_BY_MODE:
            raise ValueError(f"mode must be one of {sorted(_DDPM_BY_MODE)}")
        if pocket_representation not in ("CA", "full-atom"):
            raise ValueError("pocket_representation must be 'CA' or 'full-atom'")
        self.mode = mode
        self.pocket_representation = pocket_representation
        self.dataset_name = dataset
        self.dataset_info = dict(dataset_info(dataset))
        self.device = torch.device(device)
        info = self.dataset_info
        self.lig_type_encoder, self.lig_type_decoder = dict(info["atom_encoder"]), list(info["atom_decoder"])
        # virtual nodes (lightning_modules.py:116-135,161-173): one more ligand atom class ('Ne'), every ligand padded to
        # the largest size of the histogram during training; the class index reaches the DDPM as virtual_node_idx
        # (its losses ignore the coordinates of virtual atoms).  Sampling (lightning_modules.py:519-535): every
        # ligand gets max_num_nodes nodes and the atoms that come out as virtual are dropped before molecule building.
        self.virtual_nodes = bool(virtual_nodes)
        self.max_num_nodes = len(node_histogram) - 1
        self.virtual_atom = None
        if self.virtual_nodes:
            self.virtual_atom = len(self.lig_type_encoder)
            self.lig_type_encoder["Ne"] = self.virtual_atom
            self.lig_type_decoder.append("Ne")
        ca = pocket_representation == "CA"
        # (full-atom pockets share the ligand's encoder / decoder OBJECTS in the reference, lightning_modules.py:91-98:
        #  with virtual nodes the extra class therefore widens the pocket features as well -- mirrored, or the
        #  checkpoint's residue encoder would not load)
        self.pocket_type_encoder = info["aa_encoder"] if ca else self.lig_type_encoder
        self.pocket_type_decoder = info["aa_decoder"] if ca else self.lig_type_decoder
        if self.virtual_nodes:
            self.dataset_info["atom_encoder"], self.dataset_info["atom_decoder"] = self.lig_type_encoder, self.lig_type_decoder
        self.atom_nf, self.aa_nf, self.x_dims = len(self.lig_type_decoder), len(self.pocket_type_decoder), 3
        self.T = _get(diffusion_params, "diffusion_steps")
        # same keyword arguments as lightning_modules.py:137-159
        dyn = EGNNDynamics(
            atom_nf=self.atom_nf, residue_nf=self.aa_nf, n_dims=self.x_dims,
            joint_nf=_get(egnn_params, "joint_nf"), device=self.device,
            hidden_nf=_get(egnn_params, "hidden_nf"), act_fn=torch.nn.SiLU(),
            n_layers=_get(egnn_params, "n_layers"), attention=_get(egnn_params, "attention"),
            tanh=_get(egnn_params, "tanh"), norm_constant=_get(egnn_params, "norm_constant"),
            inv_sublayers=_get(egnn_params, "inv_sublayers"),
            sin_embedding=_get(egnn_params, "sin_embedding"),
            normalization_factor=_get(egnn_params, "normalization_factor"),
            aggregation_method=_get(egnn_params, "aggregation_method"),
            edge_cutoff_ligand=_get(egnn_params, "edge_cutoff_ligand"),
            edge_cutoff_pocket=_get(egnn_params, "edge_cutoff_pocket"),
            edge_cutoff_interaction=_get(egnn_params, "edge_cutoff_interaction"),
            update_pocket_coords=(mode == "joint"),
            reflection_equivariant=_get(egnn_params, "reflection_equivariant"),
            edge_embedding_dim=_get(egnn_params, "edge_embedding_dim"))
        # lightning_modules.py:161-173
        self.ddpm = _DDPM_BY_MODE[mode](
            dynamics=dyn, atom_nf=self.atom_nf, residue_nf=self.aa_nf, n_dims=self.x_dims,
            timesteps=self.T, noise_schedule=_get(diffusion_params, "diffusion_noise_schedule"),
            noise_precision=_get(diffusion_params, "diffusion_noise_precision"),
            loss_type=_get(diffusion_params, "diffusion_loss_type"),
            norm_values=_get(diffusion_params, "normalize_factors"),
            size_histogram=np.asarray(node_histogram), virtual_node_idx=self.virtual_atom).to(self.device)
        self.ddpm.eval()

    # -- construction from a reference checkpoint ---------------------------------------
    @classmethod
    def from_checkpoint(cls, path, device="cuda", trusted=False):
        hp, sd = load_checkpoint(path, trusted=trusted)
        gen = cls(dataset=hp["dataset"], egnn_params=hp["egnn_params"],
                  diffusion_params=hp["diffusion_params"], mode=hp["mode"],
                  node_histogram=hp["node_histogram"],
                  pocket_representation=hp.get("pocket_representation", "CA"),
                  virtual_nodes=hp.get("virtual_nodes", False), device=device)
        own = {k[len("ddpm."):]: v for k, v in sd.items() if k.startswith("ddpm.")}
        missing, unexpected = gen.ddpm.load_state_dict(own, strict=False)
        # `.4.weight` of the cross-product head aliases the coordinate head in the reference
        # (egnn_new.py:88-92); older checkpoints may or may not carry both names
        real_missing = [k for k in missing if "cross_product_mlp.4" not in k]
        if real_missing or unexpected:
            raise ValueError(f"{path}: state_dict mismatch, missing {real_missing[:5]}, "
                             f"unexpected {list(unexpected)[:5]}")
        gen.ddpm.dynamics.invalidate_engine()
        return gen

    # -- lightning_modules.py:714-752 ------------------------------------------------------
    def prepare_pocket(self, residues, repeats=1):
        if self.pocket_representation == "CA":
            coords, types, n_types = pocket_io.featurize_pocket(residues, "CA")
        else:
            coords, types, n_types = pocket_io.featurize_pocket(residues, "full-atom",
                                                                atom_encoder=self.pocket_type_encoder)
        return pocket_io.prepare_pocket(coords, types, len(self.pocket_type_encoder), repeats, self.device)

    def select_pocket_residues(self, pdb_file, pocket_ids=None, ref_ligand=None):
        """Residue selection of generate_ligands (lightning_modules.py:781-795,
        utils.py:101-128): a list of `<chain>:<resi>` ids, or everything within 8 A of
        a reference ligand given as an SDF path or as `<chain>:<resi>` of the PDB."""
        assert (pocket_ids is None) ^ (ref_ligand is None)
        residues = pocket_io.read_pdb_residues(pdb_file, hetero=True)
        if pocket_ids is not None:
            by_id = {(r["chain"], r["resseq"]): r for r in residues if not r.get("hetero")}
            return [by_id[(x.split(":")[0], int(x.split(":")[1]))] for x in pocket_ids]
        if str(ref_ligand).endswith(".sdf"):
            lig_xyz, skip = pocket_io.read_sdf_coords(ref_ligand), None
        else:
            chain, resi = ref_ligand.split(":")
            hit = [r for r in residues if r["chain"] == chain and r["resseq"] == int(resi)]
            assert len(hit) == 1, f"{ref_ligand}: {len(hit)} residues match"
            lig_xyz = np.asarray([a[2] for a in hit[0]["atoms"]], np.float32)
            skip = int(resi)
        cand = [r for r in residues if r["resseq"] != skip]   # the reference skips that number in every chain
        return pocket_io.pocket_residues_from_ligand(cand, lig_xyz)

    # -- lightning_modules.py:754-872 ------------------------------------------------------
    @torch.no_grad()
    def generate_ligands(self, pdb_file, n_samples, pocket_ids=None, ref_ligand=None, num_nodes_lig=None,
                         sanitize=False, largest_frag=False, relax_iter=0, timesteps=None,
                         n_nodes_bias=0, n_nodes_min=0, pose=None, vina=None, **kwargs):
        """`pose=True` (or a dict of `tol` / `contact`) checks every sample against the heavy atoms of the selected
        residues on the device (pose.py) and attaches the record as `m.pose`.  `vina=True` scores every sample against
        the same atoms (vina.py: a Vina-type score, not smina output) and attaches the record as `m.vina`."""
        if sanitize or relax_iter:
            raise NotImplementedError(self._RDKIT_REFUSAL)
        pose, vina = self._pose_options(pose), self._vina_options(vina)
        residues = self.select_pocket_residues(pdb_file, pocket_ids, ref_ligand)
        pocket = self.prepare_pocket(residues, repeats=n_samples)
        xh_lig, lig_mask = self.sample_for_pocket(pocket, n_samples, num_nodes_lig, timesteps,
                                                  n_nodes_bias, n_nodes_min, **kwargs)
        x, atom_type, lig_mask = self._drop_virtual(xh_lig, lig_mask)
        return build_molecules(x, atom_type, lig_mask, self.dataset_info, largest_frag=largest_frag, batch=n_samples,
                               **self._annotate(x, atom_type, lig_mask, [residues], [n_samples], pose, vina))

    def _drop_virtual(self, xh_lig, lig_mask):
        """(x, atom_type, lig_mask) of the generated atoms; with virtual nodes the atoms of the virtual class are
        removed first (lightning_modules.py:531-537)."""
        x = xh_lig[:, :self.x_dims]
        atom_type = xh_lig[:, self.x_dims:].argmax(1)
        if self.virtual_nodes:
            keep = atom_type != self.virtual_atom
            x, atom_type, lig_mask = x[keep], atom_type[keep], lig_mask[keep]
        return x, atom_type, lig_mask

    # -- pose checks of the sampled batch (pose.py): only with the samplers' `pose=` option ------------------------------
    @staticmethod
    def _pose_options(pose):
        """The samplers' `pose` keyword: None / False = off (nothing runs); True = the module's defaults; a dict with
        'tol' / 'contact' (and 'residues' where the sampler is not given any: `diversify_ligands`)."""
        if pose is None or pose is False:
            return None
        from . import pose as pose_mod
        opts = {} if pose is True else dict(pose)
        unknown = set(opts) - {"tol", "contact", "residues"}
        if unknown:
            raise ValueError(f"pose: unknown option(s) {sorted(unknown)}")
        opts.setdefault("tol", pose_mod.CLASH_TOLERANCE)
        opts.setdefault("contact", pose_mod.CONTACT_CUTOFF)
        return opts

    # -- Vina-type score of the sampled batch (vina.py): only with the samplers' `vina=` option -----------------------------
    @staticmethod
    def _vina_options(vina):
        """The samplers' `vina` keyword: None / False = off (nothing runs); True = on; a dict may carry 'residues' where the
        sampler is not given any (`diversify_ligands`) and 'minimize': True, or a dict of `step` / `tol` / `max_evals`, also
        relaxes every sample as a rigid body (vina.vina_minimize) and attaches that record as `m.vina_min`; with
        `torsions`: True in that dict (and `dofs`) the rotatable bonds turn as well, under inter + intra, and the record
        is the flexible one (`vina.MolVinaFlex`)."""
        if vina is None or vina is False:
            return None
        opts = {} if vina is True else dict(vina)
        unknown = set(opts) - {"residues", "minimize"}
        if unknown:
            raise ValueError(f"vina: unknown option(s) {sorted(unknown)}")
        minimize = opts.pop("minimize", None)
        if minimize is not None and minimize is not False:
            settings = {} if minimize is True else dict(minimize)
            unknown = set(settings) - {"step", "tol", "max_evals", "torsions", "dofs"}
            if unknown:
                raise ValueError(f"vina: unknown minimize setting(s) {sorted(unknown)}")
            opts["minimize"] = settings
        return opts

    def _job_pockets(self, attr, residue_sets, kind, atoms_of):
        """The heavy atoms of every job's residues as one `kind` (`pose.PocketAtoms` / `vina.VinaPocket`) on the device, one
        group per job.  A residue list is read by `atoms_of` and uploaded once (a test-set job hands the same list to every
        one of its batches) and kept in the dict `attr` while the list lives here."""
        cache = self.__dict__.setdefault(attr, {})
        parts = []
        for residues in residue_sets:
            hit = cache.get(id(residues))
            if hit is None or hit[0] is not residues:
                while len(cache) >= 256:
                    cache.pop(next(iter(cache)))
                hit = (residues, kind.upload([atoms_of(residues)], self.device))
                cache[id(residues)] = hit
            parts.append(hit[1])
        return kind.concat(parts)

    def _annotate(self, x, atom_type, lig_mask, residue_sets, counts, pose, vina):
        """The records of a sampled batch (after `_drop_virtual`) that `build_molecules` attaches: `pose.pose_check` and
        `vina.vina_score`, each only with its option; one group per job, `counts[k]` samples on group k.  `residue_sets`
        None: the one list an option carries as 'residues'.  -> dict(pose=..., vina=...), None where off."""
        out = dict(pose=None, vina=None)
        groups, batch = np.repeat(np.arange(len(counts)), counts), int(sum(counts))
        if pose is not None:
            from . import pose as pose_mod
            if "_pose_radii" not in self.__dict__:
                self._pose_radii = torch.as_tensor(pose_mod.radius_table(self.lig_type_decoder), device=self.device)
            sets = [pose["residues"]] if residue_sets is None else residue_sets
            pockets = self._job_pockets("_pose_pockets", sets, pose_mod.PocketAtoms, pose_mod.pocket_atoms)
            out["pose"] = pose_mod.pose_check(x, self._pose_radii[atom_type], lig_mask, pockets, groups, batch=batch,
                                              tol=pose["tol"], contact=pose["contact"])
        if vina is not None:
            from . import vina as vina_mod
            sets = [vina["residues"]] if residue_sets is None else residue_sets
            pockets = self._job_pockets("_vina_pockets", sets, vina_mod.VinaPocket, vina_mod.type_pocket)
            if "minimize" not in vina:
                out["vina"] = vina_mod.vina_score(x, atom_type, lig_mask, pockets, self.dataset_info, groups, batch=batch)
            else:                                                    # m.vina_min; x and m.vina stay as they are
                orders = vina_mod.perceive_orders(x, atom_type, lig_mask, self.dataset_info, batch)     # once, for both entries
                out["vina"] = vina_mod.vina_score(x, atom_type, lig_mask, pockets, self.dataset_info, groups, batch=batch,
                                                  orders=orders)
                out["vina_min"] = vina_mod.vina_minimize(x, atom_type, lig_mask, pockets, self.dataset_info, groups, batch=batch,
                                                         orders=orders, **vina["minimize"])
        return out

    def _scope_residues(self, pdb_file, scope, pocket_ids, ref_ligand):
        """scope 'protein': every ATOM residue of the file; 'pocket': the selection of `generate_ligands`."""
        if scope == "pocket":
            return self.select_pocket_residues(pdb_file, pocket_ids, ref_ligand)
        if scope == "protein":
            return pocket_io.read_pdb_residues(pdb_file)
        raise ValueError("scope must be 'protein' or 'pocket'")

    @torch.no_grad()
    def vina_scores(self, pdb_file, molecules, pocket_ids=None, ref_ligand=None, scope="protein"):
        """Vina-type score of given molecules against the protein of `pdb_file` (vina.py; bonds perceived from distances as
        for generated molecules).  `molecules` and `scope` as for `check_poses`.  Returns one dict per molecule, in order:
        {'n_atoms', 'untyped', 'n_rot', 'nonfinite', 'gauss1', 'gauss2', 'repulsion', 'hydrophobic', 'hbond', 'inter',
        'score'} over heavy atoms.  Not smina output: see `vina.VINA_COVERAGE`."""
        from . import vina as vina_mod
        residues = self._scope_residues(pdb_file, scope, pocket_ids, ref_ligand)
        pockets = vina_mod.VinaPocket.upload([vina_mod.type_pocket(residues)], self.device)
        return [r.as_dict() for r in vina_mod.score_molecules(molecules, pockets, self.dataset_info)]

    @torch.no_grad()
    def vina_gradients(self, pdb_file, molecules, pocket_ids=None, ref_ligand=None, scope="protein"):
        """`vina_scores` with the gradient of the score's `inter` term with respect to the heavy-atom coordinates, from
        the same launch (vina.py: `gradient_molecules`).  The same arguments.  Returns one dict per molecule, in order:
        the keys of `vina_scores`, 'grad' (float32 [n, 3], kcal/mol/A; times 'rot_factor' = the gradient of 'score'),
        'net', 'moment' (about the centroid), 'max_norm', 'rot_factor'.  See `vina.VINA_GRAD_COVERAGE`: ligand atoms only,
        rigid protein, constant typing, no minimiser."""
        from . import vina as vina_mod
        residues = self._scope_residues(pdb_file, scope, pocket_ids, ref_ligand)
        pockets = vina_mod.VinaPocket.upload([vina_mod.type_pocket(residues)], self.device)
        return [dict(r.as_dict(), grad=r.grad) for r in vina_mod.gradient_molecules(molecules, pockets, self.dataset_info)]

    @torch.no_grad()
    def vina_minimize(self, pdb_file, molecules, pocket_ids=None, ref_ligand=None, scope="protein", **settings):
        """`vina_gradients` after a rigid-body relaxation of every molecule in the protein under the score's `inter` term,
        one launch for all of them (vina.py: `minimize_molecules`; `settings`: `step`, `tol`, `max_evals`).  The same
        arguments.  Returns one dict per molecule, in order: the keys of `vina_gradients` at the returned pose, 'x'
        (float32 [n, 3], its heavy-atom coordinates), 'inter_start', 'score_start', 'status' (index into `vina.STATUS`),
        'evals', 'accepted', 'rmsd'.  See `vina.VINA_MIN_COVERAGE`: rigid ligand, rigid protein, a local search, not smina
        or qvina output.
        With `torsions=True` among the settings (and `dofs`) the relaxation is the flexible one, under inter + intra with
        the rotatable bonds turning; the dicts gain 'intra', 'intra_start', 'n_torsions', 'torsions_found' and 'theta'.
        See `vina.VINA_FLEX_COVERAGE`."""
        from . import vina as vina_mod
        residues = self._scope_residues(pdb_file, scope, pocket_ids, ref_ligand)
        pockets = vina_mod.VinaPocket.upload([vina_mod.type_pocket(residues)], self.device)
        return [dict(r.as_dict(), grad=r.grad, x=r.x, **({"theta": r.theta} if hasattr(r, "theta") else {}))
                for r in vina_mod.minimize_molecules(molecules, pockets, self.dataset_info, **settings)]

    @torch.no_grad()
    def check_poses(self, pdb_file, molecules, pocket_ids=None, ref_ligand=None, scope="protein", tol=None, contact=None):
        """Clash and contact counts of given molecules against the protein of `pdb_file` (pose.py; one launch).
        `molecules` as for `score_ligands`: `Molecule` objects, (xyz, elements) pairs or an SDF path.  scope 'protein':
        every ATOM residue of the file; 'pocket': the selection of `generate_ligands` (`pocket_ids` or `ref_ligand`).
        Returns one dict per molecule, in order: {'n_atoms', 'clash_pairs', 'clash_atoms', 'contact_pairs',
        'contact_atoms', 'nonfinite', 'min_distance'} over heavy atoms."""
        from . import pose as pose_mod
        residues = self._scope_residues(pdb_file, scope, pocket_ids, ref_ligand)
        pockets = pose_mod.PocketAtoms.upload([pose_mod.pocket_atoms(residues)], self.device)
        records = pose_mod.check_molecules(molecules, pockets, tol=pose_mod.CLASH_TOLERANCE if tol is None else tol,
                                           contact=pose_mod.CONTACT_CUTOFF if contact is None else contact)
        return [r.as_dict() for r in records]

    def _ligand_sizes(self, num_nodes_lig, n_nodes_bias=0, n_nodes_min=0):
        """Bias and minimum of generate_ligands (lightning_modules.py:806-811).  With virtual nodes every ligand already
        has `max_num_nodes` slots (the validation-time rule, :519-520, which this package uses for generation too --
        INTEGRATION.md "virtual nodes"); a positive bias must not ask for more nodes than any training sample had, so the
        sizes stay <= max_num_nodes."""
        n = torch.clamp(torch.as_tensor(num_nodes_lig, dtype=torch.int64) + n_nodes_bias, min=n_nodes_min)
        if self.virtual_nodes:
            n = torch.clamp(n, max=self.max_num_nodes)
        return n

    @torch.no_grad()
    def sample_for_pocket(self, pocket, n_samples, num_nodes_lig=None, timesteps=None,
                          n_nodes_bias=0, n_nodes_min=0, **kwargs):
        """The tensor part of generate_ligands (lightning_modules.py:797-852):
        returns (xh_lig in the pocket's original frame, lig_mask)."""
        pocket_com_before = self.ddpm._seg_mean3(pocket["x"].float(), pocket["mask"], n_samples)
        if num_nodes_lig is None:
            if self.virtual_nodes:                          # lightning_modules.py:519-520
                num_nodes_lig = torch.full((n_samples,), self.max_num_nodes, dtype=torch.int64)
            else:
                num_nodes_lig = self.ddpm.size_distribution.sample_conditional(n1=None, n2=pocket["size"])
        num_nodes_lig = self._ligand_sizes(num_nodes_lig, n_nodes_bias, n_nodes_min)
        if type(self.ddpm) == EnVariationalDiffusion:
            lig_mask = num_nodes_to_batch_mask(len(num_nodes_lig), num_nodes_lig, self.device)
            ligand = {"x": torch.zeros((len(lig_mask), self.x_dims), device=self.device),
                      "one_hot": torch.zeros((len(lig_mask), self.atom_nf), device=self.device),
                      "size": num_nodes_lig.to(self.device), "mask": lig_mask}
            lig_fixed = torch.zeros(len(lig_mask), device=self.device)
            pocket_fixed = torch.ones(len(pocket["mask"]), device=self.device)
            xh_lig, xh_pocket, lig_mask, pocket_mask = self.ddpm.inpaint(
                ligand, pocket, lig_fixed, pocket_fixed, timesteps=timesteps, **kwargs)
        elif type(self.ddpm) == ConditionalDDPM:
            xh_lig, xh_pocket, lig_mask, pocket_mask = self.ddpm.sample_given_pocket(
                pocket, num_nodes_lig, timesteps=timesteps)
        else:
            raise NotImplementedError
        pocket_com_after = self.ddpm._seg_mean3(xh_pocket[:, :self.x_dims], pocket_mask, n_samples)
        shift = pocket_com_before - pocket_com_after
        xh_lig = xh_lig.clone()
        xh_lig[:, :self.x_dims] += shift[lig_mask]
        return xh_lig, lig_mask


    # -- several different pockets in one batch ---------------------------
    @torch.no_grad()
    def generate_for_pockets(self, jobs, timesteps=None, largest_frag=False, n_nodes_bias=0,
                             n_nodes_min=0, seed=None, sample_ids=None, pose=None, vina=None, **kwargs):
        """One sampling batch over several different pockets.

        The reference's test driver (test.py:59-176) samples one pocket at a time; the
        graph is block diagonal per sample (dynamics.py:170-172), so pockets of different
        proteins can share a batch and keep the GPU full when a single pocket needs fewer
        samples than fit.  `jobs`: list of (residues, n_samples, num_nodes_lig or None).
        Returns one list of molecules per job.  With keyed noise (`seed`, and `sample_ids` = one
        global id per slot of the packed batch) a sample is the same molecule in any packing that
        gives it the same global id.
        `pose=True` (or a dict of `tol` / `contact`): one more launch checks every sample against the heavy atoms of its
        job's residues before the molecules are built; every molecule carries the record as `m.pose`.
        `vina=True`: two more launches score every sample against the same atoms (vina.py); the record is `m.vina`."""
        pose, vina = self._pose_options(pose), self._vina_options(vina)
        parts, sizes, counts = [], [], []
        base = 0
        for residues, n, n_lig in jobs:
            pk = self.prepare_pocket(residues, repeats=n)
            pk["mask"] = pk["mask"] + base
            parts.append(pk)
            if n_lig is None:
                n_lig = torch.full((n,), self.max_num_nodes, dtype=torch.int64) if self.virtual_nodes else \
                    self.ddpm.size_distribution.sample_conditional(n1=None, n2=pk["size"])
            n_lig = torch.as_tensor(n_lig, dtype=torch.int64).cpu()
            assert n_lig.numel() == n
            sizes.append(n_lig)
            counts.append(n)
            base += n
        pocket = {k: torch.cat([p[k] for p in parts]) for k in ("x", "one_hot", "size", "mask")}
        if seed is not None:
            self.ddpm.seed(seed, sample_ids=sample_ids)
        xh_lig, lig_mask = self.sample_for_pocket(pocket, base, torch.cat(sizes), timesteps,
                                                  n_nodes_bias, n_nodes_min, **kwargs)
        x, atom_type, lig_mask = self._drop_virtual(xh_lig, lig_mask)
        mols = build_molecules(x, atom_type, lig_mask, self.dataset_info, largest_frag=largest_frag, batch=base,
                               **self._annotate(x, atom_type, lig_mask, [j[0] for j in jobs], counts, pose, vina))
        out, o = [], 0
        for n in counts:
            out.append(mols[o:o + n])
            o += n
        return out


    # -- substructure inpainting (the reference's inpaint.py:63-189) ------------------------------------------
    def _check_inpaint_model(self, center):
        """ConditionalDDPM: both centring options.  Joint model: `inpaint` with every pocket node fixed, which has no
        centring argument (the reference's script cannot run it at all: it passes `center=`).  The simple conditional
        model has no pinned chain, as in `sample_for_pocket`."""
        if center not in ("ligand", "pocket"):
            raise ValueError("center must be 'ligand' or 'pocket'")
        if type(self.ddpm) == EnVariationalDiffusion:
            if center != "ligand":
                raise ValueError("the joint model centres on the known nodes; only the default center='ligand' is accepted")
        elif type(self.ddpm) != ConditionalDDPM:
            raise NotImplementedError(f"inpainting front end: {type(self.ddpm).__name__} is not supported")

    def prepare_substructure(self, pdb_file, ref_ligand, fix_atoms):
        """The atoms to keep (inpaint.py:47-60) -> (xyz float32 [n,3], int32 class ids): the first molecule of every
        SDF file of `fix_atoms`, concatenated, or the atoms of the PDB ligand `<chain>:<resi>` whose names are in
        `fix_atoms`, in file order."""
        fix_atoms = [fix_atoms] if isinstance(fix_atoms, str) else list(fix_atoms)
        if not fix_atoms:
            raise ValueError("fix_atoms is empty")
        if str(fix_atoms[0]).endswith(".sdf"):
            mols = [ligand_io.read_sdf_molecules(f)[0] for f in fix_atoms]
            xyz = np.concatenate([m[0] for m in mols])
            elements = sum((m[1] for m in mols), [])
        else:
            if str(ref_ligand).endswith(".sdf"):
                raise ValueError("atom names need the ligand inside the PDB file (ref_ligand = <chain>:<resi>)")
            residues = pocket_io.read_pdb_residues(pdb_file, hetero=True)
            xyz, elements = ligand_io.ligand_atoms_from_pdb(residues, ref_ligand, fix_atoms)
        return xyz, ligand_io.encode_elements(elements, self.lig_type_encoder)

    def _inpaint_chain(self, pocket, ligand, lig_fixed, n, center, resamplings, timesteps, frames, jump_length):
        """ddpm.inpaint on a packed batch + the move back into the pocket's frame (inpaint.py:143-170).
        -> (xh_lig [rows, 3 + atom_nf], lig_mask); with frames > 1 the rows are the frames one after the other,
        noisiest first, and the mask numbers the frames (utils.reverse_tensor, inpaint.py:152-162)."""
        nd = self.x_dims
        pocket_com_before = self.ddpm._seg_mean3(pocket["x"].float(), pocket["mask"], n)
        if type(self.ddpm) == EnVariationalDiffusion:
            pocket_fixed = torch.ones(len(pocket["mask"]), device=self.device)
            xh_lig, xh_pocket, lig_mask, pocket_mask = self.ddpm.inpaint(
                ligand, pocket, lig_fixed, pocket_fixed, resamplings=resamplings, jump_length=jump_length,
                return_frames=frames, timesteps=timesteps)
        else:
            xh_lig, xh_pocket, lig_mask, pocket_mask = self.ddpm.inpaint(
                ligand, pocket, lig_fixed, center=center, resamplings=resamplings, timesteps=timesteps,
                return_frames=frames)
        if frames > 1:
            n = xh_lig.size(0)
            xh_lig, xh_pocket = xh_lig.flip(0), xh_pocket.flip(0)
            lig_mask = torch.arange(n, device=self.device).repeat_interleave(len(lig_mask))
            pocket_mask = torch.arange(n, device=self.device).repeat_interleave(len(pocket_mask))
            xh_lig = xh_lig.reshape(-1, xh_lig.size(2))
            xh_pocket = xh_pocket.reshape(-1, xh_pocket.size(2))
        pocket_com_after = self.ddpm._seg_mean3(xh_pocket[:, :nd], pocket_mask, n)
        shift = pocket_com_before - pocket_com_after          # ([1,3] - [frames,3] for a trajectory)
        xh_lig = xh_lig.clone()
        xh_lig[:, :nd] += shift[lig_mask]
        return xh_lig, lig_mask

    @torch.no_grad()
    def inpaint_ligands(self, pdb_file, n_samples, ref_ligand, fix_atoms, add_n_nodes=None, center="ligand",
                        sanitize=False, largest_frag=False, relax_iter=0, timesteps=None, resamplings=1,
                        save_traj=False, seed=None, jump_length=1):
        """Design the rest of a ligand around a fixed substructure: the reference's `inpaint_ligand`
        (inpaint.py:63-189) with its keywords.  `ref_ligand` (SDF path or `<chain>:<resi>`) defines the pocket;
        `fix_atoms` is a list of SDF files or of atom names of the PDB ligand.  Sizes: drawn from p(n | pocket size) and
        raised to the number of fixed atoms, or `n_fixed + add_n_nodes`.  `save_traj` (n_samples = 1) returns the
        `timesteps` frames as molecules, noisiest first, without fragment selection.  `seed` keys the noise (and the
        size draw); `jump_length` reaches the joint model only."""
        if sanitize or relax_iter:
            raise NotImplementedError(self._RDKIT_REFUSAL)
        if save_traj and n_samples > 1:
            raise NotImplementedError("Can only visualize trajectory with n_samples=1.")
        self._check_inpaint_model(center)
        timesteps = self.T if timesteps is None else timesteps
        frames = timesteps if save_traj else 1
        largest_frag = False if save_traj else largest_frag
        residues = self.select_pocket_residues(pdb_file, ref_ligand=ref_ligand)
        pocket = self.prepare_pocket(residues, repeats=n_samples)
        x_fixed, t_fixed = self.prepare_substructure(pdb_file, ref_ligand, fix_atoms)
        with torch.random.fork_rng(devices=[], enabled=seed is not None):
            if seed is not None:
                torch.manual_seed(int(seed))
            sizes = ligand_io.inpaint_sizes(self.ddpm.size_distribution, pocket["size"].cpu(), len(x_fixed), add_n_nodes)
        tmpl_x, tmpl_t, tmpl_sizes = ligand_io.upload_templates([(x_fixed, t_fixed)], self.device)
        ligand, lig_fixed = ligand_io.pack_ligands(tmpl_x, tmpl_t, tmpl_sizes, [0] * n_samples, sizes.tolist(),
                                                   self.atom_nf)
        if seed is not None:
            self.ddpm.seed(seed)
        xh_lig, lig_mask = self._inpaint_chain(pocket, ligand, lig_fixed, n_samples, center, resamplings, timesteps,
                                               frames, jump_length)
        x, atom_type, lig_mask = self._drop_virtual(xh_lig, lig_mask)
        return build_molecules(x, atom_type, lig_mask, self.dataset_info, largest_frag=largest_frag,
                               batch=frames if save_traj else n_samples)

    @torch.no_grad()
    def inpaint_for_pockets(self, jobs, timesteps=None, resamplings=1, center="ligand", largest_frag=False,
                            seed=None, sample_ids=None, jump_length=1, cone_mode=2, pose=None, vina=None):
        """Several design jobs in one batch: the packed-batch twin of `generate_for_pockets`.  `jobs`: list of
        (residues, n_samples, substructure, add_n_nodes or sizes) -- `substructure` a `Molecule` or an (xyz, elements)
        pair, the last entry None (sizes drawn), an int (atoms to add) or one ligand size per sample.  Returns one list
        of molecules per job.  With keyed noise (`seed`, and `sample_ids` = one global id per slot of the packed
        batch, default 0, 1, ...) a sample is the same molecule, bit for bit, in any packing that gives it the same
        id.  For that the engine's per-batch choices must not follow the packing either: the forward cone, which the
        model otherwise switches by the number of distinct pockets in the batch (en_diffusion.cone_mode; on and off
        differ in rounding), is pinned to `cone_mode` (2 = on, 0 = off; None = the model's own per-batch rule) and the
        automatic 16-row granule is switched off for the call, as the test-set driver does (testset.make_hip_sampler).
        `pose`, `vina`: as for `generate_for_pockets`."""
        self._check_inpaint_model(center)
        pose, vina = self._pose_options(pose), self._vina_options(vina)
        if cone_mode not in (None, 0, 2):
            raise ValueError("cone_mode must be 2, 0 or None")
        parts, templates, slot_tmpl, sizes, counts = [], [], [], [], []
        base = 0
        for residues, n, sub, extra in jobs:
            pk = self.prepare_pocket(residues, repeats=n)
            pk["mask"] = pk["mask"] + base
            parts.append(pk)
            (xyz, types), = ligand_io.as_templates([sub], self.lig_type_encoder)
            if extra is None or isinstance(extra, (int, np.integer)):
                n_lig = ligand_io.inpaint_sizes(self.ddpm.size_distribution, pk["size"].cpu(), len(xyz), extra)
            else:
                n_lig = torch.as_tensor(extra, dtype=torch.int64).cpu().reshape(-1)
            assert n_lig.numel() == n
            slot_tmpl += [len(templates)] * n
            templates.append((xyz, types))
            sizes.append(n_lig)
            counts.append(n)
            base += n
        pocket = {k: torch.cat([p[k] for p in parts]) for k in ("x", "one_hot", "size", "mask")}
        tmpl_x, tmpl_t, tmpl_sizes = ligand_io.upload_templates(templates, self.device)
        ligand, lig_fixed = ligand_io.pack_ligands(tmpl_x, tmpl_t, tmpl_sizes, slot_tmpl, torch.cat(sizes).tolist(),
                                                   self.atom_nf)
        if seed is not None:
            self.ddpm.seed(seed, sample_ids=sample_ids)
        saved = self.ddpm.cone_mode, self.ddpm.edge_granule16
        if cone_mode is not None:
            self.ddpm.cone_mode = cone_mode
            if saved[1] == "auto":
                self.ddpm.edge_granule16 = 0
        try:
            xh_lig, lig_mask = self._inpaint_chain(pocket, ligand, lig_fixed, base, center, resamplings,
                                                   self.T if timesteps is None else timesteps, 1, jump_length)
        finally:
            self.ddpm.cone_mode, self.ddpm.edge_granule16 = saved
        x, atom_type, lig_mask = self._drop_virtual(xh_lig, lig_mask)
        mols = build_molecules(x, atom_type, lig_mask, self.dataset_info, largest_frag=largest_frag, batch=base,
                               **self._annotate(x, atom_type, lig_mask, [j[0] for j in jobs], counts, pose, vina))
        out, o = [], 0
        for n in counts:
            out.append(mols[o:o + n])
            o += n
        return out

    # -- diversification and the evolutionary loop (the reference's optimize.py) ------------------------------
    def _diversify_chain(self, pocket, ligand, noising_steps):
        """ddpm.diversify on a packed batch + the move back into the pocket's frame (optimize.py:116-128)."""
        if not hasattr(self.ddpm, "diversify"):
            raise NotImplementedError(f"{type(self.ddpm).__name__} has no diversify (pocket-conditioned models only)")
        n = len(pocket["size"])
        pocket_com_before = self.ddpm._seg_mean3(pocket["x"].float(), pocket["mask"], n)
        out_lig, out_pocket, lig_mask, pocket_mask = self.ddpm.diversify(ligand, pocket, noising_steps=noising_steps)
        pocket_com_after = self.ddpm._seg_mean3(out_pocket[:, :self.x_dims], pocket_mask, n)
        out_lig = out_lig.clone()
        out_lig[:, :self.x_dims] += (pocket_com_before - pocket_com_after)[lig_mask]
        return out_lig, lig_mask

    @torch.no_grad()
    def diversify_ligands(self, pocket, molecules, noising_steps, largest_frag=False, seed=None, pose=None, vina=None):
        """Partially noise and denoise ligands in their pocket: the reference's `diversify_ligands`
        (optimize.py:92-147).  `pocket`: the dict of `prepare_pocket(residues, repeats=len(molecules))`; `molecules`:
        a list of `Molecule` objects or (xyz, elements) pairs, or an SDF path -- one ligand per pocket replica.
        Returns one molecule per input, in order.  `pose`: a dict with `residues` (the residues `pocket` was prepared from:
        the pocket dict holds the model's nodes, not the protein's atoms) and optionally `tol` / `contact` attaches the pose
        record of every result as `m.pose`.  `vina`: a dict with `residues` attaches the Vina-type score record of every
        result as `m.vina` (vina.py)."""
        if not hasattr(self.ddpm, "diversify"):
            raise NotImplementedError(f"{type(self.ddpm).__name__} has no diversify (pocket-conditioned models only)")
        pose, vina = self._pose_options(pose), self._vina_options(vina)
        if vina is not None and vina.get("residues") is None:
            raise ValueError("diversify_ligands: vina needs the residues the pocket was prepared from (vina=dict(residues=...))")
        if pose is not None and pose.get("residues") is None:
            raise ValueError("diversify_ligands: pose needs the residues the pocket was prepared from (pose=dict(residues=...))")
        templates = ligand_io.as_templates(molecules, self.lig_type_encoder)
        n = len(pocket["size"])
        if len(templates) != n:
            raise ValueError(f"{len(templates)} ligands for {n} pocket replicas (one ligand per replica)")
        tmpl_x, tmpl_t, tmpl_sizes = ligand_io.upload_templates(templates, self.device)
        ligand, _ = ligand_io.pack_ligands(tmpl_x, tmpl_t, tmpl_sizes, list(range(n)), tmpl_sizes, self.atom_nf)
        if seed is not None:
            self.ddpm.seed(seed)
        xh_lig, lig_mask = self._diversify_chain(pocket, ligand, noising_steps)
        x, atom_type, lig_mask = self._drop_virtual(xh_lig, lig_mask)
        return build_molecules(x, atom_type, lig_mask, self.dataset_info, largest_frag=largest_frag, batch=n,
                               **self._annotate(x, atom_type, lig_mask, None, [n], pose, vina))

    # -- scoring given ligands (score.py) ---------------------------------------------------------------------
    @torch.no_grad()
    def score_ligands(self, pdb_file, molecules, pocket_ids=None, ref_ligand=None, n_times=10, seed=0, max_states=64):
        """The model's negative log-likelihood bound of given molecules in one pocket (lower = more likely under the
        model): `ddpm.nll_given_pocket` under a pocket-conditioned model, `ddpm.nll_of_complex(center=True)` under a joint
        one (the bound of the whole complex: for candidates in one pocket it ranks as the conditional bound does).
        `molecules` as for `diversify_ligands`: `Molecule` objects, (xyz, elements) pairs or an SDF path; the pocket is
        selected as in `generate_ligands`.  `n_times` time slots per molecule on one seeded grid shared by all of them
        ('all': every diffusion time).  Returns one dict per molecule, in order:
        {'nll', 'loss_t', 'loss_0', 'kl_prior', 'log_pN', 'n_atoms'}; a joint model adds 'loss_t_lig', the ligand rows'
        share of loss_t."""
        from .conditional_model import ConditionalDDPM
        from .en_diffusion import EnVariationalDiffusion
        joint = not isinstance(self.ddpm, ConditionalDDPM)
        if joint and not isinstance(self.ddpm, EnVariationalDiffusion):
            raise NotImplementedError(f"{type(self.ddpm).__name__}: ligands are scored under pocket-conditioned models "
                                      "(nll_given_pocket) and joint models (nll_of_complex) only")
        templates = ligand_io.as_templates(molecules, self.lig_type_encoder)
        n = len(templates)
        if n < 1:
            raise ValueError("no molecule to score")
        residues = self.select_pocket_residues(pdb_file, pocket_ids, ref_ligand)
        pocket = self.prepare_pocket(residues, repeats=n)
        tmpl_x, tmpl_t, tmpl_sizes = ligand_io.upload_templates(templates, self.device)
        ligand, _ = ligand_io.pack_ligands(tmpl_x, tmpl_t, tmpl_sizes, list(range(n)), tmpl_sizes, self.atom_nf)
        grid = dict(times="all") if isinstance(n_times, str) else dict(n_times=n_times)
        if joint:
            nll, terms = self.ddpm.nll_of_complex(ligand, pocket, seed=seed, max_states=max_states, center=True,
                                                  return_terms=True, **grid)
            loss_0 = ((terms["loss_0_x_ligand"] + terms["loss_0_x_pocket"]) + terms["loss_0_h"]) + terms["neg_log_constants"]
        else:
            nll, terms = self.ddpm.nll_given_pocket(ligand, pocket, seed=seed, max_states=max_states, return_terms=True, **grid)
            loss_0 = (terms["loss_0_x"] + terms["loss_0_h"]) + terms["neg_log_constants"]
        names = ["nll", "loss_t", "loss_0", "kl_prior", "log_pN"] + (["loss_t_lig"] if joint else [])
        cols = torch.stack([nll, terms["loss_t"], loss_0, terms["kl_prior"], terms["log_pN"]]
                           + ([terms["loss_t_lig"]] if joint else [])).cpu().tolist()
        return [dict({k: cols[j][i] for j, k in enumerate(names)}, n_atoms=int(tmpl_sizes[i])) for i in range(n)]

    def reference_ligand(self, pdb_file, ref_ligand):
        """(xyz, element symbols) of the ligand that defines the pocket: first record of an SDF file, or the group
        `<chain>:<resi>` of the PDB file."""
        if str(ref_ligand).endswith(".sdf"):
            return ligand_io.read_sdf_molecules(ref_ligand)[0]
        return ligand_io.ligand_atoms_from_pdb(pocket_io.read_pdb_residues(pdb_file, hetero=True), ref_ligand)

    def _population_step(self, pocket, reference, noising_steps, largest_frag, seed):
        """`diversify(parent_ids, generation)` of `evolve_population` on the HIP path.  The previous generation stays
        on the device as it came out of the chain: its coordinates, its atom classes (argmax on the device) and the
        slot sizes the host already knows ARE the template set of the next `pack_ligands` call, and a slot's template
        id is its parent's slot -- no coordinate crosses the host between generations.  That holds while every selected
        parent is its whole slot.  With `largest_frag=True`, or when virtual atoms were dropped, a parent can have
        fewer atoms than its slot: such a generation takes its parents from the host copies (the `Molecule` objects
        that went to the objective) and uploads them; `self.optimize_stats['host_template_generations']` lists the
        generations that did (generation 0, the reference ligand, always does)."""
        n = len(pocket["size"])
        (x0, t0), = ligand_io.as_templates([reference], self.lig_type_encoder)
        state = {"mols": [Molecule(x0, list(reference[1]))], "sizes": [len(t0)], "dev": None}
        self.optimize_stats = {"host_template_generations": []}

        def diversify(parent_ids, generation):
            assert len(parent_ids) == n
            used = sorted(set(parent_ids))
            whole = state["dev"] is not None and all(state["mols"][i].num_atoms == state["sizes"][i] for i in used)
            if whole:
                tmpl_x, tmpl_t = state["dev"]
                tmpl_sizes, slot_tmpl = state["sizes"], list(parent_ids)
            else:
                tmpl_x, tmpl_t, tmpl_sizes = ligand_io.upload_templates(
                    ligand_io.as_templates([state["mols"][i] for i in used], self.lig_type_encoder), self.device)
                new_id = {i: k for k, i in enumerate(used)}
                slot_tmpl = [new_id[i] for i in parent_ids]
                self.optimize_stats["host_template_generations"].append(generation)
            slot_sizes = [tmpl_sizes[t] for t in slot_tmpl]
            ligand, _ = ligand_io.pack_ligands(tmpl_x, tmpl_t, tmpl_sizes, slot_tmpl, slot_sizes, self.atom_nf)
            self.ddpm.seed((int(seed) << 20) + generation)
            xh_lig, lig_mask = self._diversify_chain(pocket, ligand, noising_steps)
            x, atom_type, kept_mask = self._drop_virtual(xh_lig, lig_mask)
            mols = build_molecules(x, atom_type, kept_mask, self.dataset_info, largest_frag=largest_frag, batch=n)
            state.update(mols=mols, sizes=slot_sizes,
                         dev=(xh_lig[:, :self.x_dims].contiguous(), xh_lig[:, self.x_dims:].argmax(1).to(torch.int32)))
            return [m if m.num_atoms > 0 else None for m in mols]

        return diversify

    @torch.no_grad()
    def optimize_ligands(self, pdb_file, ref_ligand, objective, population_size=100, evolution_steps=10, top_k=7,
                         noising_steps=100, largest_frag=False, seed=0, diversify=None):
        """The evolutionary loop of the reference's optimize.py (:198-246) around `diversify`: generation 0 is the
        reference ligand repeated `population_size` times; every later generation takes the `top_k` molecules of the
        previous one by `objective`, each `population_size // top_k` times, and fills the remainder by a SEEDED draw
        among them (the reference draws unseeded).  `objective` is any callable on a `Molecule`, larger = better; QED
        and SA need RDKit and are not provided -- where it is installed pass e.g. `lambda m: qed(m.to_rdkit())`;
        `vina.objective(self, residues)` is a built-in one that needs no RDKit (minus the Vina-type score of the pose).
        Molecules that come back empty do not enter the next generation.  Returns (molecules of the last generation,
        history): history is a list of {'generation', 'index', 'score', 'fate'} records, fate 'initial' (the
        reference), 'survived' (selected as a parent), 'purged', 'rejected' (no molecule) or 'final' (last generation).

        Parents stay on the device between generations when each is its whole batch slot; otherwise
        (`largest_frag=True`, dropped virtual atoms) that generation's parents are taken from their host copies --
        see `_population_step`.  `diversify(parent_ids, generation) -> list of Molecule | None`, one per slot, replaces
        the sampling step (tests, other samplers)."""
        xyz, elements = self.reference_ligand(pdb_file, ref_ligand)
        if diversify is None:
            residues = self.select_pocket_residues(pdb_file, ref_ligand=ref_ligand)
            pocket = self.prepare_pocket(residues, repeats=population_size)
            diversify = self._population_step(pocket, (xyz, elements), noising_steps, largest_frag, seed)
        return evolve_population(Molecule(np.asarray(xyz, np.float32), list(elements)), objective, diversify,
                                 population_size, evolution_steps, top_k, seed)


def evolve_population(initial, objective, diversify, population_size, evolution_steps, top_k, seed=0):
    """Selection loop of optimize.py:198-246 on the host; `diversify(parent_ids, generation)` produces generation
    `generation + 1` from the molecules of the previous one addressed by index (generation 0: index 0 = `initial`).
    -> (molecules of the last generation, history records)."""
    import random
    if not 1 <= top_k <= population_size:
        raise ValueError(f"top_k = {top_k} must lie in [1, population_size = {population_size}]")
    if evolution_steps < 1:
        raise ValueError("evolution_steps must be at least 1")
    rng = random.Random(seed)
    records = [dict(generation=0, index=0, score=objective(initial), fate="initial")]
    history = list(records)
    prev = [initial]
    for generation in range(evolution_steps):
        if generation == 0:
            parent_ids = [0] * population_size
        else:
            alive = [i for i, m in enumerate(prev) if m is not None]
            if not alive:
                raise RuntimeError(f"generation {generation} has no surviving molecule: every sample came back empty "
                                   "or was rejected, nothing to select parents from")
            top = sorted(alive, key=lambda i: -records[i]["score"])[:top_k]        # stable: ties keep slot order
            for i in top:
                records[i]["fate"] = "survived"
            parent_ids = top * (population_size // top_k)
            pool = list(parent_ids) or list(top)
            parent_ids += [rng.choice(pool) for _ in range(population_size - len(parent_ids))]
        prev = list(diversify(parent_ids, generation))
        if len(prev) != population_size:
            raise RuntimeError(f"diversify returned {len(prev)} molecules for a population of {population_size}")
        records = [dict(generation=generation + 1, index=i, score=None if m is None else objective(m),
                        fate="rejected" if m is None else "purged") for i, m in enumerate(prev)]
        history += records
    final = []
    for r, m in zip(records, prev):
        if m is not None:
            r["fate"] = "final"
            final.append(m)
    return final, history


def main(argv=None):
    """`python -m diffsbdd_amd.generate <checkpoint> --pdbfile ... --outfile ...`:
    same options as the reference's generate_ligands.py (:13-27)."""
    from .molecules import write_sdf
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("checkpoint")
    ap.add_argument("--pdbfile", required=True)
    ap.add_argument("--resi_list", nargs="+", default=None)
    ap.add_argument("--ref_ligand", default=None)
    ap.add_argument("--outfile", required=True)
    ap.add_argument("--n_samples", type=int, default=20)
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--num_nodes_lig", type=int, default=None)
    ap.add_argument("--all_frags", action="store_true")
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--relax", action="store_true")
    ap.add_argument("--resamplings", type=int, default=10)
    ap.add_argument("--jump_length", type=int, default=1)
    ap.add_argument("--timesteps", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0, help="noise is keyed by (seed, global sample index)")
    ap.add_argument("--trusted-checkpoint", action="store_true",
                    help="allow a full unpickle of the checkpoint file")
    ap.add_argument("--metrics", action="store_true",
                    help="write metrics.json next to the output (metrics.MoleculeSetMetrics of the written molecules)")
    ap.add_argument("--pose", action="store_true",
                    help="check every sample against the pocket's heavy atoms (pose.py): records to stderr and <outfile>.pose.csv")
    ap.add_argument("--vina", action="store_true",
                    help="Vina-type score of every sample against the pocket's heavy atoms (vina.py; not smina output): "
                         "records to stderr and <outfile>.vina.csv")
    a = ap.parse_args(argv)
    bs = a.batch_size or a.n_samples
    assert a.n_samples % bs == 0
    extra = dict(pose=True) if a.pose else {}
    if a.vina:
        extra["vina"] = True
    gen = LigandGenerator.from_checkpoint(a.checkpoint, device="cuda", trusted=a.trusted_checkpoint)
    molecules = []
    for i in range(a.n_samples // bs):
        gen.ddpm.seed(a.seed, sample_offset=i * bs)
        n_lig = None if a.num_nodes_lig is None else torch.full((bs,), a.num_nodes_lig, dtype=torch.int64)
        molecules += gen.generate_ligands(
            a.pdbfile, bs, a.resi_list, a.ref_ligand, n_lig, a.sanitize, largest_frag=not a.all_frags,
            relax_iter=(200 if a.relax else 0), resamplings=a.resamplings, jump_length=a.jump_length,
            timesteps=a.timesteps, **extra)
    write_sdf(a.outfile, molecules)
    if a.pose:
        from . import pose as pose_mod
        print("[generate] " + pose_mod.POSE_COVERAGE, file=sys.stderr)
        rows = [(os.path.basename(a.outfile), k, m.pose) for k, m in enumerate(molecules)]
        for _, k, rec in rows:
            print(f"[generate] pose mol_{k}: {rec.as_dict()}", file=sys.stderr)
        pose_mod.write_csv(a.outfile + ".pose.csv", rows)
    if a.vina:
        from . import vina as vina_mod
        print("[generate] " + vina_mod.VINA_COVERAGE, file=sys.stderr)
        rows = [(os.path.basename(a.outfile), k, m.vina) for k, m in enumerate(molecules)]
        for _, k, rec in rows:
            print(f"[generate] vina mol_{k}: {rec.as_dict()}", file=sys.stderr)
        vina_mod.write_csv(a.outfile + ".vina.csv", rows)
    from .molecules import PROCESS_MOLECULE_COVERAGE
    print("[generate] " + PROCESS_MOLECULE_COVERAGE, file=sys.stderr)
    print(f"wrote {len(molecules)} molecules to {a.outfile}")
    if a.metrics:
        from . import metrics
        summary = metrics.summarize([[m for m in molecules if m is not None]], gen.dataset_info, [os.path.basename(a.pdbfile)], gen.device)
        metrics.write_summary(os.path.join(os.path.dirname(os.path.abspath(a.outfile)), "metrics.json"), summary,
                              prefix="[generate] ")


if __name__ == "__main__":
    main()
