"""`python -m diffsbdd_amd.inpaint <checkpoint> --pdbfile ... --ref_ligand ... --fix_atoms ... --outfile ...`:
substructure inpainting from the command line, with the options and defaults of the reference's inpaint.py
(:192-208) on `LigandGenerator.inpaint_ligands`."""
from __future__ import annotations

import argparse
import sys


def main(argv=None):
    from .generate import LigandGenerator
    from .molecules import PROCESS_MOLECULE_COVERAGE, write_sdf
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("checkpoint")
    ap.add_argument("--pdbfile", required=True)
    ap.add_argument("--ref_ligand", required=True,
                    help="<chain>:<resi> of the ligand inside the PDB file, or an SDF file; defines the pocket")
    ap.add_argument("--fix_atoms", nargs="+", required=True,
                    help="atom names of the PDB ligand to keep (e.g. C1 N6 C5), or SDF file(s) with the substructure")
    ap.add_argument("--center", default="ligand", choices=["ligand", "pocket"])
    ap.add_argument("--outfile", required=True)
    ap.add_argument("--n_samples", type=int, default=20)
    ap.add_argument("--add_n_nodes", type=int, default=None)
    ap.add_argument("--relax", action="store_true")
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--resamplings", type=int, default=20)
    ap.add_argument("--timesteps", type=int, default=50)
    ap.add_argument("--save_traj", action="store_true")
    ap.add_argument("--seed", type=int, default=0, help="noise is keyed by (seed, global sample index)")
    ap.add_argument("--trusted-checkpoint", action="store_true",
                    help="allow a full unpickle of the checkpoint file")
    a = ap.parse_args(argv)
    gen = LigandGenerator.from_checkpoint(a.checkpoint, device="cuda", trusted=a.trusted_checkpoint)
    molecules = gen.inpaint_ligands(
        a.pdbfile, a.n_samples, a.ref_ligand, a.fix_atoms, a.add_n_nodes, center=a.center, sanitize=a.sanitize,
        largest_frag=False, relax_iter=(200 if a.relax else 0), timesteps=a.timesteps, resamplings=a.resamplings,
        save_traj=a.save_traj, seed=a.seed)
    molecules = [m for m in molecules if m.num_atoms > 0]
    write_sdf(a.outfile, molecules)
    print("[inpaint] " + PROCESS_MOLECULE_COVERAGE, file=sys.stderr)
    print(f"wrote {len(molecules)} molecules to {a.outfile}")


if __name__ == "__main__":
    main()
