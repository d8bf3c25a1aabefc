"""Ligands as input on the GPU: the batch packer (`dsbdd_pack_ligands`) bitwise against the restatement of the
reference's host loop, and the front ends built on it -- `inpaint_ligands`, `inpaint_for_pockets`,
`diversify_ligands`, `optimize_ligands`, `python -m diffsbdd_amd.inpaint` -- against the oracle's chains
(`oracle.ddpm_oracle.cond_inpaint / joint_inpaint / cond_diversify`) on the same packed inputs and the same noise,
compared after the move back into the pocket's frame.  Small architectures, T <= 20."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from diffsbdd_amd import ligand_io, synthetic
from diffsbdd_amd.molecules import Molecule
from oracle import ddpm_oracle as do
from oracle import egnn_oracle as eo
from tests.test_ligand_design import PDB, hyper_parameters, make_generator, random_pack_problem, reference_host_loop

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# the project's tolerance for free-running chains of this length against the oracle (tests/test_gpu_parity.py)
X_TOL = 1e-3

_REP = {"small_cond": "full-atom", "small_variant": "CA", "small_joint": "full-atom"}
_MODE = {"small_cond": "pocket_conditioning", "small_variant": "pocket_conditioning", "small_joint": "joint"}


def generator(arch, seed=0):
    gen = make_generator(arch, _MODE[arch], device=DEV, rep=_REP[arch])
    cfg, dd = synthetic.arch_cfg(arch)
    sd = synthetic.random_state_dict(cfg, seed=seed)
    gen.ddpm.dynamics.load_state_dict(sd)
    om = do.OracleModel(sd, cfg, cfg["atom_nf"], cfg["residue_nf"], dd["timesteps"], dd["noise_schedule"],
                        dd["noise_precision"], norm_values=dd["norm_values"], conditional=dd["conditional"])
    return gen, om


def cpu(d):
    return {k: v.detach().cpu() for k, v in d.items()}


def example_residues(name, rep, keep=None):
    """The example pocket of diffsbdd_amd/data as a residue list (one pseudo-residue per node: featurize_pocket reads
    the CA atom / every atom of a residue, so both representations come out as stored).  -> (residues, ligand xyz)"""
    from diffsbdd_amd.pocket import AA3_TO_1, AA_ENCODER, ATOM_ENCODER
    z = np.load(os.path.join(ROOT, "diffsbdd_amd", "data", f"pocket_{name}.npz"))
    key = "ca" if rep == "CA" else "fa"
    one_to_three = {v: k for k, v in AA3_TO_1.items()}
    aa_dec = {v: k for k, v in AA_ENCODER.items()}
    at_dec = {v: k for k, v in ATOM_ENCODER.items()}
    out = []
    for i, (x, t) in enumerate(zip(z[key + "_x"][:keep], z[key + "_types"][:keep])):
        resname = one_to_three[aa_dec[int(t)]] if rep == "CA" else "ALA"
        elem = "C" if rep == "CA" else at_dec[int(t)]
        out.append(dict(chain="A", resseq=i + 1, icode=" ", resname=resname, hetero=False,
                        atoms=[("CA", elem, tuple(float(v) for v in x))]))
    return out, z["ligand_x"].astype(np.float32)


def assert_molecules_equal_chain(mols, out_lig, out_pocket, lig_mask, pocket_mask, pocket_x0, n, decoder, what):
    """Molecules of a front end against the oracle's chain output moved into the pocket's frame
    (inpaint.py:164-170 / optimize.py:121-128): coordinates < 1e-3, atom types identical."""
    com0 = eo.segment_mean(pocket_x0.float(), pocket_mask, n)
    shift = com0 - eo.segment_mean(out_pocket[:, :3], pocket_mask, n)
    x_ref = (out_lig[:, :3] + shift[lig_mask]).numpy()
    t_ref = out_lig[:, 3:].argmax(1).numpy()
    worst, lo = 0.0, 0
    assert len(mols) == n
    for b, m in enumerate(mols):
        hi = lo + int((lig_mask == b).sum())
        assert m.num_atoms == hi - lo, (what, b)
        assert m.symbols == [decoder[int(t)] for t in t_ref[lo:hi]], (what, b)
        worst = max(worst, float(np.abs(m.positions - x_ref[lo:hi]).max()))
        lo = hi
    print(f"[{what}] {n} molecules, max |x - oracle| = {worst:.2e} (max |x| = {np.abs(x_ref).max():.1f})")
    assert worst < X_TOL, (what, worst)


# --------------------------------------------------------------------------- the packer
def _assert_pack_bitwise(got, want):
    (ligand, fixed), (ref, ref_fixed) = got, want
    for k in ("x", "one_hot", "size", "mask"):
        assert ligand[k].dtype == ref[k].dtype and ligand[k].shape == ref[k].shape, k
        assert torch.equal(ligand[k].cpu(), ref[k]), k
    assert fixed.dtype == ref_fixed.dtype and torch.equal(fixed.cpu(), ref_fixed)


def test_packer_is_bitwise_the_reference_host_loop_512_slots():
    templates, slot_tmpl, sizes = random_pack_problem(seed=1, n_tmpl=9, batch=512, max_extra=30)
    tmpl_x, tmpl_t, tmpl_sizes = ligand_io.upload_templates(templates, DEV)
    got = ligand_io.pack_ligands(tmpl_x, tmpl_t, tmpl_sizes, slot_tmpl, sizes, 10)
    torch.cuda.synchronize()
    _assert_pack_bitwise(got, reference_host_loop(templates, slot_tmpl, sizes, 10))
    assert got[0]["x"].shape[0] == sum(sizes) and got[0]["size"].tolist() == sizes
    # a single slot, and an atom_nf that is not 10
    got = ligand_io.pack_ligands(tmpl_x, tmpl_t, tmpl_sizes, [3], [tmpl_sizes[3] + 2], 11)
    _assert_pack_bitwise(got, reference_host_loop(templates, [3], [tmpl_sizes[3] + 2], 11))


def test_packer_takes_its_templates_from_a_previous_output_on_the_device():
    """The evolutionary loop: generation g's output (coordinates and one-hot classes as they lie on the device, its
    slot sizes known to the host) is the template set of generation g + 1; a slot's template id is its parent's slot."""
    templates, slot_tmpl, sizes = random_pack_problem(seed=2, n_tmpl=5, batch=64, max_extra=1)      # every slot == template
    sizes = [len(templates[t][1]) for t in slot_tmpl]
    tmpl_x, tmpl_t, tmpl_sizes = ligand_io.upload_templates(templates, DEV)
    first, _ = ligand_io.pack_ligands(tmpl_x, tmpl_t, tmpl_sizes, slot_tmpl, sizes, 10)
    prev_x = first["x"] + 0.25                                     # stands for the chain's output: same rows, moved
    prev_t = first["one_hot"].argmax(1).to(torch.int32)
    rng = np.random.RandomState(3)
    parents = rng.randint(0, 64, 512).tolist()
    got = ligand_io.pack_ligands(prev_x, prev_t, sizes, parents, [sizes[p] for p in parents], 10)
    torch.cuda.synchronize()
    px, pt = prev_x.cpu().numpy(), prev_t.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(sizes)])
    host_templates = [(px[off[b]:off[b + 1]], pt[off[b]:off[b + 1]]) for b in range(64)]
    _assert_pack_bitwise(got, reference_host_loop(host_templates, parents, [sizes[p] for p in parents], 10))
    assert int(got[1].sum()) == got[1].numel()                     # a whole-slot parent fixes every row


# --------------------------------------------------------------------------- inpaint_ligands vs the oracle
@pytest.mark.parametrize("arch,center,resamplings,fix", [
    ("small_cond", "ligand", 1, "names"),
    ("small_cond", "pocket", 3, "sdf"),
    ("small_variant", "ligand", 2, "names"),
    ("small_variant", "pocket", 1, "names"),
])
def test_inpaint_ligands_vs_oracle_chain(tmp_path, arch, center, resamplings, fix):
    pdb = tmp_path / "c.pdb"
    pdb.write_text(PDB)
    gen, om = generator(arch)
    n, T, add = 3, 10, 4
    if fix == "names":
        fix_atoms = ["N1", "C1", "CL1"]                             # file order: C1, N1, CL1
        x_fixed = np.asarray([[4, 4, 3], [3.3, 5.1, 3.4], [4.5, 1.4, 3.9]], np.float32)
        elements = ["C", "N", "Cl"]
    else:
        x_fixed = np.asarray([[4.1, 3.9, 3.0], [5.2, 4.3, 3.2]], np.float32)
        elements = ["C", "O"]
        sdf = tmp_path / "frag.sdf"
        sdf.write_text(Molecule(x_fixed, elements, []).to_sdf_block())
        fix_atoms = [str(sdf)]
        x_fixed = ligand_io.read_sdf_molecules(sdf)[0][0]
    t_fixed = ligand_io.encode_elements(elements, gen.lig_type_encoder)
    sizes = [len(elements) + add] * n
    ligand, lig_fixed = reference_host_loop([(x_fixed, t_fixed)], [0] * n, sizes, gen.atom_nf)
    pocket = cpu(gen.prepare_pocket(gen.select_pocket_residues(str(pdb), ref_ligand="A:100"), repeats=n))
    pocket["one_hot"] = pocket["one_hot"].float()
    tape = do.NoiseTape(21)
    o_l, o_p, lm, pm = do.cond_inpaint(om, ligand, pocket, lig_fixed.float(), tape, resamplings=resamplings, timesteps=T,
                                       center=center)
    gen.ddpm.set_noise_source(do.NoiseReplay(tape.draws))
    try:
        mols = gen.inpaint_ligands(str(pdb), n, "A:100", fix_atoms, add_n_nodes=add, center=center, timesteps=T,
                                   resamplings=resamplings)
    finally:
        gen.ddpm.set_noise_source(None)
    assert_molecules_equal_chain(mols, o_l, o_p, lm, pm, pocket["x"], n, gen.lig_type_decoder,
                                 f"inpaint {arch} center={center} r={resamplings}")
    # the fixed atoms are where they were put, in the pocket's frame (the chain keeps them up to its last noise level)
    for m in mols:
        assert m.symbols[:len(elements)] == elements


def test_inpaint_ligands_joint_model_vs_oracle_chain(tmp_path):
    """The joint model through the same front end: `ddpm.inpaint` with every pocket node fixed, against
    `joint_inpaint` with pocket_fixed = 1.  The untrained joint network drives |x| to ~2 700 Angstrom, where one fp32
    ulp is 2.4e-4: measured 8.5e-4 against the 1e-3 bound (the conditional cases: 2e-5 ... 4e-4 at |x| 120 ... 1 400)."""
    pdb = tmp_path / "c.pdb"
    pdb.write_text(PDB)
    gen, om = generator("small_joint")
    n, T, add = 2, 8, 3
    x_fixed = np.asarray([[4, 4, 3], [5.2, 4.3, 3.2]], np.float32)
    t_fixed = ligand_io.encode_elements(["C", "O"], gen.lig_type_encoder)
    ligand, lig_fixed = reference_host_loop([(x_fixed, t_fixed)], [0] * n, [2 + add] * n, gen.atom_nf)
    pocket = cpu(gen.prepare_pocket(gen.select_pocket_residues(str(pdb), ref_ligand="A:100"), repeats=n))
    pocket["one_hot"] = pocket["one_hot"].float()
    tape = do.NoiseTape(4)
    o_l, o_p, lm, pm = do.joint_inpaint(om, ligand, pocket, lig_fixed.float(), torch.ones(len(pocket["mask"])), tape,
                                        resamplings=2, jump_length=1, timesteps=T)
    gen.ddpm.set_noise_source(do.NoiseReplay(tape.draws))
    try:
        mols = gen.inpaint_ligands(str(pdb), n, "A:100", ["C1", "O1"], add_n_nodes=add, timesteps=T, resamplings=2)
    finally:
        gen.ddpm.set_noise_source(None)
    assert_molecules_equal_chain(mols, o_l, o_p, lm, pm, pocket["x"], n, gen.lig_type_decoder, "inpaint small_joint")


# --------------------------------------------------------------------------- diversify_ligands vs the oracle
@pytest.mark.parametrize("arch", ["small_cond", "small_variant"])
def test_diversify_ligands_vs_oracle_chain(arch):
    gen, om = generator(arch, seed=2)
    residues, lig_x = example_residues("3rfm", _REP[arch], keep=60)
    rng = np.random.RandomState(0)
    symbols = gen.lig_type_decoder
    inputs = []
    for n_atoms in (6, 14, 9):                                        # unequal ligands in one batch
        idx = rng.permutation(len(lig_x))[:n_atoms]
        inputs.append((lig_x[idx], [symbols[int(t)] for t in rng.randint(0, 10, n_atoms)]))
    inputs[1] = Molecule(*inputs[1])                                  # Molecule objects and pairs mix
    n = len(inputs)
    pocket = gen.prepare_pocket(residues, repeats=n)
    templates = ligand_io.as_templates(inputs, gen.lig_type_encoder)
    ligand, _ = reference_host_loop(templates, list(range(n)), [len(t) for _, t in templates], gen.atom_nf)
    pocket_c = cpu(pocket)
    pocket_c["one_hot"] = pocket_c["one_hot"].float()
    tape = do.NoiseTape(9)
    o_l, o_p, lm, pm = do.cond_diversify(om, ligand, pocket_c, 7, tape)
    gen.ddpm.set_noise_source(do.NoiseReplay(tape.draws))
    try:
        mols = gen.diversify_ligands(pocket, inputs, noising_steps=7)
    finally:
        gen.ddpm.set_noise_source(None)
    assert_molecules_equal_chain(mols, o_l, o_p, lm, pm, pocket_c["x"], n, gen.lig_type_decoder, f"diversify {arch}")


# --------------------------------------------------------------------------- keyed noise, trajectories
def _same(a, b):
    return a.symbols == b.symbols and np.array_equal(a.positions, b.positions) and a.bonds == b.bonds


def test_inpaint_for_pockets_is_packing_invariant_and_reproducible():
    """Keyed noise: a design job gives bitwise the same molecules alone and packed after another job (very unequal
    ligand sizes in one batch: 5 ... 33 atoms), and twice with the same seed."""
    gen, _ = generator("small_cond")
    res_a, lig_a = example_residues("3rfm", "full-atom")            # 286 and 287 atoms: the engine's pocket-frame path,
    res_b, lig_b = example_residues("5ndu", "full-atom")            # where cone on / off (pinned by the call) differ in rounding
    job_a = (res_a, 3, (lig_a[:4], ["C", "N", "C", "O"]), [5, 33, 9])
    job_b = (res_b, 2, Molecule(lig_b[:6], ["C", "C", "O", "N", "S", "C"]), 2)
    ids_a, ids_b = [10, 11, 12], [40, 41]
    alone = gen.inpaint_for_pockets([job_a], timesteps=8, resamplings=2, seed=5, sample_ids=ids_a)[0]
    packed = gen.inpaint_for_pockets([job_b, job_a], timesteps=8, resamplings=2, seed=5, sample_ids=ids_b + ids_a)
    assert [len(p) for p in packed] == [2, 3]
    assert [m.num_atoms for m in packed[0]] == [8, 8] and [m.num_atoms for m in packed[1]] == [5, 33, 9]
    for got, want in zip(packed[1], alone):
        assert _same(got, want)
    again = gen.inpaint_for_pockets([job_b, job_a], timesteps=8, resamplings=2, seed=5, sample_ids=ids_b + ids_a)
    assert all(_same(g, w) for g, w in zip(again[0] + again[1], packed[0] + packed[1]))
    other = gen.inpaint_for_pockets([job_a], timesteps=8, resamplings=2, seed=6, sample_ids=ids_a)[0]
    assert not any(_same(g, w) for g, w in zip(other, alone))


def test_save_traj_returns_the_frames_and_ends_in_the_plain_result(tmp_path):
    pdb = tmp_path / "c.pdb"
    pdb.write_text(PDB)
    gen, _ = generator("small_cond")
    kw = dict(add_n_nodes=3, timesteps=10, resamplings=2, seed=13)
    plain = gen.inpaint_ligands(str(pdb), 1, "A:100", ["C1", "O1"], **kw)
    frames = gen.inpaint_ligands(str(pdb), 1, "A:100", ["C1", "O1"], save_traj=True, largest_frag=True, **kw)
    assert len(plain) == 1 and len(frames) == 10
    assert all(f.num_atoms == 5 for f in frames)                    # largest_frag is forced off for a trajectory
    assert frames[-1].symbols == plain[0].symbols and np.array_equal(frames[-1].positions, plain[0].positions)
    assert not np.array_equal(frames[0].positions, frames[-1].positions)
    twice = gen.inpaint_ligands(str(pdb), 1, "A:100", ["C1", "O1"], **kw)
    assert _same(twice[0], plain[0])


# --------------------------------------------------------------------------- the evolutionary loop on the real chain
def test_optimize_ligands_two_generations(tmp_path):
    pdb = tmp_path / "c.pdb"
    pdb.write_text(PDB)
    gen, _ = generator("small_cond", seed=1)
    objective = lambda m: -float(len(m.valence_violations()))
    runs = []
    for _ in range(2):
        final, history = gen.optimize_ligands(str(pdb), "A:100", objective, population_size=8, evolution_steps=2,
                                              top_k=3, noising_steps=6, seed=4)
        runs.append((final, history))
        assert len(final) == 8 and all(m.num_atoms == 5 for m in final)            # the population size is kept
        assert [h["generation"] for h in history] == [0] + [1] * 8 + [2] * 8
        assert sum(h["fate"] == "survived" for h in history) == 3
        # only generation 0 (the reference ligand) uploads coordinates: the parents of generation 1 are gathered on the device
        assert gen.optimize_stats["host_template_generations"] == [0]
    assert all(_same(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert [h["score"] for h in runs[0][1]] == [h["score"] for h in runs[1][1]]
    # with largest_frag a parent may be smaller than its slot: that generation takes its parents from the host copies,
    # and where every parent is whole the two routes give the same templates bit for bit
    final_frag, _ = gen.optimize_ligands(str(pdb), "A:100", objective, population_size=8, evolution_steps=2, top_k=3,
                                         noising_steps=6, largest_frag=True, seed=4)
    assert 1 <= len(final_frag) <= 8 and all(1 <= m.num_atoms <= 5 for m in final_frag)


# --------------------------------------------------------------------------- command line
def test_inpaint_command_line_writes_one_record_per_molecule(tmp_path):
    from diffsbdd_amd.en_diffusion import PredefinedNoiseSchedule
    pdb = tmp_path / "c.pdb"
    pdb.write_text(PDB)
    hp = hyper_parameters("small_cond", "pocket_conditioning", "full-atom")
    cfg, _ = synthetic.arch_cfg("small_cond")
    sd = {"ddpm.dynamics." + k: v for k, v in synthetic.random_state_dict(cfg, seed=3).items()}
    sd["ddpm.buffer"] = torch.zeros(1)
    dp = hp["diffusion_params"]
    sd["ddpm.gamma.gamma"] = PredefinedNoiseSchedule(dp.diffusion_noise_schedule, dp.diffusion_steps,
                                                     dp.diffusion_noise_precision).gamma.detach().clone()
    ckpt = tmp_path / "last.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": hp, "epoch": 1, "global_step": 1}, ckpt)
    out = tmp_path / "designed.sdf"
    t0 = time.time()
    res = subprocess.run([sys.executable, "-m", "diffsbdd_amd.inpaint", str(ckpt), "--pdbfile", str(pdb),
                          "--ref_ligand", "A:100", "--fix_atoms", "C1", "N1", "--outfile", str(out), "--n_samples", "3",
                          "--add_n_nodes", "4", "--resamplings", "2", "--timesteps", "10", "--seed", "2"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(f"[cli] {time.time() - t0:.1f} s\n{res.stdout}{res.stderr[-2000:]}")
    assert res.returncode == 0, res.stderr[-4000:]
    assert "wrote 3 molecules" in res.stdout
    records = ligand_io.read_sdf_molecules(out)
    assert len(records) == 3 and all(len(e) == 6 for _, e in records)
    assert all(e[:2] == ["C", "N"] for _, e in records)
