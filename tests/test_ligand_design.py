"""Ligands as input, host side (no GPU): SDF / PDB readers, element encoding, the size rule of substructure
inpainting, the packer's plan against a line-by-line restatement of the reference's host loop (inpaint.py:114-141),
and the evolutionary loop of optimize.py with an injected diversify step."""
import argparse

import numpy as np
import pytest
import torch

from diffsbdd_amd import ligand_io, synthetic
from diffsbdd_amd import pocket as pocket_io
from diffsbdd_amd.chem_tables import dataset_info
from diffsbdd_amd.generate import LigandGenerator, evolve_population
from diffsbdd_amd.molecules import Molecule, write_sdf

# four residues around a 5-atom HETATM ligand, one far residue
PDB = """\
ATOM      1  N   ALA A   1       0.000   0.000   0.000  1.00  0.00           N
ATOM      2  CA  ALA A   1       1.458   0.000   0.000  1.00  0.00           C
ATOM      3  C   ALA A   1       2.009   1.420   0.000  1.00  0.00           C
ATOM      4  O   ALA A   1       1.251   2.390   0.000  1.00  0.00           O
ATOM      5  N   GLY A   2       3.332   1.536   0.000  1.00  0.00           N
ATOM      6  CA  GLY A   2       3.988   2.839   0.000  1.00  0.00           C
ATOM      7  C   GLY A   2       5.503   2.693   0.000  1.00  0.00           C
ATOM      8  O   GLY A   2       6.042   1.587   0.000  1.00  0.00           O
ATOM      9  N   SER A   3       6.190   3.830   0.000  1.00  0.00           N
ATOM     10  CA  SER A   3       7.646   3.830   0.000  1.00  0.00           C
ATOM     11  OG  SER A   3       8.100   5.100   0.500  1.00  0.00           O
ATOM     12  N   CYS B   7       4.000   6.000   2.000  1.00  0.00           N
ATOM     13  CA  CYS B   7       4.500   7.300   2.300  1.00  0.00           C
ATOM     14  SG  CYS B   7       5.900   7.200   3.500  1.00  0.00           S
ATOM     15  N   LEU A   9      40.000  40.000  40.000  1.00  0.00           N
ATOM     16  CA  LEU A   9      41.458  40.000  40.000  1.00  0.00           C
HETATM   17  C1  LIG A 100       4.000   4.000   3.000  1.00  0.00           C
HETATM   18  O1  LIG A 100       5.200   4.300   3.200  1.00  0.00           O
HETATM   19  N1  LIG A 100       3.300   5.100   3.400  1.00  0.00           N
HETATM   20  C2  LIG A 100       3.400   2.700   3.300  1.00  0.00           C
HETATM   21 CL1  LIG A 100       4.500   1.400   3.900  1.00  0.00          CL
END
"""


def hyper_parameters(arch, mode, pocket_representation="full-atom"):
    """Hyper-parameters in the layout of a Lightning checkpoint of the reference (lightning_modules.py:32-55)."""
    cfg, dd = synthetic.arch_cfg(arch)
    egnn = argparse.Namespace(
        device="cuda", joint_nf=cfg["joint_nf"], hidden_nf=cfg["hidden_nf"], n_layers=cfg["n_layers"],
        attention=cfg["attention"], tanh=cfg["tanh"], norm_constant=cfg["norm_constant"],
        inv_sublayers=cfg["inv_sublayers"], sin_embedding=cfg["sin_embedding"],
        normalization_factor=cfg["normalization_factor"], aggregation_method=cfg["aggregation_method"],
        edge_cutoff_ligand=cfg["edge_cutoff_ligand"], edge_cutoff_pocket=cfg["edge_cutoff_pocket"],
        edge_cutoff_interaction=cfg["edge_cutoff_interaction"],
        reflection_equivariant=cfg["reflection_equivariant"], edge_embedding_dim=cfg["edge_embedding_dim"])
    diff = argparse.Namespace(
        diffusion_steps=dd["timesteps"], diffusion_noise_schedule=dd["noise_schedule"],
        diffusion_noise_precision=dd["noise_precision"], diffusion_loss_type="l2",
        normalize_factors=list(dd["norm_values"]))
    return dict(dataset="crossdock", egnn_params=egnn, diffusion_params=diff, mode=mode,
                node_histogram=np.ones((40, 400)), pocket_representation=pocket_representation, virtual_nodes=False)


def make_generator(arch="small_cond", mode="pocket_conditioning", device="cpu", rep="full-atom"):
    return LigandGenerator(**hyper_parameters(arch, mode, rep), device=device)


# --------------------------------------------------------------------------- readers
def test_sdf_reader_round_trips_to_sdf_block(tmp_path):
    pos = (np.arange(18, dtype=np.float32).reshape(6, 3) - 7.0) / 3
    m = Molecule(pos, ["C", "Cl", "N", "O", "Br", "S"], [(1, 0, 1), (4, 3, 2), (5, 4, 1)])
    p = tmp_path / "one.sdf"
    p.write_text(m.to_sdf_block("x"))
    (xyz, elements), = ligand_io.read_sdf_molecules(p)
    assert elements == m.symbols
    assert xyz.dtype == np.float32 and xyz.shape == (6, 3)
    assert np.allclose(xyz, pos, atol=5e-5)                      # %10.4f
    # what was read writes the same block again
    assert Molecule(xyz, elements, m.bonds).to_sdf_block("x") == Molecule(
        np.round(pos.astype(np.float64), 4).astype(np.float32), m.symbols, m.bonds).to_sdf_block("x")


def test_sdf_reader_reads_every_record_and_keeps_hydrogens(tmp_path):
    a = Molecule(np.zeros((2, 3), np.float32), ["C", "O"], [(1, 0, 2)])
    b = Molecule(np.ones((3, 3), np.float32), ["N", "H", "H"], [(1, 0, 1), (2, 0, 1)])
    p = tmp_path / "two.sdf"
    write_sdf(p, [a, b])
    recs = ligand_io.read_sdf_molecules(str(p))
    assert [r[1] for r in recs] == [["C", "O"], ["N", "H", "H"]]            # no hydrogen stripping
    assert np.array_equal(recs[1][0], np.ones((3, 3), np.float32))
    enc = dataset_info("crossdock")["atom_encoder"]
    assert ligand_io.encode_elements(recs[0][1], enc).tolist() == [enc["C"], enc["O"]]
    assert ligand_io.encode_elements(recs[0][1], enc).dtype == np.int32
    with pytest.raises(ValueError, match=r"atom 1: element 'H'"):
        ligand_io.encode_elements(recs[1][1], enc)
    with pytest.raises(ValueError, match="V2000"):
        q = tmp_path / "bad.sdf"
        q.write_text("a\nb\nc\nnot a counts line\n$$$$\n")
        ligand_io.read_sdf_molecules(q)


def test_pdb_atom_names_come_back_in_file_order(tmp_path):
    pdb = tmp_path / "c.pdb"
    pdb.write_text(PDB)
    residues = pocket_io.read_pdb_residues(pdb, hetero=True)
    xyz, elements = ligand_io.ligand_atoms_from_pdb(residues, "A:100")
    assert elements == ["C", "O", "N", "C", "Cl"] and xyz.shape == (5, 3)
    xyz, elements = ligand_io.ligand_atoms_from_pdb(residues, "A:100", ["CL1", "N1", "C1"])     # shuffled
    assert elements == ["C", "N", "Cl"]
    assert np.allclose(xyz, [[4, 4, 3], [3.3, 5.1, 3.4], [4.5, 1.4, 3.9]])
    with pytest.raises(ValueError, match="C9"):
        ligand_io.ligand_atoms_from_pdb(residues, "A:100", ["C1", "C9"])
    with pytest.raises(ValueError, match="0 groups"):
        ligand_io.ligand_atoms_from_pdb(residues, "B:100")
    gen = make_generator()
    x_fixed, t_fixed = gen.prepare_substructure(str(pdb), "A:100", ["O1", "C2", "C1"])
    enc = gen.lig_type_encoder
    assert t_fixed.tolist() == [enc["C"], enc["O"], enc["C"]]
    assert np.allclose(x_fixed[2], [3.4, 2.7, 3.3])
    sdf = tmp_path / "frag.sdf"
    sdf.write_text(Molecule(np.asarray([[4, 4, 3], [5.2, 4.3, 3.2]], np.float32), ["C", "O"], []).to_sdf_block())
    x2, t2 = gen.prepare_substructure(str(pdb), "A:100", [str(sdf), str(sdf)])             # several files concatenate
    assert t2.tolist() == [enc["C"], enc["O"]] * 2 and x2.shape == (4, 3)


# --------------------------------------------------------------------------- sizes
class _FixedSizes:
    """Stands in for DistributionNodes: returns a prepared draw."""

    def __init__(self, draw):
        self.draw = torch.as_tensor(draw)

    def sample_conditional(self, n1=None, n2=None):
        assert n1 is None and len(n2) == len(self.draw)
        return self.draw.clone()


def test_size_rule_of_inpainting():
    pocket_size = torch.full((5,), 14)
    drawn = ligand_io.inpaint_sizes(_FixedSizes([3, 9, 6, 7, 30]), pocket_size, n_fixed=7)
    assert drawn.tolist() == [7, 9, 7, 7, 30] and drawn.dtype == torch.int64        # a draw below n_fixed is raised to it
    added = ligand_io.inpaint_sizes(_FixedSizes([0] * 5), pocket_size, n_fixed=7, add_n_nodes=4)
    assert added.tolist() == [11] * 5 and added.dtype == torch.int64
    assert ligand_io.inpaint_sizes(_FixedSizes([0] * 5), pocket_size, 7, add_n_nodes=0).tolist() == [7] * 5
    with pytest.raises(ValueError):
        ligand_io.inpaint_sizes(_FixedSizes([0] * 5), pocket_size, 7, add_n_nodes=-1)
    # the real distribution: a histogram that only allows ligands of 2 atoms, clamped up to 4 fixed ones
    from diffsbdd_amd.en_diffusion import DistributionNodes
    hist = np.zeros((6, 20))
    hist[2, :] = 1.0
    sizes = ligand_io.inpaint_sizes(DistributionNodes(hist), torch.tensor([14, 3, 8]), n_fixed=4)
    assert sizes.tolist() == [4, 4, 4]


# --------------------------------------------------------------------------- packer plan
def reference_host_loop(templates, slot_tmpl, num_nodes_lig, atom_nf, device="cpu"):
    """inpaint.py:114-141 restated line by line in torch, with the fixed substructure of sample i being
    templates[slot_tmpl[i]] (the reference has one substructure for all samples).  -> (ligand dict, lig_fixed).
    `device`: where the batch lives, as `model.device` in the reference (tools/bench_ligand_pack.py times it there)."""
    n_samples = len(num_nodes_lig)
    num_nodes_lig = torch.as_tensor(num_nodes_lig, dtype=torch.int64)
    ligand_mask = torch.repeat_interleave(torch.arange(n_samples), num_nodes_lig).to(device)  # num_nodes_to_batch_mask
    ligand = {"x": torch.zeros((len(ligand_mask), 3), dtype=torch.float32, device=device),
              "one_hot": torch.zeros((len(ligand_mask), atom_nf), dtype=torch.float32, device=device),
              "size": num_nodes_lig, "mask": ligand_mask}
    lig_fixed = torch.zeros_like(ligand_mask)
    for i in range(n_samples):
        x_fixed, types = templates[slot_tmpl[i]]
        x_fixed = torch.as_tensor(x_fixed, dtype=torch.float32, device=device).reshape(-1, 3)
        one_hot_fixed = torch.nn.functional.one_hot(torch.as_tensor(types, dtype=torch.int64, device=device),
                                                    num_classes=atom_nf)
        n_fixed = len(x_fixed)
        sele = (ligand_mask == i)

        x_new = ligand["x"][sele]
        x_new[:n_fixed] = x_fixed
        ligand["x"][sele] = x_new

        h_new = ligand["one_hot"][sele]
        h_new[:n_fixed] = one_hot_fixed.float()
        ligand["one_hot"][sele] = h_new

        fixed_new = lig_fixed[sele]
        fixed_new[:n_fixed] = 1
        lig_fixed[sele] = fixed_new
    return ligand, lig_fixed


def random_pack_problem(seed, n_tmpl, batch, atom_nf=10, max_extra=6):
    rng = np.random.RandomState(seed)
    templates = []
    for _ in range(n_tmpl):
        n = int(rng.randint(1, 12))
        templates.append((rng.normal(scale=4.0, size=(n, 3)).astype(np.float32), rng.randint(0, atom_nf, n).astype(np.int32)))
    slot_tmpl = rng.randint(0, n_tmpl, batch).tolist()
    extra = rng.randint(0, max_extra, batch)
    extra[::3] = 0                                              # slots that are exactly their template (n_i == n_fixed)
    sizes = [len(templates[t][1]) + int(e) for t, e in zip(slot_tmpl, extra)]
    return templates, slot_tmpl, sizes


def test_pack_plan_equals_the_reference_host_loop():
    templates, slot_tmpl, sizes = random_pack_problem(seed=5, n_tmpl=4, batch=23)
    assert any(s == len(templates[t][1]) for s, t in zip(sizes, slot_tmpl))
    assert any(s > len(templates[t][1]) for s, t in zip(sizes, slot_tmpl))
    plan = ligand_io.plan_ligand_pack([len(t) for _, t in templates], slot_tmpl, sizes)
    ligand, lig_fixed = reference_host_loop(templates, slot_tmpl, sizes, 10)
    mask = ligand["mask"]
    assert plan.n_rows == len(mask) == sum(sizes) and plan.batch == 23 and plan.n_tmpl == 4
    first_row = [int((mask == b).nonzero()[0]) for b in range(23)]
    assert plan.slot_off.tolist() == first_row + [len(mask)]
    assert plan.slot_size.tolist() == ligand["size"].tolist() and plan.slot_tmpl.tolist() == slot_tmpl
    assert plan.tmpl_ptr.tolist() == np.concatenate([[0], np.cumsum([len(t) for _, t in templates])]).tolist()
    assert plan.tmpl_rows == plan.tmpl_ptr[-1]
    assert plan.buffer.dtype == np.int32 and len(plan.buffer) == 5 + 23 + 23 + 24      # ONE integer buffer
    # what the kernel does with the plan, row by row, is what the reference's loop produced
    all_x = np.concatenate([x for x, _ in templates])
    all_t = np.concatenate([t for _, t in templates])
    for r in range(plan.n_rows):
        b = int(np.searchsorted(plan.slot_off, r, side="right")) - 1
        k = r - plan.slot_off[b]
        t0, t1 = plan.tmpl_ptr[plan.slot_tmpl[b]], plan.tmpl_ptr[plan.slot_tmpl[b] + 1]
        assert int(mask[r]) == b
        if k < t1 - t0:
            assert int(lig_fixed[r]) == 1 and np.array_equal(ligand["x"][r].numpy(), all_x[t0 + k])
            assert int(ligand["one_hot"][r].argmax()) == all_t[t0 + k] and float(ligand["one_hot"][r].sum()) == 1.0
        else:
            assert int(lig_fixed[r]) == 0 and not ligand["x"][r].any() and not ligand["one_hot"][r].any()


def test_pack_plan_and_wrapper_refuse_bad_input():
    with pytest.raises(ValueError, match="slot 1"):
        ligand_io.plan_ligand_pack([3, 5], [0, 1], [3, 4])          # smaller than its template
    with pytest.raises(ValueError, match="template id"):
        ligand_io.plan_ligand_pack([3], [0, 1], [3, 3])
    with pytest.raises(ValueError, match="slot 0"):
        ligand_io.plan_ligand_pack([0], [0], [0])                   # a slot needs a row
    with pytest.raises(ValueError):
        ligand_io.plan_ligand_pack([3], [], [])
    from diffsbdd_amd import _lib
    with pytest.raises(_lib.HipLibraryError, match="device tensors"):
        ligand_io.pack_ligands(torch.zeros(3, 3), torch.zeros(3, dtype=torch.int32), [3], [0], [4], 10)


# --------------------------------------------------------------------------- evolutionary loop
def _mol(tag):
    return Molecule(np.full((1, 3), float(tag), np.float32), ["C"], [])


def test_evolution_selects_replicates_and_fills_seeded():
    calls = []

    def diversify(parent_ids, generation):
        calls.append((generation, list(parent_ids)))
        # child i of generation g carries the tag 100 g + i; slot 4 comes back empty
        return [None if i == 4 else _mol(100 * (generation + 1) + i) for i in range(len(parent_ids))]

    # score: the slot index modulo 7, so the best of 10 slots are 6, 5, (4 is rejected), 3 -- ties (0/7 ...) keep slot order
    objective = lambda m: float(int(m.positions[0, 0]) % 100 % 7)
    final, history = evolve_population(_mol(0), objective, diversify, population_size=10, evolution_steps=3, top_k=3, seed=11)
    assert [g for g, _ in calls] == [0, 1, 2]
    assert calls[0][1] == [0] * 10                                   # generation 0: the reference repeated
    for _, ids in calls[1:]:
        assert ids[:9] == [6, 5, 3] * 3                              # top-k, each population_size // top_k times
        assert len(ids) == 10 and ids[9] in (6, 5, 3)                # the remainder: a draw among them
    again = []
    evolve_population(_mol(0), objective, lambda p, g: (again.append(list(p)), diversify(p, g))[1], 10, 3, 3, seed=11)
    assert again == [ids for _, ids in calls[:3]]                    # the fill is seeded
    fills = set()
    for s in range(12):
        rec = []
        evolve_population(_mol(0), objective, lambda p, g: (rec.append(list(p)), diversify(p, g))[1], 10, 2, 3, seed=s)
        fills.add(rec[1][9])
    assert len(fills) > 1                                            # ... and depends on the seed
    # history: (generation, score, fate) of everything that was scored
    assert history[0] == dict(generation=0, index=0, score=0.0, fate="initial")
    assert [h["generation"] for h in history] == [0] + [1] * 10 + [2] * 10 + [3] * 10
    for g in (1, 2):
        fate = {h["index"]: h["fate"] for h in history if h["generation"] == g}
        assert [i for i, f in fate.items() if f == "survived"] == [3, 5, 6]
        assert fate[4] == "rejected" and all(fate[i] == "purged" for i in (0, 1, 2, 7, 8, 9))
    last = {h["index"]: h for h in history if h["generation"] == 3}
    assert last[4]["fate"] == "rejected" and last[4]["score"] is None
    assert all(last[i]["fate"] == "final" for i in range(10) if i != 4)
    assert len(final) == 9 and [int(m.positions[0, 0]) for m in final] == [300 + i for i in range(10) if i != 4]


def test_evolution_edge_cases():
    objective = lambda m: 1.0
    with pytest.raises(RuntimeError, match="no surviving molecule"):
        evolve_population(_mol(0), objective, lambda p, g: [None] * len(p), 4, 2, 2)
    with pytest.raises(RuntimeError, match="population of 4"):
        evolve_population(_mol(0), objective, lambda p, g: [_mol(1)] * 3, 4, 2, 2)
    with pytest.raises(ValueError, match="top_k"):
        evolve_population(_mol(0), objective, lambda p, g: [_mol(1)] * 4, 4, 2, 5)
    # fewer survivors than top_k: the survivors are replicated and the rest is drawn among them
    seen = []

    def diversify(parent_ids, generation):
        seen.append(list(parent_ids))
        return [_mol(i) if i < 2 else None for i in range(len(parent_ids))]

    final, _ = evolve_population(_mol(0), objective, diversify, population_size=7, evolution_steps=2, top_k=3, seed=0)
    assert seen[1][:4] == [0, 1, 0, 1] and set(seen[1]) == {0, 1} and len(seen[1]) == 7 and len(final) == 2


def test_optimize_ligands_front_end_with_injected_step(tmp_path):
    pdb = tmp_path / "c.pdb"
    pdb.write_text(PDB)
    gen = make_generator()
    got = []

    def diversify(parent_ids, generation):
        got.append(list(parent_ids))
        return [Molecule(np.zeros((2, 3), np.float32), ["C", "O"][: 1 + (i % 2)] * 1, []) for i in range(len(parent_ids))]

    final, history = gen.optimize_ligands(str(pdb), "A:100", objective=lambda m: m.num_atoms, population_size=6,
                                          evolution_steps=2, top_k=2, diversify=diversify, seed=3)
    assert history[0]["score"] == 5 and history[0]["fate"] == "initial"          # the 5-atom ligand of the PDB file
    assert got == [[0] * 6, [1, 3, 1, 3, 1, 3]] and len(final) == 6
    sdf = tmp_path / "ref.sdf"
    sdf.write_text(Molecule(np.zeros((3, 3), np.float32), ["C", "N", "O"], []).to_sdf_block())
    _, history = gen.optimize_ligands(str(pdb), str(sdf), objective=lambda m: m.num_atoms, population_size=4,
                                      evolution_steps=1, top_k=2, diversify=diversify)
    assert history[0]["score"] == 3


# --------------------------------------------------------------------------- refusals of the front ends
def test_front_ends_refuse_what_they_cannot_do(tmp_path):
    pdb = tmp_path / "c.pdb"
    pdb.write_text(PDB)
    gen = make_generator()
    with pytest.raises(NotImplementedError) as e1:
        gen.generate_ligands(str(pdb), 2, ref_ligand="A:100", sanitize=True)
    for kw in (dict(sanitize=True), dict(relax_iter=200)):
        with pytest.raises(NotImplementedError) as e2:
            gen.inpaint_ligands(str(pdb), 2, "A:100", ["C1"], **kw)
        assert str(e2.value) == str(e1.value)                        # the same message as generate_ligands
    with pytest.raises(NotImplementedError, match="n_samples=1"):
        gen.inpaint_ligands(str(pdb), 2, "A:100", ["C1"], save_traj=True)
    with pytest.raises(ValueError, match="center"):
        gen.inpaint_ligands(str(pdb), 2, "A:100", ["C1"], center="origin")
    simple = make_generator(mode="pocket_conditioning_simple")
    with pytest.raises(NotImplementedError, match="SimpleConditionalDDPM"):
        simple.inpaint_ligands(str(pdb), 2, "A:100", ["C1"])
    joint = make_generator("small_joint", "joint")
    with pytest.raises(ValueError, match="joint model"):
        joint.inpaint_ligands(str(pdb), 2, "A:100", ["C1"], center="pocket")
    with pytest.raises(NotImplementedError, match="diversify"):
        joint.diversify_ligands({"size": torch.zeros(1)}, [(np.zeros((1, 3)), ["C"])], 3)
    # an element outside the vocabulary is named, with its atom
    with pytest.raises(ValueError, match=r"atom 1: element 'H'"):
        gen.diversify_ligands({"size": torch.zeros(1)}, [(np.zeros((2, 3)), ["C", "H"])], 3)
