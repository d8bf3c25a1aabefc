"""GPU: the callers on top of the Vina-type score kernels (diffsbdd_amd/vina.py) -- the `vina=` hook of the samplers, its
packing invariance, `LigandGenerator.vina_scores`, the built-in objective inside `optimize_ligands`, and the command line.
Small architecture, a handful of steps."""
import numpy as np
import pytest
import torch

from diffsbdd_amd import vina as V
from diffsbdd_amd.molecules import Molecule, write_sdf
from tests import _pose_cases as P
from tests import _vina_cases as C
from tests.test_gpu_ligand_design import generator
from tests.test_gpu_pose import _pinned, _same_molecule
from tests.test_ligand_design import PDB

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _jobs():
    res_a, res_b = P.ball_residues(1, 6000), P.ball_residues(2, 5700)
    return (res_a, 3, torch.tensor([19, 24, 5])), (res_b, 2, torch.tensor([21, 17]))


def _same_record(a, b):
    bits = lambda v: np.ascontiguousarray(v).view(np.int32)
    return (np.array_equal(bits(a.mol), bits(b.mol)) and np.array_equal(bits(a.atom), bits(b.atom)) and
            np.array_equal(a.ints, b.ints) and np.array_equal(a.code, b.code) and a.nonfinite == b.nonfinite)


def _fixture_pdb(path, z, name):
    """The stored pocket atoms of the fixture as ATOM records, one residue number per atom."""
    lines = []
    for k, (res, atom, x) in enumerate(zip(z[f"{name}_poc_res"], z[f"{name}_poc_atom"], z[f"{name}_poc_x"])):
        atom = str(atom)
        lines.append(f"ATOM  {k + 1:5d} {(' ' + atom) if len(atom) < 4 else atom:<4s} {str(res):>3s} A{k + 1:4d}    "
                     f"{x[0]:8.3f}{x[1]:8.3f}{x[2]:8.3f}  1.00  0.00          {atom[0]:>2s}")
    path.write_text("\n".join(lines) + "\nEND\n")


def test_generate_for_pockets_hook():
    gen, _ = generator("small_cond")
    job_a, job_b = _jobs()
    kw = dict(timesteps=4, seed=7, sample_ids=torch.arange(5))
    scored = gen.generate_for_pockets([job_a, job_b], vina=True, **kw)
    plain = gen.generate_for_pockets([job_a, job_b], vina=None, **kw)
    assert [len(p) for p in scored] == [3, 2]
    terms = np.stack([m.vina.terms for mols in scored for m in mols])
    print("terms of the five samples:\n", terms)
    assert (terms[:, :3].max(0) > 0).all()                                       # the records are not all empty
    for job, mols, bare in zip((job_a, job_b), scored, plain):
        pockets = V.VinaPocket.upload([V.type_pocket(job[0])], DEV)
        for m, p in zip(mols, bare):
            rec, = V.score_molecules([m], pockets, gen.dataset_info)            # the same sample, scored on its own
            assert _same_record(m.vina, rec) and m.vina.n_atoms == m.num_atoms
            assert _same_molecule(m, p) and not hasattr(p, "vina")                # the option changes nothing else
            # and the record is what the restatement says of these atoms and codes
            want, _, atom_bound, mol_bound = V._vina_score_host(m.positions, rec.code, [0, m.num_atoms], [0], [rec.ints],
                                                                pockets.x, pockets.code, [0, len(pockets.code)], eps=V.EPS32)
            assert np.all(np.abs(rec.atom - want.atom) <= atom_bound) and np.all(np.abs(rec.mol[:7] - want.mol[0, :7]) <= mol_bound[0])
    both = gen.generate_for_pockets([job_a, job_b], vina=True, pose=True, **kw)          # beside the pose records
    assert all(_same_record(m.vina, w.vina) and m.pose.n_atoms == m.num_atoms for a, b in zip(both, scored) for m, w in zip(a, b))
    # largest_frag: the record follows the kept atoms, rotors counted on the fragment
    frags = gen.generate_for_pockets([job_a, job_b], vina=True, largest_frag=True, **kw)
    assert any(hasattr(m, "n_generated_atoms") for mols in frags for m in mols)
    for mols in frags:
        for m in mols:
            low = V.orders_from_bonds(m.num_atoms, m.bonds).astype(np.int64)
            assert m.vina.n_atoms == m.num_atoms and m.vina.n_rot == V.type_graph(m.vina.code & 15, low + low.T)[1]
            assert m.vina.terms == pytest.approx(m.vina.atom.astype(np.float64).sum(0), rel=1e-5)
    assert len(gen._vina_pockets) == 2                                           # typed and uploaded once per job
    with pytest.raises(ValueError, match="unknown option"):
        gen.generate_for_pockets([job_a], vina=dict(tol=1.0), **kw)


def test_vina_records_do_not_depend_on_the_packing():
    gen, _ = generator("small_cond")
    job_a, job_b = _jobs()
    ids_a, ids_b = torch.tensor([100, 101, 102]), torch.tensor([7, 8])
    kw = dict(timesteps=4, seed=3, vina=True, cone_mode=2)
    sampler = lambda jobs, ids: _pinned(gen, jobs, ids, kw)
    both = sampler([job_a, job_b], torch.cat([ids_a, ids_b]))
    swapped = sampler([job_b, job_a], torch.cat([ids_b, ids_a]))
    alone_a = sampler([job_a], ids_a)
    for got in (swapped[1], alone_a[0]):
        for m, w in zip(got, both[0]):
            assert _same_molecule(m, w) and _same_record(m.vina, w.vina)
    for m, w in zip(swapped[0], both[1]):
        assert _same_record(m.vina, w.vina)
    assert sum(m.vina.terms[1] for mols in both for m in mols) > 0


def test_vina_scores_of_the_crystal_ligand_in_the_3rfm_pocket(tmp_path):
    gen, _ = generator("small_cond")
    z = C.fixture()
    pdb = tmp_path / "3rfm_pocket.pdb"
    _fixture_pdb(pdb, z, "3rfm")
    el, _ = C.fixture_ligand(z, "3rfm")
    ligands = [(z["3rfm_crystal_x"], el), (z["3rfm_shifted_x"], el)]
    out = gen.vina_scores(str(pdb), ligands)
    pockets = V.VinaPocket.upload([V.type_pocket(C.fixture_residues(z, "3rfm"))], DEV)
    assert np.array_equal(pockets.code.cpu().numpy(), z["3rfm_poc_code"]) and pockets.untemplated == [0]
    recs = V.score_molecules(ligands, pockets, gen.dataset_info)
    assert out == [r.as_dict() for r in recs] and [o["n_atoms"] for o in out] == [14, 14]
    print(out)
    assert out[0]["score"] < 0 and out[1]["repulsion"] > out[0]["repulsion"] and out[0]["nonfinite"] == 0
    # bonds perceived from distances give caffeine's codes of the file's bond list here, hence the stored score
    if np.array_equal(recs[0].code, z["3rfm_lig_code"]):
        assert out[0]["score"] == pytest.approx(float(z["3rfm_crystal_score"]), abs=1e-4)
    with pytest.raises(ValueError, match="scope"):
        gen.vina_scores(str(pdb), ligands, scope="chain")


def test_objective_inside_optimize_ligands(tmp_path):
    pdb = tmp_path / "c.pdb"
    pdb.write_text(PDB)
    gen, _ = generator("small_cond", seed=1)
    residues = gen.select_pocket_residues(str(pdb), ref_ligand="A:100")
    objective = V.objective(gen, residues)
    xyz, elements = gen.reference_ligand(str(pdb), "A:100")
    heavy = [k for k, e in enumerate(elements) if e not in ("H", "D")]
    base = Molecule(np.asarray(xyz, np.float32)[heavy], [elements[k] for k in heavy])
    calls = []

    def diversify(parent_ids, generation):                                       # the sampling step replaced: shifted copies
        calls.append(list(parent_ids))
        return [Molecule(base.positions + np.float32(0.4 * (k + 1) * (generation + 1)), list(base.symbols)) for k in range(4)]

    final, history = gen.optimize_ligands(str(pdb), "A:100", objective, population_size=4, evolution_steps=2, top_k=2,
                                          diversify=diversify)
    assert len(final) == 4 and [h["generation"] for h in history] == [0, 1, 1, 1, 1, 2, 2, 2, 2]
    pockets = V.VinaPocket.upload([V.type_pocket(residues)], DEV)
    first = [Molecule(base.positions + np.float32(0.4 * (k + 1)), list(base.symbols)) for k in range(4)]
    want = [-r.score for r in V.score_molecules(first, pockets, gen.dataset_info)]
    assert [h["score"] for h in history[1:5]] == want and len(set(want)) > 1       # larger = better = minus the score
    top = sorted(range(4), key=lambda i: -want[i])[:2]
    assert [h["index"] for h in history[1:5] if h["fate"] == "survived"] == sorted(top) and calls[1][:2] == top
    scored = Molecule(base.positions, list(base.symbols))
    scored.vina = V.score_molecules([scored], pockets, gen.dataset_info)[0]
    assert objective(scored) == -scored.vina.score == history[0]["score"]


def test_command_line_writes_one_row_per_molecule(tmp_path, capsys):
    z = C.fixture()
    pdb, sdf, out = tmp_path / "p.pdb", tmp_path / "l.sdf", tmp_path / "scores.csv"
    _fixture_pdb(pdb, z, "5ndu")
    el, bonds = C.fixture_ligand(z, "5ndu")
    bonds = [(max(i, j), min(i, j), o) for i, j, o in bonds]
    write_sdf(str(sdf), [Molecule(z["5ndu_crystal_x"], el, bonds), Molecule(z["5ndu_shifted_x"], el, bonds),
                         Molecule(z["5ndu_crystal_x"][:3], el[:3], [])])
    rows = V.main(["--pdbfile", str(pdb), "--sdf", str(sdf), "--bonds", "file", "--out", str(out), "--device", DEV])
    err = capsys.readouterr().err
    assert V.VINA_COVERAGE in err and "287 protein heavy atoms, 0 typed by element alone" in err
    lines = out.read_text().splitlines()
    assert len(lines) == 4 and len(rows) == 3 and lines[0].split(",")[:3] == ["source", "index", "n_atoms"]
    cells = [dict(zip(lines[0].split(","), l.split(","))) for l in lines[1:]]
    assert [c["n_atoms"] for c in cells] == ["49", "49", "3"] and [c["n_rot"] for c in cells] == ["10", "10", "0"]
    # written coordinates have four decimals: the stored score to that precision
    assert float(cells[0]["score"]) == pytest.approx(float(z["5ndu_crystal_score"]), abs=2e-2) and float(cells[0]["score"]) < 0
    assert float(cells[1]["repulsion"]) > float(cells[0]["repulsion"])
    rows2 = V.main(["--pdbfile", str(pdb), "--sdf", str(sdf), "--out", str(tmp_path / "d.csv"), "--device", DEV])   # --bonds distance
    assert len(rows2) == 3 and all(np.isfinite(r[2].score) for r in rows2)
