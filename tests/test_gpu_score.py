"""Scoring given ligands on the GPU (`ConditionalDDPM.nll_given_pocket`, csrc/score.h): against the oracle
(`oracle.ddpm_oracle.loss_terms`) and the reference's recorded evaluation-mode terms, against the unchanged
evaluation-mode `forward`, bitwise across chunkings / repetitions / subsets, on edge shapes, and through the front ends
(`LigandGenerator.score_ligands`, `python -m diffsbdd_amd.score`).

Shapes are the fixture's own (loss_small_cond_eval: 3 ligands of 5, 8 and 6 atoms, 40-node pockets, T = 20).
Tolerances: 1e-4 max(1, max |term|) against the oracle and 5e-3 max(1, max |term|) against the reference's own numbers --
the two bounds of tests/test_gpu_parity.py::test_loss_terms_vs_oracle_and_reference_golden, for the same reasons (float32
network on the GPU against the CPU oracle; the reference's radius graph uses torch.cdist).  nll against the oracle:
1e-4 sum_i |coef_i| max(1, max |term_i|) over the terms of the combination, the product SNR_weight * error_t linearised
(coefficient 0.5 w |error_t| on SNR_weight and 0.5 w |SNR_weight| on error_t), from the ORACLE's terms."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from diffsbdd_amd import ligand_io, score, synthetic
from diffsbdd_amd.molecules import Molecule, write_sdf
from oracle import ddpm_oracle as do
from tests._golden import Case
from tests.test_oracle_golden import LOSS_NAMES, loss_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# returned term -> name in the reference's 12-tuple
PER_SLOT = {"error_t": "error_t_lig", "SNR_weight": "SNR_weight", "t": "t_int_out"}
PER_LIGAND = {"loss_0_x": "loss_0_x_ligand", "loss_0_h": "loss_0_h", "neg_log_constants": "neg_log_constants",
              "kl_prior": "kl_prior", "delta_log_px": "delta_log_px", "log_pN": "log_pN"}


def make_model(c, simple=False):
    from diffsbdd_amd.conditional_model import ConditionalDDPM, SimpleConditionalDDPM
    from diffsbdd_amd.dynamics import EGNNDynamics
    from diffsbdd_amd.en_diffusion import DistributionNodes
    cfg, dd = c.cfg, c.ddpm
    dyn = EGNNDynamics(**cfg, device=torch.device(DEV))
    dyn.load_state_dict(c.state_dict())
    cls = SimpleConditionalDDPM if simple else ConditionalDDPM
    model = cls(dynamics=dyn.eval(), atom_nf=cfg["atom_nf"], residue_nf=cfg["residue_nf"], n_dims=3,
                size_histogram=np.ones((12, 60)), timesteps=dd["timesteps"], noise_schedule=dd["noise_schedule"],
                noise_precision=dd["noise_precision"], loss_type="l2", norm_values=dd["norm_values"]).to(DEV)
    model.size_distribution = DistributionNodes(np.ones((12, 60)))          # the golden's histogram
    return model.eval()


def make_oracle(c, simple=False):
    cfg, dd = c.cfg, c.ddpm
    om = do.OracleModel(c.state_dict(), cfg, cfg["atom_nf"], cfg["residue_nf"], dd["timesteps"], dd["noise_schedule"],
                        dd["noise_precision"], norm_values=dd["norm_values"], conditional=dd["conditional"])
    if simple:
        om.simple = True
    return om


def to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def oracle_slots(om, model, ligand, pocket, times, draws):
    """The oracle composed slot by slot: one `do.loss_terms` call per time slot k, replaying [eps_k, eps_0].
    times [B, K] (float), draws = K + 1 noise blocks.  -> dict of float32 CPU tensors in the scorer's layout."""
    K = times.shape[1]
    log_pn = lambda n1, n2: model.size_distribution.log_prob_n1_given_n2(n1, n2)
    cols = []
    for k in range(K):
        ref = do.loss_terms(om, ligand, pocket, times[:, k:k + 1].float(), do.NoiseReplay([draws[k], draws[K]]), False,
                            size_log_prob=log_pn)
        cols.append(dict(zip(LOSS_NAMES, ref)))
    out = {mine: torch.stack([torch.as_tensor(col[theirs]).float() for col in cols], 1) for mine, theirs in PER_SLOT.items()}
    out.update({mine: torch.as_tensor(cols[0][theirs]).float() for mine, theirs in PER_LIGAND.items()})
    return out


def assert_terms(got, ref, weights, nll, what, gold=None):
    """Every returned term and nll against `ref` (the oracle) at the bounds of the module docstring; `gold`: the
    reference's recorded values (5e-3)."""
    for name in list(PER_SLOT) + list(PER_LIGAND):
        v, r = got[name].float().cpu(), ref[name]
        assert v.shape == r.shape, (what, name, v.shape, r.shape)
        scale = max(1.0, r.abs().max().item())
        err = (v - r).abs().max().item()
        print(f"[{what}] {name}: max |got - oracle| = {err:.2e} (scale {scale:.3g})")
        assert err <= 1e-4 * scale, (what, name, err)
        if gold is not None:
            g = gold[name]
            eg = (v.reshape(g.shape) - g).abs().max().item()
            assert eg <= 5e-3 * max(1.0, g.abs().max().item()), (what, name, "reference", eg)
    w = torch.broadcast_to(torch.as_tensor(weights, dtype=torch.float32), ref["error_t"].shape)
    nll_ref, loss_t_ref = score.combine_terms(w, ref["SNR_weight"], ref["error_t"], *(ref[k] for k in PER_LIGAND))
    big = lambda v: max(1.0, v.abs().max().item())
    bound = (0.5 * w * (ref["SNR_weight"].abs() * big(ref["error_t"]) + ref["error_t"].abs() * big(ref["SNR_weight"]))).sum(1)
    bound = 1e-4 * (bound + sum(big(ref[k]) for k in PER_LIGAND))
    err = (nll.float().cpu() - nll_ref).abs()
    print(f"[{what}] nll {nll.tolist()} oracle {nll_ref.tolist()} |diff| {err.tolist()} bound {bound.tolist()}")
    assert bool((err <= bound).all()), (what, err.tolist(), bound.tolist())
    assert (got["loss_t"].float().cpu() - loss_t_ref).abs().max().item() <= bound.max().item()


@pytest.fixture(scope="module")
def case():
    return Case("loss_small_cond_eval")


@pytest.fixture(scope="module")
def model(case):
    return make_model(case)


# --------------------------------------------------------------------------- 1. the reference's golden, K = 1
def test_k1_vs_oracle_and_reference_golden(case, model):
    c = case
    T = c.ddpm["timesteps"]
    ligand, pocket = loss_inputs(c)
    times = c.t("t_int").view(-1, 1)                                  # 3, 20, 11
    model.set_noise_source(do.NoiseReplay(c.noise()))
    try:
        nll, terms = model.nll_given_pocket(to_dev(ligand), to_dev(pocket), times=times, weights=float(T), return_terms=True)
    finally:
        model.set_noise_source(None)
    assert nll.dtype == torch.float32 and nll.shape == (3,) and nll.is_cuda
    assert terms["weight"].tolist() == [[float(T)]] * 3
    ref = oracle_slots(make_oracle(c), model, ligand, pocket, times, c.noise())
    gold = {mine: c.t("out_" + theirs).float() for mine, theirs in {**PER_SLOT, **PER_LIGAND}.items()}
    assert_terms(terms, ref, float(T), nll, "golden K=1", gold=gold)


# --------------------------------------------------------------------------- 2. several times per ligand
def test_several_times_per_ligand_vs_oracle(case, model):
    c = case
    ligand, pocket = loss_inputs(c)
    times = torch.tensor([[1, 20, 7, 7], [20, 1, 3, 12], [5, 5, 20, 1]])          # 1, T and a repeated value in every row
    weights = torch.tensor([[6.0, 2.5, 4.0, 7.5], [1.0, 9.0, 5.0, 5.0], [3.0, 3.0, 0.5, 13.5]])
    tape = do.NoiseTape(31)
    draws = [tape((ligand["x"].shape[0], 3 + c.cfg["atom_nf"])) for _ in range(5)]
    model.set_noise_source(do.NoiseReplay(draws))
    try:
        nll, terms = model.nll_given_pocket(to_dev(ligand), to_dev(pocket), times=times, weights=weights, return_terms=True)
    finally:
        model.set_noise_source(None)
    assert torch.equal(terms["t"].cpu(), times.float()) and torch.equal(terms["weight"].cpu(), weights)
    ref = oracle_slots(make_oracle(c), model, ligand, pocket, times, draws)
    assert_terms(terms, ref, weights, nll, "K=4")


# --------------------------------------------------------------------------- 3. the unchanged evaluation-mode forward
@pytest.mark.parametrize("simple", [False, True])
def test_k1_vs_evaluation_mode_forward(case, simple):
    """Same injected t and noise: the network kernels are the same, only the reduction order of the terms differs
    (1e-5 of each term's scale).  Also: `want_pocket=False` with one t per state."""
    c = case
    T = c.ddpm["timesteps"]
    m = make_model(c, simple=simple)
    ligand, pocket = loss_inputs(c)
    m.set_noise_source(do.NoiseReplay(c.noise()))
    m.t_int_source = lambda b: c.t("t_int")
    try:
        fwd = dict(zip(LOSS_NAMES, m(to_dev(ligand), to_dev(pocket))))
        m.set_noise_source(do.NoiseReplay(c.noise()))
        nll, terms = m.nll_given_pocket(to_dev(ligand), to_dev(pocket), times=c.t("t_int").view(-1, 1), weights=float(T),
                                        return_terms=True)
    finally:
        m.set_noise_source(None)
        m.t_int_source = None
    for mine, theirs in {**PER_SLOT, **PER_LIGAND}.items():
        r = torch.as_tensor(fwd[theirs]).float().cpu()
        v = terms[mine].float().cpu().reshape(r.shape)
        scale = max(1.0, r.abs().max().item())
        err = (v - r).abs().max().item()
        print(f"[forward simple={simple}] {mine}: {err:.2e} (scale {scale:.3g})")
        assert err <= 1e-5 * scale, (simple, mine, err)


# --------------------------------------------------------------------------- 4. / 5. chunking, repetition, subset
def test_chunking_and_repetition_are_bitwise(case, model):
    """times='all': 3 x 21 = 63 states; with max_states = 7 chunk boundaries fall inside a ligand's slots."""
    ligand, pocket = (to_dev(d) for d in loss_inputs(case))
    one = model.nll_given_pocket(ligand, pocket, times="all", seed=5, max_states=64, return_terms=True)
    many = model.nll_given_pocket(ligand, pocket, times="all", seed=5, max_states=7, return_terms=True)
    again = model.nll_given_pocket(ligand, pocket, times="all", seed=5, max_states=64, return_terms=True)
    assert one[1]["t"].shape == (3, 20) and one[1]["weight"].eq(1).all()
    assert torch.isfinite(one[0]).all()
    for other, what in ((many, "max_states=7"), (again, "repeated")):
        assert torch.equal(one[0], other[0]), (what, one[0].tolist(), other[0].tolist())
        for k in one[1]:
            assert torch.equal(one[1][k], other[1][k]), (what, k)
    other_seed = model.nll_given_pocket(ligand, pocket, times="all", seed=6)
    assert not torch.equal(other_seed, one[0])


def test_subset_with_ligand_ids_is_bitwise(case, model):
    ligand, pocket = loss_inputs(case)
    full = model.nll_given_pocket(to_dev(ligand), to_dev(pocket), n_times=4, seed=3, return_terms=True)
    lsel, psel = ligand["mask"] == 2, pocket["mask"] == 2
    lig2 = {"x": ligand["x"][lsel], "one_hot": ligand["one_hot"][lsel], "size": ligand["size"][2:], "mask": ligand["mask"][lsel] - 2}
    poc2 = {"x": pocket["x"][psel], "one_hot": pocket["one_hot"][psel], "size": pocket["size"][2:], "mask": pocket["mask"][psel] - 2}
    alone = model.nll_given_pocket(to_dev(lig2), to_dev(poc2), n_times=4, seed=3, ligand_ids=[2], return_terms=True)
    assert torch.equal(alone[0], full[0][2:])
    for k in full[1]:
        assert torch.equal(alone[1][k], full[1][k][2:]), k
    # without the id the ligand is keyed as ligand 0: other noise
    assert not torch.equal(model.nll_given_pocket(to_dev(lig2), to_dev(poc2), n_times=4, seed=3), full[0][2:])


# --------------------------------------------------------------------------- 6. edge shapes
def test_edge_shapes_vs_oracle(case, model):
    """A one-atom ligand, a ligand farther than every cutoff (5 A) from its pocket, ragged pocket sizes."""
    c = case
    ligand, pocket = loss_inputs(c)
    lm, pm = ligand["mask"], pocket["mask"]
    lkeep = torch.ones_like(lm, dtype=torch.bool)
    lkeep[(lm == 0).nonzero()[1:, 0]] = False                          # ligand 0: one atom
    pkeep = torch.ones_like(pm, dtype=torch.bool)
    pkeep[(pm == 1).nonzero()[17:, 0]] = False                         # pockets of 40, 17 and 33 nodes
    pkeep[(pm == 2).nonzero()[33:, 0]] = False
    lig = {"x": ligand["x"][lkeep].clone(), "one_hot": ligand["one_hot"][lkeep], "size": torch.tensor([1, 8, 6]), "mask": lm[lkeep]}
    poc = {"x": pocket["x"][pkeep], "one_hot": pocket["one_hot"][pkeep], "size": torch.tensor([40, 17, 33]), "mask": pm[pkeep]}
    lig["x"][lig["mask"] == 2] += torch.tensor([60.0, 0.0, 0.0])       # ligand 2: no ligand-pocket edge
    d = torch.cdist(lig["x"][lig["mask"] == 2], poc["x"][poc["mask"] == 2])
    assert d.min().item() > 5.0
    times = torch.tensor([[2, 19], [20, 1], [9, 10]])
    weights = torch.tensor([12.0, 8.0])
    tape = do.NoiseTape(8)
    draws = [tape((lig["x"].shape[0], 3 + c.cfg["atom_nf"])) for _ in range(3)]
    model.set_noise_source(do.NoiseReplay(draws))
    try:
        nll, terms = model.nll_given_pocket(to_dev(lig), to_dev(poc), times=times, weights=weights, return_terms=True)
    finally:
        model.set_noise_source(None)
    ref = oracle_slots(make_oracle(c), model, lig, poc, times, draws)
    assert_terms(terms, ref, weights, nll, "edge shapes")


# --------------------------------------------------------------------------- 7. front ends
def _example():
    from tests.test_gpu_ligand_design import example_residues, generator
    gen, _ = generator("small_cond", seed=2)
    residues, lig_x = example_residues("3rfm", "full-atom", keep=60)
    rng = np.random.RandomState(1)
    symbols = [gen.lig_type_decoder[int(t)] for t in rng.randint(0, 10, len(lig_x))]
    # the reference ligand and two perturbed copies (the last one as an (xyz, elements) pair)
    mols = [Molecule(lig_x, symbols), Molecule(lig_x + rng.normal(0, 0.3, lig_x.shape).astype(np.float32), symbols),
            (lig_x + rng.normal(0, 1.0, lig_x.shape).astype(np.float32), symbols)]
    return gen, residues, mols


def test_score_ligands_is_nll_given_pocket_on_the_hand_packed_batch():
    gen, residues, mols = _example()
    gen.select_pocket_residues = lambda pdb_file, pocket_ids=None, ref_ligand=None: residues
    rows = gen.score_ligands("3rfm.pdb", mols, ref_ligand="A:1", n_times=2, seed=4)
    assert [r["n_atoms"] for r in rows] == [m.num_atoms if hasattr(m, "num_atoms") else len(m[1]) for m in mols]
    templates = ligand_io.as_templates(mols, gen.lig_type_encoder)
    tx, tt, sizes = ligand_io.upload_templates(templates, gen.device)
    ligand, _ = ligand_io.pack_ligands(tx, tt, sizes, [0, 1, 2], sizes, gen.atom_nf)
    pocket = gen.prepare_pocket(residues, repeats=3)
    nll, terms = gen.ddpm.nll_given_pocket(ligand, pocket, n_times=2, seed=4, return_terms=True)
    assert [r["nll"] for r in rows] == nll.cpu().tolist()              # bit for bit
    assert [r["loss_t"] for r in rows] == terms["loss_t"].cpu().tolist()
    assert [r["kl_prior"] for r in rows] == terms["kl_prior"].cpu().tolist()
    assert [r["log_pN"] for r in rows] == terms["log_pN"].cpu().tolist()
    loss_0 = (terms["loss_0_x"] + terms["loss_0_h"]) + terms["neg_log_constants"]
    assert [r["loss_0"] for r in rows] == loss_0.cpu().tolist()
    assert all(np.isfinite(r["nll"]) for r in rows) and set(rows[0]) == {"nll", "loss_t", "loss_0", "kl_prior", "log_pN", "n_atoms"}


def test_score_command_line_writes_one_row_per_molecule(tmp_path):
    from diffsbdd_amd.en_diffusion import PredefinedNoiseSchedule
    from tests.test_ligand_design import PDB, hyper_parameters
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
    base = np.asarray([[4, 4, 3], [5.2, 4.3, 3.2], [3.3, 5.1, 3.4], [3.4, 2.7, 3.3], [4.5, 1.4, 3.9]], np.float32)
    mols = [Molecule(base, ["C", "O", "N", "C", "Cl"]), Molecule(base[:3] + np.float32(0.2), ["C", "O", "N"]),
            Molecule(base + np.float32(0.4), ["C", "C", "N", "C", "S"])]
    sdf = tmp_path / "ligands.sdf"
    write_sdf(sdf, mols)
    out = tmp_path / "scores.csv"
    res = subprocess.run([sys.executable, "-m", "diffsbdd_amd.score", "--checkpoint", str(ckpt), "--pdbfile", str(pdb),
                          "--ligands", str(sdf), "--ref_ligand", "A:100", "--n_times", "2", "--seed", "1", "--out", str(out)],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(res.stdout, res.stderr[-2000:])
    assert res.returncode == 0, res.stderr[-4000:]
    assert "wrote 3 scores" in res.stdout
    lines = out.read_text().strip().splitlines()
    assert lines[0] == "index,nll,loss_t,loss_0,kl_prior,log_pN,n_atoms" and len(lines) == 4
    rows = [l.split(",") for l in lines[1:]]
    assert [r[0] for r in rows] == ["0", "1", "2"] and [r[-1] for r in rows] == ["5", "3", "5"]      # input order
    assert all(np.isfinite(float(v)) for r in rows for v in r[1:-1])
