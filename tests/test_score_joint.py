"""Scoring given complexes under the joint model, host side (no GPU): the combination of the terms against
`train.nll_from_terms` on the reference's recorded evaluation-mode terms (bit for bit), every refusal of
`EnVariationalDiffusion.nll_of_complex` (all raised before any launch), and the C ABI of csrc/score_joint.h."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib, score
from diffsbdd_amd.train import nll_from_terms
from tests._golden import Case
from tests.test_ligand_design import make_generator
from tests.test_oracle_golden import LOSS_NAMES, loss_inputs
from tests.test_score import _batch

JOINT_ORDER = ("SNR_weight", "error_t_lig", "error_t_pocket", "loss_0_x_ligand", "loss_0_x_pocket", "loss_0_h",
               "neg_log_constants", "kl_prior", "delta_log_px", "log_pN")


# --------------------------------------------------------------------------- host combination
def test_combine_terms_joint_is_nll_from_terms_on_the_reference_golden():
    c = Case("loss_small_joint_eval")
    terms = tuple(c.t("out_" + n) for n in LOSS_NAMES)
    ligand, pocket = loss_inputs(c)
    T = c.ddpm["timesteps"]
    want, _ = nll_from_terms(terms, ligand, pocket, loss_type="l2", training=False, T=T, x_dims=3,
                             atom_nf=c.cfg["atom_nf"], residue_nf=c.cfg["residue_nf"])
    g = dict(zip(LOSS_NAMES, terms))
    assert g["error_t_pocket"].abs().min().item() > 0                  # the joint golden: the pocket is scored
    nll, loss_t, loss_t_lig = score.combine_terms_joint(float(T), *(g[k] for k in JOINT_ORDER))
    assert nll.dtype == torch.float32 and nll.shape == want.shape == (2,)
    print(f"[combine joint] nll {nll.tolist()} nll_from_terms {want.tolist()}")
    assert torch.equal(nll, want.float())
    assert torch.equal(loss_t, (-T * 0.5 * g["SNR_weight"] * (g["error_t_lig"] + g["error_t_pocket"])).float())
    assert torch.equal(loss_t_lig, ((-0.5 * T) * g["SNR_weight"] * g["error_t_lig"]).float())
    # [B, K] inputs with K = 2: a slot of weight zero changes nothing
    two = lambda v: torch.stack([v, v], 1)
    rest = [g[k] for k in JOINT_ORDER[3:]]
    nll2, _, lig2 = score.combine_terms_joint(torch.tensor([float(T), 0.0]), two(g["SNR_weight"]), two(g["error_t_lig"]),
                                              two(g["error_t_pocket"]), *rest)
    assert torch.equal(nll2, nll) and torch.equal(lig2, loss_t_lig)


# --------------------------------------------------------------------------- refusals, all before any launch
def test_refusals_without_a_gpu():
    ddpm = make_generator("small_joint", "joint").ddpm                 # histogram [40][400], CPU
    ligand, pocket = _batch()
    # the pocket-conditioned model has the other method; a learned schedule; virtual atoms; no size table
    cond = make_generator("small_cond", "pocket_conditioning").ddpm
    with pytest.raises(NotImplementedError, match="nll_given_pocket"):
        cond.nll_of_complex(ligand, pocket)
    with pytest.raises(NotImplementedError, match="nll_given_pocket"):
        score.nll_of_complex(cond, ligand, pocket)
    from diffsbdd_amd.en_diffusion import EnVariationalDiffusion
    learned = EnVariationalDiffusion(dynamics=ddpm.dynamics, atom_nf=10, residue_nf=10, n_dims=3,
                                     size_histogram=np.ones((40, 400)), timesteps=20, noise_schedule="learned",
                                     loss_type="vlb", norm_values=(1.0, 4.0))
    with pytest.raises(NotImplementedError, match="schedule"):
        learned.nll_of_complex(ligand, pocket)
    ddpm.vnode_idx = 3
    try:
        with pytest.raises(NotImplementedError, match="virtual"):
            ddpm.nll_of_complex(ligand, pocket)
    finally:
        ddpm.vnode_idx = None
    sizes = ddpm.size_distribution
    ddpm.size_distribution = types.SimpleNamespace(log_prob=sizes.log_prob)
    try:
        with pytest.raises(NotImplementedError, match="_table"):
            ddpm.nll_of_complex(ligand, pocket)
    finally:
        ddpm.size_distribution = sizes
    # sizes outside the histogram, or of probability zero under the JOINT table: named by ligand index, no clamp
    big_l, big_p = _batch(sizes=(5, 41, 6))
    with pytest.raises(ValueError, match="ligand 1.*histogram"):
        ddpm.nll_of_complex(big_l, big_p)
    wide_l, wide_p = _batch(n_pocket=400)
    with pytest.raises(ValueError, match="ligand 0.*histogram"):
        ddpm.nll_of_complex(wide_l, wide_p)
    table = ddpm.size_distribution._table(2, torch.device("cpu"))
    saved = table[6, 40].item()
    table[6, 40] = float("-inf")
    try:
        with pytest.raises(ValueError, match="ligand 2.*probability zero"):
            ddpm.nll_of_complex(ligand, pocket)
    finally:
        table[6, 40] = saved
    # unsorted masks
    with pytest.raises(ValueError, match="sorted"):
        ddpm.nll_of_complex(dict(ligand, mask=ligand["mask"].flip(0)), pocket)
    with pytest.raises(ValueError, match="sorted"):
        ddpm.nll_of_complex(ligand, dict(pocket, mask=pocket["mask"].flip(0)))
    # the time slots
    for kw in (dict(n_times=0), dict(n_times=21), dict(times=[0, 3]), dict(times=[21]), dict(times=[2.5]),
               dict(times=torch.ones(2, 3)), dict(times=[3, 4], weights=[1.0, 2.0, 3.0]), dict(max_states=0),
               dict(ligand_ids=[0, 1])):
        with pytest.raises(ValueError):
            ddpm.nll_of_complex(ligand, pocket, **kw)
    # injected noise needs a single chunk
    ddpm.set_noise_source(lambda shape: torch.zeros(shape))
    try:
        with pytest.raises(ValueError, match="single chunk"):
            ddpm.nll_of_complex(ligand, pocket, n_times=4, max_states=7)
    finally:
        ddpm.set_noise_source(None)
    # a CPU module / CPU tensors: no fallback; the dicts and the module's generator state are untouched
    keep = {k: v.clone() for k, v in ligand.items()}
    state = (ddpm._seed, ddpm._draw, ddpm._sample_ids)
    with pytest.raises(_lib.HipLibraryError, match="nll_of_complex"):
        ddpm.nll_of_complex(ligand, pocket, n_times=2)
    assert all(torch.equal(ligand[k], keep[k]) for k in keep)
    assert (ddpm._seed, ddpm._draw, ddpm._sample_ids) == state
    assert not ddpm.training


def test_score_ligands_still_refuses_a_model_with_neither_method():
    gen = make_generator("small_joint", "joint")
    gen.ddpm = torch.nn.Identity()
    with pytest.raises(NotImplementedError, match="scored under"):
        gen.score_ligands("none.pdb", [], ref_ligand="A:1")


# --------------------------------------------------------------------------- C ABI
def test_score_joint_abi_is_declared_on_both_sides():
    with open(os.path.join(os.path.dirname(_lib._HERE), "include", "diffsbdd_hip.h")) as f:
        header = f.read()
    for name in ("dsbdd_score_joint_rows", "dsbdd_score_joint_pre", "dsbdd_score_joint_post", "dsbdd_score_joint_reduce"):
        assert name in _lib.SIGNATURES and f"int {name}(" in header
    assert _lib.ABI_VERSION == 6


def test_score_joint_entry_points_refuse_bad_arguments_without_a_launch():
    lib = _lib.load()
    assert [lib.dsbdd_score_joint_rows(w) for w in (0, 1, 2, 3)] == [10, 4, 10, 0]
    assert [lib.dsbdd_score_rows(w) for w in (0, 1, 2, 3)] == [8, 4, 8, 0]              # the conditional counts stay
    mk = lambda **kw: _lib.LossCfg(**{**dict(batch=3, n_lig=19, n_pocket=120, atom_nf=10, residue_nf=10, timesteps=20,
                                             remove_com=0, vnode_idx=-1, norm_value_x=1.0, norm_value_h=4.0, norm_bias_h=0.0,
                                             n1_tab=12, n2_tab=60), **kw})
    err = lambda: lib.dsbdd_last_error().decode()
    pre = lambda cfg, n_slots, first, n: lib.dsbdd_score_joint_pre(None, C.byref(cfg), n_slots, first, n, 64, 512, 1,
                                                                   *[None] * 20)
    post = lambda cfg, n_slots, first, n: lib.dsbdd_score_joint_post(None, C.byref(cfg), n_slots, first, n, 64, 512,
                                                                     *[None] * 11)
    for fn in (pre, post):
        assert fn(mk(), 2, 0, 6) == _lib.ERR_ARG and "null argument" in err()          # a valid chunk, no arrays
        for cfg, n_slots, first, n in ((mk(vnode_idx=3), 2, 0, 6),                   # virtual atoms
                                       (mk(), 1, 0, 3),                               # no time slot
                                       (mk(), 2, 5, 2), (mk(), 2, -1, 2), (mk(), 2, 0, 0),      # chunk outside the 6 states
                                       (mk(batch=0), 2, 0, 1), (mk(norm_value_h=0.0), 2, 0, 1),
                                       (mk(norm_value_x=-1.0), 2, 0, 1)):
            assert fn(cfg, n_slots, first, n) == _lib.ERR_ARG and "chunk" in err(), (n_slots, first, n)
    assert lib.dsbdd_score_joint_reduce(None, 3, 2, None, None, None, None) == _lib.ERR_ARG
    assert lib.dsbdd_score_joint_reduce(None, 0, 2, None, None, None, None) == _lib.ERR_ARG
