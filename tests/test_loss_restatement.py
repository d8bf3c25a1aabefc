"""Pins tests/_loss64.py -- the float64 reference of tests/test_gpu_loss_head_kernels.py -- on the CPU.

  * against oracle/ddpm_oracle.py: loss_terms(..., training=True) (itself pinned to vectors of the real reference by
    tests/test_oracle_golden.py) with the network replaced by a function that returns a given `net`, the same draws fed to
    both sides through NoiseReplay; ConditionalDDPM, SimpleConditionalDDPM and the joint model; all twelve terms and
    xh_lig_hat to 1e-12 of each term's largest magnitude (kl_prior: of its largest addend), everything in float64;
  * properties for what the oracle lacks: the virtual-atom mask, the size table's clamp, empty segments, zero cotangents;
  * the self-check: on every case of the GPU file the float32 evaluation of the restatement is inside the 1e-4 cap of the
    tolerance rule on every block, i.e. the inputs do not make the rule unsatisfiable for the reference alone.

What the self-check made shrink (the rule is not loosened): loss_0_h of t = 0 samples wherever sigma_0 norm_value_h is far
below the class spacing -- every shipped schedule, and the synthetic table with norm_value_h = 0.25.  There the float64 term
is 1e-9 .. 1e-4 per row, built from probabilities 1 - 1e-8 that float32 does not have, and the float32 restatement is off
by 1e-4 .. 1 of it (test_shrunk_loss_0_h_blocks_are_below_float32_resolution shows it).  In those cases the loss_0_h block
is compared without its t = 0 entries (_loss64.l0h_block); the term's arithmetic is checked on the synthetic table with
norm_value_h in {1, 4, 5}, where every t = 0 sample carries more than 0.1 per row.
"""
import math

import pytest
import torch

from oracle import ddpm_oracle as do
from tests import _loss64 as l64

F64 = torch.float64


def rel(a, b, mag=None):
    a, b = torch.as_tensor(a, dtype=F64).reshape(-1), torch.as_tensor(b, dtype=F64).reshape(-1)
    assert a.shape == b.shape
    mag = float(b.abs().max()) if mag is None else mag
    return float((a - b).abs().max()) / max(mag, 1e-300)


# ---- against the oracle -----------------------------------------------------------------------------------------------------
def oracle_case(width, table):
    """The ragged batch without its empty segment (the oracle's behaviour on one is not pinned): the empty pocket of
    sample 2 gets two rows.  A size table that holds every size: the oracle has no clamp."""
    lsz, psz = l64.BATCHES["ragged"]
    case = l64.make_case("ragged", width, table, "mixed", sizes=(lsz, [p or 2 for p in psz]))
    case["logpn"] = -torch.rand(301, 301, generator=torch.Generator().manual_seed(5), dtype=F64) * 9
    return case


def oracle_terms(case, model):
    a, r = case["a"], case["r"]
    m = do.OracleModel(None, None, a, r, case["T"], "polynomial_2", 1e-4, norm_values=(case["nv0"], case["nv1"]),
                       norm_biases=(None, case["nb1"]), conditional=model != "joint", simple=model == "simple")
    m.gamma = case["gamma"].double()                 # the case's table (the oracle's own gamma_table for the shipped ones)
    net = case["net_lig"].double(), case["net_poc"].double()
    m.dynamics = lambda *args: net
    lm, pm = l64.mask_of(case["lsz"]), l64.mask_of(case["psz"])
    lig = dict(x=case["lig_x"].double(), one_hot=case["lig_h"].double(), mask=lm, size=torch.tensor(case["lsz"]))
    poc = dict(x=case["poc_x"].double(), one_hot=case["poc_h"].double(), mask=pm, size=torch.tensor(case["psz"]))
    eps, npo = case["eps"].double(), case["noise_poc"].double()
    draws = [eps] if model != "joint" else [torch.cat([eps[:, :3], npo[:, :3]]), eps[:, 3:], npo[:, 3:]]
    replay = do.NoiseReplay(draws)
    default = torch.get_default_dtype()
    torch.set_default_dtype(F64)         # an integer size tensor times a python float (delta_log_px) takes the default dtype
    try:
        out = do.loss_terms(m, lig, poc, case["t_int"].double()[:, None], replay, training=True,
                            size_log_prob=lambda n1, n2: case["logpn"][n1, n2])
    finally:
        torch.set_default_dtype(default)
    assert replay.i == len(draws)
    return out


@pytest.mark.parametrize("table", l64.TABLES)
@pytest.mark.parametrize("width", list(l64.WIDTHS))
@pytest.mark.parametrize("model", l64.MODELS)
def test_restatement_agrees_with_the_oracle_in_float64(model, width, table):
    case = oracle_case(width, table)
    (delta_log_px, err_l, err_p, snr, l0xl, l0xp, l0h, nlc, kl, log_pn, t_int, xh_hat) = oracle_terms(case, model)
    cfg, pre, post = l64.reference(case, model, F64)
    ps, out = pre["per_sample"], post["out"]
    pairs = dict(delta_log_px=(ps["delta_log_px"], delta_log_px), SNR_weight=(ps["SNR_weight"], snr),
                 loss_0_h=(ps["loss_0_h"], l0h), neg_log_constants=(ps["neg_log_constants"], nlc),
                 log_pN=(ps["log_pN"], log_pn), t_int=(ps["t"] * case["T"], t_int), xh_lig_hat=(post["xh_hat"], xh_hat))
    if model == "joint":
        pairs.update(error_t_lig=(out["error_t_lig"], err_l), error_t_pocket=(out["error_t_pocket"], err_p),
                     loss_0_x_ligand=(out["loss_0_x_ligand"], l0xl), loss_0_x_pocket=(out["loss_0_x_pocket"], l0xp))
    else:
        pairs.update(error_t_lig=(out["error_t"], err_l), loss_0_x_ligand=(out["loss_0_x"], l0xl))
        assert float(err_p) == 0.0 and float(l0xp) == 0.0          # the conditional model's two constant terms
    for name, (mine, theirs) in pairs.items():
        e = rel(mine, theirs)
        print(f"  {name}: {e:.3e}")
        assert e <= 1e-12, (name, e)
    e = rel(ps["kl_prior"], kl, pre["kl_addend"])
    print(f"  kl_prior: {e:.3e} of its largest addend {pre['kl_addend']:.3e}")
    assert e <= 1e-12
    # both kinds of sample are present and select the term they should
    tz = case["t_int"] == 0
    err, l0x = pairs["error_t_lig"][0], pairs["loss_0_x_ligand"][0]
    assert tz.any() and (~tz).any()
    assert (err[tz] == 0).all() and (err[~tz] > 0).all() and (l0x[~tz] == 0).all() and (l0x[tz] > 0).all()


# ---- properties the oracle cannot pin ---------------------------------------------------------------------------------------------
def test_virtual_atoms_remove_exactly_their_coordinate_errors():
    case = l64.make_case("ragged", "crossdock_fullatom_cond", "synthetic", "mixed")
    _, pre, plain = l64.reference(case, "cond", F64, vnode_idx=-1)
    _, _, masked = l64.reference(case, "cond", F64, vnode_idx=2)
    virt = case["lig_h"][:, 2] == 1
    lo = l64.offsets(case["lsz"])
    for b, n in enumerate(case["lsz"]):          # make_case: one virtual and one real row in every sample of >= 2 rows
        assert n < 2 or (virt[lo[b]:lo[b + 1]].any() and not virt[lo[b]:lo[b + 1]].all())
    sq = ((case["eps"].double() - case["net_lig"].double()) ** 2)[:, :3].sum(1) * virt
    gone = l64.seg_sum(sq, l64.mask_of(case["lsz"]), len(case["lsz"]))
    tz = pre["per_sample"]["t_is_zero"]
    assert float(gone.min()) >= 0 and float(gone[torch.tensor(case["lsz"]) >= 7].min()) > 0
    assert rel(masked["out"]["error_t"], plain["out"]["error_t"] - gone * (1 - tz)) <= 1e-12
    assert rel(masked["out"]["loss_0_x"], plain["out"]["loss_0_x"] - 0.5 * gone * tz) <= 1e-12
    assert torch.equal(masked["xh_hat"], plain["xh_hat"]) and torch.equal(masked["out"]["info_x"], plain["out"]["info_x"])
    # a normalised one-hot with a bias is never 0: .bool() marks EVERY row (conditional_model.py:266 as written)
    biased = l64.make_case("ragged", "fullatom_biased", "synthetic", "mixed")
    _, _, post = l64.reference(biased, "cond", F64, vnode_idx=2)
    sq = (biased["eps"].double() - biased["net_lig"].double()) ** 2
    tz = (biased["t_int"] == 0).double()
    assert rel(post["out"]["error_t"], l64.seg_sum(sq[:, 3:], l64.mask_of(biased["lsz"]), 6) * (1 - tz)) <= 1e-12
    assert float(post["out"]["loss_0_x"].abs().max()) == 0.0


def test_size_table_lookup_beyond_the_table_returns_the_last_row_or_column():
    tab = torch.arange(12 * 60, dtype=F64).reshape(12, 60)
    n1, n2 = torch.tensor([0, 5, 11, 12, 300, 3, 257]), torch.tensor([0, 59, 60, 7, 1000, 60, 0])
    want = [tab[0, 0], tab[5, 59], tab[11, 59], tab[11, 7], tab[11, 59], tab[3, 59], tab[11, 0]]
    assert l64.table_lookup(tab, n1, n2).tolist() == [float(v) for v in want]
    assert l64.table_lookup(None, n1, n2).tolist() == [0.0] * 7
    case = l64.make_case("ragged", "odd", "synthetic", "mixed")
    ps = l64.reference(case, "joint", F64)[1]["per_sample"]
    assert ps["log_pN"][2] == case["logpn"][11, 0].double() and ps["log_pN"][5] == case["logpn"][11, 1].double()
    assert (l64.reference(case, "joint", F64, table=False)[1]["per_sample"]["log_pN"] == 0).all()


@pytest.mark.parametrize("model", l64.MODELS)
def test_empty_segment_counts_one_in_the_means_and_keeps_the_reference_dof(model):
    case = l64.make_case("empty", "moad_fullatom_joint", "synthetic", "mixed")
    lsz, psz = case["lsz"], case["psz"]
    assert lsz[1] == 0 and psz[2] == 0
    cfg, pre, post = l64.reference(case, model, F64)
    ps = pre["per_sample"]
    n = torch.tensor(lsz) + (torch.tensor(psz) if model == "joint" else 0)
    dof = (n * 3 if model == "simple" else (n - 1) * 3).double()           # subspace_dimensionality as written: -3 at n = 0
    assert torch.equal(ps["delta_log_px"], -dof * math.log(case["nv0"]))
    g0 = float(case["gamma"][0])
    assert rel(ps["neg_log_constants"], dof * (0.5 * g0 + 0.5 * math.log(2 * math.pi))) <= 1e-15
    for k, v in ps.items():
        assert torch.isfinite(v).all(), k
    for k, v in post["out"].items():
        assert torch.isfinite(v).all(), k
    # the empty ligand of sample 1: every sum over it is 0, its means are 0 / 1, and its pocket is only normalised
    po = l64.offsets(psz)
    if model == "joint":
        assert float(post["out"]["info_lig_x"][1]) == 0.0 and float(post["out"]["error_t_lig"][1]) == 0.0
        assert float(post["out"]["info_pocket_x"][2]) == 0.0 and float(post["out"]["info_pocket_x"][1]) > 0.0
        # noise centre of sample 2 (no pocket): over its 9 ligand rows alone
        lo = l64.offsets(lsz)
        assert rel(pre["eps_lig"][lo[2]:, :3].sum(0), torch.zeros(3), 1.0) <= 1e-14
    else:
        assert float(post["out"]["info_x"][1]) == 0.0 and float(post["out"]["error_t"][1]) == 0.0
        assert torch.equal(pre["xh_pocket"][po[1]:po[2], :3], case["poc_x"].double()[po[1]:po[2]] / case["nv0"])
        assert float(ps["loss_0_h"][1]) == 0.0


@pytest.mark.parametrize("model", ["cond", "joint"])
def test_zero_cotangents_give_a_zero_gradient(model):
    case = l64.make_case("ragged", "odd", "synthetic", "mixed")
    cfg, pre, _ = l64.reference(case, model, F64, vnode_idx=2)
    for g in l64.reference_backward(case, model, F64, cfg, pre, ()):
        assert float(g.abs().max()) == 0.0
    zero = dict(case, cot={k: torch.zeros_like(v) for k, v in case["cot"].items()})
    for g in l64.reference_backward(zero, model, F64, cfg, pre, l64.JOINT_COTANGENTS):
        assert float(g.abs().max()) == 0.0
    for g in l64.reference_backward(case, model, F64, cfg, pre, l64.JOINT_COTANGENTS):
        assert float(g.abs().max()) > 0.0


# ---- the self-check -----------------------------------------------------------------------------------------------------------
def self_check(case, model, vnode_idx):
    tag = f"{case['name']}/{model}/v{vnode_idx}"
    r64, r32 = l64.reference(case, model, F64, vnode_idx), l64.reference(case, model, torch.float32, vnode_idx)
    l64.compare_forward(tag, case, model, r32[1], r32[2], r64, r32)
    if case["name"].endswith(l64.BACKWARD_T_MODE) and model != "simple":
        for present in l64.cotangent_sets(model):
            b64 = l64.reference_backward(case, model, F64, r64[0], r64[1], present)
            b32 = l64.reference_backward(case, model, torch.float32, r32[0], r32[1], present)
            l64.compare_backward(f"{tag}.bwd[{'+'.join(present) or 'none'}]", b32, b64, b32)
    return r64


@pytest.mark.parametrize("width", list(l64.WIDTHS))
@pytest.mark.parametrize("model", l64.MODELS)
def test_float32_restatement_is_inside_the_cap_on_every_gpu_case(model, width):
    for case in l64.case_grid(width) + ([l64.big_case()] if width == "crossdock_fullatom_cond" else []):
        for v in ((-1,) if model == "joint" else (-1, 2)):
            (_, pre, _) = self_check(case, model, v)
        if case["l0h_resolved"]:        # otherwise the case proves nothing about the categorical term
            rows = torch.tensor(case["lsz"]) + (torch.tensor(case["psz"]) if model == "joint" else 0)
            live = (case["t_int"] == 0) & (rows > 0)
            per_row = pre["per_sample"]["loss_0_h"][live] / rows[live]
            assert live.sum() == 0 or float(per_row.min()) > 0.1, (case["name"], per_row)


def test_shrunk_loss_0_h_blocks_are_below_float32_resolution():
    """Why l0h_block drops the t = 0 entries where sigma_0 norm_value_h << 1: with them, the float32 restatement itself
    is off by 1e-5 .. 1e-3 of the block where sigma_0 norm_value_h ~ 0.1 (at or over the 1e-4 cap, depending on the draw) and
    returns exactly 0 for a float64 term of 1e-9 per row where it is ~ 0.01."""
    for width in l64.WIDTHS:
        for table in l64.TABLES:
            case = l64.make_case("ragged", width, table, "zeros")
            if case["l0h_resolved"]:
                continue
            worst = 0.0
            for model in ("cond", "joint"):
                v64 = l64.reference(case, model, F64)[1]["per_sample"]["loss_0_h"]
                v32 = l64.reference(case, model, torch.float32)[1]["per_sample"]["loss_0_h"]
                worst = max(worst, rel(v32, v64))
            print(f"  {case['name']}: float32 restatement off by {worst:.2e} of the block")
            # sigma_0 norm_value_h <= 0.02 on these two tables: every float32 probability is exactly 0 or 1, the term 0
            if table in ("polynomial_2/500/1e-5", "cosine/1000/1e-4"):
                assert worst > 0.99, (case["name"], worst)
