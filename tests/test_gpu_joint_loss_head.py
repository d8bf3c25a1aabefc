"""The joint model's training loss terms on HIP launches (csrc/loss_head.h loss_joint_*, diffsbdd_amd/loss_head.py
joint_forward) against the torch mirror of the reference's terms (`EnVariationalDiffusion.forward`, DSBDD_LOSS=torch).

Criterion of tests/test_gpu_train.py::test_loss_terms_on_hip_launches_agree_with_the_torch_terms: the same call under both
settings with the same t and the same seed; the twelve terms to 1e-5 of max(1, |term|max), the four logged means to 1e-5
relative, the normalised batch left in the dictionaries to 1e-6, every parameter gradient of the l2 objective to 2e-5 of
that gradient's largest entry, the same set of parameters with a gradient."""
import os
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

NAMES = ("delta_log_px", "error_t_lig", "error_t_pocket", "SNR_weight", "loss_0_x_ligand", "loss_0_x_pocket", "loss_0_h",
         "neg_log_constants", "kl_prior", "log_pN", "t_int", "xh_lig_hat")
INFO = ("eps_hat_lig_x", "eps_hat_lig_h", "eps_hat_pocket_x", "eps_hat_pocket_h")


def dev():
    return torch.device("cuda:0")


@lru_cache(maxsize=None)
def _model(workload):
    from train_step_bench import build
    model, cfg, dd = build(workload, dev())
    model.train(True)
    return model, cfg, dd


def _ragged(n_lig, n_pocket, atom_nf, residue_nf, seed):
    """Random complexes in Angstrom: ligand atoms ~ N(0, 2^2), pocket atoms ~ N(0, 4^2) around the same centre, so that
    with norm_values[0] = 5 and the small architecture's cutoffs (0.8 / 1.4 in normalised units) every sample has
    ligand-pocket edges."""
    g = torch.Generator().manual_seed(seed)

    def node_set(sizes, nf, std):
        n = sum(sizes)
        one_hot = torch.zeros(n, nf)
        one_hot[torch.arange(n), torch.randint(0, nf, (n,), generator=g)] = 1.0
        sz = torch.tensor(sizes, dtype=torch.int64)
        return {"x": (std * torch.randn(n, 3, generator=g)).to(dev()), "one_hot": one_hot.to(dev()), "size": sz.to(dev()),
                "mask": torch.repeat_interleave(torch.arange(len(sizes)), sz).to(dev())}
    return node_set(n_lig, atom_nf, 2.0), node_set(n_pocket, residue_nf, 4.0)


def _batch(case):
    from diffsbdd_amd import synthetic as S
    if case == "ragged":
        model, cfg, dd = _model("small_joint")
        T = dd["timesteps"]
        lig, poc = _ragged([1, 7, 23, 12], [300, 5, 40, 257], cfg["atom_nf"], cfg["residue_nf"], seed=11)
        return model, lig, poc, torch.tensor([[0.0], [float(T)], [13.0], [1.0]])
    if case == "one":
        model, cfg, dd = _model("small_joint")
        lig, poc = _ragged([9], [31], cfg["atom_nf"], cfg["residue_nf"], seed=12)
        return model, lig, poc, torch.tensor([[0.0]])
    assert case == "moad"
    model, cfg, dd = _model("moad_fullatom_joint")
    t = torch.tensor(np.random.default_rng(3).integers(0, dd["timesteps"] + 1, size=(3, 1)), dtype=torch.float32)
    t[0, 0] = 0.0
    return model, S.anchor_ligand(3, 23, cfg["atom_nf"], dev()), S.load_pocket("fa", 3, dev()), t


def _run(case, mode, lj=False):
    """One forward + backward of `case` under DSBDD_LOSS=mode -> terms, info, parameter gradients, the batch left in the
    dictionaries, and the ligand-pocket pairs within the interaction cutoff per sample (from the network's input)."""
    from train_step_bench import loss_of
    model, ligand, pocket, t_fix = _batch(case)
    seen = {}

    def grab(_mod, args):
        seen["z"] = tuple(a.detach().clone() for a in args[:2])
    hook = model.dynamics.register_forward_pre_hook(grab)
    old = os.environ.get("DSBDD_LOSS")
    try:
        os.environ["DSBDD_LOSS"] = mode
        model.t_int_source = lambda b: t_fix
        model.seed(77)
        model.zero_grad(set_to_none=True)
        out = model(ligand, pocket, return_info=True)
        loss = loss_of(out[:12])
        if lj:       # a gradient through xh_lig_hat as well (what the LJ auxiliary term sends): the g_hat branch of the backward
            w = torch.randn(out[11].shape, generator=torch.Generator().manual_seed(5)).to(dev())
            loss = loss + (out[11] * w).sum()
        loss.backward()
    finally:
        hook.remove()
        model.t_int_source = None
        if old is None:
            os.environ.pop("DSBDD_LOSS", None)
        else:
            os.environ["DSBDD_LOSS"] = old
    lm, pm = ligand["mask"], pocket["mask"]
    d = torch.cdist(seen["z"][0][:, :3].double(), seen["z"][1][:, :3].double())
    near = (d <= float(model.dynamics.edge_cutoff_i)) & (lm[:, None] == pm[None, :])
    lp_edges = torch.zeros(t_fix.shape[0], dtype=torch.int64, device=dev()).index_add_(0, lm, near.sum(1)).cpu()
    return dict(terms=[torch.as_tensor(v).detach().float().cpu() for v in out[:12]],
                info={k: float(v.detach()) for k, v in out[12].items()}, info_dim={k: v.dim() for k, v in out[12].items()},
                grads={k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None},
                batch=[ligand["x"].detach().cpu(), ligand["one_hot"].detach().cpu(), pocket["x"].detach().cpu(),
                       pocket["one_hot"].detach().cpu()], lp_edges=lp_edges)


@lru_cache(maxsize=None)
def _ref(case, mode, lj=False):
    """Shared, computed once; nobody modifies it."""
    return _run(case, mode, lj)


def _compare(hip, ref):
    for nme, a, b in zip(NAMES, hip["terms"], ref["terms"]):
        assert a.shape == b.shape, (nme, a.shape, b.shape)
        scale = max(1.0, b.abs().max().item())
        err = (a - b).abs().max().item()
        print(f"  {nme}: |hip - torch| {err:.3e}  scale {scale:.3e}")
        assert torch.isfinite(a).all(), nme
        assert err <= 1e-5 * scale, (nme, err, scale)
    assert set(hip["info"]) == set(ref["info"]) == set(INFO)
    for k, v in ref["info"].items():
        print(f"  {k}: hip {hip['info'][k]:.8e}  torch {v:.8e}")
        assert hip["info_dim"][k] == 0 and abs(hip["info"][k] - v) <= 1e-5 * abs(v), k
    for a, b in zip(hip["batch"], ref["batch"]):
        assert a.shape == b.shape and (a - b).abs().max().item() <= 1e-6
    assert set(hip["grads"]) == set(ref["grads"]) and len(ref["grads"]) > 0
    worst = 0.0
    for k, g in ref["grads"].items():
        scale = max(g.abs().max().item(), 1e-6)
        err = (hip["grads"][k] - g).abs().max().item()
        worst = max(worst, err / scale)
        assert err <= 2e-5 * scale, (k, err, scale)
    print(f"  parameter gradients: worst relative difference {worst:.3e}")


def test_ragged_batch_agrees_with_the_torch_terms():
    """Ligand sizes [1, 7, 23, 12], pocket sizes [300, 5, 40, 257] (a one-atom ligand; segments shorter than, one more than
    and longer than one 256-thread stride), t = [0, T, 13, 1]."""
    ref, hip = _ref("ragged", "torch"), _ref("ragged", "hip")
    assert (ref["lp_edges"] > 0).all() and (hip["lp_edges"] > 0).all(), (ref["lp_edges"], hip["lp_edges"])
    tt = ref["terms"]
    # the t = 0 sample: the L0 terms are live and the error terms masked; every other sample the other way round
    # (loss_0_h of that sample may round to 0: sigma_0 is 30 times smaller than the distance between two classes)
    assert tt[4][0].item() > 0 and tt[5][0].item() > 0
    assert tt[1][0].item() == 0 and tt[2][0].item() == 0
    assert (tt[1][1:] > 0).all() and (tt[2][1:] > 0).all()
    assert (tt[4][1:] == 0).all() and (tt[5][1:] == 0).all() and (tt[6][1:] == 0).all()
    _compare(hip, ref)


def test_batch_of_one_agrees_with_the_torch_terms():
    ref, hip = _ref("one", "torch"), _ref("one", "hip")
    assert (ref["lp_edges"] > 0).all()
    assert ref["terms"][10].dim() == 0 and ref["terms"][1].shape == (1,)
    _compare(hip, ref)


def test_shipped_joint_config_agrees_with_the_torch_terms():
    """moad_fullatom_joint at its real width (H = 192, cutoffs 0.8 / 1.4), B = 3, the example pocket and ligand pose."""
    ref, hip = _ref("moad", "torch"), _ref("moad", "hip")
    assert (ref["lp_edges"] > 0).all()
    _compare(hip, ref)


def test_gradient_through_xh_lig_hat_agrees_with_the_torch_terms():
    """loss_of(terms) + (xh_lig_hat * w).sum(): the backward kernel's g_hat branch (the LJ auxiliary term's gradient)."""
    ref, hip = _ref("ragged", "torch", True), _ref("ragged", "hip", True)
    plain = _ref("ragged", "torch")
    assert any(not torch.equal(ref["grads"][k], plain["grads"][k]) for k in plain["grads"])
    _compare(hip, ref)


def test_two_runs_are_bitwise_equal():
    a, b = _ref("ragged", "hip"), _run("ragged", "hip")
    for nme, x, y in zip(NAMES, a["terms"], b["terms"]):
        assert torch.equal(x, y), nme
    assert a["info"] == b["info"]
    assert set(a["grads"]) == set(b["grads"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


def test_routing(monkeypatch):
    """The HIP head serves training mode under autograd only; evaluation, no_grad and DSBDD_LOSS=torch keep the mirror."""
    from diffsbdd_amd import loss_head
    model, ligand, pocket, t_fix = _batch("one")
    calls = []
    real = loss_head.joint_forward

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    def clone():
        return dict(ligand), dict(pocket)
    model.t_int_source = lambda b: t_fix
    try:
        monkeypatch.delenv("DSBDD_LOSS", raising=False)
        monkeypatch.setattr(loss_head, "joint_forward", counted)
        model(*clone())
        assert calls == [1]                       # the default in training mode

        def boom(*a, **k):
            raise AssertionError("joint_forward called")
        monkeypatch.setattr(loss_head, "joint_forward", boom)
        with torch.no_grad():
            model(*clone())
        model.eval()
        model.t_int_source = lambda b: t_fix + 1  # (evaluation draws t >= 1)
        model(*clone())
        model.train(True)
        monkeypatch.setenv("DSBDD_LOSS", "torch")
        model(*clone())
    finally:
        model.train(True)
        model.t_int_source = None
