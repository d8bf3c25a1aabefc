"""GPU parity tests (-m gpu): the HIP path, called through the C-ABI, against
the oracle on the same seeded inputs and against the committed golden vectors
generated from the real reference.  Tolerance for every floating-point
comparison: 1e-4 absolute (BASELINE.json north_star: "within 1e-4 fp32 per
timestep"), stated next to each assert."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ddpm_oracle as do
from oracle import egnn_oracle as eo
from oracle import weights as W
from tests._golden import Case, DYN_CASES

pytestmark = pytest.mark.gpu
TOL = 1e-4


def dev():
    return torch.device("cuda:0")


def excess(a, b, atol=TOL, rtol=1e-5):
    """max(|a-b| - (atol + rtol*|b|)): <= 0 means allclose.  atol = the 1e-4 of the
    north star; the rtol term only matters where the state itself is large (the
    untrained joint model drives |z| to several hundred, where one fp32 ulp is
    already 6e-5)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs() - (atol + rtol * b.abs())).max().item()


def exact_pdist(x):
    d = x[:, None, :].double() - x[None, :, :].double()
    return (d * d).sum(-1).sqrt()


def make_dynamics(cfg, sd):
    from diffsbdd_amd.dynamics import EGNNDynamics
    m = EGNNDynamics(**cfg, device=dev())
    m.load_state_dict(sd)
    return m.eval()      # inference: the HIP kernels (training mode + autograd = the differentiable path, train_path.py)


def make_ddpm(c, sd=None):
    from diffsbdd_amd.conditional_model import ConditionalDDPM
    from diffsbdd_amd.en_diffusion import EnVariationalDiffusion
    cfg, dd = c.cfg, c.ddpm
    dyn = make_dynamics(cfg, sd if sd is not None else c.state_dict())
    cls = ConditionalDDPM if dd["conditional"] else EnVariationalDiffusion
    return cls(dynamics=dyn, atom_nf=cfg["atom_nf"], residue_nf=cfg["residue_nf"], n_dims=3,
               size_histogram=np.ones((4, 8)), timesteps=dd["timesteps"],
               noise_schedule=dd["noise_schedule"], noise_precision=dd["noise_precision"],
               loss_type="l2", norm_values=dd["norm_values"]).to(dev())


# ---------------------------------------------------------------------------
# kernels in isolation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,K1,K2,N,act,res,vec", [
    (1000, 256, 0, 512, 0, False, True),      # P|Q projection
    (777, 256, 256, 256, 1, False, True),     # node MLP layer 1: two sources
    (4099, 256, 0, 256, 0, True, True),       # node MLP layer 2: residual, in place
    (50, 10, 0, 20, 1, False, False),         # encoder: unaligned rows (xh[:, 3:])
    (333, 132, 0, 256, 0, False, True),       # embedding (K padded to 132)
    (333, 256, 0, 132, 0, False, True),       # embedding_out
    (65, 20, 0, 10, 0, False, True),          # decoder -> strided output
    (70000, 192, 0, 768, 0, False, True),     # big-M path (128-row tiles)
    (1, 64, 0, 64, 1, False, True),
    (2500, 192, 192, 192, 1, False, True),    # H = 192 (joint model): 64-wide K steps, 64-column tiles
    (3000, 128, 0, 384, 0, True, True),       # H = 128, residual
    (129, 256, 0, 1024, 0, False, True),      # one full + one 1-row workgroup tile, 128-column tiles
])
def test_node_linear_vs_torch_fp32(M, K1, K2, N, act, res, vec):
    from diffsbdd_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(M + N)
    lda1 = K1 if vec else K1 + 3
    A1 = torch.randn(M, lda1, generator=g)
    A2 = torch.randn(M, K2, generator=g) if K2 else None
    ldw = (N + 3) // 4 * 4
    WT = torch.zeros(K1 + K2, ldw)
    WT[:, :N] = torch.randn(K1 + K2, N, generator=g) / (K1 + K2) ** 0.5
    bias = torch.randn(N, generator=g)
    ldc = N + 3 if not vec or N == 10 else N
    Cbuf = torch.zeros(M, ldc)
    R = torch.randn(M, ldc, generator=g) if res else None
    a_view = A1[:, 3:] if not vec else A1
    ref = torch.cat([a_view[:, :K1]] + ([A2] if K2 else []), 1) @ WT[:, :N] + bias
    if act:
        ref = torch.nn.functional.silu(ref)
    if res:
        ref = ref + R[:, :N]
    d = dev()
    A1d, WTd, bd = A1.to(d), WT.to(d), bias.to(d)
    A2d = A2.to(d) if K2 else None
    Cd = R.to(d).clone() if res else Cbuf.to(d)
    a_ptr = A1d.data_ptr() + (12 if not vec else 0)
    rc = lib.dsbdd_node_linear(None, a_ptr, lda1, K1, A2d.data_ptr() if K2 else None, K2, K2, WTd.data_ptr(), ldw,
                               bd.data_ptr(), Cd.data_ptr() if res else None, ldc, Cd.data_ptr(), ldc, M, N, act)
    _lib.check(rc, "dsbdd_node_linear")
    torch.cuda.synchronize()
    out = Cd.cpu()[:, :N]
    err = (out - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err < 2e-5 * max(1.0, scale), (err, scale)
    if ldc > N and not res:   # columns beyond N are untouched
        assert Cd.cpu()[:, N:].abs().max().item() == 0.0


@pytest.mark.parametrize("name", DYN_CASES)
def test_radius_graph_vs_reference_edges(name):
    """dynamics.py:169-187: same edge set as the reference up to the cdist
    ambiguity band, sorted by (row, col), same-sample only."""
    c = Case(name)
    m = make_dynamics(c.cfg, c.state_dict())
    xl, xp = c.t("xh_lig")[:, :3], c.t("xh_pocket")[:, :3]
    ml, mp = c.t("mask_lig"), c.t("mask_pocket")
    e = m.get_edges(ml.to(dev()), mp.to(dev()), xl.to(dev()), xp.to(dev())).cpu()
    ref = c.t("edges", torch.int64)
    n = len(ml) + len(mp)
    key = e[0] * n + e[1]
    assert torch.all(key[1:] > key[:-1]), "not sorted by (row, col) / duplicates"
    mask = torch.cat([ml, mp])
    assert torch.all(mask[e[0]] == mask[e[1]])
    a = torch.zeros(n, n, dtype=torch.bool); a[ref[0], ref[1]] = True
    b = torch.zeros(n, n, dtype=torch.bool); b[e[0], e[1]] = True
    band = eo.edge_ambiguity_band(ml, mp, xl, xp, c.cfg["edge_cutoff_ligand"], c.cfg["edge_cutoff_pocket"],
                                  c.cfg["edge_cutoff_interaction"], tol=1e-3)
    assert not ((a ^ b) & ~band).any()
    # the exact-distance oracle builder must agree exactly
    e2 = eo.get_edges(ml, mp, xl, xp, c.cfg["edge_cutoff_ligand"], c.cfg["edge_cutoff_pocket"],
                      c.cfg["edge_cutoff_interaction"], exact=True)
    a2 = torch.zeros(n, n, dtype=torch.bool); a2[e2[0], e2[1]] = True
    band2 = eo.edge_ambiguity_band(ml, mp, xl, xp, c.cfg["edge_cutoff_ligand"], c.cfg["edge_cutoff_pocket"],
                                   c.cfg["edge_cutoff_interaction"], tol=1e-5)
    assert not ((a2 ^ b) & ~band2).any()


# ---------------------------------------------------------------------------
# EGNNDynamics.forward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", DYN_CASES)
def test_dynamics_forward_teacher_forced_edges(name):
    """Kernel parity: reference edge list fed to both sides; eps and every
    block's (h, x) within 1e-4 of the golden / oracle."""
    c = Case(name)
    sd = c.state_dict()
    m = make_dynamics(c.cfg, sd)
    edges = c.t("edges", torch.int64)
    n = len(c.t("mask_lig")) + len(c.t("mask_pocket"))
    th, tx = m.engine().set_trace(n)
    e_l, e_p, status = m.forward_async(c.t("xh_lig"), c.t("xh_pocket"), c.t("t"), c.t("mask_lig"),
                                       c.t("mask_pocket"), edges=edges)
    torch.cuda.synchronize()
    m.engine().clear_trace()
    assert int(status.item()) == 0
    trace = []
    eo.dynamics_forward(sd, c.cfg, c.t("xh_lig"), c.t("xh_pocket"), c.t("t"), c.t("mask_lig"),
                        c.t("mask_pocket"), edges=edges, trace=trace)
    for i, (h, x) in enumerate(trace):
        ex = (tx[i].cpu() - x).abs().max().item()
        eh = (th[i].cpu() - h).abs().max().item()
        assert ex < TOL and eh < TOL * max(1.0, h.abs().max().item()), (name, i, ex, eh)   # 1e-4
    err_l = (e_l.cpu() - c.t("eps_lig")).abs().max().item()
    err_p = (e_p.cpu() - c.t("eps_pocket")).abs().max().item()
    assert err_l < TOL and err_p < TOL, (name, err_l, err_p)                                 # 1e-4


@pytest.mark.parametrize("name", DYN_CASES)
def test_dynamics_forward_public_api(name):
    """The plain reference call signature (edges built on device)."""
    c = Case(name)
    m = make_dynamics(c.cfg, c.state_dict())
    xl, xp = c.t("xh_lig").to(dev()), c.t("xh_pocket").to(dev())
    xl0, xp0 = xl.clone(), xp.clone()
    e_l, e_p = m(xl, xp, c.t("t").to(dev()), c.t("mask_lig").to(dev()), c.t("mask_pocket").to(dev()))
    assert torch.equal(xl, xl0) and torch.equal(xp, xp0), "inputs must not be modified"
    assert e_l.shape == xl.shape and e_p.shape == xp.shape
    er, ec = m.engine().last_edges(len(xl) + len(xp))
    ref = c.t("edges", torch.int64)
    if er.numel() == ref.shape[1] and torch.equal(er, ref[0]) and torch.equal(ec, ref[1]):
        assert (e_l.cpu() - c.t("eps_lig")).abs().max().item() < TOL       # 1e-4
        assert (e_p.cpu() - c.t("eps_pocket")).abs().max().item() < TOL
    else:   # an edge inside the cdist ambiguity band flipped: compare with the oracle on OUR edges
        n = len(xl) + len(xp)
        flips = np.setxor1d((er * n + ec).numpy(), (ref[0] * n + ref[1]).numpy()).size
        print(f"[{name}] {flips} of {ref.shape[1]} edges differ from the reference's torch.cdist radius graph "
              f"(inside the cutoff ambiguity band, SURVEY.md 0.6)")
        o_l, o_p, _ = eo.dynamics_forward(c.state_dict(), c.cfg, c.t("xh_lig"), c.t("xh_pocket"), c.t("t"),
                                          c.t("mask_lig"), c.t("mask_pocket"), edges=torch.stack([er, ec]))
        assert (e_l.cpu() - o_l).abs().max().item() < TOL
        assert (e_p.cpu() - o_p).abs().max().item() < TOL


def test_nan_contract():
    """dynamics.py:155-159: ValueError in eval mode."""
    c = Case("dyn_small_cond")
    m = make_dynamics(c.cfg, c.state_dict())
    xl = c.t("xh_lig").clone()
    xl[0, 0] = float("nan")
    with pytest.raises(ValueError, match="NaN detected in EGNN output"):
        m(xl.to(dev()), c.t("xh_pocket").to(dev()), c.t("t").to(dev()), c.t("mask_lig").to(dev()),
          c.t("mask_pocket").to(dev()))


def test_single_t_broadcast():
    """dynamics.py:104-107: one t for the whole batch."""
    c = Case("dyn_small_cond")
    sd = c.state_dict()
    m = make_dynamics(c.cfg, sd)
    t1 = torch.full((1, 1), 0.37)
    edges = c.t("edges", torch.int64)
    e_l, e_p, _ = m.forward_async(c.t("xh_lig"), c.t("xh_pocket"), t1, c.t("mask_lig"), c.t("mask_pocket"),
                                  edges=edges, batch=3)
    o_l, o_p, _ = eo.dynamics_forward(sd, c.cfg, c.t("xh_lig"), c.t("xh_pocket"), t1, c.t("mask_lig"),
                                      c.t("mask_pocket"), edges=edges)
    assert (e_l.cpu() - o_l).abs().max().item() < TOL
    assert (e_p.cpu() - o_p).abs().max().item() < TOL


@pytest.mark.parametrize("arch", ["crossdock_fullatom_cond", "moad_fullatom_joint"])
def test_se3_equivariance_full_size(arch):
    """SE(3) equivariance by construction (egnn_new.py:296-316): rotate +
    translate the inputs -> velocities rotate, feature predictions invariant."""
    c = Case("dyn_fullatom_cond" if "cond" in arch else "dyn_fullatom_joint")
    m = make_dynamics(c.cfg, c.state_dict())
    g = torch.Generator().manual_seed(5)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    shift = torch.tensor([[0.3, -0.2, 0.5]])
    edges = c.t("edges", torch.int64)
    xl, xp = c.t("xh_lig"), c.t("xh_pocket")
    a_l, a_p, _ = m.forward_async(xl, xp, c.t("t"), c.t("mask_lig"), c.t("mask_pocket"), edges=edges)
    xl2 = torch.cat([xl[:, :3] @ q.T + shift, xl[:, 3:]], 1)
    xp2 = torch.cat([xp[:, :3] @ q.T + shift, xp[:, 3:]], 1)
    b_l, b_p, _ = m.forward_async(xl2, xp2, c.t("t"), c.t("mask_lig"), c.t("mask_pocket"), edges=edges)
    a_l, b_l, a_p, b_p = a_l.cpu(), b_l.cpu(), a_p.cpu(), b_p.cpu()
    assert (a_l[:, :3] @ q.T - b_l[:, :3]).abs().max().item() < TOL
    assert (a_l[:, 3:] - b_l[:, 3:]).abs().max().item() < TOL
    assert (a_p[:, :3] @ q.T - b_p[:, :3]).abs().max().item() < TOL
    assert (a_p[:, 3:] - b_p[:, 3:]).abs().max().item() < TOL


@pytest.mark.parametrize("variant", ["32", "sk"])
def test_bitwise_reproducible_and_forced_multi_tile_loop(variant, monkeypatch):
    """(variant "sk": every stage on the split-K kernels, csrc/edge_splitk.h.)  The edge aggregation has a fixed summation order (csrc/edge_mlp.h: plain stores + ordered
    head partial sums, no atomics): repeated calls are bitwise equal, and so is a run whose tiles
    are distributed differently over the workgroups.  DSBDD_EDGE_MAX_WG caps the persistent grid at
    8 (GCL) / 16 (coordinate stage) workgroups, so every workgroup walks many tiles (work queue,
    next-tile prefetch, commit_edge, the continuous W2^T stream across units) -- the path large
    batches take -- and must reproduce the reference-generated eps."""
    import os
    if variant == "sk":
        monkeypatch.setenv("DSBDD_SPLITK", "0xFFFFFFFF")
    c = Case("dyn_fullatom_cond")
    sd = c.state_dict()
    args = (c.t("xh_lig"), c.t("xh_pocket"), c.t("t"), c.t("mask_lig"), c.t("mask_pocket"))
    m = make_dynamics(c.cfg, sd)
    assert m.engine().get_option(4) == (-1 if variant == "sk" else 0)
    a, ap, _ = m.forward_async(*args)
    for _ in range(3):
        b, bp, _ = m.forward_async(*args)
        assert torch.equal(a, b) and torch.equal(ap, bp)
    os.environ["DSBDD_EDGE_MAX_WG"] = "8"
    try:
        mv = make_dynamics(c.cfg, sd)
        d1, p1, _ = mv.forward_async(*args)
        d2, p2, _ = mv.forward_async(*args)
    finally:
        del os.environ["DSBDD_EDGE_MAX_WG"]
    assert torch.equal(d1, d2) and torch.equal(p1, p2)
    assert torch.equal(a, d1) and torch.equal(ap, p1)        # independent of the tile -> workgroup assignment
    assert (d1.cpu() - c.t("eps_lig")).abs().max().item() < TOL           # 1e-4
    assert (p1.cpu() - c.t("eps_pocket")).abs().max().item() < TOL


@pytest.mark.parametrize("variant", ["32", "sk"])
def test_batch_composition_invariance_bitwise(variant, monkeypatch):
    """a sample's result must not depend on what else is in the batch.  Every
    (sample, node set) segment of the edge list starts at a wave-tile boundary and all per-row /
    per-sample sums have a fixed order, so eps of samples 0..1 evaluated alone equals, bit for bit,
    their rows in the 3-sample batch (device-built edges, both model kinds).  variant "sk": every stage on the
    split-K kernels (csrc/edge_splitk.h; H = 256 models -- the others ignore the mask)."""
    if variant == "sk":
        monkeypatch.setenv("DSBDD_SPLITK", "0xFFFFFFFF")
    for name in ("dyn_fullatom_cond", "dyn_ca_cond") if variant == "sk" else ("dyn_fullatom_cond", "dyn_fullatom_joint", "dyn_small_variant"):
        c = Case(name)
        m = make_dynamics(c.cfg, c.state_dict())
        d = dev()
        xl, xp, t, ml, mp = (c.t(k).to(d) for k in ("xh_lig", "xh_pocket", "t", "mask_lig", "mask_pocket"))
        B = int(max(ml.max(), mp.max())) + 1
        assert B >= 2
        full_l, full_p = m(xl, xp, t, ml, mp)
        keep = B - 1
        sl, sp = ml < keep, mp < keep
        sub_l, sub_p = m(xl[sl], xp[sp], t[:keep], ml[sl], mp[sp])
        assert torch.equal(sub_l, full_l[sl]) and torch.equal(sub_p, full_p[sp]), name
        # ... and the last sample alone (relabelled 0)
        sl, sp = ml == keep, mp == keep
        one_l, one_p = m(xl[sl], xp[sp], t[keep:], ml[sl] - keep, mp[sp] - keep)
        assert torch.equal(one_l, full_l[sl]) and torch.equal(one_p, full_p[sp]), name


# ---------------------------------------------------------------------------
# DDPM steps and loops
# ---------------------------------------------------------------------------
def test_cond_reverse_step_teacher_forced():
    """conditional_model.py:432-464 per timestep: golden z_t in, z_s out, 1e-4."""
    c = Case("ddpm_small_cond")
    model = make_ddpm(c)
    noise = c.noise()
    d = dev()
    lm = torch.repeat_interleave(torch.arange(len(c.t("num_nodes_lig"))), c.t("num_nodes_lig")).to(d)
    pm = c.t("pocket_mask").to(d)
    worst = 0.0
    for i, g in enumerate(c.steps()):
        model.set_noise_source(do.NoiseReplay([noise[1 + i]]))
        zs, ps = model.sample_p_zs_given_zt(g["s"].to(d), g["t"].to(d), g["zt"].to(d), g["pt"].to(d), lm, pm)
        worst = max(worst, (zs.cpu() - g["zs"]).abs().max().item(), (ps.cpu() - g["ps"]).abs().max().item())
    assert worst < TOL, worst   # 1e-4 per timestep


@pytest.mark.parametrize("name", ["ddpm_small_cond", "ddpm_small_variant"])
def test_sample_given_pocket_free_running(name):
    """conditional_model.py:478-555 end to end with the reference's noise tape."""
    c = Case(name)
    model = make_ddpm(c)
    model.set_noise_source(do.NoiseReplay(c.noise()))
    out_l, out_p, lm, pm = model.sample_given_pocket(c.pocket(), c.t("num_nodes_lig"),
                                                     timesteps=int(c.z["timesteps"]))
    ref_l, ref_p = c.t("out_lig"), c.t("out_pocket")
    assert out_l.shape == ref_l.shape and out_p.shape == ref_p.shape
    assert (out_l.cpu()[:, :3] - ref_l[:, :3]).abs().max().item() < 1e-3    # 20 free-running steps
    assert torch.equal(out_l.cpu()[:, 3:].long(), ref_l[:, 3:].long())
    assert (out_p.cpu() - ref_p).abs().max().item() < 1e-3
    assert torch.equal(lm.cpu(), c.t("lig_mask"))


def test_cond_inpaint_and_diversify_vs_golden():
    c = Case("ddpm_small_cond_inpaint")
    model = make_ddpm(c)
    model.set_noise_source(do.NoiseReplay(c.noise()))
    out_l, out_p, _, _ = model.inpaint(c.pocket("ligand_"), c.pocket(), c.t("lig_fixed"),
                                       resamplings=int(c.z["resamplings"]), timesteps=int(c.z["timesteps"]))
    assert (out_l.cpu()[:, :3] - c.t("out_lig")[:, :3]).abs().max().item() < 1e-3
    assert torch.equal(out_l.cpu()[:, 3:].long(), c.t("out_lig")[:, 3:].long())
    assert (out_p.cpu() - c.t("out_pocket")).abs().max().item() < 1e-3
    model.set_noise_source(do.NoiseReplay(c.noise("divnoise_", "n_draws_div")))
    d_l, d_p, _, _ = model.diversify(c.pocket("ligand_"), c.pocket(), int(c.z["div_steps"]))
    assert (d_l.cpu()[:, :3] - c.t("div_lig")[:, :3]).abs().max().item() < 1e-3
    assert torch.equal(d_l.cpu()[:, 3:].long(), c.t("div_lig")[:, 3:].long())


def test_fused_keyed_step_is_bitwise_the_separate_launches():
    """csrc/ddpm.h cond_step_keyed_kernel (one launch per reverse step: keyed noise evaluated in place + posterior update
    [+ RePaint iteration + q(z_t | z_s) jump] + the next call's time word) against the separate launches it replaces
    (dsbdd_randn_keyed x 1-3, dsbdd_cond_reverse_update, dsbdd_cond_repaint_update, fill): the same chains, the same
    seed -- torch.equal on everything returned, for sample_given_pocket, inpaint (resamplings 1 and 3, some atoms fixed)
    and diversify, with ragged ligand sizes; and the fused kernel against the ORACLE on its own draws."""
    c = Case("ddpm_small_cond_inpaint")
    outs = {}
    for fused in (True, False):
        model = make_ddpm(c)
        model.fused_step = fused
        res = []
        model.seed(77)
        res += list(model.sample_given_pocket(c.pocket(), c.pocket("ligand_")["size"], timesteps=12))
        for r in (1, 3):
            model.seed(78 + r)
            res += list(model.inpaint(c.pocket("ligand_"), c.pocket(), c.t("lig_fixed"), resamplings=r, timesteps=8))
        model.seed(90)
        res += list(model.diversify(c.pocket("ligand_"), c.pocket(), 5))
        torch.cuda.synchronize()
        outs[fused] = [t.clone() for t in res]
    assert len(outs[True]) == len(outs[False]) == 16
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)
    # the fused path against the oracle, the oracle drawing the same keyed noise (dsbdd_randn_keyed) draw by draw
    from tests.test_testset import _KeyedNoise
    model = make_ddpm(c)
    model.seed(5)
    sizes = c.pocket("ligand_")["size"]
    n = len(sizes)
    o_l, o_p, lm, pm = model.sample_given_pocket(c.pocket(), sizes, timesteps=6)
    om = do.OracleModel(c.state_dict(), c.cfg, c.cfg["atom_nf"], c.cfg["residue_nf"], c.ddpm["timesteps"],
                        c.ddpm["noise_schedule"], c.ddpm["noise_precision"], norm_values=c.ddpm["norm_values"], conditional=True)
    noise = _KeyedNoise(5, torch.arange(n), torch.repeat_interleave(torch.arange(n), sizes), dev())
    r_l, r_p, _, _ = do.cond_sample_given_pocket(om, c.pocket(), sizes, noise, timesteps=6)
    assert (o_l.cpu()[:, :3] - r_l[:, :3]).abs().max().item() < 1e-3
    assert torch.equal(o_l.cpu()[:, 3:].long(), r_l[:, 3:].long())


def test_folded_scans_are_bitwise_the_scan_kernels(monkeypatch):
    """Round 5: the exclusive scans between the two passes of the radius graph and of the level ordering are computed by
    the fill / place kernels themselves (integer wave sums over segment totals; csrc/level_list.h, level_place_kernel) instead of
    two single-workgroup launches.  DSBDD_FOLD_SCAN=0 selects the old launches: the edge lists, the level structures and
    every output must be IDENTICAL -- ragged batch with a sample without ligand atoms and one without pocket atoms,
    calls that return the pocket part (natural-order list) and ligand-only calls (level-ordered list), and a chain with
    a pocket frame (second list of block 0)."""
    cfg, _ = W.arch_cfg("small_cond")
    sd = W.random_state_dict(cfg, 4)
    xl, xp, t, ml, mp = _random_problem(cfg, [23, 0, 9, 40, 1], [36, 50, 0, 20, 44], seed=17)
    N = len(ml) + len(mp)
    c = Case("ddpm_small_cond")
    res = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("DSBDD_FOLD_SCAN", fold)
        m = make_dynamics(cfg, sd)
        f_l, f_p = m(*[v.to(dev()) for v in (xl, xp, t, ml, mp)])
        er, ec = m.engine().last_edges(N)
        slots = m.engine().edge_slots(N)
        tt = torch.full((1,), 0.4)
        e_l, _, st = m.forward_async(xl, xp, tt, ml, mp, want_pocket=False, batch=5)
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        lv = m.engine().last_levels(N)
        model = make_ddpm(c)
        model.frame_min_pocket_nodes = 1            # small pockets take the frame too: block 0's second list
        model.seed(3)
        chain = model.sample_given_pocket(c.pocket(), c.t("num_nodes_lig"), timesteps=5)
        res[fold] = ([f_l, f_p, er, ec, e_l, chain[0], chain[1]], slots, lv)
    a, b = res["1"], res["0"]
    assert a[1] == b[1]
    for u, v in zip(a[0], b[0]):
        assert torch.equal(u, v)
    for k in a[2]:
        assert np.array_equal(np.asarray(a[2][k]), np.asarray(b[2][k])), k


def test_joint_step_sample_and_inpaint_vs_golden():
    c = Case("ddpm_small_joint")
    model = make_ddpm(c)
    d = dev()
    noise = c.noise()
    lm, pm = c.t("lig_mask").to(d), c.t("pocket_mask").to(d)
    worst = 0.0
    worst = -1.0
    for i, g in enumerate(c.steps()):          # en_diffusion.py:503-557 per timestep
        model.set_noise_source(do.NoiseReplay(noise[3 + 3 * i: 6 + 3 * i]))
        zs, ps = model.sample_p_zs_given_zt(g["s"].to(d), g["t"].to(d), g["zt"].to(d), g["pt"].to(d), lm, pm)
        worst = max(worst, excess(zs, g["zs"]), excess(ps, g["ps"]))
    assert worst <= 0, worst   # atol 1e-4 (+ rtol 1e-5: |z| reaches ~650 here)
    model.set_noise_source(do.NoiseReplay(noise))
    out_l, out_p, _, _ = model.sample(len(c.t("num_nodes_lig")), c.t("num_nodes_lig"), c.t("num_nodes_pocket"),
                                      timesteps=int(c.z["timesteps"]))
    assert excess(out_l[:, :3], c.t("out_lig")[:, :3], atol=1e-3, rtol=1e-4) <= 0
    assert torch.equal(out_l.cpu()[:, 3:].long(), c.t("out_lig")[:, 3:].long())
    assert excess(out_p[:, :3], c.t("out_pocket")[:, :3], atol=1e-3, rtol=1e-4) <= 0
    # RePaint with the joint model (what generate_ligands does, lightning_modules.py:814-834)
    model.set_noise_source(do.NoiseReplay(c.noise("inpnoise_", "n_draws_inp")))
    n_lig = c.t("num_nodes_lig")
    lmask = torch.repeat_interleave(torch.arange(len(n_lig)), n_lig)
    ligand = {"x": torch.zeros(len(lmask), 3), "one_hot": torch.zeros(len(lmask), c.cfg["atom_nf"]),
              "size": n_lig, "mask": lmask}
    pocket = c.pocket("inp_pocket_")
    o_l, o_p, _, _ = model.inpaint(ligand, pocket, torch.zeros(len(lmask)), torch.ones(len(pocket["mask"])),
                                   resamplings=int(c.z["inp_resamplings"]), jump_length=1,
                                   timesteps=int(c.z["inp_timesteps"]))
    assert excess(o_l[:, :3], c.t("inp_out_lig")[:, :3], atol=1e-3, rtol=1e-4) <= 0
    assert torch.equal(o_l.cpu()[:, 3:].long(), c.t("inp_out_lig")[:, 3:].long())
    assert excess(o_p[:, :3], c.t("inp_out_pocket")[:, :3], atol=1e-3, rtol=1e-4) <= 0


# ---------------------------------------------------------------------------
# BASELINE-size properties (no oracle needed)
# ---------------------------------------------------------------------------
def _bench_problem(arch, B, n_lig=23):
    import os
    from tests._golden import GOLDEN_DIR
    z = np.load(os.path.join(GOLDEN_DIR, "pocket_3rfm.npz"))
    from diffsbdd_amd.pocket import prepare_pocket
    cfg, dd = W.arch_cfg(arch)
    key = "ca" if cfg["residue_nf"] == 20 else "fa"
    pocket = prepare_pocket(z[key + "_x"], z[key + "_types"], cfg["residue_nf"], repeats=B)
    return cfg, dd, pocket


def test_full_size_chain_properties():
    """crossdock_fullatom_cond, B=64 (BASELINE configs[2] shape), 5 reverse
    steps with the keyed generator: finite, ligand COM == 0 after every step
    (en_diffusion.py:925-930), pocket moved rigidly, one-hot output, and the
    result is independent of how the batch is sharded (B=64 == 2 x B=32)."""
    from diffsbdd_amd.conditional_model import ConditionalDDPM
    cfg, dd, pocket = _bench_problem("crossdock_fullatom_cond", 64)
    sd = W.random_state_dict(cfg, 0)

    def run(pk, n, offset):
        model = ConditionalDDPM(dynamics=make_dynamics(cfg, sd), atom_nf=10, residue_nf=10, n_dims=3,
                                size_histogram=np.ones((4, 8)), timesteps=dd["timesteps"],
                                noise_schedule=dd["noise_schedule"], noise_precision=dd["noise_precision"],
                                loss_type="l2", norm_values=dd["norm_values"]).to(dev())
        model.seed(1234, sample_offset=offset)
        pk = {k: v.clone() for k, v in pk.items()}
        return model.sample_given_pocket(pk, torch.full((n,), 23), timesteps=5)

    out_l, out_p, lm, pm = run(pocket, 64, 0)
    assert torch.isfinite(out_l).all() and torch.isfinite(out_p).all()
    assert out_l.shape == (64 * 23, 13) and out_p.shape == (64 * 286, 13)
    com = torch.zeros(64, 3, device=out_l.device).index_add_(0, lm, out_l[:, :3]) / 23
    assert com.abs().max().item() < 1e-3
    oh = out_l[:, 3:]
    assert torch.all((oh == 0) | (oh == 1)) and torch.all(oh.sum(1) == 1)
    # rigid pocket: pairwise distances inside sample 0 unchanged
    p0 = out_p[:286, :3].cpu()
    ref = torch.from_numpy(np.load(__import__("os").path.join(
        __import__("tests._golden", fromlist=["GOLDEN_DIR"]).GOLDEN_DIR, "pocket_3rfm.npz"))["fa_x"])
    # (exact pairwise distances: torch.cdist's matmul form is off by 2e-2 on un-centred PDB coordinates)
    assert (exact_pdist(p0) - exact_pdist(ref)).abs().max().item() < 1e-3
    # sharding invariance
    half = {k: v[: len(v) // 2] for k, v in pocket.items()}
    a_l, _, _, _ = run(half, 32, 0)
    b_l, _, _, _ = run(half, 32, 32)
    # bitwise: fixed summation order everywhere + keyed noise (identical for W = 1/2/4/8)
    both = torch.cat([a_l, b_l])
    assert torch.equal(both, out_l)
    again, _, _, _ = run(pocket, 64, 0)
    assert torch.equal(again, out_l)                           # and run-to-run


def test_keyed_noise_statistics_and_sharding():
    from diffsbdd_amd import _lib
    lib = _lib.load()
    d = dev()
    B, n = 16, 40
    mask = torch.repeat_interleave(torch.arange(B), n).to(d)
    out = torch.empty(B * n, 13, device=d)
    _lib.check(lib.dsbdd_randn_keyed(None, out.data_ptr(), mask.data_ptr(), B * n, 13, B, 0, None,
                                     C.c_uint64(7), C.c_uint64(3), 0))
    torch.cuda.synchronize()
    assert abs(out.mean().item()) < 0.05 and abs(out.std().item() - 1.0) < 0.05
    assert torch.isfinite(out).all()
    # second shard of 8 samples with offset 8 == rows of the full draw
    mask2 = torch.repeat_interleave(torch.arange(8), n).to(d)
    out2 = torch.empty(8 * n, 13, device=d)
    _lib.check(lib.dsbdd_randn_keyed(None, out2.data_ptr(), mask2.data_ptr(), 8 * n, 13, 8, 8, None,
                                     C.c_uint64(7), C.c_uint64(3), 0))
    torch.cuda.synchronize()
    assert torch.equal(out2, out[8 * n:])
    # a different draw index gives different numbers
    _lib.check(lib.dsbdd_randn_keyed(None, out2.data_ptr(), mask2.data_ptr(), 8 * n, 13, 8, 8, None,
                                     C.c_uint64(7), C.c_uint64(4), 0))
    torch.cuda.synchronize()
    assert not torch.equal(out2, out[8 * n:])
    # explicit global ids: samples 15, 3, 8 of the full draw, packed in that order
    ids = torch.tensor([15, 3, 8], device=d)
    mask3 = torch.repeat_interleave(torch.arange(3), n).to(d)
    out3 = torch.empty(3 * n, 13, device=d)
    _lib.check(lib.dsbdd_randn_keyed(None, out3.data_ptr(), mask3.data_ptr(), 3 * n, 13, 3, 0, ids.data_ptr(),
                                     C.c_uint64(7), C.c_uint64(3), 0))
    torch.cuda.synchronize()
    assert torch.equal(out3, torch.cat([out[15 * n:16 * n], out[3 * n:4 * n], out[8 * n:9 * n]]))


def test_bench_two_ranks_sharing_the_gpu():
    """The N > 1 path of bench.py end to end (`python bench.py --gpus 2`, self-launched ranks, per-rank
    sample offsets, gather of the finished ligands, max-over-ranks timing) with two
    ranks on the one available GPU over gloo (RCCL refuses two ranks on one device)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    # the bare command: bench.py starts its own ranks (self_launch) when WORLD_SIZE is unset
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"),
           "--gpus", "2", "--steps", "1", "--warmup", "0", "--timesteps", "3", "--batch", "4",
           "--backend", "gloo", "--share-gpu", "--no-cpu-baseline"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout            # rank 0 prints exactly one JSON line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["global_batch"] == 8
    assert d["rccl_ranks"] == 2 and d["backend"] == "gloo"
    assert d["value"] > 0 and d["unit"] == "ligands/s" and d["cpu_baseline"] is None


def test_bench_plain_run_times_the_headline_only_full_adds_the_legs():
    """A plain `bench.py` run times the warm-up and --steps chains and nothing else: every leg that takes runs of its own
    (other_states, emulated, cpu_baseline, other_workloads) is null.  `--full` runs them."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
            "--timesteps", "3", "--batch", "4"]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--other-steps", "1",
                                                 "--emulated-steps", "1"])):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-2000:]
        js = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(js) == 1, out.stdout
        lines[name] = json.loads(js[0])
    plain, full = lines["plain"], lines["full"]
    for d in (plain, full):
        assert d["value"] > 0 and d["steps"] == 1 and d["warmup"] == 1 and d["dtype"] == "f32"
        assert d["roofline"]["timed_launches"] > 0
    assert plain["other_states"] is None and plain["emulated"] is None
    assert plain["cpu_baseline"] is None and plain["other_workloads"] is None
    assert full["other_states"]["value"] > 0 and full["emulated"]["value"] > 0


def test_bench_four_ranks_config3_per_rank_shape_equals_sequential_runs(tmp_path):
    """The multi-rank path of bench.py as the driver launches it -- `python -m torch.distributed.run --nproc-per-node W
    bench.py --gpus W` -- with BASELINE configs[3]'s 64 pockets per rank, W = 4 ranks sharing the one GPU of this box over
    gloo (RCCL refuses several ranks per device; the one-rank RCCL path is tests/test_gpu_rccl.py).  Four ranks, not
    configs[3]'s eight: this process, the launcher and the ranks all hold the device, and a shared GPU host admits at
    most six such processes at once.  The JSON line reports 4 ranks and the sample offsets 0, 64, 128, 192; the gathered
    256 x 23 rows are BITWISE those of four sequential world-1 chains (one per shard, same seed, offset = the shard's
    first global sample id)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    import bench
    W, B = 4, 64
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dump = str(tmp_path / "lig4.npz")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    T = 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(W), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", str(W), "--steps", "1",
           "--warmup", "0", "--timesteps", str(T), "--backend", "gloo", "--share-gpu", "--no-cpu-baseline",
           "--no-kernel-timing", "--dump-ligands", dump]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == W and d["rccl_ranks"] == W and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == W * B and d["config"]["batch_per_gpu"] == B
    assert d["rank_sample_offsets"] == [B * r for r in range(W)]
    z = np.load(dump)
    assert z["all_lig"].shape == (W * B * 23, 13) and z["all_mask"].shape == (W * B * 23,)
    assert np.array_equal(z["all_mask"], np.repeat(np.arange(W * B), 23))
    # W sequential world-1 chains in this process: bench.py's own protocol (chain(200): seed 200, anchored states)
    d0 = dev()
    cfg, dd, model = bench.build_model("crossdock_fullatom_cond", d0)
    rows = []
    for r in range(W):
        model.seed(200, sample_offset=B * r)
        pocket = bench.load_pocket("fa", B, d0)
        ligand = bench.anchor_ligand(B, 23, cfg["atom_nf"], d0)
        o_l, _, lmask, _ = model.inpaint(ligand, pocket, torch.ones(B * 23, device=d0), resamplings=1, timesteps=T)
        rows.append(o_l.cpu())
    seq = torch.cat(rows).numpy()
    assert np.array_equal(seq, z["all_lig"])                                         # bitwise


# ---------------------------------------------------------------------------
# edge cases beyond the goldens (oracle computed on the spot)
# ---------------------------------------------------------------------------
def _random_problem(cfg, n_lig, n_poc, seed, lig_shift=None, spread=3.0):
    g = torch.Generator().manual_seed(seed)
    B = len(n_lig)
    ml = torch.repeat_interleave(torch.arange(B), torch.tensor(n_lig))
    mp = torch.repeat_interleave(torch.arange(B), torch.tensor(n_poc))
    xl = torch.randn(len(ml), 3, generator=g) * spread
    if lig_shift is not None:
        xl = xl + torch.tensor(lig_shift)[ml]
    xp = torch.randn(len(mp), 3, generator=g) * 6.0
    hl = torch.randn(len(ml), cfg["atom_nf"], generator=g)
    hp = torch.randn(len(mp), cfg["residue_nf"], generator=g)
    t = torch.rand(B, 1, generator=g)
    return torch.cat([xl, hl], 1), torch.cat([xp, hp], 1), t, ml, mp


@pytest.mark.parametrize("granule", ["32", "16", "sk"])
@pytest.mark.parametrize("arch,max_wg", [("small_cond", 0), ("small_variant", 0), ("small_joint", 0),
                                         ("small_cond", 8), ("small_variant", 8), ("small_joint", 8),
                                         ("crossdock_ca_cond", 0), ("crossdock_ca_cond", 8), ("crossdock_fullatom_cond", 16)])
def test_rows_spanning_many_tiles(arch, max_wg, granule, monkeypatch):
    """A 150-atom ligand: fully connected ligand rows have degree > 150, so one
    row's edge segment spans 5+ wave tiles / 2+ workgroup tiles.  granule "16": every stage on the 16-edge-granule
    kernels (csrc/edge_wave16.h: a row then spans 10+ wave tiles; head slots per 16-edge tile).  granule "sk": every
    stage on the split-K kernels (csrc/edge_splitk.h, H = 256: a workgroup per 32-edge tile; with the grid capped at 8 / 16
    workgroups every workgroup walks many items, both MLPs of the coordinate stage as separate populations).  The split-K
    kernels serve hidden_nf 256 only: for the other architectures the engine ignores the mask, and the result must be
    bitwise that of the same call without it."""
    import os
    if granule == "16":
        monkeypatch.setenv("DSBDD_GRANULE16", "0xFFFFFFFF")
    if granule == "sk":
        monkeypatch.setenv("DSBDD_SPLITK", "0xFFFFFFFF")
    cfg, _ = W.arch_cfg(arch)
    sd = W.random_state_dict(cfg, 3)
    xl, xp, t, ml, mp = _random_problem(cfg, [150, 3, 40], [40, 30, 5], seed=11,
                                        spread=0.5 if arch == "small_joint" else 3.0)
    o_l, o_p, edges = eo.dynamics_forward(sd, cfg, xl, xp, t, ml, mp)
    os.environ["DSBDD_EDGE_MAX_WG"] = str(max_wg)
    try:
        m = make_dynamics(cfg, sd)
        e_l, e_p, st = m.forward_async(xl, xp, t, ml, mp, edges=edges)
        e_l2, e_p2, _ = m.forward_async(xl, xp, t, ml, mp, edges=edges)
        assert torch.equal(e_l, e_l2) and torch.equal(e_p, e_p2)                            # each variant bitwise reproducible
        f_l, f_p = m(xl.to(dev()), xp.to(dev()), t.to(dev()), ml.to(dev()), mp.to(dev()))   # device-built edges
        if granule == "sk" and cfg["hidden_nf"] != 256:
            monkeypatch.delenv("DSBDD_SPLITK")
            n_l, n_p, _ = make_dynamics(cfg, sd).forward_async(xl, xp, t, ml, mp, edges=edges)
            assert torch.equal(e_l, n_l) and torch.equal(e_p, n_p)                          # the mask is ignored
    finally:
        del os.environ["DSBDD_EDGE_MAX_WG"]
    assert int(st.item()) == 0
    assert excess(e_l, o_l) <= 0 and excess(e_p, o_p) <= 0
    er, ec = m.engine().last_edges(len(ml) + len(mp))
    if er.numel() == edges.shape[1] and torch.equal(er, edges[0]) and torch.equal(ec, edges[1]):
        assert excess(f_l, o_l) <= 0 and excess(f_p, o_p) <= 0


@pytest.mark.parametrize("arch", ["small_cond", "small_joint", "crossdock_ca_cond", "crossdock_fullatom_cond"])
def test_edge_granule_variants_agree(arch, monkeypatch):
    """The 16-edge-granule kernels (csrc/edge_wave16.h) and -- H = 256 -- the split-K kernels (csrc/edge_splitk.h) against
    the 32-edge ones on the same call: another k grouping inside the fp32 MFMA chains (split-K: four partial sums over a
    quarter of k each) and another summation tree of the row sums -- rounding only (2e-5 stated, ~1e-6 measured); the
    ligand-output-only call (level-ordered list, head slots at list offsets) included."""
    cfg, _ = W.arch_cfg(arch)
    sd = W.random_state_dict(cfg, 2)
    xl, xp, t, ml, mp = _random_problem(cfg, [23, 9, 40, 1], [36, 50, 20, 44], seed=17,
                                        spread=0.5 if arch == "small_joint" else 3.0)
    out = {}
    variants = ("32", "16", "sk") if cfg["hidden_nf"] == 256 else ("32", "16")
    for granule in variants:
        monkeypatch.delenv("DSBDD_GRANULE16", raising=False)
        monkeypatch.delenv("DSBDD_SPLITK", raising=False)
        if granule == "16":
            monkeypatch.setenv("DSBDD_GRANULE16", "0xFFFFFFFF")
        elif granule == "sk":
            monkeypatch.setenv("DSBDD_SPLITK", "0xFFFFFFFF")
        m = make_dynamics(cfg, sd)
        a = m.forward_async(xl, xp, t, ml, mp)
        b = m.forward_async(xl, xp, t[:1], ml, mp, want_pocket=False) if not cfg["update_pocket_coords"] else a
        torch.cuda.synchronize()
        assert int(a[2].item()) == 0 and int(b[2].item()) == 0
        out[granule] = (a[0].clone(), a[1].clone(), b[0].clone())
    for other in variants[1:]:
        for u, v in zip(out["32"], out[other]):
            assert (u - v).abs().max().item() < 2e-5 * max(1.0, v.abs().max().item()), other
        # (the variant really switched -- except under the emulated path of the DSBDD_EMU gate run, where the engine ignores
        # both masks by design: every edge stage then runs the emulated 32-edge kernel, include/diffsbdd_hip.h DSBDD_OPT_EMU)
        import os
        if os.environ.get("DSBDD_EMU", "0") in ("", "0"):
            assert not torch.equal(out["32"][0], out[other][0]) or arch == "small_joint"
        else:
            assert torch.equal(out["32"][0], out[other][0])


def test_ligand_without_pocket_neighbours_and_batch_of_one():
    """No interaction edges at all (ligand 100 A away): the active-node list is
    the ligand alone; and a single sample with a single t (dynamics.py:105-107)."""
    cfg, _ = W.arch_cfg("small_cond")
    sd = W.random_state_dict(cfg, 5)
    xl, xp, t, ml, mp = _random_problem(cfg, [6], [25], seed=2, lig_shift=[[100.0, 0.0, 0.0]])
    t1 = t.reshape(1, 1)
    o_l, o_p, edges = eo.dynamics_forward(sd, cfg, xl, xp, t1, ml, mp)
    assert int(((edges[0] < 6) & (edges[1] >= 6)).sum()) == 0
    m = make_dynamics(cfg, sd)
    f_l, f_p = m(xl.to(dev()), xp.to(dev()), t1.to(dev()), ml.to(dev()), mp.to(dev()))
    assert excess(f_l, o_l) <= 0 and excess(f_p, o_p) <= 0
    assert f_p[:, :3].abs().max().item() == 0.0          # pocket coordinates are not updated


def test_joint_full_width_inpaint_runs_at_scale():
    """moad_fullatom_joint (H = 192, edge-type embedding, pocket coordinates updated):
    RePaint with resamplings = 2 as BASELINE configs[4] uses it, 8 pockets, 3 steps:
    finite, COM-free, one-hot, fixed pocket returned unchanged up to the rigid shift."""
    from diffsbdd_amd.en_diffusion import EnVariationalDiffusion
    cfg, dd = W.arch_cfg("moad_fullatom_joint")
    sd = W.random_state_dict(cfg, 0)
    model = EnVariationalDiffusion(dynamics=make_dynamics(cfg, sd), atom_nf=10, residue_nf=10, n_dims=3,
                                   size_histogram=np.ones((4, 8)), timesteps=dd["timesteps"],
                                   noise_schedule=dd["noise_schedule"], noise_precision=dd["noise_precision"],
                                   loss_type="l2", norm_values=dd["norm_values"]).to(dev())
    _, _, pocket = _bench_problem("crossdock_fullatom_cond", 8)
    B, nl = 8, 23
    lmask = torch.repeat_interleave(torch.arange(B), nl)
    ligand = {"x": torch.zeros(B * nl, 3), "one_hot": torch.zeros(B * nl, 10),
              "size": torch.full((B,), nl), "mask": lmask}
    model.seed(7)
    out_l, out_p, lm, pm = model.inpaint(ligand, pocket, torch.zeros(B * nl), torch.ones(len(pocket["mask"])),
                                         resamplings=2, jump_length=1, timesteps=3)
    assert out_l.shape == (B * nl, 13) and out_p.shape == (B * 286, 13)
    assert torch.isfinite(out_l).all() and torch.isfinite(out_p).all()
    oh = out_l[:, 3:]
    assert torch.all((oh == 0) | (oh == 1)) and torch.all(oh.sum(1) == 1)
    com = torch.zeros(B, 3, device=out_l.device).index_add_(0, torch.cat([lm, pm]), torch.cat([out_l[:, :3], out_p[:, :3]]))
    assert (com / (nl + 286)).abs().max().item() < 5e-2
    # sharding invariance of the RePaint chain, bitwise: samples 4..7 as their own batch with offset 4
    _, _, pocket4 = _bench_problem("crossdock_fullatom_cond", 4)
    lmask4 = torch.repeat_interleave(torch.arange(4), nl)
    ligand4 = {"x": torch.zeros(4 * nl, 3), "one_hot": torch.zeros(4 * nl, 10), "size": torch.full((4,), nl),
               "mask": lmask4}
    model.seed(7, sample_offset=4)
    h_l, h_p, _, _ = model.inpaint(ligand4, pocket4, torch.zeros(4 * nl), torch.ones(len(pocket4["mask"])),
                                   resamplings=2, jump_length=1, timesteps=3)
    assert torch.equal(h_l, out_l[4 * nl:]) and torch.equal(h_p, out_p[4 * 286:])


def test_eager_calls_between_graph_replays():
    """Timed (eager) calls interleaved with replays of the captured graph must not disturb each
    other: with hipMemsetAsync inside the call sequence the zero fills lost their ordering against
    graph launches on the same stream (chains blew up after a few hundred mixed calls); the engine
    now zero-fills with its own kernel.  Same inputs 90 times, every 3rd call eager + timed."""
    c = Case("dyn_fullatom_cond")
    m = make_dynamics(c.cfg, c.state_dict())
    d = dev()
    args = [c.t(k).to(d) for k in ("xh_lig", "xh_pocket", "t", "mask_lig", "mask_pocket")]
    B = int(args[3].max().item()) + 1
    eps = torch.empty_like(args[0])
    eps_p = torch.empty_like(args[1])
    status = torch.zeros(1, dtype=torch.int32, device=d)
    eng = m.engine()
    first, worst = None, 0.0
    eng.profile(3, max_launches=4096)
    try:
        for i in range(90):
            m.forward_async(*args, status=status, batch=B, eps_lig=eps, eps_pocket=eps_p)
            out = eps.clone()
            if first is None:
                first = out
            worst = max(worst, (out - first).abs().max().item())
    finally:
        ms, n = eng.profile_read()
        eng.profile(0, 0)
    replays, captures, eager = eng.graph_stats()
    assert replays >= 50 and captures >= 1 and eager >= 30, (replays, captures, eager)
    assert n == 30 * c.cfg["n_layers"] * c.cfg["inv_sublayers"] and ms > 0
    assert int(status.item()) == 0
    assert worst < 1e-5, worst
    assert (first.cpu() - c.t("eps_lig")).abs().max().item() < TOL


def test_unsorted_masks_raise_and_manual_seed_controls_noise():
    """Masks must be sorted (the kernels find a sample's rows by binary search): an unsorted mask is
    reported at the end of the call instead of silently sampling wrong segments.  Without an explicit
    seed() the keyed generator takes its key from torch's global RNG: torch.manual_seed reproduces a
    chain, different seeds give different ligands."""
    c = Case("ddpm_small_cond")
    model = make_ddpm(c)
    n_lig = c.t("num_nodes_lig")

    def run():
        return model.sample_given_pocket(c.pocket(), n_lig, timesteps=4)[0]

    torch.manual_seed(11)
    a = run()
    model._seed, model._draw = None, 0
    torch.manual_seed(11)
    b = run()
    model._seed, model._draw = None, 0
    torch.manual_seed(12)
    d = run()
    assert torch.equal(a, b) and (a[:, :3] - d[:, :3]).abs().max().item() > 1e-2
    bad = c.pocket()
    bad["mask"] = bad["mask"].flip(0)
    with pytest.raises(ValueError, match="sorted"):
        model.sample_given_pocket(bad, n_lig, timesteps=2)


@pytest.mark.parametrize("name", ["loss_small_cond_eval", "loss_small_cond_train", "loss_small_joint_eval",
                                  "loss_small_joint_train"])
def test_loss_terms_vs_oracle_and_reference_golden(name):
    """SURVEY.md 8f-3 (evaluation half): `forward()` -- the 12 loss terms of conditional_model.py:202-330 /
    en_diffusion.py:336-469 -- with the network passes on the HIP kernels, against the oracle on the same
    t_int / noise (1e-4 relative to each term's scale) and against the values the real reference returned."""
    from tests.test_oracle_golden import LOSS_NAMES, loss_inputs
    c = Case(name)
    cfg, dd = c.cfg, c.ddpm
    training = bool(int(c.z["training"]))
    model = make_ddpm(c)
    model.size_distribution = type(model.size_distribution)(np.ones((12, 60)))      # the golden's histogram
    model.train(training)
    model.set_noise_source(do.NoiseReplay(c.noise()))
    model.t_int_source = lambda b: c.t("t_int")
    ligand, pocket = loss_inputs(c)
    with torch.no_grad():
        out = model(ligand, pocket, return_info=True)
    terms, info = out[:12], out[12]
    om = do.OracleModel(c.state_dict(), cfg, cfg["atom_nf"], cfg["residue_nf"], dd["timesteps"], dd["noise_schedule"],
                        dd["noise_precision"], norm_values=dd["norm_values"], conditional=dd["conditional"])
    ligand, pocket = loss_inputs(c)
    ref = do.loss_terms(om, ligand, pocket, c.t("t_int"), do.NoiseReplay(c.noise()), training)
    for nme, v, r in zip(LOSS_NAMES, terms, ref):
        v = torch.as_tensor(v).float().cpu()
        gold = c.t("out_" + nme)
        assert v.shape == gold.shape, (nme, v.shape, gold.shape)
        scale = max(1.0, gold.abs().max().item())
        if r is not None:
            assert (v - torch.as_tensor(r).float()).abs().max().item() <= 1e-4 * scale, (name, nme)   # vs oracle
        # vs the reference's own numbers (its radius graph uses torch.cdist: an edge at the cutoff may differ)
        assert (v - gold).abs().max().item() <= 5e-3 * scale, (name, nme, (v - gold).abs().max().item())
    for k, v in info.items():
        assert abs(float(v) - float(c.t("info_" + k))) <= 5e-3 * max(1.0, abs(float(c.t("info_" + k)))), k


def _trainable_terms(terms):
    """The terms of the 12-tuple that depend on the network (error_t_lig, error_t_pocket, loss_0_x_ligand,
    loss_0_x_pocket, loss_0_h), reduced like the l2 objective of lightning_modules.py:262-275 up to constant factors."""
    return sum(torch.as_tensor(terms[i]).float().mean() for i in (1, 2, 4, 5, 6))


@pytest.mark.parametrize("name", ["loss_small_cond_train", "loss_small_joint_train"])
def test_training_step_gradients_vs_oracle_autograd(name):
    """SURVEY.md 8f-3, backward half: in training mode with autograd recording, `forward()` returns loss terms that
    carry their graph (diffsbdd_amd/train_path.py) -- `loss.backward()` fills every parameter's .grad.  Against the
    oracle differentiated by autograd on the CPU (same t_int, same noise): loss terms 1e-4, every parameter gradient
    1e-4 relative to that gradient's largest entry.  Then three optimiser steps on the fixed batch lower the loss
    (what `training_step` + AdamW do, lightning_modules.py:184,337-363)."""
    from tests.test_oracle_golden import loss_inputs
    c = Case(name)
    cfg, dd = c.cfg, c.ddpm
    model = make_ddpm(c)
    model.size_distribution = type(model.size_distribution)(np.ones((12, 60)))
    model.train(True)
    model.set_noise_source(do.NoiseReplay(c.noise()))
    model.t_int_source = lambda b: c.t("t_int")
    terms = model(*loss_inputs(c))
    loss = _trainable_terms(terms)
    assert loss.requires_grad
    loss.backward()
    # the oracle, differentiated
    sd = {k: v.clone().requires_grad_(True) for k, v in c.state_dict().items()}
    om = do.OracleModel(sd, cfg, cfg["atom_nf"], cfg["residue_nf"], dd["timesteps"], dd["noise_schedule"],
                        dd["noise_precision"], norm_values=dd["norm_values"], conditional=dd["conditional"])
    ref = do.loss_terms(om, *loss_inputs(c), c.t("t_int"), do.NoiseReplay(c.noise()), True)
    ref_loss = _trainable_terms(ref)
    assert abs(loss.item() - ref_loss.item()) <= 1e-4 * max(1.0, abs(ref_loss.item()))
    ref_loss.backward()
    n_checked = 0
    for pname, p in model.dynamics.named_parameters():
        g_ref = sd[pname].grad
        if pname.endswith("coord_mlp.4.weight"):                 # one Parameter shared by both coordinate MLPs
            twin = pname.replace("coord_mlp", "cross_product_mlp")
            if twin in sd and sd[twin].grad is not None:
                g_ref = g_ref + sd[twin].grad
        if p.grad is None and g_ref is None:                      # (the conditional loss never reads the pocket decoder)
            continue
        assert p.grad is not None and g_ref is not None, pname
        scale = max(g_ref.abs().max().item(), 1e-6)
        err = (p.grad.cpu() - g_ref).abs().max().item()
        assert err <= 1e-4 * scale + 1e-7, (pname, err, scale)
        n_checked += 1
    assert n_checked >= 40
    # a few optimiser steps on the same batch
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, amsgrad=True, weight_decay=1e-12)
    losses = []
    for _ in range(4):
        model.set_noise_source(do.NoiseReplay(c.noise()))
        opt.zero_grad()
        l = _trainable_terms(model(*loss_inputs(c)))
        l.backward()
        opt.step()
        losses.append(l.item())
    assert losses[-1] < losses[0], losses
    # evaluation on the updated parameters runs on the HIP kernels again (the engine repacks its weights)
    # (the optimiser's in-place updates are noticed: the HIP evaluation packs the new weights.)  Same t_int and noise
    # as the training passes, evaluated under no_grad in training mode = the fused kernels on the updated parameters
    model.set_noise_source(do.NoiseReplay(c.noise()))
    with torch.no_grad():
        ev = _trainable_terms(model(*loss_inputs(c))).item()
    model.set_noise_source(do.NoiseReplay(c.noise()))
    chk = _trainable_terms(model(*loss_inputs(c))).item()        # autograd path, same parameters
    assert abs(ev - chk) <= 1e-4 * max(1.0, abs(chk)), (ev, chk)
    assert ev < losses[0]


def _replay(c, prefix):
    n = int(c.z["n_" + prefix])
    return do.NoiseReplay([torch.from_numpy(c.z[f"{prefix}_{i}"]) for i in range(n)])


def _dict(c, prefix):
    return {k: c.t(prefix + k) for k in ("x", "one_hot", "size", "mask")}


def test_cond_api_variants_vs_reference_golden():
    """Reference-generated vectors (tests/golden/make_golden_variants.py) for the conditional API variants:
    chain frames (return_frames = timesteps, conditional_model.py:518-555), RePaint centred at the pocket with
    frames (:557-686, center='pocket'), and SimpleConditionalDDPM (:702-746: no COM projection)."""
    from diffsbdd_amd.conditional_model import SimpleConditionalDDPM
    c = Case("ddpm_variants_cond")
    T = int(c.z["timesteps"])
    model = make_ddpm(c)
    model.set_noise_source(_replay(c, "fnoise"))
    fl, fp, _, _ = model.sample_given_pocket(_dict(c, "pocket_"), c.t("num_nodes_lig"), return_frames=T, timesteps=T)
    assert fl.shape == c.t("frames_lig").shape and fp.shape == c.t("frames_pocket").shape
    assert excess(fl[..., :3], c.t("frames_lig")[..., :3], atol=1e-3, rtol=1e-4) <= 0         # 4 free-running steps
    assert excess(fp[..., :3], c.t("frames_pocket")[..., :3], atol=1e-3, rtol=1e-4) <= 0
    assert torch.equal(fl[0].cpu()[:, 3:].long(), c.t("frames_lig")[0][:, 3:].long())        # final frame: one-hot
    assert excess(fl[1:, :, 3:], c.t("frames_lig")[1:, :, 3:], atol=1e-3, rtol=1e-4) <= 0     # intermediate z_h
    model.set_noise_source(_replay(c, "pnoise"))
    pl, pp, _, _ = model.inpaint(_dict(c, "ligand_"), _dict(c, "pocket_"), c.t("lig_fixed"), resamplings=2,
                                 return_frames=T, timesteps=T, center="pocket")
    assert excess(pl[..., :3], c.t("pocketc_lig")[..., :3], atol=1e-3, rtol=1e-4) <= 0
    assert excess(pp[..., :3], c.t("pocketc_pocket")[..., :3], atol=1e-3, rtol=1e-4) <= 0
    assert torch.equal(pl[0].cpu()[:, 3:].long(), c.t("pocketc_lig")[0][:, 3:].long())
    cfg, dd = c.cfg, c.ddpm
    simple = SimpleConditionalDDPM(dynamics=make_dynamics(cfg, c.state_dict()), atom_nf=cfg["atom_nf"],
                                   residue_nf=cfg["residue_nf"], n_dims=3, size_histogram=np.ones((4, 8)),
                                   timesteps=dd["timesteps"], noise_schedule=dd["noise_schedule"],
                                   noise_precision=dd["noise_precision"], loss_type="l2",
                                   norm_values=dd["norm_values"]).to(dev())
    simple.set_noise_source(_replay(c, "snoise"))
    sl, sp, _, _ = simple.sample_given_pocket(_dict(c, "pocket_"), c.t("num_nodes_lig"), timesteps=T)
    assert excess(sl[:, :3], c.t("simple_lig")[:, :3], atol=1e-3, rtol=1e-4) <= 0
    assert torch.equal(sl.cpu()[:, 3:].long(), c.t("simple_lig")[:, 3:].long())
    assert excess(sp[:, :3], c.t("simple_pocket")[:, :3], atol=1e-3, rtol=1e-4) <= 0


def test_joint_api_variants_vs_reference_golden():
    """Joint model: chain frames of sample() (en_diffusion.py:618-651) and RePaint with jump_length = 2,
    resamplings = 2, some ligand atoms and one sample's pocket fixed (en_diffusion.py:676-837)."""
    c = Case("ddpm_variants_joint")
    model = make_ddpm(c)
    T = int(c.z["timesteps"])
    model.set_noise_source(_replay(c, "fnoise"))
    fl, fp, _, _ = model.sample(2, c.t("num_nodes_lig"), c.t("num_nodes_pocket"), return_frames=T, timesteps=T)
    assert fl.shape == c.t("frames_lig").shape
    assert excess(fl[..., :3], c.t("frames_lig")[..., :3], atol=1e-3, rtol=1e-4) <= 0
    assert excess(fp[..., :3], c.t("frames_pocket")[..., :3], atol=1e-3, rtol=1e-4) <= 0
    assert torch.equal(fl[0].cpu()[:, 3:].long(), c.t("frames_lig")[0][:, 3:].long())
    model.set_noise_source(_replay(c, "jnoise"))
    jl, jp, _, _ = model.inpaint(_dict(c, "ligand_"), _dict(c, "inp_pocket_"), c.t("lig_fixed"), c.t("pocket_fixed"),
                                 resamplings=2, jump_length=2, timesteps=int(c.z["jump_timesteps"]))
    assert excess(jl[:, :3], c.t("jump_lig")[:, :3], atol=1e-3, rtol=1e-4) <= 0
    assert torch.equal(jl.cpu()[:, 3:].long(), c.t("jump_lig")[:, 3:].long())
    assert excess(jp[:, :3], c.t("jump_pocket")[:, :3], atol=1e-3, rtol=1e-4) <= 0
    assert torch.equal(jp.cpu()[:, 3:].long(), c.t("jump_pocket")[:, 3:].long())


@pytest.mark.parametrize("want_pocket", [True, False])
def test_edge_capacity_overflow_is_flagged_not_fatal(want_pocket):
    """A caller-supplied edge bound that is too small (the engine sizes its lists from it) must end in the
    overflow status bit -- no index past the lists' capacity in any kernel, including the level-ordering kernels of
    the ligand-output-only path -- and the next call with a proper bound must be unaffected."""
    from diffsbdd_amd import _lib
    from diffsbdd_amd.engine import edge_capacity
    c = Case("dyn_fullatom_cond")
    m = make_dynamics(c.cfg, c.state_dict())
    d = dev()
    args = [c.t(k).to(d) for k in ("xh_lig", "xh_pocket", "t", "mask_lig", "mask_pocket")]
    B = int(args[3].max().item()) + 1
    good = edge_capacity(args[3], args[4], B)
    ok = m.forward_async(*args, batch=B, edge_cap=good, want_pocket=want_pocket)
    torch.cuda.synchronize()
    assert int(ok[2].item()) == 0
    # the engine must not depend on what its workspace held before: fill it with garbage first (torch's caching
    # allocator hands out used memory; stale list entries once sent the edge kernels to wild addresses here)
    m3 = make_dynamics(c.cfg, c.state_dict())
    m3.engine().ensure_workspace(args[0].shape[0], args[1].shape[0], B, good)
    m3.engine().workspace.random_(0, 256)
    ok3 = m3.forward_async(*args, batch=B, edge_cap=good, want_pocket=want_pocket)
    torch.cuda.synchronize()
    assert int(ok3[2].item()) == 0 and torch.equal(ok3[0], ok[0])
    m2 = make_dynamics(c.cfg, c.state_dict())
    m2.engine().ensure_workspace(args[0].shape[0], args[1].shape[0], B, 256)
    m2.engine().workspace.random_(0, 256)
    bad = m2.forward_async(*args, batch=B, edge_cap=256, want_pocket=want_pocket)
    torch.cuda.synchronize()
    assert int(bad[2].item()) & _lib.STATUS_EDGE_OVERFLOW
    again = m2.forward_async(*args, batch=B, edge_cap=good, want_pocket=want_pocket)
    torch.cuda.synchronize()
    assert int(again[2].item()) == 0 and torch.equal(again[0], ok[0])
