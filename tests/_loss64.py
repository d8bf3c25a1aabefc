"""Plain torch restatements of the loss-head entry points of include/diffsbdd_hip.h (dsbdd_loss_cond_pre / _post and
dsbdd_loss_joint_pre / _post), written from the header's contract and the reference's formulas -- not from
csrc/loss_head.h and not from the package's torch mirror -- for tests/test_loss_restatement.py (which pins them to
oracle/ddpm_oracle.py on the CPU) and tests/test_gpu_loss_head_kernels.py.  No GPU code.

Every function takes a dtype: float64 is the reference, float32 the yardstick (`err_ref` of tests/_steps64.py: within).
Citations are <file of the reference's equivariant_diffusion/>:<line>, as in oracle/ddpm_oracle.py.

Conventions
  lsz, psz      ligand / pocket rows of each sample (the masks are repeat_interleave(arange(B), sizes))
  cfg           dict: T, gamma (the schedule's table gamma[0..T]), nv0, nv1, nb1 (norm_value_x, norm_value_h, norm_bias_h),
                remove_com, vnode_idx (-1: none), logpn ([n1_tab][n2_tab] tensor or None)
  per_sample    dict of [B] tensors named as the header names the rows (PS_ROWS, in the header's order)
The backward entry points have no restatement: their reference is torch.autograd.grad through cond_post / joint_post
(post_backward below), an absent cotangent being a zero one.
"""
import math

import torch

from tests._steps64 import ULP4, offsets, within  # noqa: F401  (within: re-exported for the two test files)

PS_ROWS = ("t", "gamma_t", "gamma_s", "alpha_t", "sigma_t", "SNR_weight", "neg_log_constants", "kl_prior", "loss_0_h",
           "log_pN", "delta_log_px", "t_is_zero")
COND_OUT_ROWS = ("error_t", "loss_0_x", "info_x", "info_h")
JOINT_OUT_ROWS = ("error_t_lig", "error_t_pocket", "loss_0_x_ligand", "loss_0_x_pocket", "info_lig_x", "info_lig_h",
                  "info_pocket_x", "info_pocket_h")


def within_at(name, hip, ref64, ref32, mag):
    """`within` of tests/_steps64.py with the magnitude given by the caller.  Two quantities only: kl_prior (mag = the
    largest addend of gaussian_KL, whose addends cancel) and neg_log_constants (its own magnitude)."""
    hip, ref64, ref32 = (torch.as_tensor(v).detach().cpu().double().reshape(-1) for v in (hip, ref64, ref32))
    if ref64.numel() == 0:
        assert hip.numel() == 0
        return 0.0, 0.0
    mag = max(float(mag), 1e-30)
    err_ref = float((ref32 - ref64).abs().max()) / mag
    err = float((hip - ref64).abs().max()) / mag
    bound = max(2 * err_ref, ULP4)
    print(f"  {name}: err_ref {err_ref:.3e}  hip {err:.3e}  bound {bound:.3e}  (magnitude {mag:.3e})")
    assert torch.isfinite(hip).all(), name
    assert err <= bound and err <= 1e-4, (name, err, bound)
    return err_ref, err


# ---- pieces -----------------------------------------------------------------------------------------------------------------
def mask_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor([int(s) for s in sizes], dtype=torch.int64))


def seg_sum(x, mask, B):
    """sum_except_batch, en_diffusion.py:944-946: all trailing axes, then the rows of each sample."""
    rows = x.sum(dim=tuple(range(1, x.dim()))) if x.dim() > 1 else x
    return torch.zeros(B, dtype=x.dtype).index_add_(0, mask, rows)


def seg_mean3(x, mask, B, count):
    """scatter_mean of a [n][3] block; an empty sample has mean 0 (count clamped to 1, as the header says)."""
    s = torch.zeros(B, 3, dtype=x.dtype).index_add_(0, mask, x)
    return s / count.clamp(min=1).to(x.dtype)[:, None]


def gamma_lookup(gamma, t, T):
    """PredefinedNoiseSchedule.forward, en_diffusion.py:1188-1190: gamma[round(t T)], python indexing (s = -1 / T at t = 0
    reads the LAST entry)."""
    return gamma[torch.round(t * T).long()]


def alpha_of(g):
    return torch.sqrt(torch.sigmoid(-g))        # en_diffusion.py:870-873


def sigma_of(g):
    return torch.sqrt(torch.sigmoid(g))         # en_diffusion.py:865-868


def gaussian_kl_addends(mu2, q_sigma, d):
    """The three addends of gaussian_KL against N(0, 1), en_diffusion.py:838-853 with p_sigma = 1."""
    return d * torch.log(1.0 / q_sigma), 0.5 * (d * q_sigma ** 2 + mu2), -0.5 * d


def cdf(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2)))       # en_diffusion.py:875-878


def log_ph_rows(h_norm, z_h, sigma_rows, nv1, nb1, epsilon=1e-10):
    """Per row: sum_k log p(class k | z_h) onehot_k, the categorical part of log_pxh_given_z0_without_constants
    (conditional_model.py:83-108, en_diffusion.py:216-255): the normal N(z_h, sigma nv1) integrated over [0.5, 1.5] around
    each class, normalised over the classes."""
    sigma_cat = (sigma_rows * nv1)[:, None]
    onehot = h_norm * nv1 + nb1
    centered = (z_h * nv1 + nb1) - 1
    logp = torch.log(cdf((centered + 0.5) / sigma_cat) - cdf((centered - 0.5) / sigma_cat) + epsilon)
    logp = logp - torch.logsumexp(logp, dim=1, keepdim=True)
    return (logp * onehot).sum(1)


def table_lookup(logpn, n1, n2):
    """The size table with the header's clamp: a size beyond the table reads its last row / column; no table: 0."""
    if logpn is None:
        return torch.zeros(len(n1), dtype=torch.float64)
    i1 = torch.clamp(n1, max=logpn.shape[0] - 1)
    i2 = torch.clamp(n2, max=logpn.shape[1] - 1)
    return logpn[i1, i2]


def _schedule(cfg, t_int, dtype):
    """forward(), conditional_model.py:218-235 / en_diffusion.py:349-366, and the per-sample scalars every term uses."""
    T, gamma = cfg["T"], cfg["gamma"].to(dtype)
    t_int = t_int.to(dtype)
    t, s = t_int / T, (t_int - 1) / T
    g_t, g_s = gamma_lookup(gamma, t, T), gamma_lookup(gamma, s, T)
    ones, zeros = torch.ones_like(t), torch.zeros_like(t)
    return dict(t=t, gamma_t=g_t, gamma_s=g_s, alpha_t=alpha_of(g_t), sigma_t=sigma_of(g_t),
                SNR_weight=1 - torch.exp(-(g_s - g_t)),                     # conditional_model.py:270, SNR: en_diffusion.py:909-912
                t_is_zero=(t_int == 0).to(dtype),
                g_0=gamma_lookup(gamma, zeros, T), g_T=gamma_lookup(gamma, ones, T))


def _size_terms(cfg, sc, dof, mu2_x, mu2_h, dtype):
    """neg_log_constants (en_diffusion.py:171-183), kl_prior (conditional_model.py:43-56 / en_diffusion.py:138-155),
    delta_log_px (conditional_model.py:198-200) for the subspace dimension `dof`."""
    dof = dof.to(dtype)
    sigma_T = sigma_of(sc["g_T"])
    ax, ah = gaussian_kl_addends(mu2_x, sigma_T, dof), gaussian_kl_addends(mu2_h, sigma_T, torch.ones_like(dof))
    kl = (ax[0] + ax[1] + ax[2]) + (ah[0] + ah[1] + ah[2])
    addend = torch.stack([a.abs() for a in ax + ah]).max()
    return dict(neg_log_constants=-(dof * (-0.5 * sc["g_0"] - 0.5 * math.log(2 * math.pi))), kl_prior=kl,
                delta_log_px=-dof * math.log(cfg["nv0"])), float(addend)


def _per_sample(sc, terms, loss_0_h, log_pN, dtype):
    d = {k: sc[k] for k in ("t", "gamma_t", "gamma_s", "alpha_t", "sigma_t", "SNR_weight", "t_is_zero")}
    d.update(terms, loss_0_h=loss_0_h, log_pN=log_pN.to(dtype))
    return {k: d[k] for k in PS_ROWS}


def _normalize(cfg, x, h, dtype):
    """normalize(), en_diffusion.py:880-895."""
    return x.to(dtype) / cfg["nv0"], (h.to(dtype) - cfg["nb1"]) / cfg["nv1"]


# ---- the conditional model --------------------------------------------------------------------------------------------------
def cond_pre(cfg, lig_x, lig_h, poc_x, poc_h, lsz, psz, eps, t_int, dtype):
    """dsbdd_loss_cond_pre -> dict(z_t, xh_pocket, per_sample, lig_xn, lig_hn, poc_xn, poc_hn, kl_addend).
    ConditionalDDPM.forward up to the network call (conditional_model.py:202-250) and every term that does not read the
    network's output (:270-291, :316); cfg.remove_com = 0: SimpleConditionalDDPM (:713-721: no centring, dof = 3 n)."""
    B = len(lsz)
    lm, pm = mask_of(lsz), mask_of(psz)
    nl, npk = torch.tensor(lsz), torch.tensor(psz)
    eps = eps.to(dtype)
    sc = _schedule(cfg, t_int, dtype)
    lxn, lhn = _normalize(cfg, lig_x, lig_h, dtype)
    pxn, phn = _normalize(cfg, poc_x, poc_h, dtype)
    xl, xp = lxn, pxn
    if cfg["remove_com"]:                                                  # remove_mean_batch, :688-696 (ligand COM from both)
        m = seg_mean3(xl, lm, B, nl)
        xl, xp = xl - m[lm], xp - m[pm]
    xh0 = torch.cat([xl, lhn], 1)
    z = sc["alpha_t"][lm, None] * xh0 + sc["sigma_t"][lm, None] * eps       # noised_representation, :162-183
    zx = z[:, :3]
    if cfg["remove_com"]:
        m = seg_mean3(zx, lm, B, nl)
        zx, xp = zx - m[lm], xp - m[pm]
    z_t = torch.cat([zx, z[:, 3:]], 1)
    dof = (nl - 1) * 3 if cfg["remove_com"] else nl * 3                   # subspace_dimensionality, en_diffusion.py:914-917
    mu = alpha_of(sc["g_T"])[lm, None] * xh0                               # kl_prior, :30-56
    terms, addend = _size_terms(cfg, sc, dof, seg_sum(mu[:, :3] ** 2, lm, B), seg_sum(mu[:, 3:] ** 2, lm, B), dtype)
    # training mode: the L0 term of z_t with gamma_t, selected by [t = 0] (:282-291)
    l0h = -seg_sum(log_ph_rows(lhn, z_t[:, 3:], sc["sigma_t"][lm], cfg["nv1"], cfg["nb1"]), lm, B) * sc["t_is_zero"]
    ps = _per_sample(sc, terms, l0h, table_lookup(cfg["logpn"], nl, npk), dtype)
    return dict(z_t=z_t, xh_pocket=torch.cat([xp, phn], 1), per_sample=ps, lig_xn=lxn, lig_hn=lhn, poc_xn=pxn, poc_hn=phn,
                kl_addend=addend)


def _virtual_rows(cfg, lig_h, dtype):
    """ligand['one_hot'][:, vnode_idx].bool() of the NORMALISED one-hot (conditional_model.py:76-78, :264-266)."""
    if cfg["vnode_idx"] < 0:
        return torch.zeros(len(lig_h), dtype=torch.bool)
    return ((lig_h.to(dtype) - cfg["nb1"]) / cfg["nv1"])[:, cfg["vnode_idx"]].bool()


def _error_rows(eps, net, mask, B, count, tz, virtual=None):
    """error_t (x [t > 0]), loss_0_x (x [t = 0]) and the logged means of |net| for one node set."""
    sq = (eps - net) ** 2
    if virtual is not None:                                                # coordinates of virtual atoms do not contribute
        keep = torch.ones_like(sq)
        keep[virtual, :3] = 0
        sq = sq * keep
    cnt = count.clamp(min=1).to(net.dtype)
    return (seg_sum(sq, mask, B) * (1 - tz), 0.5 * seg_sum(sq[:, :3], mask, B) * tz,
            seg_sum(net[:, :3].abs().mean(1), mask, B) / cnt, seg_sum(net[:, 3:].abs().mean(1), mask, B) / cnt)


def cond_post(cfg, net, eps, z_t, lig_h, lsz, alpha_t, sigma_t, t_is_zero, dtype):
    """dsbdd_loss_cond_post -> dict(xh_hat, out) with out named by COND_OUT_ROWS.  conditional_model.py:256-267 (xh_hat,
    error_t), :58-81 (loss_0_x), :289-294 (the [t = 0] masks), :318-325 (the logged means, here per sample)."""
    B, lm = len(lsz), mask_of(lsz)
    net, eps, z_t = net.to(dtype), eps.to(dtype), z_t.to(dtype)
    a, s, tz = alpha_t.to(dtype), sigma_t.to(dtype), t_is_zero.to(dtype)
    xh_hat = z_t / a[lm, None] - net * s[lm, None] / a[lm, None]           # xh_given_zt_and_epsilon, en_diffusion.py:471-477
    rows = _error_rows(eps, net, lm, B, torch.tensor(lsz), tz, _virtual_rows(cfg, lig_h, dtype))
    return dict(xh_hat=xh_hat, out=dict(zip(COND_OUT_ROWS, rows)))


# ---- the joint model --------------------------------------------------------------------------------------------------------
def joint_pre(cfg, lig_x, lig_h, poc_x, poc_h, lsz, psz, noise_lig, noise_poc, t_int, dtype):
    """dsbdd_loss_joint_pre -> dict(eps_lig, eps_poc, z_lig, z_poc, per_sample, the normalised batch, kl_addend).
    EnVariationalDiffusion.forward up to the network call (en_diffusion.py:336-375): the x part of the noise is centred
    over the sample's ligand + pocket rows (:559-578), the data is neither centred nor masked."""
    B = len(lsz)
    lm, pm = mask_of(lsz), mask_of(psz)
    nl, npk = torch.tensor(lsz), torch.tensor(psz)
    sc = _schedule(cfg, t_int, dtype)
    lxn, lhn = _normalize(cfg, lig_x, lig_h, dtype)
    pxn, phn = _normalize(cfg, poc_x, poc_h, dtype)
    nzl, nzp = noise_lig.to(dtype), noise_poc.to(dtype)
    m = seg_mean3(torch.cat([nzl[:, :3], nzp[:, :3]]), torch.cat([lm, pm]), B, nl + npk)       # remove_mean_batch, :932-942
    eps_l = torch.cat([nzl[:, :3] - m[lm], nzl[:, 3:]], 1)
    eps_p = torch.cat([nzp[:, :3] - m[pm], nzp[:, 3:]], 1)
    xh_l, xh_p = torch.cat([lxn, lhn], 1), torch.cat([pxn, phn], 1)
    z_l = sc["alpha_t"][lm, None] * xh_l + sc["sigma_t"][lm, None] * eps_l                     # :302-317
    z_p = sc["alpha_t"][pm, None] * xh_p + sc["sigma_t"][pm, None] * eps_p
    dof = (nl + npk - 1) * 3
    a_T = alpha_of(sc["g_T"])                                                                  # kl_prior_with_pocket, :109-155
    mu_l, mu_p = a_T[lm, None] * xh_l, a_T[pm, None] * xh_p
    terms, addend = _size_terms(cfg, sc, dof, seg_sum(mu_l[:, :3] ** 2, lm, B) + seg_sum(mu_p[:, :3] ** 2, pm, B),
                                seg_sum(mu_l[:, 3:] ** 2, lm, B) + seg_sum(mu_p[:, 3:] ** 2, pm, B), dtype)
    lp = seg_sum(log_ph_rows(lhn, z_l[:, 3:], sc["sigma_t"][lm], cfg["nv1"], cfg["nb1"]), lm, B) \
        + seg_sum(log_ph_rows(phn, z_p[:, 3:], sc["sigma_t"][pm], cfg["nv1"], cfg["nb1"]), pm, B)   # :252-258
    ps = _per_sample(sc, terms, -lp * sc["t_is_zero"], table_lookup(cfg["logpn"], nl, npk), dtype)
    return dict(eps_lig=eps_l, eps_poc=eps_p, z_lig=z_l, z_poc=z_p, per_sample=ps, lig_xn=lxn, lig_hn=lhn, poc_xn=pxn,
                poc_hn=phn, kl_addend=addend)


def joint_post(cfg, net_lig, net_poc, eps_lig, eps_poc, z_lig, lsz, psz, alpha_t, sigma_t, t_is_zero, dtype):
    """dsbdd_loss_joint_post -> dict(xh_hat, out) with out named by JOINT_OUT_ROWS (en_diffusion.py:381-390, :207-214,
    :416-424, :451-464)."""
    B, lm, pm = len(lsz), mask_of(lsz), mask_of(psz)
    net_l, net_p, eps_l, eps_p, z_l = (v.to(dtype) for v in (net_lig, net_poc, eps_lig, eps_poc, z_lig))
    a, s, tz = alpha_t.to(dtype), sigma_t.to(dtype), t_is_zero.to(dtype)
    xh_hat = z_l / a[lm, None] - net_l * s[lm, None] / a[lm, None]
    el, l0l, ilx, ilh = _error_rows(eps_l, net_l, lm, B, torch.tensor(lsz), tz)
    ep, l0p, ipx, iph = _error_rows(eps_p, net_p, pm, B, torch.tensor(psz), tz)
    return dict(xh_hat=xh_hat, out=dict(zip(JOINT_OUT_ROWS, (el, ep, l0l, l0p, ilx, ilh, ipx, iph))))


# ---- the backward entry points: autograd through the float64 post restatement -------------------------------------------------
def post_backward(outputs, cotangents, nets):
    """d (sum of <output, cotangent>) / d net for each net; a cotangent that is None is a zero one."""
    total = None
    for o, g in zip(outputs, cotangents):
        if g is not None:
            term = (o * g.to(o.dtype)).sum()
            total = term if total is None else total + term
    if total is None:
        return [torch.zeros_like(n) for n in nets]
    return list(torch.autograd.grad(total, nets, allow_unused=True))


def cond_post_backward(cfg, net, eps, z_t, lig_h, lsz, alpha_t, sigma_t, t_is_zero, g_err, g_l0x, g_hat, dtype=torch.float64):
    net = net.to(dtype).clone().requires_grad_(True)
    r = cond_post(cfg, net, eps, z_t, lig_h, lsz, alpha_t, sigma_t, t_is_zero, dtype)
    return post_backward([r["out"]["error_t"], r["out"]["loss_0_x"], r["xh_hat"]], [g_err, g_l0x, g_hat], [net])[0]


def joint_post_backward(cfg, net_lig, net_poc, eps_lig, eps_poc, z_lig, lsz, psz, alpha_t, sigma_t, t_is_zero, g_err_lig,
                        g_err_poc, g_l0x_lig, g_l0x_poc, g_hat, dtype=torch.float64):
    nl = net_lig.to(dtype).clone().requires_grad_(True)
    npk = net_poc.to(dtype).clone().requires_grad_(True)
    r = joint_post(cfg, nl, npk, eps_lig, eps_poc, z_lig, lsz, psz, alpha_t, sigma_t, t_is_zero, dtype)
    o = r["out"]
    g = post_backward([o["error_t_lig"], o["error_t_pocket"], o["loss_0_x_ligand"], o["loss_0_x_pocket"], r["xh_hat"]],
                      [g_err_lig, g_err_poc, g_l0x_lig, g_l0x_poc, g_hat], [nl, npk])
    return [torch.zeros_like(n) if v is None else v for v, n in zip(g, (nl, npk))]


# ---- the inputs of tests/test_gpu_loss_head_kernels.py, seeded on the host ----------------------------------------------------
# (here, so that tests/test_loss_restatement.py can show on the CPU that the tolerance rule is satisfiable on every one)
BATCHES = {
    # a one-atom ligand (dof = 0), 257 rows = one more than the 256-thread stride, 300 rows = a second stride pass, an empty
    # and a one-row pocket, no boundary at a multiple of anything
    "ragged": ([1, 7, 257, 23, 12, 300], [300, 5, 0, 40, 257, 1]),
    # an empty ligand and an empty pocket inside the batch
    "empty": ([4, 0, 9], [6, 3, 0]),
}
# (atom_nf, residue_nf, norm_value_x, norm_value_h, norm_bias_h); the first three rows are filled from the package's configs
WIDTHS = {"crossdock_fullatom_cond": None, "crossdock_ca_cond": None, "moad_fullatom_joint": None,
          "odd": (3, 7, 1.0, 4.0, 0.0),                   # 3 + nf is no multiple of 4
          "odd_biased": (3, 7, 5.0, 0.25, 0.5),
          "fullatom_biased": (10, 10, 5.0, 0.25, 0.5)}
TABLES = ("polynomial_2/500/5e-4", "polynomial_2/500/1e-5", "cosine/1000/1e-4", "synthetic")
T_MODES = ("mixed", "zeros", "nonzero")
SYNTHETIC_T = 16


def widths(name):
    if WIDTHS[name] is None:
        from diffsbdd_amd import synthetic
        base, ddpm = synthetic.arch_cfg(name)
        return (base["atom_nf"], base["residue_nf"], float(ddpm["norm_values"][0]), float(ddpm["norm_values"][1]), 0.0)
    return WIDTHS[name]


def gamma_of(table):
    """-> (gamma [T + 1] float32, T).  The shipped schedules from the oracle's own table; `synthetic`: monotone with
    gamma[0] = -2, where sigma_0 = 0.345 is comparable to the class spacing for norm_value_h of 1 .. 5."""
    if table == "synthetic":
        return torch.linspace(-2.0, 8.0, SYNTHETIC_T + 1), SYNTHETIC_T
    from oracle.ddpm_oracle import gamma_table
    kind, T, precision = table.split("/")
    return gamma_table(kind, int(T), float(precision)), int(T)


def t_int_of(mode, T, B):
    full = {"mixed": [0, T, 1, 13, 0, T - 1], "zeros": [0] * 6, "nonzero": [T, 1, 13, 2, T - 2, T - 1]}[mode]
    return torch.tensor(full[:B], dtype=torch.float32)


def l0h_resolved(table, nv1):
    """Whether loss_0_h of a t = 0 sample is a float32 quantity at all.  With the shipped schedules sigma_0 norm_value_h is
    5 .. 50 times smaller than half the class spacing: the true class has probability 1 - 1e-8 or 1 + 1e-10 (the epsilon),
    which is no float32, the float64 term is ~ 1e-9 .. 1e-7 per row and the float32 restatement returns 0 or rounding
    noise: `within`, relative to the block's own magnitude, fails the float32 restatement itself (err_ref ~ 1; measured by
    tests/test_loss_restatement.py).  The same holds on the synthetic table for norm_value_h = 0.25.  Those cases are
    SHRUNK, not the rule loosened: their loss_0_h block is compared without its t = 0 entries (see l0h_block)."""
    return table == "synthetic" and nv1 >= 1.0


def l0h_block(case, values):
    """The loss_0_h entries of `values` [B] that the tolerance rule is applied to in this case."""
    values = torch.as_tensor(values).detach().cpu()
    return values if case["l0h_resolved"] else values[case["t_int"] != 0]


def make_case(batch, width, table, t_mode, seed=0, sizes=None, t_int=None):
    """One set of float32 host inputs for all six entry points of both models."""
    lsz, psz = sizes or BATCHES[batch]
    a, r, nv0, nv1, nb1 = widths(width)
    gamma, T = gamma_of(table)
    B = len(lsz)
    g = torch.Generator().manual_seed(7919 * seed + 31 * list(WIDTHS).index(width) + 7 * TABLES.index(table)
                                      + T_MODES.index(t_mode) + (1000 if batch == "empty" else 0))
    lm, pm = mask_of(lsz), mask_of(psz)
    nl, npk = len(lm), len(pm)
    centre = (torch.rand(B, 3, generator=g) - 0.5) * 10.0 + torch.tensor([3.0, -4.0, 2.5])     # un-centred, a few Angstrom off
    lig_x = centre[lm] + torch.randn(nl, 3, generator=g) * 2.5 + 0.7
    poc_x = centre[pm] + torch.randn(npk, 3, generator=g) * 7.0
    lt = torch.randint(0, a, (nl,), generator=g)
    lo = offsets(lsz)
    for b, n in enumerate(lsz):            # class 2 = the virtual atom: one virtual and one real row in every sample >= 2 rows
        if n >= 2:
            lt[lo[b]], lt[lo[b] + 1] = 2, 0
    lig_h = torch.nn.functional.one_hot(lt, a).float()
    poc_h = torch.nn.functional.one_hot(torch.randint(0, r, (npk,), generator=g), r).float()
    eps = torch.randn(nl, 3 + a, generator=g)               # the conditional model's draw = the joint model's ligand noise
    noise_poc = torch.randn(npk, 3 + r, generator=g)
    net_lig = eps + 0.3 * torch.randn(nl, 3 + a, generator=g)
    net_poc = noise_poc + 0.3 * torch.randn(npk, 3 + r, generator=g)
    cot = dict(g_err=torch.randn(B, generator=g), g_l0x=torch.randn(B, generator=g), g_hat=torch.randn(nl, 3 + a, generator=g),
               g_err_poc=torch.randn(B, generator=g), g_l0x_poc=torch.randn(B, generator=g))
    logpn = -torch.rand(12, 60, generator=g) * 9.0 - 0.5                                       # sizes 257 and 300 exceed both axes
    t_int = t_int_of(t_mode, T, B) if t_int is None else t_int
    return dict(name=f"{batch}-{width}-{table}-{t_mode}", lsz=list(lsz), psz=list(psz), a=a, r=r, T=T, gamma=gamma, nv0=nv0,
                nv1=nv1, nb1=nb1, logpn=logpn, t_int=t_int, lig_x=lig_x, lig_h=lig_h, poc_x=poc_x, poc_h=poc_h, eps=eps,
                noise_poc=noise_poc, net_lig=net_lig, net_poc=net_poc, cot=cot, l0h_resolved=l0h_resolved(table, nv1))


def cfg_of(case, remove_com=1, vnode_idx=-1, table=True):
    return dict(T=case["T"], gamma=case["gamma"], nv0=case["nv0"], nv1=case["nv1"], nb1=case["nb1"], remove_com=remove_com,
                vnode_idx=vnode_idx, logpn=case["logpn"] if table else None)


def case_grid(width):
    """Every case of one feature-width / normalisation row: both batches x four gamma tables x three t_int patterns."""
    return [make_case(b, width, tab, tm) for b in BATCHES for tab in TABLES for tm in T_MODES]


def big_case(width="crossdock_fullatom_cond"):
    """More than 1024 x 256 elements of d_net: the second pass of the backward kernels' grid-stride loop.  Conditional:
    64 x 320 ligand rows x 13 = 266 240; joint: + 64 x 20 pocket rows x 13."""
    t_int = t_int_of("mixed", SYNTHETIC_T, 6).repeat(11)[:64]
    return make_case("big", width, "synthetic", "mixed", sizes=([320] * 64, [20] * 64), t_int=t_int)


# ---- a case through pre -> post (-> backward) in one dtype ---------------------------------------------------------------------
MODELS = ("cond", "simple", "joint")          # ConditionalDDPM (remove_com = 1), SimpleConditionalDDPM (0), the joint model
COND_COTANGENTS = ("g_err", "g_l0x", "g_hat")
JOINT_COTANGENTS = ("g_err", "g_err_poc", "g_l0x", "g_l0x_poc", "g_hat")


def reference(case, model, dtype, vnode_idx=-1, table=True):
    """-> (cfg, pre, post): the post restatement is fed with the pre restatement's outputs of the same dtype."""
    c = case
    cfg = cfg_of(c, remove_com=0 if model == "simple" else 1, vnode_idx=vnode_idx, table=table)
    if model == "joint":
        pre = joint_pre(cfg, c["lig_x"], c["lig_h"], c["poc_x"], c["poc_h"], c["lsz"], c["psz"], c["eps"], c["noise_poc"],
                        c["t_int"], dtype)
        ps = pre["per_sample"]
        post = joint_post(cfg, c["net_lig"], c["net_poc"], pre["eps_lig"], pre["eps_poc"], pre["z_lig"], c["lsz"], c["psz"],
                          ps["alpha_t"], ps["sigma_t"], ps["t_is_zero"], dtype)
    else:
        pre = cond_pre(cfg, c["lig_x"], c["lig_h"], c["poc_x"], c["poc_h"], c["lsz"], c["psz"], c["eps"], c["t_int"], dtype)
        ps = pre["per_sample"]
        post = cond_post(cfg, c["net_lig"], c["eps"], pre["z_t"], c["lig_h"], c["lsz"], ps["alpha_t"], ps["sigma_t"],
                         ps["t_is_zero"], dtype)
    return cfg, pre, post


def reference_backward(case, model, dtype, cfg, pre, present):
    """d_net (conditional) or [d_net_lig, d_net_pocket] (joint) by autograd through the post restatement in `dtype`;
    present: the names of the cotangents that are given (the others are absent = zero)."""
    c, ps = case, pre["per_sample"]
    g = {k: (c["cot"][k] if k in present else None) for k in JOINT_COTANGENTS}
    if model == "joint":
        return joint_post_backward(cfg, c["net_lig"], c["net_poc"], pre["eps_lig"], pre["eps_poc"], pre["z_lig"], c["lsz"],
                                   c["psz"], ps["alpha_t"], ps["sigma_t"], ps["t_is_zero"], g["g_err"], g["g_err_poc"],
                                   g["g_l0x"], g["g_l0x_poc"], g["g_hat"], dtype)
    return [cond_post_backward(cfg, c["net_lig"], c["eps"], pre["z_t"], c["lig_h"], c["lsz"], ps["alpha_t"], ps["sigma_t"],
                               ps["t_is_zero"], g["g_err"], g["g_l0x"], g["g_hat"], dtype)]


PRE_TENSORS = {"cond": ("z_t", "xh_pocket", "lig_xn", "lig_hn", "poc_xn", "poc_hn"),
               "joint": ("eps_lig", "eps_poc", "z_lig", "z_poc", "lig_xn", "lig_hn", "poc_xn", "poc_hn")}
PRE_TENSORS["simple"] = PRE_TENSORS["cond"]
EXACT_ROWS = ("t", "t_is_zero")               # compared with the float32 restatement bit for bit, not by the rule


def compare_forward(tag, case, model, got_pre, got_post, ref64, ref32):
    """The tolerance rule on every output block of pre and post: got_* are dicts shaped like the restatement's (the
    kernel's outputs, or -- in the self-check -- the float32 restatement's).  -> {block: (err_ref, err)}."""
    (_, p64, o64), (_, p32, o32) = ref64, ref32
    res = {}
    for k in PRE_TENSORS[model]:
        res[k] = within(f"{tag}.{k}", got_pre[k], p64[k], p32[k])
    for k in PS_ROWS:
        g, r64, r32 = got_pre["per_sample"][k], p64["per_sample"][k], p32["per_sample"][k]
        if k in EXACT_ROWS:
            assert torch.equal(torch.as_tensor(g).cpu().float(), r32.float()), (tag, k)
        elif k == "kl_prior":
            res[k] = within_at(f"{tag}.{k}", g, r64, r32, p64["kl_addend"])
        elif k == "neg_log_constants":
            res[k] = within_at(f"{tag}.{k}", g, r64, r32, float(r64.abs().max()))
        elif k == "loss_0_h":
            res[k] = within(f"{tag}.{k}", l0h_block(case, g), l0h_block(case, r64), l0h_block(case, r32))
        else:
            res[k] = within(f"{tag}.{k}", g, r64, r32)
    res["xh_hat"] = within(f"{tag}.xh_hat", got_post["xh_hat"], o64["xh_hat"], o32["xh_hat"])
    for k in o64["out"]:
        res[k] = within(f"{tag}.{k}", got_post["out"][k], o64["out"][k], o32["out"][k])
    return res


BACKWARD_T_MODE = "mixed"     # the backward reads t only through [t = 0]: the pattern with both kinds of sample


def cotangent_sets(model):
    """Conditional: all eight present / absent combinations.  Joint: all present, all absent, each of the five absent alone."""
    if model != "joint":
        return [tuple(k for k, on in zip(COND_COTANGENTS, bits) if on)
                for bits in ((a, b, c) for a in (1, 0) for b in (1, 0) for c in (1, 0))]
    return [JOINT_COTANGENTS, ()] + [tuple(k for k in JOINT_COTANGENTS if k != off) for off in JOINT_COTANGENTS]


def compare_backward(tag, got, ref64, ref32):
    """The tolerance rule on d_net (conditional) or d_net_lig, d_net_pocket (joint)."""
    names = ("d_net",) if len(ref64) == 1 else ("d_net_lig", "d_net_pocket")
    return {n: within(f"{tag}.{n}", g, a, b) for n, g, a, b in zip(names, got, ref64, ref32)}
