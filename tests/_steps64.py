"""Plain torch restatements of the per-sample DDPM step entry points of include/diffsbdd_hip.h, written from the header's
comments (not from the kernels), for tests/test_gpu_noise_and_steps.py.  They run in the dtype of their inputs: float64 is
the reference, float32 the yardstick (`err_ref` of the tolerance rule below).

Calling convention, the same for every restatement:  f(L, P, S, lsz, psz, **scalars) -> (L_out, P_out, S_out)
  L  dict of per-ligand-row tensors   [sum(lsz)][...]      lsz[b] = ligand rows of sample b
  P  dict of per-pocket-row tensors   [sum(psz)][...]      psz[b] = pocket rows of sample b
  S  dict of per-sample tensors       [B][...]
and the outputs hold only what the entry point writes.  Inputs are never modified.
"""
import torch

ULP4 = 4 * 2.0 ** -23


def offsets(sizes):
    o = [0]
    for s in sizes:
        o.append(o[-1] + int(s))
    return o


def samples(lsz, psz):
    lo, po = offsets(lsz), offsets(psz)
    for b in range(len(lsz)):
        yield b, slice(lo[b], lo[b + 1]), slice(po[b], po[b + 1]), int(lsz[b]), int(psz[b])


def _sum3(x):
    return x[:, :3].sum(0)


def cond_reverse_update(L, P, S, lsz, psz, *, alpha_ts, c_eps, sigma, remove_com):
    """z_lig <- z_lig/alpha_ts - c_eps*eps_lig + sigma*noise ; then the ligand centre of mass of each sample is subtracted
    from its ligand AND pocket x."""
    z = L["z"] / alpha_ts - c_eps * L["eps"] + sigma * L["noise"]
    poc = P["poc"].clone()
    if remove_com:
        for b, sl, sp, nl, npk in samples(lsz, psz):
            m = _sum3(z[sl]) / max(nl, 1)
            z[sl, :3] -= m
            poc[sp, :3] -= m
    return {"z": z}, {"poc": poc}, {}


def _centred_noise(nl_, np_, lsz, psz):
    """x part of the noise made COM-free over each sample's ligand + pocket rows."""
    nl_, np_ = nl_.clone(), np_.clone()
    for b, sl, sp, nl, npk in samples(lsz, psz):
        m = (_sum3(nl_[sl]) + _sum3(np_[sp])) / max(nl + npk, 1)
        nl_[sl, :3] -= m
        np_[sp, :3] -= m
    return nl_, np_


def _remove_joint_com(zl, zp, lsz, psz):
    for b, sl, sp, nl, npk in samples(lsz, psz):
        m = (_sum3(zl[sl]) + _sum3(zp[sp])) / max(nl + npk, 1)
        zl[sl, :3] -= m
        zp[sp, :3] -= m


def joint_reverse_update(L, P, S, lsz, psz, *, alpha_ts, c_eps, sigma, center_noise):
    """Both node sets updated like the conditional step, the joint COM removed; center_noise: the x part of the noise
    is first made COM-free over the sample's ligand + pocket rows."""
    nl_, np_ = _centred_noise(L["noise"], P["noise"], lsz, psz) if center_noise else (L["noise"], P["noise"])
    zl = L["z"] / alpha_ts - c_eps * L["eps"] + sigma * nl_
    zp = P["poc"] / alpha_ts - c_eps * P["eps"] + sigma * np_
    _remove_joint_com(zl, zp, lsz, psz)
    return {"z": zl}, {"poc": zp}, {}


def segment_mean3(rows, sizes):
    """out[b][0..2] = mean over the rows of sample b of x[:, 0..2], count clamped to >= 1."""
    o = offsets(sizes)
    return torch.stack([_sum3(rows[o[b]:o[b + 1]]) / max(int(sizes[b]), 1) for b in range(len(sizes))])


def cond_affine_noise(L, P, S, lsz, psz, *, a, sigma, remove_com):
    """z_lig <- a * z_lig + sigma * noise ; remove_com: ligand COM subtracted from ligand and pocket x."""
    z = a * L["z"] + sigma * L["noise"]
    poc = P["poc"].clone()
    if remove_com:
        for b, sl, sp, nl, npk in samples(lsz, psz):
            m = _sum3(z[sl]) / max(nl, 1)
            z[sl, :3] -= m
            poc[sp, :3] -= m
    return {"z": z}, {"poc": poc}, {}


def joint_affine_noise(L, P, S, lsz, psz, *, a, sigma, center_noise, remove_com):
    """z <- a * z + sigma * noise on both node sets, noise optionally COM-centred (x part), result optionally COM-free.
    a = 0 draws from the noise alone: z is not read."""
    nl_, np_ = _centred_noise(L["noise"], P["noise"], lsz, psz) if center_noise else (L["noise"], P["noise"])
    if a == 0:
        zl, zp = sigma * nl_, sigma * np_
    else:
        zl, zp = a * L["z"] + sigma * nl_, a * P["poc"] + sigma * np_
    if remove_com:
        _remove_joint_com(zl, zp, lsz, psz)
    return {"z": zl}, {"poc": zp}, {}


def cond_repaint_update(L, P, S, lsz, psz, *, alpha_s, sigma_s, alpha_ts, sigma_ts, resample, remove_com):
    """One RePaint iteration of the conditional model.  On entry z = denoised ("unknown") state, poc = pocket moved by
    that step.  Known part noised to level s around the moved pocket, COM of the fixed atoms of both parts aligned, blend
    by `fixed`, optional q(z_t | z_s) resampling step; the pocket follows every translation."""
    zu, poc = L["z"].clone(), P["poc"].clone()
    out = torch.empty_like(zu)
    for b, sl, sp, nl, npk in samples(lsz, psz):
        shift = _sum3(poc[sp]) / max(npk, 1) - S["com0"][b]
        known = L["xh0"][sl].clone()
        known[:, :3] += shift
        zk = alpha_s * known + sigma_s * L["noise"][sl]
        if remove_com:
            m1 = _sum3(zk) / max(nl, 1)
            zk[:, :3] -= m1
            poc[sp, :3] -= m1
        f = L["fixed"][sl]
        nf = max(float(f.sum()), 1.0)
        dx = _sum3(zu[sl] * f[:, None]) / nf - _sum3(zk * f[:, None]) / nf
        zk[:, :3] += dx
        poc[sp, :3] += dx
        v = zk * f[:, None] + zu[sl] * (1 - f[:, None])
        if resample:
            v = alpha_ts * v + sigma_ts * L["noise2"][sl]
            if remove_com:
                m2 = _sum3(v) / max(nl, 1)
                v[:, :3] -= m2
                poc[sp, :3] -= m2
        out[sl] = v
    return {"z": out}, {"poc": poc}, {}


def cond_step_keyed(L, P, S, lsz, psz, *, alpha_ts, c_eps, sigma, repaint, alpha_s, sigma_s, sigma_ts, remove_com):
    """The posterior update with the noise of draw d (L["noise"]); repaint = 1: followed by the RePaint iteration (known
    part noised with draw d + 1 = L["noise1"]); 2: and the q(z_t | z_s) jump (draw d + 2 = L["noise2"])."""
    Lo, Po, _ = cond_reverse_update(L, P, S, lsz, psz, alpha_ts=alpha_ts, c_eps=c_eps, sigma=sigma, remove_com=remove_com)
    if not repaint:
        return Lo, Po, {}
    L2 = dict(z=Lo["z"], xh0=L["xh0"], fixed=L["fixed"], noise=L["noise1"], noise2=L["noise2"])
    return cond_repaint_update(L2, dict(poc=Po["poc"]), S, lsz, psz, alpha_s=alpha_s, sigma_s=sigma_s, alpha_ts=alpha_ts,
                               sigma_ts=sigma_ts, resample=repaint == 2, remove_com=remove_com)


def joint_repaint_update(L, P, S, lsz, psz, *, alpha_s, sigma_s, alpha_ts, sigma_ts, jump):
    """One RePaint iteration of the joint model: known part q(z_s | x) with COM-centred noise, COM alignment over the
    fixed ligand + pocket nodes, blend, optional jump back q(z_t | z_s) (COM-centred noise) + joint COM removal."""
    n1l, n1p = _centred_noise(L["noise"], P["noise"], lsz, psz)
    kl, kp = alpha_s * L["xh0"] + sigma_s * n1l, alpha_s * P["xh0"] + sigma_s * n1p
    fl, fp = L["fixed"][:, None], P["fixed"][:, None]
    for b, sl, sp, nl, npk in samples(lsz, psz):
        nk = max(float(fl[sl].sum() + fp[sp].sum()), 1.0)
        dx = (_sum3(L["z"][sl] * fl[sl]) + _sum3(P["poc"][sp] * fp[sp])) / nk \
            - (_sum3(kl[sl] * fl[sl]) + _sum3(kp[sp] * fp[sp])) / nk
        kl[sl, :3] += dx
        kp[sp, :3] += dx
    zl, zp = kl * fl + L["z"] * (1 - fl), kp * fp + P["poc"] * (1 - fp)
    if jump:
        n2l, n2p = _centred_noise(L["noise2"], P["noise2"], lsz, psz)
        zl, zp = alpha_ts * zl + sigma_ts * n2l, alpha_ts * zp + sigma_ts * n2p
        _remove_joint_com(zl, zp, lsz, psz)
    return {"z": zl}, {"poc": zp}, {}


# ---- evaluation helpers ---------------------------------------------------------------------------------------------------
def cast(d, dtype):
    return {k: v.to(dtype) for k, v in d.items()}


def evaluate(fn, L, P, S, lsz, psz, dtype, **scalars):
    """fn on copies of the inputs in `dtype`."""
    return fn(cast(L, dtype), cast(P, dtype), cast(S, dtype), lsz, psz, **scalars)


def within(name, hip, ref64, ref32):
    """The tolerance rule of tests/test_gpu_trainer.py: err_ref = the float32 restatement against the float64 one; the
    kernel must satisfy
    |hip - f64| <= max(2 err_ref, 4 ulp) relative to the block's largest magnitude, and 1e-4 at most.
    -> (err_ref, err_hip), both relative."""
    hip, ref64, ref32 = (torch.as_tensor(v).detach().cpu().double().reshape(-1) for v in (hip, ref64, ref32))
    if ref64.numel() == 0:
        assert hip.numel() == 0
        return 0.0, 0.0
    mag = max(float(ref64.abs().max()), 1e-30)
    err_ref = float((ref32 - ref64).abs().max()) / mag
    err = float((hip - ref64).abs().max()) / mag
    bound = max(2 * err_ref, ULP4)
    print(f"  {name}: err_ref {err_ref:.3e}  hip {err:.3e}  bound {bound:.3e}  (magnitude {mag:.3e})")
    assert torch.isfinite(hip).all(), name
    assert err <= bound and err <= 1e-4, (name, err, bound)
    return err_ref, err
