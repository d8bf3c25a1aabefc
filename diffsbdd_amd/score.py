"""Score GIVEN ligands in their pockets by the model's negative log-likelihood bound (pocket-conditioned models).

The only other route to the bound is `ConditionalDDPM.forward` in evaluation mode (conditional_model.py:202-330 of the
reference, what `Trainer.validate` uses): one random diffusion time per complex, two network calls for it, ~ 250 small
torch launches around them -- a single-sample estimate that cannot rank poses or molecules.  Here:

Estimator.  Ligand b gets K time slots with integer times t[b,k] in 1..T and weights w[b,k], and one zero slot (t = 0).
Every state is evaluated exactly as the reference's evaluation branch does it -- normalise, remove the ligand's centre of
mass from ligand and pocket, z = alpha_t xh0 + sigma_t eps centred again together with the state's own pocket copy, the
network on (z, xh_pocket, t / T), error_t = sum (eps - net)^2 over the ligand's rows and all columns, SNR_weight =
1 - SNR(gamma_s - gamma_t); the zero slot gives loss_0_x, loss_0_h (on z_0, gamma_0) -- and

    loss_t(b) = sum_k ((-0.5 w[b,k]) SNR_weight(t[b,k])) error_t(b,k)          (k ascending, float32)
    nll(b)    = (((loss_t + ((loss_0_x + loss_0_h) + neg_log_constants)) + kl_prior) - delta_log_px) - log_pN

which with K = 1 and w = T is `train.nll_from_terms(..., training=False)` on the reference's 12-tuple, operation for
operation.  `time_grid` cuts {1..T} into K contiguous strata, draws one time per stratum from a seeded host generator and
weights it by the stratum's size; the same grid serves every ligand of a call (common random numbers: what ranking
needs).  K = T is the full bound for the drawn noise, K = 1 the reference's estimator.

States and chunks.  The states of a call are the (ligand, slot) pairs, ligand-major, time slots first, the zero slot last:
g = b (K + 1) + k.  They are processed in chunks of at most `max_states` states -- one network call per chunk, whatever
ligand the chunk begins or ends in -- by the kernels of csrc/score.h: the noise launch, `dsbdd_score_cond_pre`, the network
call, `dsbdd_score_cond_post`; one `dsbdd_score_reduce` per call.  The inputs are read through the state -> ligand
indirection; nothing is repeated in torch.  No pocket frame and no forward cone: both need ONE t per network call
(csrc/forward.h), and a chunk carries one t per state.

Noise.  Keyed generator (`dsbdd_randn_keyed`, csrc/ddpm.h): the draw of state (ligand id i, slot k) of a call with n_slots
slots per ligand is the block of global sample id  i * n_slots + k,  draw index 0, stream id `NOISE_STREAM`, under `seed`:
a function of (seed, ligand_id, slot, n_slots) only -- not of the batch, the chunking or the module's own generator state
(`_seed`, `_draw`, `_sample_ids` are neither read nor written).  An injected `noise_source` is asked once per slot for
(N_lig, 3 + atom_nf), time slots in order, then the zero slot (K = 1: the reference's order); it needs a single chunk.

The joint model.  `nll_of_complex` (`EnVariationalDiffusion.nll_of_complex`, csrc/score_joint.h) is the same estimator
for the model that diffuses ligand and pocket together: the bound of -log p(ligand, pocket).  Same time grid, states,
chunks and launch sequence (`dsbdd_score_joint_pre`, the network call with both outputs, `dsbdd_score_joint_post`; one
`dsbdd_score_joint_reduce`); both node sets are noised, error_t and loss_0_x have a ligand and a pocket part, the degrees
of freedom are 3 (N_lig + N_pocket - 1) and log_pN is the joint log p(N_lig, N_pocket).  For candidates in one pocket
p(ligand, pocket) = p(ligand | pocket) p(pocket): the joint bound ranks them as the conditional one does, up to the
slack of the bound; `loss_t_lig` is the ligand rows' share of loss_t.  Its noise keying and `center` are described at
the function.  Out of scope for either model: virtual atoms, learned schedules, sharing pocket work across states.
"""
from __future__ import annotations

import argparse
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

__all__ = ["time_grid", "combine_terms", "nll_given_pocket", "combine_terms_joint", "nll_of_complex", "NOISE_STREAM",
           "NOISE_STREAM_JOINT_LIG", "NOISE_STREAM_JOINT_POCKET", "main"]

NOISE_STREAM = 5          # stream id of the scorer's keyed draws (sampling chains use 0 and 1, the joint training loss 1 and 2)
NOISE_STREAM_JOINT_LIG, NOISE_STREAM_JOINT_POCKET = 6, 7            # nll_of_complex: one block per node set
DEFAULT_N_TIMES = 10


# --------------------------------------------------------------------------- the estimator, host side
def time_grid(T, n_times, seed=0):
    """-> (times int64 [K], weights float32 [K]): {1..T} cut into K = n_times contiguous strata lo_j = floor(j T / K) + 1 ..
    hi_j = floor((j + 1) T / K), one time per stratum drawn uniformly from `torch.Generator().manual_seed(seed)` (stratum
    order), weight = the stratum's size.  K = T: every time once, weight 1; K = 1: one time, weight T."""
    T, K = int(T), int(n_times)
    if K < 1 or K > T:
        raise ValueError(f"n_times = {K} must lie in [1, T = {T}]")
    gen = torch.Generator().manual_seed(int(seed))
    times, weights = [], []
    for j in range(K):
        lo, hi = j * T // K + 1, (j + 1) * T // K
        times.append(int(torch.randint(lo, hi + 1, (1,), generator=gen)))
        weights.append(float(hi - lo + 1))
    return torch.tensor(times, dtype=torch.int64), torch.tensor(weights, dtype=torch.float32)


def combine_terms(weight, SNR_weight, error_t, loss_0_x, loss_0_h, neg_log_constants, kl_prior, delta_log_px, log_pN):
    """The combination `dsbdd_score_reduce` does on the device, in torch (float32, the same order): weight / SNR_weight /
    error_t are [B, K], the other terms [B].  -> (nll [B], loss_t [B])."""
    f = lambda v: torch.as_tensor(v).to(torch.float32)
    SNR_weight, error_t = f(SNR_weight), f(error_t)
    if error_t.dim() == 1:                                           # K = 1 given as [B]
        SNR_weight, error_t = SNR_weight.reshape(-1, 1), error_t.reshape(-1, 1)
    weight = f(weight).to(error_t.device)
    weight = weight.reshape(-1, 1) if weight.dim() == 1 and error_t.shape[1] == 1 and weight.numel() == error_t.shape[0] \
        else weight
    weight = torch.broadcast_to(weight, error_t.shape)
    loss_t = torch.zeros(error_t.shape[0], dtype=torch.float32, device=error_t.device)
    for k in range(error_t.shape[1]):
        loss_t = loss_t + ((-0.5 * weight[:, k]) * SNR_weight[:, k]) * error_t[:, k]
    loss_0 = (f(loss_0_x) + f(loss_0_h)) + f(neg_log_constants)
    nll = (((loss_t + loss_0) + f(kl_prior)) - f(delta_log_px)) - f(log_pN)
    return nll, loss_t


def _slots(T, B, n_times, times, weights, seed):
    """-> (t float32 [B, K], w float32 [B, K]) on the host, validated."""
    if isinstance(times, str):
        if times != "all":
            raise ValueError("times must be a tensor, a list or 'all'")
        n_times, times = T, None
    if times is None:
        t, w = time_grid(T, min(DEFAULT_N_TIMES, T) if n_times is None else n_times, seed)
        t = t.to(torch.float32)
    else:
        t = torch.as_tensor(times).detach().cpu().to(torch.float64)
        if t.dim() not in (1, 2) or t.numel() == 0 or (t.dim() == 2 and t.shape[0] != B):
            raise ValueError(f"times must have shape [K] or [B = {B}, K], got {tuple(t.shape)}")
        if bool((t != t.round()).any()) or bool((t < 1).any()) or bool((t > T).any()):
            raise ValueError(f"times must be integers in 1..T = {T}")
        t = t.to(torch.float32)
        w = None
    K = t.shape[-1]
    if weights is not None:
        w = torch.as_tensor(weights).detach().cpu().to(torch.float32)
        if w.dim() == 0:
            w = w.expand(K)
        if tuple(w.shape) not in ((K,), (B, K)):
            raise ValueError(f"weights must have shape [K = {K}] or [B = {B}, K], got {tuple(w.shape)}")
        if not bool(torch.isfinite(w).all()):
            raise ValueError("weights must be finite")
    elif w is None:
        w = torch.full((K,), float(T) / K, dtype=torch.float32)
    expand = lambda v: (v.unsqueeze(0).expand(B, K) if v.dim() == 1 else v).contiguous()
    return expand(t), expand(w)


def _check_model(ddpm, joint=False):
    """`joint`: the call is `nll_of_complex` (the model that diffuses both node sets), else `nll_given_pocket`."""
    from .conditional_model import ConditionalDDPM
    from .en_diffusion import EnVariationalDiffusion, PredefinedNoiseSchedule
    what = "nll_of_complex" if joint else "nll_given_pocket"
    if joint:
        if isinstance(ddpm, ConditionalDDPM):
            raise NotImplementedError(f"{type(ddpm).__name__}: a pocket-conditioned model has no likelihood of the complex; "
                                      "score its ligands with nll_given_pocket")
        if not isinstance(ddpm, EnVariationalDiffusion):
            raise NotImplementedError(f"{type(ddpm).__name__}: complexes are scored under the joint model only")
    elif not isinstance(ddpm, ConditionalDDPM):
        raise NotImplementedError(f"{type(ddpm).__name__}: ligands are scored under pocket-conditioned models only "
                                  "(the joint model scores complexes: nll_of_complex)")
    if not isinstance(ddpm.gamma, PredefinedNoiseSchedule):
        raise NotImplementedError(f"{what} needs a predefined noise schedule (the kernels read its gamma table)")
    if ddpm.vnode_idx is not None:
        raise NotImplementedError(f"{what} does not support virtual atoms (vnode_idx is set)")
    if getattr(ddpm.size_distribution, "_table", None) is None:
        raise NotImplementedError(f"{what} reads log p(N_lig {', ' if joint else '| '}N_pocket) from DistributionNodes._table")


def _check_batch(ddpm, ligand, pocket, table=0):
    """Sizes and masks of the batch, on the host (one copy of four small tensors).  `table`: which table of
    `DistributionNodes._table` the sizes must lie in (0: log p(N_lig | N_pocket), 2: log p(N_lig, N_pocket)).
    -> (n_lig list, n_pocket list)"""
    nl = [int(v) for v in ligand['size'].detach().cpu().reshape(-1).tolist()]
    npk = [int(v) for v in pocket['size'].detach().cpu().reshape(-1).tolist()]
    B = len(nl)
    if B < 1 or len(npk) != B:
        raise ValueError(f"{B} ligands for {len(npk)} pockets (pocket b belongs to ligand b; at least one)")
    logp = ddpm.size_distribution._table(table, torch.device("cpu"))
    n1, n2 = logp.shape
    for b in range(B):
        if nl[b] < 1:
            raise ValueError(f"ligand {b} has no atoms")
        if nl[b] >= n1 or npk[b] < 0 or npk[b] >= n2:
            raise ValueError(f"ligand {b}: sizes (n_lig = {nl[b]}, n_pocket = {npk[b]}) lie outside the size histogram "
                             f"[{n1}][{n2}] of the model")
        if not np.isfinite(float(logp[nl[b], npk[b]])):
            raise ValueError(f"ligand {b}: sizes (n_lig = {nl[b]}, n_pocket = {npk[b]}) have probability zero under the "
                             "model's size histogram")
    for name, d, sizes in (("ligand", ligand, nl), ("pocket", pocket, npk)):
        m = d['mask'].detach().cpu().to(torch.int64).reshape(-1)
        if m.numel() > 1 and bool((m[1:] < m[:-1]).any()):
            raise ValueError(f"{name} mask must be sorted ascending: the HIP kernels locate a sample's rows by binary search")
        if m.numel() != sum(sizes) or d['x'].shape[0] != m.numel() or d['one_hot'].shape[0] != m.numel() or (
                m.numel() and (int(m[0]) < 0 or int(m[-1]) >= B)) or torch.bincount(m, minlength=B).tolist() != sizes:
            raise ValueError(f"{name} mask does not match {name}['size']")
    return nl, npk


def _on_device(ddpm, ligand, pocket, what="nll_given_pocket"):
    p = next(ddpm.dynamics.parameters())
    if p.device.type != 'cuda':
        raise _lib.HipLibraryError(f"{what} runs on the HIP kernels only: move the model to a GPU "
                                   f"(parameters are on {p.device}); there is no CPU fallback")
    for name, d in (("ligand", ligand), ("pocket", pocket)):
        for k in ('x', 'one_hot', 'mask'):
            if not d[k].is_cuda:
                raise _lib.HipLibraryError(f"{what} needs device tensors ({name}['{k}'] is on {d[k].device}); "
                                           "there is no CPU fallback")
    return p.device


def _chunks(n_states, max_states):
    return [(g, min(max_states, n_states - g)) for g in range(0, n_states, max_states)]


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _plan(ddpm, ligand, pocket, n_times, times, weights, seed, ligand_ids, max_states, joint):
    """What both scorers do before their first launch: every refusal, the inputs as the kernels read them, the state
    list with the rows and the edge bound of every chunk, and the one upload of t and w.  -> namespace of the names
    assigned below."""
    table = 2 if joint else 0          # DistributionNodes._table: log p(N_lig, N_pocket) / log p(N_lig | N_pocket)
    # ---- refusals: everything before the first launch
    _check_model(ddpm, joint)
    if int(max_states) < 1:
        raise ValueError("max_states must be at least 1")
    nl, npk = _check_batch(ddpm, ligand, pocket, table)
    B, T = len(nl), int(ddpm.T)
    t_bk, w_bk = _slots(T, B, n_times, times, weights, seed)
    K = t_bk.shape[1]
    S = K + 1                                                        # slots per ligand: the zero slot is the last
    n_states = B * S
    ids = list(range(B)) if ligand_ids is None else [int(v) for v in torch.as_tensor(ligand_ids).reshape(-1).tolist()]
    if len(ids) != B or any(i < 0 for i in ids) or (max(ids) + 1) * S >= 2 ** 32:
        raise ValueError(f"ligand_ids needs {B} non-negative entries with ligand_id * (K + 1) below 2^32")
    chunks = _chunks(n_states, int(max_states))
    if ddpm.noise_source is not None and len(chunks) > 1:
        raise ValueError(f"injected noise needs a single chunk: {n_states} states for max_states = {max_states}")
    dev = _on_device(ddpm, ligand, pocket, "nll_of_complex" if joint else "nll_given_pocket")

    # ---- inputs as the kernels read them (no copy when they already are float32 / int64 and contiguous)
    lib = _lib.load()
    f32 = dict(dtype=torch.float32, device=dev)
    lx = ligand['x'].detach().to(**f32).contiguous()
    lh = ligand['one_hot'].detach().to(**f32).contiguous()
    px = pocket['x'].detach().to(**f32).contiguous()
    ph = pocket['one_hot'].detach().to(**f32).contiguous()
    lm = ligand['mask'].detach().to(device=dev, dtype=torch.int64).contiguous()
    pm = pocket['mask'].detach().to(device=dev, dtype=torch.int64).contiguous()
    a, r = lh.shape[1], ph.shape[1]
    ldl, ldp = 3 + a, 3 + r
    tab = ddpm.size_distribution._table(table, dev).to(torch.float32).contiguous()
    cfg = _lib.LossCfg(batch=B, n_lig=lx.shape[0], n_pocket=px.shape[0], atom_nf=a, residue_nf=r, timesteps=T,
                       remove_com=0 if joint else int(bool(ddpm._remove_com)), vnode_idx=-1,
                       norm_value_x=float(ddpm.norm_values[0]), norm_value_h=float(ddpm.norm_values[1]),
                       norm_bias_h=float(ddpm.norm_biases[1]), n1_tab=tab.shape[0], n2_tab=tab.shape[1])
    gamma_table = ddpm.gamma.gamma.detach().to(**f32).contiguous()

    # ---- the state list, on the host: rows and edge bound of every chunk; one upload of t, w and the noise keys
    st_nl, st_np = np.repeat(np.asarray(nl, np.int64), S), np.repeat(np.asarray(npk, np.int64), S)
    seg = lambda v: (v + 31) // 32 * 32
    st_cap = seg(st_nl * (st_nl + st_np)) + seg(st_np * (st_nl + st_np))          # engine.edge_capacity, per state
    rows_l = [int(st_nl[g:g + n].sum()) for g, n in chunks]
    rows_p = [int(st_np[g:g + n].sum()) for g, n in chunks]
    caps = [int(st_cap[g:g + n].sum()) for g, n in chunks]
    cap_l, cap_p = max(rows_l), max(rows_p)
    meta = np.zeros((2, B, S), np.float32)
    meta[0, :, :K], meta[1, :, :K] = t_bk.numpy(), w_bk.numpy()
    meta_d = torch.from_numpy(meta.reshape(2, n_states)).to(dev)
    t_int, w_all = meta_d[0], meta_d[1]
    return SimpleNamespace(B=B, K=K, S=S, n_states=n_states, ids=ids, chunks=chunks, dev=dev, lib=lib, f32=f32, lx=lx, lh=lh,
                           px=px, ph=ph, lm=lm, pm=pm, ldl=ldl, ldp=ldp, tab=tab, cfg=cfg, gamma_table=gamma_table, nl=nl,
                           npk=npk, st_nl=st_nl, st_np=st_np, rows_l=rows_l, rows_p=rows_p, caps=caps, cap_l=cap_l,
                           cap_p=cap_p, t_int=t_int, w_all=w_all)


@torch.no_grad()
def nll_given_pocket(ddpm, ligand, pocket, n_times=None, times=None, weights=None, seed=0, ligand_ids=None, max_states=64,
                     return_terms=False):
    """`ConditionalDDPM.nll_given_pocket` (see the module docstring).  `ligand` / `pocket`: the un-normalised dicts of
    `forward` ('x', 'one_hot', 'size', 'mask'), pocket b belongs to ligand b; they are not modified.  `n_times` (default 10,
    at most T) or `times` ('all', or integers in 1..T of shape [K] or [B, K]) select the time slots, `weights` ([K] or
    [B, K], default T / K for explicit times) their weights.  `ligand_ids` (default 0..B-1) key the noise.
    -> nll float32 [B] on the device; with `return_terms` also a dict: t, weight, SNR_weight, error_t [B, K] and loss_t,
    loss_0_x, loss_0_h, neg_log_constants, kl_prior, delta_log_px, log_pN [B]."""
    p = _plan(ddpm, ligand, pocket, n_times, times, weights, seed, ligand_ids, max_states, joint=False)
    B, K, S, n_states, ids, chunks, dev, lib, f32 = p.B, p.K, p.S, p.n_states, p.ids, p.chunks, p.dev, p.lib, p.f32
    lx, lh, px, ph, lm, pm, ldl, ldp, tab, cfg, gamma_table = (p.lx, p.lh, p.px, p.ph, p.lm, p.pm, p.ldl, p.ldp, p.tab, p.cfg,
                                                               p.gamma_table)
    nl, st_nl, rows_l, rows_p, caps, cap_l, cap_p, t_int, w_all = (p.nl, p.st_nl, p.rows_l, p.rows_p, p.caps, p.cap_l, p.cap_p,
                                                                   p.t_int, p.w_all)
    keyed = ddpm.noise_source is None
    if keyed:
        keys = torch.from_numpy((np.asarray(ids, np.int64)[:, None] * S + np.arange(S, dtype=np.int64)[None, :]).reshape(-1))
        row_state = torch.from_numpy(np.repeat(np.arange(n_states, dtype=np.int64), st_nl))     # state of every ligand row
        keys, row_state = keys.to(dev), row_state.to(dev)
        row_first = np.concatenate([[0], np.cumsum(st_nl)])
        eps = torch.empty(cap_l, ldl, **f32)
    else:
        # one draw per slot over the whole ligand batch, gathered into the state order (single chunk)
        draws = torch.stack([ddpm.noise_source((lx.shape[0], ldl)).to(**f32) for _ in range(S)])      # [S, N_lig, ldl]
        off = np.concatenate([[0], np.cumsum(nl)])
        src = np.concatenate([k * lx.shape[0] + np.arange(off[b], off[b + 1]) for b in range(B) for k in range(S)])
        eps = draws.reshape(S * lx.shape[0], ldl)[torch.from_numpy(src).to(dev)].contiguous()

    # ---- per-chunk arrays, sized for the largest chunk and reused (stream order keeps the chunks apart)
    z = torch.empty(cap_l, ldl, **f32)
    xh_pocket = torch.empty(cap_p, ldp, **f32)
    net = torch.empty(cap_l, ldl, **f32)
    mask_l = torch.empty(cap_l, dtype=torch.int64, device=dev)
    mask_p = torch.empty(cap_p, dtype=torch.int64, device=dev)
    t_state = torch.empty(max(n for _, n in chunks), **f32)
    ps = torch.empty(lib.dsbdd_score_rows(0), n_states, **f32)
    pl = torch.empty(lib.dsbdd_score_rows(1), B, **f32)
    out = torch.empty(lib.dsbdd_score_rows(2), B, **f32)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    # the engine's workspace for the largest chunk, once (growing it in the middle of the call would synchronise)
    ddpm.dynamics.engine().ensure_workspace(cap_l, cap_p, max(n for _, n in chunks), max(caps))
    stream = _stream(dev)
    for (g0, n), n_l, n_p, cap in zip(chunks, rows_l, rows_p, caps):
        if keyed:
            r0 = int(row_first[g0])
            _lib.check(lib.dsbdd_randn_keyed(stream, eps.data_ptr(), row_state.data_ptr() + 8 * r0, n_l, ldl, n_states, 0,
                                             keys.data_ptr(), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint64(0),
                                             NOISE_STREAM), "dsbdd_randn_keyed")
        _lib.check(lib.dsbdd_score_cond_pre(stream, C.byref(cfg), S, g0, n, cap_l, cap_p, lx.data_ptr(), lh.data_ptr(),
                                            lm.data_ptr(), px.data_ptr(), ph.data_ptr(), pm.data_ptr(), eps.data_ptr(),
                                            t_int.data_ptr(), gamma_table.data_ptr(), tab.data_ptr(), z.data_ptr(),
                                            xh_pocket.data_ptr(), mask_l.data_ptr(), mask_p.data_ptr(), t_state.data_ptr(),
                                            ps.data_ptr(), pl.data_ptr()), "dsbdd_score_cond_pre")
        ddpm.dynamics.forward_async(z[:n_l], xh_pocket[:n_p], t_state[:n], mask_l[:n_l], mask_p[:n_p], status=status,
                                    want_pocket=False, eps_lig=net[:n_l], batch=n, edge_cap=cap)
        _lib.check(lib.dsbdd_score_cond_post(stream, C.byref(cfg), S, g0, n, cap_l, cap_p, lh.data_ptr(), lm.data_ptr(),
                                             pm.data_ptr(), net.data_ptr(), eps.data_ptr(), z.data_ptr(), ps.data_ptr()),
                   "dsbdd_score_cond_post")
    _lib.check(lib.dsbdd_score_reduce(stream, B, S, w_all.data_ptr(), ps.data_ptr(), pl.data_ptr(), out.data_ptr()),
               "dsbdd_score_reduce")
    ddpm._check_status(status)                                       # the one host synchronisation of the call
    nll = out[0]
    if not return_terms:
        return nll
    per_state = ps.view(-1, B, S)
    names_s = {"SNR_weight": 4, "error_t": 5}                        # rows SS_SNR_W, SS_ERR_T of csrc/score.h
    terms = {"t": t_int.view(B, S)[:, :K].contiguous(), "weight": w_all.view(B, S)[:, :K].contiguous()}
    terms.update({k: per_state[i, :, :K].contiguous() for k, i in names_s.items()})
    terms.update({k: out[i] for i, k in enumerate(("nll", "loss_t", "loss_0_x", "loss_0_h", "neg_log_constants", "kl_prior",
                                                   "delta_log_px", "log_pN")) if k != "nll"})
    return nll, terms


# --------------------------------------------------------------------------- the joint model
def combine_terms_joint(weight, SNR_weight, error_t_lig, error_t_pocket, loss_0_x_ligand, loss_0_x_pocket, loss_0_h,
                        neg_log_constants, kl_prior, delta_log_px, log_pN):
    """The combination `dsbdd_score_joint_reduce` does on the device, in torch (float32, the same order): weight /
    SNR_weight / error_t_lig / error_t_pocket are [B, K] (K = 1 may be given as [B]), the other terms [B].
    -> (nll [B], loss_t [B], loss_t_lig [B]); loss_t_lig is loss_t's sum over error_t_lig alone."""
    f = lambda v: torch.as_tensor(v).to(torch.float32)
    SNR_weight, e_l, e_p = f(SNR_weight), f(error_t_lig), f(error_t_pocket)
    if e_l.dim() == 1:                                               # K = 1 given as [B]
        SNR_weight, e_l, e_p = SNR_weight.reshape(-1, 1), e_l.reshape(-1, 1), e_p.reshape(-1, 1)
    weight = f(weight).to(e_l.device)
    if weight.dim() == 1 and e_l.shape[1] == 1 and weight.numel() == e_l.shape[0]:
        weight = weight.reshape(-1, 1)
    weight = torch.broadcast_to(weight, e_l.shape)
    loss_t = torch.zeros(e_l.shape[0], dtype=torch.float32, device=e_l.device)
    loss_t_lig = torch.zeros_like(loss_t)
    for k in range(e_l.shape[1]):
        coef = (-0.5 * weight[:, k]) * SNR_weight[:, k]
        loss_t = loss_t + coef * (e_l[:, k] + e_p[:, k])
        loss_t_lig = loss_t_lig + coef * e_l[:, k]
    loss_0 = ((f(loss_0_x_ligand) + f(loss_0_x_pocket)) + f(loss_0_h)) + f(neg_log_constants)
    nll = (((loss_t + loss_0) + f(kl_prior)) - f(delta_log_px)) - f(log_pN)
    return nll, loss_t, loss_t_lig


@torch.no_grad()
def nll_of_complex(ddpm, ligand, pocket, n_times=None, times=None, weights=None, seed=0, ligand_ids=None, max_states=64,
                   center=True, return_terms=False):
    """`EnVariationalDiffusion.nll_of_complex`: the joint model's negative log-likelihood bound of GIVEN ligand-pocket
    complexes, -log p(ligand, pocket) -- the estimator of the module docstring for the model that noises and scores both
    node sets (the evaluation branch of `EnVariationalDiffusion.forward`).  Arguments as for `nll_given_pocket`.

    `center` (default True) subtracts the complex's mean over ligand + pocket rows first, on the device.  The joint
    `forward` never centres; dataset.py centres every training complex, and the bound is not translation invariant
    (kl_prior carries alpha_T^2 |x|^2 of the absolute coordinates, and float32 coordinates tens of Angstrom from the origin
    lose digits before the network sees their differences), so raw PDB coordinates must be centred to be scored as the
    model was trained.  `center=False` scores the coordinates as given (already centred data; parity with `forward`).

    Noise: state (ligand id i, slot k) draws its ligand block [n_lig][3 + atom_nf] on stream id `NOISE_STREAM_JOINT_LIG`
    and its pocket block [n_pocket][3 + residue_nf] on `NOISE_STREAM_JOINT_POCKET` (draw index 0, global sample id
    i (K + 1) + k); the kernel centres the coordinate part over both.  An injected `noise_source` is asked per slot in the
    reference's order -- (N_lig + N_pocket, 3), (N_lig, atom_nf), (N_pocket, residue_nf) -- time slots first, then the zero
    slot; it needs a single chunk.
    -> nll float32 [B] on the device; with `return_terms` also a dict: t, weight, SNR_weight, error_t_lig, error_t_pocket
    [B, K] and loss_t, loss_t_lig (loss_t's sum over error_t_lig alone), loss_0_x_ligand, loss_0_x_pocket, loss_0_h,
    neg_log_constants, kl_prior, delta_log_px, log_pN [B]."""
    p = _plan(ddpm, ligand, pocket, n_times, times, weights, seed, ligand_ids, max_states, joint=True)
    B, K, S, n_states, chunks, dev, lib, f32, ldl, ldp = p.B, p.K, p.S, p.n_states, p.chunks, p.dev, p.lib, p.f32, p.ldl, p.ldp
    cap_l, cap_p = p.cap_l, p.cap_p
    n_lig, n_poc = p.lx.shape[0], p.px.shape[0]
    keyed = ddpm.noise_source is None
    if keyed:
        keys = torch.from_numpy((np.asarray(p.ids, np.int64)[:, None] * S + np.arange(S, dtype=np.int64)[None, :]).reshape(-1))
        states = np.arange(n_states, dtype=np.int64)
        # state of every ligand row, then of every pocket row (one upload)
        row_state = torch.from_numpy(np.concatenate([np.repeat(states, p.st_nl), np.repeat(states, p.st_np)])).to(dev)
        keys = keys.to(dev)
        first_l, first_p = np.concatenate([[0], np.cumsum(p.st_nl)]), np.concatenate([[0], np.cumsum(p.st_np)])
        pocket_rows = int(first_l[-1])                               # offset of the pocket part of row_state
        noise_l, noise_p = torch.empty(cap_l, ldl, **f32), torch.empty(cap_p, ldp, **f32)
    else:
        # per slot the reference's three draws over the whole batch, gathered into the state order (single chunk)
        draws_l, draws_p = [], []
        for _ in range(S):
            zx = ddpm.noise_source((n_lig + n_poc, 3)).to(**f32)
            draws_l.append(torch.cat([zx[:n_lig], ddpm.noise_source((n_lig, ldl - 3)).to(**f32)], dim=1))
            draws_p.append(torch.cat([zx[n_lig:], ddpm.noise_source((n_poc, ldp - 3)).to(**f32)], dim=1))

        def gather(draws, sizes, n_rows):
            off = np.concatenate([[0], np.cumsum(sizes)])
            src = np.concatenate([k * n_rows + np.arange(off[b], off[b + 1]) for b in range(B) for k in range(S)])
            return torch.cat(draws)[torch.from_numpy(src).to(dev)].contiguous()
        noise_l, noise_p = gather(draws_l, p.nl, n_lig), gather(draws_p, p.npk, n_poc)

    # ---- per-chunk arrays, sized for the largest chunk and reused (stream order keeps the chunks apart)
    eps_l, z_l, net_l = (torch.empty(cap_l, ldl, **f32) for _ in range(3))
    eps_p, z_p, net_p = (torch.empty(cap_p, ldp, **f32) for _ in range(3))
    mask_l = torch.empty(cap_l, dtype=torch.int64, device=dev)
    mask_p = torch.empty(cap_p, dtype=torch.int64, device=dev)
    t_state = torch.empty(max(n for _, n in chunks), **f32)
    ps = torch.empty(lib.dsbdd_score_joint_rows(0), n_states, **f32)
    pl = torch.empty(lib.dsbdd_score_joint_rows(1), B, **f32)
    out = torch.empty(lib.dsbdd_score_joint_rows(2), B, **f32)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    # the engine's workspace for the largest chunk, once (growing it in the middle of the call would synchronise)
    ddpm.dynamics.engine().ensure_workspace(cap_l, cap_p, max(n for _, n in chunks), max(p.caps))
    stream = _stream(dev)
    seed64 = C.c_uint64(int(seed) & (2 ** 64 - 1))
    for (g0, n), n_l, n_p, cap in zip(chunks, p.rows_l, p.rows_p, p.caps):
        if keyed:
            for noise, r0, rows, ld, sid in ((noise_l, int(first_l[g0]), n_l, ldl, NOISE_STREAM_JOINT_LIG),
                                             (noise_p, pocket_rows + int(first_p[g0]), n_p, ldp, NOISE_STREAM_JOINT_POCKET)):
                if rows:
                    _lib.check(lib.dsbdd_randn_keyed(stream, noise.data_ptr(), row_state.data_ptr() + 8 * r0, rows, ld, n_states,
                                                     0, keys.data_ptr(), seed64, C.c_uint64(0), sid), "dsbdd_randn_keyed")
        _lib.check(lib.dsbdd_score_joint_pre(stream, C.byref(p.cfg), S, g0, n, cap_l, cap_p, int(bool(center)), p.lx.data_ptr(),
                                             p.lh.data_ptr(), p.lm.data_ptr(), p.px.data_ptr(), p.ph.data_ptr(), p.pm.data_ptr(),
                                             noise_l.data_ptr(), noise_p.data_ptr(), p.t_int.data_ptr(),
                                             p.gamma_table.data_ptr(), p.tab.data_ptr(), eps_l.data_ptr(), eps_p.data_ptr(),
                                             z_l.data_ptr(), z_p.data_ptr(), mask_l.data_ptr(), mask_p.data_ptr(),
                                             t_state.data_ptr(), ps.data_ptr(), pl.data_ptr()), "dsbdd_score_joint_pre")
        ddpm.dynamics.forward_async(z_l[:n_l], z_p[:n_p], t_state[:n], mask_l[:n_l], mask_p[:n_p], status=status,
                                    want_pocket=True, eps_lig=net_l[:n_l], eps_pocket=net_p[:n_p], batch=n, edge_cap=cap)
        _lib.check(lib.dsbdd_score_joint_post(stream, C.byref(p.cfg), S, g0, n, cap_l, cap_p, p.lh.data_ptr(), p.lm.data_ptr(),
                                              p.ph.data_ptr(), p.pm.data_ptr(), net_l.data_ptr(), net_p.data_ptr(),
                                              eps_l.data_ptr(), eps_p.data_ptr(), z_l.data_ptr(), z_p.data_ptr(), ps.data_ptr()),
                   "dsbdd_score_joint_post")
    _lib.check(lib.dsbdd_score_joint_reduce(stream, B, S, p.w_all.data_ptr(), ps.data_ptr(), pl.data_ptr(), out.data_ptr()),
               "dsbdd_score_joint_reduce")
    ddpm._check_status(status)                                       # the one host synchronisation of the call
    nll = out[0]
    if not return_terms:
        return nll
    per_state = ps.view(-1, B, S)
    names_s = {"SNR_weight": 4, "error_t_lig": 5, "error_t_pocket": 6}        # rows SJ_SNR_W, SJ_ERR_LIG, SJ_ERR_POC
    names_o = ("nll", "loss_t", "loss_t_lig", "loss_0_x_ligand", "loss_0_x_pocket", "loss_0_h", "neg_log_constants",
               "kl_prior", "delta_log_px", "log_pN")                              # rows SJO_* of csrc/score_joint.h
    terms = {"t": p.t_int.view(B, S)[:, :K].contiguous(), "weight": p.w_all.view(B, S)[:, :K].contiguous()}
    terms.update({k: per_state[i, :, :K].contiguous() for k, i in names_s.items()})
    terms.update({k: out[i] for i, k in enumerate(names_o) if k != "nll"})
    return nll, terms


# --------------------------------------------------------------------------- command line
def main(argv=None):
    """`python -m diffsbdd_amd.score --checkpoint CKPT --pdbfile P --ligands L.sdf (--ref_ligand R | --resi_list ...) --out
    scores.csv`: one row per molecule of the SDF file, in input order.  A joint checkpoint is scored by `nll_of_complex`
    and writes the extra column loss_t_lig."""
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--pdbfile", required=True)
    ap.add_argument("--ligands", required=True, help="SDF file with the molecules to score")
    where = ap.add_mutually_exclusive_group(required=True)
    where.add_argument("--ref_ligand", default=None)
    where.add_argument("--resi_list", nargs="+", default=None)
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--n_times", type=int, default=DEFAULT_N_TIMES)
    how.add_argument("--all_times", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max_states", type=int, default=64)
    ap.add_argument("--out", required=True)
    ap.add_argument("--trusted-checkpoint", action="store_true", help="allow a full unpickle of the checkpoint file")
    a = ap.parse_args(argv)
    from .generate import LigandGenerator
    gen = LigandGenerator.from_checkpoint(a.checkpoint, device="cuda", trusted=a.trusted_checkpoint)
    rows = gen.score_ligands(a.pdbfile, a.ligands, pocket_ids=a.resi_list, ref_ligand=a.ref_ligand,
                             n_times="all" if a.all_times else a.n_times, seed=a.seed, max_states=a.max_states)
    cols = ("nll", "loss_t", "loss_0", "kl_prior", "log_pN", "n_atoms")
    if rows and "loss_t_lig" in rows[0]:                             # a joint checkpoint: the ligand rows' share of loss_t
        cols = cols[:2] + ("loss_t_lig",) + cols[2:]
    with open(a.out, "w") as f:
        f.write("index," + ",".join(cols) + "\n")
        for i, row in enumerate(rows):
            f.write(f"{i}," + ",".join(str(row[c]) if c == "n_atoms" else repr(float(row[c])) for c in cols) + "\n")
    print(f"wrote {len(rows)} scores to {a.out}")


if __name__ == "__main__":
    main()
