"""Plain torch restatement of the six scoring entry points of include/diffsbdd_hip.h (dsbdd_score_cond_pre / _post /
_reduce and dsbdd_score_joint_pre / _post / _reduce), written from the header's two "likelihood bound" blocks and from
tests/_loss64.py -- not from csrc/score*.h and not from diffsbdd_amd/score.py -- for tests/test_score_restatement.py (which
pins it to oracle/ddpm_oracle.py on the CPU) and tests/test_gpu_score_kernels.py.  No GPU code.

The construction: a call with B ligands and n_slots = K + 1 slots IS the loss head on an expanded batch of B * n_slots
samples.  Sample g = b * n_slots + k is ligand b with its pocket, t_int = t[b][k] for k < K and 0 for the zero slot; since
states are ligand-major, row P(g) of the header is sample g's first row in the expanded batch, and a chunk's arrays are the
contiguous slice [P(first), P(first + n)) of the expanded arrays.  The draws (eps, noise_*, net_*) are made directly in
expanded layout.  With t_int = 0 the training-mode L0 terms of the loss head (evaluated on z_t, selected by [t = 0]) are
the evaluation branch's separate pass at t = 0.

Every function takes a dtype: float64 is the reference, float32 the yardstick (`err_ref` of tests/_steps64.py: within).
"""
import torch

from tests import _loss64 as l64
from tests._loss64 import within, within_at
from tests._steps64 import offsets

F64, F32 = torch.float64, torch.float32

MODELS = ("cond", "simple", "joint0", "joint1")       # remove_com = 1, remove_com = 0, the joint model with center 0 / 1
STATE_ROWS = {"cond": ("t", "gamma_t", "alpha_t", "sigma_t", "SNR_weight", "error_t", "loss_0_x", "loss_0_h"),
              "joint": ("t", "gamma_t", "alpha_t", "sigma_t", "SNR_weight", "error_t_lig", "error_t_pocket", "loss_0_x_ligand",
                        "loss_0_x_pocket", "loss_0_h")}
PRE_ROWS = ("t", "gamma_t", "alpha_t", "sigma_t", "SNR_weight")
LIGAND_ROWS = ("kl_prior", "neg_log_constants", "delta_log_px", "log_pN")
OUT_ROWS = {"cond": ("nll", "loss_t", "loss_0_x", "loss_0_h", "neg_log_constants", "kl_prior", "delta_log_px", "log_pN"),
            "joint": ("nll", "loss_t", "loss_t_lig", "loss_0_x_ligand", "loss_0_x_pocket", "loss_0_h", "neg_log_constants",
                      "kl_prior", "delta_log_px", "log_pN")}
TENSORS = {"cond": ("z", "xh_pocket"), "joint": ("eps_lig", "eps_poc", "z_lig", "z_poc")}
LIG_TENSORS = ("z", "eps_lig", "z_lig")               # the others have pocket rows


def family(model):
    return "joint" if model.startswith("joint") else "cond"


# ---- the expanded batch -------------------------------------------------------------------------------------------------------
def expanded_sizes(sizes, n_slots):
    return [int(n) for n in sizes for _ in range(n_slots)]


def expanded_rows(sizes, n_slots):
    """Caller row of every row of the expanded batch (ligand b's rows, n_slots times, then ligand b + 1's)."""
    o = offsets(sizes)
    idx = [i for b in range(len(sizes)) for _ in range(n_slots) for i in range(o[b], o[b + 1])]
    return torch.tensor(idx, dtype=torch.int64)


def zero_slots(B, n_slots):
    return torch.arange(B * n_slots) % n_slots == n_slots - 1


def t_int_expanded(times, n_slots):
    """[B][K] -> [B * n_slots] with 0 on the zero slots."""
    B = times.shape[0]
    return torch.cat([times.float(), torch.zeros(B, 1)], 1).reshape(-1)


def size_lookup(logpn, n1, n2, dtype):
    """The size table WITHOUT a clamp (unlike the loss head): a size beyond the table has no log p(N): NaN."""
    inside = (n1 < logpn.shape[0]) & (n2 < logpn.shape[1])
    v = logpn.to(dtype)[n1.clamp(max=logpn.shape[0] - 1), n2.clamp(max=logpn.shape[1] - 1)]
    return torch.where(inside, v, torch.full_like(v, float("nan")))


def reference(case, model, dtype, logpn=None):
    """-> dict(tensors, per_state, per_ligand, t_out, kl_addend): pre and post of one model on the whole call (all states
    in one chunk), the post restatement fed with the pre restatement's outputs of the same dtype."""
    c, fam = case, family(model)
    B, n_slots = len(c["lsz"]), c["n_slots"]
    lsz_e, psz_e = expanded_sizes(c["lsz"], n_slots), expanded_sizes(c["psz"], n_slots)
    il, ip = expanded_rows(c["lsz"], n_slots), expanded_rows(c["psz"], n_slots)
    t_int = t_int_expanded(c["times"], n_slots)
    cfg = l64.cfg_of(c, remove_com=0 if model == "simple" else 1)
    logpn = c["logpn"] if logpn is None else logpn
    lig_x, poc_x = c["lig_x"].to(dtype), c["poc_x"].to(dtype)
    if model == "joint1":               # center: the complex's mean over ligand + pocket rows, in this dtype
        lm, pm = l64.mask_of(c["lsz"]), l64.mask_of(c["psz"])
        m = l64.seg_mean3(torch.cat([lig_x, poc_x]), torch.cat([lm, pm]), B, torch.tensor(c["lsz"]) + torch.tensor(c["psz"]))
        lig_x, poc_x = lig_x - m[lm], poc_x - m[pm]
    if fam == "joint":
        pre = l64.joint_pre(cfg, lig_x[il], c["lig_h"][il], poc_x[ip], c["poc_h"][ip], lsz_e, psz_e, c["eps"], c["noise_poc"],
                            t_int, dtype)
        ps = pre["per_sample"]
        post = l64.joint_post(cfg, c["net_lig"], c["net_poc"], pre["eps_lig"], pre["eps_poc"], pre["z_lig"], lsz_e, psz_e,
                              ps["alpha_t"], ps["sigma_t"], ps["t_is_zero"], dtype)["out"]
        tensors = {k: pre[k] for k in TENSORS["joint"]}
    else:
        pre = l64.cond_pre(cfg, lig_x[il], c["lig_h"][il], poc_x[ip], c["poc_h"][ip], lsz_e, psz_e, c["eps"], t_int, dtype)
        ps = pre["per_sample"]
        post = l64.cond_post(cfg, c["net_lig"], c["eps"], pre["z_t"], c["lig_h"][il], lsz_e, ps["alpha_t"], ps["sigma_t"],
                             ps["t_is_zero"], dtype)["out"]
        tensors = dict(z=pre["z_t"], xh_pocket=pre["xh_pocket"])
    zs = zero_slots(B, n_slots)
    per_state = {k: ps[k] for k in ("t", "gamma_t", "alpha_t", "sigma_t")}
    per_state["SNR_weight"] = torch.where(zs, torch.zeros_like(ps["SNR_weight"]), ps["SNR_weight"])
    for k in STATE_ROWS[fam][5:-1]:
        per_state[k] = post[k]            # error_t*: x [t > 0], loss_0_x*: x [t = 0] by the post restatement
    per_state["loss_0_h"] = ps["loss_0_h"]
    per_ligand = {k: ps[k][0::n_slots] for k in ("kl_prior", "neg_log_constants", "delta_log_px")}
    per_ligand["log_pN"] = size_lookup(logpn, torch.tensor(c["lsz"]), torch.tensor(c["psz"]), dtype)
    return dict(tensors=tensors, per_state=per_state, per_ligand=per_ligand, t_out=ps["t"], kl_addend=pre["kl_addend"])


def reduce(model, per_state, per_ligand, weights, dtype):
    """dsbdd_score_reduce / _joint_reduce -> dict named by OUT_ROWS (+ "addend": the largest addend of nll over the
    ligands whose nll is finite).  weights [B][K]; float32: the documented order -- k ascending, ((-0.5 w) SNR_weight)
    error_t, every operation rounded on its own, then the left-to-right sum of nll."""
    fam = family(model)
    st = {k: torch.as_tensor(v).detach().cpu().to(dtype) for k, v in per_state.items()}
    pl = {k: torch.as_tensor(v).detach().cpu().to(dtype) for k, v in per_ligand.items()}
    w = weights.to(dtype)
    B, K = w.shape
    n_slots = K + 1
    col = lambda name, k: st[name].reshape(B, n_slots)[:, k]
    loss_t, loss_t_lig = torch.zeros(B, dtype=dtype), torch.zeros(B, dtype=dtype)
    addends = []
    for k in range(K):
        coef = (-0.5 * w[:, k]) * col("SNR_weight", k)
        if fam == "joint":
            term, term_lig = coef * (col("error_t_lig", k) + col("error_t_pocket", k)), coef * col("error_t_lig", k)
            loss_t_lig = loss_t_lig + term_lig
        else:
            term = coef * col("error_t", k)
        loss_t = loss_t + term
        addends.append(term)
    l0h, nlc = col("loss_0_h", K), pl["neg_log_constants"]
    if fam == "joint":
        l0xl, l0xp = col("loss_0_x_ligand", K), col("loss_0_x_pocket", K)
        loss_0 = ((l0xl + l0xp) + l0h) + nlc
        out = dict(loss_t_lig=loss_t_lig, loss_0_x_ligand=l0xl, loss_0_x_pocket=l0xp)
        addends += [l0xl, l0xp]
    else:
        l0x = col("loss_0_x", K)
        loss_0 = (l0x + l0h) + nlc
        out = dict(loss_0_x=l0x)
        addends += [l0x]
    nll = (((loss_t + loss_0) + pl["kl_prior"]) - pl["delta_log_px"]) - pl["log_pN"]
    out.update(nll=nll, loss_t=loss_t, loss_0_h=l0h, neg_log_constants=nlc, kl_prior=pl["kl_prior"],
               delta_log_px=pl["delta_log_px"], log_pN=pl["log_pN"])
    addends += [l0h, nlc, pl["kl_prior"], pl["delta_log_px"], pl["log_pN"]]
    finite = torch.isfinite(nll)
    big = torch.stack([a.abs() for a in addends])[:, finite]
    out = {k: out[k] for k in OUT_ROWS[fam]}
    out["addend"] = float(big.max()) if big.numel() else 0.0
    return out


# ---- the inputs of tests/test_gpu_score_kernels.py, seeded on the host --------------------------------------------------------
# a one-atom ligand (dof = 0), 257 rows = one more than the 256-thread stride, 300 rows = a second pass, an empty and a
# 257-row pocket; no empty ligand (dof < 0: not a defined input of this estimator)
MAIN = ([1, 7, 257, 23, 300], [300, 5, 0, 40, 257])
# sizes at the edge of a [12][60] table: n1_tab - 1, n1_tab; n2_tab - 1, n2_tab; and far beyond
BOUNDARY = ([11, 12, 11, 7, 257, 300], [59, 5, 60, 40, 0, 257])
# B = 130 tiny ligands: the third 64-thread block of the reduce kernels and its ragged end
TINY = ([1 + b % 3 for b in range(130)], [b % 4 for b in range(130)])
BATCHES = {"main": MAIN, "boundary": BOUNDARY, "tiny": TINY}
WIDTHS = ("crossdock_fullatom_cond", "crossdock_ca_cond", "moad_fullatom_joint", "odd", "odd_biased")
TABLES = ("polynomial_2/500/5e-4", "synthetic")
BIG_TABLE, SMALL_TABLE = (301, 301), (12, 60)


def times_of(T, B, K):
    """[B][K] integer times in [1, T]: K = T: every time; otherwise 1, T and interior values in every row, rotated by b so
    that every slot position sees all three kinds."""
    if K == T:
        return torch.arange(1, T + 1).float().repeat(B, 1)
    rows = []
    for b in range(B):
        base = [1, T, 2 + b % (T - 2), T - 1 - b % (T - 2)]
        rows.append([base[(k + b) % 4] for k in range(K)])
    return torch.tensor(rows, dtype=F32)


def make_case(batch, width, table, K, seed=0):
    """One set of float32 host inputs for all six entry points: the caller's batch, and the draws in expanded layout."""
    lsz, psz = BATCHES[batch]
    a, r, nv0, nv1, nb1 = l64.widths(width)
    gamma, T = l64.gamma_of(table)
    B, n_slots = len(lsz), K + 1
    g = torch.Generator().manual_seed(104729 * seed + 131 * WIDTHS.index(width) + 17 * TABLES.index(table) + K
                                      + 1009 * list(BATCHES).index(batch))
    lm, pm = l64.mask_of(lsz), l64.mask_of(psz)
    nl, npk = len(lm), len(pm)
    centre = (torch.rand(B, 3, generator=g) - 0.5) * 10.0 + torch.tensor([3.0, -4.0, 2.5])     # un-centred, a few Angstrom off
    lig_x = centre[lm] + torch.randn(nl, 3, generator=g) * 2.5 + 0.7
    poc_x = centre[pm] + torch.randn(npk, 3, generator=g) * 7.0
    lig_h = torch.nn.functional.one_hot(torch.randint(0, a, (nl,), generator=g), a).float()
    poc_h = torch.nn.functional.one_hot(torch.randint(0, r, (npk,), generator=g), r).float()
    ne, pe = nl * n_slots, npk * n_slots
    eps = torch.randn(ne, 3 + a, generator=g)               # the conditional model's draw = the joint model's ligand noise
    noise_poc = torch.randn(pe, 3 + r, generator=g)
    net_lig = eps + 0.3 * torch.randn(ne, 3 + a, generator=g)
    net_poc = noise_poc + 0.3 * torch.randn(pe, 3 + r, generator=g)
    weights = 0.5 + 7.5 * torch.rand(B, K, generator=g)
    logpn = -torch.rand(*BIG_TABLE, generator=g) * 9.0 - 0.5
    logpn_small = -torch.rand(*SMALL_TABLE, generator=g) * 9.0 - 0.5
    return dict(name=f"{batch}-{width}-{table}-K{K}", lsz=list(lsz), psz=list(psz), a=a, r=r, T=T, gamma=gamma, nv0=nv0,
                nv1=nv1, nb1=nb1, logpn=logpn, logpn_small=logpn_small, K=K, n_slots=n_slots, times=times_of(T, B, K),
                weights=weights, lig_x=lig_x, lig_h=lig_h, poc_x=poc_x, poc_h=poc_h, eps=eps, noise_poc=noise_poc,
                net_lig=net_lig, net_poc=net_poc, l0h_resolved=l64.l0h_resolved(table, nv1))


def slot_counts(table):
    """K per table: n_slots = 2 (the minimum) and 4; on the synthetic table also all T = 16 times (n_slots = 17)."""
    return (1, 3, l64.SYNTHETIC_T) if table == "synthetic" else (1, 3)


def case_grid(width):
    """The main batch on one feature-width / normalisation row: both tables x their slot counts."""
    return [make_case("main", width, table, K) for table in TABLES for K in slot_counts(table)]


def chunk_cases():
    """Chunking, capacity, repetition and composition: n_slots = 17 (chunks of 7 states without any slot 0) and 4."""
    return [make_case("main", "crossdock_fullatom_cond", "synthetic", l64.SYNTHETIC_T),
            make_case("main", "odd", "polynomial_2/500/5e-4", 3)]


def table_cases():
    return [make_case("main", "moad_fullatom_joint", "synthetic", 3), make_case("boundary", "odd", "polynomial_2/500/5e-4", 1)]


def tiny_case():
    return make_case("tiny", "crossdock_ca_cond", "synthetic", 2)


def gpu_cases():
    """Every case tests/test_gpu_score_kernels.py runs (it builds its cases through the functions above only)."""
    cases = [c for w in WIDTHS for c in case_grid(w)] + chunk_cases() + table_cases() + [tiny_case()]
    return {c["name"]: c for c in cases}


def sub_case(case, b):
    """Ligand b alone (B = 1): its own rows, the same times, weights and draws."""
    n_slots = case["n_slots"]
    lo, po = offsets(case["lsz"]), offsets(case["psz"])
    sl, sp = slice(lo[b], lo[b + 1]), slice(po[b], po[b + 1])
    el, ep = slice(n_slots * lo[b], n_slots * lo[b + 1]), slice(n_slots * po[b], n_slots * po[b + 1])
    sub = dict(case, lsz=[case["lsz"][b]], psz=[case["psz"][b]], times=case["times"][b:b + 1], weights=case["weights"][b:b + 1])
    for k in ("lig_x", "lig_h"):
        sub[k] = case[k][sl]
    for k in ("poc_x", "poc_h"):
        sub[k] = case[k][sp]
    for k in ("eps", "net_lig"):
        sub[k] = case[k][el]
    for k in ("noise_poc", "net_poc"):
        sub[k] = case[k][ep]
    return sub, el, ep


# ---- the comparison of both test files --------------------------------------------------------------------------------------
def l0h_block(case, values):
    """The loss_0_h entries the tolerance rule is applied to: all of them where the term is a float32 quantity
    (_loss64.l0h_resolved), otherwise without the zero slots (what remains is exactly 0 on both sides)."""
    values = torch.as_tensor(values).detach().cpu()
    return values if case["l0h_resolved"] else values[~zero_slots(len(case["lsz"]), case["n_slots"])]


def compare(tag, case, model, got, ref64, ref32, keep=None):
    """The tolerance rule on every output block of pre and post; `got` is shaped like reference()'s result (the kernels'
    outputs, or -- in the self-check -- the float32 restatement).  per_state `t` and t_out: the float32 restatement's bits.
    keep: the ligands whose log_pN is defined (a size beyond the table: NaN on every side, asserted here).
    -> {block: (err_ref, err)}."""
    fam, res = family(model), {}
    for k in TENSORS[fam]:
        res[k] = within(f"{tag}.{k}", got["tensors"][k], ref64["tensors"][k], ref32["tensors"][k])
    for k in STATE_ROWS[fam]:
        g, r64, r32 = got["per_state"][k], ref64["per_state"][k], ref32["per_state"][k]
        if k == "t":
            assert torch.equal(torch.as_tensor(g).cpu().float(), r32.float()), (tag, k)
        elif k == "loss_0_h":
            res[k] = within(f"{tag}.{k}", l0h_block(case, g), l0h_block(case, r64), l0h_block(case, r32))
        else:
            res[k] = within(f"{tag}.{k}", g, r64, r32)
    assert torch.equal(torch.as_tensor(got["t_out"]).cpu().float(), ref32["t_out"].float()), (tag, "t_out")
    for k in LIGAND_ROWS:
        g, r64, r32 = (torch.as_tensor(v[k]).detach().cpu() for v in (got["per_ligand"], ref64["per_ligand"], ref32["per_ligand"]))
        if k == "log_pN" and keep is not None:
            assert torch.equal(torch.isnan(g), ~keep) and torch.equal(torch.isnan(r32), ~keep), (tag, "log_pN beyond the table")
            g, r64, r32 = g[keep], r64[keep], r32[keep]
        if k == "kl_prior":
            res[k] = within_at(f"{tag}.{k}", g, r64, r32, ref64["kl_addend"])
        elif k == "neg_log_constants":
            res[k] = within_at(f"{tag}.{k}", g, r64, r32, float(r64.abs().max()))
        else:
            res[k] = within(f"{tag}.{k}", g, r64, r32)
    return res


def compare_reduce(tag, model, got, out64, out32, keep=None):
    """The tolerance rule on what _reduce computes (dicts named by OUT_ROWS): nll against the largest addend of the
    combination, loss_t (and loss_t_lig; same-sign addends) against their own magnitude.  The other rows are copies of
    per_state / per_ligand entries, compared there.  keep: the ligands whose nll is defined.  -> {"out." + row: ...}."""
    sel = (lambda v: torch.as_tensor(v).detach().cpu()) if keep is None else (lambda v: torch.as_tensor(v).detach().cpu()[keep])
    res = {"out.nll": within_at(f"{tag}.out.nll", sel(got["nll"]), sel(out64["nll"]), sel(out32["nll"]), out64["addend"])}
    for k in ("loss_t", "loss_t_lig")[:2 if family(model) == "joint" else 1]:
        res["out." + k] = within(f"{tag}.out.{k}", got[k], out64[k], out32[k])
    return res


def full_reference(case, model, logpn=None):
    """-> (ref64, ref32, out64, out32): both dtypes through pre, post and reduce."""
    r64, r32 = reference(case, model, F64, logpn), reference(case, model, F32, logpn)
    o64 = reduce(model, r64["per_state"], r64["per_ligand"], case["weights"], F64)
    o32 = reduce(model, r32["per_state"], r32["per_ligand"], case["weights"], F32)
    return r64, r32, o64, o32
