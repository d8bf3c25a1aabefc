"""The six loss-head kernels of csrc/loss_head.h, each through the C ABI and in isolation -- no network call, no trainer, no
model object -- against tests/_loss64.py, the float64 restatement of the header's contract that
tests/test_loss_restatement.py pins to oracle/ddpm_oracle.py on the CPU:

  * dsbdd_loss_cond_pre (remove_com 1 and 0) and dsbdd_loss_joint_pre: every output block; the `t` and [t = 0] rows exact;
    with the normalised-batch pointers and the size table NULL every other output keeps its bits and log_pN is 0;
  * dsbdd_loss_cond_post / _joint_post fed with the KERNEL's pre outputs, against the restatement fed with the float64 ones;
    error_t exactly 0 on t = 0 samples, loss_0_x exactly 0 on the others, per_sample unchanged;
  * dsbdd_loss_cond_post_backward (all eight present / absent combinations of g_err, g_l0x, g_hat) and _joint_post_backward
    (all present, all absent, each absent alone) against torch.autograd.grad through the float64 post restatement; the
    coordinates of virtual-atom rows exactly -g_hat sigma_t / alpha_t; one case per model beyond 1024 x 256 elements;
  * bitwise: a repeated call, and every sample evaluated alone (B = 1) against its rows and columns inside the batch.

Inputs (tests/_loss64.py: make_case): ragged batch [1, 7, 257, 23, 12, 300] / [300, 5, 0, 40, 257, 1], a batch with an empty
ligand and an empty pocket, four feature widths, the shipped normalisations and (5, 0.25, 0.5), the shipped gamma tables
and a synthetic one with gamma[0] = -2 where loss_0_h is ~ 1 per row, t_int with 0 / T / 1 / 13 / T - 1, all zero, and
without a zero (so that SNR_weight is measured against its own ~ 1e-2), a [12][60] size table that sizes 257 and 300
exceed, virtual atoms in every sample.  Every output buffer carries GUARD sentinel rows; inputs are checked unchanged.

Tolerance: tests/_steps64.py: within -- |hip - f64| <= max(2 err_ref, 4 ulp) of the block's largest magnitude and 1e-4 at
most, err_ref = the float32 restatement against the float64 one; kl_prior against its largest addend (_loss64.within_at).
No other constant.  The figures printed on the MI355X are in profiles/loss_head_error.md.
"""
import ctypes as C

import pytest
import torch

from tests import _loss64 as l64

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GUARD = 2
F64, F32 = torch.float64, torch.float32


def dev():
    return torch.device("cuda:0")


def lib_():
    from diffsbdd_amd import _lib
    return _lib, _lib.load()


def p(t):
    return None if t is None else t.data_ptr()


def up(t):
    """A device copy with GUARD sentinel rows behind it."""
    pad = torch.full((GUARD,) + tuple(t.shape[1:]), SENTINEL)
    return torch.cat([t.float(), pad]).contiguous().to(dev())


def sentinel(rows, *cols):
    return torch.full((rows + GUARD,) + cols, SENTINEL, device=dev())


def body(buf, n, what):
    assert (buf[n:] == SENTINEL).all(), (what, "guard rows written")
    return buf[:n]


class Dev:
    """One case on the device: inputs with guard rows, and the launches of one model."""

    def __init__(self, case, model):
        _lib, _ = lib_()
        self.c, self.model = case, model
        self.B, self.nl, self.np = len(case["lsz"]), sum(case["lsz"]), sum(case["psz"])
        self.a, self.r = case["a"], case["r"]
        self.inp = {k: up(case[k]) for k in ("lig_x", "lig_h", "poc_x", "poc_h", "eps", "noise_poc", "net_lig", "net_poc",
                                             "t_int", "gamma", "logpn")}
        self.inp.update({k: up(v) for k, v in case["cot"].items()})
        # (guard entries behind the masks too: a node set with no rows at all still has an address)
        self.inp["ml"], self.inp["mp"] = (torch.cat([l64.mask_of(s), torch.full((GUARD,), 2 ** 40)]).to(dev())
                                          for s in (case["lsz"], case["psz"]))
        self.before = {k: v.clone() for k, v in self.inp.items()}

    def cfg(self, vnode_idx=-1):
        from diffsbdd_amd import _lib
        c = self.c
        return _lib.LossCfg(self.B, self.nl, self.np, self.a, self.r, c["T"], 0 if self.model == "simple" else 1, vnode_idx,
                            c["nv0"], c["nv1"], c["nb1"], c["logpn"].shape[0], c["logpn"].shape[1])

    def inputs_unchanged(self):
        for k, v in self.inp.items():
            assert torch.equal(v, self.before[k]), (k, "input modified")

    # ---- launches: each returns what the restatement returns, as device tensors without their guard rows ----------------
    def pre(self, table=True, norm=True):
        _lib, lib = lib_()
        i, nl, npk, a, r = self.inp, self.nl, self.np, self.a, self.r
        rows = lib.dsbdd_loss_rows()
        assert rows == len(l64.PS_ROWS)
        ps = sentinel(rows, self.B)
        nb = dict(lig_xn=sentinel(nl, 3), lig_hn=sentinel(nl, a), poc_xn=sentinel(npk, 3), poc_hn=sentinel(npk, r))
        nptr = [p(nb[k]) if norm else None for k in ("lig_xn", "lig_hn", "poc_xn", "poc_hn")]
        cfg, tab = self.cfg(), p(i["logpn"]) if table else None
        if self.model == "joint":
            o = dict(eps_lig=sentinel(nl, 3 + a), eps_poc=sentinel(npk, 3 + r), z_lig=sentinel(nl, 3 + a),
                     z_poc=sentinel(npk, 3 + r))
            _lib.check(lib.dsbdd_loss_joint_pre(None, C.byref(cfg), p(i["lig_x"]), p(i["lig_h"]), p(i["ml"]), p(i["poc_x"]),
                                                p(i["poc_h"]), p(i["mp"]), p(i["eps"]), p(i["noise_poc"]), p(i["t_int"]),
                                                p(i["gamma"]), tab, p(o["eps_lig"]), p(o["eps_poc"]), p(o["z_lig"]),
                                                p(o["z_poc"]), p(ps), *nptr), "dsbdd_loss_joint_pre")
            n_of = dict(eps_lig=nl, eps_poc=npk, z_lig=nl, z_poc=npk)
        else:
            o = dict(z_t=sentinel(nl, 3 + a), xh_pocket=sentinel(npk, 3 + r))
            _lib.check(lib.dsbdd_loss_cond_pre(None, C.byref(cfg), p(i["lig_x"]), p(i["lig_h"]), p(i["ml"]), p(i["poc_x"]),
                                               p(i["poc_h"]), p(i["mp"]), p(i["eps"]), p(i["t_int"]), p(i["gamma"]), tab,
                                               p(o["z_t"]), p(o["xh_pocket"]), p(ps), *nptr), "dsbdd_loss_cond_pre")
            n_of = dict(z_t=nl, xh_pocket=npk)
        torch.cuda.synchronize()
        out = {k: body(v, n_of[k], k) for k, v in o.items()}
        for k, n in (("lig_xn", nl), ("lig_hn", nl), ("poc_xn", npk), ("poc_hn", npk)):
            if norm:
                out[k] = body(nb[k], n, k)
            else:
                assert (nb[k] == SENTINEL).all()
        out["ps"] = body(ps, rows, "per_sample")
        out["per_sample"] = {k: out["ps"][j] for j, k in enumerate(l64.PS_ROWS)}
        return out

    def post(self, pre, vnode_idx=-1):
        _lib, lib = lib_()
        i, cfg = self.inp, self.cfg(vnode_idx)
        ps0 = pre["ps"].clone()
        xh_hat = sentinel(self.nl, 3 + self.a)
        if self.model == "joint":
            names = l64.JOINT_OUT_ROWS
            assert lib.dsbdd_loss_joint_out_rows() == len(names)
            out = sentinel(len(names), self.B)
            _lib.check(lib.dsbdd_loss_joint_post(None, C.byref(cfg), p(i["net_lig"]), p(i["net_poc"]), p(pre["eps_lig"]),
                                                 p(pre["eps_poc"]), p(pre["z_lig"]), p(i["ml"]), p(i["mp"]), p(pre["ps"]),
                                                 p(xh_hat), p(out)), "dsbdd_loss_joint_post")
        else:
            names = l64.COND_OUT_ROWS
            assert lib.dsbdd_loss_out_rows() == len(names)
            out = sentinel(len(names), self.B)
            _lib.check(lib.dsbdd_loss_cond_post(None, C.byref(cfg), p(i["net_lig"]), p(i["eps"]), p(pre["z_t"]), p(i["lig_h"]),
                                                p(i["ml"]), p(pre["ps"]), p(xh_hat), p(out)), "dsbdd_loss_cond_post")
        torch.cuda.synchronize()
        assert torch.equal(pre["ps"], ps0), "per_sample modified by post"
        out = body(out, len(names), "out")
        return dict(xh_hat=body(xh_hat, self.nl, "xh_hat"), raw=out, out={k: out[j] for j, k in enumerate(names)})

    def backward(self, pre, present, vnode_idx=-1):
        _lib, lib = lib_()
        i, cfg = self.inp, self.cfg(vnode_idx)
        g = {k: (p(i[k]) if k in present else None) for k in l64.JOINT_COTANGENTS}
        d_lig = sentinel(self.nl, 3 + self.a)
        if self.model == "joint":
            d_poc = sentinel(self.np, 3 + self.r)
            _lib.check(lib.dsbdd_loss_joint_post_backward(
                None, C.byref(cfg), p(i["net_lig"]), p(i["net_poc"]), p(pre["eps_lig"]), p(pre["eps_poc"]), p(i["ml"]),
                p(i["mp"]), p(pre["ps"]), g["g_err"], g["g_err_poc"], g["g_l0x"], g["g_l0x_poc"], g["g_hat"], p(d_lig),
                p(d_poc)), "dsbdd_loss_joint_post_backward")
            torch.cuda.synchronize()
            return [body(d_lig, self.nl, "d_net_lig"), body(d_poc, self.np, "d_net_pocket")]
        _lib.check(lib.dsbdd_loss_cond_post_backward(None, C.byref(cfg), p(i["net_lig"]), p(i["eps"]), p(i["lig_h"]),
                                                     p(i["ml"]), p(pre["ps"]), g["g_err"], g["g_l0x"], g["g_hat"], p(d_lig)),
                   "dsbdd_loss_cond_post_backward")
        torch.cuda.synchronize()
        return [body(d_lig, self.nl, "d_net")]


def soft(failures, f, *a, **k):
    try:
        return f(*a, **k)
    except AssertionError as exc:
        failures.append(str(exc)[:300])


def vnodes(model):
    return (-1,) if model == "joint" else (2, -1)


def same_bits(x, y, what):
    for k in x:
        if isinstance(x[k], torch.Tensor):
            assert torch.equal(x[k], y[k]), (what, k)


# =========================================================================================================================
# pre and post
# =========================================================================================================================
def check_forward(case, model):
    D = Dev(case, model)
    tag = f"{case['name']}/{model}"
    pre = D.pre()
    tz = case["t_int"] == 0
    for v in vnodes(model):
        r64, r32 = l64.reference(case, model, F64, v), l64.reference(case, model, F32, v)
        post = D.post(pre, v)
        l64.compare_forward(f"{tag}/v{v}", case, model, pre, post, r64, r32)
        err = [post["out"][k].cpu() for k in post["out"] if k.startswith("error_t")]
        l0x = [post["out"][k].cpu() for k in post["out"] if k.startswith("loss_0_x")]
        assert all((e[tz] == 0).all() for e in err) and all((x[~tz] == 0).all() for x in l0x), (tag, "[t = 0] selection")
        post2 = D.post(pre, v)                                              # a repeated call: the same bits
        assert torch.equal(post2["xh_hat"], post["xh_hat"]) and torch.equal(post2["raw"], post["raw"]), (tag, "post repeats")
    # an empty segment reads and writes nothing: its per-sample rows are the restatement's (compared above), in float32
    # exactly where they are sums over no rows
    for b, (n_l, n_p) in enumerate(zip(case["lsz"], case["psz"])):
        if n_l == 0 and model != "joint":
            assert float(pre["per_sample"]["loss_0_h"][b]) == 0.0 and float(post["out"]["info_x"][b]) == 0.0
        if n_l == 0 and model == "joint":
            assert float(post["out"]["info_lig_x"][b]) == 0.0 and float(post["out"]["error_t_lig"][b]) == 0.0
        if n_p == 0 and model == "joint":
            assert float(post["out"]["info_pocket_x"][b]) == 0.0 and float(post["out"]["error_t_pocket"][b]) == 0.0
    # no size table, no normalised-batch outputs: log_pN is 0, everything else has the same bits (also: pre repeats)
    bare = D.pre(table=False, norm=False)
    for k, v in bare.items():
        if k in ("ps", "per_sample"):
            continue
        assert torch.equal(v, pre[k]), (tag, k, "changes with the optional pointers")
    for k in l64.PS_ROWS:
        if k == "log_pN":
            assert (bare["per_sample"][k] == 0).all(), (tag, "log_pN without a table")
        else:
            assert torch.equal(bare["per_sample"][k], pre["per_sample"][k]), (tag, k, "changes with the optional pointers")
    same_bits(D.pre(), pre, (tag, "pre repeats"))
    D.inputs_unchanged()


@pytest.mark.parametrize("width", list(l64.WIDTHS))
@pytest.mark.parametrize("model", l64.MODELS)
def test_pre_and_post_vs_float64_restatement(model, width):
    failures = []
    for case in l64.case_grid(width):
        soft(failures, check_forward, case, model)
    assert not failures, failures


def test_synthetic_table_makes_the_categorical_term_live():
    """On the synthetic table (resolved normalisations) the KERNEL's loss_0_h of every t = 0 sample with at least one row
    exceeds 0.1 per row as well: what is compared there is the term's arithmetic, not a rounded zero."""
    for model in ("cond", "joint"):
        for width in ("crossdock_fullatom_cond", "crossdock_ca_cond", "moad_fullatom_joint", "odd"):
            case = l64.make_case("ragged", width, "synthetic", "zeros")
            assert case["l0h_resolved"]
            got = Dev(case, model).pre()["per_sample"]["loss_0_h"].cpu()
            want = l64.reference(case, model, F64)[1]["per_sample"]["loss_0_h"]
            rows = torch.tensor(case["lsz"]) + (torch.tensor(case["psz"]) if model == "joint" else 0)
            print(f"  {case['name']}/{model}: loss_0_h per row  hip {(got / rows).tolist()}  f64 {(want / rows).tolist()}")
            assert float((want / rows).min()) > 0.1 and float((got / rows).min()) > 0.1


# =========================================================================================================================
# backward
# =========================================================================================================================
def check_backward(case, model, D=None, sets=None):
    D = D or Dev(case, model)
    tag = f"{case['name']}/{model}"
    pre = D.pre()
    lm = l64.mask_of(case["lsz"])
    for v in vnodes(model):
        r64, r32 = l64.reference(case, model, F64, v), l64.reference(case, model, F32, v)
        for present in sets or l64.cotangent_sets(model):
            b64 = l64.reference_backward(case, model, F64, r64[0], r64[1], present)
            b32 = l64.reference_backward(case, model, F32, r32[0], r32[1], present)
            got = D.backward(pre, present, v)
            l64.compare_backward(f"{tag}/v{v}.bwd[{'+'.join(present) or 'none'}]", got, b64, b32)
            if not present:
                assert all((g == 0).all() for g in got), (tag, "no cotangent: d_net is exactly 0")
            if v >= 0:
                # virtual-atom rows: the error terms do not reach their coordinates, only xh_hat's gradient does
                virt = l64._virtual_rows(r64[0], case["lig_h"], F64)
                assert virt.any()
                sig, alp = pre["per_sample"]["sigma_t"].cpu()[lm], pre["per_sample"]["alpha_t"].cpu()[lm]
                want = -(case["cot"]["g_hat"][:, :3] * sig[:, None] / alp[:, None]) if "g_hat" in present \
                    else torch.zeros(len(lm), 3)
                assert torch.equal(got[0].cpu()[virt, :3], want[virt]), (tag, present, "coordinates of virtual atoms")
            again = D.backward(pre, present, v)
            assert all(torch.equal(x, y) for x, y in zip(again, got)), (tag, "backward repeats")
    D.inputs_unchanged()


@pytest.mark.parametrize("width", list(l64.WIDTHS))
@pytest.mark.parametrize("model", ["cond", "joint"])
def test_post_backward_vs_autograd_through_float64_restatement(model, width):
    failures = []
    for case in l64.case_grid(width):
        if case["name"].endswith(l64.BACKWARD_T_MODE):
            soft(failures, check_backward, case, model)
    assert not failures, failures


@pytest.mark.parametrize("model", ["cond", "joint"])
def test_backward_grid_stride_second_pass(model):
    """More elements than 1024 workgroups x 256 threads cover in one pass; compared in full."""
    case = l64.big_case()
    n = sum(case["lsz"]) * (3 + case["a"]) + (sum(case["psz"]) * (3 + case["r"]) if model == "joint" else 0)
    assert sum(case["lsz"]) * (3 + case["a"]) > 1024 * 256 and n > 1024 * 256
    full = l64.JOINT_COTANGENTS if model == "joint" else l64.COND_COTANGENTS
    check_forward(case, model)
    check_backward(case, model, sets=[full, ("g_err",)])


# =========================================================================================================================
# batch composition
# =========================================================================================================================
def sub_case(case, b):
    """Sample b alone (B = 1) with the same rows, eps, t and net."""
    lo, po = l64.offsets(case["lsz"]), l64.offsets(case["psz"])
    sl, sp = slice(lo[b], lo[b + 1]), slice(po[b], po[b + 1])
    sub = dict(case, lsz=[case["lsz"][b]], psz=[case["psz"][b]], t_int=case["t_int"][b:b + 1])
    for k in ("lig_x", "lig_h", "eps", "net_lig"):
        sub[k] = case[k][sl]
    for k in ("poc_x", "poc_h", "noise_poc", "net_poc"):
        sub[k] = case[k][sp]
    sub["cot"] = {k: (v[sl] if k == "g_hat" else v[b:b + 1]) for k, v in case["cot"].items()}
    return sub, sl, sp


def check_composition(case, model):
    D = Dev(case, model)
    v = vnodes(model)[0]
    full = l64.JOINT_COTANGENTS if model == "joint" else l64.COND_COTANGENTS
    pre = D.pre()
    post, bwd = D.post(pre, v), D.backward(pre, full, v)
    for b in range(len(case["lsz"])):
        sub, sl, sp = sub_case(case, b)
        what = (case["name"], model, b, "depends on the batch")
        S = Dev(sub, model)
        s_pre = S.pre()
        s_post, s_bwd = S.post(s_pre, v), S.backward(s_pre, full, v)
        assert torch.equal(s_pre["ps"][:, 0], pre["ps"][:, b]), what + ("per_sample",)
        assert torch.equal(s_post["raw"][:, 0], post["raw"][:, b]), what + ("out",)
        for k in l64.PRE_TENSORS[model]:
            rows = sl if k in ("z_t", "eps_lig", "z_lig", "lig_xn", "lig_hn") else sp
            assert torch.equal(s_pre[k], pre[k][rows]), what + (k,)
        assert torch.equal(s_post["xh_hat"], post["xh_hat"][sl]), what + ("xh_hat",)
        assert torch.equal(s_bwd[0], bwd[0][sl]), what + ("d_net",)
        if model == "joint":
            assert torch.equal(s_bwd[1], bwd[1][sp]), what + ("d_net_pocket",)


@pytest.mark.parametrize("width", list(l64.WIDTHS))
@pytest.mark.parametrize("model", l64.MODELS)
def test_each_sample_alone_has_the_bits_it_has_in_the_batch(model, width):
    """One workgroup per sample with fixed-order sums: nothing leaks across a segment boundary."""
    failures = []
    for batch in l64.BATCHES:
        for table in ("polynomial_2/500/5e-4", "synthetic"):
            soft(failures, check_composition, l64.make_case(batch, width, table, "mixed"), model)
    assert not failures, failures
