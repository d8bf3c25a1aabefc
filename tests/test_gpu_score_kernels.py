"""The six scoring kernels of csrc/score.h and csrc/score_joint.h, each through the C ABI and in isolation -- no network call,
no model object -- against tests/_score64.py, the float64 restatement of the header's contract that
tests/test_score_restatement.py pins to oracle/ddpm_oracle.py on the CPU:

  * dsbdd_score_cond_pre (remove_com 1 and 0) and dsbdd_score_joint_pre (center 0 and 1): every output block by the rule;
    per_state `t` and t_out with the float32 restatement's bits; both masks exactly the chunk-local state id of every row;
    per_ligand written exactly for the ligands whose slot 0 lies in the chunk; SNR_weight of zero slots exactly 0; t_int and
    weights of zero slots hold NaN ("not read") and changing them changes no bit;
  * _post fed with the KERNEL's pre outputs, against the restatement fed with the float64 ones; error_t* exactly 0 on zero
    slots, loss_0_* exactly 0 on time slots, the rows _pre wrote unchanged;
  * _reduce on what the kernels produced: by the rule against the float64 formula, and with the float32 restatement's bits
    (the header fixes the order, the kernel disables contraction); B = 130 for the third 64-thread block;
  * chunking (7 states, 1 state, an uneven split ending on a zero slot) against one chunk, bit for bit, every chunk in fresh
    sentinel buffers; capacities exact, larger, and one row short for the chunk's last state; a [12][60] size table that sizes
    in the batch exceed; a repeated call; every ligand alone (B = 1).

Inputs (tests/_score64.py): ligands [1, 7, 257, 23, 300] with pockets [300, 5, 0, 40, 257] -- dof = 0, one row more than the
256-thread stride, a second pass, an empty pocket -- five feature widths / normalisations, a shipped gamma table and the
synthetic one, n_slots 2, 4 and 17, times 1, T and interior.  Every buffer carries GUARD sentinel rows, inputs are checked
unchanged after every launch, every return code goes through _lib.check.

Tolerance: tests/_steps64.py: within -- |hip - f64| <= max(2 err_ref, 4 ulp) of the block's largest magnitude and 1e-4 at
most, err_ref = the float32 restatement against the float64 one; kl_prior, neg_log_constants and nll through
_loss64.within_at (nll: the largest addend of the combination).  No other constant.  The figures printed on the MI355X are
in profiles/score_kernels_error.md.
"""
import ctypes as C

import pytest
import torch

from tests import _loss64 as l64
from tests import _score64 as s64

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
MASK_SENTINEL = -7
GUARD = 2
F64, F32 = torch.float64, torch.float32


def dev():
    return torch.device("cuda:0")


def lib_():
    from diffsbdd_amd import _lib
    return _lib, _lib.load()


def p(t):
    return t.data_ptr()


def up(t):
    """A device copy with GUARD sentinel rows behind it."""
    pad = torch.full((GUARD,) + tuple(t.shape[1:]), SENTINEL)
    return torch.cat([t.float(), pad]).contiguous().to(dev())


def chunk_rows(t, r0, r1, cap):
    """Rows [r0, r1) of an expanded array as a chunk array of `cap` rows (+ GUARD): cut at the cap, padded with sentinels."""
    rows = t[r0:min(r1, r0 + cap)].float()
    pad = torch.full((cap - len(rows) + GUARD,) + tuple(t.shape[1:]), SENTINEL)
    return torch.cat([rows, pad]).contiguous().to(dev())


def sentinel(rows, *cols, mask=False):
    if mask:
        return torch.full((rows + GUARD,), MASK_SENTINEL, dtype=torch.int64, device=dev())
    return torch.full((rows + GUARD,) + cols, SENTINEL, device=dev())


def untouched(buf):
    return bool((buf == (MASK_SENTINEL if buf.dtype == torch.int64 else SENTINEL)).all())


def same(a, b):
    """Bit for bit; NaN where NaN (its sign and payload are no part of the contract: x - NaN differs between host and device)."""
    if a.dtype == torch.float32:
        if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
            return False
        a, b = torch.nan_to_num(a, nan=0.0, posinf=float("inf"), neginf=float("-inf")), \
            torch.nan_to_num(b, nan=0.0, posinf=float("inf"), neginf=float("-inf"))
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


class Dev:
    """One case on the device: the caller's batch with guard rows, and the launches of one model, chunk by chunk."""

    def __init__(self, case, model, logpn=None, unread=float("nan")):
        _lib, lib = lib_()
        c = self.c = case
        self.model, self.fam = model, s64.family(model)
        self.B, self.n_slots = len(c["lsz"]), c["n_slots"]
        self.S = self.B * self.n_slots
        self.a, self.r = c["a"], c["r"]
        self.lo, self.po = (l64.offsets(s64.expanded_sizes(s, self.n_slots)) for s in (c["lsz"], c["psz"]))
        self.zs = s64.zero_slots(self.B, self.n_slots)
        self.logpn = c["logpn"] if logpn is None else logpn
        # zero slots of t_int and weights: "not read"
        t_int = s64.t_int_expanded(c["times"], self.n_slots)
        w = torch.cat([c["weights"], torch.zeros(self.B, 1)], 1).reshape(-1)
        t_int[self.zs], w[self.zs] = unread, unread
        self.inp = {k: up(c[k]) for k in ("lig_x", "lig_h", "poc_x", "poc_h", "gamma")}
        self.inp.update(logpn=up(self.logpn), t_int=up(t_int), weights=up(w))
        # (guard entries behind the masks too: a node set with no rows at all still has an address)
        self.inp["ml"], self.inp["mp"] = (torch.cat([l64.mask_of(s), torch.full((GUARD,), 2 ** 40)]).to(dev())
                                          for s in (c["lsz"], c["psz"]))
        self.before = {k: v.clone() for k, v in self.inp.items()}
        rows = lib.dsbdd_score_joint_rows if self.fam == "joint" else lib.dsbdd_score_rows
        self.n_state, self.n_ligand, self.n_out = rows(0), rows(1), rows(2)
        assert (self.n_state, self.n_ligand, self.n_out) == (len(s64.STATE_ROWS[self.fam]), len(s64.LIGAND_ROWS),
                                                             len(s64.OUT_ROWS[self.fam]))
        assert rows(3) == 0

    def cfg(self):
        from diffsbdd_amd import _lib
        c = self.c
        return _lib.LossCfg(self.B, sum(c["lsz"]), sum(c["psz"]), self.a, self.r, c["T"], 0 if self.model == "simple" else 1, -1,
                            c["nv0"], c["nv1"], c["nb1"], self.logpn.shape[0], self.logpn.shape[1])

    def inputs_unchanged(self, more=()):
        for k, v in self.inp.items():
            assert same(v, self.before[k]), (k, "input modified")
        for what, v, before in more:
            assert same(v, before), (what, "input modified")

    def chunk(self, first, n, cap_l=None, cap_p=None):
        """_pre and _post of the states [first, first + n) in fresh sentinel buffers.  Asserts what no launch may do -- a
        row at or beyond the cap, a row of a state that does not fit, a per_state column outside the chunk, a per_ligand
        column whose slot 0 is not a fitting state of the chunk, a per_state row of the other kernel -- and returns the rows
        and columns the chunk owns, on the host."""
        _lib, lib = lib_()
        c, i, fam, a, r = self.c, self.inp, self.fam, self.a, self.r
        L0, L1, P0, P1 = self.lo[first], self.lo[first + n], self.po[first], self.po[first + n]
        cap_l = L1 - L0 if cap_l is None else cap_l
        cap_p = P1 - P0 if cap_p is None else cap_p
        fits = [self.lo[g + 1] - L0 <= cap_l and self.po[g + 1] - P0 <= cap_p for g in range(first, first + n)]
        nfit = sum(fits)
        assert fits == [True] * nfit + [False] * (n - nfit)
        wl, wp = self.lo[first + nfit] - L0, self.po[first + nfit] - P0          # rows that are written
        eps, noise_poc, net_lig, net_poc = (chunk_rows(c[k], r0, r1, cap) for k, r0, r1, cap in (
            ("eps", L0, L1, cap_l), ("noise_poc", P0, P1, cap_p), ("net_lig", L0, L1, cap_l), ("net_poc", P0, P1, cap_p)))
        draws = [(k, v, v.clone()) for k, v in (("eps", eps), ("noise_poc", noise_poc), ("net_lig", net_lig), ("net_poc", net_poc))]
        ps, pl = sentinel(self.n_state, self.S), sentinel(self.n_ligand, self.B)
        ml, mp, t_out = sentinel(cap_l, mask=True), sentinel(cap_p, mask=True), sentinel(n)
        cfg = self.cfg()
        head = (None, C.byref(cfg), self.n_slots, first, n, cap_l, cap_p)
        if fam == "joint":
            o = dict(eps_lig=sentinel(cap_l, 3 + a), eps_poc=sentinel(cap_p, 3 + r), z_lig=sentinel(cap_l, 3 + a),
                     z_poc=sentinel(cap_p, 3 + r))
            _lib.check(lib.dsbdd_score_joint_pre(*head, int(self.model == "joint1"), p(i["lig_x"]), p(i["lig_h"]), p(i["ml"]),
                                                 p(i["poc_x"]), p(i["poc_h"]), p(i["mp"]), p(eps), p(noise_poc), p(i["t_int"]),
                                                 p(i["gamma"]), p(i["logpn"]), p(o["eps_lig"]), p(o["eps_poc"]), p(o["z_lig"]),
                                                 p(o["z_poc"]), p(ml), p(mp), p(t_out), p(ps), p(pl)), "dsbdd_score_joint_pre")
        else:
            o = dict(z=sentinel(cap_l, 3 + a), xh_pocket=sentinel(cap_p, 3 + r))
            _lib.check(lib.dsbdd_score_cond_pre(*head, p(i["lig_x"]), p(i["lig_h"]), p(i["ml"]), p(i["poc_x"]), p(i["poc_h"]),
                                                p(i["mp"]), p(eps), p(i["t_int"]), p(i["gamma"]), p(i["logpn"]), p(o["z"]),
                                                p(o["xh_pocket"]), p(ml), p(mp), p(t_out), p(ps), p(pl)), "dsbdd_score_cond_pre")
        torch.cuda.synchronize()
        self.inputs_unchanged(draws)
        after_pre = {k: v.clone() for k, v in dict(o, ps=ps, pl=pl, ml=ml, mp=mp, t_out=t_out).items()}
        assert untouched(ps[len(s64.PRE_ROWS):]), "pre wrote a per_state row of post"
        if fam == "joint":
            _lib.check(lib.dsbdd_score_joint_post(*head, p(i["lig_h"]), p(i["ml"]), p(i["poc_h"]), p(i["mp"]), p(net_lig),
                                                  p(net_poc), p(o["eps_lig"]), p(o["eps_poc"]), p(o["z_lig"]), p(o["z_poc"]),
                                                  p(ps)), "dsbdd_score_joint_post")
        else:
            _lib.check(lib.dsbdd_score_cond_post(*head, p(i["lig_h"]), p(i["ml"]), p(i["mp"]), p(net_lig), p(eps), p(o["z"]),
                                                 p(ps)), "dsbdd_score_cond_post")
        torch.cuda.synchronize()
        self.inputs_unchanged(draws)
        n_pre = len(s64.PRE_ROWS)
        for k, v in after_pre.items():        # post writes its own per_state rows and nothing else
            now = dict(o, ps=ps, pl=pl, ml=ml, mp=mp, t_out=t_out)[k]
            assert same(now[:n_pre] if k == "ps" else now, v[:n_pre] if k == "ps" else v), (k, "modified by post")
        what = (c["name"], self.model, first, n, cap_l, cap_p)
        for k, v in o.items():
            w = wl if k in s64.LIG_TENSORS else wp
            assert untouched(v[w:]), what + (k, "a row beyond the rows of the fitting states was written")
        assert untouched(ml[wl:]) and untouched(mp[wp:]) and untouched(t_out[n:]), what + ("masks / t_out beyond their rows",)
        assert untouched(ps[:, :first]) and untouched(ps[:, first + n:]) and untouched(ps[self.n_state:]), \
            what + ("per_state outside the chunk's columns",)
        owned = [g // self.n_slots for g in range(first, first + nfit) if g % self.n_slots == 0]
        others = torch.ones(self.B, dtype=torch.bool)
        others[owned] = False
        assert untouched(pl[:, others.to(dev())]) and untouched(pl[self.n_ligand:]), what + ("per_ligand of a ligand without slot 0 here",)
        assert not (pl[:self.n_ligand, owned] == SENTINEL).any(), what + ("per_ligand of a slot 0 of the chunk not written",)
        # the masks: the chunk-local state id of every row, sorted, exactly, as int64
        sizes_l, sizes_p = ([self.lo[g + 1] - self.lo[g] for g in range(first, first + nfit)],
                            [self.po[g + 1] - self.po[g] for g in range(first, first + nfit)])
        assert ml.dtype == torch.int64 and torch.equal(ml[:wl].cpu(), l64.mask_of(sizes_l)), what + ("mask_lig_out",)
        assert torch.equal(mp[:wp].cpu(), l64.mask_of(sizes_p)), what + ("mask_pocket_out",)
        return dict(tensors={k: v[:(wl if k in s64.LIG_TENSORS else wp)].cpu() for k, v in o.items()},
                    ps=ps[:self.n_state, first:first + n].cpu(), pl=pl[:self.n_ligand].cpu(), owned=owned,
                    t_out=t_out[:n].cpu(), nfit=nfit)

    def run(self, chunks, extra=(0, 0)):
        """The whole call in the given chunks [(first, n)], assembled: dict shaped like _score64.reference's result, plus the
        raw per_state / per_ligand arrays."""
        assert [f for f, _ in chunks] == [0] + [f + n for f, n in chunks[:-1]] and sum(n for _, n in chunks) == self.S
        ps, pl = torch.full((self.n_state, self.S), SENTINEL), torch.full((self.n_ligand, self.B), SENTINEL)
        parts = []
        for first, n in chunks:
            need = self.lo[first + n] - self.lo[first], self.po[first + n] - self.po[first]
            part = self.chunk(first, n, need[0] + extra[0], need[1] + extra[1])
            assert part["nfit"] == n
            ps[:, first:first + n] = part["ps"]
            pl[:, part["owned"]] = part["pl"][:, part["owned"]]
            parts.append(part)
        assert not (pl == SENTINEL).any()
        return self.result({k: torch.cat([q["tensors"][k] for q in parts]) for k in parts[0]["tensors"]}, ps, pl,
                           torch.cat([q["t_out"] for q in parts]))

    def result(self, tensors, ps, pl, t_out):
        return dict(tensors=tensors, ps=ps, pl=pl, t_out=t_out,
                    per_state={k: ps[j] for j, k in enumerate(s64.STATE_ROWS[self.fam])},
                    per_ligand={k: pl[j] for j, k in enumerate(s64.LIGAND_ROWS)})

    def reduce(self, ps, pl):
        _lib, lib = lib_()
        ps_d, pl_d, out = up(ps), up(pl), sentinel(self.n_out, self.B)
        before = ps_d.clone(), pl_d.clone()
        fn = lib.dsbdd_score_joint_reduce if self.fam == "joint" else lib.dsbdd_score_reduce
        _lib.check(fn(None, self.B, self.n_slots, p(self.inp["weights"]), p(ps_d), p(pl_d), p(out)), "dsbdd_score_reduce")
        torch.cuda.synchronize()
        self.inputs_unchanged([("per_state", ps_d, before[0]), ("per_ligand", pl_d, before[1])])
        assert untouched(out[self.n_out:]), "reduce: guard rows written"
        out = out[:self.n_out].cpu()
        return dict({k: out[j] for j, k in enumerate(s64.OUT_ROWS[self.fam])}, raw=out)


def soft(failures, f, *a, **k):
    try:
        return f(*a, **k)
    except AssertionError as exc:
        failures.append(str(exc)[:300])


def same_result(x, y, what, skip=()):
    for k in x["tensors"]:
        assert same(x["tensors"][k], y["tensors"][k]), what + (k,)
    for k in ("ps", "pl", "t_out"):
        if k not in skip:
            assert same(x[k], y[k]), what + (k,)


def whole(D):
    return D.run([(0, D.S)])


def reduce_checks(tag, D, got, keep=None):
    """_reduce on what the kernels produced: by the rule against the float64 formula on the same terms, and the float32
    restatement's bits in every row (the copied rows included).  The terms themselves are compared block by block in
    _score64.compare; nll of the whole chain against the float64 chain is not put under the rule: the rounding of up to
    n_slots + 6 addends, each inside its own bound, adds up in the sum, which the sum's own err_ref does not bound."""
    case, model = D.c, D.model
    out = D.reduce(got["ps"], got["pl"])
    o32 = s64.reduce(model, got["per_state"], got["per_ligand"], case["weights"], F32)
    i64 = s64.reduce(model, got["per_state"], got["per_ligand"], case["weights"], F64)
    res = s64.compare_reduce(tag + "/reduce", model, out, i64, o32, keep)
    for k in s64.OUT_ROWS[D.fam]:
        assert same(out[k], o32[k]), (tag, k, "reduce: not the bits of the float32 restatement in the documented order",
                                      out[k].tolist()[:8], o32[k].tolist()[:8])
    if keep is not None:
        assert torch.equal(torch.isnan(out["nll"]), ~keep), (tag, "nll is NaN exactly beyond the size table")
    return out, res


# =========================================================================================================================
# pre, post and reduce against the restatement
# =========================================================================================================================
def check_case(case, model):
    D = Dev(case, model)
    tag = f"{case['name']}/{model}"
    got = whole(D)
    r64, r32, o64, o32 = s64.full_reference(case, model)
    s64.compare(tag, case, model, got, r64, r32)
    zs, st = D.zs, got["per_state"]
    assert (st["SNR_weight"][zs] == 0).all(), (tag, "SNR_weight of zero slots")
    for k, v in st.items():
        if k.startswith("error_t"):
            assert (v[zs] == 0).all() and (v[~zs] != 0).sum() > 0, (tag, k, "zero slots")
        if k.startswith("loss_0_"):
            assert (v[~zs] == 0).all(), (tag, k, "time slots")
    if D.fam == "joint":                # loss_t_lig differs from loss_t: the pocket's error is there
        with_pocket = torch.tensor(case["psz"]).repeat_interleave(D.n_slots) > 0
        assert (st["error_t_pocket"][~zs & with_pocket] != 0).all(), (tag, "error_t_pocket")
    if case["l0h_resolved"]:            # the categorical term is live: more than 0.1 per row on every zero slot
        rows = torch.tensor(case["lsz"]) + (torch.tensor(case["psz"]) if D.fam == "joint" else 0)
        assert float((st["loss_0_h"][zs] / rows).min()) > 0.1, (tag, "loss_0_h per row")
    reduce_checks(tag, D, got)
    # t_int and weights of zero slots are not read: a valid value in place of the NaN changes no bit
    D2 = Dev(case, model, unread=3.0)
    got2 = whole(D2)
    same_result(got, got2, (tag, "depends on t_int of a zero slot"))
    assert same(D2.reduce(got2["ps"], got2["pl"])["raw"], D.reduce(got["ps"], got["pl"])["raw"]), (tag, "weights of a zero slot")


@pytest.mark.parametrize("width", list(s64.WIDTHS))
@pytest.mark.parametrize("model", s64.MODELS)
def test_pre_post_reduce_vs_float64_restatement(model, width):
    failures = []
    for case in s64.case_grid(width):
        soft(failures, check_case, case, model)
    assert not failures, failures


@pytest.mark.parametrize("model", s64.MODELS)
def test_reduce_past_the_first_64_thread_block(model):
    """B = 130 tiny ligands, n_slots = 3: two full blocks of the reduce kernels and a third with two live threads."""
    case = s64.tiny_case()
    assert len(case["lsz"]) == 130 and case["n_slots"] == 3
    check_case(case, model)


# =========================================================================================================================
# chunks and capacities
# =========================================================================================================================
def chunkings(D):
    S, ns = D.S, D.n_slots
    by = lambda n: [(f, min(n, S - f)) for f in range(0, S, n)]
    uneven = [(0, 2 * ns), (2 * ns, 1), (2 * ns + 1, S - 2 * ns - 1)]       # the first chunk ends on ligand 1's zero slot
    return {"7 states": by(7), "1 state": by(1), "uneven": uneven}


@pytest.mark.parametrize("model", s64.MODELS)
def test_chunked_calls_have_the_bits_of_one_chunk(model):
    """The offset arithmetic P(g) against the expanded batch's own row offsets (the harness cuts the chunk arrays out of
    the expanded arrays at them), and against itself: bit for bit in every output."""
    for case in s64.chunk_cases():
        D = Dev(case, model)
        one = whole(D)
        for name, chunks in chunkings(D).items():
            if name == "7 states" and D.n_slots == 17:
                slot0 = [[g for g in range(f, f + n) if g % 17 == 0] for f, n in chunks]
                assert any(not s for s in slot0) and any(f % 17 and (f + n) % 17 for f, n in chunks)
            same_result(one, D.run(chunks), (case["name"], model, name))


def check_capacity(case, model):
    D = Dev(case, model)
    tag, S, K = f"{case['name']}/{model}", D.S, case["K"]
    one = whole(D)
    same_result(one, D.run([(0, S)], extra=(5, 3)), (tag, "larger capacities"))
    same_result(one, D.run([(0, 7), (7, S - 7)], extra=(1, 0)), (tag, "larger cap_lig, two chunks"))
    # one row short for the chunk's LAST state: (first, n, which capacity)
    for first, n, short in ((0, S - 1, "lig"), (0, S, "pocket"), (5, S - 5, "lig"), (3, S - 4, "pocket")):
        need_l, need_p = D.lo[first + n] - D.lo[first], D.po[first + n] - D.po[first]
        part = D.chunk(first, n, need_l - (short == "lig"), need_p - (short == "pocket"))
        what = (tag, first, n, "cap_" + short + " one row short")
        assert part["nfit"] == n - 1, what
        g = first + n - 1
        zero_slot = g % D.n_slots == K
        col = dict(zip(s64.STATE_ROWS[D.fam], part["ps"][:, n - 1]))
        print(f"  {what}: last state {g} ({'zero' if zero_slot else 'time'} slot) -> "
              + ", ".join(f"{k} {float(v):.4g}" for k, v in col.items()))
        assert torch.isnan(col["gamma_t"]), what + ("gamma_t",)
        assert float(col["SNR_weight"]) == 0.0 if zero_slot else torch.isnan(col["SNR_weight"]), what + ("SNR_weight",)
        for k in s64.STATE_ROWS[D.fam][len(s64.PRE_ROWS):]:
            assert torch.isnan(col[k]), what + (k, "post of a state that does not fit")
        # every state that fits: the full-capacity run, bit for bit (its rows, columns and per_ligand)
        assert same(part["ps"][:, :n - 1], one["ps"][:, first:g]), what + ("per_state of the fitting states",)
        assert same(part["t_out"][:n - 1], one["t_out"][first:g]), what + ("t_out",)
        assert same(part["pl"][:, part["owned"]], one["pl"][:, part["owned"]]), what + ("per_ligand",)
        for k, v in part["tensors"].items():
            r0 = (D.lo if k in s64.LIG_TENSORS else D.po)[first]
            assert same(v, one["tensors"][k][r0:r0 + len(v)]), what + (k,)
        # and the call's result: the bound of that ligand is NaN, every other ligand keeps its bits
        ps = one["ps"].clone()
        ps[:, first:first + n] = part["ps"]
        bad = D.reduce(ps, one["pl"])
        good = D.reduce(one["ps"], one["pl"])
        b = g // D.n_slots
        others = torch.arange(D.B) != b
        assert torch.isnan(bad["nll"][b]) and same(bad["raw"][:, others], good["raw"][:, others]), what + ("nll",)


@pytest.mark.parametrize("model", s64.MODELS)
def test_capacities_exact_larger_and_one_row_short(model):
    """cap_* exactly the chunk's rows is every other test of this file (the guard rows start right at the cap).  Here:
    larger capacities change no bit and leave the spare rows alone; a capacity one row short for the chunk's last state --
    legal arguments of the documented contract "a state that does not fit writes no row and NaN scalars".  "NaN scalars" is
    taken to mean what makes the ligand's bound NaN: gamma_t is NaN; SNR_weight is NaN on a time slot and stays the zero
    slot's exact 0 (it multiplies nothing there); _post writes NaN to all its rows of the state, so loss_t (time slot) or
    loss_0_x / loss_0_h (zero slot) and with them nll are NaN.  t, alpha_t, sigma_t and t_out of such a state are not
    asserted.  No row at or beyond the cap and no row of that state is written (Dev.chunk)."""
    failures = []
    for case in s64.chunk_cases():
        soft(failures, check_capacity, case, model)
    assert not failures, failures


# =========================================================================================================================
# the size table
# =========================================================================================================================
@pytest.mark.parametrize("model", s64.MODELS)
def test_size_beyond_the_table_is_nan_for_that_ligand_only(model):
    """Unlike the loss head there is no clamp: log_pN and nll are NaN exactly for the ligands with n_lig >= n1_tab or
    n_pocket >= n2_tab (the boundary batch has sizes n1_tab - 1, n1_tab, n2_tab - 1, n2_tab); every other output is bitwise
    that of the [301][301] table's run, log_pN and nll of the other ligands read another value and go by the rule."""
    for case in s64.table_cases():
        tag = f"{case['name']}/{model}/small-table"
        small = case["logpn_small"]
        keep = torch.tensor([n < small.shape[0] and q < small.shape[1] for n, q in zip(case["lsz"], case["psz"])])
        assert (~keep).sum() >= 2 and keep.any()
        big_run = whole(Dev(case, model))
        D = Dev(case, model, logpn=small)
        got = whole(D)
        same_result(big_run, got, (tag, "depends on the size table"), skip=("pl",))
        j = s64.LIGAND_ROWS.index("log_pN")
        rest = [q for q in range(len(s64.LIGAND_ROWS)) if q != j]
        assert same(big_run["pl"][rest], got["pl"][rest]) and torch.isfinite(big_run["pl"]).all(), tag
        r64, r32, o64, o32 = s64.full_reference(case, model, small)
        s64.compare(tag, case, model, got, r64, r32, keep)
        out, _ = reduce_checks(tag, D, got, keep)
        big_out = Dev(case, model).reduce(big_run["ps"], big_run["pl"])
        for k in s64.OUT_ROWS[D.fam]:
            if k not in ("nll", "log_pN"):
                assert same(out[k], big_out[k]), (tag, k)


# =========================================================================================================================
# bitwise properties
# =========================================================================================================================
@pytest.mark.parametrize("model", s64.MODELS)
def test_repeated_call_and_every_ligand_alone_have_the_same_bits(model):
    """One workgroup per state with fixed-order sums: a repeated call gives the same bits, and every ligand evaluated alone
    (B = 1, its own rows, the same times and draws) has the rows and columns it has inside the batch."""
    for case in s64.chunk_cases():
        D = Dev(case, model)
        one = whole(D)
        same_result(one, whole(D), (case["name"], model, "repeated"))
        out = D.reduce(one["ps"], one["pl"])
        assert same(out["raw"], D.reduce(one["ps"], one["pl"])["raw"]), (case["name"], model, "reduce repeated")
        ns = D.n_slots
        for b in range(D.B):
            sub, el, ep = s64.sub_case(case, b)
            what = (case["name"], model, b, "depends on the batch")
            A = Dev(sub, model)
            alone = whole(A)
            for k, v in alone["tensors"].items():
                assert same(v, one["tensors"][k][el if k in s64.LIG_TENSORS else ep]), what + (k,)
            assert same(alone["ps"], one["ps"][:, b * ns:(b + 1) * ns]), what + ("per_state",)
            assert same(alone["pl"][:, 0], one["pl"][:, b]), what + ("per_ligand",)
            assert same(alone["t_out"], one["t_out"][b * ns:(b + 1) * ns]), what + ("t_out",)
            assert same(A.reduce(alone["ps"], alone["pl"])["raw"][:, 0], out["raw"][:, b]), what + ("out",)
