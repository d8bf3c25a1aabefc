"""Pins tests/_score64.py -- the float64 reference of tests/test_gpu_score_kernels.py -- on the CPU.

  * against oracle/ddpm_oracle.py: loss_terms(..., training=False) slot by slot (composed as oracle_slots of
    tests/test_gpu_score.py does), the network replaced by a function that returns the case's `net` rows of the state (one
    return for the time pass, one for the t = 0 pass), the draws fed through NoiseReplay, everything in float64;
    ConditionalDDPM, SimpleConditionalDDPM and the joint model (center = 1: the oracle gets the complex centred beforehand);
    every term and nll to 1e-12 of the term's largest magnitude (kl_prior: of its largest addend, nll: of the largest
    addend of the combination); a size table that holds every size, since the oracle has no clamp;
  * the self-check: on every case of the GPU file the float32 restatement passes the GPU file's own comparison functions,
    i.e. the inputs do not make the tolerance rule unsatisfiable for the reference alone;
  * the float64 `reduce` against diffsbdd_amd.score.combine_terms / combine_terms_joint.  Those evaluate in float32 by
    construction (the device's order), so: the float32 `reduce` has their bits, and the float64 one agrees by the rule.
"""
import pytest
import torch

from oracle import ddpm_oracle as do
from tests import _loss64 as l64
from tests import _score64 as s64

F64, F32 = torch.float64, torch.float32


def rel(a, b, mag=None):
    a, b = torch.as_tensor(a, dtype=F64).reshape(-1), torch.as_tensor(b, dtype=F64).reshape(-1)
    assert a.shape == b.shape
    mag = float(b.abs().max()) if mag is None else mag
    return float((a - b).abs().max()) / max(mag, 1e-300)


# ---- against the oracle -----------------------------------------------------------------------------------------------------
def oracle_case(width, table, K):
    """The main batch with two rows in place of its empty pocket (the oracle's behaviour on one is not pinned)."""
    case = s64.make_case("main", width, table, K)
    lsz, psz = case["lsz"], [p or 2 for p in case["psz"]]
    g = torch.Generator().manual_seed(11)
    npk, r = sum(psz), case["r"]
    case.update(psz=psz, poc_x=torch.randn(npk, 3, generator=g) * 7.0 + 2.0,
                poc_h=torch.nn.functional.one_hot(torch.randint(0, r, (npk,), generator=g), r).float(),
                noise_poc=torch.randn(npk * case["n_slots"], 3 + r, generator=g),
                net_poc=torch.randn(npk * case["n_slots"], 3 + r, generator=g))
    case["logpn"] = case["logpn"].double()
    return case


def slot_rows(sizes, n_slots, k):
    """Rows of the expanded batch that the states (b, k), b = 0 .. B - 1, own: the caller's batch as slot k sees it."""
    o = s64.offsets(s64.expanded_sizes(sizes, n_slots))
    return torch.cat([torch.arange(o[b * n_slots + k], o[b * n_slots + k + 1]) for b in range(len(sizes))])


def oracle_slots(case, model):
    """-> list over k of the oracle's 12-tuple for time slot k (its L0 terms: the zero slot)."""
    fam, c = s64.family(model), case
    m = do.OracleModel(None, None, c["a"], c["r"], c["T"], "polynomial_2", 1e-4, norm_values=(c["nv0"], c["nv1"]),
                       norm_biases=(None, c["nb1"]), conditional=fam != "joint", simple=model == "simple")
    m.gamma = c["gamma"].double()
    lm, pm = l64.mask_of(c["lsz"]), l64.mask_of(c["psz"])
    lig_x, poc_x = c["lig_x"].double(), c["poc_x"].double()
    if model == "joint1":
        B = len(c["lsz"])
        mean = l64.seg_mean3(torch.cat([lig_x, poc_x]), torch.cat([lm, pm]), B, torch.tensor(c["lsz"]) + torch.tensor(c["psz"]))
        lig_x, poc_x = lig_x - mean[lm], poc_x - mean[pm]
    lig = dict(x=lig_x, one_hot=c["lig_h"].double(), mask=lm, size=torch.tensor(c["lsz"]))
    poc = dict(x=poc_x, one_hot=c["poc_h"].double(), mask=pm, size=torch.tensor(c["psz"]))
    K, n_slots = c["K"], c["n_slots"]
    cols = []
    default = torch.get_default_dtype()
    torch.set_default_dtype(F64)         # an integer size tensor times a python float (delta_log_px) takes the default dtype
    try:
        for k in range(K):
            draws, nets = [], []
            for slot in (k, K):
                rl, rp = slot_rows(c["lsz"], n_slots, slot), slot_rows(c["psz"], n_slots, slot)
                e, npo = c["eps"].double()[rl], c["noise_poc"].double()[rp]
                draws += [e] if fam != "joint" else [torch.cat([e[:, :3], npo[:, :3]]), e[:, 3:], npo[:, 3:]]
                nets.append((c["net_lig"].double()[rl], c["net_poc"].double()[rp]))
            replay, it = do.NoiseReplay(draws), iter(nets)
            m.dynamics = lambda *args: next(it)
            cols.append(do.loss_terms(m, lig, poc, c["times"][:, k:k + 1].double(), replay, False,
                                      size_log_prob=lambda n1, n2: c["logpn"][n1, n2]))
            assert replay.i == len(draws) and next(it, None) is None
    finally:
        torch.set_default_dtype(default)
    return cols


@pytest.mark.parametrize("table,K", [("polynomial_2/500/5e-4", 3), ("synthetic", 1), ("synthetic", 3)])
@pytest.mark.parametrize("width", ["crossdock_fullatom_cond", "moad_fullatom_joint", "odd", "odd_biased"])
@pytest.mark.parametrize("model", s64.MODELS)
def test_restatement_agrees_with_the_oracle_in_float64(model, width, table, K):
    case = oracle_case(width, table, K)
    fam, B, n_slots = s64.family(model), len(case["lsz"]), K + 1
    cols = oracle_slots(case, model)
    ref = s64.reference(case, model, F64)
    st = {k: v.reshape(B, n_slots) for k, v in ref["per_state"].items()}
    pl = ref["per_ligand"]

    def check(name, mine, theirs, mag=None):
        e = rel(mine, theirs, mag)
        print(f"  {name}: {e:.3e}")
        assert e <= 1e-12, (name, e)

    names = ("delta_log_px", "error_t_lig", "error_t_pocket", "SNR_weight", "loss_0_x_ligand", "loss_0_x_pocket", "loss_0_h",
             "neg_log_constants", "kl_prior", "log_pN", "t_int", "xh_lig_hat")
    slot = lambda name: torch.stack([torch.as_tensor(dict(zip(names, col))[name]).double() for col in cols], 1)
    check("t", st["t"][:, :K] * case["T"], slot("t_int"))
    check("SNR_weight", st["SNR_weight"][:, :K], slot("SNR_weight"))
    check("error_t_lig", st["error_t_lig" if fam == "joint" else "error_t"][:, :K], slot("error_t_lig"))
    check("loss_0_x_ligand", st["loss_0_x_ligand" if fam == "joint" else "loss_0_x"][:, K:].expand(B, K), slot("loss_0_x_ligand"))
    check("loss_0_h", st["loss_0_h"][:, K:].expand(B, K), slot("loss_0_h"))
    if fam == "joint":
        check("error_t_pocket", st["error_t_pocket"][:, :K], slot("error_t_pocket"))
        check("loss_0_x_pocket", st["loss_0_x_pocket"][:, K:].expand(B, K), slot("loss_0_x_pocket"))
    for k in ("neg_log_constants", "delta_log_px", "log_pN"):
        check(k, pl[k][:, None].expand(B, K), slot(k))
    check("kl_prior", pl["kl_prior"][:, None].expand(B, K), slot("kl_prior"), ref["kl_addend"])
    # the selection by slot kind is exact
    zs = s64.zero_slots(B, n_slots)
    for k, v in ref["per_state"].items():
        if k.startswith("error_t"):
            assert (v[zs] == 0).all() and (v[~zs] > 0).all(), k
        if k.startswith("loss_0_x"):
            assert (v[~zs] == 0).all() and (v[zs] > 0).all(), k
    assert (ref["per_state"]["SNR_weight"][zs] == 0).all() and (ref["per_state"]["loss_0_h"][~zs] == 0).all()
    # nll: the header's formula on the ORACLE's terms, written out here
    w = case["weights"].double()
    err = slot("error_t_lig") + (slot("error_t_pocket") if fam == "joint" else 0)
    loss_t = (-0.5 * w * slot("SNR_weight") * err).sum(1)
    o = {n: slot(n)[:, 0] for n in names[:10] if fam == "joint" or not n.endswith("_pocket")}
    l0x = o["loss_0_x_ligand"] + (o["loss_0_x_pocket"] if fam == "joint" else 0)
    nll = loss_t + l0x + o["loss_0_h"] + o["neg_log_constants"] + o["kl_prior"] - o["delta_log_px"] - o["log_pN"]
    out = s64.reduce(model, ref["per_state"], ref["per_ligand"], case["weights"], F64)
    check("loss_t", out["loss_t"], loss_t)
    check("nll", out["nll"], nll, out["addend"])
    if fam == "joint":
        check("loss_t_lig", out["loss_t_lig"], (-0.5 * w * slot("SNR_weight") * slot("error_t_lig")).sum(1))


def test_size_lookup_has_no_clamp():
    tab = torch.arange(12 * 60, dtype=F64).reshape(12, 60)
    n1, n2 = torch.tensor([0, 11, 12, 11, 300, 5]), torch.tensor([0, 59, 7, 60, 1000, 59])
    got = s64.size_lookup(tab, n1, n2, F64)
    assert got[[0, 1, 5]].tolist() == [0.0, float(tab[11, 59]), float(tab[5, 59])] and torch.isnan(got[[2, 3, 4]]).all()
    case = s64.table_cases()[1]
    ref = s64.reference(case, "joint0", F64, case["logpn_small"])
    want = [n >= 12 or p >= 60 for n, p in zip(case["lsz"], case["psz"])]
    assert torch.isnan(ref["per_ligand"]["log_pN"]).tolist() == want == [False, True, True, False, True, True]
    out = s64.reduce("joint0", ref["per_state"], ref["per_ligand"], case["weights"], F64)
    assert torch.isnan(out["nll"]).tolist() == want and out["addend"] > 0


# ---- the self-check -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", s64.MODELS)
def test_float32_restatement_passes_the_gpu_comparison_on_every_gpu_case(model):
    cases = s64.gpu_cases()
    for name, case in cases.items():
        print(name)
        tables = [None] + ([case["logpn_small"]] if name in {c["name"] for c in s64.table_cases()} else [])
        for tab in tables:
            r64, r32, o64, o32 = s64.full_reference(case, model, tab)
            tag = f"{name}/{model}" + ("/small-table" if tab is not None else "")
            if tab is not None:        # log_pN and nll are NaN exactly beyond the table: compared on the others
                keep = torch.isfinite(r64["per_ligand"]["log_pN"])
                assert torch.equal(torch.isnan(o32["nll"]), ~keep) and torch.equal(torch.isnan(o64["nll"]), ~keep)
            else:
                keep = None
            s64.compare(tag, case, model, r32, r64, r32, keep)
            s64.compare_reduce(tag, model, o32, o64, o32, keep)
            # the reduce alone, on float32 terms (what the GPU file feeds it): float32 order against float64 arithmetic
            i64 = s64.reduce(model, r32["per_state"], r32["per_ligand"], case["weights"], F64)
            s64.compare_reduce(tag + "/reduce-alone", model, o32, i64, o32, keep)
        if case["l0h_resolved"]:        # otherwise the case proves nothing about the categorical term
            n_slots = case["n_slots"]
            rows = torch.tensor(case["lsz"]) + (torch.tensor(case["psz"]) if s64.family(model) == "joint" else 0)
            per_row = r64["per_state"]["loss_0_h"][n_slots - 1::n_slots] / rows
            assert float(per_row.min()) > 0.1, (name, per_row)
    # the grid (the chunk and table cases on the main batch are members of it), the boundary batch and the tiny one
    assert len(cases) == len(s64.WIDTHS) * 5 + 2


def test_gpu_case_list_has_the_shapes_the_kernels_can_go_wrong_at():
    lsz, psz = s64.MAIN
    assert 1 in lsz and 257 in lsz and 300 in lsz and 0 in psz and 257 in psz and 0 not in lsz
    assert {c["n_slots"] for c in s64.case_grid("odd")} == {2, 4, 17}
    for c in s64.gpu_cases().values():
        t = c["times"]
        assert t.min() >= 1 and t.max() <= c["T"] and (t == t.round()).all()
        assert (t == 1).any() and (t == c["T"]).any() and ((t > 1) & (t < c["T"])).any(), c["name"]
    assert len(s64.TINY[0]) == 130 and min(s64.TINY[0]) >= 1


# ---- reduce against the package's torch combination ---------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["cond", "joint0"])
def test_reduce_against_combine_terms(model):
    from diffsbdd_amd import score
    for case in s64.chunk_cases() + [s64.tiny_case()]:
        B, K = case["weights"].shape
        r64, r32, o64, o32 = s64.full_reference(case, model)
        st = {k: v.reshape(B, K + 1) for k, v in r32["per_state"].items()}
        pl = r32["per_ligand"]
        tail = [pl[k] for k in ("neg_log_constants", "kl_prior", "delta_log_px", "log_pN")]
        if model == "cond":
            nll, loss_t = score.combine_terms(case["weights"], st["SNR_weight"][:, :K], st["error_t"][:, :K], st["loss_0_x"][:, K],
                                              st["loss_0_h"][:, K], *tail)
        else:
            nll, loss_t, loss_t_lig = score.combine_terms_joint(
                case["weights"], st["SNR_weight"][:, :K], st["error_t_lig"][:, :K], st["error_t_pocket"][:, :K],
                st["loss_0_x_ligand"][:, K], st["loss_0_x_pocket"][:, K], st["loss_0_h"][:, K], *tail)
            assert torch.equal(loss_t_lig, o32["loss_t_lig"]), case["name"]
        assert nll.dtype == F32 and torch.equal(nll, o32["nll"]) and torch.equal(loss_t, o32["loss_t"]), case["name"]
        # and the float64 formula on the same float32 terms, by the rule
        i64 = s64.reduce(model, r32["per_state"], r32["per_ligand"], case["weights"], F64)
        s64.compare_reduce(f"{case['name']}/{model}/combine_terms", model, dict(o32, nll=nll, loss_t=loss_t), i64, o32)
