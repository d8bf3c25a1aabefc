"""CPU: the conditions tests/test_gpu_train_degenerate.py relies on, with no code under test involved -- the float64
reference of every (case, architecture) of tests/_train64.py is finite, the float32 oracle stays within 5e-5 of it for
every quantity (so `2 err_ref` is never cut by the 1e-4 cap of `within_case` and the cap never decides an outcome), the
cases have the structure they claim, the exact edge list is unambiguous at 1e-4 (the device list must equal it element for
element), and the structural zeros are exactly 0 in float64.

Worst err_ref per case measured here: ragged 4.5e-6 (small_cond), 1.9e-6 (small_joint), 2.1e-5 (small_variant, seed 26:
d_xh_atoms at norm_constant 0; 8.5e-5 at seed 21, 5.1e-5 at 25), 1.1e-5 (crossdock_ca_cond), 9.1e-6
(crossdock_fullatom_cond), 5.5e-6 (moad_fullatom_joint); hole 6.0e-6; no_ligand 1.6e-5; no_pocket 5.4e-6; far 7.4e-6 /
1.9e-5; single 6.4e-7; shared_t 5.0e-6.
"""
import pytest
import torch

from tests import _train64 as T

ERR_REF_MAX = 5e-5


@pytest.mark.parametrize("case,arch", T.PAIRS)
def test_reference_is_finite_and_the_float32_oracle_is_close(case, arch):
    r64 = T.reference(case, arch, torch.float64)
    names = T.param_names(T.inputs(case, arch)["cfg"])
    assert set(r64) == {"eps_l", "eps_p", "d_xh_atoms", "d_xh_residues", *names}
    for k, v in r64.items():
        assert v.dtype == torch.float64 and torch.isfinite(v).all(), k
    errs, med = T.err_refs(case, arch)
    worst = max(errs, key=errs.get)
    print(f"  {case} {arch}: worst err_ref {errs[worst]:.3e} ({worst}), median {med:.3e}, {len(errs)} quantities")
    assert errs[worst] <= ERR_REF_MAX, (worst, errs[worst])
    assert 0 < med <= ERR_REF_MAX


@pytest.mark.parametrize("case,arch", T.PAIRS)
def test_case_has_the_structure_it_claims(case, arch):
    spec, p = T.CASES[case], T.inputs(case, arch)
    cfg, ml, mp = p["cfg"], p["ml"], p["mp"]
    n_l, n_p = len(ml), len(mp)
    B = len(spec["n_lig"])
    assert torch.bincount(ml, minlength=B).tolist() == spec["n_lig"] and torch.bincount(mp, minlength=B).tolist() == spec["n_poc"]
    assert p["xl"].shape == (n_l, 3 + cfg["atom_nf"]) and p["xp"].shape == (n_p, 3 + cfg["residue_nf"])
    assert p["t"].shape == ((1, 1) if spec["shared_t"] else (B, 1))
    if case in ("ragged", "shared_t"):
        assert spec["n_lig"][1] == 0 and spec["n_lig"][2] == 1 and spec["n_poc"][3] == 0
    if case == "hole":
        assert spec["n_lig"][1] == 0 and spec["n_poc"][1] == 0
    if case == "no_ligand":
        assert n_l == 0 and n_p > 0
    if case == "no_pocket":
        assert n_p == 0 and n_l > 0
    # the edge list: counts of get_edges, the ligand-row prefix, symmetric, self loops, nothing near a cutoff
    edges = T.exact_edges(case, arch)
    row, col = edges
    E = edges.shape[1]
    direct = T.eo.get_edges(ml, mp, p["xl"][:, :3].double(), p["xp"][:, :3].double(), *T.cutoffs(cfg), exact=True)
    assert torch.equal(edges, direct) and E == direct.shape[1]
    assert torch.equal(row, row.sort().values)                               # sorted by row: the ligand rows are a prefix
    e_lig = int((row < n_l).sum())
    assert e_lig == int(torch.searchsorted(row, torch.tensor(n_l)))
    assert e_lig >= n_l and E >= n_l + n_p                                     # self loops
    key = row * (n_l + n_p) + col
    assert torch.equal((col * (n_l + n_p) + row).sort().values, key)         # every edge has its reverse
    assert T.ambiguous_pairs(case, arch, 1e-4) == 0
    if case == "no_ligand":
        assert e_lig == 0
    if case == "no_pocket":
        assert e_lig == E
    if case == "single":
        assert E == 2 and torch.equal(row, col)
    if spec["moved"] is not None:
        b = spec["moved"][0]
        mine = (row < n_l) & (ml[row.clamp(max=max(n_l - 1, 0))] == b)
        assert int(mine.sum()) > 0 and bool((col[mine] < n_l).all())        # no ligand-pocket edge for the moved ligand
        others = (row < n_l) & ~mine
        assert bool((col[others] >= n_l).any())                              # ... while the other ligands keep theirs


@pytest.mark.parametrize("case,arch", T.PAIRS)
def test_structural_zeros_are_exact_in_float64(case, arch):
    r64, r32 = T.reference(case, arch, torch.float64), T.reference(case, arch, torch.float32)
    zeros = T.structural_zeros(case, arch)
    if case in ("no_ligand", "no_pocket", "single"):
        assert zeros
    for k in zeros:
        assert r64[k].numel() and T.magnitude(r64[k]) == 0.0 and T.magnitude(r32[k]) == 0.0, k
    # nothing else vanishes: every other quantity is a live comparison
    for k, v in r64.items():
        if k not in zeros and v.numel():
            assert T.magnitude(v) > 0.0, k
