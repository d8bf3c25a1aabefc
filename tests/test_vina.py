"""Host logic of diffsbdd_amd/vina.py: the numpy restatements of vina_type_kernel and vina_score_kernel (the specification
the GPU tests compare the kernels with) at hand-checkable values, the residue table, the crystal fixture against its
independent float64 statement, the error bound, and the front ends' argument handling.  No GPU."""
import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib, metrics, pose, vina as V
from tests import _vina_cases as C


def _pair(d, code_i=V.C_C | V.HYDROPHOBIC, code_j=V.C_C | V.HYDROPHOBIC, r=None):
    """The restatement on one ligand atom at the origin and one pocket atom at distance r on the x axis (r from d)."""
    r = d + V.XS_RADII[V.CLASSES[code_i & 15]] + V.XS_RADII[V.CLASSES[code_j & 15]] if r is None else r
    st, margin = V._vina_score_host(np.zeros((1, 3), np.float32), [code_i], [0, 1], [0], [[1, 0, 0, 0]],
                                    np.asarray([[r, 0, 0]], np.float32), [code_j], [0, 1])
    return st.atom[0], st.mol[0], margin


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_pair_terms_at_hand_values():
    t = V.pair_terms(np.asarray([0.0, -0.7, -0.35, 1.0, -1.0]))
    assert t[0].tolist() == [1.0, np.exp(-2.25), 0.0, 1.0, 0.0]
    assert t[1, 4] == 1.0 and t[2, 4] == pytest.approx(0.5, abs=1e-15) and t[3, 3] == 0.5 and t[4, 2] == 1.0
    # continuity at every kink: hydrophobic at 0.5 and 1.5, hbond at -0.7 and 0, repulsion at 0
    for k, kink in ((3, 0.5), (3, 1.5), (4, -0.7), (4, 0.0), (2, 0.0)):
        lo, hi = V.pair_terms(np.asarray([kink - 1e-9, kink + 1e-9]))[:, k]
        assert abs(lo - hi) < 1e-8, (k, kink)
    # flags switch the two conditional terms off
    assert V.pair_terms(np.asarray([0.0]), hydrophobic=False, hbond=False)[0].tolist() == [1.0, np.exp(-2.25), 0.0, 0.0, 0.0]
    # through the restatement: two hydrophobic carbons 3.8 A apart sit at d = 0 (3.8f - 1.9 - 1.9 is 0 to 1e-7)
    atom, mol, _ = _pair(0.0)
    assert atom == pytest.approx([1.0, np.exp(-2.25), 0.0, 1.0, 0.0], abs=1e-6)
    assert mol[V.M_INTER] == pytest.approx(np.dot(V.WEIGHTS, atom), rel=1e-15) and mol[V.M_SCORE] == mol[V.M_INTER]
    # r = 8 exactly is not counted, the float32 below it is
    far = V.C_I | V.HYDROPHOBIC
    atom, _, margin = _pair(None, far, far, r=8.0)
    assert not atom.any() and margin == 0.0
    atom, _, _ = _pair(None, far, far, r=float(np.nextafter(np.float32(8.0), np.float32(0.0))))
    assert atom[1] > 0 and atom[0] > 0
    # a pair where both directions of hbond hold is counted once
    both = V.C_O | V.DONOR | V.ACCEPTOR
    atom, _, _ = _pair(-0.7 - 1e-3, both, both)
    assert atom[4] == 1.0
    atom, _, _ = _pair(-0.35, V.C_N | V.DONOR, V.C_O | V.ACCEPTOR)
    assert atom[4] == pytest.approx(0.5, abs=1e-6) and atom[3] == 0.0
    assert _pair(-0.35, V.C_N | V.DONOR, V.C_N | V.DONOR)[0][4] == 0.0          # two donors: none
    # untyped atoms take no part; N_rot divides
    assert not _pair(None, 0, V.C_C, r=3.8)[0].any() and not _pair(None, V.C_C, 13, r=3.8)[0].any()
    st, _ = V._vina_score_host(np.zeros((1, 3), np.float32), [17], [0, 1], [0], [[1, 0, 4, 0]],
                               np.asarray([[3.8, 0, 0]], np.float32), [17], [0, 1])
    assert st.mol[0, V.M_SCORE] == pytest.approx(st.mol[0, V.M_INTER] / (1 + 4 * V.ROT_WEIGHT), rel=1e-15)


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_typing_of_hand_built_graphs():
    G = C.GRAPHS
    code, rot = C.type_host(*G["ethanol"])
    assert [C.flags(c) for c in code] == ["H", "", "DA"] and rot == 0
    assert C.type_host(*G["butane"])[1] == 1
    code, rot = C.type_host(*G["cyclohexane"])
    assert rot == 0 and all(C.flags(c) == "H" for c in code)
    assert C.type_host(*G["biphenyl"])[1] == 1
    assert C.flags(C.type_host(*G["pyridine"])[0][0]) == "A"
    assert C.flags(C.type_host(*G["piperidine"])[0][0]) == "D"
    assert C.flags(C.type_host(*G["trimethylamine"])[0][0]) == ""
    assert C.flags(C.type_host(*G["acetonitrile"])[0][2]) == "A"
    code, _ = C.type_host(*G["acetamide"])
    assert [C.flags(c) for c in code] == ["H", "", "A", "D"]
    assert C.flags(C.type_host(*G["nitromethane"])[0][1]) == ""
    code, _ = C.type_host(*G["chlorobenzene"])
    assert C.flags(code[6]) == "H" and C.flags(code[0]) == "" and all(C.flags(c) == "H" for c in code[1:6])
    code, _ = C.type_host(*G["methylborane"])
    assert code.tolist() == [V.C_C | V.HYDROPHOBIC, V.C_C, 0]               # boron untyped, its carbon not hydrophobic
    assert C.type_host(*C.join(G["naphthalene"], C.chain(4), links=[(10, 2, 1)]))[1] == 3
    assert C.type_host(*C.ring(20))[1] == 0 and C.type_host(*C.chain(128))[1] == 125
    # caffeine from the fixture's bond list
    z = C.fixture()
    el, bonds = C.fixture_ligand(z, "3rfm")
    code, rot = C.type_host(el, bonds)
    assert rot == 0 and not (code & V.DONOR).any() and not (code & V.HYDROPHOBIC).any()
    acceptors = [a for a in range(len(el)) if code[a] & V.ACCEPTOR]
    degree = np.bincount(np.asarray(bonds)[:, :2].reshape(-1), minlength=len(el))
    assert sorted(acceptors) == sorted([a for a, e in enumerate(el) if e == "O"] +
                                       [a for a, e in enumerate(el) if e == "N" and degree[a] == 2])
    assert sum(el[a] == "O" for a in acceptors) == 2 and sum(el[a] == "N" for a in acceptors) == 1
    # renumbering the atoms permutes the codes and keeps N_rot
    el5, bonds5 = C.fixture_ligand(z, "5ndu")
    code5, rot5 = C.type_host(el5, bonds5, sorted(set(el5)))
    perm = np.random.RandomState(1).permutation(len(el5))                  # new index of old atom a: perm[a]
    el_p = [None] * len(el5)
    for a, p in enumerate(perm):
        el_p[p] = el5[a]
    code_p, rot_p = C.type_host(el_p, [(perm[i], perm[j], o) for i, j, o in bonds5], sorted(set(el5)))
    assert rot_p == rot5 == 10 and np.array_equal(code_p[perm], code5)


def test_typing_of_the_ragged_batch_on_the_host():
    b = C.type_batch()
    code, mol = V._vina_type_host(*(b[k] for k in C.TYPE_KEYS), fill=-7)
    assert mol[:, 2].tolist() == [0, 0, 0, 0, 3, 0, 125, 125, 1, 0, 1, 0, 0, 8, 1, 0]
    assert mol[7].tolist() == [128, 0, 125, 0] and mol[9].tolist() == [2, 1, 0, 0] and mol[10].tolist() == [2, 2, 1, 0]
    off = b["true_off"]
    assert (code[off[11]:off[13]] == -7).all() and (code[off[7] + 128:off[8]] == 0).all() and (code[:off[11]] != -7).all()


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_residue_table():
    T = V.RESIDUE_TABLE
    sizes = {"GLY": 4, "ALA": 5, "SER": 6, "CYS": 6, "VAL": 7, "THR": 7, "PRO": 7, "ILE": 8, "LEU": 8, "ASP": 8, "ASN": 8,
             "MET": 8, "GLU": 9, "GLN": 9, "LYS": 9, "HIS": 10, "PHE": 11, "ARG": 11, "TYR": 12, "TRP": 14}
    assert {r: len(t) for r, t in T.items()} == sizes and sum(sizes.values()) == 167
    assert all("OXT" not in t and {"N", "CA", "C", "O"} <= set(t) for t in T.values())
    assert set(T["TRP"]) == {"N", "CA", "C", "O", "CB", "CG", "CD1", "CD2", "NE1", "CE2", "CE3", "CZ2", "CZ3", "CH2"}
    f = lambda res, atom: C.flags(T[res][atom])
    for res in T:
        assert f(res, "N") == ("" if res == "PRO" else "D") and f(res, "O") == "A" and f(res, "CA") == "" and f(res, "C") == ""
    assert C.flags(V.OXT_CODE) == "A"
    assert f("SER", "OG") == "DA" and f("SER", "CB") == "" and f("LEU", "CD1") == "H" and f("LYS", "NZ") == "D"
    assert f("ASP", "OD1") == "A" and f("ASP", "OD2") == "A" and f("HIS", "ND1") == "DA" and f("HIS", "NE2") == "DA"
    assert f("MET", "SD") == "" and f("MET", "CG") == "" and f("MET", "CE") == "" and f("MET", "CB") == "H"
    assert T["MET"]["SD"] & 15 == V.C_S and f("TYR", "OH") == "DA" and f("TRP", "NE1") == "D" and f("ARG", "NH1") == "D"
    # a residue list: template, OXT, fallback by element, water and hydrogens dropped, a metal
    atom = lambda name, el, x: (name, el, (float(x), 0.0, 0.0))
    residues = [
        dict(resname="SER", atoms=[atom("N", "N", 0), atom("OG", "O", 1), atom("HG", "H", 2), atom("OXT", "O", 3), atom("XX", "C", 4)]),
        dict(resname="HOH", atoms=[atom("O", "O", 5)]), dict(resname="WAT", atoms=[atom("O", "O", 6)]),
        dict(resname="LIG", atoms=[atom("C1", "C", 7), atom("N1", "N", 8), atom("O1", "O", 9), atom("CL", "CL", 10), atom("SE", "Se", 11)]),
        dict(resname="ZN", atoms=[atom("ZN", "ZN", 12)]),
    ]
    tp = V.type_pocket(residues)
    assert tp.x[:, 0].tolist() == [0, 1, 3, 4, 7, 8, 9, 10, 11, 12]
    assert tp.code.tolist() == [V.C_N | V.DONOR, V.C_O | V.DONOR | V.ACCEPTOR, V.C_O | V.ACCEPTOR, V.C_C, V.C_C, V.C_N,
                                V.C_O | V.ACCEPTOR, V.C_CL | V.HYDROPHOBIC, 0, V.C_METAL | V.DONOR]
    assert tp.untemplated == 7
    assert [V.class_of(m) for m in V.METALS] == [V.C_METAL] * 8 and V.class_of("B") == 0 and V.class_of("cl") == V.C_CL


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_fixture_against_its_independent_float64_statement():
    z = C.fixture()
    assert z["names"].tolist() == ["3rfm", "5ndu"]
    for name in z["names"]:
        el, bonds = C.fixture_ligand(z, name)
        code, rot = C.type_host(el, bonds)
        assert np.array_equal(code, z[f"{name}_lig_code"]) and rot == int(z[f"{name}_n_rot"])
        tp = V.type_pocket(C.fixture_residues(z, name))
        assert np.array_equal(tp.code, z[f"{name}_poc_code"]) and tp.untemplated == 0 and np.array_equal(tp.x, z[f"{name}_poc_x"])
        n, scores = len(el), {}
        for variant in ("crystal", "shifted"):
            st, margin = V._vina_score_host(z[f"{name}_{variant}_x"], code, [0, n], [0], [[n, 0, rot, 0]], tp.x, tp.code,
                                            [0, len(tp.code)])
            assert margin > float(z["margin"])
            want = z[f"{name}_{variant}_terms"]
            assert np.all(np.abs(st.mol[0, :5] - want) <= 1e-12 * np.abs(want))
            assert np.all(np.abs(st.atom - z[f"{name}_{variant}_atom"]) <= 1e-12 * np.abs(z[f"{name}_{variant}_atom"]) + 1e-300)
            assert st.mol[0, V.M_INTER] == pytest.approx(float(z[f"{name}_{variant}_inter"]), rel=1e-12)
            assert st.mol[0, V.M_SCORE] == pytest.approx(float(z[f"{name}_{variant}_score"]), rel=1e-12)
            scores[variant] = st.mol[0]
        assert scores["crystal"][V.M_SCORE] < 0                                  # the crystal pose scores negative
        assert scores["shifted"][2] > scores["crystal"][2]                       # pushed into the protein: more repulsion


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_error_bound_holds_plain_float32_and_scales_with_eps():
    """Recorded: the restatement evaluated in float32 (numpy) uses at most 0.060 / 0.068 / 0.107 / 0.037 / 0.020 of the bound
    per atom (gauss1, gauss2, repulsion, hydrophobic, hbond) and 0.019 per molecule on this batch; the kernel's own fractions
    are in profiles/vina_score_error.md."""
    b = C.score_batch()
    st, margin, atom_bound, mol_bound = C.score_reference()
    assert margin > C.MARGIN                                                     # the condition on the inputs
    live = st.flag == 0
    assert live.sum() == 15 and np.isnan(mol_bound[b["nan_mol"]]).all() and np.isnan(st.mol[b["nan_mol"], :7]).all()
    assert (mol_bound[live] >= 0).all() and (mol_bound[live][:, :5].max(0) > 0).all() and (mol_bound[b["empty_mol"]] == 0).all()
    ab2, mb2 = V.error_bound(*(b[k] for k in C.SCORE_KEYS), eps=2 * V.EPS32)
    assert np.allclose(mb2[live], 2 * mol_bound[live], rtol=1e-5) and np.allclose(ab2[np.isfinite(ab2)], 2 * atom_bound[np.isfinite(ab2)], rtol=1e-5)
    # the same restatement evaluated in float32 stays inside the bound: it is neither vacuous nor violated by plain float32
    st32, _ = V._vina_score_host(*(b[k] for k in C.SCORE_KEYS), dtype=np.float32)
    assert st32.atom.dtype == np.float32
    with np.errstate(invalid="ignore", divide="ignore"):
        fa = np.abs(st32.atom.astype(np.float64) - st.atom) / atom_bound
        fm = np.abs(st32.mol[:, :7].astype(np.float64) - st.mol[:, :7]) / mol_bound
    print("float32 restatement / bound, per term (atoms):", np.nanmax(fa, 0), "(molecules, inter, score):", np.nanmax(fm, 0))
    assert np.nanmax(fa) <= 1.0 and np.nanmax(fm) <= 1.0
    assert np.nanmax(fa) > 1e-3                                                  # and the bound is within three decades of it
    # the batch was built to exercise every term, hbond in both directions, and the cutoff
    assert (st.mol[live][:, :5].max(0) > 0).all()
    off, goff = b["mol_off"], b["group_off"]
    gives = takes = beyond = False
    for m in (2, 3, 4, 12, 13):
        lo, hi, glo, ghi = off[m], off[m + 1], goff[b["mol_group"][m]], goff[b["mol_group"][m] + 1]
        r, r32, d, counted, hyd, hb = V._molecule_pairs(b["lig_x"][lo:hi], b["lig_code"][lo:hi], b["poc_x"][glo:ghi],
                                                        b["poc_code"][glo:ghi], np.float64)
        ci, cj = b["lig_code"][lo:hi, None], b["poc_code"][None, glo:ghi]
        close = counted & (d < 0)
        gives |= bool((close & ((ci & 96) == V.DONOR) & ((cj & 96) == V.ACCEPTOR)).any())      # the ligand gives the hydrogen
        takes |= bool((close & ((ci & 96) == V.ACCEPTOR) & ((cj & 96) == V.DONOR)).any())      # the ligand takes it
        beyond |= bool((~counted & ((ci & 15) == 1) & ((cj & 15) == 1)).any())                 # typed pairs beyond 8 A
    assert gives and takes and beyond
    assert not st.atom[off[b["untyped_mol"]]:off[b["untyped_mol"] + 1]].any()


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_front_end_argument_handling(tmp_path):
    x, t, m = torch.zeros((2, 3)), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    pocket = V.TypedPocket(np.zeros((1, 3), np.float32), np.asarray([1], np.int32))
    with pytest.raises(_lib.HipLibraryError):
        V.vina_score(x, t, m, [pocket], "crossdock")
    with pytest.raises(_lib.HipLibraryError):
        V.type_ligands(x, t, m, "crossdock")
    with pytest.raises(_lib.HipLibraryError):
        V.score_molecules([(np.zeros((1, 3)), ["C"])], [pocket], device="cpu")
    with pytest.raises(ValueError, match="bonds"):
        V.score_molecules([(np.zeros((1, 3)), ["C"])], [pocket], bonds="guess")
    with pytest.raises(ValueError, match="bond list"):
        V.score_molecules([(np.zeros((1, 3)), ["C"])], [pocket], bonds="file")
    with pytest.raises(ValueError, match="atom decoder"):
        V.score_molecules([(np.zeros((1, 3)), ["Se"])], [pocket])
    with pytest.raises(ValueError, match="offsets"):
        V.VinaPocket(torch.zeros((2, 3)), torch.zeros(2, dtype=torch.int32), [0, 3])
    with pytest.raises(ValueError, match="bond"):
        V.orders_from_bonds(2, [(2, 0, 1)])
    assert V.class_table(C.DECODER).tolist() == [1, 2, 3, 5, 0, 8, 7, 4, 9, 6]
    # heavy atoms only, bonds renumbered
    (xyz, el, bonds), = V.as_ligands([(np.arange(12).reshape(4, 3), ["C", "H", "o", "Cl"], [(1, 0, 1), (2, 0, 2), (3, 2, 1)])])
    assert el == ["C", "O", "Cl"] and bonds == [(1, 0, 2), (2, 1, 1)] and xyz[:, 0].tolist() == [0, 6, 9]
    # the record of a fragment: rows kept, sums and rotors recomputed
    rec = V.MolVina(np.zeros(8, np.float32), np.asarray([4, 0, 1, 0], np.int32), np.arange(20, dtype=np.float32).reshape(4, 5),
                    np.asarray([17, 17, 17, 17], np.int32))
    part = rec.subset([0, 1, 2], [(1, 0, 1), (2, 1, 1)])
    assert part.n_atoms == 3 and part.n_rot == 0 and part.terms.tolist() == [15, 18, 21, 24, 27]
    assert part.inter == pytest.approx(float(np.dot(V.WEIGHTS, [15, 18, 21, 24, 27])), rel=1e-6) and part.score == part.inter
    # objective: larger = better = minus the score; a pose that is not finite ranks last
    class Gen:
        device, dataset_info = torch.device("cpu"), {"atom_decoder": C.DECODER}
    value = V.objective(Gen, [])
    good, bad, nan = (type("M", (), {"vina": V.MolVina(np.asarray([0, 0, 0, 0, 0, s, s, 0], np.float32), np.zeros(4, np.int32),
                                                      np.zeros((0, 5), np.float32), np.zeros(0, np.int32))})() for s in (-7.5, 2.0, np.nan))
    assert value(good) == 7.5 and value(bad) == -2.0 and value(good) > value(bad) > value(nan) == float("-inf")
    # the SDF reader of the command line, and its parser
    path = tmp_path / "m.sdf"
    path.write_text("m\n\n\n  3  2  0  0  0  0  0  0  0  0\n" + "".join(
        f"{x:10.4f}{0:10.4f}{0:10.4f} {s:<3s} 0  0\n" for x, s in ((0, "C"), (1.5, "O"), (2.4, "H"))) +
        "  1  2  1  0\n  2  3  1  0\nM  END\n$$$$\n")
    (xyz, el, bonds), = V.read_sdf_records(str(path))
    assert el == ["C", "O", "H"] and bonds == [(0, 1, 1), (1, 2, 1)] and xyz[1, 0] == 1.5
    a = V.parse_args(["--pdbfile", "p.pdb", "--sdf", "a.sdf", "b.sdf"])
    assert (a.scope, a.bonds, a.out, a.sdf, a.dataset) == ("protein", "distance", None, ["a.sdf", "b.sdf"], "crossdock")
    assert V.parse_args(["--pdbfile", "p", "--sdf", "a", "--bonds", "file", "--scope", "pocket", "--ref_ligand", "A:1"]).bonds == "file"
    with pytest.raises(SystemExit):
        V.parse_args(["--pdbfile", "p", "--sdf", "a", "--scope", "pocket"])
    with pytest.raises(SystemExit):
        V.parse_args(["--pdbfile", "p", "--sdf", "a", "--bonds", "openbabel"])
    out = tmp_path / "s.csv"
    V.write_csv(str(out), [("a.sdf", 0, part)])
    lines = out.read_text().splitlines()
    assert lines[0].split(",") == ["source", "index"] + list(V.CSV_COLUMNS) and len(lines) == 2 and lines[1].startswith("a.sdf,0,3,0,0,0,")


def test_constants_and_coverage_statements():
    assert V.XS_RADII == {"C": 1.9, "N": 1.8, "O": 1.7, "P": 2.1, "S": 2.0, "F": 1.5, "Cl": 1.8, "Br": 2.0, "I": 2.2, "metal": 1.2}
    assert V.WEIGHTS == (-0.035579, -0.005156, 0.840245, -0.035069, -0.587439) and V.ROT_WEIGHT == 0.05846 and V.CUTOFF == 8.0
    assert V.TILE == 1024 and V.EPS32 == 2.0 ** -24
    low = V.VINA_COVERAGE.lower()
    for word in ("not", "smina", "hydrogens", "rigid", "rotors" if "rotors" in low else "n_rot", "distances"):
        assert word in low, word
    # the statements of the other modules are theirs, unchanged
    assert metrics.METRICS_COVERAGE is __import__("diffsbdd_amd.metrics", fromlist=["x"]).METRICS_COVERAGE
    assert "smina docking score" in metrics.METRICS_COVERAGE and "NOT = a docking score" in pose.POSE_COVERAGE
    assert not hasattr(V, "METRICS_COVERAGE") and not hasattr(V, "POSE_COVERAGE")
    res, args = _lib.SIGNATURES["dsbdd_vina_score"]
    assert len(args) == 14 and len(_lib.SIGNATURES["dsbdd_vina_type"][1]) == 10 and _lib.ABI_VERSION == 6


def test_c_entries_refuse_bad_arguments_without_a_launch():
    lib = _lib.load()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    assert lib.dsbdd_vina_type(None, p, p, p, 0, 1, p, 8, p, p) == _lib.OK                   # batch 0: nothing launched
    assert lib.dsbdd_vina_type(None, None, p, p, 1, 1, p, 8, p, p) == _lib.ERR_ARG and b"null" in lib.dsbdd_last_error()
    assert lib.dsbdd_vina_type(None, p, p, p, -1, 1, p, 8, p, p) == _lib.ERR_ARG
    assert lib.dsbdd_vina_type(None, p, p, p, 1, 0, p, 8, p, p) == _lib.ERR_ARG
    assert lib.dsbdd_vina_type(None, p, p, p, 1, 1, p, 0, p, p) == _lib.ERR_ARG
    assert lib.dsbdd_vina_type(None, p, p, p, 1, 1, p, _lib.MOL_MAX_ATOMS + 1, p, p) == _lib.ERR_ARG and b"n_max" in lib.dsbdd_last_error()
    assert lib.dsbdd_vina_score(None, p, p, p, 0, p, p, p, p, p, 1, p, p, p) == _lib.OK
    assert lib.dsbdd_vina_score(None, p, p, p, -1, p, p, p, p, p, 1, p, p, p) == _lib.ERR_ARG
    assert lib.dsbdd_vina_score(None, p, p, p, 1, p, p, p, p, p, -1, p, p, p) == _lib.ERR_ARG
    for k in (1, 2, 3, 5, 6, 7, 8, 9, 11, 12, 13):
        args = [None, p, p, p, 1, p, p, p, p, p, 1, p, p, p]
        args[k] = None
        assert lib.dsbdd_vina_score(*args) == _lib.ERR_ARG, k
