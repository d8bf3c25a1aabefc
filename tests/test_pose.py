"""Host logic of diffsbdd_amd/pose.py: the numpy restatement of pose_check_kernel (the specification the GPU tests compare
against) on the crystal fixture and on exact cases, the records and the filter built on it, the argument checks of the C
entry (no launch) and the command line."""
import ctypes

import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib, pose
from diffsbdd_amd.molecules import Molecule
from tests import _pose_cases as P

INF_BITS = int(np.float32(np.inf).view(np.int32))
FIXTURE, CONTACT = P.fixture_cases()


def host(lig, pockets, group=None, tol=pose.CLASH_TOLERANCE, contact=pose.CONTACT_CUTOFF):
    """`_pose_check_host` of ligands [(xyz, radii)] against pockets [(xyz, radii)]."""
    cat = lambda parts, k: np.concatenate([np.asarray(p[k], np.float32) for p in parts])
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])])
    return pose._pose_check_host(cat(lig, 0), cat(lig, 1), off(lig), list(range(len(lig))) if group is None else group,
                                 cat(pockets, 0), cat(pockets, 1), off(pockets), tol, contact)


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FIXTURE, ids=[c[0] for c in FIXTURE])
def test_restatement_equals_the_float64_brute_force_of_the_fixture(case):
    _, (lig_x, lig_el), (poc_x, poc_el), tol, atom64, dmin64 = case
    st = pose._check_molecules_host([(lig_x, lig_el)], [(poc_x, pose.radii_of(poc_el))], tol=tol, contact=CONTACT)
    assert st.atom.dtype == np.int32 and st.mol.dtype == np.int32
    assert np.array_equal(st.atom[:, :3], atom64)                                  # clashes, contacts, nearest: equal
    want = dmin64.astype(np.float32)
    assert np.all(np.abs(st.atom_distance - want) <= np.spacing(want))           # within 1 float32 ulp
    assert st.mol[0].tolist()[:6] == [len(lig_x), atom64[:, 0].sum(), (atom64[:, 0] > 0).sum(), atom64[:, 1].sum(),
                                      (atom64[:, 1] > 0).sum(), 0]
    assert st.min_distance[0] == st.atom_distance.min() and st.mol[0, 7] == 0


def test_fixture_holds_the_anchors_it_was_made_for():
    by = {c[0]: c for c in FIXTURE}
    for name, n_lig, n_poc, contacts, shifted in (("3rfm", 14, 286, 29, 15), ("5ndu", 49, 287, 68, 29)):
        crystal, zero, moved = by[f"{name}_crystal_tol0.5"], by[f"{name}_crystal_tol0.0"], by[f"{name}_shifted_tol0.5"]
        assert len(crystal[1][0]) == n_lig and len(crystal[2][0]) == n_poc
        assert crystal[4][:, 0].sum() == 0 and zero[4][:, 0].sum() == 4 and crystal[4][:, 1].sum() == contacts
        assert moved[4][:, 0].sum() == shifted


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_ties_and_exact_thresholds():
    pocket = (P.EXACT_POCKET_X, P.EXACT_POCKET_R)
    st = host([(P.EXACT_A, P.EXACT_R), (P.EXACT_B, P.EXACT_R)], [pocket], group=[0, 0], tol=0.5, contact=4.0)
    # A: two pocket atoms at d = 3 -> the smaller index; d == 1.75 + 1.75 - 0.5 is no clash; d == 4.0 is no contact
    assert st.atom[0].tolist() == P.EXACT_A_ATOM == [0, 2, 0, st.atom[0, 3]]
    assert st.atom_distance[0] == 3.0
    # B: d = 2 clashes, d == 4.0 to the second atom is no contact
    assert st.atom[1].tolist() == P.EXACT_B_ATOM
    assert st.mol[:, :6].tolist() == [[1, 0, 0, 2, 1, 0], [1, 1, 1, 1, 1, 0]]
    # one ulp of the limit (2^-22 at 3.0: tol 0.5 - 2^-22 is exact in float32) / of the cutoff flips them
    below = host([(P.EXACT_A, P.EXACT_R)], [pocket], tol=0.5 - 2.0 ** -22, contact=4.0)
    assert below.atom[0, 0] == 2
    above = host([(P.EXACT_A, P.EXACT_R)], [pocket], tol=0.5, contact=float(np.nextafter(np.float32(4), np.float32(5))))
    assert above.atom[0, 1] == 3


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    rng = np.random.RandomState(1)
    pa = (rng.uniform(0, 6, (30, 3)).astype(np.float32), np.full(30, 1.7, np.float32))
    pb = (rng.uniform(0, 6, (5, 3)).astype(np.float32), np.full(5, 1.55, np.float32))
    empty = (np.zeros((0, 3), np.float32), np.zeros(0, np.float32))
    m0 = (rng.uniform(0, 6, (4, 3)).astype(np.float32), np.full(4, 1.7, np.float32))
    m_nan = (m0[0].copy(), m0[1])
    m_nan[0][2, 1] = np.nan
    pockets = [pa, empty, pb, pa]                  # group 3 is referenced by nobody
    st = host([m0, empty, m0, m_nan, m0], pockets, group=[2, 0, 1, 0, 0])          # unsorted groups
    off = st.mol_off
    # an empty molecule: a row of its own, no atoms
    assert st.mol[1].tolist() == [0, 0, 0, 0, 0, 0, INF_BITS, 0]
    # an empty group: nothing to clash with
    assert st.mol[2].tolist() == [4, 0, 0, 0, 0, 0, INF_BITS, 0]
    assert st.atom[off[2]:off[3]].tolist() == [[0, 0, -1, INF_BITS]] * 4
    # molecules 0 and 4 are the same atoms on different groups; 4 equals the one-pocket call
    alone = host([m0], [pa])
    assert np.array_equal(st.atom[off[4]:off[5]], alone.atom) and np.array_equal(st.mol[4], alone.mol[0])
    assert not np.array_equal(st.atom[off[0]:off[1]], alone.atom)
    # NaN: the molecule is flagged, the atom has no counts and no nearest, the other atoms are those of the clean molecule
    rows = st.atom[off[3]:off[4]]
    assert st.mol[3, pose.M_NONFINITE] == 1 and st.nonfinite.tolist() == [0, 0, 0, 1, 0]
    assert rows[2].tolist() == [0, 0, -1, INF_BITS]
    assert np.array_equal(np.delete(rows, 2, 0), np.delete(alone.atom, 2, 0))
    # a group id outside [0, G) is an argument error
    with pytest.raises(ValueError, match="mol_group"):
        host([m0], pockets, group=[4])
    with pytest.raises(ValueError, match="mol_group"):
        host([m0], pockets, group=[-1])
    with pytest.raises(ValueError):
        host([m0], [pa], tol=-0.1)
    with pytest.raises(ValueError):
        host([m0], [pa], contact=float("nan"))


def test_radii_and_pocket_atoms():
    assert pose.CLASH_TOLERANCE == 0.5 and pose.CONTACT_CUTOFF == 4.0 and pose.DEFAULT_RADIUS == 2.0
    want = dict(C=1.70, N=1.55, O=1.52, F=1.47, P=1.80, S=1.80, Cl=1.75, Br=1.85, I=1.98, B=1.92, Se=1.90)
    assert pose.VDW_RADII == want
    assert pose.radii_of(["C", "CL", "Zn", "se"]).tolist() == [np.float32(v) for v in (1.70, 1.75, 2.00, 1.90)]
    residues = [dict(chain="A", resseq=1, icode=" ", resname="SER", hetero=False,
                     atoms=[("N", "N", (0.0, 0.0, 0.0)), ("H", "H", (0.0, 1.0, 0.0)), ("CA", "C", (1.0, 0.0, 0.0)),
                            ("D1", "D", (2.0, 0.0, 0.0))]),
                dict(chain="A", resseq=2, icode=" ", resname="HIS", hetero=False,
                     atoms=[("ZN", "Zn", (5.0, 0.0, 0.0)), ("HB", "H", (5.0, 1.0, 0.0)), ("OG", "O", (6.0, 0.0, 0.0))])]
    x, r = pose.pocket_atoms(residues)
    assert x.dtype == np.float32 and r.dtype == np.float32
    assert x.tolist() == [[0, 0, 0], [1, 0, 0], [5, 0, 0], [6, 0, 0]]               # heavy atoms, file order
    assert r.tolist() == [np.float32(v) for v in (1.55, 1.70, 2.00, 1.52)]
    # hydrogens are dropped on the ligand side too
    (lx, lr, keep), = pose.as_ligands([Molecule(np.arange(9, dtype=np.float32).reshape(3, 3), ["C", "H", "Xx"])])
    assert keep.tolist() == [0, 2] and lr.tolist() == [np.float32(1.7), np.float32(2.0)] and lx.tolist() == [[0, 1, 2], [6, 7, 8]]
    with pytest.raises(ValueError, match="hydrogens"):
        pose.radius_table(["C", "H"])


# 4 ---------------------------------------------------------------------------------------------------------------------------
def _with_pose(clash_pairs, contact_atoms, n_atoms, nonfinite=0):
    m = Molecule(np.zeros((n_atoms, 3), np.float32), ["C"] * n_atoms)
    mol = np.asarray([n_atoms, clash_pairs, min(clash_pairs, n_atoms), contact_atoms, contact_atoms, nonfinite, 0, 0], np.int32)
    m.pose = pose.MolPose(mol, np.zeros((n_atoms, 4), np.int32), np.ones(n_atoms, bool))
    return m


def test_pose_filter():
    strict, loose = pose.pose_filter(), pose.pose_filter(max_clash_pairs=2)
    assert strict(_with_pose(0, 0, 5)) and not strict(_with_pose(1, 0, 5))
    assert loose(_with_pose(2, 0, 5)) and not loose(_with_pose(3, 0, 5))
    assert not loose(_with_pose(0, 5, 5, nonfinite=1))
    assert not strict(None)
    frac = pose.pose_filter(max_clash_pairs=0, min_contact_fraction=0.5)
    assert frac(_with_pose(0, 3, 6)) and not frac(_with_pose(0, 2, 6)) and not frac(_with_pose(1, 6, 6))
    assert not frac(_with_pose(0, 0, 0))                                  # no atom is in contact with anything
    with pytest.raises(ValueError, match="pose"):
        strict(Molecule(np.zeros((1, 3), np.float32), ["C"]))            # never passes silently


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_subset_equals_recomputing_on_the_subset():
    b = P.ragged_batch()
    st = pose._pose_check_host(*(b[k] for k in ("lig_x", "lig_r", "mol_off", "mol_group", "poc_x", "poc_r", "group_off")))
    for mol in (5, 3, b["nan_mol"]):
        lo, hi = int(b["mol_off"][mol]), int(b["mol_off"][mol + 1])
        for local in (np.arange(0, hi - lo, 2), np.asarray([1]), np.arange(hi - lo), np.asarray([0, 2, 3, 4])):
            rows = lo + local
            part = st.subset(rows)
            again = pose._pose_check_host(b["lig_x"][rows], b["lig_r"][rows], [0, len(rows)], [b["mol_group"][mol]],
                                          b["poc_x"], b["poc_r"], b["group_off"])
            assert np.array_equal(part.atom, again.atom) and np.array_equal(part.mol, again.mol[0])
            # the same through a molecule's record, and what largest_fragment() carries along
            rec = st.molecules()[mol].subset(local)
            assert np.array_equal(rec.atom, part.atom) and np.array_equal(rec.mol, part.mol)
    whole = st.molecules()
    assert all(np.array_equal(w.mol, st.mol[k]) for k, w in enumerate(whole))
    assert all(np.array_equal(w.subset(np.arange(w.n_atoms)).mol, w.mol) for w in whole)
    m = Molecule(np.zeros((4, 3), np.float32), ["C"] * 4, bonds=[(1, 0, 1), (2, 1, 1)])         # atom 3 alone
    lo = int(b["mol_off"][2])
    m.pose = st.subset(lo + np.arange(4))
    frag = m.largest_fragment()
    assert frag.num_atoms == 3 and np.array_equal(frag.pose.mol, st.subset(lo + np.arange(3)).mol)
    assert frag.pose.as_dict()["n_atoms"] == 3


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_device_entry_points_refuse_cpu_tensors():
    x = torch.zeros((3, 3))
    pocket = [(np.zeros((2, 3), np.float32), np.ones(2, np.float32))]
    with pytest.raises(_lib.HipLibraryError, match="device tensors"):
        pose.pose_check(x, torch.ones(3), torch.zeros(3, dtype=torch.int64), pocket)
    with pytest.raises(_lib.HipLibraryError, match="device tensors"):
        pose.check_molecules([(np.zeros((3, 3), np.float32), ["C", "N", "O"])], pocket, device="cpu")


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_c_entry_refuses_bad_arguments_without_a_launch():
    lib = _lib.load()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)                   # never dereferenced: every call returns before a launch
    good = dict(lig_x=p, lig_r=p, mol_off=p, batch=1, mol_group=p, poc_x=p, poc_r=p, group_off=p, n_groups=1, tol=0.5,
                contact=4.0, atom_out=p, mol_out=p)

    def call(**change):
        a = dict(good, **change)
        return lib.dsbdd_pose_check(None, a["lig_x"], a["lig_r"], a["mol_off"], a["batch"], a["mol_group"], a["poc_x"],
                                    a["poc_r"], a["group_off"], a["n_groups"], a["tol"], a["contact"], a["atom_out"],
                                    a["mol_out"])

    for name in ("lig_x", "lig_r", "mol_off", "mol_group", "poc_x", "poc_r", "group_off", "atom_out", "mol_out"):
        assert call(**{name: None}) == _lib.ERR_ARG, name
        assert b"null" in lib.dsbdd_last_error()
    for change in (dict(batch=-1), dict(n_groups=-1), dict(batch=2 ** 31), dict(tol=-0.5), dict(tol=float("nan")),
                   dict(tol=float("inf")), dict(contact=-1.0), dict(contact=float("nan")), dict(contact=float("inf"))):
        assert call(**change) == _lib.ERR_ARG, change
    assert call(batch=0) == _lib.OK             # nothing to do: no launch
    assert call(batch=0, tol=-1.0) == _lib.ERR_ARG


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_command_line_options():
    a = pose.parse_args(["--pdbfile", "p.pdb", "--sdf", "a.sdf", "b.sdf"])
    assert (a.scope, a.ref_ligand, a.tol, a.contact, a.out, a.sdf) == ("protein", None, 0.5, 4.0, None, ["a.sdf", "b.sdf"])
    a = pose.parse_args(["--pdbfile", "p.pdb", "--sdf", "a.sdf", "--scope", "pocket", "--ref_ligand", "A:330", "--tol", "0.25",
                         "--contact", "4.5", "--out", "pose.csv"])
    assert (a.scope, a.ref_ligand, a.tol, a.contact, a.out) == ("pocket", "A:330", 0.25, 4.5, "pose.csv")
    for bad in (["--scope", "pocket"], ["--scope", "chain"], ["--tol", "-1"]):
        with pytest.raises(SystemExit):
            pose.parse_args(["--pdbfile", "p.pdb", "--sdf", "a.sdf"] + bad)
    with pytest.raises(ValueError, match="ref_ligand"):
        pose.select_residues("p.pdb", "pocket", None)
    for word in ("heavy atoms", "no hydrogens", "rigid protein", "only the residues given", "docking score", "PoseBusters",
                 "PoseCheck"):
        assert word in pose.POSE_COVERAGE, word


def test_csv_and_summary(tmp_path):
    mols = [_with_pose(0, 3, 6), _with_pose(2, 1, 4), None]
    path = tmp_path / "pose.csv"
    pose.write_csv(str(path), [("x.sdf", k, m.pose) for k, m in enumerate(mols[:2])])
    lines = path.read_text().splitlines()
    assert lines[0] == "source,index,n_atoms,clash_pairs,clash_atoms,contact_pairs,contact_atoms,nonfinite,min_distance"
    assert lines[1].startswith("x.sdf,0,6,0,0,3,3,0,") and lines[2].startswith("x.sdf,1,4,2,2,1,1,0,") and len(lines) == 3
    assert pose.summarize_poses(mols) == {"n": 2, "mean_clash_pairs": 1.0, "share_clash_free": 0.5}


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_entry():
    res, args = _lib.SIGNATURES["dsbdd_pose_check"]
    assert res is ctypes.c_int and len(args) == 14
    assert _lib.ABI_VERSION == 6


def test_hooks_are_off_by_default_and_named():
    import inspect

    from diffsbdd_amd import testset
    from diffsbdd_amd.generate import LigandGenerator
    for name in ("generate_ligands", "generate_for_pockets", "inpaint_for_pockets", "diversify_ligands"):
        assert inspect.signature(getattr(LigandGenerator, name)).parameters["pose"].default is None, name
    assert inspect.signature(testset.make_hip_sampler).parameters["pose"].default is None
    assert LigandGenerator._pose_options(None) is None and LigandGenerator._pose_options(False) is None
    assert LigandGenerator._pose_options(True) == {"tol": 0.5, "contact": 4.0}
    assert LigandGenerator._pose_options({"tol": 0.0}) == {"tol": 0.0, "contact": 4.0}
    with pytest.raises(ValueError, match="unknown"):
        LigandGenerator._pose_options({"cutoff": 1.0})
    # the driver's filter: a conjunction, None without any
    both = testset.all_of(pose.pose_filter(0), lambda m: m.num_atoms > 2)
    assert testset.all_of(None, None) is None and both(_with_pose(0, 0, 3)) and not both(_with_pose(0, 0, 2))
    assert not both(_with_pose(1, 0, 3))
