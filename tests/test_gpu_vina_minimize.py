"""GPU: dsbdd_vina_minimize (csrc/vina_minimize.h) through the C ABI: its rows at the returned pose bit for bit against
dsbdd_vina_score_grad on that pose, monotone, rigid and bounded, one step replayed from the gradient launch's rows, the
one-atom cases against the wells of the pair energy, bitwise reproducibility under re-packing, the front ends, and the
device against the float64 restatement `vina._vina_minimize_host` (status classes; the table is printed).  Outputs live in
guarded sentinel buffers."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib, vina as V
from diffsbdd_amd.molecules import Molecule, write_sdf
from tests import _vina_cases as C
from tests import _vina_grad_cases as GC
from tests import _vina_min_cases as MC
from tests import test_gpu_vina_kernels as K
from tests.test_gpu_vina_grad import _crystal, bits, launch_grad

pytestmark = pytest.mark.gpu

DEV = K.DEV
NAMES = ("atom", "mol", "flag", "grad", "mol_grad", "x", "pose", "energies", "stat")
BUDGET = 24


def launch_min(b, step=V.MIN_STEP, tol=V.MIN_TOL, max_evals=V.MIN_EVALS):
    """dsbdd_vina_minimize on a batch of numpy inputs -> dict of NAMES: the five outputs of `launch_grad`, x [N,3], pose [B,8],
    energies [B,4] (float32) and stat [B,4] (int32); rows nothing was written to hold the sentinel's bit pattern."""
    lib = _lib.load()
    t = {k: torch.as_tensor(np.ascontiguousarray(b[k]), device=DEV) for k in C.SCORE_KEYS}
    N, B = len(b["lig_x"]), len(b["mol_off"]) - 1
    shapes = ((N, V.ATOM_OUT), (B, V.MOL_OUT), (B, 0), (N, V.ATOM_GRAD), (B, V.MOL_GRAD), (N, 3), (B, V.MOL_POSE), (B, V.MOL_MIN),
              (B, V.MOL_STAT))
    bufs = [K._guarded(*s) for s in shapes]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda k: (t[k] if t[k].numel() else torch.zeros(4, dtype=t[k].dtype, device=DEV)).data_ptr()
    out = [buf[K.GUARD:].data_ptr() for buf in bufs]
    rc = lib.dsbdd_vina_minimize(stream, ptr("lig_x"), ptr("lig_code"), ptr("mol_off"), B, ptr("mol_group"), ptr("mol_int"),
                                 ptr("poc_x"), ptr("poc_code"), ptr("group_off"), len(b["group_off"]) - 1, *out[:5],
                                 float(step), float(tol), int(max_evals), *out[5:])
    _lib.check(rc, "dsbdd_vina_minimize")
    torch.cuda.synchronize()
    assert all(K._intact(buf, s[0]) for buf, s in zip(bufs, shapes))          # nothing written before or after the outputs
    K._unchanged(t, b, C.SCORE_KEYS)
    got = [buf.cpu().numpy()[K.GUARD:K.GUARD + s[0]] for buf, s in zip(bufs, shapes)]
    return {name: (a if name in ("flag", "stat") else a.view(np.float32)) for name, a in zip(NAMES, got)}


def same(a, b, names=NAMES):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in names)


def at_pose(b, x):
    out = dict(b)
    out["lig_x"] = np.ascontiguousarray(x)
    return out


@functools.lru_cache(maxsize=None)
def ragged():
    """`grad_batch()` minimised with a budget of 24 evaluations: one launch, shared by the tests that read it."""
    return launch_min(GC.grad_batch(), max_evals=BUDGET)


# 1 ---------------------------------------------------------------------------------------------------------------------------
def test_returned_rows_are_those_of_the_gradient_launch_on_the_returned_pose():
    b = GC.grad_batch()
    assert len(b["mol_off"]) - 1 == 17 and np.diff(b["mol_off"]).tolist()[:6] == [5, 3, 20, 33, 25, 300]
    got = ragged()
    live = np.arange(17) != b["nan_mol"]
    assert np.isfinite(got["x"][np.repeat(live, np.diff(b["mol_off"]))]).all()
    want = launch_grad(at_pose(b, got["x"]))
    for name, w in zip(NAMES[:5], want):
        assert np.array_equal(bits(got[name]), bits(w)), name
    assert np.array_equal(bits(got["energies"][:, V.E_FINAL]), bits(want[1][:, V.M_INTER]))
    start = launch_grad(b)
    assert np.array_equal(bits(got["energies"][:, V.E_START]), bits(start[1][:, V.M_INTER]))
    assert got["stat"][:, V.S_ACCEPTED].max() >= 5 and not np.array_equal(got["x"], b["lig_x"])     # something did move


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_monotone_rigid_and_bounded():
    b = GC.grad_batch()
    got = ragged()
    E, stat, off = got["energies"], got["stat"], b["mol_off"]
    live = np.arange(17) != b["nan_mol"]
    assert (E[live, V.E_FINAL] <= E[live, V.E_START]).all()
    first = MC.first_step()
    print("first step, per molecule (E at the input, E after 0.25 A, margin):", first.tolist())
    for m in (2, 3, 4, 5, 6, 12, 13, 14):
        assert first[m, 0] - first[m, 1] > first[m, 2] and first[m, 0] > 20, (m, first[m])           # above the score's error: a clash
        assert E[m, V.E_FINAL] < E[m, V.E_START] and stat[m, V.S_ACCEPTED] >= 1, m
    assert (stat[live, V.S_EVALS] <= BUDGET + 1).all() and (stat[live, V.S_EVALS] >= 1).all() and (stat[:, 3] == 0).all()
    assert (stat[:, V.S_ACCEPTED] <= stat[:, V.S_EVALS]).all() and np.isin(stat[live, V.S_STATUS], (0, 1, 2)).all()
    used = MC.check_rigid(b["lig_x"], got["x"], got["pose"], off, skip=(b["nan_mol"],))
    print("largest fraction of the pose tolerance, of the distance tolerance:", used)
    for m in (0, b["empty_mol"], b["untyped_mol"], 10):                      # empty group, no atoms, all untyped, group id out of range
        rows = slice(off[m], off[m + 1])
        assert stat[m].tolist() == [2, 1, 0, 0] and np.array_equal(bits(got["x"][rows]), bits(b["lig_x"][rows])), m
        assert got["pose"][m, :7].tolist() == [0, 0, 0, 1, 0, 0, 0] and E[m].tolist() == [0, 0, 0, 0] and not got["grad"][rows].any()
    m = b["nan_mol"]
    rows = slice(off[m], off[m + 1])
    assert stat[m].tolist() == [3, 0, 0, 0] and got["flag"][m] == 1 and got["flag"].sum() == 1
    assert np.array_equal(bits(got["x"][rows]), bits(b["lig_x"][rows]))
    for name in ("atom", "grad"):
        assert np.isnan(got[name][rows]).all(), name
    for name in ("mol", "mol_grad", "pose", "energies"):
        assert np.isnan(got[name][m]).all(), name


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_one_step_replayed_from_the_gradient_launch():
    b = GC.grad_batch()
    cases = [C.sub_batch(b, [m])[0] for m in (2, 6, 15)] + [MC.one_atom(r0) for r0 in MC.STARTS]
    seen = set()
    for k, one in enumerate(cases):
        _, mol0, _, _, mg0 = launch_grad(one)
        xt = MC.trial_coordinates(one, V.MIN_STEP, rows=(mg0[0, V.G_NET], mg0[0, V.G_MOMENT]))
        moved = np.sqrt(((xt.astype(np.float64) - one["lig_x"]) ** 2).sum(1)).max()
        assert 0 < moved <= V.MIN_STEP + 4 * MC.ulp32(np.abs(xt).max())      # no atom moves more than L (and two roundings)
        trial = at_pose(one, xt)
        _, mol1, _, _, _ = launch_grad(trial)
        E0, E1 = mol0[0, V.M_INTER], mol1[0, V.M_INTER]
        bound = V.error_bound(*(trial[key] for key in C.SCORE_KEYS))[1][0, V.M_INTER]
        print(f"case {k}: E = {E0!r}, E' = {E1!r}, twice the bound {2 * bound:.3e}")
        assert abs(float(E1) - float(E0)) > 2 * bound, k                     # the decision does not hang on a rounding
        got = launch_min(one, max_evals=2)
        accepted = bool(E1 < E0)
        seen.add(accepted)
        assert got["stat"][0].tolist() == [0, 2 if accepted else 3, int(accepted), 0], k
        if accepted:
            assert (np.abs(got["x"].astype(np.float64) - xt) <= MC.ulp32(xt)).all(), k
            assert got["energies"][0, V.E_STEP] == np.float32(V.MIN_STEP)
        else:
            assert np.array_equal(bits(got["x"]), bits(one["lig_x"])), k
            assert got["energies"][0, V.E_STEP] == 0 and got["pose"][0, :7].tolist() == [0, 0, 0, 1, 0, 0, 0]
        assert np.array_equal(bits(got["energies"][0, V.E_START]), bits(E0))
    assert True in seen


# 4 ---------------------------------------------------------------------------------------------------------------------------
def test_one_atom_cases_converge_to_their_wells():
    got = launch_min(MC.one_atom_batch())
    for k, r0 in enumerate(MC.STARTS):
        r = float(np.linalg.norm(got["x"][k].astype(np.float64)))
        print(f"r0 = {r0}: r_final = {r:.5f}, target {MC.target(r0):.5f}, stat {got['stat'][k].tolist()}")
        assert got["stat"][k, V.S_STATUS] == 1 and abs(r - MC.target(r0)) <= 2 * MC.TOL, (r0, r)
        assert got["stat"][k, V.S_EVALS] <= V.MIN_EVALS + 1


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_bitwise_reproducible_and_independent_of_the_batch():
    b = GC.grad_batch()
    first, again = ragged(), launch_min(b, max_evals=BUDGET)
    assert same(first, again)
    off = b["mol_off"]
    per_atom = ("atom", "grad", "x")
    for m in (2, 5, 16):                                                    # each alone
        one, rows = C.sub_batch(b, [m])
        got = launch_min(one, max_evals=BUDGET)
        for name in NAMES:
            want = first[name][rows] if name in per_atom else first[name][m:m + 1]
            assert np.array_equal(bits(got[name]), bits(want)), (m, name)
    order = np.random.RandomState(4).permutation(17).tolist()              # the batch with its molecules permuted
    assert order != sorted(order)
    perm, rows = C.sub_batch(b, order)
    got = launch_min(perm, max_evals=BUDGET)
    for name in NAMES:
        want = first[name][rows] if name in per_atom else first[name][order]
        assert np.array_equal(bits(got[name]), bits(want)), name


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_front_end_on_the_displaced_crystal_fixture():
    z = C.fixture()
    for name in z["names"]:
        x, at, mask, pockets, decoder, orders = _crystal(z, name)
        moved = MC.rigid_motion(z[f"{name}_crystal_x"])                       # 0.5 A and 10 degrees, float64, here
        xm = torch.as_tensor(moved, device=DEV)
        keep = xm.clone()
        st = V.vina_minimize(xm, at, mask, pockets, decoder, orders=orders)
        assert isinstance(st, V.VinaMinimized) and torch.equal(xm, keep) and st.x.data_ptr() != xm.data_ptr()
        assert tuple(st.x.shape) == (len(x), 3) and tuple(st.pose.shape) == (1, 8) and tuple(st.energies.shape) == (1, 4)
        assert int(st.status[0]) in (0, 1, 2) and 1 <= int(st.evals[0]) <= V.MIN_EVALS + 1 and int(st.accepted[0]) <= int(st.evals[0])
        assert float(st.score[0]) <= float(st.score_start[0])
        assert torch.equal(st.score_start, st.energies[:, 0] * st.mol_grad[:, 7]) and torch.equal(st.inter_start, st.energies[:, 0])
        want = np.sqrt(((st.x.cpu().numpy().astype(np.float64) - moved.astype(np.float64)) ** 2).sum(1).mean())
        assert st.rmsd.dtype == torch.float64 and float(st.rmsd[0]) == pytest.approx(want, rel=1e-12)
        ref = V.vina_score(st.x, at, mask, pockets, decoder, orders=orders)
        assert torch.equal(ref.mol.view(torch.int32), st.mol.view(torch.int32)) and torch.equal(ref.atom.view(torch.int32), st.atom.view(torch.int32))
        start = V.vina_score(xm, at, mask, pockets, decoder, orders=orders)
        assert torch.equal(start.inter, st.inter_start)
        print(f"{name}: score {float(start.score[0]):.4f} -> {float(st.score[0]):.4f}, status {V.STATUS[int(st.status[0])]}, evals {int(st.evals[0])}, rmsd {float(st.rmsd[0]):.3f}")
        rec, = st.molecules()
        assert isinstance(rec, V.MolVinaMin) and np.array_equal(rec.x, st.x.cpu().numpy()) and rec.rmsd == float(st.rmsd[0])
        assert rec.status == int(st.status[0]) and rec.score_start == pytest.approx(float(st.score_start[0]), rel=1e-6)
    with pytest.raises(_lib.HipLibraryError):
        V.vina_minimize(xm.cpu(), at.cpu(), mask.cpu(), pockets, decoder, orders=orders.cpu())
    with pytest.raises(ValueError, match="max_evals"):
        V.vina_minimize(xm, at, mask, pockets, decoder, orders=orders, max_evals=0)


def test_front_end_on_batches_without_atoms():
    """N = 0: both coordinate pointers are stand-ins, which must be two addresses (the C entry refuses lig_x == x_out)."""
    pockets = V.VinaPocket.upload([V.TypedPocket(np.asarray([[3.8, 0, 0]], np.float32), np.asarray([17], np.int32))], DEV)
    empty = lambda: (torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV),
                     torch.zeros(0, dtype=torch.int64, device=DEV))
    for _ in range(2):                                                      # a second call reuses whatever the first one freed
        none = V.vina_minimize(*empty(), pockets, "crossdock", batch=0)
        assert tuple(none.x.shape) == (0, 3) and tuple(none.pose.shape) == (0, 8) and tuple(none.stat.shape) == (0, 4)
        assert tuple(none.rmsd.shape) == (0,) and none.molecules() == []
        hollow = V.vina_minimize(*empty(), pockets, "crossdock", batch=3)
        assert hollow.stat.cpu().tolist() == [[2, 1, 0, 0]] * 3 and hollow.flag.cpu().tolist() == [0, 0, 0]
        assert hollow.pose.cpu().tolist() == [[0, 0, 0, 1, 0, 0, 0, 1]] * 3 and not hollow.energies.cpu().numpy().any()
        assert not hollow.mol.cpu().numpy().any() and hollow.rmsd.cpu().tolist() == [0, 0, 0] and tuple(hollow.x.shape) == (0, 3)
        recs = hollow.molecules()
        assert len(recs) == 3 and all(r.status == 2 and r.evals == 1 and r.x.shape == (0, 3) and r.rmsd == 0 for r in recs)
    assert V.minimize_molecules([], pockets) == [] and V.gradient_molecules([], pockets) == []
    # one carbon 4.4 A from a hydrophobic carbon beside a molecule without atoms: the first moves, the second has no gradient
    st = V.vina_minimize(torch.tensor([[4.4, 0, 0]], device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
                         torch.zeros(1, dtype=torch.int64, device=DEV), pockets, "crossdock", mol_group=[0, 0], batch=2)
    assert st.status.cpu().tolist() == [1, 2] and float(st.inter[0]) < float(st.inter_start[0]) and float(st.rmsd[0]) > 0


def test_generator_and_samplers_attach_the_relaxation(tmp_path):
    from tests.test_gpu_ligand_design import generator
    from tests.test_ligand_design import PDB
    pdb = tmp_path / "c.pdb"
    pdb.write_text(PDB)
    gen, _ = generator("small_cond")
    residues = gen.select_pocket_residues(str(pdb), ref_ligand="A:100")
    job = [(residues, 2, torch.tensor([9, 14]))]
    (plain,) = gen.generate_for_pockets(job, timesteps=4, seed=5, sample_ids=torch.arange(2), vina=True)
    (mols,) = gen.generate_for_pockets(job, timesteps=4, seed=5, sample_ids=torch.arange(2), vina={"minimize": {"max_evals": 40}})
    assert len(mols) == 2 and not any(hasattr(m, "vina_min") for m in plain)
    pockets = V.VinaPocket.upload([V.type_pocket(residues)], DEV)
    recs = V.minimize_molecules(mols, pockets, gen.dataset_info, max_evals=40)
    out = gen.vina_minimize(str(pdb), mols, ref_ligand="A:100", scope="pocket", max_evals=40)
    for m, p, r, o in zip(mols, plain, recs, out):
        assert np.array_equal(m.positions, p.positions) and m.vina.as_dict() == p.vina.as_dict()      # the sample itself is untouched
        rec = m.vina_min
        heavy = sum(e not in ("H", "D") for e in m.symbols)
        assert isinstance(rec, V.MolVinaMin) and rec.x.shape == (heavy, 3) and rec.x.dtype == np.float32
        assert rec.inter_start == m.vina.inter and rec.status in (0, 1, 2) and rec.evals <= 41
        assert not np.isfinite(rec.inter) or rec.inter <= rec.inter_start
        assert np.array_equal(bits(r.x), bits(rec.x)) and r.as_dict() == rec.as_dict()                # the written-molecule path agrees
        assert np.array_equal(o["x"], r.x) and np.array_equal(o["grad"], r.grad)
        assert {k: o[k] for k in r.as_dict()} == r.as_dict() and set(V.MIN_CSV_COLUMNS) <= set(o)
    with pytest.raises(ValueError, match="minimize"):
        gen.generate_for_pockets(job, timesteps=4, seed=5, sample_ids=torch.arange(2), vina={"minimize": {"evals": 3}})


def test_command_line_writes_the_relaxed_molecules(tmp_path, capsys):
    from tests.test_gpu_vina import _fixture_pdb
    z = C.fixture()
    pdb, sdf, out, relaxed = tmp_path / "p.pdb", tmp_path / "l.sdf", tmp_path / "scores.csv", tmp_path / "relaxed.sdf"
    _fixture_pdb(pdb, z, "5ndu")
    el, bonds = C.fixture_ligand(z, "5ndu")
    bonds = [(max(i, j), min(i, j), o) for i, j, o in bonds]
    write_sdf(str(sdf), [Molecule(MC.rigid_motion(z["5ndu_crystal_x"]), el, bonds), Molecule(z["5ndu_shifted_x"][:3], el[:3], [])])
    rows = V.main(["--pdbfile", str(pdb), "--sdf", str(sdf), "--bonds", "file", "--out", str(out), "--minimize", str(relaxed),
                   "--max_evals", "60", "--device", DEV])
    err = capsys.readouterr().err
    assert V.VINA_COVERAGE in err and V.VINA_MIN_COVERAGE in err
    lines = out.read_text().splitlines()
    assert lines[0].split(",") == ["source", "index"] + list(V.MIN_CSV_COLUMNS) and len(lines) == 3 and len(rows) == 2
    back = V.read_sdf_records(str(relaxed))
    given = V.read_sdf_records(str(sdf))
    assert len(back) == 2
    for k, ((xyz, elements, bd), (_, el0, bd0), (_, _, rec)) in enumerate(zip(back, given, rows)):
        assert elements == el0 and bd == bd0
        assert np.abs(xyz - rec.x).max() <= 0.5e-4 + 1e-6                     # the SDF's four decimals
        cells = dict(zip(lines[0].split(","), lines[k + 1].split(",")))
        assert int(cells["status"]) == rec.status and int(cells["evals"]) == rec.evals <= 61
        assert float(cells["inter_start"]) == rec.inter_start and float(cells["score"]) == rec.score and float(cells["rmsd"]) == rec.rmsd
        assert rec.score <= rec.score_start
    # what the file holds scores as the row says, to the four decimals of its coordinates
    pockets = V.VinaPocket.upload([V.type_pocket(C.fixture_residues(z, "5ndu"))], DEV)
    again = V.score_molecules(str(relaxed), pockets, bonds="file")
    assert again[0].score == pytest.approx(rows[0][2].score, abs=0.05)
    plain = V.main(["--pdbfile", str(pdb), "--sdf", str(sdf), "--bonds", "file", "--out", str(tmp_path / "plain.csv"), "--device", DEV])
    assert (tmp_path / "plain.csv").read_text().splitlines()[0].split(",") == ["source", "index"] + list(V.CSV_COLUMNS)
    assert plain[0][2].inter == rows[0][2].inter_start


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_device_against_the_restatement_status_classes():
    b = C.score_batch()
    want, _ = MC.min_reference()
    got = launch_min(b)
    print("molecule | device E_final, evals, status | restatement E_final, evals, status | E_start")
    for m in range(16):
        print(f"{m:2d} | {got['energies'][m, V.E_FINAL]:12.6f} {got['stat'][m, V.S_EVALS]:4d} {V.STATUS[got['stat'][m, V.S_STATUS]]:11s} | "
              f"{want.energies[m, V.E_FINAL]:12.6f} {want.stat[m, V.S_EVALS]:4d} {V.STATUS[want.stat[m, V.S_STATUS]]:11s} | "
              f"{got['energies'][m, V.E_START]:12.6f}")
    live = np.arange(16) != b["nan_mol"]
    assert (got["energies"][live, V.E_FINAL] <= got["energies"][live, V.E_START]).all()
    assert MC.status_class(got["stat"]) == MC.status_class(want.stat)
