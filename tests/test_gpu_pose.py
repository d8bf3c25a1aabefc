"""GPU: dsbdd_pose_check (csrc/pose_check.h) bit for bit against its numpy restatement in diffsbdd_amd/pose.py, the crystal
fixture against its float64 brute force, and the callers on top: the `pose=` hook of `generate_for_pockets`, its packing
invariance, and the test-set driver refilling slots whose pose clashes.  Small architecture, a handful of steps."""
import ctypes

import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib, pose
from diffsbdd_amd import testset as ts
from tests import _pose_cases as P
from tests.test_gpu_ligand_design import generator

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("lig_x", "lig_r", "mol_off", "mol_group", "poc_x", "poc_r", "group_off")
INF_BITS = int(np.float32(np.inf).view(np.int32))
GUARD, SENTINEL = 7, 0x5A5A5A5A


def launch(b, tol=pose.CLASH_TOLERANCE, contact=pose.CONTACT_CUTOFF):
    """The C entry on a batch of numpy inputs, outputs inside guarded buffers -> (atom, mol, guards intact, inputs after)."""
    lib = _lib.load()
    t = {k: torch.as_tensor(b[k], device=DEV) for k in KEYS}
    N, B = len(b["lig_x"]), len(b["mol_off"]) - 1
    atom = torch.full((N + 2 * GUARD, pose.ATOM_OUT), SENTINEL, dtype=torch.int32, device=DEV)
    mol = torch.full((B + 2 * GUARD, pose.MOL_OUT), SENTINEL, dtype=torch.int32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.dsbdd_pose_check(stream, t["lig_x"].data_ptr(), t["lig_r"].data_ptr(), t["mol_off"].data_ptr(), B,
                              t["mol_group"].data_ptr(), t["poc_x"].data_ptr(), t["poc_r"].data_ptr(),
                              t["group_off"].data_ptr(), len(b["group_off"]) - 1, tol, contact,
                              atom[GUARD:].data_ptr(), mol[GUARD:].data_ptr())
    _lib.check(rc, "dsbdd_pose_check")
    torch.cuda.synchronize()
    atom, mol = atom.cpu().numpy(), mol.cpu().numpy()
    intact = all((part == SENTINEL).all() for part in (atom[:GUARD], atom[GUARD + N:], mol[:GUARD], mol[GUARD + B:]))
    return atom[GUARD:GUARD + N], mol[GUARD:GUARD + B], intact, {k: v.cpu().numpy() for k, v in t.items()}


# 10 --------------------------------------------------------------------------------------------------------------------------
def test_kernel_bitwise_against_the_restatement_on_a_ragged_batch():
    b = P.ragged_batch()
    assert len(b["mol_off"]) - 1 == 16 and len(b["lig_x"]) == 712
    want = pose._pose_check_host(*(b[k] for k in KEYS))
    atom, mol, intact, after = launch(b)
    assert intact                                                       # nothing written before or after the outputs
    for k in KEYS:                                                      # inputs unchanged (NaN compares by bit pattern)
        assert np.array_equal(after[k].view(np.int32), np.ascontiguousarray(b[k]).view(np.int32)), k
    assert atom.dtype == want.atom.dtype and mol.dtype == want.mol.dtype
    bad = np.nonzero((atom != want.atom).any(1))[0]
    assert len(bad) == 0, (bad[:5], atom[bad[:5]], want.atom[bad[:5]])
    assert np.array_equal(mol, want.mol), np.nonzero((mol != want.mol).any(1))[0]
    # the cases the batch was built for did happen
    off = b["mol_off"]
    for m, row in b["exact"].items():
        assert atom[off[m]].tolist() == row
    assert mol[b["nan_mol"], pose.M_NONFINITE] == 1 and mol[:, pose.M_NONFINITE].sum() == 1
    assert mol[0].tolist() == [0, 0, 0, 0, 0, 0, INF_BITS, 0] and mol[7].tolist() == [7, 0, 0, 0, 0, 0, INF_BITS, 0]
    big = atom[off[6]:off[7]]                                           # 300 atoms on the 1025-atom group
    assert (big[:, 0] > 0).any() and (big[:, 0] == 0).any() and big[0, 2] == 1024 and (big[1:, 2] < 1024).any()
    # the same with the other tolerance and cutoff
    atom2, mol2, intact2, _ = launch(b, tol=0.0, contact=3.25)
    want2 = pose._pose_check_host(*(b[k] for k in KEYS), tol=0.0, contact=3.25)
    assert intact2 and np.array_equal(atom2, want2.atom) and np.array_equal(mol2, want2.mol)
    assert not np.array_equal(atom2[:, :2], atom[:, :2])


# 11 --------------------------------------------------------------------------------------------------------------------------
def test_crystal_complexes_against_the_float64_fixture():
    cases, contact = P.fixture_cases()
    assert len(cases) == 8
    for key, (lig_x, lig_el), (poc_x, poc_el), tol, atom64, dmin64 in cases:
        pockets = pose.PocketAtoms.upload([(poc_x, pose.radii_of(poc_el))], DEV)
        st = pose.pose_check(torch.as_tensor(lig_x, device=DEV), torch.as_tensor(pose.radii_of(lig_el), device=DEV),
                             torch.zeros(len(lig_x), dtype=torch.int64, device=DEV), pockets, tol=tol, contact=contact)
        atom, mol = st.atom.cpu().numpy(), st.mol.cpu().numpy()
        assert np.array_equal(atom[:, :3], atom64), key
        want = dmin64.astype(np.float32)
        assert np.all(np.abs(st.atom_distance.cpu().numpy() - want) <= np.spacing(want)), key
        assert mol[0, :6].tolist() == [len(lig_x), atom64[:, 0].sum(), (atom64[:, 0] > 0).sum(), atom64[:, 1].sum(),
                                       (atom64[:, 1] > 0).sum(), 0], key
        # the written-molecule front end: hydrogens dropped, the same record
        rec, = pose.check_molecules([(lig_x, lig_el)], pockets, tol=tol, contact=contact)
        assert np.array_equal(rec.atom, atom) and np.array_equal(rec.mol, mol[0]), key


# 12, 13 ----------------------------------------------------------------------------------------------------------------------
def _pockets():
    """Two different pockets wide enough for an untrained model's samples to meet their atoms (P.ball_residues)."""
    return P.ball_residues(1, 6000), P.ball_residues(2, 5700)


def _jobs():
    res_a, res_b = _pockets()
    return (res_a, 3, torch.tensor([19, 24, 5])), (res_b, 2, torch.tensor([21, 17]))


def _assert_pose_is_the_restatement(m, residues):
    want = pose._check_molecules_host([m], [pose.pocket_atoms(residues)])
    assert np.array_equal(m.pose.atom, want.atom) and np.array_equal(m.pose.mol, want.mol[0])
    assert m.pose.n_atoms == m.num_atoms


def _same_molecule(a, b):
    return a.symbols == b.symbols and np.array_equal(a.positions, b.positions) and a.bonds == b.bonds


def test_generate_for_pockets_hook():
    gen, _ = generator("small_cond")
    job_a, job_b = _jobs()
    kw = dict(timesteps=4, seed=7, sample_ids=torch.arange(5))
    checked = gen.generate_for_pockets([job_a, job_b], pose=True, **kw)
    plain = gen.generate_for_pockets([job_a, job_b], **kw)
    assert [len(p) for p in checked] == [3, 2]
    pairs = [(m.pose.clash_pairs, m.pose.contact_pairs) for mols in checked for m in mols]
    print("clash / contact pairs:", pairs)
    assert sum(c for c, _ in pairs) > 0 and sum(t for _, t in pairs) > 0         # the records are not all empty
    for job, mols, bare in zip((job_a, job_b), checked, plain):
        for m, p in zip(mols, bare):
            _assert_pose_is_the_restatement(m, job[0])
            assert _same_molecule(m, p) and not hasattr(p, "pose")            # the option changes nothing else
    # a dict sets the thresholds
    loose = gen.generate_for_pockets([job_a, job_b], pose=dict(tol=0.0, contact=6.0), **kw)
    for job, mols in zip((job_a, job_b), loose):
        for m in mols:
            want = pose._check_molecules_host([m], [pose.pocket_atoms(job[0])], tol=0.0, contact=6.0)
            assert np.array_equal(m.pose.atom, want.atom) and np.array_equal(m.pose.mol, want.mol[0])
    # largest_frag: the record follows the kept atoms
    frags = gen.generate_for_pockets([job_a, job_b], pose=True, largest_frag=True, **kw)
    assert any(hasattr(m, "n_generated_atoms") for mols in frags for m in mols)          # something was cut
    for job, mols, whole in zip((job_a, job_b), frags, checked):
        for m, w in zip(mols, whole):
            _assert_pose_is_the_restatement(m, job[0])
            assert m.num_atoms <= w.num_atoms
    # the job's pocket atoms were uploaded once
    assert len(gen._pose_pockets) == 2


def test_pose_records_do_not_depend_on_the_packing():
    gen, _ = generator("small_cond")
    job_a, job_b = _jobs()
    ids_a, ids_b = torch.tensor([100, 101, 102]), torch.tensor([7, 8])
    kw = dict(timesteps=4, seed=3, pose=True, cone_mode=2)
    sampler = lambda jobs, ids: _pinned(gen, jobs, ids, kw)
    both = sampler([job_a, job_b], torch.cat([ids_a, ids_b]))
    swapped = sampler([job_b, job_a], torch.cat([ids_b, ids_a]))
    alone_a = sampler([job_a], ids_a)
    for got in (swapped[1], alone_a[0]):
        for m, w in zip(got, both[0]):
            assert _same_molecule(m, w)
            assert np.array_equal(m.pose.atom, w.pose.atom) and np.array_equal(m.pose.mol, w.pose.mol)
    for m, w in zip(swapped[0], both[1]):
        assert np.array_equal(m.pose.atom, w.pose.atom) and np.array_equal(m.pose.mol, w.pose.mol)
    assert sum(m.pose.contact_pairs for mols in both for m in mols) > 0


def _pinned(gen, jobs, ids, kw):
    """generate_for_pockets with the forward cone pinned, as testset.make_hip_sampler does for packing invariance."""
    kw = dict(kw)
    saved = gen.ddpm.cone_mode, gen.ddpm.edge_granule16
    gen.ddpm.cone_mode = kw.pop("cone_mode")
    if saved[1] == "auto":
        gen.ddpm.edge_granule16 = 0
    try:
        return gen.generate_for_pockets(jobs, sample_ids=ids, **kw)
    finally:
        gen.ddpm.cone_mode, gen.ddpm.edge_granule16 = saved


# 14 --------------------------------------------------------------------------------------------------------------------------
def test_driver_refills_slots_whose_pose_clashes():
    gen, _ = generator("small_cond")
    res_a, res_b = _pockets()
    sampler = ts.make_hip_sampler(gen, timesteps=4, seed=5, largest_frag=False, pose=True)

    def fresh():
        return ts.number_jobs([ts.PocketJob("ball_a", res_a, len(res_a), 4, num_nodes_lig=20),
                               ts.PocketJob("ball_b", res_b, len(res_b), 4, num_nodes_lig=14)])

    # K from the first batch: the driver's first batch is a function of (seed, global sample ids) alone
    jobs = fresh()
    plan = ts.plan_batch(sorted(jobs, key=lambda j: (j.n_nodes, j.index)), 8)
    first = {job.name: [m.pose.clash_pairs for m in mols] for (job, _), mols in zip(plan, sampler(plan, 0))}
    counts = first["ball_a"] + first["ball_b"]
    print("clash pairs of the first batch:", counts)
    assert len(counts) == 8 and min(counts) < max(counts), counts
    K = max(c for c in counts if c < max(counts))                   # some pass, the worst do not
    passes = pose.pose_filter(max_clash_pairs=K)
    jobs = fresh()
    drv = ts.TestSetDriver(sampler, 8, is_valid=passes)
    done = drv.run(jobs)
    assert len(drv.batches) >= 2                                     # rejected slots were refilled
    assert sum(j.n_generated for j in done) > 8
    for j in done:
        assert len(j.valid) == j.n_samples == 4                      # cut to n_samples
        assert all(passes(m) and m.pose.clash_pairs <= K for m in j.valid)
        assert len(j.raw) == j.n_generated
    rejected = [m for j in done for m in j.raw if not passes(m)]
    assert rejected and all(m.pose.clash_pairs > K for m in rejected)
    assert [m.pose.clash_pairs for j in done for m in j.raw[:4]] == counts         # the first batch was the one K came from
    summary = pose.summarize_poses([m for j in done for m in j.valid])
    assert summary["n"] == 8 and summary["mean_clash_pairs"] <= K


# 15 --------------------------------------------------------------------------------------------------------------------------
def test_empty_batch_and_device_group_ids():
    pockets = pose.PocketAtoms.upload([(P.EXACT_POCKET_X, P.EXACT_POCKET_R)], DEV)
    none = pose.pose_check(torch.zeros((0, 3), device=DEV), torch.zeros(0, device=DEV),
                           torch.zeros(0, dtype=torch.int64, device=DEV), pockets, batch=0)
    assert tuple(none.atom.shape) == (0, 4) and tuple(none.mol.shape) == (0, 8) and none.molecules() == []
    lib = _lib.load()
    p = pockets.x.data_ptr()
    assert lib.dsbdd_pose_check(None, p, p, p, 0, p, p, p, p, 1, 0.5, 4.0, p, p) == _lib.OK
    # molecules without atoms only
    hollow = pose.pose_check(torch.zeros((0, 3), device=DEV), torch.zeros(0, device=DEV),
                             torch.zeros(0, dtype=torch.int64, device=DEV), pockets, batch=3)
    assert hollow.mol.cpu().tolist() == [[0, 0, 0, 0, 0, 0, INF_BITS, 0]] * 3
    # group ids that are device data are range-checked by the kernel: outside [0, G) reads as an empty group
    x = torch.as_tensor(np.concatenate([P.EXACT_A, P.EXACT_B, P.EXACT_A]), device=DEV)
    r = torch.full((3,), 1.75, device=DEV)
    mask = torch.arange(3, device=DEV)
    st = pose.pose_check(x, r, mask, pockets, mol_group=torch.tensor([0, 99, -1], dtype=torch.int32, device=DEV))
    assert st.atom.cpu().tolist() == [P.EXACT_A_ATOM, [0, 0, -1, INF_BITS], [0, 0, -1, INF_BITS]]
    with pytest.raises(ValueError, match="mol_group"):                    # host data: refused before the launch
        pose.pose_check(x, r, mask, pockets, mol_group=[0, 99, 0])
    # integer class ids go through the decoder's radii
    ids = torch.tensor([6, 6, 6], device=DEV)                             # 'Cl' of the crossdock decoder
    from diffsbdd_amd.chem_tables import dataset_info
    assert dataset_info("crossdock")["atom_decoder"][6] == "Cl"
    typed = pose.pose_check(x, ids, mask, pockets, mol_group=[0, 0, 0], info="crossdock")
    assert typed.atom.cpu().tolist() == [P.EXACT_A_ATOM, P.EXACT_B_ATOM, P.EXACT_A_ATOM]
