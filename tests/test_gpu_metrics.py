"""GPU: dsbdd_mol_graph_stats and dsbdd_fp_diversity (csrc/mol_metrics.h) against their numpy restatements in
diffsbdd_amd/metrics.py -- integers and keys bit for bit, the float64 pair sums to the rounding of the sum -- and the callers
on top of them: MoleculeSetMetrics, reference_from_dataset, the trainer's `sample_eval` block."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from diffsbdd_amd import _lib
from diffsbdd_amd import metrics as M
from diffsbdd_amd.chem_tables import dataset_info
from tests._golden import GOLDEN_DIR
from tests import _metrics_util as U

pytestmark = pytest.mark.gpu

FULL = dataset_info("crossdock_full")            # its last type, 'others', has no valence entry
MAXV = M.max_valence_table(FULL)
C, N, O, OTHERS = FULL["atom_encoder"]["C"], FULL["atom_encoder"]["N"], FULL["atom_encoder"]["O"], len(MAXV) - 1
FIELDS = ("valence", "label", "stats", "keys", "fingerprint", "type_counts")


def dev():
    return torch.device("cuda:0")


def on_device(mols, n_max=None, in_key=True):
    orders, types, off = U.pack(mols, n_max)
    return M.mol_graph_stats(*(torch.as_tensor(v, device=dev()) for v in (orders, types, off, MAXV)), in_key)


def on_host(mols, n_max=None, in_key=True):
    return M._mol_graph_stats_host(*U.pack(mols, n_max), MAXV, in_key)


def same(a, b, fields=FIELDS):
    for f in fields:
        x, y = M._np(getattr(a, f)), M._np(getattr(b, f))
        assert x.dtype == y.dtype and np.array_equal(x, y), f


def star(centre, leaves, order=1):
    return [centre] + leaves, [(a, 0, order) for a in range(1, len(leaves) + 1)]


def ragged_batch():
    rng = np.random.RandomState(3)
    tree = ([int(t) for t in rng.randint(0, 4, 128)],
            [(a, int(rng.randint(max(a - 6, 0), a)), 1) for a in range(1, 128)] + [(100, 3, 2), (127, 64, 1)])
    return [
        ([], []),                                            # kept by the offsets alone
        ([N], []), ([C, O], [(1, 0, 2)]),
        U.chain(63), U.chain(64, N), U.chain(65),            # lane wrap
        tree,                                                # n = n_max
        U.chain(70),                                         # propagation and BFS depth beyond one wave
        U.chain(65, ring=True),
        ([C, N, O, N, C, C], [(2, 0, 1), (3, 1, 2), (5, 4, 1)]),          # three fragments of two
        ([C, C, N, C], [(2, 1, 3), (1, 0, 1)]),              # triple bond; atom 3 alone
        star(C, [C, C, N, O]), star(C, [C, C, N, O, C]),     # carbon at its limit, and one over it
        star(OTHERS, [C] * 6, order=2),                      # no valence entry: never over
        ([], []),
    ] + U.random_pool(12, seed=7)


@pytest.mark.parametrize("in_key", [True, False])
def test_mol_graph_stats_bitwise_against_the_restatement(in_key):
    mols = ragged_batch()
    got, want = on_device(mols, 128, in_key), on_host(mols, 128, in_key)
    same(got, want)
    st = M._np(got.stats)
    assert st[6].tolist()[:1] == [128] and st[8].tolist() == [65, 65, 0, 1, 65, 0, 0, 0] and st[9].tolist()[3:6] == [3, 2, 0]
    assert st[11, M.N_OVER_VALENCE] == 0 and st[12, M.N_OVER_VALENCE] == 1 and st[13, M.N_OVER_VALENCE] == 0
    assert st[0].tolist() == [0, 0, 0, 0, 0, -1, 0, 0]


def clouds(seed=0, count=12):
    """Random point clouds dense enough to bond: x, types, mask (a sample without atoms in the middle)."""
    rng = np.random.RandomState(seed)
    sizes = [int(n) for n in rng.randint(1, 40, count)]
    sizes[count // 2] = 0
    x = np.concatenate([rng.uniform(0, 1.1 * max(n, 1) ** (1 / 3), (n, 3)) for n in sizes]).astype(np.float32)
    t = rng.choice([C, C, C, N, O, OTHERS], len(x)).astype(np.int32)
    return x, t, np.repeat(np.arange(count), sizes).astype(np.int64), count


def chains(seed=1, count=20):
    """Zig-zag chains of C / N / O, 1.40 Angstrom apart (a single bond for every pair of the three; N-O only just), 1-4
    atoms: mostly valid and connected, with repeats among them."""
    rng = np.random.RandomState(seed)
    sizes = [int(n) for n in rng.randint(1, 5, count)]
    x = np.concatenate([np.stack([1.40 * np.arange(n), 0.02 * rng.rand(n), np.zeros(n)], 1) + rng.uniform(-5, 5, 3)
                        for n in sizes]).astype(np.float32)
    t = rng.choice([C, C, N, O], len(x)).astype(np.int32)
    return x, t, np.repeat(np.arange(count), sizes).astype(np.int64), count


def test_graph_stats_from_coordinates_against_the_restatement():
    x, t, mask, B = clouds()
    got = M.graph_stats(*(torch.as_tensor(v, device=dev()) for v in (x, t, mask)), FULL, batch=B)
    want = M._graph_stats_host(x, t, mask, FULL, batch=B)
    same(got, want)
    assert np.array_equal(M._np(got.sizes), want.sizes) and M._np(got.stats)[:, M.N_BONDS].sum() > 20


def test_results_do_not_depend_on_batch_order_or_n_max():
    mols = ragged_batch()
    mols = [m for m in mols if len(m[0]) <= 70]
    a, b = on_device(mols, 70), on_device(mols[::-1], 128)
    for f in ("stats", "keys", "fingerprint", "type_counts"):
        assert np.array_equal(M._np(getattr(a, f)), M._np(getattr(b, f))[::-1]), f
    off = np.concatenate([[0], np.cumsum([len(m[0]) for m in mols])])
    va, vb = M._np(a.valence), M._np(b.valence)
    la, lb = M._np(a.label), M._np(b.label)
    for k in range(len(mols)):
        lo, hi = off[k], off[k + 1]
        rlo = len(va) - hi
        assert np.array_equal(va[lo:hi], vb[rlo:rlo + hi - lo]) and np.array_equal(la[lo:hi], lb[rlo:rlo + hi - lo])


def test_atlas_keys_on_the_device():
    pytest.importorskip("networkx")
    mols = [m for m, _ in U.atlas_set()]
    got, want = on_device(mols), on_host(mols)
    same(got, want, ("keys", "fingerprint", "stats"))
    assert len(np.unique(got.keys_u64()[:, 0])) == len(np.unique(want.keys_u64()[:, 0]))


def test_fp_diversity_against_float64_numpy():
    rng = np.random.RandomState(5)
    sizes = [0, 1, 2, 3, 130]
    fp = rng.randint(0, 2 ** 32, (sum(sizes), 64), dtype=np.uint64).astype(np.uint32)
    fp[rng.rand(*fp.shape) < 0.5] &= rng.randint(0, 2 ** 32, dtype=np.uint64).astype(np.uint32)
    fp[3], fp[4], fp[5] = 0, 0, 0xFFFFFFFF                   # the group of three: two empty rows and a full one
    fp[10], fp[11], fp[12] = 0, 0xFFFFFFFF, 0
    off = np.concatenate([[0], np.cumsum(sizes)])
    t = torch.as_tensor(fp.view(np.int32), device=dev())
    total, pairs = M.fp_diversity(t, off)
    again, _ = M.fp_diversity(t.clone(), off)
    want, want_pairs = M._fp_diversity_host(fp, off)
    assert pairs.tolist() == want_pairs.tolist() == [0, 0, 1, 3, 8385]
    err = np.abs(M._np(total) - want)
    print("  pair sums", M._np(total).tolist(), " |device - numpy|", err.tolist())
    assert float(total[3]) == 2.0                            # (empty, empty) = 0, (empty, full) = 1 twice
    assert err.max() <= 1e-12
    assert torch.equal(total, again)


def test_molecule_set_metrics_on_the_device_equal_the_restatement():
    (x1, t1, m1, b1), (x2, t2, m2, b2) = chains(), clouds(seed=2, count=4)
    x, t, mask, B = np.concatenate([x1, x2]), np.concatenate([t1, t2]), np.concatenate([m1, m2 + b1]), b1 + b2
    groups = np.arange(B) % 5
    ref = M._graph_stats_host(x, t, mask, FULL, batch=B)
    kw = dict(reference_keys=ref.keys_u64()[::3, 0], reference_type_counts=np.arange(1, len(MAXV) + 1),
              connectivity_thresh=0.6)
    tens = [torch.as_tensor(v, device=dev()) for v in (x, t, mask)]
    got = M.MoleculeSetMetrics(FULL, **kw).evaluate(*tens, groups=groups, batch=B, per_group=True)
    want = M.MoleculeSetMetrics(FULL, _host=True, **kw).evaluate(x, t, mask, groups=groups, batch=B, per_group=True)
    print(" ", {k: v for k, v in got.items() if k != "groups"})
    assert got["n_connected"] > got["n_unique"] >= 3 and got["n_valid"] < B and got["n_groups"] == 5
    for a, b in zip([got] + got["groups"], [want] + want["groups"]):
        for k in b:
            if k == "diversity":
                assert abs(a[k] - b[k]) <= 1e-12, k
            elif k != "groups":
                assert a[k] == b[k], k


def test_reference_from_dataset_in_two_chunkings():
    from diffsbdd_amd.dataset import ProcessedDataset
    info = dataset_info("crossdock")
    ds = ProcessedDataset(os.path.join(GOLDEN_DIR, "trainer_complexes.npz"), device=dev())
    k1, c1 = M.reference_from_dataset(ds, info, chunk=4)
    k2, c2 = M.reference_from_dataset(ds, info, chunk=1)
    assert k1.dtype == np.uint64 and np.array_equal(k1, k2) and np.array_equal(k1, np.sort(k1)) and np.array_equal(c1, c2)
    assert c1.sum() == 45 and 1 <= len(k1) <= 6
    # the same six ligands as the items of trainer_dataset.npz hold them (uncentred)
    z = np.load(os.path.join(GOLDEN_DIR, "trainer_dataset.npz"))
    items = {k: [torch.as_tensor(z[f"item{i}_{k}"]) for i in range(int(z["n"]))] for k in ("lig_coords", "lig_one_hot")}
    k3, c3 = M.reference_from_dataset(SimpleNamespace(items=items, device=torch.device("cpu")), info, chunk=5)
    assert np.array_equal(c3, c1) and np.array_equal(k3, k1)
    host = M._graph_stats_host(torch.cat(ds.items["lig_coords"]), torch.cat(ds.items["lig_one_hot"]).argmax(1),
                               np.repeat(np.arange(6), [len(v) for v in ds.items["lig_coords"]]), info)
    assert np.array_equal(np.unique(host.keys_u64()[:, 0]), k1)


def test_entry_points_refuse_bad_arguments_without_launching():
    lib = _lib.load()
    p = ctypes.c_void_p(4096)                                # never dereferenced: the checks come first
    args = lambda **kw: [kw.get("order", p), p, p, kw.get("batch", 1), 3, p, kw.get("n_max", 8), 1, p, p, p, p, p, p]
    assert lib.dsbdd_mol_graph_stats(None, *args(order=None)) == _lib.ERR_ARG and b"null" in lib.dsbdd_last_error()
    assert lib.dsbdd_mol_graph_stats(None, *args(n_max=_lib.MOL_MAX_ATOMS + 1)) == _lib.ERR_ARG
    assert b"n_max" in lib.dsbdd_last_error()
    assert lib.dsbdd_mol_graph_stats(None, *args(n_max=0)) == _lib.ERR_ARG
    assert lib.dsbdd_mol_graph_stats(None, *args(batch=-1)) == _lib.ERR_ARG
    assert lib.dsbdd_fp_diversity(None, None, p, 1, p, p) == _lib.ERR_ARG
    assert lib.dsbdd_fp_diversity(None, ctypes.c_void_p(4100), p, 1, p, p) == _lib.ERR_ARG and b"aligned" in lib.dsbdd_last_error()
    assert lib.dsbdd_fp_diversity(None, p, p, -1, p, p) == _lib.ERR_ARG
    with pytest.raises(ValueError, match="exceeds the supported 128"):
        M.graph_stats(torch.zeros((129, 3), device=dev()), torch.zeros(129, dtype=torch.int32, device=dev()),
                      torch.zeros(129, dtype=torch.int64, device=dev()), FULL)


# ---- the trainer's sample_eval block -------------------------------------------------------------------------------------------
def _sample_records(tr):
    return [r for r in map(json.loads, open(tr.metrics_path)) if "sample/validity" in r]


def test_trainer_sample_eval_logs_records_and_leaves_the_training_alone(tmp_path):
    from diffsbdd_amd import train as T
    from tests.test_gpu_trainer import HIST, _same, _state, complexes, small_config
    ds = complexes()
    block = dict(every_n_epochs=1, n_samples=5, batch_size=3, timesteps=20)

    def config(name, **extra):
        cfg = small_config(tmp=tmp_path / name)
        cfg.update(n_epochs=2, **extra)
        return cfg

    a = T.Trainer(config("a", sample_eval=block), HIST, ds, ds, device=dev())
    a.fit()
    assert a.ddpm.training
    plain = T.Trainer(config("plain"), HIST, ds, ds, device=dev())
    plain.fit()
    _same(_state(a), _state(plain))                          # bitwise: weights, optimiser state, clip queue, step
    recs = _sample_records(a)
    print(" ", recs)
    assert [r["epoch"] for r in recs] == [0, 1] and [r["step"] for r in recs] == [3, 6] and not _sample_records(plain)
    for r in recs:
        for k in ("validity", "connectivity", "uniqueness", "novelty", "diversity"):
            assert 0.0 <= r["sample/" + k] <= 1.0, k
        assert r["sample/n"] == 5 >= r["sample/n_valid"] >= r["sample/n_connected"] >= r["sample/n_unique"] >= 0
        assert r["sample/validity"] == r["sample/n_valid"] / 5 and np.isfinite(r["sample/kl_div_atom_types"])
    # stop after the first epoch, resume from its checkpoint: the second epoch's record is the uninterrupted run's
    b = T.Trainer(config("b", sample_eval=block), HIST, ds, ds, device=dev())
    b.fit(max_steps=3)
    assert b.epoch == 1 and _sample_records(b) == [recs[0]]
    c = T.Trainer.resume(os.path.join(b.ckpt_dir, "last.ckpt"), ds, ds, device=dev())
    assert c.sample_eval == block
    c.fit()
    assert _sample_records(c) == recs
    _same(_state(a), _state(c))


def test_trainer_sample_eval_of_the_joint_model(tmp_path):
    """The joint model draws whole complexes with `ddpm.sample`: one group, sizes from the joint size distribution."""
    from diffsbdd_amd import train as T
    from tests.test_gpu_trainer import HIST, complexes, small_config
    ds = complexes()
    cfg = small_config("small_joint", tmp=tmp_path)
    cfg.update(n_epochs=1, sample_eval=dict(n_samples=3, batch_size=2))
    tr = T.Trainer(cfg, HIST, ds, ds, device=dev())
    tr.fit()
    (rec,) = _sample_records(tr)
    print(" ", rec)
    assert tr.ddpm.training and rec["epoch"] == 0 and rec["step"] == 3
    assert rec["sample/n"] == 3 >= rec["sample/n_valid"] >= rec["sample/n_connected"] >= rec["sample/n_unique"] >= 0
    for k in ("validity", "connectivity", "uniqueness", "novelty", "diversity"):
        assert 0.0 <= rec["sample/" + k] <= 1.0, k
