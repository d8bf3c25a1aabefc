"""Host logic of diffsbdd_amd/metrics.py: the numpy restatements of the two kernels (the specification the GPU tests compare
against), MoleculeSetMetrics on a hand-built set, the trainer's config key and the command line."""
import itertools
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch

from diffsbdd_amd import metrics as M
from diffsbdd_amd.chem_tables import dataset_info
from tests._golden import GOLDEN_DIR
from tests import _metrics_util as U

INFO = dataset_info("crossdock")
MAXV = M.max_valence_table(INFO)
C, N, O = (INFO["atom_encoder"][s] for s in "CNO")


def stats_of(mols, in_key=True, n_max=None):
    return M._mol_graph_stats_host(*U.pack(mols, n_max), MAXV, in_key)


def keys_of(mols, in_key=True):
    return stats_of(mols, in_key).keys_u64()[:, 0]


def golden_ligands():
    """The ligands of the 6-complex trainer file as (types, edges), bonds from the distance tables."""
    z = np.load(os.path.join(GOLDEN_DIR, "trainer_complexes.npz"))
    types, mask = z["lig_one_hot"].argmax(1), z["lig_mask"]
    off = np.concatenate([[0], np.cumsum(np.bincount(mask))]).astype(np.int32)
    orders = M._bond_orders_host(z["lig_coords"], types, off, INFO, int(np.diff(off).max()))
    out = []
    for b in range(len(off) - 1):
        ii, jj = np.nonzero(orders[b])
        out.append(([int(t) for t in types[off[b]:off[b + 1]]], [(int(i), int(j), int(orders[b, i, j])) for i, j in zip(ii, jj)]))
    return out


@pytest.fixture(scope="module")
def pool():
    return U.random_pool(300, seed=0) + golden_ligands()


def test_key_does_not_depend_on_the_atom_order(pool):
    rng = np.random.RandomState(1)
    shuffled = [U.renumber(m, rng.permutation(len(m[0])).tolist()) for m in pool]
    a, b = stats_of(pool), stats_of(shuffled)
    assert np.array_equal(a.keys_u64(), b.keys_u64())
    assert np.array_equal(a.fingerprint, b.fingerprint) and np.array_equal(a.stats[:, :5], b.stats[:, :5])
    assert np.array_equal(keys_of(pool, False), keys_of(shuffled, False))


def test_equal_keys_are_isomorphic_molecules_on_the_pool(pool):
    nx = pytest.importorskip("networkx")
    from networkx.algorithms.isomorphism import categorical_edge_match, categorical_node_match
    keys = keys_of(pool)
    graphs = [U.to_networkx(m) for m in pool]
    nm, em = categorical_node_match("t", None), categorical_edge_match("o", None)
    n_iso = 0
    for i, j in itertools.combinations(range(len(pool)), 2):
        if len(pool[i][0]) != len(pool[j][0]):
            assert keys[i] != keys[j]
            continue
        iso = nx.is_isomorphic(graphs[i], graphs[j], node_match=nm, edge_match=em)
        n_iso += iso
        assert iso == (keys[i] == keys[j]), (pool[i], pool[j])
    print(f"  {n_iso} isomorphic pairs in the pool, all key-equal; no false merge")
    assert n_iso >= 1


def test_atlas_low_cycle_rank_graphs_get_distinct_keys():
    pytest.importorskip("networkx")
    atlas = U.atlas_set()
    assert len(atlas) == 461
    keys = keys_of([m for m, _ in atlas])
    low = np.asarray([rank <= 2 for _, rank in atlas])
    assert low.sum() == 149 and len(np.unique(keys[low])) == 149
    print(f"  atlas: {len(np.unique(keys))} distinct keys over {len(atlas)} graphs (not asserted)")
    kd, kb = keys_of([U.DECALIN, U.BICYCLOPENTYL])
    assert kd != kb


def test_bond_order_switch():
    single, double = ([C, C, O], [(1, 0, 1), (2, 1, 1)]), ([C, C, O], [(1, 0, 1), (2, 1, 2)])
    a, b = keys_of([single, double])
    assert a != b
    a, b = keys_of([single, double], in_key=False)
    assert a == b
    assert keys_of([double])[0] != keys_of([double], in_key=False)[0]


def test_fragment_tie_keeps_the_fragment_of_atom_0():
    # atoms 0-2 and 1-3 bonded: two fragments of two; then a third, smaller one
    mol = ([C, N, O, N, C], [(2, 0, 1), (3, 1, 2)])
    gs = stats_of([mol])
    assert gs.label.tolist() == [0, 1, 0, 1, 4]
    assert gs.stats[0].tolist() == [5, 2, 0, 3, 2, 0, 0, 0]
    assert gs.valence.tolist() == [1, 2, 1, 2, 0]
    # the largest fragment's key is the key of that fragment alone; the whole sample's is another
    assert gs.keys_u64()[0, 0] == keys_of([([C, O], [(1, 0, 1)])])[0] != gs.keys_u64()[0, 1]
    swapped = ([N, C, N, O, C], [(2, 0, 2), (3, 1, 1)])               # now atom 0's fragment is N=N
    assert stats_of([swapped]).keys_u64()[0, 0] == keys_of([([N, N], [(1, 0, 2)])])[0]


def test_restatement_does_not_depend_on_batch_or_n_max(pool):
    a, b = stats_of(pool[:40]), stats_of(pool[:40][::-1], n_max=17)
    assert np.array_equal(a.keys_u64(), b.keys_u64()[::-1]) and np.array_equal(a.fingerprint, b.fingerprint[::-1])


# ---- MoleculeSetMetrics ------------------------------------------------------------------------------------------------------
def hand_set():
    """x, types, mask, groups of 8 samples (Angstrom; C-C 1.5 single, C-O 1.4 single, C-N 1.45 single):
    0 oxygen with three carbons (over-valent), 1 two C-C fragments, 2 and 3 C-C-O in both atom orders, 4 C-C-N,
    5 empty, 6 one carbon, 7 C-C-O again in another group."""
    mols = [
        ([O, C, C, C], [[0, 0, 0], [1.4, 0, 0], [0, 1.4, 0], [0, 0, 1.4]]),
        ([C, C, C, C], [[0, 0, 0], [1.5, 0, 0], [10, 0, 0], [11.5, 0, 0]]),
        ([C, C, O], [[0, 0, 0], [1.5, 0, 0], [2.9, 0, 0]]),
        ([O, C, C], [[5, 1, 2.9], [5, 1, 1.5], [5, 1, 0]]),
        ([C, C, N], [[0, 0, 0], [1.5, 0, 0], [2.95, 0, 0]]),
        ([], []),
        ([C], [[1, 2, 3]]),
        ([C, O, C], [[1.5, 0, 0], [2.9, 0, 0], [0, 0, 0]]),
    ]
    x = np.asarray([p for _, pts in mols for p in pts], np.float32).reshape(-1, 3)
    t = np.asarray([a for ts, _ in mols for a in ts], np.int32)
    mask = np.asarray([b for b, (ts, _) in enumerate(mols) for _ in ts], np.int64)
    return x, t, mask, [0, 0, 1, 1, 1, 2, 3, 4]


def popcount_distance(a, b):
    a, b = (int.from_bytes(np.asarray(v).tobytes(), "little") for v in (a, b))
    union = bin(a | b).count("1")
    return 1.0 - bin(a & b).count("1") / union if union else 0.0


def test_molecule_set_metrics_on_a_hand_built_set():
    x, t, mask, groups = hand_set()
    gs = M._graph_stats_host(x, t, mask, INFO, batch=8)
    assert gs.stats[:, M.N_ATOMS].tolist() == [4, 4, 3, 3, 3, 0, 1, 3]
    assert gs.stats[:, M.N_OVER_VALENCE].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert gs.stats[:, M.N_FRAGMENTS].tolist() == [1, 2, 1, 1, 1, 0, 1, 1]
    keys = gs.keys_u64()[:, 0]
    assert keys[2] == keys[3] == keys[7] and len({int(k) for k in keys[[2, 4, 6]]}) == 3
    ref_counts = np.asarray([50, 20, 30, 0, 0, 0, 0, 0, 0, 0])
    m = M.MoleculeSetMetrics(INFO, reference_keys=[keys[4]], reference_type_counts=ref_counts, _host=True)
    r = m.evaluate(x, t, mask, groups=groups, batch=8, per_group=True)
    assert (r["n"], r["n_valid"], r["n_connected"], r["n_unique"], r["n_novel"], r["n_groups"]) == (8, 6, 5, 3, 2, 5)
    assert r["validity"] == 6 / 8 and r["connectivity"] == 5 / 6 and r["uniqueness"] == 3 / 5 and r["novelty"] == 2 / 3
    # diversity: group 0 has no connected molecule, group 1 the pairs (2,3) (2,4) (3,4), groups 2-4 fewer than two molecules
    d = popcount_distance(gs.fingerprint[2], gs.fingerprint[4])
    assert popcount_distance(gs.fingerprint[2], gs.fingerprint[3]) == 0.0 and 0.0 < d < 1.0
    per = {g["group"]: g for g in r["groups"]}
    assert per[1]["diversity"] == pytest.approx(2 * d / 3, abs=1e-15) and per[1]["uniqueness"] == 2 / 3
    assert [per[g]["diversity"] for g in (0, 2, 3, 4)] == [0.0] * 4 and per[3]["n_connected"] == 1
    assert r["diversity"] == pytest.approx(2 * d / 3 / 5, abs=1e-15)
    # the KL divergence, written out: counts over ALL generated atoms, invalid samples included
    counts = np.bincount(t, minlength=10).astype(np.float64)
    p, q = ref_counts / ref_counts.sum(), counts / counts.sum()
    expect = -sum(p[k] * math.log(q[k] / p[k] + 1e-10) for k in range(3))
    assert r["kl_div_atom_types"] == pytest.approx(expect, abs=1e-15)
    # thresh 0.5: sample 1 counts as connected through its first C-C fragment
    half = M.MoleculeSetMetrics(INFO, connectivity_thresh=0.5, _host=True).evaluate(x, t, mask, groups=groups, batch=8)
    assert (half["n_connected"], half["n_unique"]) == (6, 4) and half["uniqueness"] == 4 / 6
    assert half["novelty"] is None and half["n_novel"] is None and half["kl_div_atom_types"] == -1


def test_zero_denominators_give_zero():
    m = M.MoleculeSetMetrics(INFO, reference_keys=[], reference_type_counts=np.ones(10), _host=True)
    none = m.evaluate(np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int64), batch=0)
    for k in ("validity", "connectivity", "uniqueness", "novelty", "diversity"):
        assert none[k] == 0.0, k
    assert none["n"] == none["n_groups"] == 0 and math.isfinite(none["kl_div_atom_types"])
    x, t, mask, _ = hand_set()
    bad = m.evaluate(x[:4], t[:4], mask[:4], batch=2)           # one over-valent sample and an empty one
    assert (bad["n"], bad["n_valid"]) == (2, 0)
    assert bad["validity"] == bad["connectivity"] == bad["uniqueness"] == bad["novelty"] == bad["diversity"] == 0.0
    frag = m.evaluate(x[4:8], t[4:8], mask[4:8] - 1, batch=1)   # valid but not connected
    assert (frag["n_valid"], frag["n_connected"], frag["validity"]) == (1, 0, 1.0)
    assert frag["connectivity"] == frag["uniqueness"] == frag["novelty"] == 0.0


def test_fp_diversity_restatement_by_hand():
    fp = np.zeros((4, 64), np.uint32)
    fp[0, 0], fp[1, 63] = 0b0111, 0b1110 << 28                        # rows 2 and 3 stay empty
    total, pairs = M._fp_diversity_host(fp.view(np.int32), [0, 0, 1, 4, 4])
    assert pairs.tolist() == [0, 0, 3, 0] and total[2] == 1.0 + 1.0 + 0.0    # (1,2) (1,3): nothing shared; (2,3): empty union
    total, pairs = M._fp_diversity_host(fp.view(np.int32), [0, 2])
    assert pairs.tolist() == [1] and total[0] == 1.0
    fp[1, 0] = 0b1110
    assert M._fp_diversity_host(fp.view(np.int32), [0, 2])[0][0] == 1 - 2 / 7     # |a & b| = 2, |a | b| = 4 + 3


def test_device_entry_points_refuse_cpu_tensors():
    from diffsbdd_amd._lib import HipLibraryError
    x, t, mask, _ = hand_set()
    with pytest.raises(HipLibraryError):
        M.graph_stats(torch.as_tensor(x), torch.as_tensor(t), torch.as_tensor(mask), INFO)
    with pytest.raises(HipLibraryError):
        M.fp_diversity(torch.zeros((2, 64), dtype=torch.int32), [0, 2])


# ---- config and command line -------------------------------------------------------------------------------------------------
def _config(**extra):
    return dict(dataset="crossdock", datadir=".", mode="pocket_conditioning", batch_size=2, lr=1e-3, n_epochs=1,
                egnn_params={}, diffusion_params={}, **extra)


def test_sample_eval_is_a_config_key_of_its_own():
    from diffsbdd_amd.train import check_config
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cfg = check_config(_config(sample_eval=dict(every_n_epochs=2, n_samples=4, batch_size=2, timesteps=10)))
        check_config(_config())
    assert cfg["sample_eval"]["n_samples"] == 4
    with pytest.warns(UserWarning, match=r"accepted and ignored: eval_epochs, eval_params \(no wandb, visualisation or "
                                         r"RDKit-based evaluation in this trainer\)"):
        check_config(_config(eval_params={"n_eval_samples": 10}, eval_epochs=5))
    for bad in ({"n_sample": 4}, {"n_samples": 0}, {"timesteps": 2.5}, [1]):
        with pytest.raises(ValueError):
            check_config(_config(sample_eval=bad))


def test_command_line_on_a_tiny_sdf(tmp_path, monkeypatch, capsys):
    from diffsbdd_amd.molecules import Molecule, write_sdf
    x, t, mask, _ = hand_set()
    dec = INFO["atom_decoder"]
    mols = [Molecule(x[mask == b], [dec[a] for a in t[mask == b]]) for b in range(8)]
    write_sdf(tmp_path / "a.sdf", [mols[2], mols[3], mols[4]])
    write_sdf(tmp_path / "b.sdf", [mols[0], mols[6]])
    monkeypatch.setattr(M, "graph_stats", M._graph_stats_host)
    monkeypatch.setattr(M, "fp_diversity", M._fp_diversity_host)
    out = tmp_path / "metrics.json"
    res = M.main(["--sdf", str(tmp_path / "a.sdf"), str(tmp_path / "b.sdf"), "--dataset", "crossdock", "--device", "cpu",
                  "--out", str(out)])
    printed = capsys.readouterr().out
    assert M.METRICS_COVERAGE in printed and json.loads(printed.strip().splitlines()[-1])["n"] == 5
    saved = json.loads(out.read_text())
    assert saved == json.loads(json.dumps(res)) and saved["coverage"] == M.METRICS_COVERAGE
    assert (saved["n"], saved["n_valid"], saved["n_connected"], saved["n_unique"], saved["n_groups"]) == (5, 4, 4, 3, 2)
    assert saved["novelty"] is None and saved["kl_div_atom_types"] == -1
    ga, gb = saved["groups"]
    assert ga["name"].endswith("a.sdf") and (ga["n"], ga["n_unique"]) == (3, 2) and ga["diversity"] > 0
    assert gb["name"].endswith("b.sdf") and (gb["n"], gb["n_valid"], gb["diversity"]) == (2, 1, 0.0)
    assert saved["diversity"] == pytest.approx(ga["diversity"] / 2)
    for word in ("QED", "SanitizeMol", "RDKFingerprint", "SMILES", "not proven isomorphic"):
        assert word in M.METRICS_COVERAGE
