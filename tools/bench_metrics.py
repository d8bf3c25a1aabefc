"""Molecule-set metrics on the device (`metrics.graph_stats` + `metrics.fp_diversity`: three launches) against the host
path for the part that has one: `build_molecules` (one launch, the order matrices copied to the host) followed by
`Molecule.fragments` and `Molecule.valence_violations` per molecule.

  python tools/bench_metrics.py                 64 pockets x 100 samples of 10-40 atoms, then a 10^5-molecule reference set
  python tools/bench_metrics.py --only device --reps K     K calls and nothing else timed (for a kernel trace)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsbdd_amd import metrics as M  # noqa: E402
from diffsbdd_amd.chem_tables import dataset_info  # noqa: E402
from diffsbdd_amd.molecules import build_molecules  # noqa: E402


def grow_molecule(rng, n):
    """A molecule-like point cloud: every new atom 1.40 Angstrom from a random earlier one, at least 1.3 from all others."""
    x = np.zeros((n, 3))
    for a in range(1, n):
        for _ in range(20):
            d = rng.normal(size=3)
            p = x[rng.randint(a)] + 1.40 * d / np.linalg.norm(d)
            if np.min(np.linalg.norm(x[:a] - p, axis=1)) >= 1.3:
                break
        x[a] = p
    return x.astype(np.float32)


def problem(n_molecules, n_base=800, seed=0):
    """`n_molecules` draws (with repeats) from `n_base` grown molecules of 10-40 atoms; types C/C/N/O."""
    rng = np.random.RandomState(seed)
    base = [grow_molecule(rng, int(rng.randint(10, 41))) for _ in range(n_base)]
    base_t = [rng.choice([0, 0, 1, 2], len(b)).astype(np.int32) for b in base]
    pick = rng.randint(0, n_base, n_molecules)
    sizes = np.asarray([len(base[k]) for k in pick])
    return (np.concatenate([base[k] for k in pick]), np.concatenate([base_t[k] for k in pick]),
            np.repeat(np.arange(n_molecules), sizes).astype(np.int64))


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pockets", type=int, default=64)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--reference", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["device", "host"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing taken anywhere else says nothing about these kernels")
    dev, info = torch.device("cuda:0"), dataset_info("crossdock")
    B = a.pockets * a.samples
    x, t, mask = (torch.as_tensor(v, device=dev) for v in problem(B))
    groups = np.arange(B) // a.samples
    off = np.arange(0, B + 1, a.samples)
    set_metrics = M.MoleculeSetMetrics(info)

    def device_path():
        gs = M.graph_stats(x, t, mask, info, batch=B)
        return gs, M.fp_diversity(gs.fingerprint, off)

    def host_path():
        mols = build_molecules(x, t, mask, info, batch=B)
        return [len(m.fragments()) for m in mols], [len(m.valence_violations()) for m in mols]

    if a.only:
        fn = device_path if a.only == "device" else host_path
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        print(f"{a.only}: {a.reps} calls")
        return
    (gs, _), (frags, viol) = device_path(), host_path()
    st = M._np(gs.stats)
    same = st[:, M.N_FRAGMENTS].tolist() == frags and st[:, M.N_OVER_VALENCE].tolist() == viol
    res = {"molecules": B, "atoms": int(x.shape[0]), "groups": a.pockets, "fragments_and_violations_agree": same}
    res["graph_stats_ms"] = timed(lambda: M.graph_stats(x, t, mask, info, batch=B), a.reps)
    res["fp_diversity_ms"] = timed(lambda: M.fp_diversity(gs.fingerprint, off), a.reps)
    res["device_path_ms"] = timed(device_path, a.reps)
    res["evaluate_ms"] = timed(lambda: set_metrics.evaluate(x, t, mask, groups=groups, batch=B), max(a.reps // 2, 3))
    res["host_path_ms"] = timed(host_path, 3, warmup=1)
    xr, tr, mr = (torch.as_tensor(v, device=dev) for v in problem(a.reference, seed=1))
    res["reference_molecules"] = a.reference
    res["reference_graph_stats_ms"] = timed(lambda: M.graph_stats(xr, tr, mr, info, batch=a.reference), max(a.reps // 4, 3))
    print(f"{B} molecules ({res['atoms']} atoms) in {a.pockets} groups; fragment counts and valence violations of the two "
          f"paths agree: {same}")
    for k, label in (("graph_stats_ms", "graph_stats (bond orders + graph kernel)"), ("fp_diversity_ms", "fp_diversity"),
                     ("device_path_ms", "both, as one call sequence"), ("evaluate_ms", "MoleculeSetMetrics.evaluate (with host part)"),
                     ("host_path_ms", "build_molecules + fragments + valence_violations"),
                     ("reference_graph_stats_ms", f"graph_stats of {a.reference} molecules")):
        med, lo, hi = res[k]
        print(f"  {label:55s} median {med:10.3f} ms  (min {lo:.3f}, max {hi:.3f})")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
