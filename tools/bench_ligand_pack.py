"""Packed ligand batch of the design front ends: `ligand_io.pack_ligands` (one launch of dsbdd_pack_ligands) against
the torch restatement of the reference's loop over samples (inpaint.py:114-141; tests/test_ligand_design.py
`reference_host_loop`, on the device like the reference's `model.device`).

  python tools/bench_ligand_pack.py                      warmed medians of both, outputs compared bitwise
  python tools/bench_ligand_pack.py --only pack --reps K   K calls and nothing else timed: run it under
  python tools/bench_ligand_pack.py --only torch --reps K  `rocprofv3 --kernel-trace --stats` to count launches
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffsbdd_amd import ligand_io  # noqa: E402
from tests.test_ligand_design import reference_host_loop  # noqa: E402


def problem(n_samples, n_fixed, atom_nf, seed=0):
    """One substructure for all samples (the reference's case), sizes n_fixed .. n_fixed + 19."""
    rng = np.random.RandomState(seed)
    tmpl = (rng.normal(scale=4.0, size=(n_fixed, 3)).astype(np.float32), rng.randint(0, atom_nf, n_fixed).astype(np.int32))
    sizes = (n_fixed + rng.randint(0, 20, n_samples)).tolist()
    return [tmpl], [0] * n_samples, sizes


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    total, enqueue = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        enqueue.append((t1 - t0) * 1e3)
        total.append((t2 - t0) * 1e3)
    return statistics.median(total), statistics.median(enqueue), min(total), max(total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_samples", type=int, default=512)
    ap.add_argument("--n_fixed", type=int, default=12)
    ap.add_argument("--atom_nf", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", choices=["pack", "torch"], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing taken anywhere else says nothing about this kernel")
    dev = "cuda:0"
    templates, slot_tmpl, sizes = problem(a.n_samples, a.n_fixed, a.atom_nf)
    tmpl_x, tmpl_t, tmpl_sizes = ligand_io.upload_templates(templates, dev)
    pack = lambda: ligand_io.pack_ligands(tmpl_x, tmpl_t, tmpl_sizes, slot_tmpl, sizes, a.atom_nf)
    loop = lambda: reference_host_loop(templates, slot_tmpl, sizes, a.atom_nf, device=dev)
    if a.only:
        fn = pack if a.only == "pack" else loop
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        print(f"{a.only}: {a.reps} calls")
        return
    (lig, fixed), (ref, ref_fixed) = pack(), loop()
    same = all(torch.equal(lig[k].cpu(), ref[k].cpu()) for k in ("x", "one_hot", "mask", "size")) and \
        torch.equal(fixed, ref_fixed)
    p = timed(pack, a.reps, 10)
    t = timed(loop, max(a.reps // 5, 5), 2)
    print(f"n_samples = {a.n_samples}, n_fixed = {a.n_fixed}, rows = {sum(sizes)}, outputs bitwise equal: {same}")
    print(f"pack_ligands    median {p[0]:8.3f} ms per call (host returns after {p[1]:.3f} ms; min {p[2]:.3f}, max {p[3]:.3f}; {a.reps} calls)")
    print(f"reference loop  median {t[0]:8.3f} ms per call (host returns after {t[1]:.3f} ms; min {t[2]:.3f}, max {t[3]:.3f})")
    print(f"ratio {t[0] / p[0]:.0f} x")


if __name__ == "__main__":
    main()
