"""Cost of the pose check (`pose.pose_check`: one launch of dsbdd_pose_check) next to its numpy restatement, at the two sizes
of profiles/pose_check.md: one sampling batch (120 molecules of about 25 atoms on one 286-atom pocket) and a test set's
worth (64 pockets x 120 molecules).  Kernel times by device events around the launch alone (outputs allocated before),
warm-up, median of `--reps` launches; the Python entry (allocations and the offsets included) by a host clock around a
synchronised call.

  python tools/bench_pose.py [--reps 30] [--out pose_check.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffsbdd_amd import _lib, pose  # noqa: E402


def problem(n_groups, n_mols, seed=0):
    """`n_groups` pockets (the packaged 3rfm / 5ndu full-atom pockets in turn, each moved somewhere else) with `n_mols`
    ligands of 20-30 atoms each, scattered (sigma 2.5 A) around the crystal ligand's place."""
    rng = np.random.RandomState(seed)
    packaged = [np.load(os.path.join(ROOT, "diffsbdd_amd", "data", f"pocket_{n}.npz")) for n in ("3rfm", "5ndu")]
    radii = np.asarray(sorted(set(pose.VDW_RADII.values())), np.float32)
    pockets, lig_x, lig_r, sizes, groups = [], [], [], [], []
    for g in range(n_groups):
        z = packaged[g % 2]
        move = rng.uniform(-50, 50, 3).astype(np.float32)
        pockets.append((z["fa_x"] + move, rng.choice(radii, len(z["fa_x"])).astype(np.float32)))
        centre = z["ligand_x"].mean(0) + move
        for _ in range(n_mols):
            n = int(rng.randint(20, 31))
            lig_x.append((centre + rng.normal(0, 2.5, (n, 3))).astype(np.float32))
            lig_r.append(rng.choice(radii, n).astype(np.float32))
            sizes.append(n)
            groups.append(g)
    mask = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    pairs = int(sum(n * len(pockets[g][0]) for n, g in zip(sizes, groups)))
    return pockets, np.concatenate(lig_x), np.concatenate(lig_r), mask, np.asarray(groups), pairs


def measure(n_groups, n_mols, reps, dev):
    pockets, x, r, mask, groups, pairs = problem(n_groups, n_mols)
    B = len(groups)
    up = pose.PocketAtoms.upload(pockets, dev)
    xd, rd, md = (torch.as_tensor(v, device=dev) for v in (x, r, mask))
    st = pose.pose_check(xd, rd, md, up, groups, batch=B)
    torch.cuda.synchronize()
    # the launch alone, on the tensors of that call
    lib = _lib.load()
    gd = torch.as_tensor(groups.astype(np.int32), device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    launch = lambda: lib.dsbdd_pose_check(stream, xd.data_ptr(), rd.data_ptr(), st.mol_off.data_ptr(), B, gd.data_ptr(),
                                          up.x.data_ptr(), up.r.data_ptr(), up.group_off.data_ptr(), up.n_groups,
                                          pose.CLASH_TOLERANCE, pose.CONTACT_CUTOFF, st.atom.data_ptr(), st.mol.data_ptr())
    for _ in range(5):
        assert launch() == 0
    torch.cuda.synchronize()
    kernel_ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert launch() == 0
        b.record()
        b.synchronize()
        kernel_ms.append(a.elapsed_time(b))
    call_ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        pose.pose_check(xd, rd, md, up, groups, batch=B)
        torch.cuda.synchronize()
        call_ms.append((time.perf_counter() - t0) * 1e3)
    off = np.concatenate([[0], np.cumsum(np.bincount(mask, minlength=B))])
    px, pr = np.concatenate([p[0] for p in pockets]), np.concatenate([p[1] for p in pockets])
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = pose._pose_check_host(x, r, off, groups, px, pr, up.offsets)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    same = np.array_equal(st.atom.cpu().numpy(), want.atom) and np.array_equal(st.mol.cpu().numpy(), want.mol)
    k, c, h = statistics.median(kernel_ms), statistics.median(call_ms), statistics.median(host_ms)
    return {"groups": n_groups, "molecules": B, "ligand_atoms": int(len(x)), "pocket_atoms": int(len(px)), "pairs": pairs,
            "bitwise_equal_to_restatement": bool(same), "reps": reps,
            "kernel_ms_median": k, "kernel_ms_min": min(kernel_ms), "kernel_ms_max": max(kernel_ms),
            "kernel_pairs_per_s": pairs / (k * 1e-3), "call_ms_median": c, "call_ms_min": min(call_ms),
            "host_restatement_ms_median": h, "host_pairs_per_s": pairs / (h * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing taken anywhere else says nothing about this kernel")
    dev = torch.device("cuda:0")
    res = [measure(1, 120, a.reps, dev), measure(64, 120, a.reps, dev)]
    for r in res:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
