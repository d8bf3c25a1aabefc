"""Cost of the fused score + gradient launch (dsbdd_vina_score_grad) against the score launch alone (dsbdd_vina_score), and
the observed error of the gradient as a fraction of `vina.grad_error_bound`: the figures of profiles/vina_grad.md and
profiles/vina_grad_error.md.

Cost: two batches -- the ragged batch of the tests (tests/_vina_grad_cases.grad_batch: 17 molecules of 0..300 atoms on
groups of 0..3077 pocket atoms) and 64 molecules of 20-30 atoms scattered inside one synthetic pocket of 400 typed atoms at
protein density (one atom per 60 cubic A; seeded).  Device events around windows of `--launches` launches after warm-up,
the two entries alternating window by window, median over `--rounds` windows each.  `--baseline_lib`: a build of the
library at another commit, whose dsbdd_vina_score is timed in the same process as the score launch `as it was`; without
it only this build's two entries are timed.

  python tools/bench_vina_grad.py [--rounds 15] [--launches 200] [--baseline_lib other/libdiffsbdd_hip.so] [--out vina_grad.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffsbdd_amd import _lib, vina  # noqa: E402
from tests import _vina_cases as C  # noqa: E402
from tests import _vina_grad_cases as GC  # noqa: E402


def pocket_batch(n_mols=64, n_pocket=400, seed=0):
    rng = np.random.RandomState(seed)
    box = (60.0 * n_pocket) ** (1.0 / 3.0)
    codes = C._CODES[:16]
    sizes = rng.randint(20, 31, n_mols)
    return {"lig_x": rng.uniform(0, box, (int(sizes.sum()), 3)).astype(np.float32),
            "lig_code": rng.choice(codes, int(sizes.sum())).astype(np.int32),
            "mol_off": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), "mol_group": np.zeros(n_mols, np.int32),
            "mol_int": np.stack([sizes, 0 * sizes, rng.randint(0, 11, n_mols), 0 * sizes], 1).astype(np.int32),
            "poc_x": rng.uniform(0, box, (n_pocket, 3)).astype(np.float32), "poc_code": rng.choice(codes, n_pocket).astype(np.int32),
            "group_off": np.asarray([0, n_pocket], np.int32)}


def windows(entries, launches, rounds):
    """entries: {name: launch}; windows of `launches` launches, the entries alternating -> {name: ms per launch, median}."""
    for launch in entries.values():
        for _ in range(20):
            launch()
    torch.cuda.synchronize()
    ms = {name: [] for name in entries}
    for _ in range(rounds):
        for name, launch in entries.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                launch()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / launches)
    return {name: {"median_us": 1e3 * statistics.median(v), "min_us": 1e3 * min(v), "max_us": 1e3 * max(v)} for name, v in ms.items()}


def cost(b, dev, launches, rounds, baseline):
    lib = _lib.load()
    t = {k: torch.as_tensor(np.ascontiguousarray(b[k]), device=dev) for k in C.SCORE_KEYS}
    N, B, G = len(b["lig_x"]), len(b["mol_off"]) - 1, len(b["group_off"]) - 1
    f32 = dict(dtype=torch.float32, device=dev)
    outs = [[torch.zeros((N, 5), **f32), torch.zeros((B, 8), **f32), torch.zeros(B, dtype=torch.int32, device=dev)] for _ in range(3)]
    grads = [torch.zeros((N, 3), **f32), torch.zeros((B, 8), **f32)]
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    head = (stream, t["lig_x"].data_ptr(), t["lig_code"].data_ptr(), t["mol_off"].data_ptr(), B, t["mol_group"].data_ptr(),
            t["mol_int"].data_ptr(), t["poc_x"].data_ptr(), t["poc_code"].data_ptr(), t["group_off"].data_ptr(), G)
    ptrs = lambda ts: tuple(v.data_ptr() for v in ts)

    def score():
        assert lib.dsbdd_vina_score(*head, *ptrs(outs[0])) == 0

    def fused():
        assert lib.dsbdd_vina_score_grad(*head, *ptrs(outs[1]), *ptrs(grads)) == 0

    entries = {"vina_score": score, "vina_score_grad": fused}
    if baseline is not None:
        def before():
            assert baseline.dsbdd_vina_score(*head, *ptrs(outs[2])) == 0
        entries = {"vina_score_baseline": before, **entries}
    res = windows(entries, launches, rounds)
    counted = int(sum(GC.molecule_pairs(b, m)[4].sum() for m in range(B)))
    res.update(molecules=B, ligand_atoms=N, pocket_atoms=int(len(b["poc_x"])), counted_pairs=counted, launches=launches, rounds=rounds,
               grad_over_score=res["vina_score_grad"]["median_us"] / res["vina_score"]["median_us"],
               score_outputs_bitwise_equal=bool(all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs[0], outs[1]))))
    if baseline is not None:
        res.update(grad_over_baseline_score=res["vina_score_grad"]["median_us"] / res["vina_score_baseline"]["median_us"],
                   baseline_outputs_bitwise_equal=bool(all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                                                           for x, y in zip(outs[0], outs[2]))))
    return res, (grads[0].cpu().numpy(), grads[1].cpu().numpy())


def fractions(b, got):
    want, grad_bound, mol_bound = vina._vina_grad_host(*(b[k] for k in C.SCORE_KEYS), eps=vina.EPS32)
    with np.errstate(invalid="ignore", divide="ignore"):
        fa = np.abs(got[0].astype(np.float64) - want.grad) / grad_bound
        fm = np.abs(got[1].astype(np.float64) - want.mol_grad) / mol_bound
    fa, fm = np.where(np.isfinite(fa), fa, 0.0), np.where(np.isfinite(fm), fm, 0.0)
    return {"atom_grad": float(fa.max()), "net": float(fm[:, :3].max()), "moment": float(fm[:, 3:6].max()),
            "max_norm": float(fm[:, 6].max()), "rot_factor": float(fm[:, 7].max()), "kink_margin": float(want.kink_margin)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--baseline_lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing taken anywhere else says nothing about these kernels")
    dev = torch.device("cuda:0")
    _lib.load()
    baseline = None
    if a.baseline_lib:
        baseline = ctypes.CDLL(a.baseline_lib)
        baseline.dsbdd_vina_score.restype, baseline.dsbdd_vina_score.argtypes = _lib.SIGNATURES["dsbdd_vina_score"]
    res = {"device": torch.cuda.get_device_name(0), "baseline_lib": a.baseline_lib}
    for name, b in (("ragged_batch", GC.grad_batch()), ("pocket_400_x64", pocket_batch())):
        res[name], got = cost(b, dev, a.launches, a.rounds, baseline)
        res[name]["error_over_bound"] = fractions(b, got)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
