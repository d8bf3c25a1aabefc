#!/usr/bin/env python
"""Wall time of `EnVariationalDiffusion.nll_of_complex` against the loop of evaluation-mode `forward` calls it replaces
(profiles/score_joint.md).

Problem: a shipped joint architecture at its real width with seeded random weights, the example full-atom pocket (3rfm,
286 atoms) repeated, 23-atom anchored ligands, every complex centred on the host.  Route A is one `nll_of_complex` call
with K time slots per complex; route B is K evaluation-mode `ddpm(ligand, pocket)` calls on the same complexes with the
grid's k-th time injected (each call: its own t = 0 pass, two network calls, the terms in torch).  HIP events around
each call, the profiler off; warm-up calls of both routes, then rounds alternating the two.

    python tools/score_joint_bench.py [--workload moad_fullatom_joint] [--complexes 16] [--n_times 10] [--max_states 64]
    python tools/score_joint_bench.py --trace-calls 2     # only route A, for a kernel trace of its own"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from diffsbdd_amd import score, synthetic as S  # noqa: E402
from train_step_bench import build  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="moad_fullatom_joint")
    ap.add_argument("--complexes", type=int, default=16)
    ap.add_argument("--n_lig", type=int, default=23)
    ap.add_argument("--n_times", type=int, default=10)
    ap.add_argument("--max_states", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls of each route per round")
    ap.add_argument("--trace-calls", type=int, default=0, help="run only this many nll_of_complex calls (after one warm-up)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_joint_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    model, cfg, dd = build(a.workload, dev)
    assert not dd["conditional"], f"{a.workload} is not a joint architecture"
    model.eval()
    B, K, T = a.complexes, a.n_times, dd["timesteps"]
    ligand = S.anchor_ligand(B, a.n_lig, cfg["atom_nf"], dev)
    pocket = S.load_pocket("fa", B, dev)
    n_p = pocket["x"].shape[0] // B
    mean = torch.cat([ligand["x"].view(B, -1, 3), pocket["x"].view(B, n_p, 3)], 1).double().mean(1).float()
    ligand["x"] = ligand["x"] - mean[ligand["mask"]]
    pocket["x"] = pocket["x"] - mean[pocket["mask"]]
    times, _ = score.time_grid(T, K, seed=0)

    def fused():
        return model.nll_of_complex(ligand, pocket, n_times=K, seed=0, max_states=a.max_states)

    def loop():
        out = []
        for k in range(K):
            model.t_int_source = lambda b, k=k: torch.full((b, 1), float(times[k]))
            out.append(model(dict(ligand), dict(pocket)))                 # forward normalises its dicts in place
        model.t_int_source = None
        return out

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    if a.trace_calls:
        fused()
        torch.cuda.synchronize()
        for _ in range(a.trace_calls):
            fused()
        torch.cuda.synchronize()
        return
    model.seed(1)
    for _ in range(a.warmup):
        fused()
        loop()
    torch.cuda.synchronize()
    ms = {"fused": [], "loop": []}
    for _ in range(a.rounds):
        for name, fn in (("fused", fused), ("loop", loop)):
            ms[name] += [timed(fn) for _ in range(a.calls)]
    nll = fused()
    assert bool(torch.isfinite(nll).all())
    res = dict(workload=a.workload, device=torch.cuda.get_device_name(0), complexes=B, n_lig=a.n_lig, n_pocket=n_p,
               n_times=K, T=T, states=B * (K + 1), max_states=a.max_states,
               chunks=len(score._chunks(B * (K + 1), a.max_states)), samples_per_route=len(ms["fused"]))
    for name, v in ms.items():
        res[name + "_ms"] = dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
    res["loop_over_fused"] = round(res["loop_ms"]["median"] / res["fused_ms"]["median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
