"""Cost of the one-launch minimiser (dsbdd_vina_minimize) per evaluation against one dsbdd_vina_score_grad launch, and of a
whole minimisation against the same iteration driven from the host: the figures of profiles/vina_minimize.md.

Two batches, those of tools/bench_vina_grad.py: the ragged batch of the tests and 64 molecules of 20-30 atoms in one
synthetic pocket of 400 typed atoms.  Device events around windows of `--launches` launches after warm-up, the entries
alternating window by window, median over `--rounds` windows each.

The host-driven loop (written here only, as the baseline) is the iteration of `vina._vina_minimize_host` in lockstep over the
batch: per evaluation one dsbdd_vina_score_grad launch on the coordinates of every molecule's pose under evaluation, one
read-back of mol_out and mol_grad, the decisions and the next coordinates in numpy (`vina.pose_step`,
`vina.pose_coordinates`), one upload.  A molecule that has stopped keeps its returned pose in the batch.  Wall time around
whole runs, median over `--rounds` runs after one untimed run; the device launch is timed the same way beside it.

  python tools/bench_vina_minimize.py [--rounds 9] [--launches 5] [--out vina_minimize.json]
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
from diffsbdd_amd import _lib, vina as V  # noqa: E402
from tests import _vina_cases as C  # noqa: E402
from tests import _vina_grad_cases as GC  # noqa: E402
from tools.bench_vina_grad import pocket_batch, windows  # noqa: E402


class Launches:
    """The two entries on one set of device buffers."""

    def __init__(self, b, dev):
        self.lib, self.b, self.dev = _lib.load(), b, dev
        self.t = {k: torch.as_tensor(np.ascontiguousarray(b[k]), device=dev) for k in C.SCORE_KEYS}
        self.N, self.B, self.G = len(b["lig_x"]), len(b["mol_off"]) - 1, len(b["group_off"]) - 1
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        N, B = self.N, self.B
        self.five = [torch.zeros((N, 5), **f32), torch.zeros((B, 8), **f32), torch.zeros(B, **i32), torch.zeros((N, 3), **f32),
                     torch.zeros((B, 8), **f32)]
        self.more = [torch.zeros((N, 3), **f32), torch.zeros((B, 8), **f32), torch.zeros((B, 4), **f32), torch.zeros((B, 4), **i32)]
        self.x = self.t["lig_x"].clone()                                    # the host loop's coordinates
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def head(self, x):
        t = self.t
        return (self.stream, x.data_ptr(), t["lig_code"].data_ptr(), t["mol_off"].data_ptr(), self.B, t["mol_group"].data_ptr(),
                t["mol_int"].data_ptr(), t["poc_x"].data_ptr(), t["poc_code"].data_ptr(), t["group_off"].data_ptr(), self.G)

    def grad(self, x=None):
        assert self.lib.dsbdd_vina_score_grad(*self.head(self.t["lig_x"] if x is None else x), *(v.data_ptr() for v in self.five)) == 0

    def minimize(self, step=V.MIN_STEP, tol=V.MIN_TOL, max_evals=V.MIN_EVALS):
        assert self.lib.dsbdd_vina_minimize(*self.head(self.t["lig_x"]), *(v.data_ptr() for v in self.five), step, tol, max_evals,
                                            *(v.data_ptr() for v in self.more)) == 0

    def host_loop(self, step=V.MIN_STEP, tol=V.MIN_TOL, max_evals=V.MIN_EVALS):
        """The iteration in lockstep from the host -> (x float32 [N,3], stat int32 [B,4], E float32 [B])."""
        step, tol, max_evals = V._settings(step, tol, max_evals)
        b, B, off = self.b, self.B, self.b["mol_off"]
        x_in = np.asarray(b["lig_x"], np.float32)
        mols = []
        for m in range(B):
            x0 = x_in[off[m]:off[m + 1]]
            with np.errstate(invalid="ignore"):
                s = x0.astype(np.float64) - (x0.astype(np.float64).sum(0) / len(x0) if len(x0) else 0.0)
            mols.append(dict(x0=x0, rho2=max(float((s * s).sum() / len(x0)), 1.0) if len(x0) else 1.0,
                             rho_max=float(np.sqrt((s * s).sum(1).max())) if len(x0) else 0.0, pose=(np.zeros(3), np.asarray([1.0, 0, 0, 0])),
                             trial=None, phase="first", E=None, F=None, M=None, L=step, u=0.0, evals=0, accepted=0, rejected=False,
                             status=0, live=bool(np.isfinite(x0).all())))
        x = x_in.copy()
        while any(s["live"] for s in mols):
            self.x.copy_(torch.as_tensor(x, device=self.dev))
            self.grad(self.x)
            mol, mg = self.five[1].cpu().numpy(), self.five[4].cpu().numpy()     # the read-back: it waits for the launch
            for m, s in enumerate(mols):
                if not s["live"]:
                    continue
                E1, F1, M1 = mol[m, V.M_INTER], mg[m, V.G_NET].astype(np.float64), mg[m, V.G_MOMENT].astype(np.float64)
                s["evals"] += 1
                moved = False
                if s["phase"] == "final":
                    s["live"] = False
                    continue
                if s["phase"] == "first":
                    s["E"], s["F"], s["M"], moved = E1, F1, M1, True
                elif E1 < s["E"]:
                    s["pose"], s["E"], s["F"], s["M"], moved = s["trial"], E1, F1, M1, True
                    s["L"], s["accepted"], s["rejected"] = min(2 * s["L"], step), s["accepted"] + 1, False
                else:
                    s["L"], s["rejected"] = 0.5 * s["L"], True
                stop = False
                if moved:
                    s["u"] = V._norm3(s["F"]) + s["rho_max"] * V._norm3(s["M"]) / s["rho2"]
                    if not s["u"] > 0:
                        s["status"], stop = 2, True
                if not stop and s["L"] < tol:
                    s["status"], stop = 1, True
                if not stop and s["evals"] >= max_evals:
                    s["status"], stop = 0, True
                if stop:
                    x[off[m]:off[m + 1]] = V.pose_coordinates(s["x0"], *s["pose"])
                    s["phase"], s["live"] = "final", s["rejected"]
                    continue
                s["trial"] = V.pose_step(*s["pose"], s["F"], s["M"], s["rho2"], s["L"] / s["u"])
                s["phase"] = "trial"
                x[off[m]:off[m + 1]] = V.pose_coordinates(s["x0"], *s["trial"])
        stat = np.asarray([[s["status"] if np.isfinite(s["x0"]).all() else 3, s["evals"], s["accepted"], 0] for s in mols], np.int32)
        return x, stat, np.asarray([np.nan if s["E"] is None else s["E"] for s in mols], np.float32)


def wall(run, rounds):
    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing taken anywhere else says nothing about these kernels")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "launches": a.launches,
           "settings": [V.MIN_STEP, V.MIN_TOL, V.MIN_EVALS]}
    for name, b in (("ragged_batch", GC.grad_batch()), ("pocket_400_x64", pocket_batch())):
        k = Launches(b, dev)
        r = windows({"vina_score_grad": k.grad, "vina_minimize": k.minimize}, a.launches, a.rounds)
        torch.cuda.synchronize()
        stat = k.more[3].cpu().numpy()
        x_dev, E_dev = k.more[0].cpu().numpy(), k.more[2].cpu().numpy()[:, V.E_FINAL]
        top = int(stat[:, V.S_EVALS].max())
        r.update(molecules=k.B, ligand_atoms=k.N, largest_evals=top, total_evals=int(stat[:, V.S_EVALS].sum()),
                 status_counts=np.bincount(stat[:, V.S_STATUS], minlength=4).tolist(),
                 per_evaluation_us=r["vina_minimize"]["median_us"] / top,
                 per_evaluation_over_grad_launch=r["vina_minimize"]["median_us"] / top / r["vina_score_grad"]["median_us"])
        x_host, stat_host, E_host = k.host_loop()
        r["host_loop_wall"] = wall(k.host_loop, a.rounds)
        r["one_launch_wall"] = wall(k.minimize, a.rounds)
        r["host_loop_over_one_launch"] = r["host_loop_wall"]["median_ms"] / r["one_launch_wall"]["median_ms"]
        r["host_loop_largest_evals"] = int(stat_host[:, V.S_EVALS].max())
        r["host_loop_equals_launch"] = {"stat": bool(np.array_equal(stat_host, stat)),
                                        "x_bits": bool(np.array_equal(x_host.view(np.int32), x_dev.view(np.int32))),
                                        "E_bits": bool(np.array_equal(E_host.view(np.int32), E_dev.view(np.int32)))}
        res[name] = r
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
