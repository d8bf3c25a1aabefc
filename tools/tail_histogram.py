#!/usr/bin/env python
"""Item counts of the message-stage launches over one benchmark chain (anchored headline chain, B = 64, T = 500).

After every EGNN call the level ends (BUF_LEVEL_END) and the shell-list counts are read back (one sync per call: this
is a counting run, not a timing run), and the number of 128-edge workgroup items of the stages 1..5 is formed from
the call's plan the way forward.h sets their ranges.  Block 0's two-list launch is not counted (its lists have no
read-out); its size does not depend on the ligand's position.  Prints a markdown table per stage: items, R = items mod S
(S = 512 resident workgroups), the histogram of R / S in eighths, and how many launches the split rule of edge_wave.h
touches (R <= S/4, or S/2 < R <= 3S/4).

    python tools/tail_histogram.py [timesteps] > profiles/<tag>_items.md
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from diffsbdd_amd import _lib  # noqa: E402
from diffsbdd_amd.engine import HipEngine  # noqa: E402

S = 512


def main():
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 500
    device = torch.device("cuda", 0)
    arch, key, B = bench.WORKLOADS["crossdock_fullatom_cond"]
    cfg, dd, model = bench.build_model(arch, device)
    pocket0 = bench.load_pocket(key, B, device)
    anchor = bench.anchor_ligand(B, 23, cfg["atom_nf"], device)
    eng = model.dynamics.engine()
    log = []
    inner = HipEngine.forward_async

    def counted(self, *a, **k):
        out = inner(self, *a, **k)
        torch.cuda.synchronize(self.device)
        end = self._read(self.buffer_ptr(_lib.BUF_LEVEL_END), 10, np.int32).astype(np.int64)
        cnt = np.zeros(2, dtype=np.int32)
        self.lib.dsbdd_engine_shell_read(self.handle, ctypes.c_int(1), ctypes.c_int(0), ctypes.c_void_p(cnt.ctypes.data),
                                         ctypes.c_int64(2))
        radius, ghost, _ = self.last_plan()
        shell = self.get_option(_lib.OPT_SHELL)
        tiles = lambda n: (int(n) + 127) // 128
        items = []
        for g in range(1, len(radius)):
            r = radius[g]
            if ghost[g] and shell and g in (1, 2):
                items.append(tiles(end[r - 1]) + tiles(cnt[g - 1]))
            else:
                items.append(tiles(end[r] if ghost[g] else end[5 + r]))
        log.append(items)
        return out

    HipEngine.forward_async = counted
    model.seed(200, sample_offset=0)
    model.inpaint({k: v.clone() for k, v in anchor.items()}, {k: v.clone() for k, v in pocket0.items()},
                  torch.ones(B * 23, device=device), resamplings=1, timesteps=T)
    HipEngine.forward_async = inner
    a = np.array(log)
    print(f"{len(a)} calls, plan {eng.last_plan()[:2]}, S = {S}\n")
    print("| stage | items min / mean / max | R / S in eighths (launches per bin 0..7) | R <= S/4 | S/2 < R <= 3S/4 | not split |")
    print("|---|---|---|---|---|---|")
    tot = np.zeros(3, dtype=np.int64)
    for g in range(a.shape[1]):
        it = a[:, g]
        R = it % S
        hist = np.bincount(R * 8 // S, minlength=8)
        lo, mid = int((4 * R <= S).sum()), int(((2 * R > S) & (4 * R <= 3 * S)).sum())
        tot += (lo, mid, len(it) - lo - mid)
        print(f"| {g + 1} | {it.min()} / {it.mean():.1f} / {it.max()} | {' '.join(map(str, hist))} | {lo} | {mid} | {len(it) - lo - mid} |")
    print(f"| all | | | {tot[0]} | {tot[1]} | {tot[2]} |")


if __name__ == "__main__":
    main()
