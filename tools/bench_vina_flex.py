"""Cost of the one-launch flexible minimiser (dsbdd_vina_flex) per evaluation against the rigid one (dsbdd_vina_minimize), and of
a whole relaxation against the same iteration driven from the host; and how far E falls on the displaced 5ndu fixture with and
without torsions: the figures of profiles/vina_flex.md.

The two batches of tools/bench_vina_minimize.py.  They carry codes and no bond graph, so every molecule is given the graph
of a chain over its atoms in index order (the tree of `vina._vina_torsions_host` on it: up to 32 rotors kept; the 300-atom
molecule is longer than the masks and stays rigid).  Four entries on the same buffers: dsbdd_vina_minimize, dsbdd_vina_flex
with that tree, dsbdd_vina_flex with an empty tree (no rotor, no pair: what the second sweep and the decision split cost
on their own), and dsbdd_vina_flex with that tree and dofs = 1 (the intramolecular pairs are summed, no rotor turns: what
the pairs cost without the rotations).  Device events around windows of `--launches` launches after warm-up, the entries alternating window by
window, median over `--rounds` windows each; per evaluation = that over the largest evaluation count of the batch.

The host-driven loop (written here only, as the baseline) is the iteration of `vina._vina_flex_host` in lockstep over the
batch: per evaluation one dsbdd_vina_score_grad and one dsbdd_vina_intra launch, one read-back of their rows, the decisions
and the next coordinates in numpy (`vina.flex_geometry`, `vina.flex_step`, `vina.torsion_coordinates`), one upload.  Wall
time around whole runs, median over `--rounds` runs after one untimed run; the device launch is timed the same way beside it.

  python tools/bench_vina_flex.py [--rounds 9] [--launches 5] [--out vina_flex.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffsbdd_amd import vina as V  # noqa: E402
from tests import _vina_cases as C  # noqa: E402
from tests import _vina_grad_cases as GC  # noqa: E402
from tests import _vina_min_cases as MC  # noqa: E402
from tools.bench_vina_grad import pocket_batch, windows  # noqa: E402
from tools.bench_vina_minimize import Launches, wall  # noqa: E402


def chain_tree(b):
    """The tree of a chain over every molecule's atoms in index order, typed by the batch's own codes."""
    off = np.asarray(b["mol_off"], np.int64)
    sizes = np.diff(off)
    n_max = int(min(max(sizes.max(), 1), 128))
    order = np.zeros((len(sizes), n_max, n_max), np.int8)
    for m, n in enumerate(sizes):
        k = np.arange(1, min(n, n_max))
        order[m, k, k - 1] = 1
    classes = np.asarray(b["lig_code"], np.int64) & V.CLASS_MASK
    return V._vina_torsions_host(order, classes, off, np.arange(16))


class FlexLaunches(Launches):
    """`Launches` with the flexible entry and the intramolecular one on the same buffers."""

    def __init__(self, b, dev, tree):
        super().__init__(b, dev)
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        N, B = self.N, self.B
        self.tree = [torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (tree.ints, tree.ends, tree.sides, tree.pair_mask)]
        self.none = [torch.zeros_like(self.tree[0]), self.tree[1], self.tree[2], torch.zeros_like(self.tree[3])]
        self.intra_out = [torch.zeros((N, 5), **f32), torch.zeros((B, 8), **f32), torch.zeros(B, **i32), torch.zeros((N, 3), **f32)]
        self.flex_more = [torch.zeros((N, 3), **f32), torch.zeros((B, 8), **f32), torch.zeros((B, 8), **f32), torch.zeros((B, 4), **i32),
                          torch.zeros((B, 32), **f32), torch.zeros((B, 32), **f32)]

    def flex(self, tree=None, dofs=3, step=V.MIN_STEP, tol=V.MIN_TOL, max_evals=V.MIN_EVALS):
        tree = self.tree if tree is None else tree
        assert self.lib.dsbdd_vina_flex(*self.head(self.t["lig_x"]), *(v.data_ptr() for v in tree), dofs, step, tol, max_evals,
                                        *(v.data_ptr() for v in self.five), *(v.data_ptr() for v in self.intra_out),
                                        *(v.data_ptr() for v in self.flex_more)) == 0

    def flex_rigid_tree(self):
        self.flex(self.none)

    def flex_rigid_dofs(self):
        self.flex(dofs=1)

    def intra(self, x):
        t = self.t
        assert self.lib.dsbdd_vina_intra(self.stream, x.data_ptr(), t["lig_code"].data_ptr(), t["mol_off"].data_ptr(), self.B,
                                         self.tree[3].data_ptr(), *(v.data_ptr() for v in self.intra_out)) == 0

    def host_flex(self, tree, step=V.MIN_STEP, tol=V.MIN_TOL, max_evals=V.MIN_EVALS):
        """The flexible iteration in lockstep from the host -> (x float32 [N,3], stat int32 [B,4], E float32 [B])."""
        step, tol, max_evals = V._settings(step, tol, max_evals)
        b, B, off = self.b, self.B, self.b["mol_off"]
        x_in = np.asarray(b["lig_x"], np.float32)
        mols = []
        for m in range(B):
            x0 = x_in[off[m]:off[m + 1]]
            K = V.valid_torsions(tree, m, len(x0))
            mols.append(dict(x0=x0, rotors=K, pose=(np.zeros(3), np.asarray([1.0, 0, 0, 0]), np.zeros(len(K))), trial=None, phase="first",
                             E=None, L=step, u=0.0, geo=None, F=None, M=None, evals=0, accepted=0, rejected=False, status=0,
                             live=bool(np.isfinite(x0).all())))
        x = x_in.copy()
        place = lambda s, pose: V.torsion_coordinates(s["x0"], s["rotors"], pose[2], pose[0], pose[1])
        while any(s["live"] for s in mols):
            self.x.copy_(torch.as_tensor(x, device=self.dev))
            self.grad(self.x)
            self.intra(self.x)
            mol, mg, g = self.five[1].cpu().numpy(), self.five[4].cpu().numpy(), self.five[3].cpu().numpy().astype(np.float64)
            imol, ig = self.intra_out[1].cpu().numpy(), self.intra_out[3].cpu().numpy().astype(np.float64)
            for m, s in enumerate(mols):
                if not s["live"]:
                    continue
                E1 = float(mol[m, V.M_INTER]) + float(imol[m, V.M_INTER])
                s["evals"] += 1
                moved = False
                if s["phase"] == "final":
                    s["live"] = False
                    continue
                if s["phase"] == "first":
                    s["E"], moved = E1, True
                elif E1 < s["E"]:
                    s["pose"], s["E"], moved = s["trial"], E1, True
                    s["L"], s["accepted"], s["rejected"] = min(2 * s["L"], step), s["accepted"] + 1, False
                else:
                    s["L"], s["rejected"] = 0.5 * s["L"], True
                stop = False
                if moved:
                    rows = slice(off[m], off[m + 1])
                    s["F"], s["M"] = mg[m, V.G_NET].astype(np.float64), mg[m, V.G_MOMENT].astype(np.float64)
                    s["geo"] = V.flex_geometry(x[rows], s["rotors"], g[rows] + ig[rows])
                    c, rho2, rho_max, tau, reach, rho2k = s["geo"]
                    s["u"] = V.flex_slope(s["F"], s["M"], rho2, rho_max, tau, reach, rho2k)
                    if not s["u"] > 0:
                        s["status"], stop = 2, True
                if not stop and s["L"] < tol:
                    s["status"], stop = 1, True
                if not stop and s["evals"] >= max_evals:
                    s["status"], stop = 0, True
                if stop:
                    x[off[m]:off[m + 1]] = place(s, s["pose"])
                    s["phase"], s["live"] = "final", s["rejected"]
                    continue
                c, rho2, rho_max, tau, reach, rho2k = s["geo"]
                s["trial"] = V.flex_step(*s["pose"], s["F"], s["M"], tau, c, rho2, rho2k, s["L"] / s["u"])
                s["phase"] = "trial"
                x[off[m]:off[m + 1]] = place(s, s["trial"])
        stat = np.asarray([[s["status"] if np.isfinite(s["x0"]).all() else 3, s["evals"], s["accepted"], 0] for s in mols], np.int32)
        return x, stat, np.asarray([np.nan if s["E"] is None else s["E"] for s in mols], np.float32)


def fixture_fall(dev):
    """The displaced 5ndu ligand of the fixture through the front end, default settings: rigid, and with torsions."""
    from tests.test_gpu_vina_grad import _crystal
    z = C.fixture()
    x, at, mask, pockets, decoder, orders = _crystal(z, "5ndu")
    xm = torch.as_tensor(MC.rigid_motion(z["5ndu_crystal_x"]), device=dev)
    rigid = V.vina_minimize(xm, at, mask, pockets, decoder, orders=orders)
    flex = V.vina_minimize(xm, at, mask, pockets, decoder, orders=orders, torsions=True)
    crystal = V.vina_score(x, at, mask, pockets, decoder, orders=orders)
    return {"inter_crystal": float(crystal.inter[0]),
            "rigid": {"inter_start": float(rigid.inter_start[0]), "inter": float(rigid.inter[0]), "evals": int(rigid.evals[0]),
                      "status": V.STATUS[int(rigid.status[0])], "rmsd": float(rigid.rmsd[0])},
            "torsions": {"inter_start": float(flex.inter_start[0]), "inter": float(flex.inter[0]), "intra_start": float(flex.intra_start[0]),
                         "intra": float(flex.intra[0]), "E_start": float(flex.energies[0, V.X_E_START]),
                         "E": float(flex.energies[0, V.X_E_FINAL]), "evals": int(flex.evals[0]), "status": V.STATUS[int(flex.status[0])],
                         "rmsd": float(flex.rmsd[0]), "largest_theta_deg": float(np.rad2deg(flex.theta.abs().max().item()))}}


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
        tree = chain_tree(b)
        k = FlexLaunches(b, dev, tree)
        r = windows({"vina_minimize": k.minimize, "vina_flex": k.flex, "vina_flex_no_rotors": k.flex_rigid_tree,
                     "vina_flex_dofs_1": k.flex_rigid_dofs}, a.launches, a.rounds)
        k.minimize()
        torch.cuda.synchronize()
        evals_rigid = int(k.more[3].cpu().numpy()[:, V.S_EVALS].max())
        k.flex_rigid_tree()
        torch.cuda.synchronize()
        evals_none = int(k.flex_more[3].cpu().numpy()[:, V.S_EVALS].max())
        k.flex_rigid_dofs()
        torch.cuda.synchronize()
        evals_dofs1 = int(k.flex_more[3].cpu().numpy()[:, V.S_EVALS].max())
        k.flex()
        torch.cuda.synchronize()
        stat = k.flex_more[3].cpu().numpy()
        x_dev, E_dev = k.flex_more[0].cpu().numpy(), k.flex_more[2].cpu().numpy()[:, V.X_E_FINAL]
        top = int(stat[:, V.S_EVALS].max())
        per = {"vina_minimize": r["vina_minimize"]["median_us"] / evals_rigid, "vina_flex": r["vina_flex"]["median_us"] / top,
               "vina_flex_no_rotors": r["vina_flex_no_rotors"]["median_us"] / evals_none,
               "vina_flex_dofs_1": r["vina_flex_dofs_1"]["median_us"] / evals_dofs1}
        r.update(molecules=k.B, ligand_atoms=k.N, rotors_kept=int(tree.kept.sum()), largest_rotors=int(tree.kept.max()),
                 intra_pairs=int(V.unpack_masks(tree.pair_mask, 128).sum() // 2),
                 largest_evals={"vina_minimize": evals_rigid, "vina_flex": top, "vina_flex_no_rotors": evals_none,
                                "vina_flex_dofs_1": evals_dofs1},
                 status_counts=np.bincount(stat[:, V.S_STATUS], minlength=4).tolist(), per_evaluation_us=per,
                 flex_over_rigid_per_evaluation=per["vina_flex"] / per["vina_minimize"],
                 no_rotors_over_rigid_per_evaluation=per["vina_flex_no_rotors"] / per["vina_minimize"],
                 dofs_1_over_rigid_per_evaluation=per["vina_flex_dofs_1"] / per["vina_minimize"])
        x_host, stat_host, E_host = k.host_flex(tree)
        r["host_loop_wall"] = wall(lambda: k.host_flex(tree), max(a.rounds // 3, 1))
        r["one_launch_wall"] = wall(k.flex, a.rounds)
        r["host_loop_over_one_launch"] = r["host_loop_wall"]["median_ms"] / r["one_launch_wall"]["median_ms"]
        r["host_loop_largest_evals"] = int(stat_host[:, V.S_EVALS].max())
        r["host_loop_equals_launch"] = {"stat": bool(np.array_equal(stat_host, stat)),
                                        "x_bits": bool(np.array_equal(x_host.view(np.int32), x_dev.view(np.int32))),
                                        "E_bits": bool(np.array_equal(E_host.view(np.int32), E_dev.view(np.int32)))}
        res[name] = r
    res["fixture_5ndu_displaced"] = fixture_fall(dev)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
