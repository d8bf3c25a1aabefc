"""Cost and observed error of the Vina-type score (`vina.vina_score`: dsbdd_vina_type + dsbdd_vina_score), the figures of
profiles/vina_score.md and profiles/vina_score_error.md.

Cost: 64 molecules of 20-30 atoms on the packaged 3rfm pocket (286 heavy atoms, typed by element: the package stores no
atom names), scattered (sigma 2.5 A) around the crystal ligand's place.  Device events around the two launches alone (bond
orders, inputs and outputs prepared before), warm-up, median of `--reps`; `dsbdd_pose_check` on the same atoms in the same
process for comparison; the Python entry (bond orders and allocations included) by a host clock around a synchronised call.
Error: |kernel - float64 restatement| as a fraction of `vina.error_bound`, per term, on the ragged batch of the tests and on
the crystal fixture.

  python tools/bench_vina.py [--reps 30] [--out vina_score.json]
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
from diffsbdd_amd import _lib, pose, vina  # noqa: E402
from diffsbdd_amd.chem_tables import dataset_info  # noqa: E402
from diffsbdd_amd.molecules import bond_orders  # noqa: E402
from diffsbdd_amd.pocket import ATOM_ENCODER  # noqa: E402


def events(launch, reps):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def cost(reps, dev, n_mols=64, seed=0):
    rng = np.random.RandomState(seed)
    info = dataset_info("crossdock")
    z = np.load(os.path.join(ROOT, "diffsbdd_amd", "data", "pocket_3rfm.npz"))
    decoder = {v: k for k, v in ATOM_ENCODER.items()}
    elements = [decoder[int(t)] for t in z["fa_types"]]
    poc_x = z["fa_x"].astype(np.float32)
    pockets = vina.VinaPocket.upload([(poc_x, np.asarray([vina.code_by_element(e) for e in elements], np.int32))], dev)
    pose_pockets = pose.PocketAtoms.upload([(poc_x, pose.radii_of(elements))], dev)
    sizes = rng.randint(20, 31, n_mols)
    x = (z["ligand_x"].mean(0) + rng.normal(0, 2.5, (int(sizes.sum()), 3))).astype(np.float32)
    types = rng.choice([0, 0, 0, 1, 2], len(x))                               # C, N, O of the crossdock decoder
    mask = np.repeat(np.arange(n_mols), sizes).astype(np.int64)
    xd, td, md = (torch.as_tensor(v, device=dev) for v in (x, types, mask))
    st = vina.vina_score(xd, td, md, pockets, info, batch=n_mols)
    orders, _ = bond_orders(xd, td, md, info, batch=n_mols)
    torch.cuda.synchronize()
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    t32 = td.to(torch.int32)
    table = torch.as_tensor(vina.class_table(info["atom_decoder"]), device=dev)
    groups = torch.zeros(n_mols, dtype=torch.int32, device=dev)
    code, mol_int = torch.zeros_like(st.lig_code), torch.zeros_like(st.mol_int)
    atom, mol, flag = torch.zeros_like(st.atom), torch.zeros_like(st.mol), torch.zeros_like(st.flag)

    def type_launch():
        assert lib.dsbdd_vina_type(stream, orders.data_ptr(), t32.data_ptr(), st.mol_off.data_ptr(), n_mols, len(table),
                                   table.data_ptr(), int(orders.shape[1]), code.data_ptr(), mol_int.data_ptr()) == 0

    def score_launch():
        assert lib.dsbdd_vina_score(stream, xd.data_ptr(), code.data_ptr(), st.mol_off.data_ptr(), n_mols, groups.data_ptr(),
                                    mol_int.data_ptr(), pockets.x.data_ptr(), pockets.code.data_ptr(),
                                    pockets.group_off.data_ptr(), 1, atom.data_ptr(), mol.data_ptr(), flag.data_ptr()) == 0

    def both():
        type_launch()
        score_launch()

    radii = torch.as_tensor(pose.radius_table(info["atom_decoder"]), device=dev)[td]
    ps = pose.pose_check(xd, radii, md, pose_pockets, batch=n_mols)

    def pose_launch():
        assert lib.dsbdd_pose_check(stream, xd.data_ptr(), radii.data_ptr(), ps.mol_off.data_ptr(), n_mols, groups.data_ptr(),
                                    pose_pockets.x.data_ptr(), pose_pockets.r.data_ptr(), pose_pockets.group_off.data_ptr(), 1,
                                    pose.CLASH_TOLERANCE, pose.CONTACT_CUTOFF, ps.atom.data_ptr(), ps.mol.data_ptr()) == 0

    out = {"molecules": n_mols, "ligand_atoms": int(len(x)), "pocket_atoms": int(len(poc_x)), "pairs": int(len(x) * len(poc_x)),
           "n_max": int(orders.shape[1]), "reps": reps, "vina_type": events(type_launch, reps),
           "vina_score": events(score_launch, reps), "both_launches": events(both, reps), "pose_check": events(pose_launch, reps)}
    same = torch.equal(atom, st.atom) and torch.equal(mol, st.mol) and torch.equal(code, st.lig_code)
    call_ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        vina.vina_score(xd, td, md, pockets, info, batch=n_mols)
        torch.cuda.synchronize()
        call_ms.append((time.perf_counter() - t0) * 1e3)
    out.update(bitwise_equal_to_the_entry=bool(same), call_ms_median=statistics.median(call_ms), call_ms_min=min(call_ms),
               mean_score=float(st.score.mean()))
    return out


def _fractions(got_atom, got_mol, want, atom_bound, mol_bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        fa = np.abs(got_atom.astype(np.float64) - want.atom) / atom_bound
        fm = np.abs(got_mol[:, :7].astype(np.float64) - want.mol[:, :7]) / mol_bound
    fa, fm = np.where(np.isfinite(fa), fa, 0.0), np.where(np.isfinite(fm), fm, 0.0)
    return {"atom_terms": fa.max(0).tolist(), "mol_terms_inter_score": fm.max(0).tolist()}


def errors(dev):
    from tests import _vina_cases as C
    out = {}
    b = C.score_batch()
    want, margin, atom_bound, mol_bound = C.score_reference()
    t = {k: torch.as_tensor(np.ascontiguousarray(b[k]), device=dev) for k in C.SCORE_KEYS}
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def run(t, N, B, G):
        atom = torch.zeros((N, 5), device=dev)
        mol, flag = torch.zeros((B, 8), device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        assert lib.dsbdd_vina_score(stream, *(t[k].data_ptr() for k in C.SCORE_KEYS[:3]), B, t["mol_group"].data_ptr(),
                                    t["mol_int"].data_ptr(), t["poc_x"].data_ptr(), t["poc_code"].data_ptr(),
                                    t["group_off"].data_ptr(), G, atom.data_ptr(), mol.data_ptr(), flag.data_ptr()) == 0
        torch.cuda.synchronize()
        return atom.cpu().numpy(), mol.cpu().numpy()

    atom, mol = run(t, len(b["lig_x"]), 16, 6)
    out["ragged_batch"] = dict(_fractions(atom, mol, want, atom_bound, mol_bound), margin=margin)
    st32, _ = vina._vina_score_host(*(b[k] for k in C.SCORE_KEYS), dtype=np.float32)
    out["ragged_batch_float32_restatement"] = _fractions(st32.atom, st32.mol, want, atom_bound, mol_bound)
    z = C.fixture()
    for name in z["names"]:
        n = len(z[f"{name}_lig_code"])
        for variant in ("crystal", "shifted"):
            sb = {"lig_x": z[f"{name}_{variant}_x"], "lig_code": z[f"{name}_lig_code"], "mol_off": np.asarray([0, n], np.int32),
                  "mol_group": np.zeros(1, np.int32), "mol_int": np.asarray([[n, 0, int(z[f"{name}_n_rot"]), 0]], np.int32),
                  "poc_x": z[f"{name}_poc_x"], "poc_code": z[f"{name}_poc_code"],
                  "group_off": np.asarray([0, len(z[f"{name}_poc_x"])], np.int32)}
            want, margin, atom_bound, mol_bound = vina._vina_score_host(*(sb[k] for k in C.SCORE_KEYS), eps=vina.EPS32)
            t = {k: torch.as_tensor(np.ascontiguousarray(sb[k]), device=dev) for k in C.SCORE_KEYS}
            atom, mol = run(t, n, 1, 1)
            out[f"{name}_{variant}"] = dict(_fractions(atom, mol, want, atom_bound, mol_bound), margin=margin,
                                            score=float(mol[0, 6]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing taken anywhere else says nothing about these kernels")
    dev = torch.device("cuda:0")
    res = {"cost": cost(a.reps, dev), "error_over_bound": errors(dev)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
