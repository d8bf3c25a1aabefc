#!/usr/bin/env python
"""Bit identity of the graph and geometry kernels between two builds of the library (profiles/graph_parts.md).

    DSBDD_LIB=build_ab/libparent.so python tools/graph_parts_ab.py dump build_ab/parent.npz
    python tools/graph_parts_ab.py dump build_ab/change.npz
    python tools/graph_parts_ab.py compare build_ab/parent.npz build_ab/change.npz

`dump` runs, in this process and under whatever library DSBDD_LIB selects, the calls that reach every kernel of
csrc/radius_graph.h, level_list.h and geometry.h at the tests' own small shapes, and stores every array they return or
leave behind.  `compare` needs every array of both files equal (np.array_equal) and none all zero."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dump(path):
    import torch
    from oracle import weights as W
    from tests import test_gpu_cone_shell as cs
    from tests import test_gpu_train as tr
    from tests._golden import Case
    from tests.test_gpu_parity import _random_problem, dev, make_ddpm, make_dynamics

    out = {}

    def put(name, v):
        out[name] = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)

    # the ragged problem of test_folded_scans_are_bitwise_the_scan_kernels, with and without the folded scans
    cfg, _ = W.arch_cfg("small_cond")
    sd = W.random_state_dict(cfg, 4)
    xl, xp, t, ml, mp = _random_problem(cfg, [23, 0, 9, 40, 1], [36, 50, 0, 20, 44], seed=17)
    N = len(ml) + len(mp)
    for fold in ("1", "0"):
        os.environ["DSBDD_FOLD_SCAN"] = fold
        m = make_dynamics(cfg, sd)
        f_l, f_p = m(*[v.to(dev()) for v in (xl, xp, t, ml, mp)])
        er, ec = m.engine().last_edges(N)
        for k, v in (("eps_lig", f_l), ("eps_pocket", f_p), ("row", er), ("col", ec), ("slots", m.engine().edge_slots(N))):
            put(f"ragged/fold{fold}/all/{k}", v)
        e_l, _, st = m.forward_async(xl, xp, torch.full((1,), 0.4), ml, mp, want_pocket=False, batch=5)
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        put(f"ragged/fold{fold}/lig/eps_lig", e_l)
        for k, v in m.engine().last_levels(N).items():
            if not k.startswith("ghost_"):                       # (no frame: no ghost rows, both counts are 0)
                put(f"ragged/fold{fold}/lig/{k}", v)
    os.environ.pop("DSBDD_FOLD_SCAN")

    # the public builder (compact list) on the same problem
    m = make_dynamics(cfg, sd)
    eng = m.engine()
    from diffsbdd_amd import _lib
    from diffsbdd_amd.engine import edge_capacity
    d = dev()
    mld, mpd = ml.to(d), mp.to(d)
    x = torch.cat((xl[:, :3], xp[:, :3]), 0).to(d).contiguous()
    cap = max(edge_capacity(mld, mpd, 5), 1)
    i32 = dict(dtype=torch.int32, device=d)
    bufs = {"node_batch": torch.zeros(N, **i32), "lig_off": torch.zeros(6, **i32), "poc_off": torch.zeros(6, **i32),
            "deg": torch.zeros(N, **i32), "row_ptr": torch.zeros(N + 1, **i32), "row": torch.zeros(cap, **i32),
            "col": torch.zeros(cap, **i32), "d0": torch.zeros(cap, dtype=torch.float32, device=d)}
    status = torch.zeros(1, **i32)
    _lib.check(eng.lib.dsbdd_build_edges(torch.cuda.current_stream(d).cuda_stream, x.data_ptr(), mld.data_ptr(),
                                         mpd.data_ptr(), len(ml), len(mp), 5, eng.cfg,
                                         *[bufs[k].data_ptr() for k in ("node_batch", "lig_off", "poc_off", "deg", "row_ptr",
                                                                        "row", "col", "d0")],
                                         cap, status.data_ptr()), "dsbdd_build_edges")
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    E = int(bufs["row_ptr"][-1].item())
    for k, v in bufs.items():
        put(f"build_edges/{k}", v[:E] if k in ("row", "col", "d0") else v)

    # frame + cone, shell on and off: the problems of tests/test_gpu_cone_shell.py
    for kind in ("ragged", "shapes"):
        for shell in (True, False):
            r = cs.run(cs.select(kind, [0, 1, 2, 3]), shell, want_lists=shell)
            tag = f"cone/{kind}/shell{int(shell)}"
            put(tag + "/eps", r["eps"]); put(tag + "/edges", r["edges"]); put(tag + "/level", r["level"]); put(tag + "/h", r["h"])
            put(tag + "/plan", np.array(r["plan"][0] + r["plan"][1] + [r["plan"][2]]))
            if shell:
                sh = r["shell"]
                for k in ("stats", "slots", "ptr", "deg"):
                    put(f"{tag}/sh_{k}", sh[k])
                for s in range(2):
                    put(f"{tag}/sh_row{s}", sh["row"][s]); put(f"{tag}/sh_col{s}", sh["col"][s])

    # teacher-forced edges
    c = Case("dyn_small_cond")
    m = make_dynamics(c.cfg, c.state_dict())
    n = len(c.t("mask_lig")) + len(c.t("mask_pocket"))
    th, tx = m.engine().set_trace(n)
    e_l, e_p, st = m.forward_async(c.t("xh_lig"), c.t("xh_pocket"), c.t("t"), c.t("mask_lig"), c.t("mask_pocket"),
                                   edges=c.t("edges", torch.int64))
    torch.cuda.synchronize()
    m.engine().clear_trace()
    assert int(st.item()) == 0
    for k, v in (("eps_lig", e_l), ("eps_pocket", e_p), ("trace_h", th), ("trace_x", tx)):
        put(f"teacher_forced/{k}", v)

    # joint model (every coordinate updated, mean removed) and the one-coordinate-MLP variant
    for arch in ("small_joint", "small_variant"):
        acfg, _ = W.arch_cfg(arch)
        m = make_dynamics(acfg, W.random_state_dict(acfg, 4))
        a = _random_problem(acfg, [23, 0, 9, 40, 1], [36, 50, 0, 20, 44], seed=17)
        f_l, f_p = m(*[v.to(dev()) for v in a])
        put(f"{arch}/eps_lig", f_l); put(f"{arch}/eps_pocket", f_p)

    # one training step at the smallest configuration of tests/test_gpu_train.py: loss and every gradient
    for arch in ("small_cond", "small_joint", "small_variant"):
        acfg, _ = W.arch_cfg(arch)
        m = tr.make_dynamics(acfg, W.random_state_dict(acfg, seed=1))
        m.train(True)
        a = tr.problem(acfg, [5, 7, 6], [40, 35, 38], 21)
        gen = torch.Generator().manual_seed(99)
        wl, wp = torch.randn(a[0].shape, generator=gen), torch.randn(a[1].shape, generator=gen)
        o_l, o_p = m(*[v.to(dev()) for v in a])
        loss = (o_l * wl.to(dev())).sum() + (o_p * wp.to(dev())).sum()
        loss.backward()
        put(f"train/{arch}/loss", loss); put(f"train/{arch}/out_lig", o_l); put(f"train/{arch}/out_pocket", o_p)
        for pname, p in m.named_parameters():
            if p.grad is not None:
                put(f"train/{arch}/grad/{pname}", p.grad)

    # a keyed sampling chain of five steps with a frame
    c = Case("ddpm_small_cond")
    model = make_ddpm(c)
    model.frame_min_pocket_nodes = 1
    model.seed(3)
    chain = model.sample_given_pocket(c.pocket(), c.t("num_nodes_lig"), timesteps=5)
    torch.cuda.synchronize()
    for k, v in zip(("ligand", "pocket", "ligand_mask", "pocket_mask"), chain):
        put(f"chain/{k}", v)

    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path} (library: {os.environ.get('DSBDD_LIB') or 'of the tree'})")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), sorted(set(a.files) ^ set(b.files))
    differ = [k for k in a.files if not np.array_equal(a[k], b[k])]
    zero = [k for k in a.files if a[k].size and not np.any(a[k])]
    print(f"{len(a.files)} arrays compared, {len(differ)} differ, {len(zero)} all zero")
    for k in differ:
        print("  differs:", k)
    for k in zero:
        print("  all zero:", k)
    return 1 if differ or zero else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
