"""The training step's buffer layouts are pinned: parameter count, pack buffer, per-call workspace, edge-stage scratch
and weight-gradient scratch, for a fixed set of configurations (CPU only: the size queries are host code, the graph
struct holds fake non-null addresses and nothing is dereferenced)."""
import ctypes as C
import json
import os

import pytest

from diffsbdd_amd import _lib, synthetic
from diffsbdd_amd.engine import make_config
from oracle import weights as W
from tests._golden import GOLDEN_DIR
from tests.test_workspace_layout import ARCHS, _hp

# (n_nodes, n_edges, n_lig, batch): full-atom x 16, C-alpha x 96, and one graph smaller than a tile
SHAPES = [(4944, 91152, 368, 16), (8736, 633600, 2208, 96), (12, 144, 4, 1)]
# read when a handle is created / on first use: the recorded numbers hold with all of them unset
SWITCHES = ["DSBDD_TRAIN_STORE_Z2", "DSBDD_TRAIN_STREAMS", "DSBDD_WGRAD_MINKC", "DSBDD_WGRAD_MAXWG", "DSBDD_TRAIN_WG_PER_CU"]


def sizes(lib, arch):
    """{"params": n, "pack": bytes, "<shape>": [workspace, scratch, wgrad scratch] ...} of one architecture."""
    cfg = W.arch_cfg(arch)[0]
    h = C.c_void_p()
    assert lib.dsbdd_train_net_create(C.byref(make_config(**_hp(cfg))), C.byref(h)) == _lib.OK
    try:
        out = {"params": int(lib.dsbdd_train_net_param_count(h)), "pack": int(lib.dsbdd_train_net_pack_bytes(h))}
        H = cfg["hidden_nf"]
        fake = 4096
        for n_nodes, n_edges, n_lig, batch in SHAPES:
            g = _lib.TrainGraph(erow=fake, ecol=fake, ed0=fake, row_ptr=fake, deg=fake, rev=fake, node_batch=fake,
                                lig_off=fake, poc_off=fake, n_lig=n_lig, n_nodes=n_nodes, n_edges=n_edges, batch=batch)
            out[f"{n_nodes}x{n_edges}x{n_lig}x{batch}"] = [
                int(lib.dsbdd_train_net_workspace_bytes(h, C.byref(g))),
                int(lib.dsbdd_train_scratch_bytes(H, n_nodes, n_edges)),
                int(lib.dsbdd_train_wgrad_scratch_bytes(n_edges, H, H))]
        return out
    finally:
        lib.dsbdd_train_net_destroy(h)


@pytest.mark.parametrize("arch", ARCHS)
def test_training_layout_is_the_recorded_one(arch):
    """Expected numbers: tests/golden/train_layout.json, recorded by running `sizes` above against a library built from
    commit 697f470 (the last one with three hand-written carvers); they are never regenerated from the code under test."""
    if any(s in os.environ for s in SWITCHES):
        pytest.fail("unset " + ", ".join(s for s in SWITCHES if s in os.environ) + ": the layout is recorded without them")
    with open(os.path.join(GOLDEN_DIR, "train_layout.json")) as f:
        want = json.load(f)[arch]
    got = sizes(_lib.load(), arch)
    assert got == want
    # one index per parameter TENSOR: dynamics_param_shapes lists the shared output layer of a block's two coordinate MLPs
    # under both names (cross_product_mlp.4.weight is coord_mlp.4.weight), the C side indexes it once
    cfg = W.arch_cfg(arch)[0]
    names = list(synthetic.dynamics_param_shapes(cfg))
    aliases = [k for k in names if k.endswith("cross_product_mlp.4.weight")]
    assert len(aliases) == (0 if cfg["reflection_equivariant"] else cfg["n_layers"])
    assert got["params"] == len(names) - len(aliases)
    assert all(v > 0 and v % 256 == 0 for k, v3 in got.items() if "x" in k for v in v3)
