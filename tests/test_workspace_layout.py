"""The engine's workspace layout is pinned: total size and the offset of every buffer reachable through
dsbdd_engine_buffer, for a fixed set of configurations (CPU only: the library loads without a GPU, the base address is
a fake 256-aligned one and nothing is dereferenced)."""
import ctypes
import json
import os

import pytest

from diffsbdd_amd import _lib
from diffsbdd_amd.engine import make_config
from oracle import weights as W
from tests._golden import GOLDEN_DIR

BASE = 1 << 20          # fake 256-aligned workspace address
N_BUFFERS = 17          # DSBDD_BUF_EDGE_ROW .. DSBDD_BUF_LEVEL_STATS

# (n_lig, n_pocket, batch, edge capacity): the benchmark shapes (full-atom x 64, C-alpha x 32) and two small ones
SHAPES = [(1472, 18304, 64, 6_200_000), (736, 2176, 32, 400_000), (23, 286, 1, 20_000), (4, 8, 1, 144)]
# the three benchmark architectures (hidden_nf 256, 256, 192), the small one (64) and the E(3) variant
# (reflection_equivariant, two invariant sub-layers, hidden_nf 128)
ARCHS = ["crossdock_fullatom_cond", "crossdock_ca_cond", "moad_fullatom_joint", "small_cond", "small_variant"]


def _hp(cfg):
    return dict(atom_nf=cfg["atom_nf"], residue_nf=cfg["residue_nf"], joint_nf=cfg["joint_nf"],
                hidden_nf=cfg["hidden_nf"], n_layers=cfg["n_layers"], inv_sublayers=cfg["inv_sublayers"],
                attention=cfg["attention"], tanh=cfg["tanh"], update_pocket_coords=cfg["update_pocket_coords"],
                reflection_equivariant=cfg["reflection_equivariant"], edge_embedding_dim=cfg["edge_embedding_dim"],
                edge_cutoff_ligand=cfg["edge_cutoff_ligand"], edge_cutoff_pocket=cfg["edge_cutoff_pocket"],
                edge_cutoff_interaction=cfg["edge_cutoff_interaction"],
                normalization_factor=cfg["normalization_factor"], norm_constant=cfg["norm_constant"])


def layout(lib, arch, shape):
    """[total bytes, offset of buffer 0, ..., offset of buffer 16] of one configuration."""
    cfg = make_config(**_hp(W.arch_cfg(arch)[0]))
    h = ctypes.c_void_p()
    assert lib.dsbdd_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        total = lib.dsbdd_engine_workspace_bytes(h, *shape)
        assert total > 0
        assert lib.dsbdd_engine_bind_workspace(h, ctypes.c_void_p(BASE), total, *shape) == 0
        out = [int(total)]
        for which in range(N_BUFFERS):
            p = ctypes.c_void_p()
            assert lib.dsbdd_engine_buffer(h, which, ctypes.byref(p)) == 0
            out.append(int(p.value) - BASE)
        assert lib.dsbdd_engine_buffer(h, N_BUFFERS, ctypes.byref(ctypes.c_void_p())) == _lib.ERR_ARG
        return out
    finally:
        lib.dsbdd_engine_destroy(h)


@pytest.mark.parametrize("arch", ARCHS)
def test_workspace_layout_is_the_recorded_one(arch):
    """Expected numbers: tests/golden/workspace_layout.json, recorded by running `layout` above against a library built
    from commit 0fabb57 (the last one whose workspace was laid out by the numbered size table); they are never
    regenerated from the code under test."""
    with open(os.path.join(GOLDEN_DIR, "workspace_layout.json")) as f:
        want = json.load(f)
    lib = _lib.load()
    for shape in SHAPES:
        got = layout(lib, arch, shape)
        key = f"{arch}/{'x'.join(map(str, shape))}"
        assert len(want[key]) == 1 + N_BUFFERS
        assert got == want[key], key
        assert all(o % 256 == 0 and 0 <= o < got[0] for o in got[1:]), key
