"""GPU: the training pass of `EGNNDynamics` on ragged and degenerate batches against a float64 evaluation.

Both HIP paths -- the network walk (`EGNNTrainFunction`, csrc/train_net.h; the default) and the per-stage Functions
(`DSBDD_TRAIN=functions`, train_hip.py over csrc/train.h) -- run one forward and one backward on the cases of
tests/_train64.py that the graph builder accepts (`_train64.GPU_PAIRS`): a sample without ligand atoms, a one-atom ligand,
a sample without pocket atoms, a sample id without any node, a ligand out of reach of its pocket, a two-node graph of
self loops, one shared t.  (A batch with no ligand or no pocket atom at all is refused by dsbdd_build_edges; its cases
are kept in `_train64.CASES` with their CPU checks.)  Outputs, both input gradients and every parameter gradient are
held to `_train64.within_case` against the float64 oracle on the exact CPU edge list: max(2 err_ref, 4 ulp) of the
quantity's largest float64 magnitude, 1e-4 at most, err_ref = the float32 oracle's own error (or the median of it over the
case).  tests/test_train_reference.py checks on the CPU what this relies on.  The figures printed here on one MI355X are in
profiles/train_net_error.md.
"""
import contextlib
import copy
import functools
import os

import pytest
import torch

from oracle import weights as W
from tests import _train64 as T
from tests._steps64 import ULP4

pytestmark = pytest.mark.gpu

PATHS = ("net", "functions")
F64, F32 = torch.float64, torch.float32


def dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def path_env(path):
    return env(DSBDD_TRAIN=None if path == "net" else path)


def fresh_module(arch):
    """A new module: a new per-module handle, created under the environment of the moment."""
    from diffsbdd_amd.dynamics import EGNNDynamics
    cfg, _ = W.arch_cfg(arch)
    m = EGNNDynamics(**cfg, device=dev())
    m.load_state_dict(copy.deepcopy(W.random_state_dict(cfg, seed=1)))
    m.train(True)
    return m


@functools.lru_cache(maxsize=None)
def graph_module(arch):
    return fresh_module(arch)          # (read only: the graph builder takes the cutoffs from it)


def forward_backward(m, case, arch, loss_on=("l", "p"), input_grads=True):
    """One forward and one backward on the case's inputs -> ({quantity: CPU tensor or None}, status or None)."""
    p = T.inputs(case, arch)
    m.zero_grad(set_to_none=True)
    xl = p["xl"].to(dev()).clone().requires_grad_(input_grads)
    xp = p["xp"].to(dev()).clone().requires_grad_(input_grads)
    o_l, o_p = m(xl, xp, p["t"].to(dev()), p["ml"].to(dev()), p["mp"].to(dev()))
    assert o_l.requires_grad and o_p.requires_grad
    status = getattr(o_l.grad_fn, "status", None)
    loss = 0
    if "l" in loss_on:
        loss = loss + (o_l * p["wl"].to(dev())).sum()
    if "p" in loss_on:
        loss = loss + (o_p * p["wp"].to(dev())).sum()
    loss.backward()
    out = dict(eps_l=o_l.detach().cpu(), eps_p=o_p.detach().cpu())
    if input_grads:           # (an input without rows may come back without a gradient tensor: there is nothing to hold)
        for k, v in (("d_xh_atoms", xl), ("d_xh_residues", xp)):
            assert v.grad is not None or v.numel() == 0, k
            out[k] = torch.zeros(v.shape) if v.grad is None else v.grad.cpu()
    for n, q in m.named_parameters():
        out[n] = None if q.grad is None else q.grad.detach().cpu().clone()
    return out, None if status is None else int(status.item())


def check_against_float64(got, case, arch, label, loss_on=("l", "p"), absent=()):
    """Every quantity of `got` through `within_case`; the zeros as the module docstring of the profile says."""
    r64, r32 = T.reference(case, arch, F64, loss_on), T.reference(case, arch, F32, loss_on)
    _, floor = T.err_refs(case, arch, loss_on)
    assert set(got) == set(r64), set(got) ^ set(r64)
    figures = {}
    for k, ref in r64.items():
        if k.startswith(absent):
            assert got[k] is None, (label, k)
            continue
        assert got[k] is not None, (label, k)
        assert got[k].shape == ref.shape, (label, k, got[k].shape, ref.shape)
        assert torch.isfinite(got[k]).all(), (label, k)
        if ref.numel() == 0:
            continue
        if T.magnitude(ref) == 0.0:
            nz = T.magnitude(got[k])
            if case == "single":       # zero by value (x_i - x_i), not by a skipped launch: exact, or noise of the live quantity
                live = T.magnitude(T.reference("ragged", arch, F64)[k])
                print(f"  {label} {k}: float64 is 0, hip max {nz:.3e} (4 ulp of its magnitude in ragged: {ULP4 * live:.3e})")
                assert nz <= ULP4 * live, (label, k, nz)
            else:
                assert k in T.structural_zeros(case, arch), (label, k)
                assert nz == 0.0, (label, k, nz)
            continue
        figures[k] = T.within_case(k, got[k], ref, r32[k], floor, label)
    return figures


@pytest.mark.parametrize("case,arch", T.GPU_PAIRS)
def test_graph_is_the_cpu_list(case, arch):
    """`TrainGraph` (dsbdd_build_edges in the compact layout + dsbdd_train_edge_rev) on degenerate masks: the edge list is
    the exact CPU list element for element, e_lig its ligand-row prefix, every edge has its reverse."""
    from diffsbdd_amd.train_hip import TrainGraph
    p = T.inputs(case, arch)
    x = torch.cat((p["xl"][:, :3], p["xp"][:, :3]), 0).to(dev()).contiguous()
    t = p["t"]
    g = TrainGraph(graph_module(arch), p["ml"].to(dev()), p["mp"].to(dev()), x, batch=int(t.numel()) if t.numel() > 1 else None)
    want = T.exact_edges(case, arch)
    assert g.E == want.shape[1] and g.N == len(p["ml"]) + len(p["mp"]) and g.n_lig == len(p["ml"])
    assert torch.equal(g.edges().cpu(), want)
    assert g.e_lig == int((want[0] < len(p["ml"])).sum())
    rev = g.rev[:g.E].cpu().long()
    assert int((rev < 0).sum()) == 0
    assert torch.equal(want[0][rev], want[1]) and torch.equal(want[1][rev], want[0])
    d0 = ((x[want[0].to(dev())] - x[want[1].to(dev())]).double() ** 2).sum(1)
    assert (g.ed0[:g.E].double() - d0).abs().max().item() <= 1e-6 * max(d0.max().item(), 1.0)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case,arch", T.GPU_PAIRS)
def test_forward_backward_vs_float64(case, arch, path):
    label = f"{path}/{arch}/{case}"
    with path_env(path):
        got, status = forward_backward(fresh_module(arch), case, arch)
    if path == "net":
        assert status == 0, status            # (the per-stage path has no status word: its outputs are checked finite)
    check_against_float64(got, case, arch, label)


@pytest.mark.parametrize("path", PATHS)
def test_unused_output_leaves_no_gradient(path):
    """The pocket-conditioned loss ignores eps_pocket: residue_decoder.* keeps no gradient at all (autograd's None, not
    zeros), everything else meets the bound of the loss on eps_l alone."""
    case, arch = "ragged", "small_cond"
    with path_env(path):
        got, _ = forward_backward(fresh_module(arch), case, arch, loss_on=("l",))
    n_absent = sum(1 for k in got if k.startswith("residue_decoder."))
    assert n_absent == 4
    check_against_float64(got, case, arch, f"{path}/{arch}/{case}/eps_l-only", loss_on=("l",), absent=("residue_decoder.",))


def same_bits(a, b, where):
    assert set(a) == set(b)
    for k in a:
        assert (a[k] is None) == (b[k] is None), (where, k)
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), (where, k, (a[k] - b[k]).abs().max().item() if a[k].numel() else 0.0)


@pytest.mark.parametrize("arch", ["small_cond", "small_joint"])
@pytest.mark.parametrize("case", ["ragged"])
def test_degenerate_backward_keeps_its_bits_across_streams_and_z2(case, arch):
    """DSBDD_TRAIN_STREAMS (side streams of the backward) and DSBDD_TRAIN_STORE_Z2 (kept z2 or recompute) are read when the
    handle is created: fresh modules.  The stream mask must not move a bit, repeats are identical, and both z2 modes meet
    the float64 bound."""
    runs = {}
    for mask in ("0", "15"):
        with env(DSBDD_TRAIN=None, DSBDD_TRAIN_STREAMS=mask, DSBDD_TRAIN_STORE_Z2=None):
            m = fresh_module(arch)
            runs[mask] = [forward_backward(m, case, arch)[0] for _ in range(2)]
    ref = runs["0"][0]
    assert len(ref) > 10
    for mask, rr in runs.items():
        for i, r in enumerate(rr):
            same_bits(r, ref, (mask, i))
    for z2 in ("0", "1"):
        with env(DSBDD_TRAIN=None, DSBDD_TRAIN_STREAMS=None, DSBDD_TRAIN_STORE_Z2=z2):
            got, status = forward_backward(fresh_module(arch), case, arch)
        assert status == 0
        check_against_float64(got, case, arch, f"net,z2={z2}/{arch}/{case}")
