"""The keyed noise generator and the eight per-sample DDPM step kernels of csrc/ddpm.h, each through the C ABI and in
isolation, against references that no GPU code produced:

  * dsbdd_randn_keyed element by element against oracle/keyed_noise.py (pinned on the host by tests/test_keyed_noise.py:
    published Philox known answers, distribution, key domain), one call per row of a key table that moves one input;
  * dsbdd_cond_step_keyed (noise evaluated in place) against the float64 step restatement fed with HOST noise;
  * tests.test_testset._KeyedNoise -- the noise source of every oracle chain test -- against the host values;
  * the eight step entry points against float64 torch restatements written from the header (tests/_steps64.py) on a ragged
    batch with empty / one-row / > 256-row samples, un-centred coordinates, dl != dp, every flag; plus: inputs that are
    not in-place are unchanged, rows of other samples and guard rows are untouched, bitwise reproducibility, bitwise
    batch-composition invariance (the header's claim).

Tolerance: the rule of tests/test_gpu_trainer.py (tests/_steps64.py: within).  err_ref = the float32 evaluation of the
same restatement against the float64 one; the kernel must satisfy |hip - f64| <= max(2 err_ref, 4 ulp) relative to the
output tensor's largest magnitude, and never exceed 1e-4.  The figures each test prints on the MI355X are recorded in
profiles/ddpm_kernels_error.md.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import keyed_noise as kn
from tests import _steps64 as s64

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GUARD = 2


def dev():
    return torch.device("cuda:0")


def lib_():
    from diffsbdd_amd import _lib
    return _lib, _lib.load()


def f32(v):
    """A scalar as the float the C ABI receives."""
    return float(np.float32(v))


def mask_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor([int(s) for s in sizes], dtype=torch.int64))


# =========================================================================================================================
# noise
# =========================================================================================================================
def hip_randn(sizes, n_cols, seed, draw, stream, offset=0, ids=None):
    _lib, lib = lib_()
    d = dev()
    n = int(sum(sizes))
    mask = mask_of(sizes).to(d)
    out = torch.full((n + GUARD, n_cols), SENTINEL, device=d)
    idt = None if ids is None else torch.tensor([i if i < 2 ** 63 else i - 2 ** 64 for i in ids], dtype=torch.int64, device=d)
    _lib.check(lib.dsbdd_randn_keyed(None, out.data_ptr(), mask.data_ptr(), n, n_cols, len(sizes), offset,
                                     None if idt is None else idt.data_ptr(), C.c_uint64(seed), C.c_uint64(draw),
                                     C.c_uint32(stream)), "dsbdd_randn_keyed")
    torch.cuda.synchronize()
    assert (out[n:] == SENTINEL).all()
    return out[:n].cpu()


RAGGED = [5, 0, 1, 1000, 0, 37, 3]
EVEN = [40] * 6
KEY_TABLE = {   # each row moves one input of the base row
    "base": dict(),
    "seed_high_word": dict(seed=(0x9E3779B9 << 32) | 7),
    "seed_all_bits": dict(seed=2 ** 64 - 1),
    "draw_2^32": dict(draw=2 ** 32),
    "draw_high_bits": dict(draw=(0xC0FFEE << 32) | 3),
    "stream_1": dict(stream=1),
    "stream_max": dict(stream=0xFFFFFFFF),
    "offset_crosses_2^32": dict(offset=2 ** 32 - 3),
    "offset_beyond_2^32": dict(offset=(7 << 32) + 11),
    "ids_unsorted_above_2^32": dict(ids=[15, 3, (5 << 32) | 9, 8, 2 ** 32 - 1, 0]),
    "cols_1": dict(n_cols=1),
    "cols_3": dict(n_cols=3),
    "cols_23": dict(n_cols=23),
    "ragged": dict(sizes=RAGGED),
    "ragged_ids_cols_23": dict(sizes=RAGGED, n_cols=23, ids=[9, 2 ** 32 + 1, 4, 77, 5, 2 ** 40, 1]),
}


@pytest.mark.parametrize("row", list(KEY_TABLE))
def test_randn_keyed_vs_host_restatement(row):
    k = dict(seed=7, draw=3, stream=0, offset=0, ids=None, n_cols=13, sizes=EVEN)
    k.update(KEY_TABLE[row])
    hip = hip_randn(k["sizes"], k["n_cols"], k["seed"], k["draw"], k["stream"], k["offset"], k["ids"])
    ref = {dt: kn.randn_keyed(k["seed"], k["draw"], k["stream"], k["ids"], k["sizes"], k["n_cols"], dt, k["offset"])
           for dt in (np.float64, np.float32)}
    assert hip.shape == ref[np.float64].shape
    e = s64.within(f"randn_keyed[{row}]", hip, ref[np.float64], torch.from_numpy(ref[np.float32]))
    print(f"WORST randn_keyed {e[0]:.3e} {e[1]:.3e}")
    if row != "base" and k["sizes"] is EVEN and k["n_cols"] == 13:
        # the row's input reached the counter: a block unrelated to the base block
        base = torch.from_numpy(kn.randn_keyed(7, 3, 0, None, EVEN, 13, np.float64))
        assert float((base - hip.double()).abs().max()) > 1.0


def test_randn_keyed_large_draw_is_finite_and_inside_the_tail_bound():
    """8 M values in one call: every value finite, |z| <= sqrt(48 ln 2) (what a 24-bit u1 in (0, 1] allows)."""
    rows, B, cols = 9616, 64, 13
    _lib, lib = lib_()
    d = dev()
    mask = mask_of([rows] * B).to(d)
    out = torch.empty((rows * B, cols), device=d)
    assert out.numel() >= 8_000_000
    _lib.check(lib.dsbdd_randn_keyed(None, out.data_ptr(), mask.data_ptr(), rows * B, cols, B, 0, None, C.c_uint64(7),
                                     C.c_uint64(3), C.c_uint32(0)), "dsbdd_randn_keyed")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    big = float(out.abs().max())
    print(f"  largest |z| of {out.numel()} values: {big:.6f}  (bound {kn.MAX_ABS:.6f})")
    assert big <= kn.MAX_ABS
    # its first 400 rows are the first sample of tests/test_keyed_noise.py's block: a sample's rows do not depend on its length
    ref = kn.randn_keyed(7, 3, 0, None, [400], cols, np.float64)
    ref32 = kn.randn_keyed(7, 3, 0, None, [400], cols, np.float32)
    s64.within("randn_keyed[8M, first 400 rows]", out[:400].cpu(), ref, torch.from_numpy(ref32))


def test_oracle_chain_noise_source_returns_the_host_values():
    """tests.test_testset._KeyedNoise feeds every "vs oracle" chain test that draws keyed noise; its first four draws are
    the restatement's draws 0 - 3 (stream 0, the given global ids), so those oracles no longer rest on the kernel."""
    from tests.test_testset import _KeyedNoise
    sizes, ids, seed = [11, 3, 0, 24, 7], [12, 5, 40, 2, 9], 5
    src = _KeyedNoise(seed, ids, mask_of(sizes), dev())
    for draw, cols in enumerate((13, 13, 3, 13)):
        got = src((sum(sizes), cols))
        ref = kn.randn_keyed(seed, draw, 0, ids, sizes, cols, np.float64)
        ref32 = kn.randn_keyed(seed, draw, 0, ids, sizes, cols, np.float32)
        s64.within(f"_KeyedNoise draw {draw}", got, ref, torch.from_numpy(ref32))
    assert src.i == 4


# =========================================================================================================================
# step kernels
# =========================================================================================================================
BATCHES = {"ragged": ([23, 0, 1, 257, 300, 5, 0], [286, 40, 0, 1, 513, 3, 0]), "single": ([23], [286])}
SHAPES = [("ragged", 10, 10), ("ragged", 10, 20), ("ragged", 11, 21), ("single", 11, 21)]
COEF = dict(alpha_ts=f32(0.98731), c_eps=f32(0.04217), sigma=f32(0.11093), alpha_s=f32(0.81347), sigma_s=f32(0.58159),
            sigma_ts=f32(0.15891), a=f32(0.93517))


def fixed_mask(sizes, mode, g, zero_samples=()):
    """mode: ones / zeros / mixed.  mixed varies per sample: random 0/1, all ones, all zeros in turn."""
    out = []
    for b, n in enumerate(sizes):
        kind = mode if mode != "mixed" else ("random", "ones", "zeros")[b % 3]
        if b in zero_samples:
            kind = "zeros"
        out.append({"ones": torch.ones(n), "zeros": torch.zeros(n),
                    "random": (torch.rand(n, generator=g) < 0.5).float()}[kind])
    return torch.cat(out)


def make_case(batch, atom_nf, residue_nf, fixed="mixed", seed=0):
    """float32 inputs on the host.  Coordinates un-centred at PDB-like magnitude (sample centres tens of Angstrom from the
    origin), so that the COM subtractions cancel."""
    lsz, psz = BATCHES[batch]
    g = torch.Generator().manual_seed(1000 * atom_nf + residue_nf + seed)
    dl, dp = 3 + atom_nf, 3 + residue_nf
    centre = (torch.rand(len(lsz), 3, generator=g) - 0.5) * 120.0

    def rows(sizes, d, spread):
        m = mask_of(sizes)
        x = centre[m] + torch.randn(len(m), 3, generator=g) * spread
        return torch.cat([x, torch.randn(len(m), d - 3, generator=g)], 1)

    def randn(sizes, d):
        return torch.randn(int(sum(sizes)), d, generator=g)

    L = dict(z=rows(lsz, dl, 3.0), eps=randn(lsz, dl), noise=randn(lsz, dl), noise2=randn(lsz, dl), xh0=rows(lsz, dl, 3.0))
    P = dict(poc=rows(psz, dp, 9.0), eps=randn(psz, dp), noise=randn(psz, dp), noise2=randn(psz, dp),
             xh0=rows(psz, dp, 9.0))
    # samples 4 and 5 (where present): no fixed pocket node, so that with no fixed ligand atom the count clamps to 1
    L["fixed"] = fixed_mask(lsz, fixed, g)
    P["fixed"] = fixed_mask(psz, "ones", g, zero_samples=(4, 5))
    S = dict(com0=s64.segment_mean3(P["poc"], psz) + torch.randn(len(lsz), 3, generator=g) * 0.5)
    return L, P, S, list(lsz), list(psz), dl, dp


class Dev:
    """Device copies of a case with GUARD sentinel rows behind every per-row tensor."""

    def __init__(self, L, P, S, lsz, psz):
        d = dev()

        def up(t):
            pad = torch.full((GUARD,) + tuple(t.shape[1:]), SENTINEL)
            return torch.cat([t.float(), pad]).contiguous().to(d)
        self.L = {k: up(v) for k, v in L.items()}
        self.P = {k: up(v) for k, v in P.items()}
        self.S = {k: v.float().contiguous().to(d) for k, v in S.items()}
        self.nl, self.np, self.B = int(sum(lsz)), int(sum(psz)), len(lsz)
        # (guard entries behind the masks too: a set with no rows at all still has an address)
        self.ml, self.mp = (torch.cat([mask_of(s), torch.full((GUARD,), 2 ** 40)]).to(d) for s in (lsz, psz))
        self.L["scratch"] = torch.full_like(self.L["z"], SENTINEL)
        self.P["scratch"] = torch.full_like(self.P["poc"], SENTINEL)

    def snapshot(self):
        return ({k: v.clone() for k, v in self.L.items()}, {k: v.clone() for k, v in self.P.items()},
                {k: v.clone() for k, v in self.S.items()})


def p(t):
    return t.data_ptr()


# name -> (restatement, launcher, scalar names).  A launcher gets (lib, D: Dev, batch, atom_nf, residue_nf, **scalars) and
# returns the status code; every entry point writes L["z"] and P["poc"] in place (+ its scratch).
def _run_cond_reverse(lib, D, B, anf, rnf, *, alpha_ts, c_eps, sigma, remove_com):
    return lib.dsbdd_cond_reverse_update(None, p(D.L["z"]), p(D.P["poc"]), p(D.L["eps"]), p(D.L["noise"]), p(D.ml), p(D.mp),
                                         D.nl, D.np, B, anf, rnf, alpha_ts, c_eps, sigma, remove_com)


def _run_joint_reverse(lib, D, B, anf, rnf, *, alpha_ts, c_eps, sigma, center_noise):
    return lib.dsbdd_joint_reverse_update(None, p(D.L["z"]), p(D.P["poc"]), p(D.L["eps"]), p(D.P["eps"]), p(D.L["noise"]),
                                          p(D.P["noise"]), p(D.ml), p(D.mp), D.nl, D.np, B, anf, rnf, alpha_ts, c_eps,
                                          sigma, center_noise)


def _run_cond_affine(lib, D, B, anf, rnf, *, a, sigma, remove_com):
    return lib.dsbdd_cond_affine_noise(None, p(D.L["z"]), p(D.P["poc"]), p(D.L["noise"]), p(D.ml), p(D.mp), D.nl, D.np, B,
                                       anf, rnf, a, sigma, remove_com)


def _run_joint_affine(lib, D, B, anf, rnf, *, a, sigma, center_noise, remove_com):
    return lib.dsbdd_joint_affine_noise(None, p(D.L["z"]), p(D.P["poc"]), p(D.L["noise"]), p(D.P["noise"]), p(D.ml),
                                        p(D.mp), D.nl, D.np, B, anf, rnf, a, sigma, center_noise, remove_com)


def _run_cond_repaint(lib, D, B, anf, rnf, *, alpha_s, sigma_s, alpha_ts, sigma_ts, resample, remove_com):
    return lib.dsbdd_cond_repaint_update(None, p(D.L["z"]), p(D.P["poc"]), p(D.L["scratch"]), p(D.L["xh0"]),
                                         p(D.S["com0"]), p(D.L["fixed"]), p(D.L["noise"]), p(D.L["noise2"]), p(D.ml),
                                         p(D.mp), D.nl, D.np, B, anf, rnf, alpha_s, sigma_s, alpha_ts, sigma_ts, resample,
                                         remove_com)


def _run_joint_repaint(lib, D, B, anf, rnf, *, alpha_s, sigma_s, alpha_ts, sigma_ts, jump):
    return lib.dsbdd_joint_repaint_update(None, p(D.L["z"]), p(D.P["poc"]), p(D.L["scratch"]), p(D.P["scratch"]),
                                          p(D.L["xh0"]), p(D.P["xh0"]), p(D.L["fixed"]), p(D.P["fixed"]), p(D.L["noise"]),
                                          p(D.P["noise"]), p(D.L["noise2"]), p(D.P["noise2"]), p(D.ml), p(D.mp), D.nl,
                                          D.np, B, anf, rnf, alpha_s, sigma_s, alpha_ts, sigma_ts, jump)


def _grid(**axes):
    return [dict(zip(axes, v)) for v in itertools.product(*axes.values())]


def _c(*names):
    return {n: COEF[n] for n in names}


ENTRY = {
    "cond_reverse_update": (s64.cond_reverse_update, _run_cond_reverse,
                            [dict(_c("alpha_ts", "c_eps", "sigma"), **f) for f in _grid(remove_com=[0, 1])]),
    "joint_reverse_update": (s64.joint_reverse_update, _run_joint_reverse,
                             [dict(_c("alpha_ts", "c_eps", "sigma"), **f) for f in _grid(center_noise=[0, 1])]),
    "cond_affine_noise": (s64.cond_affine_noise, _run_cond_affine,
                          [dict(_c("sigma"), **f) for f in _grid(a=[COEF["a"], 1.0], remove_com=[0, 1])]),
    "joint_affine_noise": (s64.joint_affine_noise, _run_joint_affine,
                           [dict(_c("sigma"), **f) for f in _grid(a=[COEF["a"], 0.0], center_noise=[0, 1],
                                                                  remove_com=[0, 1])]),
    "cond_repaint_update": (s64.cond_repaint_update, _run_cond_repaint,
                            [dict(_c("alpha_s", "sigma_s", "alpha_ts", "sigma_ts"), **f)
                             for f in _grid(resample=[0, 1], remove_com=[0, 1])]),
    "joint_repaint_update": (s64.joint_repaint_update, _run_joint_repaint,
                             [dict(_c("alpha_s", "sigma_s", "alpha_ts", "sigma_ts"), **f) for f in _grid(jump=[0, 1])]),
}
FIXED_MODES = {"cond_repaint_update": ["ones", "zeros", "mixed"], "joint_repaint_update": ["ones", "zeros", "mixed"]}


def launch(name, D, B, anf, rnf, scalars):
    _lib, lib = lib_()
    _lib.check(ENTRY[name][1](lib, D, B, anf, rnf, **scalars), "dsbdd_" + name)
    torch.cuda.synchronize()


def sub_case(L, P, S, lsz, psz, b):
    """Sample b alone, relabelled 0."""
    lo, po = s64.offsets(lsz), s64.offsets(psz)
    return ({k: v[lo[b]:lo[b + 1]] for k, v in L.items()}, {k: v[po[b]:po[b + 1]] for k, v in P.items()},
            {k: v[b:b + 1] for k, v in S.items()}, [lsz[b]], [psz[b]])


def check_entry(name, case, anf, rnf, scalars, run=None, extra_in=None, worst=None):
    """One entry point on one case with one set of scalars: values, untouched inputs / guard rows / other samples,
    reproducibility, batch-composition invariance.  `run` overrides the launcher (the keyed step)."""
    fn = ENTRY[name][0] if name in ENTRY else s64.cond_step_keyed
    run = run or (lambda D, B, ids=None: launch(name, D, B, anf, rnf, scalars))
    L, P, S, lsz, psz = case
    B = len(lsz)
    nan_z = scalars.get("a", 1.0) == 0.0
    Lh, Ph = dict(L), dict(P)
    if nan_z:                  # a = 0 must not read z: NaN on the device, a finite stand-in for the restatement
        Lh["z"], Ph["poc"] = torch.full_like(L["z"], float("nan")), torch.full_like(P["poc"], float("nan"))
    D = Dev(Lh, Ph, S, lsz, psz)
    before = D.snapshot()
    run(D, B)
    # ---- values ------------------------------------------------------------------------------------------------------
    L64, P64 = dict(L, **(extra_in or {}).get(torch.float64, {})), P
    L32 = dict(L, **(extra_in or {}).get(torch.float32, {}))
    ref64 = s64.evaluate(fn, L64, P64, S, lsz, psz, torch.float64, **scalars)
    ref32 = s64.evaluate(fn, L32, P, S, lsz, psz, torch.float32, **scalars)
    tag = f"{name}[{' '.join(f'{k}={v:g}' for k, v in scalars.items() if k not in COEF or k == 'a')}]"
    for key, which, n in (("z", 0, D.nl), ("poc", 1, D.np)):
        hip = (D.L if which == 0 else D.P)[key][:n].cpu()
        e = s64.within(f"{tag}.{key}", hip, ref64[which][key], ref32[which][key])
        if worst is not None and e[1] >= worst.get(key, (0, -1))[1]:
            worst[key] = e
    if nan_z and not scalars["center_noise"] and not scalars["remove_com"]:      # then the result is sigma * noise itself
        for out, noise in ((D.L["z"][:D.nl], L["noise"]), (D.P["poc"][:D.np], P["noise"])):
            assert float((out.cpu().double() - scalars["sigma"] * noise.double()).abs().max()) <= 1e-6
    # ---- what must not change ------------------------------------------------------------------------------------------
    after = D.snapshot()
    for bd, ad, n, written in ((before[0], after[0], D.nl, ("z", "scratch")), (before[1], after[1], D.np, ("poc", "scratch"))):
        for k in bd:
            if k in written:
                assert torch.equal(ad[k][n:], bd[k][n:]), (name, k, "guard rows")
            else:
                assert torch.equal(ad[k], bd[k]), (name, k, "input modified")
    assert torch.equal(after[2]["com0"], before[2]["com0"])
    # ---- bitwise reproducible ---------------------------------------------------------------------------------------------
    D2 = Dev(Lh, Ph, S, lsz, psz)
    run(D2, B)
    assert torch.equal(D2.L["z"], D.L["z"]) and torch.equal(D2.P["poc"], D.P["poc"]), (name, "not reproducible")
    # ---- only the first `batch` samples are touched, and they do not depend on the others --------------------------------
    if B > 1:
        Bh = 4
        lo, po = s64.offsets(lsz), s64.offsets(psz)
        D3 = Dev(Lh, Ph, S, lsz, psz)
        run(D3, Bh)
        for k, Dd, o, bd in (("z", D3.L, lo, before[0]), ("poc", D3.P, po, before[1])):
            assert torch.equal(Dd[k][:o[Bh]], (D.L if k == "z" else D.P)[k][:o[Bh]]), (name, k, "depends on later samples")
            same = torch.equal(Dd[k][o[Bh]:], bd[k][o[Bh]:]) if not nan_z else \
                bool(torch.isnan(Dd[k][o[Bh]:o[B]]).all()) and torch.equal(Dd[k][o[B]:], bd[k][o[B]:])
            assert same, (name, k, "rows of other samples written")
        # ---- a sample evaluated alone, relabelled 0, equals its rows in the batch, bit for bit -------------------------
        for b in range(B):
            if lsz[b] + psz[b] == 0:
                continue
            sub = sub_case(Lh, Ph, S, lsz, psz, b)
            D4 = Dev(*sub)
            run(D4, 1, b)
            assert torch.equal(D4.L["z"][:lsz[b]], D.L["z"][lo[b]:lo[b + 1]]), (name, b, "ligand rows depend on the batch")
            assert torch.equal(D4.P["poc"][:psz[b]], D.P["poc"][po[b]:po[b + 1]]), (name, b, "pocket rows depend on the batch")


def soft(failures, f, *a, **k):
    try:
        f(*a, **k)
    except AssertionError as exc:
        failures.append(str(exc)[:300])


@pytest.mark.parametrize("batch,anf,rnf", SHAPES)
@pytest.mark.parametrize("name", list(ENTRY))
def test_step_entry_point_vs_float64_restatement(name, batch, anf, rnf):
    failures, worst = [], {}
    for mode in FIXED_MODES.get(name, ["mixed"]):
        L, P, S, lsz, psz, dl, dp = make_case(batch, anf, rnf, fixed=mode)
        for scalars in ENTRY[name][2]:
            if name in FIXED_MODES:
                print(f" fixed = {mode}")
            soft(failures, check_entry, name, (L, P, S, lsz, psz), anf, rnf, scalars, worst=worst)
    for key, e in worst.items():
        print(f"WORST {name}.{key} {e[0]:.3e} {e[1]:.3e}")
    assert not failures, failures


@pytest.mark.parametrize("batch,anf,rnf", SHAPES)
def test_segment_mean3_vs_float64_restatement(batch, anf, rnf):
    _lib, lib = lib_()
    L, P, S, lsz, psz, dl, dp = make_case(batch, anf, rnf)
    worst = (0.0, -1.0)
    for rows, sizes, ld in ((L["z"], lsz, dl), (P["poc"], psz, dp), (L["z"][:, :3].contiguous(), lsz, 3)):
        B, n = len(sizes), int(sum(sizes))
        d = dev()
        x = torch.cat([rows, torch.full((GUARD, ld), SENTINEL)]).to(d)
        x0, m = x.clone(), mask_of(sizes).to(d)
        out = torch.full((B + GUARD, 3), SENTINEL, device=d)
        _lib.check(lib.dsbdd_segment_mean3(None, p(x), ld, p(m), n, B, p(out)), "dsbdd_segment_mean3")
        torch.cuda.synchronize()
        assert torch.equal(x, x0) and (out[B:] == SENTINEL).all()
        ref64 = s64.segment_mean3(rows.double(), sizes)
        e = s64.within(f"segment_mean3[ld={ld}]", out[:B].cpu(), ref64, s64.segment_mean3(rows, sizes))
        worst = max(worst, e, key=lambda v: v[1])
        for b, s in enumerate(sizes):                    # an empty sample: count clamped to 1, the mean is 0
            if s == 0:
                assert (out[b] == 0).all()
        out2 = torch.full_like(out, SENTINEL)
        _lib.check(lib.dsbdd_segment_mean3(None, p(x), ld, p(m), n, B, p(out2)), "dsbdd_segment_mean3")
        torch.cuda.synchronize()
        assert torch.equal(out2, out)
        o = s64.offsets(sizes)
        for b, s in enumerate(sizes):                    # each sample alone, relabelled 0
            if s == 0:
                continue
            xb, mb = x[o[b]:o[b + 1]].contiguous(), torch.zeros(s, dtype=torch.int64, device=d)
            ob = torch.full((1 + GUARD, 3), SENTINEL, device=d)
            _lib.check(lib.dsbdd_segment_mean3(None, p(xb), ld, p(mb), s, 1, p(ob)), "dsbdd_segment_mean3")
            torch.cuda.synchronize()
            assert torch.equal(ob[0], out[b]) and (ob[1:] == SENTINEL).all(), (b, "depends on the batch")
    print(f"WORST segment_mean3.out {worst[0]:.3e} {worst[1]:.3e}")


# ---- the fused keyed step: noise evaluated in place ---------------------------------------------------------------------------
KEYED_SEED, KEYED_DRAW = (0xABCD << 32) | 7, 6
KEYED_IDS = {"ragged": [17, 3, 900, 2 ** 32 - 1, 5, 44, 8], "single": [70000]}


@pytest.mark.parametrize("id_mode", ["sample_ids", "sample_offset"])
@pytest.mark.parametrize("repaint", [0, 1, 2])
@pytest.mark.parametrize("batch,anf,rnf", SHAPES)
def test_cond_step_keyed_vs_float64_restatement_on_host_noise(batch, anf, rnf, repaint, id_mode):
    """Expected values: tests/_steps64.py in float64 on oracle/keyed_noise.py's draws d, d + 1, d + 2 -- no GPU draw."""
    _lib, lib = lib_()
    failures, worst = [], {}
    t_next = f32(0.37)
    for mode, remove_com in itertools.product(["mixed"] if repaint == 0 else ["ones", "zeros", "mixed"], [0, 1]):
        L, P, S, lsz, psz, dl, dp = make_case(batch, anf, rnf, fixed=mode)
        offset = 1000
        gids = KEYED_IDS[batch] if id_mode == "sample_ids" else [b + offset for b in range(len(lsz))]
        noise = {dt: {k: torch.from_numpy(kn.randn_keyed(KEYED_SEED, KEYED_DRAW + j, 0, gids, lsz, dl, nd))
                      for j, k in enumerate(("noise", "noise1", "noise2"))}
                 for dt, nd in ((torch.float64, np.float64), (torch.float32, np.float32))}
        scalars = dict(_c("alpha_ts", "c_eps", "sigma", "alpha_s", "sigma_s", "sigma_ts"), repaint=repaint,
                       remove_com=remove_com)
        Lin = {k: v for k, v in L.items() if k in ("z", "eps", "xh0", "fixed")}
        Pin = {"poc": P["poc"]}

        def run(D, B, alone=None, scalars=scalars, gids=gids):
            d = dev()
            # whole batch: explicit ids or the offset; one sample alone: its own global id, by either route
            ids = gids if alone is None else [gids[alone]]
            use_ids = id_mode == "sample_ids"
            idt = torch.tensor(ids, dtype=torch.int64, device=d) if use_ids else None
            off = 0 if use_ids else ids[0]
            t_word = torch.full((1 + GUARD,), -1.0, device=d)
            _lib.check(lib.dsbdd_cond_step_keyed(
                None, p(D.L["z"]), p(D.P["poc"]), p(D.L["eps"]), p(D.L["scratch"]), p(D.L["xh0"]), p(D.S["com0"]),
                p(D.L["fixed"]), p(D.ml), p(D.mp), D.nl, D.np, B, anf, rnf, scalars["alpha_ts"], scalars["c_eps"],
                scalars["sigma"], repaint, scalars["alpha_s"], scalars["sigma_s"], scalars["sigma_ts"], remove_com,
                C.c_uint64(KEYED_SEED), C.c_uint64(KEYED_DRAW), off, None if idt is None else p(idt), p(t_word), t_next),
                "dsbdd_cond_step_keyed")
            torch.cuda.synchronize()
            assert t_word.tolist() == [t_next, -1.0, -1.0], t_word.tolist()

        print(f" fixed = {mode}")
        soft(failures, check_entry, "cond_step_keyed", (Lin, Pin, S, lsz, psz), anf, rnf, scalars, run=run,
             extra_in=noise, worst=worst)
    for key, e in worst.items():
        print(f"WORST cond_step_keyed.{key} {e[0]:.3e} {e[1]:.3e}")
    assert not failures, failures
