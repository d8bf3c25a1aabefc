"""Inputs and references shared by tests/test_vina_minimize.py and tests/test_gpu_vina_minimize.py: the one-atom cases on a
line, the float64 restatement of the minimiser on the scoring batch of tests/_vina_cases.py (computed once per process; must
not be modified), and the bounds the rigidity checks use, derived here."""
import functools

import numpy as np

from diffsbdd_amd import vina as V
from tests import _vina_cases as C
from tests import _vina_grad_cases as GC

AXIS = np.asarray([1.0, 2.0, 2.0]) / 3.0                  # a unit vector with exact float64 components' squares summing to 1
STARTS = (4.5, 3.0, 6.0)                                  # r0 of the one-atom cases: inner well from both sides, outer well
R_SUM = 2 * V.XS_RADII["C"]                               # 3.8: d = r - 3.8 for a carbon / carbon pair
TOL = float(np.float32(V.MIN_TOL))


def pair_energy(d):
    """`inter` of one class-C ligand atom (code 1: no flags) and one class-C pocket atom at surface distance d, float64."""
    d = np.asarray(d, np.float64)
    w = V.WEIGHTS
    return w[0] * np.exp(-(2 * d) ** 2) + w[1] * np.exp(-((d - 3) / 2) ** 2) + w[2] * np.where(d < 0, d * d, 0.0)


@functools.lru_cache(maxsize=None)
def well(lo, hi):
    """argmin of `pair_energy` on [lo, hi] by a float64 scan at 1e-6 A (two orders below tol)."""
    d = np.linspace(lo, hi, int(round((hi - lo) * 1e6)) + 1)
    return float(d[int(np.argmin(pair_energy(d)))])


def target(r0):
    """The distance the one-atom case started at r0 must end at: the well it is in (the barrier between the two wells of
    this pair is the maximum of `pair_energy` between them, near d = 1.2; r0 = 6.0 is d = 2.2, beyond it)."""
    return R_SUM + (well(-0.5, 0.5) if r0 < 5.5 else well(2.0, 4.0))


def one_atom(r0):
    """One class-C ligand atom at r0 along AXIS from one class-C pocket atom at the origin: the scoring inputs."""
    return {"lig_x": (r0 * AXIS).astype(np.float32)[None], "lig_code": np.asarray([1], np.int32), "mol_off": np.asarray([0, 1], np.int32),
            "mol_group": np.zeros(1, np.int32), "mol_int": np.asarray([[1, 0, 0, 0]], np.int32),
            "poc_x": np.zeros((1, 3), np.float32), "poc_code": np.asarray([1], np.int32), "group_off": np.asarray([0, 1], np.int32)}


def one_atom_batch():
    """The three one-atom cases as one batch of three molecules on one group."""
    parts = [one_atom(r0) for r0 in STARTS]
    b = dict(parts[0])
    b["lig_x"], b["lig_code"] = np.concatenate([p["lig_x"] for p in parts]), np.concatenate([p["lig_code"] for p in parts])
    b["mol_off"], b["mol_group"] = np.arange(4, dtype=np.int32), np.zeros(3, np.int32)
    b["mol_int"] = np.concatenate([p["mol_int"] for p in parts])
    return b


@functools.lru_cache(maxsize=None)
def min_reference(seed=0):
    """(VinaMinimized of `_vina_minimize_host` on `score_batch(seed)` with the default settings, its trace): once."""
    b = C.score_batch(seed)
    trace = []
    return V._vina_minimize_host(*(b[k] for k in C.SCORE_KEYS), trace=trace), tuple(trace)


@functools.lru_cache(maxsize=None)
def first_step(seed=0):
    """Of every molecule of `grad_batch(seed)`: (E at the input, E after the first trial step of 0.25 A, twice the sum of the
    score's error bounds of `inter` at the input and at the trial coordinates), float64, from the restatement run with
    max_evals = 2; NaN where no trial is made.  A float32 evaluation of both energies orders them as the restatement does
    when the first exceeds the second by more than the third."""
    b = GC.grad_batch(seed)
    trace = []
    st = V._vina_minimize_host(*(b[k] for k in C.SCORE_KEYS), max_evals=2, trace=trace)
    B = len(b["mol_off"]) - 1
    out = np.full((B, 3), np.nan)
    for m in range(B):
        e = [float(v) for k, v in trace if k == m]
        if st.stat[m, V.S_STATUS] in (2, 3) or len(e) < 2:
            continue
        one, _ = C.sub_batch(b, [m])
        trial = dict(one)
        trial["lig_x"] = trial_coordinates(one, V.MIN_STEP)
        bound = sum(V.error_bound(*(v[k] for k in C.SCORE_KEYS))[1][0, V.M_INTER] for v in (one, trial))
        out[m] = e[0], e[1], 2 * bound
    return out


def trial_coordinates(one, step, rows=None):
    """The coordinates of the first trial of the one-molecule batch `one`, in float64 and rounded once: from `rows` = (F,
    M) float32 at the input (the restatement's own if None), by `pose_step` and `pose_coordinates`."""
    x0 = np.asarray(one["lig_x"], np.float32)
    if rows is None:
        g = V._vina_grad_host(*(one[k] for k in C.SCORE_KEYS))
        rows = g.mol_grad[0, V.G_NET].astype(np.float32), g.mol_grad[0, V.G_MOMENT].astype(np.float32)
    F, M = (np.asarray(v, np.float32).astype(np.float64) for v in rows)
    s = x0.astype(np.float64) - x0.astype(np.float64).sum(0) / len(x0)
    rho2, rho_max = max(float((s * s).sum() / len(x0)), 1.0), float(np.sqrt((s * s).sum(1).max()))
    u = V._norm3(F) + rho_max * V._norm3(M) / rho2
    shift, q = V.pose_step(np.zeros(3), [1.0, 0.0, 0.0, 0.0], F, M, rho2, float(np.float32(step)) / u)
    return V.pose_coordinates(x0, shift, q)


# ---- rigidity -------------------------------------------------------------------------------------------------------------------
def ulp32(v):
    """The spacing of float32 at |v| (elementwise, float64)."""
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


def pose_tolerance(x0, pose32):
    """Per component, how far the returned float32 x may be from float32((c0 + T) + R(q) s) recomputed from the pose as it
    is STORED (float32 [8]) -> [n, 3].  One float32 ulp of |x| (the kernel's own rounding against the recomputation's, and
    the last float64 bit of sin, cos, sqrt and of fused multiply-adds moving a rounding), and the rounding of the stored
    pose: |dT_k| <= 2^-24 |T_k|, |dq_k| <= 2^-24 each; an entry of R(q) is 2 (ab +- cd) or 1 - 2 (a^2 + b^2) in the components,
    so |dR_kj| <= 4 (|q|_1) 2^-24 <= 8 2^-24 (|q|_1 <= 2 for a unit quaternion), and |d(R s)_k| <= 8 2^-24 |s|_1.  The
    recomputed value is then rounded as well, which the one ulp covers together with the kernel's."""
    x0 = np.asarray(x0, np.float32).astype(np.float64)
    s = x0 - x0.sum(0) / max(len(x0), 1)
    x = V.pose_coordinates(x0.astype(np.float32), pose32[V.P_SHIFT].astype(np.float64), pose32[V.P_QUAT].astype(np.float64))
    return x, ulp32(x) + 2.0 ** -24 * np.abs(pose32[V.P_SHIFT].astype(np.float64))[None, :] + 8 * 2.0 ** -24 * np.abs(s).sum(1)[:, None]


def distance_tolerance(x):
    """How far a distance between two atoms of the returned x [n, 3] may be from the input's.  Every returned component is
    the exact rigid image's within half a float32 ulp, <= 2^-24 |x_k| (the float64 error of forming it is 2^-29 of that), so
    an atom is displaced by at most sqrt(3) 2^-24 max |x| and a distance changes by at most twice that; the input distances
    are exact in float64 up to 2^-52.  The quaternion is unit to 2^-52, which scales distances by as much."""
    top = float(np.abs(np.asarray(x, np.float64)).max()) if len(x) else 0.0
    return 2 * np.sqrt(3.0) * 2.0 ** -24 * top * (1 + 2.0 ** -20)


def distances(x):
    x = np.asarray(x, np.float64)
    return np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))


def check_rigid(x_in, x_out, pose, off, skip=()):
    """The rigidity assertions of both test files on a batch: `x_out` against the recomputation from `pose` [B, 8] as stored
    (float32 on the device; the restatement's float64 pose is rounded to float32 first, which the tolerance covers), and the
    intra-ligand distances of every molecule with n >= 2.  -> the largest fractions of the two tolerances used."""
    used = [0.0, 0.0]
    for m in range(len(off) - 1):
        lo, hi = int(off[m]), int(off[m + 1])
        if m in skip or hi <= lo:
            continue
        p32 = np.asarray(pose[m], np.float32)
        want, tol = pose_tolerance(x_in[lo:hi], p32)
        err = np.abs(x_out[lo:hi].astype(np.float64) - want.astype(np.float64))
        assert (err <= tol).all(), (m, float((err / tol).max()))
        used[0] = max(used[0], float((err / tol).max()))
        assert abs(float((p32[V.P_QUAT].astype(np.float64) ** 2).sum()) - 1.0) <= 8 * 2.0 ** -24, m
        if hi - lo >= 2:
            dtol = distance_tolerance(x_out[lo:hi])
            dev = np.abs(distances(x_out[lo:hi]) - distances(x_in[lo:hi])).max()
            assert dev <= dtol, (m, dev, dtol)
            used[1] = max(used[1], float(dev / dtol))
    return used


def status_class(stat):
    return [V.STATUS[int(s)] for s in np.asarray(stat)[:, V.S_STATUS]]


def rigid_motion(x, shift=0.5, degrees=10.0, axis=(2.0, -1.0, 2.0), direction=(2.0, 3.0, -6.0)):
    """x [n, 3] moved as a rigid body, in float64: rotated by `degrees` about `axis` through its centroid, then translated by
    `shift` A along `direction` -> float32."""
    x = np.asarray(x, np.float64)
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.asarray(direction, np.float64) / np.linalg.norm(direction) * shift
    a = np.deg2rad(degrees)
    c = x.mean(0)
    s = x - c
    rot = s * np.cos(a) + np.cross(k, s) * np.sin(a) + np.outer(s @ k, k) * (1 - np.cos(a))
    return (c + t + rot).astype(np.float32)
