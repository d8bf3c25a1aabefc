"""Inputs and references shared by tests/test_vina_grad.py and tests/test_gpu_vina_grad.py: the scoring batch of
tests/_vina_cases.py with one more molecule (an atom exactly on a pocket atom of a multi-tile group), the float64
restatement of the gradient with its error bound (computed once per process; must not be modified), and an energy written
here on its own, in float64 on float64 coordinates, for finite differences."""
import functools

import numpy as np

from diffsbdd_amd import vina as V
from tests import _vina_cases as C

H = 1e-4                                   # finite-difference step, A
KINK_MARGIN = 1e-4                         # no flagged pair of the GPU batch is closer to a kink of its terms
_W = np.asarray(V.WEIGHTS, np.float64)
_R = np.asarray([0.0] + [V.XS_RADII[c] for c in V.CLASSES[1:]] + [0.0] * 5, np.float64)       # by the code's low four bits
# sup |T'|, sup |T''|, sup |T'''| over d of gauss1 = exp(-4 d^2) and gauss2 = exp(-((d - 3) / 2)^2): with f(a) = exp(-a^2),
# sup |f'| = sqrt(2 / e) = 0.858, sup |f''| = 2 (a = 0), sup |f'''| = |8 a^3 - 12 a| exp(-a^2) at a^2 = (3 - sqrt 6) / 2 = 3.904;
# gauss1 = f(2 d) scales them by 2, 4, 8, gauss2 = f((d - 3) / 2) by 1/2, 1/4, 1/8.  Rounded up.
SUP_GAUSS1, SUP_GAUSS2 = (1.716, 8.0, 32.0), (0.429, 0.5, 0.5)


@functools.lru_cache(maxsize=None)
def grad_batch(seed=0):
    """`score_batch(seed)` + molecule 16: six typed atoms on the 3 TILE + 5 group, atom 2 exactly on the first typed pocket
    atom of the group's second tile (a carbon / carbon pair with r = 0: terms as ever, no gradient)."""
    b = dict(C.score_batch(seed))
    rng = np.random.RandomState(1000 + seed)
    goff = b["group_off"]
    q, qcode = b["poc_x"][goff[4]:goff[5]], b["poc_code"][goff[4]:goff[5]]
    typed = np.nonzero(((qcode & 15) >= 1) & ((qcode & 15) <= 10))[0]
    on = int(typed[typed >= V.TILE][0])
    x = (q[on] + rng.uniform(-6, 6, (6, 3))).astype(np.float32)
    for _ in range(100):
        close = (np.abs(C._distances32(x, q).astype(np.float64) - V.CUTOFF) < 2 * C.MARGIN).any(1)
        if not close.any():
            break
        x[close] = (q[on] + rng.uniform(-6, 6, (int(close.sum()), 3))).astype(np.float32)
    x[2] = q[on]
    code = np.asarray([17, 34, 17, 66, 98, 22], np.int32)
    b["lig_x"], b["lig_code"] = np.concatenate([b["lig_x"], x]), np.concatenate([b["lig_code"], code])
    b["mol_off"] = np.concatenate([b["mol_off"], [b["mol_off"][-1] + 6]]).astype(np.int32)
    b["mol_group"] = np.concatenate([b["mol_group"], [4]]).astype(np.int32)
    b["mol_int"] = np.concatenate([b["mol_int"], [[6, 0, 3, 0]]]).astype(np.int32)
    b["coincident"] = (16, 2, on)                                          # molecule, atom in it, pocket atom in its group
    return b


@functools.lru_cache(maxsize=None)
def grad_reference(seed=0, appended=True):
    """(VinaGradients float64, grad_bound, mol_grad_bound) of `grad_batch(seed)` (or of `score_batch(seed)`): once."""
    b = grad_batch(seed) if appended else C.score_batch(seed)
    return V._vina_grad_host(*(b[k] for k in C.SCORE_KEYS), eps=V.EPS32)


def molecule_pairs(b, m):
    """The pair masks of molecule m of batch b, formed here from the codes and the float32 distances: (x float32 [n,3],
    q float32 [g,3], R_i, R_j, counted, hydrophobic, hbond, r32)."""
    off, goff = b["mol_off"], b["group_off"]
    g = int(b["mol_group"][m])
    lo, hi = int(off[m]), int(off[m + 1])
    glo, ghi = (int(goff[g]), int(goff[g + 1])) if 0 <= g < len(goff) - 1 else (0, 0)
    x, q = b["lig_x"][lo:hi], b["poc_x"][glo:ghi]
    ci, cj = b["lig_code"][lo:hi].astype(np.int64), b["poc_code"][glo:ghi].astype(np.int64)
    ki, kj = ci & 15, cj & 15
    typed = ((ki >= 1) & (ki <= 10))[:, None] & ((kj >= 1) & (kj <= 10))[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        r32 = C._distances32(x, q)
        counted = typed & (r32 < np.float32(8.0))
    hyd = ((ci[:, None] & 16) != 0) & ((cj[None, :] & 16) != 0)
    hb = (((ci[:, None] & 32) != 0) & ((cj[None, :] & 64) != 0)) | (((ci[:, None] & 64) != 0) & ((cj[None, :] & 32) != 0))
    return x, q, _R[ki], _R[kj], counted, hyd, hb, r32


def frozen_energy(x64, q64, ri, rj, counted, hyd, hb):
    """`inter` of every atom of one molecule against its group in float64 on float64 coordinates, over the FROZEN pair set
    `counted`: -> (energy [n], sum of |weighted terms| [n], d [n, m])."""
    e = x64[:, None, :] - q64[None, :, :]
    d = np.sqrt((e * e).sum(-1)) - ri[:, None] - rj[None, :]
    terms = (_W[0] * np.exp(-(2 * d) ** 2), _W[1] * np.exp(-(0.5 * (d - 3)) ** 2), _W[2] * np.minimum(d, 0.0) ** 2,
             _W[3] * np.where(hyd, np.clip(1.5 - d, 0.0, 1.0), 0.0), _W[4] * np.where(hb, np.clip(-d / 0.7, 0.0, 1.0), 0.0))
    total, size = sum(terms), sum(np.abs(t) for t in terms)
    return np.where(counted, total, 0.0).sum(1), np.where(counted, size, 0.0).sum(1), d


def kink_distance(d, counted, hyd, hb):
    """The smallest |d - kink| over the counted pairs and the kinks that apply to each: 0 for every pair (repulsion), 0.5 and
    1.5 for hydrophobic pairs, -0.7 (and 0) for hbond pairs."""
    out = np.abs(d)
    out = np.where(hyd, np.minimum(out, np.minimum(np.abs(d - 0.5), np.abs(d - 1.5))), out)
    out = np.where(hb, np.minimum(out, np.abs(d + 0.7)), out)
    return float(out[counted].min()) if counted.any() else np.inf


def third_derivative_bound(r, d, counted, hyd, hb, h=H):
    """sup over a step of h of |d^3 / dt^3| of a pair's weighted terms along a coordinate axis, summed over the counted pairs
    of every atom -> [n].  Along an axis d' = u_k, d'' = (1 - u_k^2) / r, d''' = -3 u_k (1 - u_k^2) / r^2, so |d'| <= 1,
    |d''| <= 1 / r, |d' d''| <= 0.385 / r < 1 / r, |d'''| <= 1.155 / r^2, and (T o d)''' = T''' d'^3 + 3 T'' d' d'' + T' d''' is at
    most S3 + 3 S2 / rho + 1.155 S1 / rho^2 with rho = r - h and S1..S3 the sups of |T'|, |T''|, |T'''| on the step: the
    constants above for the gaussians; (2 (|d| + h), 2, 0) for the repulsion where d < 0 and 0 where d > 0 (no pair is
    within 2 h of the kink); (1, 0, 0) for a hydrophobic and (1 / 0.7, 0, 0) for an hbond pair on any branch."""
    rho = np.where(counted, r - h, 1.0)
    s1 = np.abs(_W[0]) * SUP_GAUSS1[0] + np.abs(_W[1]) * SUP_GAUSS2[0] + np.abs(_W[2]) * np.where(d < 0, 2 * (np.abs(d) + h), 0.0) + \
        np.abs(_W[3]) * hyd + np.abs(_W[4]) * hb / 0.7
    s2 = np.abs(_W[0]) * SUP_GAUSS1[1] + np.abs(_W[1]) * SUP_GAUSS2[1] + np.abs(_W[2]) * np.where(d < 0, 2.0, 0.0)
    s3 = np.abs(_W[0]) * SUP_GAUSS1[2] + np.abs(_W[1]) * SUP_GAUSS2[2]
    return np.where(counted, s3 + 3 * s2 / rho + 1.155 * s1 / rho ** 2, 0.0).sum(1)
