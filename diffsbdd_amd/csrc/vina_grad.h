// Analytic gradient of the Vina-type interaction term with respect to the ligand coordinates, from the sweep that scores
// (vina_score.h): one launch, one workgroup per molecule, pair_sweep under VinaGradPolicy = VinaPolicy's record and calls
// for the five terms (atom_out, mol_out and mol_flag come out bit for bit as vina_score_kernel writes them) and three more
// doubles per atom for the gradient.
//
// Per counted pair (i ligand atom, j pocket atom; counted as in vina_score_kernel: both typed, float32 r^2 < 64), with
// e = (dx, dy, dz) the float32 differences pair_dist2 forms, r = sqrtf(r^2), and from here on float64: d = r - R_i - R_j,
// u = e / r (each float32 converted, then divided), and the derivatives in d, one-sided at the kinks as the terms are:
//   gauss1' = -8 d exp(-4 d^2);  gauss2' = -c exp(-c^2), c = (d - 3) / 2;  repulsion' = 2 d if d < 0, else 0;
//   hydrophobic' = -1 if 0.5 < d < 1.5, else 0;  hbond' = -1 / 0.7 if -0.7 < d < 0, else 0
// g_i = sum_j (sum_k w_k T_k'(d_ij)) u_ij = d inter / d x_i in kcal/mol/A.  A pair with r^2 == 0 has no direction: it adds to
// the terms and nothing to the gradient.  The cutoff at 8 A is a jump of the score itself (as in Vina) and the gradient
// ignores it: what comes out is the gradient of the sum over the pairs counted at x, not of a smoothed score.
//
// Per molecule: F = sum_i g_i, the moment about the centroid sum_i (x_i - c) x g_i (c the mean of all n atoms; sum x_i,
// sum g_i and sum x_i x g_i are carried in float64 and M - c x F is formed once), max_i |g_i| over the float64 norms, and
// 1 / (1 + 0.05846 N_rot), the factor between d inter / d x and d score / d x.  Sums, carries between tiles (in the output
// row, float32) and merges in the order pair_sweep fixes: no atomics, bitwise reproducible, independent of the batch.
#pragma once
#include "vina_score.h"

namespace dsbdd {

constexpr int kVinaMolGrad = 8;     // floats per molecule: F (3), moment about the centroid (3), max |g_i|, 1 / (1 + w N_rot)

struct VinaGradArgs {
  VinaScoreArgs score;     // what vina_score_kernel takes, its outputs included
  float* atom_grad;        // [N][3]
  float* mol_grad;         // [B][kVinaMolGrad]
};

// sum_k w_k T_k'(d) of one pair; the exponentials are those of vina_pair_terms
__device__ inline double vina_pair_slope(double d, bool hydrophobic, bool hbond) {
  const double a = d * 2.0, c = (d - 3.0) * 0.5;
  double s = kVinaWeight[0] * (-8.0 * d * exp(-(a * a))) + kVinaWeight[1] * (-c * exp(-(c * c)));
  if (d < 0.0) s += kVinaWeight[2] * (2.0 * d);
  if (hydrophobic && d > 0.5 && d < 1.5) s -= kVinaWeight[3];
  if (hbond && d > -0.7 && d < 0.0) s -= kVinaWeight[4] / 0.7;
  return s;
}

struct VinaGradPolicy {
  using Atom = VinaPolicy::Atom;
  struct Record { VinaPolicy::Record t; double g[3]; };     // 8 doubles, walked by fully unrolled loops only
  struct Total { VinaPolicy::Total t; double x[3], f[3], m[3], top; };     // sum x_i, sum g_i, sum x_i x g_i, max |g_i|
  const VinaGradArgs& p;
  const VinaPolicy terms;  // on p.score: the five terms go through its calls
  Total* part;             // [kThreads / 64] in LDS

  __device__ static Record zero() { return {VinaPolicy::zero(), {0, 0, 0}}; }
  __device__ static Total zero_total() { return {VinaPolicy::zero_total(), {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, 0}; }
  __device__ float tile_word(size_t r) const { return terms.tile_word(r); }
  __device__ Atom atom(size_t r, float x, float y, float z) const { return terms.atom(r, x, y, z); }
  __device__ static bool skip(const Atom& a) { return VinaPolicy::skip(a); }
  __device__ static void pair(Record& acc, const Atom& a, const float4 q, int) {
    VinaPolicy::Pair v;
    if (!VinaPolicy::counted(a, q, v)) return;
    vina_pair_terms(v.d, v.hyd, v.hb, acc.t.t);
    if (!(v.s > 0.0f)) return;                                      // the atoms coincide: no direction
    const double k = vina_pair_slope(v.d, v.hyd, v.hb), r = (double)v.r;
    acc.g[0] += k * ((double)(a.x - q.x) / r);
    acc.g[1] += k * ((double)(a.y - q.y) / r);
    acc.g[2] += k * ((double)(a.z - q.z) / r);
  }
  __device__ static void fold(Record& acc, int o) {
    VinaPolicy::fold(acc.t, o);
    for (int k = 0; k < 3; ++k) acc.g[k] += __shfl_xor(acc.g[k], o);
  }
  __device__ void carry(Record& acc, size_t r) const {
    terms.carry(acc.t, r);
    const float* out = p.atom_grad + 3 * r;
    for (int k = 0; k < 3; ++k) acc.g[k] += (double)out[k];
  }
  __device__ void store(const Record& acc, size_t r) const {
    terms.store(acc.t, r);
    float* out = p.atom_grad + 3 * r;
    for (int k = 0; k < 3; ++k) out[k] = (float)acc.g[k];
  }
  __device__ static void merge(Total& s, const Total& o) {
    VinaPolicy::merge(s.t, o.t);
    for (int k = 0; k < 3; ++k) {
      s.x[k] += o.x[k];
      s.f[k] += o.f[k];
      s.m[k] += o.m[k];
    }
    s.top = fmax(s.top, o.top);
  }
  __device__ static void total(Total& w, const Record& acc, const Atom& a) {
    VinaPolicy::total(w.t, acc.t, a);
    const double x[3] = {(double)a.x, (double)a.y, (double)a.z};
    for (int k = 0; k < 3; ++k) {
      w.x[k] += x[k];
      w.f[k] += acc.g[k];
      w.m[k] += x[(k + 1) % 3] * acc.g[(k + 2) % 3] - x[(k + 2) % 3] * acc.g[(k + 1) % 3];
    }
    w.top = fmax(w.top, sqrt((acc.g[0] * acc.g[0] + acc.g[1] * acc.g[1]) + acc.g[2] * acc.g[2]));
  }
  __device__ void finish(int b, int n, const Total& s) const {
    terms.finish(b, n, s.t);
    float* mol = p.mol_grad + (size_t)kVinaMolGrad * b;
    double c[3] = {0, 0, 0};
    if (n > 0)
      for (int k = 0; k < 3; ++k) c[k] = s.x[k] / (double)n;
    for (int k = 0; k < 3; ++k) {
      mol[k] = (float)s.f[k];
      mol[3 + k] = (float)(s.m[k] - (c[(k + 1) % 3] * s.f[(k + 2) % 3] - c[(k + 2) % 3] * s.f[(k + 1) % 3]));
    }
    mol[6] = (float)s.top;
    mol[7] = (float)(1.0 / vina_rot_divisor(p.score.mol_int, b));
  }
};

__global__ __launch_bounds__(kThreads) void vina_grad_kernel(VinaGradArgs p) {
  __shared__ VinaGradPolicy::Total part[kThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const PairRows rows = pair_rows(p.score.pairs, b);
  if (vina_nonfinite(p.score, rows, b)) {                           // NaN in the gradient floats the molecule owns as well
    const float nan = __builtin_nanf("");
    for (int k = tid; k < 3 * rows.n; k += kThreads) p.atom_grad[3 * (size_t)rows.lo + k] = nan;
    if (tid < kVinaMolGrad) p.mol_grad[(size_t)kVinaMolGrad * b + tid] = nan;
    return;
  }
  VinaGradPolicy pol{p, {p.score, nullptr}, part};
  pair_sweep(p.score.pairs, rows, pol);
}

}  // namespace dsbdd
