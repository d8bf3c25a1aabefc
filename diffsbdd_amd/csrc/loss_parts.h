// The parts that the twelve loss and score kernels share (loss_head.h, score.h, score_joint.h).  A kernel keeps its own row
// offsets, passes and output rows; a formula that two of them must compute to the same bit is stated here once: a sample's
// schedule scalars and rows, the size terms, a row's KL sums, the categorical term, the conditioned model's row steps, the
// joint model's noise rows, the squared-error rows, one element of their gradient.  Plain inline functions on the caller's
// locals; one that reaches block_sum or a barrier (rows_by_thread0, block_mean3, cond_lig_centre) is called on
// workgroup-uniform paths only.  Contraction is part of a formula's identity: where two kernels differ in it there are two
// functions, next to each other, each naming the other.  What stays written out, and why: profiles/loss_parts.md.
#pragma once
#include "common.h"
#include "ddpm.h"          // block_sum
#include "graph_parts.h"   // lower_bound_i64, SampleRows

namespace dsbdd {

struct LossCfg {
  int batch, n_lig, n_pocket, atom_nf, residue_nf, T;
  int remove_com;          // ConditionalDDPM: 1 (ligand COM removed from ligand and pocket); SimpleConditionalDDPM: 0
  int vnode_idx;           // class index of the virtual atom, or -1
  float nv0, nv1, nb1;     // norm_values[0], norm_values[1], norm_biases[1]
  int n1_tab, n2_tab;      // log p(n_lig | n_pocket) table [n1_tab][n2_tab]
};

constexpr int kLossThreads = 256;
// (block_sum of ddpm.h: fixed-order sum of one value per thread, every thread gets the total)
static_assert(kLossThreads == kThreads, "block_sum reduces kThreads values");
__device__ __forceinline__ float sigmoid_ref(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float cdf_gauss(float x) { return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)); }
// PredefinedNoiseSchedule.forward: gamma[round(t * T)] with python's negative indexing (s = -1 / T at t = 0)
__device__ __forceinline__ float gamma_at(const float* table, int T, float t) {
  int i = (int)rintf(t * (float)T);
  if (i < 0) i += T + 1;
  if (i > T) i = T;
  return table[i];
}

// ---- per-sample scalars (forward(): t, s, gamma; alpha / sigma) -----------------------------------------------------------
struct Schedule { float tt, g_t, g_s, alpha_t, sigma_t; };
__device__ __forceinline__ Schedule schedule_at(const float* gamma_table, int T, float ti) {
  Schedule s;
  s.tt = ti / (float)T;
  const float ss = (ti - 1.0f) / (float)T;
  s.g_t = gamma_at(gamma_table, T, s.tt); s.g_s = gamma_at(gamma_table, T, ss);
  s.alpha_t = sqrtf(sigmoid_ref(-s.g_t)); s.sigma_t = sqrtf(sigmoid_ref(s.g_t));
  return s;
}
__device__ __forceinline__ float snr_weight(const Schedule& s) { return 1.0f - expf(-(s.g_s - s.g_t)); }   // 1 - SNR(gamma_s - gamma_t)
struct PriorEnds { float g_0, alpha_T, sigma_T; };
__device__ __forceinline__ PriorEnds prior_ends(const float* gamma_table, int T) {
  const float g_T = gamma_table[T];
  return PriorEnds{gamma_table[0], sqrtf(sigmoid_ref(-g_T)), sqrtf(sigmoid_ref(g_T))};
}

// ---- a sample's rows ------------------------------------------------------------------------------------------------------
// thread 0 finds the bounds of sample b in both masks, the workgroup waits for them (the loss kernels; the score kernels
// have score_rows_of).  seg: 4 ints of LDS.
__device__ __forceinline__ SampleRows rows_by_thread0(const long long* lig_mask, int n_lig, const long long* poc_mask, int n_pocket,
                                                      int b, int* seg) {
  if (threadIdx.x == 0) {
    seg[0] = lower_bound_i64(lig_mask, n_lig, b); seg[1] = lower_bound_i64(lig_mask, n_lig, b + 1);
    seg[2] = lower_bound_i64(poc_mask, n_pocket, b); seg[3] = lower_bound_i64(poc_mask, n_pocket, b + 1);
  }
  __syncthreads();
  return SampleRows{seg[0], seg[1], seg[2], seg[3]};
}
__device__ __forceinline__ float seg_count(int n) { return (float)(n > 1 ? n : 1); }   // seg_mean: count clamped to >= 1
// m = the three thread sums, each through block_sum, over cnt
__device__ __forceinline__ void block_mean3(float s0, float s1, float s2, float cnt, float* red, float (&m)[3]) {
  m[0] = block_sum(s0, red) / cnt; m[1] = block_sum(s1, red) / cnt; m[2] = block_sum(s2, red) / cnt;
}

// ---- size terms -----------------------------------------------------------------------------------------------------------
// subspace_dimensionality: of the ligand (conditioned model), of ligand + pocket (joint model)
__device__ __forceinline__ float cond_dof(const LossCfg& c, int nl) { return c.remove_com ? (float)((nl - 1) * 3) : (float)(nl * 3); }
__device__ __forceinline__ float joint_dof(int nn) { return (float)((nn - 1) * 3); }
// -log_constants_p_x_given_z0
__device__ __forceinline__ float neg_log_constants(float dof, float g_0) { return -(dof * (-(0.5f * g_0) - 0.91893853320467274178f)); }
__device__ __forceinline__ float delta_log_px(float dof, float nv0) { return -dof * logf(nv0); }

// kl_prior = gaussian_KL(sx, sigma_T, 1, dof) + gaussian_KL(sh, sigma_T, 1, 1), with gaussian_KL(mu2, sigma_T, 1, d) =
// d log(1 / sigma_T) + 0.5 (d sigma_T^2 + mu2) - 0.5 d.  The conditioned kernels' form, under the default contraction (d =
// 3 (n_lig - 1) is small); the joint kernels' is kl_prior_rounded: they round differently, neither replaces the other.
__device__ __forceinline__ float kl_prior_contracted(float sx, float sh, float sigma_T, float dof) {
  const float lq = logf(1.0f / sigma_T), q2 = sigma_T * sigma_T;
  const float kl_x = dof * lq + 0.5f * (dof * q2 + sx) - 0.5f * dof;
  const float kl_h = lq + 0.5f * (q2 + sh) - 0.5f;
  return kl_x + kl_h;
}
// The joint kernels' form (the conditioned one: kl_prior_contracted).  With d = 3 (n_lig + n_pocket - 1) ~ 1e3 the addends
// are ~ +-d / 2 and cancel to ~ mu2 / 2 << 1, so a product left unrounded inside an fma moves the result by ulp(d / 2) ~
// 3e-5: every operation is rounded on its own here, as the mirror's separate torch operations are.
__device__ __forceinline__ float gaussian_kl_rounded(float mu2, float sigma_T, float d) {
#pragma clang fp contract(off)
  const float lq = logf(1.0f / sigma_T), q2 = sigma_T * sigma_T;
  return d * lq + 0.5f * (d * q2 + mu2) - 0.5f * d;
}
__device__ __forceinline__ float kl_prior_rounded(float sx, float sh, float sigma_T, float dof) {
  return gaussian_kl_rounded(sx, sigma_T, dof) + gaussian_kl_rounded(sh, sigma_T, 1.0f);
}

// log p(N_lig | N_pocket) (joint: log p(N_lig, N_pocket)).  The loss kernels clamp to the table (0 without one); the score
// kernels' host refuses sizes outside the table before any launch: no clamp, NaN (log_pn_or_nan).
__device__ __forceinline__ float log_pn_clamped(const LossCfg& c, const float* table, int nl, int np) {
  if (!table) return 0.f;
  const int i1 = nl < c.n1_tab ? nl : c.n1_tab - 1, i2 = np < c.n2_tab ? np : c.n2_tab - 1;
  return table[(size_t)i1 * c.n2_tab + i2];
}
__device__ __forceinline__ float log_pn_or_nan(const LossCfg& c, const float* table, int nl, int np) {
  return (nl < c.n1_tab && np < c.n2_tab) ? table[(size_t)nl * c.n2_tab + np] : NAN;
}

// ---- KL sums of the prior (kl_prior): one row's part ----------------------------------------------------------------------
// x, h: the row's raw coordinates and its nc raw features; mc: what the normalised coordinates are shifted by
__device__ __forceinline__ void kl_row(const LossCfg& c, float inv0, float inv1, const float* x, const float* h, int nc,
                                       const float (&mc)[3], float alpha_T, float& sx, float& sh) {
#pragma unroll
  for (int d = 0; d < 3; ++d) { const float mu = alpha_T * (x[d] * inv0 - mc[d]); sx += mu * mu; }
  for (int k = 0; k < nc; ++k) { const float mu = alpha_T * ((h[k] - c.nb1) * inv1); sh += mu * mu; }
}

// ---- the categorical term -------------------------------------------------------------------------------------------------
// one row of _log_ph_given_z0: sum_k (log p_k - logsumexp) onehot_k for the nc feature columns zh of a noised row; h = the
// row's raw one-hot (the mirror un-normalises the normalised one: same operations here).  Three passes over the columns.
// loss_cond_pre_kernel takes the first, mx = max_k log p_k, from its registers while it writes zh (cond_z_row<true>) and
// adds the terms to its running sum one by one (cat_row_add), not as a row's subtotal.  log p_k is written out four
// times: behind a function of its own the two cdf arguments are paired differently (profiles/loss_parts.md).
__device__ __forceinline__ void cat_row_add(const float* zh, const float* h, int nc, float nv1, float nb1, float inv1, float sig_cat,
                                            float mx, float& acc) {
  float se = 0.f;
  for (int k = 0; k < nc; ++k) {
    const float cen = (zh[k] * nv1 + nb1) - 1.0f;
    const float lp = logf(cdf_gauss((cen + 0.5f) / sig_cat) - cdf_gauss((cen - 0.5f) / sig_cat) + 1e-10f);
    se += expf(lp - mx);
  }
  const float lse = mx + logf(se);
  for (int k = 0; k < nc; ++k) {
    const float cen = (zh[k] * nv1 + nb1) - 1.0f;
    const float lp = logf(cdf_gauss((cen + 0.5f) / sig_cat) - cdf_gauss((cen - 0.5f) / sig_cat) + 1e-10f);
    const float onehot = ((h[k] - nb1) * inv1) * nv1 + nb1;
    acc += (lp - lse) * onehot;
  }
}
__device__ __forceinline__ float cat_row(const float* zh, const float* h, int nc, float nv1, float nb1, float inv1, float sig_cat) {
  float mx = -INFINITY;
  for (int k = 0; k < nc; ++k) {
    const float cen = (zh[k] * nv1 + nb1) - 1.0f;
    const float lp = logf(cdf_gauss((cen + 0.5f) / sig_cat) - cdf_gauss((cen - 0.5f) / sig_cat) + 1e-10f);
    mx = fmaxf(mx, lp);
  }
  float acc = 0.f;
  cat_row_add(zh, h, nc, nv1, nb1, inv1, sig_cat, mx, acc);
  return acc;
}
// this thread's part of sum log p(h | z) over the n rows of one node set (rows [o0, o0 + n) of z, rows [r0, r0 + n) of the
// caller's one-hot)
__device__ __forceinline__ float cat_rows(const LossCfg& c, int r0, int n, int o0, int nc, const float* z, const float* h,
                                          float sig_cat) {
  const float inv1 = 1.0f / c.nv1;
  float lh = 0.f;
  for (int i = (int)threadIdx.x; i < n; i += kLossThreads)
    lh += cat_row(z + (size_t)(o0 + i) * (3 + nc) + 3, h + (size_t)(r0 + i) * nc, nc, c.nv1, c.nb1, inv1, sig_cat);
  return lh;
}

// ---- the conditioned model's row steps (x, h: a row's raw coordinates and features; er: its noise row) --------------------
// ligand centre of mass of the normalised coordinates (_remove_lig_com); zero without remove_com
__device__ __forceinline__ void cond_lig_centre(const LossCfg& c, float inv0, const float* lig_x, int l0, int l1, float cnt,
                                                float* red, float (&m1)[3]) {
  m1[0] = m1[1] = m1[2] = 0.f;
  if (!c.remove_com) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int i = l0 + (int)threadIdx.x; i < l1; i += kLossThreads) { s0 += lig_x[3 * i] * inv0; s1 += lig_x[3 * i + 1] * inv0; s2 += lig_x[3 * i + 2] * inv0; }
  block_mean3(s0, s1, s2, cnt, red, m1);
}
// zr = the row of z_t: the noised coordinates centred by m2, the noised features.  CAT: returns max_k log p_k of the row's
// features (cat_row's first pass), else -inf
template <bool CAT>
__device__ __forceinline__ float cond_z_row(const LossCfg& c, float inv0, float inv1, const float* x, const float* h, const float* er,
                                           int nc, const float (&m1)[3], const float (&m2)[3], float alpha_t, float sigma_t,
                                           float* zr, float* xn_out, float* hn_out) {
  const float sig_cat = sigma_t * c.nv1;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float xn = x[d] * inv0;
    if (xn_out) xn_out[d] = xn;                                   // normalize() leaves the normalised batch in the caller's dicts
    zr[d] = (alpha_t * (xn - m1[d]) + sigma_t * er[d]) - m2[d];
  }
  float mx = -INFINITY;
  for (int k = 0; k < nc; ++k) {
    const float hn = (h[k] - c.nb1) * inv1;
    if (hn_out) hn_out[k] = hn;
    const float z = alpha_t * hn + sigma_t * er[3 + k];
    zr[3 + k] = z;
    if constexpr (CAT) {
      const float cen = (z * c.nv1 + c.nb1) - 1.0f;
      const float lp = logf(cdf_gauss((cen + 0.5f) / sig_cat) - cdf_gauss((cen - 0.5f) / sig_cat) + 1e-10f);
      mx = fmaxf(mx, lp);
    }
  }
  return mx;
}
// pr = the pocket row: normalised, shifted by both ligand centres
__device__ __forceinline__ void cond_pocket_row(const LossCfg& c, float inv0, float inv1, const float* x, const float* h, int nc,
                                                const float (&m1)[3], const float (&m2)[3], float* pr, float* xn_out,
                                                float* hn_out) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float xn = x[d] * inv0;
    if (xn_out) xn_out[d] = xn;
    pr[d] = (xn - m1[d]) - m2[d];
  }
  for (int k = 0; k < nc; ++k) {
    const float hn = (h[k] - c.nb1) * inv1;
    if (hn_out) hn_out[k] = hn;
    pr[3 + k] = hn;
  }
}

// ---- the joint model: noise rows of a node set ------------------------------------------------------------------------------
// eps = noise with its x part centred by m (_joint_noise), z = alpha_t xh + sigma_t eps (noised_representation), xh = the
// normalised row.  Two functions: z's coordinates round differently in the two kernels and must go on doing so.  In
// loss_joint_pre_kernel (noise_rows_train: rows [r0, r1), the normalised batch to xn_out / hn_out where given, returns
// this thread's part of sum log p(h | z_t)) both products are rounded, then added; in score_joint_pre_kernel
// (noise_rows_score) alpha_t xh is fused into the sum.  One function gave the score kernel the other rounding.
__device__ __forceinline__ float noise_rows_train(const LossCfg& c, int r0, int r1, int nc, const float* x, const float* h,
                                                  const float* noise, const float (&m)[3], float alpha_t, float sigma_t,
                                                  float* eps, float* z, float* xn_out, float* hn_out) {
  const int ld = 3 + nc;
  const float inv0 = 1.0f / c.nv0, inv1 = 1.0f / c.nv1, sig_cat = sigma_t * c.nv1;
  float lh = 0.f;
  for (int i = r0 + (int)threadIdx.x; i < r1; i += kLossThreads) {
    const float* nr = noise + (size_t)i * ld;
    float* er = eps + (size_t)i * ld;
    float* zr = z + (size_t)i * ld;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float xn = x[3 * i + d] * inv0;
      if (xn_out) xn_out[3 * i + d] = xn;                         // normalize() leaves the normalised batch in the caller's dicts
      const float e = nr[d] - m[d];
      er[d] = e;
      zr[d] = alpha_t * xn + sigma_t * e;
    }
    for (int k = 0; k < nc; ++k) {
      const float hn = (h[(size_t)i * nc + k] - c.nb1) * inv1;
      if (hn_out) hn_out[(size_t)i * nc + k] = hn;
      const float e = nr[3 + k];
      er[3 + k] = e;
      zr[3 + k] = alpha_t * hn + sigma_t * e;
    }
    lh += cat_row(zr + 3, h + (size_t)i * nc, nc, c.nv1, c.nb1, inv1, sig_cat);
  }
  return lh;
}
// rows [r0, r0 + n) of the caller's batch -> rows [o0, o0 + n) of the chunk's arrays, coordinates shifted by mc, mask = j
__device__ __forceinline__ void noise_rows_score(const LossCfg& c, int r0, int n, int o0, int nc, const float* x, const float* h,
                                                 const float* noise, const float (&mc)[3], const float (&m)[3], float alpha_t,
                                                 float sigma_t, float* eps, float* z, long long* mask, int j) {
  const int ld = 3 + nc;
  const float inv0 = 1.0f / c.nv0, inv1 = 1.0f / c.nv1;
  for (int i = (int)threadIdx.x; i < n; i += kLossThreads) {
    const size_t o = (size_t)(o0 + i), src = (size_t)(r0 + i);
    const float* nr = noise + o * ld;
    float* er = eps + o * ld;
    float* zr = z + o * ld;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float xn = x[3 * src + d] * inv0 - mc[d];
      const float e = nr[d] - m[d];
      er[d] = e;
      zr[d] = alpha_t * xn + sigma_t * e;
    }
    for (int k = 0; k < nc; ++k) {
      const float hn = (h[src * nc + k] - c.nb1) * inv1;
      const float e = nr[3 + k];
      er[3 + k] = e;
      zr[3 + k] = alpha_t * hn + sigma_t * e;
    }
    mask[o] = j;
  }
}

// ---- squared-error rows ---------------------------------------------------------------------------------------------------
// this thread's parts of sum (eps - net)^2 over all columns (all) and the coordinates (x) of rows [r0, r1); virt_h: the raw
// one-hot where a virtual atom's coordinates count zero (LossCfg::vnode_idx), or null.  INFO: also the per-row means of
// |net_x|, |net_h| (ax, ah) and, where given, xh_hat = z / alpha_t - net sigma_t / alpha_t (xh_given_zt_and_epsilon).
struct ErrorSums { float all, x, ax, ah; };
template <bool INFO>
__device__ __forceinline__ void error_rows(const LossCfg& c, int r0, int r1, int nc, const float* net, const float* eps,
                                           const float* virt_h, ErrorSums& s, const float* z = nullptr, float alpha_t = 1.0f,
                                           float sigma_t = 0.0f, float* xh_hat = nullptr) {
  const int ld = 3 + nc;
  for (int i = r0 + (int)threadIdx.x; i < r1; i += kLossThreads) {
    const bool virt = virt_h && c.vnode_idx >= 0 && virt_h[(size_t)i * nc + c.vnode_idx] != c.nb1;   // ((one_hot - nb) / nv).bool()
    float sx_ = 0.f, sa = 0.f, mx_ = 0.f, mh = 0.f;
    for (int k = 0; k < ld; ++k) {
      const size_t o = (size_t)i * ld + k;
      const float nt = net[o], d = eps[o] - nt;
      float sq = d * d;
      if (k < 3 && virt) sq = 0.f;
      sa += sq;
      if (k < 3) sx_ += sq;
      if constexpr (INFO) {
        if (k < 3) mx_ += fabsf(nt); else mh += fabsf(nt);
        if (xh_hat) xh_hat[o] = z[o] / alpha_t - nt * sigma_t / alpha_t;
      }
    }
    s.all += sa; s.x += sx_;
    if constexpr (INFO) { s.ax += mx_ / 3.0f; s.ah += mh / (float)nc; }
  }
}

// ---- one element of the error terms' gradient -----------------------------------------------------------------------------
// d net = -2 (eps - net) w - g_hat sigma_t / alpha_t,  w = bwd_weight + bwd_weight_coord on the coordinates
__device__ __forceinline__ float bwd_weight(const float* g_err, int b, float tz) { return (g_err ? g_err[b] : 0.f) * (1.0f - tz); }
__device__ __forceinline__ float bwd_weight_coord(const float* g_l0x, int b, float tz) { return 0.5f * (g_l0x ? g_l0x[b] : 0.f) * tz; }
// g_hat: the element's gradient of xh_hat, or null; sigma_t, alpha_t: the sample's, read only with g_hat
__device__ __forceinline__ float bwd_element(float e, float nt, float w, const float* g_hat, const float* sigma_t, const float* alpha_t) {
  float g = -2.0f * (e - nt) * w;
  if (g_hat) g -= *g_hat * *sigma_t / *alpha_t;
  return g;
}

}  // namespace dsbdd
