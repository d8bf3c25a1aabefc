// The joint model's likelihood bound of GIVEN ligand-pocket complexes (diffsbdd_amd/score.py:
// EnVariationalDiffusion.nll_of_complex).
//
// The evaluation branch of EnVariationalDiffusion.forward (en_diffusion.py:336-469 of the reference) scores one random
// time per complex with two network calls.  Here, as in score.h for the pocket-conditioned model, every complex b gets K
// time slots and one zero slot, and all (complex, slot) states of a chunk go through one network call.  States, chunks and
// the closed-form row offsets are those of score.h (ScoreChunk, score_rows_of); the joint model noises and scores BOTH
// node sets, so a state owns noised ligand rows AND noised pocket rows in the chunk's arrays.
//
//   score_joint_pre_kernel     one workgroup per state: normalises both node sets (optionally centred at the complex's
//                              mean over ligand + pocket rows: what dataset.py does to every training complex; the joint
//                              forward() itself never centres), centres the state's noise over ligand + pocket rows,
//                              writes eps and z = alpha_t xh + sigma_t eps of both node sets, both int64 masks with
//                              chunk-local state ids, t / T, gamma_t / alpha_t / sigma_t / SNR_weight; the state that is
//                              a complex's slot 0 also writes kl_prior, neg_log_constants, delta_log_px, log_pN;
//   score_joint_post_kernel    one workgroup per state: error_t_lig / error_t_pocket (time slots), loss_0_x_ligand /
//                              loss_0_x_pocket / loss_0_h (zero slots);
//   score_joint_reduce_kernel  once per call, one thread per complex: loss_t = sum_k (k ascending) and the bound.
//
// Formulas and their order are those of loss_joint_pre_kernel / loss_joint_post_kernel (loss_head.h) and of the evaluation
// branch of the torch mirror; every sum is a fixed-order reduction inside the state's workgroup or a serial loop, no
// atomics.  LossCfg::remove_com and ::vnode_idx are not read (the host refuses virtual atoms).
#pragma once
#include "score.h"

namespace dsbdd {

enum { SJ_T = 0, SJ_GAMMA_T, SJ_ALPHA_T, SJ_SIGMA_T, SJ_SNR_W, SJ_ERR_LIG, SJ_ERR_POC, SJ_L0X_LIG, SJ_L0X_POC, SJ_L0_H,
       SJ_ROWS };                                                                                       // per state
// per complex: SL_KL, SL_NEG_LOG_C, SL_DELTA_LOG_PX, SL_LOG_PN of score.h
enum { SJO_NLL = 0, SJO_LOSS_T, SJO_LOSS_T_LIG, SJO_L0X_LIG, SJO_L0X_POC, SJO_L0_H, SJO_NEG_LOG_C, SJO_KL, SJO_DELTA_LOG_PX,
       SJO_LOG_PN, SJO_ROWS };

__device__ __forceinline__ bool score_rows_fit(const ScoreChunk& s, const ScoreRows& r) {
  return r.ol >= 0 && r.op >= 0 && r.ol + r.nl <= s.cap_lig && r.op + r.np <= s.cap_pocket;
}

// one node set of a state: rows [r0, r0 + n) of the caller's batch -> rows [o0, o0 + n) of the chunk's arrays.
// eps = noise with its x part centred by m, z = alpha_t xh + sigma_t eps with xh = the normalised row, its coordinates
// shifted by mc; the mask rows get the chunk-local state id j
__device__ __forceinline__ void score_joint_noise_rows(const LossCfg& c, int r0, int n, int o0, int nc, const float* x,
                                                       const float* h, const float* noise, const float (&mc)[3],
                                                       const float (&m)[3], float alpha_t, float sigma_t, float* eps, float* z,
                                                       long long* mask, int j) {
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
      const float e = nr[d] - m[d];                                 // _joint_noise: zx - seg_mean(zx)[comb]
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

__global__ __launch_bounds__(kLossThreads) void score_joint_pre_kernel(
    LossCfg c, ScoreChunk s, int center, const float* lig_x, const float* lig_h, const long long* lig_mask, const float* poc_x,
    const float* poc_h, const long long* poc_mask, const float* noise_lig, const float* noise_poc, const float* t_int,
    const float* gamma_table, const float* logpn_table, float* eps_lig, float* eps_poc, float* z_lig, float* z_poc,
    long long* mask_l, long long* mask_p, float* t_out, float* ps, float* pl) {
  __shared__ float red[kLossThreads];
  __shared__ ScoreRows rows;
  const int j = blockIdx.x, t = threadIdx.x, g = s.first + j;
  const int a = c.atom_nf, r = c.residue_nf, ldl = 3 + a, ldp = 3 + r;
  if (t == 0) rows = score_rows_of(c, s, g, lig_mask, poc_mask);
  __syncthreads();
  const int b = rows.b, l0 = rows.l0, nl = rows.nl, p0 = rows.p0, np = rows.np, ol = rows.ol, op = rows.op;
  const int l1 = l0 + nl, p1 = p0 + np, nn = nl + np, S = s.n_states;
  const bool zero_slot = rows.k == s.n_slots - 1;
  const float inv0 = 1.0f / c.nv0, inv1 = 1.0f / c.nv1;
  const float cnt = (float)(nn > 1 ? nn : 1);                     // seg_mean: count clamped to >= 1

  // per-state scalars (forward(): t, s, gamma; alpha / sigma); the zero slot is the separate pass at t = 0
  const float ti = zero_slot ? 0.0f : t_int[g];
  const float tt = ti / (float)c.T, ss = (ti - 1.0f) / (float)c.T;
  const float g_t = gamma_at(gamma_table, c.T, tt), g_s = gamma_at(gamma_table, c.T, ss);
  const float alpha_t = sqrtf(sigmoid_ref(-g_t)), sigma_t = sqrtf(sigmoid_ref(g_t));
  const bool fits = score_rows_fit(s, rows);
  if (t == 0) {
    const float bad = fits ? 0.0f : NAN;
    t_out[j] = tt;
    ps[SJ_T * S + g] = tt; ps[SJ_GAMMA_T * S + g] = g_t + bad;
    ps[SJ_ALPHA_T * S + g] = alpha_t; ps[SJ_SIGMA_T * S + g] = sigma_t;
    ps[SJ_SNR_W * S + g] = zero_slot ? 0.0f : (1.0f - expf(-(g_s - g_t))) + bad;         // 1 - SNR(gamma_s - gamma_t)
  }
  if (!fits) return;

  // 1. the complex's mean of the normalised coordinates over ligand + pocket rows (ligand rows first), and the centre of
  //    the state's noise x part over the same rows (_joint_noise)
  float c0 = 0.f, c1 = 0.f, c2 = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
  for (int i = l0 + t; i < l1; i += kLossThreads) {
    const float* nr = noise_lig + (size_t)(ol + i - l0) * ldl;
    n0 += nr[0]; n1 += nr[1]; n2 += nr[2];
    c0 += lig_x[3 * i] * inv0; c1 += lig_x[3 * i + 1] * inv0; c2 += lig_x[3 * i + 2] * inv0;
  }
  for (int i = p0 + t; i < p1; i += kLossThreads) {
    const float* nr = noise_poc + (size_t)(op + i - p0) * ldp;
    n0 += nr[0]; n1 += nr[1]; n2 += nr[2];
    c0 += poc_x[3 * i] * inv0; c1 += poc_x[3 * i + 1] * inv0; c2 += poc_x[3 * i + 2] * inv0;
  }
  float m[3], mc[3] = {0.f, 0.f, 0.f};
  m[0] = block_sum(n0, red) / cnt; m[1] = block_sum(n1, red) / cnt; m[2] = block_sum(n2, red) / cnt;
  if (center) { mc[0] = block_sum(c0, red) / cnt; mc[1] = block_sum(c1, red) / cnt; mc[2] = block_sum(c2, red) / cnt; }

  // 2. centred eps, z = alpha_t xh + sigma_t eps (noised_representation) and the masks of both node sets
  score_joint_noise_rows(c, l0, nl, ol, a, lig_x, lig_h, noise_lig, mc, m, alpha_t, sigma_t, eps_lig, z_lig, mask_l, j);
  score_joint_noise_rows(c, p0, np, op, r, poc_x, poc_h, noise_poc, mc, m, alpha_t, sigma_t, eps_poc, z_poc, mask_p, j);

  // 3. the per-complex terms, once per complex: on its slot 0
  if (rows.k != 0) return;
  const float g_T = gamma_table[c.T], g_0 = gamma_table[0];
  const float alpha_T = sqrtf(sigmoid_ref(-g_T)), sigma_T = sqrtf(sigmoid_ref(g_T));
  // KL sums of the prior (kl_prior_with_pocket: ligand part, then the pocket part added)
  float sxl = 0.f, shl = 0.f, sxp = 0.f, shp = 0.f;
  for (int i = l0 + t; i < l1; i += kLossThreads) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { const float mu = alpha_T * (lig_x[3 * i + d] * inv0 - mc[d]); sxl += mu * mu; }
    for (int k = 0; k < a; ++k) { const float mu = alpha_T * ((lig_h[(size_t)i * a + k] - c.nb1) * inv1); shl += mu * mu; }
  }
  for (int i = p0 + t; i < p1; i += kLossThreads) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { const float mu = alpha_T * (poc_x[3 * i + d] * inv0 - mc[d]); sxp += mu * mu; }
    for (int k = 0; k < r; ++k) { const float mu = alpha_T * ((poc_h[(size_t)i * r + k] - c.nb1) * inv1); shp += mu * mu; }
  }
  sxl = block_sum(sxl, red); shl = block_sum(shl, red); sxp = block_sum(sxp, red); shp = block_sum(shp, red);
  if (t == 0) {
    const int B = c.batch;
    const float sx = sxl + sxp, sh = shl + shp;
    const float dof = (float)((nn - 1) * 3);                                          // subspace_dimensionality(n_lig + n_pocket)
    pl[SL_NEG_LOG_C * B + b] = -(dof * (-(0.5f * g_0) - 0.91893853320467274178f));    // -log_constants_p_x_given_z0
    pl[SL_KL * B + b] = joint_gaussian_kl(sx, sigma_T, dof) + joint_gaussian_kl(sh, sigma_T, 1.0f);
    // log p(N_lig, N_pocket); the host refuses sizes outside the table before any launch (no clamp: NaN here)
    pl[SL_LOG_PN * B + b] = (nl < c.n1_tab && np < c.n2_tab) ? logpn_table[(size_t)nl * c.n2_tab + np] : NAN;
    pl[SL_DELTA_LOG_PX * B + b] = -dof * logf(c.nv0);
  }
}

// this thread's part of sum log p(h | z_0) over the n rows of one node set (rows [o0, o0 + n) of the chunk's z, rows
// [r0, r0 + n) of the caller's one-hot)
__device__ __forceinline__ float score_joint_cat_rows(const LossCfg& c, int r0, int n, int o0, int nc, const float* z,
                                                      const float* h, float sig_cat) {
  const float inv1 = 1.0f / c.nv1;
  float lh = 0.f;
  for (int i = (int)threadIdx.x; i < n; i += kLossThreads)
    lh += joint_cat_row(z + (size_t)(o0 + i) * (3 + nc) + 3, h + (size_t)(r0 + i) * nc, nc, c.nv1, c.nb1, inv1, sig_cat);
  return lh;
}

// after the network call.  Time slots: error_t_lig / error_t_pocket = sum over the node set's rows and all its columns of
// (eps - net)^2.  Zero slots: loss_0_x_* = 0.5 sum over the coordinates, loss_0_h = - (sum_lig + sum_pocket) of the
// categorical log-likelihood of z_0 (_log_ph_given_z0 with gamma_0)
__global__ __launch_bounds__(kLossThreads) void score_joint_post_kernel(
    LossCfg c, ScoreChunk s, const float* lig_h, const long long* lig_mask, const float* poc_h, const long long* poc_mask,
    const float* net_lig, const float* net_poc, const float* eps_lig, const float* eps_poc, const float* z_lig,
    const float* z_poc, float* ps) {
  __shared__ float red[kLossThreads];
  __shared__ ScoreRows rows;
  const int j = blockIdx.x, t = threadIdx.x, g = s.first + j, S = s.n_states;
  if (t == 0) rows = score_rows_of(c, s, g, lig_mask, poc_mask);
  __syncthreads();
  const int ol = rows.ol, op = rows.op, nl = rows.nl, np = rows.np;
  const bool zero_slot = rows.k == s.n_slots - 1;
  if (!score_rows_fit(s, rows)) {
    if (t == 0)
      for (int q = SJ_ERR_LIG; q <= SJ_L0_H; ++q) ps[q * S + g] = NAN;
    return;
  }
  const float sig_cat = ps[SJ_SIGMA_T * S + g] * c.nv1;
  float el = 0.f, elx = 0.f, ep = 0.f, epx = 0.f, unused0 = 0.f, unused1 = 0.f, lh_l = 0.f, lh_p = 0.f;
  joint_error_rows(ol, ol + nl, c.atom_nf, net_lig, eps_lig, nullptr, 1.0f, 0.0f, nullptr, el, elx, unused0, unused1);
  joint_error_rows(op, op + np, c.residue_nf, net_poc, eps_poc, nullptr, 1.0f, 0.0f, nullptr, ep, epx, unused0, unused1);
  if (zero_slot) {
    lh_l = score_joint_cat_rows(c, rows.l0, nl, ol, c.atom_nf, z_lig, lig_h, sig_cat);
    lh_p = score_joint_cat_rows(c, rows.p0, np, op, c.residue_nf, z_poc, poc_h, sig_cat);
  }
  el = block_sum(el, red); elx = block_sum(elx, red); ep = block_sum(ep, red); epx = block_sum(epx, red);
  lh_l = block_sum(lh_l, red); lh_p = block_sum(lh_p, red);
  if (t == 0) {
    ps[SJ_ERR_LIG * S + g] = zero_slot ? 0.0f : el;
    ps[SJ_ERR_POC * S + g] = zero_slot ? 0.0f : ep;
    ps[SJ_L0X_LIG * S + g] = zero_slot ? 0.5f * elx : 0.0f;
    ps[SJ_L0X_POC * S + g] = zero_slot ? 0.5f * epx : 0.0f;
    ps[SJ_L0_H * S + g] = zero_slot ? -(lh_l + lh_p) : 0.0f;
  }
}

// loss_t(b) = sum_k ((-0.5 w[b][k]) SNR_weight) (error_t_lig + error_t_pocket)  (k ascending, float32: the order of
// lightning_modules.py:262-275 with w = T), loss_t_lig the same sum over error_t_lig alone, then
// nll = (((loss_t + (((loss_0_x_ligand + loss_0_x_pocket) + loss_0_h) + neg_log_constants)) + kl_prior) - delta_log_px) - log_pN
__global__ void score_joint_reduce_kernel(int B, int n_slots, const float* weights, const float* ps, const float* pl,
                                          float* out) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int S = B * n_slots, gz = b * n_slots + n_slots - 1;
  float loss_t = 0.f, loss_t_lig = 0.f;
  for (int k = 0; k + 1 < n_slots; ++k) {
    const int g = b * n_slots + k;
    const float coef = (-0.5f * weights[g]) * ps[SJ_SNR_W * S + g];
    const float e_l = ps[SJ_ERR_LIG * S + g], e_p = ps[SJ_ERR_POC * S + g];
    loss_t += coef * (e_l + e_p);
    loss_t_lig += coef * e_l;
  }
  const float l0xl = ps[SJ_L0X_LIG * S + gz], l0xp = ps[SJ_L0X_POC * S + gz], l0h = ps[SJ_L0_H * S + gz];
  const float nlc = pl[SL_NEG_LOG_C * B + b], kl = pl[SL_KL * B + b], dlp = pl[SL_DELTA_LOG_PX * B + b], lpn = pl[SL_LOG_PN * B + b];
  const float loss_0 = ((l0xl + l0xp) + l0h) + nlc;
  out[SJO_NLL * B + b] = (((loss_t + loss_0) + kl) - dlp) - lpn;
  out[SJO_LOSS_T * B + b] = loss_t; out[SJO_LOSS_T_LIG * B + b] = loss_t_lig;
  out[SJO_L0X_LIG * B + b] = l0xl; out[SJO_L0X_POC * B + b] = l0xp; out[SJO_L0_H * B + b] = l0h;
  out[SJO_NEG_LOG_C * B + b] = nlc; out[SJO_KL * B + b] = kl;
  out[SJO_DELTA_LOG_PX * B + b] = dlp; out[SJO_LOG_PN * B + b] = lpn;
}

}  // namespace dsbdd
