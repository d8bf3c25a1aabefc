// The model's likelihood bound of GIVEN ligands in their pockets (diffsbdd_amd/score.py: ConditionalDDPM.nll_given_pocket).
//
// The evaluation branch of ConditionalDDPM.forward (conditional_model.py:202-330 of the reference) scores one random time
// per complex with two network calls.  Here every ligand b gets K time slots (integer times t[b][k] in 1..T, weights
// w[b][k]) and one zero slot (t = 0), and all (ligand, slot) STATES of a call are evaluated by few large network calls:
//
//   state g = b * n_slots + k, n_slots = K + 1, k = K is the zero slot (ligand-major, time slots first);
//   a CHUNK is the states [first, first + n): one network call.  A chunk may begin and end inside a ligand's slots.
//   In the chunk's arrays state g owns ligand rows [pref_l(g) - pref_l(first), +nl_b) and pocket rows likewise, with
//   pref_l(g) = n_slots * l0_b + k * nl_b (l0_b = ligand b's first row in the caller's batch): no offset table.
//
//   score_cond_pre_kernel   one workgroup per state of the chunk: reads ligand b and its pocket through g -> b (the inputs
//                           are never repeated in memory), writes the state's z rows, centred pocket rows, the int64 masks
//                           with state-local ids, its t, and gamma_t / alpha_t / sigma_t / SNR_weight; the state that is a
//                           ligand's slot 0 also writes kl_prior, neg_log_constants, delta_log_px, log_pN;
//   score_cond_post_kernel  one workgroup per state: error_t (time slots), loss_0_x and loss_0_h (zero slots);
//   score_reduce_kernel     once per call, one thread per ligand: loss_t = sum_k (k ascending) and the bound.
//
// Formulas and their order are those of loss_cond_pre_kernel / loss_cond_post_kernel (loss_head.h); every sum is a
// fixed-order reduction inside the state's workgroup or a serial loop, no atomics.  Virtual atoms are not supported.
#pragma once
#include "common.h"
#include "ddpm.h"
#include "graph_parts.h"   // lower_bound_i64
#include "loss_head.h"

namespace dsbdd {

enum { SS_T = 0, SS_GAMMA_T, SS_ALPHA_T, SS_SIGMA_T, SS_SNR_W, SS_ERR_T, SS_L0_X, SS_L0_H, SS_ROWS };    // per state
enum { SL_KL = 0, SL_NEG_LOG_C, SL_DELTA_LOG_PX, SL_LOG_PN, SL_ROWS };                                   // per ligand
enum { SO_NLL = 0, SO_LOSS_T, SO_L0_X, SO_L0_H, SO_NEG_LOG_C, SO_KL, SO_DELTA_LOG_PX, SO_LOG_PN, SO_ROWS };

// LossCfg: batch = number of ligands B, n_lig / n_pocket = rows of the caller's batch; vnode_idx is not read
struct ScoreChunk {
  int n_slots;        // K + 1
  int first;          // first state of the chunk
  int n_states;       // B * n_slots
  int cap_lig, cap_pocket;    // rows of the chunk's arrays: a state that would not fit writes nothing but NaN scalars
};

// rows of state g in the caller's batch and in the chunk's arrays
struct ScoreRows { int b, k, l0, nl, p0, np, ol, op; };

__device__ __forceinline__ ScoreRows score_rows_of(const LossCfg& c, const ScoreChunk& s, int g, const long long* lig_mask,
                                                   const long long* poc_mask) {
  ScoreRows r;
  r.b = g / s.n_slots; r.k = g % s.n_slots;
  r.l0 = lower_bound_i64(lig_mask, c.n_lig, r.b); r.nl = lower_bound_i64(lig_mask, c.n_lig, r.b + 1) - r.l0;
  r.p0 = lower_bound_i64(poc_mask, c.n_pocket, r.b); r.np = lower_bound_i64(poc_mask, c.n_pocket, r.b + 1) - r.p0;
  const int bf = s.first / s.n_slots, kf = s.first % s.n_slots;
  const int lf = lower_bound_i64(lig_mask, c.n_lig, bf), nlf = lower_bound_i64(lig_mask, c.n_lig, bf + 1) - lf;
  const int pf = lower_bound_i64(poc_mask, c.n_pocket, bf), npf = lower_bound_i64(poc_mask, c.n_pocket, bf + 1) - pf;
  r.ol = (s.n_slots * r.l0 + r.k * r.nl) - (s.n_slots * lf + kf * nlf);
  r.op = (s.n_slots * r.p0 + r.k * r.np) - (s.n_slots * pf + kf * npf);
  return r;
}

__global__ __launch_bounds__(kLossThreads) void score_cond_pre_kernel(
    LossCfg c, ScoreChunk s, const float* lig_x, const float* lig_h, const long long* lig_mask, const float* poc_x,
    const float* poc_h, const long long* poc_mask, const float* eps, const float* t_int, const float* gamma_table,
    const float* logpn_table, float* z, float* xh_pocket, long long* mask_l, long long* mask_p, float* t_out, float* ps,
    float* pl) {
  __shared__ float red[kLossThreads];
  __shared__ ScoreRows rows;
  const int j = blockIdx.x, t = threadIdx.x, g = s.first + j;
  const int a = c.atom_nf, r = c.residue_nf, ldl = 3 + a, ldp = 3 + r;
  if (t == 0) rows = score_rows_of(c, s, g, lig_mask, poc_mask);
  __syncthreads();
  const int b = rows.b, l0 = rows.l0, nl = rows.nl, p0 = rows.p0, np = rows.np, ol = rows.ol, op = rows.op;
  const int l1 = l0 + nl, p1 = p0 + np, S = s.n_states;
  const bool zero_slot = rows.k == s.n_slots - 1;
  const float inv0 = 1.0f / c.nv0, inv1 = 1.0f / c.nv1;          // normalize(): a division by a python scalar multiplies by its inverse
  const float cnt = (float)(nl > 1 ? nl : 1);                     // seg_mean: count clamped to >= 1

  // per-state scalars (forward(): t, s, gamma; alpha / sigma); the zero slot is the separate pass at t = 0 (:285-302)
  const float ti = zero_slot ? 0.0f : t_int[g];
  const float tt = ti / (float)c.T, ss = (ti - 1.0f) / (float)c.T;
  const float g_t = gamma_at(gamma_table, c.T, tt), g_s = gamma_at(gamma_table, c.T, ss);
  const float alpha_t = sqrtf(sigmoid_ref(-g_t)), sigma_t = sqrtf(sigmoid_ref(g_t));
  const bool fits = ol >= 0 && op >= 0 && ol + nl <= s.cap_lig && op + np <= s.cap_pocket;
  if (t == 0) {
    const float bad = fits ? 0.0f : NAN;
    t_out[j] = tt;
    ps[SS_T * S + g] = tt; ps[SS_GAMMA_T * S + g] = g_t + bad;
    ps[SS_ALPHA_T * S + g] = alpha_t; ps[SS_SIGMA_T * S + g] = sigma_t;
    ps[SS_SNR_W * S + g] = zero_slot ? 0.0f : (1.0f - expf(-(g_s - g_t))) + bad;         // 1 - SNR(gamma_s - gamma_t)
  }
  if (!fits) return;

  // 1. ligand centre of mass of the normalised coordinates (_remove_lig_com)
  float m1[3] = {0.f, 0.f, 0.f};
  if (c.remove_com) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int i = l0 + t; i < l1; i += kLossThreads) { s0 += lig_x[3 * i] * inv0; s1 += lig_x[3 * i + 1] * inv0; s2 += lig_x[3 * i + 2] * inv0; }
    m1[0] = block_sum(s0, red) / cnt; m1[1] = block_sum(s1, red) / cnt; m1[2] = block_sum(s2, red) / cnt;
  }
  // 2. the centre of mass of the noised coordinates (noised_representation)
  float m2[3] = {0.f, 0.f, 0.f};
  if (c.remove_com) {
    float z0 = 0.f, z1 = 0.f, z2 = 0.f;
    for (int i = l0 + t; i < l1; i += kLossThreads) {
      const float* er = eps + (size_t)(ol + i - l0) * ldl;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float x = lig_x[3 * i + d] * inv0 - m1[d];
        const float v = alpha_t * x + sigma_t * er[d];
        if (d == 0) z0 += v; else if (d == 1) z1 += v; else z2 += v;
      }
    }
    m2[0] = block_sum(z0, red) / cnt; m2[1] = block_sum(z1, red) / cnt; m2[2] = block_sum(z2, red) / cnt;
  }
  // 3. z of the state, its mask rows
  for (int i = l0 + t; i < l1; i += kLossThreads) {
    const size_t o = (size_t)(ol + i - l0);
    const float* er = eps + o * ldl;
    float* zr = z + o * ldl;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float x = lig_x[3 * i + d] * inv0 - m1[d];
      zr[d] = (alpha_t * x + sigma_t * er[d]) - m2[d];
    }
    for (int k = 0; k < a; ++k) {
      const float h = (lig_h[(size_t)i * a + k] - c.nb1) * inv1;
      zr[3 + k] = alpha_t * h + sigma_t * er[3 + k];
    }
    mask_l[o] = j;
  }
  // 4. the state's own copy of the pocket: normalised, shifted by both ligand centres
  for (int i = p0 + t; i < p1; i += kLossThreads) {
    const size_t o = (size_t)(op + i - p0);
    float* pr = xh_pocket + o * ldp;
#pragma unroll
    for (int d = 0; d < 3; ++d) pr[d] = ((poc_x[3 * i + d] * inv0) - m1[d]) - m2[d];
    for (int k = 0; k < r; ++k) pr[3 + k] = (poc_h[(size_t)i * r + k] - c.nb1) * inv1;
    mask_p[o] = j;
  }
  // 5. the per-ligand terms, once per ligand: on its slot 0
  if (rows.k != 0) return;
  const float g_T = gamma_table[c.T], g_0 = gamma_table[0];
  const float alpha_T = sqrtf(sigmoid_ref(-g_T)), sigma_T = sqrtf(sigmoid_ref(g_T));
  float sx = 0.f, sh = 0.f;
  for (int i = l0 + t; i < l1; i += kLossThreads) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float x = lig_x[3 * i + d] * inv0 - m1[d];
      const float mu = alpha_T * x;
      sx += mu * mu;
    }
    for (int k = 0; k < a; ++k) {
      const float h = (lig_h[(size_t)i * a + k] - c.nb1) * inv1;
      const float mu = alpha_T * h;
      sh += mu * mu;
    }
  }
  sx = block_sum(sx, red); sh = block_sum(sh, red);
  if (t == 0) {
    const int B = c.batch;
    const float dof = c.remove_com ? (float)((nl - 1) * 3) : (float)(nl * 3);       // subspace_dimensionality
    pl[SL_NEG_LOG_C * B + b] = -(dof * (-(0.5f * g_0) - 0.91893853320467274178f));    // -log_constants_p_x_given_z0
    // gaussian_KL(mu2, sigma_T, 1, d) = d log(1 / sigma_T) + 0.5 (d sigma_T^2 + mu2) - 0.5 d;  d = dof for x, 1 for h
    const float lq = logf(1.0f / sigma_T), q2 = sigma_T * sigma_T;
    const float kl_x = dof * lq + 0.5f * (dof * q2 + sx) - 0.5f * dof;
    const float kl_h = lq + 0.5f * (q2 + sh) - 0.5f;
    pl[SL_KL * B + b] = kl_x + kl_h;
    // log p(N_lig | N_pocket); the host refuses sizes outside the table before any launch (no clamp: NaN here)
    pl[SL_LOG_PN * B + b] = (nl < c.n1_tab && np < c.n2_tab) ? logpn_table[(size_t)nl * c.n2_tab + np] : NAN;
    pl[SL_DELTA_LOG_PX * B + b] = -dof * logf(c.nv0);
  }
}

// after the network call.  Time slots: error_t = sum over the ligand's rows and all 3 + atom_nf columns of (eps - net)^2.
// Zero slots: loss_0_x = 0.5 sum over the coordinates, loss_0_h = - sum of the categorical log-likelihood of z_0
// (_log_ph_given_z0 with gamma_0)
__global__ __launch_bounds__(kLossThreads) void score_cond_post_kernel(
    LossCfg c, ScoreChunk s, const float* lig_h, const long long* lig_mask, const long long* poc_mask, const float* net,
    const float* eps, const float* z, float* ps) {
  __shared__ float red[kLossThreads];
  __shared__ ScoreRows rows;
  const int j = blockIdx.x, t = threadIdx.x, g = s.first + j, a = c.atom_nf, ld = 3 + a, S = s.n_states;
  if (t == 0) rows = score_rows_of(c, s, g, lig_mask, poc_mask);
  __syncthreads();
  const int l0 = rows.l0, nl = rows.nl, ol = rows.ol;
  const bool zero_slot = rows.k == s.n_slots - 1;
  const bool fits = ol >= 0 && rows.op >= 0 && ol + nl <= s.cap_lig && rows.op + rows.np <= s.cap_pocket;
  if (!fits) {
    if (t == 0) { ps[SS_ERR_T * S + g] = NAN; ps[SS_L0_X * S + g] = NAN; ps[SS_L0_H * S + g] = NAN; }
    return;
  }
  const float inv1 = 1.0f / c.nv1, sig_cat = ps[SS_SIGMA_T * S + g] * c.nv1;
  float e_all = 0.f, e_x = 0.f, lh = 0.f;
  for (int i = t; i < nl; i += kLossThreads) {
    const size_t o = (size_t)(ol + i) * ld;
    float sx_ = 0.f, sa = 0.f;
    for (int k = 0; k < ld; ++k) {
      const float d = eps[o + k] - net[o + k];
      const float sq = d * d;
      sa += sq;
      if (k < 3) sx_ += sq;
    }
    e_all += sa; e_x += sx_;
    if (zero_slot) lh += joint_cat_row(z + o + 3, lig_h + (size_t)(l0 + i) * a, a, c.nv1, c.nb1, inv1, sig_cat);
  }
  e_all = block_sum(e_all, red); e_x = block_sum(e_x, red); lh = block_sum(lh, red);
  if (t == 0) {
    ps[SS_ERR_T * S + g] = zero_slot ? 0.0f : e_all;
    ps[SS_L0_X * S + g] = zero_slot ? 0.5f * e_x : 0.0f;
    ps[SS_L0_H * S + g] = zero_slot ? -lh : 0.0f;
  }
}

// loss_t(b) = sum_k w[b][k] (-0.5 SNR_weight error_t)  (k ascending, float32; a term is ((-0.5 w) SNR_weight) error_t, the
// order of lightning_modules.py:262-275 with w = T), then
// nll = loss_t + ((loss_0_x + loss_0_h) + neg_log_constants) + kl_prior - delta_log_px - log_pN, left to right
__global__ void score_reduce_kernel(int B, int n_slots, const float* weights, const float* ps, const float* pl, float* out) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int S = B * n_slots, gz = b * n_slots + n_slots - 1;
  float loss_t = 0.f;
  for (int k = 0; k + 1 < n_slots; ++k) {
    const int g = b * n_slots + k;
    loss_t += ((-0.5f * weights[g]) * ps[SS_SNR_W * S + g]) * ps[SS_ERR_T * S + g];
  }
  const float l0x = ps[SS_L0_X * S + gz], l0h = ps[SS_L0_H * S + gz];
  const float nlc = pl[SL_NEG_LOG_C * B + b], kl = pl[SL_KL * B + b], dlp = pl[SL_DELTA_LOG_PX * B + b], lpn = pl[SL_LOG_PN * B + b];
  const float loss_0 = (l0x + l0h) + nlc;
  out[SO_NLL * B + b] = (((loss_t + loss_0) + kl) - dlp) - lpn;
  out[SO_LOSS_T * B + b] = loss_t;
  out[SO_L0_X * B + b] = l0x; out[SO_L0_H * B + b] = l0h;
  out[SO_NEG_LOG_C * B + b] = nlc; out[SO_KL * B + b] = kl;
  out[SO_DELTA_LOG_PX * B + b] = dlp; out[SO_LOG_PN * B + b] = lpn;
}

}  // namespace dsbdd
