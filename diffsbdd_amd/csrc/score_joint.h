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
// The formulas are those of loss_joint_pre_kernel / loss_joint_post_kernel (loss_head.h) and of the evaluation branch of
// the torch mirror, written once in loss_parts.h; every sum is a fixed-order reduction inside the state's workgroup or a
// serial loop, no atomics.  LossCfg::remove_com and ::vnode_idx are not read (the host refuses virtual atoms).
#pragma once
#include "score.h"

namespace dsbdd {

enum { SJ_T = 0, SJ_GAMMA_T, SJ_ALPHA_T, SJ_SIGMA_T, SJ_SNR_W, SJ_ERR_LIG, SJ_ERR_POC, SJ_L0X_LIG, SJ_L0X_POC, SJ_L0_H,
       SJ_ROWS };                                                                                       // per state
static_assert(SJ_T == SS_T && SJ_GAMMA_T == SS_GAMMA_T && SJ_ALPHA_T == SS_ALPHA_T && SJ_SIGMA_T == SS_SIGMA_T && SJ_SNR_W == SS_SNR_W,
              "write_state_scalars");
// per complex: SL_KL, SL_NEG_LOG_C, SL_DELTA_LOG_PX, SL_LOG_PN of score.h
enum { SJO_NLL = 0, SJO_LOSS_T, SJO_LOSS_T_LIG, SJO_L0X_LIG, SJO_L0X_POC, SJO_L0_H, SJO_NEG_LOG_C, SJO_KL, SJO_DELTA_LOG_PX,
       SJO_LOG_PN, SJO_ROWS };

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
  const int l0 = rows.l0, nl = rows.nl, p0 = rows.p0, np = rows.np, ol = rows.ol, op = rows.op;
  const int l1 = l0 + nl, p1 = p0 + np, nn = nl + np;
  const bool zero_slot = rows.k == s.n_slots - 1;
  const float inv0 = 1.0f / c.nv0, inv1 = 1.0f / c.nv1;
  const float cnt = seg_count(nn);
  // the zero slot is the separate pass at t = 0
  const Schedule sc = schedule_at(gamma_table, c.T, zero_slot ? 0.0f : t_int[g]);
  const bool fits = score_rows_fit(s, rows);
  if (t == 0) write_state_scalars(sc, zero_slot, fits, s.n_states, g, j, t_out, ps);
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
  block_mean3(n0, n1, n2, cnt, red, m);
  if (center) block_mean3(c0, c1, c2, cnt, red, mc);

  // 2. centred eps, z = alpha_t xh + sigma_t eps (noised_representation) and the masks of both node sets
  noise_rows_score(c, l0, nl, ol, a, lig_x, lig_h, noise_lig, mc, m, sc.alpha_t, sc.sigma_t, eps_lig, z_lig, mask_l, j);
  noise_rows_score(c, p0, np, op, r, poc_x, poc_h, noise_poc, mc, m, sc.alpha_t, sc.sigma_t, eps_poc, z_poc, mask_p, j);

  // 3. the per-complex terms, once per complex: on its slot 0
  if (rows.k != 0) return;
  const PriorEnds e = prior_ends(gamma_table, c.T);
  // KL sums of the prior (kl_prior_with_pocket: ligand part, then the pocket part added)
  float sxl = 0.f, shl = 0.f, sxp = 0.f, shp = 0.f;
  for (int i = l0 + t; i < l1; i += kLossThreads) kl_row(c, inv0, inv1, lig_x + 3 * i, lig_h + (size_t)i * a, a, mc, e.alpha_T, sxl, shl);
  for (int i = p0 + t; i < p1; i += kLossThreads) kl_row(c, inv0, inv1, poc_x + 3 * i, poc_h + (size_t)i * r, r, mc, e.alpha_T, sxp, shp);
  sxl = block_sum(sxl, red); shl = block_sum(shl, red); sxp = block_sum(sxp, red); shp = block_sum(shp, red);
  if (t == 0) {
    const float dof = joint_dof(nn);
    write_ligand_terms(c, rows.b, dof, e.g_0, kl_prior_rounded(sxl + sxp, shl + shp, e.sigma_T, dof),
                       log_pn_or_nan(c, logpn_table, nl, np), pl);
  }
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
  ErrorSums l{0.f, 0.f, 0.f, 0.f}, p{0.f, 0.f, 0.f, 0.f};
  float lh_l = 0.f, lh_p = 0.f;
  error_rows<false>(c, ol, ol + nl, c.atom_nf, net_lig, eps_lig, nullptr, l);
  error_rows<false>(c, op, op + np, c.residue_nf, net_poc, eps_poc, nullptr, p);
  if (zero_slot) {
    lh_l = cat_rows(c, rows.l0, nl, ol, c.atom_nf, z_lig, lig_h, sig_cat);
    lh_p = cat_rows(c, rows.p0, np, op, c.residue_nf, z_poc, poc_h, sig_cat);
  }
  const float el = block_sum(l.all, red), elx = block_sum(l.x, red), ep = block_sum(p.all, red), epx = block_sum(p.x, red);
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
  static_assert(SJO_KL == SJO_NEG_LOG_C + 1 && SJO_DELTA_LOG_PX == SJO_NEG_LOG_C + 2 && SJO_LOG_PN == SJO_NEG_LOG_C + 3, "out_tail");
  out[SJO_NLL * B + b] = reduce_tail(loss_t, (l0xl + l0xp) + l0h, pl, B, b, out + SJO_NEG_LOG_C * B);
  out[SJO_LOSS_T * B + b] = loss_t; out[SJO_LOSS_T_LIG * B + b] = loss_t_lig;
  out[SJO_L0X_LIG * B + b] = l0xl; out[SJO_L0X_POC * B + b] = l0xp; out[SJO_L0_H * B + b] = l0h;
}

}  // namespace dsbdd
