// The loss terms of the pocket-conditioned training step around the network call, as three launches (round 6).
//
// ConditionalDDPM.forward (conditional_model.py:202-330 of the reference; diffsbdd_amd/conditional_model.py mirrors it in
// torch) normalises the batch, removes the ligand's centre of mass, noises the ligand (z_t = alpha_t xh0 + sigma_t eps,
// centred again), evaluates the network, and returns twelve per-sample terms.  In torch that is ~ 250 launches of a few
// microseconds around a 10-ms step -- 0.8 ms of GPU time in launch gaps (profiles/r6l_*).  Here:
//
//   loss_cond_pre_kernel   one workgroup per sample: normalisation, both centrings, z_t, the centred pocket, and every
//                          term that does not read the network's output: SNR weight, -log Z of p(x | z0), KL of the prior,
//                          the categorical likelihood term L0_h of z_t (training mode evaluates it on z_t), log p(N_lig |
//                          N_pocket), delta log p(x);
//   loss_cond_post_kernel  the squared-error terms (error_t, L0_x), xh_hat, the two logged means;
//   loss_cond_post_bwd_kernel  their gradient w.r.t. the network's output.
//
// Every per-sample sum is a fixed-order reduction inside the sample's workgroup (torch: index_add_ with atomics).
// Formulas and their order follow the torch mirror line by line; they are written once, in loss_parts.h, for these kernels
// and the score kernels (score.h, score_joint.h), and a kernel here is the sequence of those steps over its own rows.
// tests/test_gpu_train.py compares all twelve terms and the parameter gradients between the two paths, and
// tests/test_gpu_loss_head_kernels.py drives each of the six kernels alone through the C ABI against a float64 restatement
// of the header's contract (tests/_loss64.py, pinned to the oracle by tests/test_loss_restatement.py).
//
// The joint model (EnVariationalDiffusion.forward, diffsbdd_amd/en_diffusion.py) has the same three launches further down:
// loss_joint_pre_kernel / loss_joint_post_kernel / loss_joint_post_bwd_kernel (tests/test_gpu_joint_loss_head.py).
#pragma once
#include "loss_parts.h"    // LossCfg, kLossThreads and every formula

namespace dsbdd {

enum {
  LS_T = 0, LS_GAMMA_T, LS_GAMMA_S, LS_ALPHA_T, LS_SIGMA_T, LS_SNR_W, LS_NEG_LOG_C, LS_KL, LS_L0_H, LS_LOG_PN, LS_DELTA_LOG_PX,
  LS_T_IS_ZERO, LS_ROWS
};
enum { LO_ERR_T = 0, LO_L0_X, LO_INFO_X, LO_INFO_H, LO_ROWS };

// engine.edge_capacity in one launch: out[0] = the masks are sorted ascending with ids in [0, batch), out[1] = sum over the
// samples of the complete graph's edges with every (sample, node set) segment rounded up to 32 (csrc/radius_graph.h).  One
// workgroup; ~ 25 torch launches (two bincounts, the comparisons, their reductions) before every training forward otherwise.
__global__ __launch_bounds__(kLossThreads) void edge_capacity_kernel(const long long* ml, int n_l, const long long* mp, int n_p,
                                                                      int batch, long long* out) {
  __shared__ long long cap_s[kLossThreads];
  __shared__ int ok_s[kLossThreads];
  const int t = threadIdx.x;
  int ok = 1;
  for (int i = t; i + 1 < n_l; i += kLossThreads) ok &= ml[i + 1] >= ml[i];
  for (int i = t; i + 1 < n_p; i += kLossThreads) ok &= mp[i + 1] >= mp[i];
  if (t == 0) {
    if (n_l > 0) ok &= ml[0] >= 0 && ml[n_l - 1] < batch;
    if (n_p > 0) ok &= mp[0] >= 0 && mp[n_p - 1] < batch;
  }
  long long cap = 0;
  for (int b = t; b < batch; b += kLossThreads) {
    const long long nl = lower_bound_i64(ml, n_l, b + 1) - lower_bound_i64(ml, n_l, b);
    const long long np = lower_bound_i64(mp, n_p, b + 1) - lower_bound_i64(mp, n_p, b);
    const long long n = nl + np;
    cap += (nl * n + 31) / 32 * 32 + (np * n + 31) / 32 * 32;
  }
  cap_s[t] = cap; ok_s[t] = ok;
  __syncthreads();
  for (int o = kLossThreads / 2; o > 0; o >>= 1) {
    if (t < o) { cap_s[t] += cap_s[t + o]; ok_s[t] &= ok_s[t + o]; }
    __syncthreads();
  }
  if (t == 0) { out[0] = ok_s[0]; out[1] = cap_s[0]; }
}

// the twelve per-sample rows of a pre kernel (one thread); lh = sum log p(h | z_t) over the sample's noised rows
__device__ __forceinline__ void write_sample_terms(const LossCfg& c, int b, float ti, const Schedule& s, float g_0, float dof,
                                                   float kl, float lh, float lpn, float* ps) {
  const int B = c.batch;
  const float tz = ti == 0.0f ? 1.0f : 0.0f;
  ps[LS_T * B + b] = s.tt; ps[LS_GAMMA_T * B + b] = s.g_t; ps[LS_GAMMA_S * B + b] = s.g_s;
  ps[LS_ALPHA_T * B + b] = s.alpha_t; ps[LS_SIGMA_T * B + b] = s.sigma_t;
  ps[LS_SNR_W * B + b] = snr_weight(s); ps[LS_NEG_LOG_C * B + b] = neg_log_constants(dof, g_0);
  ps[LS_KL * B + b] = kl; ps[LS_L0_H * B + b] = -lh * tz;
  ps[LS_LOG_PN * B + b] = lpn; ps[LS_DELTA_LOG_PX * B + b] = delta_log_px(dof, c.nv0);
  ps[LS_T_IS_ZERO * B + b] = tz;
}

__global__ __launch_bounds__(kLossThreads) void loss_cond_pre_kernel(
    LossCfg c, const float* lig_x, const float* lig_h, const long long* lig_mask, const float* poc_x, const float* poc_h,
    const long long* poc_mask, const float* eps, const float* t_int, const float* gamma_table, const float* logpn_table,
    float* z_t, float* xh_pocket, float* ps, float* lig_xn, float* lig_hn, float* poc_xn, float* poc_hn) {
  __shared__ float red[kLossThreads];
  __shared__ int seg[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const int a = c.atom_nf, r = c.residue_nf, ldl = 3 + a, ldp = 3 + r;
  const SampleRows rows = rows_by_thread0(lig_mask, c.n_lig, poc_mask, c.n_pocket, b, seg);
  const int l0 = rows.l0, l1 = rows.l1, p0 = rows.p0, p1 = rows.p1;
  const float inv0 = 1.0f / c.nv0, inv1 = 1.0f / c.nv1;          // normalize(): a division by a python scalar multiplies by its inverse
  const float cnt = seg_count(l1 - l0);
  const float ti = t_int[b];
  const Schedule s = schedule_at(gamma_table, c.T, ti);
  const PriorEnds e = prior_ends(gamma_table, c.T);

  // 1. ligand centre of mass of the normalised coordinates (_remove_lig_com)
  float m1[3];
  cond_lig_centre(c, inv0, lig_x, l0, l1, cnt, red, m1);
  // 2. KL sums of the prior (kl_row's formulas) and the centre of mass of the noised coordinates (pass 2 of
  //    score_cond_pre_kernel) in one pass.  Written out in both: which products of the three coordinates get paired and
  //    fused follows the surrounding statements (profiles/loss_parts.md)
  float sx = 0.f, sh = 0.f, z0 = 0.f, z1 = 0.f, z2 = 0.f;
  for (int i = l0 + t; i < l1; i += kLossThreads) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float x = lig_x[3 * i + d] * inv0 - m1[d];
      const float mu = e.alpha_T * x;
      sx += mu * mu;
      const float z = s.alpha_t * x + s.sigma_t * eps[(size_t)i * ldl + d];
      if (d == 0) z0 += z; else if (d == 1) z1 += z; else z2 += z;
    }
    for (int k = 0; k < a; ++k) {
      const float h = (lig_h[(size_t)i * a + k] - c.nb1) * inv1;
      const float mu = e.alpha_T * h;
      sh += mu * mu;
    }
  }
  sx = block_sum(sx, red); sh = block_sum(sh, red);
  float m2[3] = {0.f, 0.f, 0.f};
  if (c.remove_com) block_mean3(z0, z1, z2, cnt, red, m2);

  // 3. z_t and the categorical term -log p(h | z_t) (_log_ph_given_z0 on z_t: training mode, conditional_model.py:285-302)
  const float sig_cat = s.sigma_t * c.nv1;
  float lh = 0.f;
  for (int i = l0 + t; i < l1; i += kLossThreads) {
    float* zr = z_t + (size_t)i * ldl;
    const float mx = cond_z_row<true>(c, inv0, inv1, lig_x + 3 * i, lig_h + (size_t)i * a, eps + (size_t)i * ldl, a, m1, m2, s.alpha_t,
                                      s.sigma_t, zr, lig_xn ? lig_xn + 3 * i : nullptr, lig_hn ? lig_hn + (size_t)i * a : nullptr);
    cat_row_add(zr + 3, lig_h + (size_t)i * a, a, c.nv1, c.nb1, inv1, sig_cat, mx, lh);
  }
  lh = block_sum(lh, red);
  // 4. the pocket: normalised, shifted by both ligand centres
  for (int i = p0 + t; i < p1; i += kLossThreads)
    cond_pocket_row(c, inv0, inv1, poc_x + 3 * i, poc_h + (size_t)i * r, r, m1, m2, xh_pocket + (size_t)i * ldp,
                    poc_xn ? poc_xn + 3 * i : nullptr, poc_hn ? poc_hn + (size_t)i * r : nullptr);
  if (t == 0) {
    const float dof = cond_dof(c, l1 - l0);
    write_sample_terms(c, b, ti, s, e.g_0, dof, kl_prior_contracted(sx, sh, e.sigma_T, dof), lh,
                       log_pn_clamped(c, logpn_table, l1 - l0, p1 - p0), ps);
  }
}

// error terms after the network call: error_t = sum (eps - net)^2 (x (1 - [t = 0])), L0_x = 0.5 sum over the coordinates
// (x [t = 0]), xh_hat = z_t / alpha_t - net sigma_t / alpha_t, and the logged per-sample means of |net|
__global__ __launch_bounds__(kLossThreads) void loss_cond_post_kernel(
    LossCfg c, const float* net, const float* eps, const float* z_t, const float* lig_h, const long long* lig_mask,
    const float* ps, float* xh_hat, float* out) {
  __shared__ float red[kLossThreads];
  __shared__ int seg[2];
  const int b = blockIdx.x, t = threadIdx.x, B = c.batch;
  if (t == 0) { seg[0] = lower_bound_i64(lig_mask, c.n_lig, b); seg[1] = lower_bound_i64(lig_mask, c.n_lig, b + 1); }
  __syncthreads();
  const int l0 = seg[0], l1 = seg[1];
  const float alpha_t = ps[LS_ALPHA_T * B + b], sigma_t = ps[LS_SIGMA_T * B + b], tz = ps[LS_T_IS_ZERO * B + b];
  ErrorSums e{0.f, 0.f, 0.f, 0.f};
  error_rows<true>(c, l0, l1, c.atom_nf, net, eps, lig_h, e, z_t, alpha_t, sigma_t, xh_hat);
  e.all = block_sum(e.all, red); e.x = block_sum(e.x, red); e.ax = block_sum(e.ax, red); e.ah = block_sum(e.ah, red);
  if (t == 0) {
    const float cnt = seg_count(l1 - l0);
    out[LO_ERR_T * B + b] = e.all * (1.0f - tz); out[LO_L0_X * B + b] = (0.5f * e.x) * tz;
    out[LO_INFO_X * B + b] = e.ax / cnt; out[LO_INFO_H * B + b] = e.ah / cnt;
  }
}

// d net = -2 (eps - net) [g_err (1 - tz) + 0.5 g_l0x tz on the coordinates] (zero on the coordinates of virtual atoms)
//         - g_hat sigma_t / alpha_t
__global__ __launch_bounds__(kLossThreads) void loss_cond_post_bwd_kernel(
    LossCfg c, const float* net, const float* eps, const float* lig_h, const long long* lig_mask, const float* ps,
    const float* g_err, const float* g_l0x, const float* g_hat, float* d_net) {
  const int a = c.atom_nf, ld = 3 + a, B = c.batch;
  const size_t n = (size_t)c.n_lig * ld;
  for (size_t o = (size_t)blockIdx.x * kLossThreads + threadIdx.x; o < n; o += (size_t)gridDim.x * kLossThreads) {
    const int i = (int)(o / ld), k = (int)(o % ld);
    const int b = (int)lig_mask[i];
    const float tz = ps[LS_T_IS_ZERO * B + b];
    float w = bwd_weight(g_err, b, tz);
    if (k < 3) {
      w += bwd_weight_coord(g_l0x, b, tz);
      if (c.vnode_idx >= 0 && lig_h[(size_t)i * a + c.vnode_idx] != c.nb1) w = 0.f;
    }
    d_net[o] = bwd_element(eps[o], net[o], w, g_hat ? g_hat + o : nullptr, ps + LS_SIGMA_T * B + b, ps + LS_ALPHA_T * B + b);
  }
}

// ---- the joint model (EnVariationalDiffusion.forward, training mode; en_diffusion.py:336-469 of the reference) -----------
// Same three launches for the model that diffuses ligand and pocket together: both node sets are noised, both have error
// and L0_x terms, the noise (not the data) is centred over the sample's ligand + pocket rows, and there is neither a
// centre-of-mass projection of the data nor a virtual-atom mask (LossCfg::remove_com and ::vnode_idx are not read).
enum { LJ_ERR_LIG = 0, LJ_ERR_POC, LJ_L0X_LIG, LJ_L0X_POC, LJ_INFO_LIG_X, LJ_INFO_LIG_H, LJ_INFO_POC_X, LJ_INFO_POC_H, LJ_ROWS };

__global__ __launch_bounds__(kLossThreads) void loss_joint_pre_kernel(
    LossCfg c, const float* lig_x, const float* lig_h, const long long* lig_mask, const float* poc_x, const float* poc_h,
    const long long* poc_mask, const float* noise_lig, const float* noise_poc, const float* t_int, const float* gamma_table,
    const float* logpn_table, float* eps_lig, float* eps_poc, float* z_lig, float* z_poc, float* ps, float* lig_xn,
    float* lig_hn, float* poc_xn, float* poc_hn) {
  __shared__ float red[kLossThreads];
  __shared__ int seg[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const int a = c.atom_nf, r = c.residue_nf, ldl = 3 + a, ldp = 3 + r;
  const SampleRows rows = rows_by_thread0(lig_mask, c.n_lig, poc_mask, c.n_pocket, b, seg);
  const int l0 = rows.l0, l1 = rows.l1, p0 = rows.p0, p1 = rows.p1;
  const int nl = l1 - l0, np = p1 - p0, nn = nl + np;
  const float inv0 = 1.0f / c.nv0, inv1 = 1.0f / c.nv1;
  const float ti = t_int[b];
  const Schedule s = schedule_at(gamma_table, c.T, ti);
  const PriorEnds e = prior_ends(gamma_table, c.T);

  // 1. centre of the noise's x part over ligand + pocket rows (_joint_noise) and the KL sums of the prior
  //    (kl_prior_with_pocket: ligand part, then the pocket part added), one pass; the data is not centred
  const float mc[3] = {0.f, 0.f, 0.f};
  float n0 = 0.f, n1 = 0.f, n2 = 0.f, sxl = 0.f, shl = 0.f, sxp = 0.f, shp = 0.f;
  for (int i = l0 + t; i < l1; i += kLossThreads) {
    n0 += noise_lig[(size_t)i * ldl]; n1 += noise_lig[(size_t)i * ldl + 1]; n2 += noise_lig[(size_t)i * ldl + 2];
    kl_row(c, inv0, inv1, lig_x + 3 * i, lig_h + (size_t)i * a, a, mc, e.alpha_T, sxl, shl);
  }
  for (int i = p0 + t; i < p1; i += kLossThreads) {
    n0 += noise_poc[(size_t)i * ldp]; n1 += noise_poc[(size_t)i * ldp + 1]; n2 += noise_poc[(size_t)i * ldp + 2];
    kl_row(c, inv0, inv1, poc_x + 3 * i, poc_h + (size_t)i * r, r, mc, e.alpha_T, sxp, shp);
  }
  float m[3];
  block_mean3(n0, n1, n2, seg_count(nn), red, m);
  sxl = block_sum(sxl, red); shl = block_sum(shl, red); sxp = block_sum(sxp, red); shp = block_sum(shp, red);

  // 2. centred eps, z_t = alpha_t xh + sigma_t eps (noised_representation), the normalised batch, and the categorical
  //    term -log p(h | z_t) of both node sets (loss0 on z_t: training mode, en_diffusion.py:413-424)
  float lh_l = noise_rows_train(c, l0, l1, a, lig_x, lig_h, noise_lig, m, s.alpha_t, s.sigma_t, eps_lig, z_lig, lig_xn, lig_hn);
  float lh_p = noise_rows_train(c, p0, p1, r, poc_x, poc_h, noise_poc, m, s.alpha_t, s.sigma_t, eps_poc, z_poc, poc_xn, poc_hn);
  lh_l = block_sum(lh_l, red); lh_p = block_sum(lh_p, red);
  if (t == 0) {
    const float dof = joint_dof(nn);
    write_sample_terms(c, b, ti, s, e.g_0, dof, kl_prior_rounded(sxl + sxp, shl + shp, e.sigma_T, dof), lh_l + lh_p,
                       log_pn_clamped(c, logpn_table, nl, np), ps);
  }
}

__global__ __launch_bounds__(kLossThreads) void loss_joint_post_kernel(
    LossCfg c, const float* net_lig, const float* net_poc, const float* eps_lig, const float* eps_poc, const float* z_lig,
    const long long* lig_mask, const long long* poc_mask, const float* ps, float* xh_lig_hat, float* out) {
  __shared__ float red[kLossThreads];
  __shared__ int seg[4];
  const int b = blockIdx.x, t = threadIdx.x, B = c.batch;
  const SampleRows rows = rows_by_thread0(lig_mask, c.n_lig, poc_mask, c.n_pocket, b, seg);
  const float alpha_t = ps[LS_ALPHA_T * B + b], sigma_t = ps[LS_SIGMA_T * B + b], tz = ps[LS_T_IS_ZERO * B + b];
  ErrorSums l{0.f, 0.f, 0.f, 0.f}, p{0.f, 0.f, 0.f, 0.f};
  error_rows<true>(c, rows.l0, rows.l1, c.atom_nf, net_lig, eps_lig, nullptr, l, z_lig, alpha_t, sigma_t, xh_lig_hat);
  error_rows<true>(c, rows.p0, rows.p1, c.residue_nf, net_poc, eps_poc, nullptr, p);
  l.all = block_sum(l.all, red); l.x = block_sum(l.x, red); l.ax = block_sum(l.ax, red); l.ah = block_sum(l.ah, red);
  p.all = block_sum(p.all, red); p.x = block_sum(p.x, red); p.ax = block_sum(p.ax, red); p.ah = block_sum(p.ah, red);
  if (t == 0) {
    const float cl = seg_count(rows.l1 - rows.l0), cp = seg_count(rows.p1 - rows.p0);
    out[LJ_ERR_LIG * B + b] = l.all * (1.0f - tz); out[LJ_ERR_POC * B + b] = p.all * (1.0f - tz);
    out[LJ_L0X_LIG * B + b] = (0.5f * l.x) * tz; out[LJ_L0X_POC * B + b] = (0.5f * p.x) * tz;
    out[LJ_INFO_LIG_X * B + b] = l.ax / cl; out[LJ_INFO_LIG_H * B + b] = l.ah / cl;
    out[LJ_INFO_POC_X * B + b] = p.ax / cp; out[LJ_INFO_POC_H * B + b] = p.ah / cp;
  }
}

// d net = -2 (eps - net) [g_err (1 - tz) + 0.5 g_l0x tz on the coordinates] per node set; the ligand also gets
// - g_hat sigma_t / alpha_t (the gradient of xh_lig_hat: the LJ term).  One grid-stride loop over both outputs.
__global__ __launch_bounds__(kLossThreads) void loss_joint_post_bwd_kernel(
    LossCfg c, const float* net_lig, const float* net_poc, const float* eps_lig, const float* eps_poc,
    const long long* lig_mask, const long long* poc_mask, const float* ps, const float* g_err_lig, const float* g_err_poc,
    const float* g_l0x_lig, const float* g_l0x_poc, const float* g_hat, float* d_net_lig, float* d_net_poc) {
  const int ldl = 3 + c.atom_nf, ldp = 3 + c.residue_nf, B = c.batch;
  const size_t n_l = (size_t)c.n_lig * ldl, n = n_l + (size_t)c.n_pocket * ldp;
  for (size_t q = (size_t)blockIdx.x * kLossThreads + threadIdx.x; q < n; q += (size_t)gridDim.x * kLossThreads) {
    const bool lig = q < n_l;
    const size_t o = lig ? q : q - n_l;
    const int ld = lig ? ldl : ldp;
    const int i = (int)(o / ld), k = (int)(o % ld);
    const int b = (int)(lig ? lig_mask[i] : poc_mask[i]);
    const float tz = ps[LS_T_IS_ZERO * B + b];
    float w = bwd_weight(lig ? g_err_lig : g_err_poc, b, tz);
    if (k < 3) w += bwd_weight_coord(lig ? g_l0x_lig : g_l0x_poc, b, tz);
    (lig ? d_net_lig : d_net_poc)[o] = bwd_element(lig ? eps_lig[o] : eps_poc[o], lig ? net_lig[o] : net_poc[o], w,
                                                   lig && g_hat ? g_hat + o : nullptr, ps + LS_SIGMA_T * B + b,
                                                   ps + LS_ALPHA_T * B + b);
  }
}

}  // namespace dsbdd
