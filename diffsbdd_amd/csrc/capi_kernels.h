// Thin C-ABI wrappers of the stand-alone kernels (included by engine.hip): DDPM steps (ddpm.h), keyed noise, node GEMM,
// the node chain's row split (chain_split.h), bond orders (molecule.h), molecule graph statistics and fingerprint distances (mol_metrics.h), pose checks, the Vina-type score, its gradient, the rigid-body minimiser, the torsion tree, the intramolecular term and the flexible minimiser (pose_check.h, vina_score.h, vina_grad.h, vina_minimize.h, vina_torsion.h, vina_intra.h, vina_flex.h on pair_sweep.h), ligand packing (ligand_pack.h), the radius graph (radius_graph.h).
#pragma once

extern "C" {

int dsbdd_cond_reverse_update(void* stream, float* z_lig, float* xh_pocket, const float* eps_lig,
                              const float* noise, const int64_t* mask_lig, const int64_t* mask_pocket,
                              int64_t n_lig, int64_t n_pocket, int64_t batch, int32_t atom_nf,
                              int32_t residue_nf, float alpha_ts, float c_eps, float sigma, int32_t remove_com) {
  StreamDevice stream_device_(stream);
  if (!z_lig || !xh_pocket || !eps_lig || !noise || !mask_lig || !mask_pocket || batch < 1)
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(cond_update_kernel, dim3((int)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     z_lig, xh_pocket, eps_lig, noise, mask_lig, (int)n_lig, mask_pocket, (int)n_pocket,
                     3 + atom_nf, 3 + residue_nf, alpha_ts, c_eps, sigma, remove_com);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_joint_reverse_update(void* stream, float* z_lig, float* z_pocket, const float* eps_lig,
                               const float* eps_pocket, const float* noise_lig, const float* noise_pocket,
                               const int64_t* mask_lig, const int64_t* mask_pocket, int64_t n_lig,
                               int64_t n_pocket, int64_t batch, int32_t atom_nf, int32_t residue_nf,
                               float alpha_ts, float c_eps, float sigma, int32_t center_noise) {
  StreamDevice stream_device_(stream);
  if (!z_lig || !z_pocket || !eps_lig || !eps_pocket || !noise_lig || !noise_pocket || !mask_lig ||
      !mask_pocket || batch < 1)
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(joint_update_kernel, dim3((int)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     z_lig, z_pocket, eps_lig, eps_pocket, noise_lig, noise_pocket, mask_lig, (int)n_lig,
                     mask_pocket, (int)n_pocket, 3 + atom_nf, 3 + residue_nf, alpha_ts, c_eps, sigma, center_noise);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_segment_mean3(void* stream, const float* x, int32_t ld, const int64_t* mask, int64_t n_rows,
                        int64_t batch, float* out) {
  StreamDevice stream_device_(stream);
  if (!x || !mask || !out || batch < 1 || ld < 3 || n_rows < 0) return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(segment_mean3_kernel, dim3((int)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     x, ld, mask, (int)n_rows, out);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_cond_affine_noise(void* stream, float* z_lig, float* xh_pocket, const float* noise,
                            const int64_t* mask_lig, const int64_t* mask_pocket, int64_t n_lig,
                            int64_t n_pocket, int64_t batch, int32_t atom_nf, int32_t residue_nf, float a,
                            float sigma, int32_t remove_com) {
  StreamDevice stream_device_(stream);
  if (!z_lig || !xh_pocket || !noise || !mask_lig || !mask_pocket || batch < 1)
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(cond_affine_noise_kernel, dim3((int)batch), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), z_lig, xh_pocket, noise, mask_lig, (int)n_lig, mask_pocket,
                     (int)n_pocket, 3 + atom_nf, 3 + residue_nf, a, sigma, remove_com);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_joint_affine_noise(void* stream, float* z_lig, float* z_pocket, const float* noise_lig,
                             const float* noise_pocket, const int64_t* mask_lig, const int64_t* mask_pocket,
                             int64_t n_lig, int64_t n_pocket, int64_t batch, int32_t atom_nf,
                             int32_t residue_nf, float a, float sigma, int32_t center_noise,
                             int32_t remove_com) {
  StreamDevice stream_device_(stream);
  if (!z_lig || !z_pocket || !noise_lig || !noise_pocket || !mask_lig || !mask_pocket || batch < 1)
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(joint_affine_noise_kernel, dim3((int)batch), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), z_lig, z_pocket, noise_lig, noise_pocket, mask_lig,
                     (int)n_lig, mask_pocket, (int)n_pocket, 3 + atom_nf, 3 + residue_nf, a, sigma, center_noise,
                     remove_com);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_cond_repaint_update(void* stream, float* z_lig, float* xh_pocket, float* scratch_lig,
                              const float* xh0_lig, const float* com_pocket0, const float* fixed,
                              const float* noise_known, const float* noise_resample, const int64_t* mask_lig,
                              const int64_t* mask_pocket, int64_t n_lig, int64_t n_pocket, int64_t batch,
                              int32_t atom_nf, int32_t residue_nf, float alpha_s, float sigma_s,
                              float alpha_ts, float sigma_ts, int32_t resample, int32_t remove_com) {
  StreamDevice stream_device_(stream);
  if (!z_lig || !xh_pocket || !scratch_lig || !xh0_lig || !com_pocket0 || !fixed || !noise_known ||
      (resample && !noise_resample) || !mask_lig || !mask_pocket || batch < 1)
    return fail(DSBDD_ERR_ARG, "bad argument");
  CondRepaintArgs a{z_lig, xh_pocket, scratch_lig, xh0_lig, com_pocket0, fixed, noise_known, noise_resample,
                    mask_lig, mask_pocket, (int)n_lig, (int)n_pocket, 3 + atom_nf, 3 + residue_nf, alpha_s,
                    sigma_s, alpha_ts, sigma_ts, resample, remove_com};
  hipLaunchKernelGGL(cond_repaint_kernel, dim3((int)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_cond_step_keyed(void* stream, float* z_lig, float* xh_pocket, const float* eps_lig, float* scratch_lig,
                          const float* xh0_lig, const float* com_pocket0, const float* fixed, const int64_t* mask_lig,
                          const int64_t* mask_pocket, int64_t n_lig, int64_t n_pocket, int64_t batch, int32_t atom_nf,
                          int32_t residue_nf, float alpha_ts, float c_eps, float sigma, int32_t repaint, float alpha_s,
                          float sigma_s, float sigma_ts, int32_t remove_com, uint64_t seed, uint64_t draw_index,
                          int64_t sample_offset, const int64_t* sample_ids, float* t_word, float t_next) {
  StreamDevice stream_device_(stream);
  if (!z_lig || !xh_pocket || !eps_lig || !mask_lig || !mask_pocket || batch < 1 || repaint < 0 || repaint > 2 ||
      (repaint && (!scratch_lig || !xh0_lig || !com_pocket0 || !fixed)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  CondStepArgs a{};
  a.rp = CondRepaintArgs{z_lig, xh_pocket, scratch_lig, xh0_lig, com_pocket0, fixed, nullptr, nullptr, mask_lig, mask_pocket,
                         (int)n_lig, (int)n_pocket, 3 + atom_nf, 3 + residue_nf, alpha_s, sigma_s, alpha_ts, sigma_ts,
                         repaint == 2, remove_com};
  a.eps = eps_lig; a.u_alpha_ts = alpha_ts; a.u_c_eps = c_eps; a.u_sigma = sigma; a.repaint = repaint;
  a.seed = seed; a.draw = draw_index; a.sample_offset = sample_offset; a.sample_ids = sample_ids;
  a.t_word = t_word; a.t_next = t_next;
  hipLaunchKernelGGL(cond_step_keyed_kernel, dim3((int)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_joint_repaint_update(void* stream, float* z_lig, float* z_pocket, float* scratch_lig,
                               float* scratch_pocket, const float* xh0_lig, const float* xh0_pocket,
                               const float* fixed_lig, const float* fixed_pocket, const float* noise_known_lig,
                               const float* noise_known_pocket, const float* noise_jump_lig,
                               const float* noise_jump_pocket, const int64_t* mask_lig,
                               const int64_t* mask_pocket, int64_t n_lig, int64_t n_pocket, int64_t batch,
                               int32_t atom_nf, int32_t residue_nf, float alpha_s, float sigma_s,
                               float alpha_ts, float sigma_ts, int32_t jump) {
  StreamDevice stream_device_(stream);
  if (!z_lig || !z_pocket || !scratch_lig || !scratch_pocket || !xh0_lig || !xh0_pocket || !fixed_lig ||
      !fixed_pocket || !noise_known_lig || !noise_known_pocket || (jump && (!noise_jump_lig || !noise_jump_pocket)) ||
      !mask_lig || !mask_pocket || batch < 1)
    return fail(DSBDD_ERR_ARG, "bad argument");
  JointRepaintArgs a{z_lig, z_pocket, scratch_lig, scratch_pocket, xh0_lig, xh0_pocket, fixed_lig, fixed_pocket,
                     noise_known_lig, noise_known_pocket, noise_jump_lig, noise_jump_pocket, mask_lig, mask_pocket,
                     (int)n_lig, (int)n_pocket, 3 + atom_nf, 3 + residue_nf, alpha_s, sigma_s, alpha_ts, sigma_ts,
                     jump};
  hipLaunchKernelGGL(joint_repaint_kernel, dim3((int)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_randn_keyed(void* stream, float* out, const int64_t* mask, int64_t n_rows, int32_t n_cols,
                      int64_t batch, int64_t sample_offset, const int64_t* sample_ids, uint64_t seed,
                      uint64_t draw_index, uint32_t stream_id) {
  StreamDevice stream_device_(stream);
  (void)batch;
  if (!out || !mask || n_rows < 0 || n_cols < 1) return fail(DSBDD_ERR_ARG, "bad argument");
  const int64_t n = n_rows * n_cols;
  if (n == 0) return DSBDD_OK;
  hipLaunchKernelGGL(randn_keyed_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), out, mask, (int)n_rows, (int)n_cols, sample_offset,
                     sample_ids, seed, draw_index, stream_id);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_node_linear(void* stream, const float* A1, int32_t lda1, int32_t K1, const float* A2, int32_t lda2,
                      int32_t K2, const float* WT, int32_t ldw, const float* bias, const float* R, int32_t ldr,
                      float* C, int32_t ldc, int64_t M, int32_t N, int32_t act) {
  StreamDevice stream_device_(stream);
  if (!A1 || !WT || !C || K1 < 1 || K2 < 0 || (K2 > 0 && !A2) || (ldw & 3) || N > ldw ||
      (reinterpret_cast<uintptr_t>(WT) & 15))
    return fail(DSBDD_ERR_ARG, "bad argument (WT must be 16-byte aligned with ldw % 4 == 0)");
  HIP_TRY(nl(static_cast<hipStream_t>(stream), A1, lda1, K1, A2, lda2, K2, WT, ldw, bias, R, ldr, C, ldc, M, N, act));
  return DSBDD_OK;
}

// the argument checks of the two chain-split entry points (H, projections and rows as launch_node_chain takes them)
static bool chain_split_args_ok(int32_t M, int32_t n_proj, const void* proj_N, const void* proj_first, const void* proj_count,
                                int32_t H, int32_t grid, const void* header, const void* pieces, int64_t capacity) {
  return header && capacity >= 0 && (capacity == 0 || pieces) && grid >= 1 && (H == 64 || H == 128 || H == 192 || H == 256) &&
         n_proj >= 0 && n_proj <= kChainMaxProj && (n_proj == 0 || (proj_N && proj_first && proj_count)) && M <= (8 << 20);
}
static const char* const kChainSplitBadArg =
    "bad argument (null output, grid < 1, H not 64 / 128 / 192 / 256, more than 3 projections or more than 8 M rows)";

// both policies (Split = ChainSplit / ChainDealt) behind one body each
extern "C++" {
template <class Split>
static int64_t chain_split_host(int32_t M, int32_t do_mlp, int32_t n_proj, const int32_t* proj_N, const int32_t* proj_first,
                                const int32_t* proj_count, int32_t H, int32_t grid, uint32_t* header, int32_t* pieces,
                                int64_t capacity) {
  if (!chain_split_args_ok(M, n_proj, proj_N, proj_first, proj_count, H, grid, header, pieces, capacity))
    return fail(DSBDD_ERR_ARG, kChainSplitBadArg);
  ChainSplitIn in{};
  in.M = M; in.do_mlp = do_mlp; in.n_proj = n_proj; in.H = H; in.grid = grid;
  for (int q = 0; q < n_proj; ++q) { in.N[q] = proj_N[q]; in.first[q] = proj_first[q]; in.count[q] = proj_count[q]; }
  const Split sp(in);
  sp.report(header);
  return chain_split_list(sp, grid, grid, ~0u, pieces, capacity);
}

template <class Split>
static int chain_split_probe(void* stream, int32_t M, const int32_t* m_count, int32_t do_mlp, int32_t n_proj,
                             const int32_t* proj_N, const int32_t* proj_first, const int32_t* const* proj_count, int32_t H,
                             int32_t grid, uint32_t* header, int32_t* pieces, int64_t capacity, int64_t* n_pieces) {
  StreamDevice stream_device_(stream);
  if (!n_pieces || !chain_split_args_ok(M, n_proj, proj_N, proj_first, proj_count, H, grid, header, pieces, capacity))
    return fail(DSBDD_ERR_ARG, kChainSplitBadArg);
  NodeChainArgs a{};
  a.M = M; a.m_count = m_count; a.do_mlp = do_mlp; a.n_proj = n_proj;
  for (int q = 0; q < n_proj; ++q) { a.proj[q].N = proj_N[q]; a.proj[q].first = proj_first[q]; a.proj[q].count = proj_count[q]; }
  hipLaunchKernelGGL(chain_split_probe_kernel<Split>, dim3(grid), dim3(64), 0, static_cast<hipStream_t>(stream), a, (int)H,
                     header, pieces, (long long)capacity, reinterpret_cast<long long*>(n_pieces));
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}
}  // extern "C++"

int64_t dsbdd_chain_split_host(int32_t M, int32_t do_mlp, int32_t n_proj, const int32_t* proj_N,
                               const int32_t* proj_first, const int32_t* proj_count, int32_t H, int32_t grid,
                               uint32_t* header, int32_t* pieces, int64_t capacity) {
  return chain_split_host<ChainSplit>(M, do_mlp, n_proj, proj_N, proj_first, proj_count, H, grid, header, pieces, capacity);
}

int dsbdd_chain_split_probe(void* stream, int32_t M, const int32_t* m_count, int32_t do_mlp, int32_t n_proj,
                            const int32_t* proj_N, const int32_t* proj_first, const int32_t* const* proj_count,
                            int32_t H, int32_t grid, uint32_t* header, int32_t* pieces, int64_t capacity,
                            int64_t* n_pieces) {
  return chain_split_probe<ChainSplit>(stream, M, m_count, do_mlp, n_proj, proj_N, proj_first, proj_count, H, grid, header,
                                       pieces, capacity, n_pieces);
}

int64_t dsbdd_chain_deal_host(int32_t M, int32_t do_mlp, int32_t n_proj, const int32_t* proj_N,
                              const int32_t* proj_first, const int32_t* proj_count, int32_t H, int32_t grid,
                              uint32_t* header, int32_t* pieces, int64_t capacity) {
  return chain_split_host<ChainDealt>(M, do_mlp, n_proj, proj_N, proj_first, proj_count, H, grid, header, pieces, capacity);
}

int dsbdd_chain_deal_probe(void* stream, int32_t M, const int32_t* m_count, int32_t do_mlp, int32_t n_proj,
                           const int32_t* proj_N, const int32_t* proj_first, const int32_t* const* proj_count,
                           int32_t H, int32_t grid, uint32_t* header, int32_t* pieces, int64_t capacity,
                           int64_t* n_pieces) {
  return chain_split_probe<ChainDealt>(stream, M, m_count, do_mlp, n_proj, proj_N, proj_first, proj_count, H, grid, header,
                                      pieces, capacity, n_pieces);
}

int dsbdd_bond_orders(void* stream, const float* x, const int32_t* atom_type, const int32_t* mol_off,
                      int64_t batch, int32_t n_types, const float* bonds1, const float* bonds2,
                      const float* bonds3, float margin1, float margin2, float margin3, int32_t n_max,
                      int8_t* order) {
  StreamDevice stream_device_(stream);
  if (!x || !atom_type || !mol_off || !bonds1 || !bonds2 || !bonds3 || !order || batch < 1 || n_types < 1 ||
      n_max < 1)
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemsetAsync(order, 0, (size_t)batch * n_max * n_max, s));
  BondArgs a{x, atom_type, mol_off, bonds1, bonds2, bonds3, margin1, margin2, margin3, n_types, n_max,
             reinterpret_cast<signed char*>(order)};
  hipLaunchKernelGGL(bond_orders_kernel, dim3((unsigned)batch), dim3(64), 0, s, a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_mol_graph_stats(void* stream, const int8_t* order, const int32_t* atom_type, const int32_t* mol_off, int64_t batch,
                          int32_t n_types, const int32_t* max_valence, int32_t n_max, int32_t orders_in_key,
                          int32_t* valence, int32_t* label, int32_t* stats, uint64_t* keys, uint32_t* fingerprint,
                          int32_t* type_counts) {
  StreamDevice stream_device_(stream);
  if (!order || !atom_type || !mol_off || !max_valence || !valence || !label || !stats || !keys || !fingerprint ||
      !type_counts)
    return fail(DSBDD_ERR_ARG, "null argument");
  if (batch < 0 || batch > 0x7fffffff || n_types < 1) return fail(DSBDD_ERR_ARG, "bad batch or n_types");
  if (n_max < 1 || n_max > kMolMaxAtoms)
    return fail(DSBDD_ERR_ARG, "n_max must be in [1, " + std::to_string(kMolMaxAtoms) + "]");
  if (batch == 0) return DSBDD_OK;
  MolGraphArgs a{reinterpret_cast<const signed char*>(order), atom_type, mol_off, max_valence, n_types, n_max,
                 orders_in_key != 0, valence, label, stats, reinterpret_cast<mm_u64*>(keys), fingerprint, type_counts};
  hipLaunchKernelGGL(mol_graph_kernel, dim3((unsigned)batch), dim3(64), mol_graph_lds_bytes(n_max),
                     static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_fp_diversity(void* stream, const uint32_t* fingerprint, const int32_t* group_off, int64_t n_groups, double* sum,
                       int64_t* pairs) {
  StreamDevice stream_device_(stream);
  if (!fingerprint || !group_off || !sum || !pairs) return fail(DSBDD_ERR_ARG, "null argument");
  if (n_groups < 0 || n_groups > 0x7fffffff) return fail(DSBDD_ERR_ARG, "bad n_groups");
  if (reinterpret_cast<uintptr_t>(fingerprint) & 15) return fail(DSBDD_ERR_ARG, "fingerprints must be 16-byte aligned");
  if (n_groups == 0) return DSBDD_OK;
  hipLaunchKernelGGL(fp_diversity_kernel, dim3((unsigned)n_groups), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint4*>(fingerprint), group_off, sum, reinterpret_cast<long long*>(pairs));
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

// the counts of the two pair entries (pair_sweep.h: PairBatch holds them as int)
static int check_pair_counts(int64_t batch, int64_t n_groups) {
  if (batch < 0 || batch > 0x7fffffff || n_groups < 0 || n_groups > 0x7fffffff)
    return fail(DSBDD_ERR_ARG, "bad batch or n_groups");
  return DSBDD_OK;
}

int dsbdd_pose_check(void* stream, const float* lig_x, const float* lig_r, const int32_t* mol_off, int64_t batch,
                     const int32_t* mol_group, const float* poc_x, const float* poc_r, const int32_t* group_off,
                     int64_t n_groups, float tol, float contact, int32_t* atom_out, int32_t* mol_out) {
  StreamDevice stream_device_(stream);
  if (!lig_x || !lig_r || !mol_off || !mol_group || !poc_x || !poc_r || !group_off || !atom_out || !mol_out)
    return fail(DSBDD_ERR_ARG, "null argument");
  if (int rc = check_pair_counts(batch, n_groups)) return rc;
  if (!std::isfinite(tol) || tol < 0.f || !std::isfinite(contact) || contact < 0.f)
    return fail(DSBDD_ERR_ARG, "tol and contact must be finite and not negative");
  if (batch == 0) return DSBDD_OK;
  PoseArgs a{{lig_x, mol_off, mol_group, poc_x, group_off, (int)batch, (int)n_groups}, lig_r, poc_r, tol, contact,
             atom_out, mol_out};
  hipLaunchKernelGGL(pose_check_kernel, dim3((unsigned)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_vina_type(void* stream, const int8_t* order, const int32_t* atom_type, const int32_t* mol_off, int64_t batch,
                    int32_t n_types, const int32_t* class_elem, int32_t n_max, int32_t* lig_code, int32_t* mol_int) {
  StreamDevice stream_device_(stream);
  if (!order || !atom_type || !mol_off || !class_elem || !lig_code || !mol_int) return fail(DSBDD_ERR_ARG, "null argument");
  if (batch < 0 || batch > 0x7fffffff || n_types < 1) return fail(DSBDD_ERR_ARG, "bad batch or n_types");
  if (n_max < 1 || n_max > kMolMaxAtoms)
    return fail(DSBDD_ERR_ARG, "n_max must be in [1, " + std::to_string(kMolMaxAtoms) + "]");
  if (batch == 0) return DSBDD_OK;
  VinaTypeArgs a{reinterpret_cast<const signed char*>(order), atom_type, mol_off, class_elem, (int)batch, n_types, n_max,
                 lig_code, mol_int};
  hipLaunchKernelGGL(vina_type_kernel, dim3((unsigned)batch), dim3(64), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_vina_score(void* stream, const float* lig_x, const int32_t* lig_code, const int32_t* mol_off, int64_t batch,
                     const int32_t* mol_group, const int32_t* mol_int, const float* poc_x, const int32_t* poc_code,
                     const int32_t* group_off, int64_t n_groups, float* atom_out, float* mol_out, int32_t* mol_flag) {
  StreamDevice stream_device_(stream);
  if (!lig_x || !lig_code || !mol_off || !mol_group || !mol_int || !poc_x || !poc_code || !group_off || !atom_out ||
      !mol_out || !mol_flag)
    return fail(DSBDD_ERR_ARG, "null argument");
  if (int rc = check_pair_counts(batch, n_groups)) return rc;
  if (batch == 0) return DSBDD_OK;
  VinaScoreArgs a{{lig_x, mol_off, mol_group, poc_x, group_off, (int)batch, (int)n_groups}, lig_code, mol_int, poc_code,
                  atom_out, mol_out, mol_flag};
  hipLaunchKernelGGL(vina_score_kernel, dim3((unsigned)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_vina_score_grad(void* stream, const float* lig_x, const int32_t* lig_code, const int32_t* mol_off, int64_t batch,
                          const int32_t* mol_group, const int32_t* mol_int, const float* poc_x, const int32_t* poc_code,
                          const int32_t* group_off, int64_t n_groups, float* atom_out, float* mol_out, int32_t* mol_flag,
                          float* atom_grad, float* mol_grad) {
  StreamDevice stream_device_(stream);
  if (!lig_x || !lig_code || !mol_off || !mol_group || !mol_int || !poc_x || !poc_code || !group_off || !atom_out ||
      !mol_out || !mol_flag || !atom_grad || !mol_grad)
    return fail(DSBDD_ERR_ARG, "null argument");
  if (int rc = check_pair_counts(batch, n_groups)) return rc;
  if (batch == 0) return DSBDD_OK;
  VinaGradArgs a{{{lig_x, mol_off, mol_group, poc_x, group_off, (int)batch, (int)n_groups}, lig_code, mol_int, poc_code,
                  atom_out, mol_out, mol_flag}, atom_grad, mol_grad};
  hipLaunchKernelGGL(vina_grad_kernel, dim3((unsigned)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_vina_minimize(void* stream, const float* lig_x, const int32_t* lig_code, const int32_t* mol_off, int64_t batch,
                        const int32_t* mol_group, const int32_t* mol_int, const float* poc_x, const int32_t* poc_code,
                        const int32_t* group_off, int64_t n_groups, float* atom_out, float* mol_out, int32_t* mol_flag,
                        float* atom_grad, float* mol_grad, float step, float tol, int32_t max_evals, float* x_out,
                        float* mol_pose, float* mol_min, int32_t* mol_stat) {
  StreamDevice stream_device_(stream);
  if (!lig_x || !lig_code || !mol_off || !mol_group || !mol_int || !poc_x || !poc_code || !group_off || !atom_out ||
      !mol_out || !mol_flag || !atom_grad || !mol_grad || !x_out || !mol_pose || !mol_min || !mol_stat)
    return fail(DSBDD_ERR_ARG, "null argument");
  if (int rc = check_pair_counts(batch, n_groups)) return rc;
  if (!std::isfinite(step) || !(step > 0.f) || !std::isfinite(tol) || !(tol > 0.f))
    return fail(DSBDD_ERR_ARG, "step and tol must be finite and positive");
  if (max_evals < 1 || max_evals > kVinaMaxEvals)
    return fail(DSBDD_ERR_ARG, "max_evals must be in [1, " + std::to_string(kVinaMaxEvals) + "]");
  if (batch == 0) return DSBDD_OK;                                  // nothing is read or written
  if (lig_x == x_out) return fail(DSBDD_ERR_ARG, "lig_x and x_out must not alias");
  // the sweep reads the pose under evaluation from x_out
  VinaMinArgs a{{{{x_out, mol_off, mol_group, poc_x, group_off, (int)batch, (int)n_groups}, lig_code, mol_int, poc_code,
                  atom_out, mol_out, mol_flag}, atom_grad, mol_grad}, lig_x, step, tol, max_evals, x_out, mol_pose, mol_min,
                mol_stat};
  hipLaunchKernelGGL(vina_minimize_kernel, dim3((unsigned)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_vina_torsions(void* stream, const int8_t* order, const int32_t* atom_type, const int32_t* mol_off, int64_t batch,
                        int32_t n_types, const int32_t* class_elem, int32_t n_max, int32_t* tor_int, int32_t* tor_end,
                        int32_t* tor_side, int32_t* pair_mask) {
  StreamDevice stream_device_(stream);
  if (!order || !atom_type || !mol_off || !class_elem || !tor_int || !tor_end || !tor_side || !pair_mask)
    return fail(DSBDD_ERR_ARG, "null argument");
  if (batch < 0 || batch > 0x7fffffff || n_types < 1) return fail(DSBDD_ERR_ARG, "bad batch or n_types");
  if (n_max < 1 || n_max > kMolMaxAtoms)
    return fail(DSBDD_ERR_ARG, "n_max must be in [1, " + std::to_string(kMolMaxAtoms) + "]");
  if (batch == 0) return DSBDD_OK;
  VinaTorsionArgs a{reinterpret_cast<const signed char*>(order), atom_type, mol_off, class_elem, (int)batch, n_types, n_max,
                    tor_int, tor_end, tor_side, pair_mask};
  hipLaunchKernelGGL(vina_torsion_kernel, dim3((unsigned)batch), dim3(64), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_vina_intra(void* stream, const float* lig_x, const int32_t* lig_code, const int32_t* mol_off, int64_t batch,
                     const int32_t* pair_mask, float* atom_out, float* mol_out, int32_t* mol_flag, float* atom_grad) {
  StreamDevice stream_device_(stream);
  if (!lig_x || !lig_code || !mol_off || !pair_mask || !atom_out || !mol_out || !mol_flag || !atom_grad)
    return fail(DSBDD_ERR_ARG, "null argument");
  if (int rc = check_pair_counts(batch, 0)) return rc;
  if (batch == 0) return DSBDD_OK;
  // the molecule's own rows are the group of its sweep
  VinaIntraArgs a{{{{lig_x, mol_off, nullptr, lig_x, mol_off, (int)batch, (int)batch}, lig_code, nullptr, lig_code, atom_out,
                    mol_out, mol_flag}, atom_grad, nullptr}, pair_mask};
  hipLaunchKernelGGL(vina_intra_kernel, dim3((unsigned)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_vina_flex(void* stream, const float* lig_x, const int32_t* lig_code, const int32_t* mol_off, int64_t batch,
                    const int32_t* mol_group, const int32_t* mol_int, const float* poc_x, const int32_t* poc_code,
                    const int32_t* group_off, int64_t n_groups, const int32_t* tor_int, const int32_t* tor_end,
                    const int32_t* tor_side, const int32_t* pair_mask, int32_t dofs, float step, float tol, int32_t max_evals,
                    float* atom_out, float* mol_out, int32_t* mol_flag, float* atom_grad, float* mol_grad, float* intra_atom,
                    float* intra_mol, int32_t* intra_flag, float* intra_grad, float* x_out, float* mol_pose, float* mol_flex,
                    int32_t* mol_stat, float* theta, float* tau) {
  StreamDevice stream_device_(stream);
  if (!lig_x || !lig_code || !mol_off || !mol_group || !mol_int || !poc_x || !poc_code || !group_off || !tor_int || !tor_end ||
      !tor_side || !pair_mask || !atom_out || !mol_out || !mol_flag || !atom_grad || !mol_grad || !intra_atom || !intra_mol ||
      !intra_flag || !intra_grad || !x_out || !mol_pose || !mol_flex || !mol_stat || !theta || !tau)
    return fail(DSBDD_ERR_ARG, "null argument");
  if (int rc = check_pair_counts(batch, n_groups)) return rc;
  if (!std::isfinite(step) || !(step > 0.f) || !std::isfinite(tol) || !(tol > 0.f))
    return fail(DSBDD_ERR_ARG, "step and tol must be finite and positive");
  if (max_evals < 1 || max_evals > kVinaMaxEvals)
    return fail(DSBDD_ERR_ARG, "max_evals must be in [1, " + std::to_string(kVinaMaxEvals) + "]");
  if (dofs < 1 || dofs > (kVinaDofRigid | kVinaDofTorsions)) return fail(DSBDD_ERR_ARG, "dofs must be 1, 2 or 3");
  if (batch == 0) return DSBDD_OK;                                  // nothing is read or written
  if (lig_x == x_out) return fail(DSBDD_ERR_ARG, "lig_x and x_out must not alias");
  // both sweeps read the pose under evaluation from x_out
  VinaFlexArgs a{{{{{x_out, mol_off, mol_group, poc_x, group_off, (int)batch, (int)n_groups}, lig_code, mol_int, poc_code,
                    atom_out, mol_out, mol_flag}, atom_grad, mol_grad}, lig_x, step, tol, max_evals, x_out, mol_pose, mol_flex,
                  mol_stat},
                 {{{{x_out, mol_off, nullptr, x_out, mol_off, (int)batch, (int)batch}, lig_code, nullptr, lig_code, intra_atom,
                    intra_mol, intra_flag}, intra_grad, nullptr}, pair_mask},
                 tor_int, tor_end, tor_side, dofs, theta, tau};
  hipLaunchKernelGGL(vina_flex_kernel, dim3((unsigned)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_pack_ligands(void* stream, const float* tmpl_x, const int32_t* tmpl_type, const int32_t* tmpl_ptr,
                       int32_t n_tmpl, int64_t tmpl_rows, const int32_t* slot_tmpl, const int32_t* slot_size,
                       const int32_t* slot_off, int64_t batch, int64_t n_rows, int32_t atom_nf, float* x,
                       float* one_hot, int64_t* lig_fixed, int64_t* mask, int64_t* size) {
  StreamDevice stream_device_(stream);
  if (!tmpl_ptr || !slot_tmpl || !slot_size || !slot_off || !x || !one_hot || !lig_fixed || !mask || !size)
    return fail(DSBDD_ERR_ARG, "null argument");
  if ((tmpl_rows > 0 && (!tmpl_x || !tmpl_type)) || tmpl_rows < 0 || n_tmpl < 0 || atom_nf < 1)
    return fail(DSBDD_ERR_ARG, "bad template set");
  if (batch < 1 || n_rows < batch || n_rows > 0x7fffffff / 4)
    return fail(DSBDD_ERR_ARG, "every slot needs at least one row (n_rows >= batch)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  PackArgs a{tmpl_x, tmpl_type, tmpl_ptr, slot_tmpl, slot_size, slot_off, n_tmpl, (int)tmpl_rows, (int)batch,
             (int)n_rows, atom_nf, x, one_hot, reinterpret_cast<long long*>(lig_fixed),
             reinterpret_cast<long long*>(mask), reinterpret_cast<long long*>(size)};
  hipLaunchKernelGGL(pack_ligands_kernel, dim3((unsigned)((n_rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_build_edges(void* stream, const float* x, const int64_t* mask_lig, const int64_t* mask_pocket,
                      int64_t n_lig, int64_t n_pocket, int64_t batch, const dsbdd_config* cfg,
                      int32_t* node_batch, int32_t* lig_off, int32_t* poc_off, int32_t* deg, int32_t* row_ptr,
                      int32_t* edge_row, int32_t* edge_col, float* edge_d0, int64_t edge_capacity,
                      int32_t* status) {
  StreamDevice stream_device_(stream);
  if (!x || !mask_lig || !mask_pocket || !cfg || !node_batch || !lig_off || !poc_off || !deg || !row_ptr ||
      !edge_row || !edge_col || !edge_d0 || !status || batch < 1)
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int N = (int)(n_lig + n_pocket), B = (int)batch;
  const int work = N > B + 1 ? N : B + 1;
  hipLaunchKernelGGL(prep_kernel, dim3((work + 255) / 256), dim3(256), 0, s, mask_lig, (int)n_lig, mask_pocket,
                     (int)n_pocket, B, node_batch, lig_off, poc_off, (int*)nullptr);
  HIP_TRY(hipGetLastError());
  return build_edges_impl(s, x, (int)n_lig, N, B, *cfg, node_batch, lig_off, poc_off, deg, row_ptr, edge_row,
                          edge_col, edge_d0, edge_capacity, status);
}

}  // extern "C"
