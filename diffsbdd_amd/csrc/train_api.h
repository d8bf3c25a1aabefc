// C-ABI entry points of training (included by engine.hip): argument checks around the building blocks (train_blocks.h)
// and the network walk (train_net.h), then the native training loop around the network call: the loss terms of the
// pocket-conditioned step (loss_head.h), the likelihood bound of given ligands (score.h, score_joint.h; all three over loss_parts.h), the fused clipping + AdamW step (optim.h), the auxiliary LJ loss (lj_loss.h).
#pragma once

static LossCfg loss_cfg_of(const dsbdd_loss_cfg* c) {
  return LossCfg{c->batch, c->n_lig, c->n_pocket, c->atom_nf, c->residue_nf, c->timesteps, c->remove_com, c->vnode_idx,
                 c->norm_value_x, c->norm_value_h, c->norm_bias_h, c->n1_tab, c->n2_tab};
}
static bool loss_cfg_ok(const dsbdd_loss_cfg* c) {
  return c && c->batch > 0 && c->n_lig >= 0 && c->n_pocket >= 0 && c->atom_nf > 0 && c->residue_nf > 0 && c->timesteps > 0 &&
         c->norm_value_x > 0.f && c->norm_value_h > 0.f && c->vnode_idx < c->atom_nf;
}

extern "C" {

// ---- building blocks (train_blocks.h) -----------------------------------------------------------------------------------
size_t dsbdd_train_scratch_bytes(int32_t H, int64_t n_nodes, int64_t n_edges) {
  if (!hidden_nf_ok(H) || n_nodes < 1 || n_edges < 0) return 0;
  return carve_train(nullptr, H, n_nodes, n_edges).bytes;
}

size_t dsbdd_train_wgrad_scratch_bytes(int64_t K, int64_t M, int64_t N) {
  if (K < 1 || M < 1 || N < 1) return 0;
  return wgrad_floats_upto(K, M, N) * 4;      // covers every K' <= K (the plan is not monotonic in K)
}

size_t dsbdd_train_wgrad_plan_bytes(int64_t K, int64_t M, int64_t N) {
  if (K < 1 || M < 1 || N < 1) return 0;
  return wgrad_plan(K, M, N).floats * 4;      // what a call with exactly this K writes (tests: <= the bound above)
}

int dsbdd_train_edge_rev(void* stream, const dsbdd_train_graph* g, int32_t* rev) {
  StreamDevice stream_device_(stream);
  if (!graph_ok(g) || !rev) return fail(DSBDD_ERR_ARG, "bad argument");
  if (g->n_edges == 0) return DSBDD_OK;
  return launch_1d(edge_rev_kernel, (size_t)g->n_edges, static_cast<hipStream_t>(stream), g->erow, g->ecol, g->row_ptr, g->deg,
                   (int)g->n_edges, (int)g->n_nodes, rev);
}

int dsbdd_train_sample_mean(void* stream, const float* x, const dsbdd_train_graph* g, float* mean) {
  StreamDevice stream_device_(stream);
  if (!graph_ok(g) || !x || !mean) return fail(DSBDD_ERR_ARG, "bad argument");
  return sample_mean_impl(static_cast<hipStream_t>(stream), x, g, mean);
}

int dsbdd_train_gcl_forward(void* stream, int32_t H, const dsbdd_train_graph* g, const dsbdd_train_mlp* m, const float* x,
                            float norm_factor, float* agg, void* scratch, size_t scratch_bytes) {
  return gcl_forward_impl(stream, H, g, m, x, norm_factor, agg, scratch, scratch_bytes, nullptr);
}

int dsbdd_train_coord_forward(void* stream, int32_t H, const dsbdd_train_graph* g, const dsbdd_train_mlp* m, int32_t n_mlp,
                              const float* x, const float* mean, int64_t n_upd, float norm_constant, float coords_range,
                              int32_t use_tanh, float norm_factor, float* x_out, void* scratch, size_t scratch_bytes) {
  return coord_forward_impl(stream, H, g, m, n_mlp, x, mean, n_upd, norm_constant, coords_range, use_tanh, norm_factor, x_out,
                            scratch, scratch_bytes, nullptr, 0);
}

int dsbdd_train_gcl_backward(void* stream, int32_t H, const dsbdd_train_graph* g, const dsbdd_train_mlp* m, const float* x,
                             float norm_factor, const float* d_agg, const dsbdd_train_mlp_grad* out, float* d_x,
                             void* scratch, size_t scratch_bytes) {
  return gcl_backward_impl(stream, H, g, m, x, norm_factor, d_agg, out, d_x, scratch, scratch_bytes, nullptr);
}

int dsbdd_train_coord_backward(void* stream, int32_t H, const dsbdd_train_graph* g, const dsbdd_train_mlp* m, int32_t n_mlp,
                               const float* x, const float* mean, int64_t n_upd, int64_t e_upd, float norm_constant,
                               float coords_range, int32_t use_tanh, float norm_factor, const float* d_xout,
                               const dsbdd_train_mlp_grad* out, float* d_x, float* d_mean, void* scratch,
                               size_t scratch_bytes) {
  return coord_backward_impl(stream, H, g, m, n_mlp, x, mean, n_upd, e_upd, norm_constant, coords_range, use_tanh, norm_factor,
                             d_xout, out, d_x, d_mean, scratch, scratch_bytes, nullptr);
}

int dsbdd_train_radial_backward(void* stream, const dsbdd_train_graph* g, const float* x, const float* gd, float* d_x) {
  StreamDevice stream_device_(stream);
  if (!graph_ok(g) || !g->rev || !x || !gd || !d_x) return fail(DSBDD_ERR_ARG, "bad argument");
  return radial_backward_impl(static_cast<hipStream_t>(stream), g, x, gd, d_x);
}

int dsbdd_train_wgrad(void* stream, const float* A, int32_t lda, const float* B, int32_t ldb, int64_t K, int32_t M,
                      int32_t N, float* C, void* scratch, size_t scratch_bytes) {
  StreamDevice stream_device_(stream);
  if (!A || !B || !C || K < 1 || M < 1 || N < 1 || lda < M || ldb < N || !scratch) return fail(DSBDD_ERR_ARG, "bad argument");
  if (wgrad_plan(K, M, N).floats * 4 > scratch_bytes) return fail(DSBDD_ERR_CAPACITY, "scratch too small");
  return wgrad_impl(static_cast<hipStream_t>(stream), A, lda, B, ldb, K, M, N, C, static_cast<float*>(scratch), scratch_bytes / 4);
}

int dsbdd_train_colsum(void* stream, const float* A, int32_t lda, int64_t M, int32_t N, float* out, void* scratch,
                       size_t scratch_bytes) {
  StreamDevice stream_device_(stream);
  if (!A || !out || M < 1 || N < 1 || lda < N || !scratch) return fail(DSBDD_ERR_ARG, "bad argument");
  if ((size_t)((M + 31) / 32) * N * 4 > scratch_bytes) return fail(DSBDD_ERR_CAPACITY, "scratch too small");
  HIP_TRY(reduce_parts(static_cast<hipStream_t>(stream), A, (int)M, (size_t)lda, N, out, static_cast<float*>(scratch)));
  return DSBDD_OK;
}

// ---- the network walk (train_net.h) -------------------------------------------------------------------------------------
int dsbdd_train_net_create(const dsbdd_config* cfg, dsbdd_train_net** out) {
  if (!cfg || !out) return fail(DSBDD_ERR_ARG, "null argument");
  if (!hidden_nf_ok(cfg->hidden_nf) || cfg->n_layers < 1 || cfg->inv_sublayers < 1 || cfg->atom_nf < 1 || cfg->residue_nf < 1)
    return fail(DSBDD_ERR_ARG, "unsupported configuration");
  *out = tn_create(*cfg);
  return DSBDD_OK;
}
void dsbdd_train_net_destroy(dsbdd_train_net* n) {
  if (n && n->side_ready) n->side.destroy();
  delete n;
}
int dsbdd_train_net_param_count(const dsbdd_train_net* n) { return n ? n->ix.n : 0; }
size_t dsbdd_train_net_pack_bytes(const dsbdd_train_net* n) { return n ? tn_carve_pack(nullptr, n->cfg).bytes : 0; }
size_t dsbdd_train_net_workspace_bytes(const dsbdd_train_net* n, const dsbdd_train_graph* g) {
  if (!n || !graph_ok(g)) return 0;
  return tn_carve_ws(nullptr, tn_dims(n->cfg, g), n->store_z2).bytes;
}

// pack_is_current != 0: the caller holds the pack over an accumulation window -- no re-layout; DSBDD_ERR_STATE unless the
// pack buffer was last written for exactly these parameter tensors
int dsbdd_train_net_forward_held(dsbdd_train_net* net, void* stream, const dsbdd_train_graph* g, const float* const* params,
                                 void* pack, size_t pack_bytes, void* ws, size_t ws_bytes, const float* xh_lig,
                                 const float* xh_pocket, const float* t, int64_t t_count, int32_t zero_nan, float* eps_lig,
                                 float* eps_pocket, int32_t* status, int32_t pack_is_current) {
  if (!net) return fail(DSBDD_ERR_ARG, "null handle");
  StreamDevice stream_device_(stream);
  if (!net || !graph_ok(g) || !params || !pack || !ws || !t || !status || t_count < 1 || (g->n_lig > 0 && (!xh_lig || !eps_lig)) ||
      (g->n_nodes > g->n_lig && (!xh_pocket || !eps_pocket)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  for (int i = 0; i < net->ix.n; ++i) if (!params[i]) return fail(DSBDD_ERR_ARG, "null parameter " + std::to_string(i));
  TrainForward f(net, stream, g, params, pack, ws);
  if (f.pk.bytes > pack_bytes) return fail(DSBDD_ERR_CAPACITY, "pack buffer too small (dsbdd_train_net_pack_bytes)");
  if (f.w.bytes > ws_bytes) return fail(DSBDD_ERR_CAPACITY, "workspace too small (dsbdd_train_net_workspace_bytes)");
  return f.run(xh_lig, xh_pocket, t, t_count, zero_nan, eps_lig, eps_pocket, status, pack_is_current != 0);
}
int dsbdd_train_net_forward(dsbdd_train_net* net, void* stream, const dsbdd_train_graph* g, const float* const* params,
                            void* pack, size_t pack_bytes, void* ws, size_t ws_bytes, const float* xh_lig,
                            const float* xh_pocket, const float* t, int64_t t_count, int32_t zero_nan, float* eps_lig,
                            float* eps_pocket, int32_t* status) {
  if (!net) return fail(DSBDD_ERR_ARG, "bad argument");
  return dsbdd_train_net_forward_held(net, stream, g, params, pack, pack_bytes, ws, ws_bytes, xh_lig, xh_pocket, t, t_count,
                                      zero_nan, eps_lig, eps_pocket, status, 0);
}

// accumulate [param_count] or null (null: every gradient is overwritten)
static int tn_backward(dsbdd_train_net* net, void* stream, const dsbdd_train_graph* g, const float* const* params,
                       float* const* grads, const uint8_t* accumulate, void* pack, size_t pack_bytes, void* ws,
                       size_t ws_bytes, int64_t e_upd, const float* d_eps_lig, const float* d_eps_pocket, float* d_xh_lig,
                       float* d_xh_pocket) {
  StreamDevice stream_device_(stream);      // (makes the stream's device current: the side streams are created on it)
  if (!net || !graph_ok(g) || !g->rev || !params || !grads || !pack || !ws) return fail(DSBDD_ERR_ARG, "bad argument");
  for (int i = 0; i < net->ix.n; ++i)
    if (!params[i] || !grads[i]) return fail(DSBDD_ERR_ARG, "null parameter / gradient " + std::to_string(i));
  if ((g->n_lig > 0 && !d_eps_lig) || (g->n_nodes > g->n_lig && !d_eps_pocket)) return fail(DSBDD_ERR_ARG, "null output gradient");
  if (net->cfg.update_pocket_coords) e_upd = g->n_edges;      // (else: row_ptr[n_lig], the edge prefix of the ligand rows, a host value)
  if (e_upd < 0 || e_upd > g->n_edges) return fail(DSBDD_ERR_ARG, "e_upd out of range");
  TrainBackward f(net, stream, g, params, grads, accumulate, pack, ws, e_upd, d_xh_lig || d_xh_pocket);
  if (f.pk.bytes > pack_bytes || f.w.bytes > ws_bytes) return fail(DSBDD_ERR_CAPACITY, "buffer too small");
  return f.run(d_eps_lig, d_eps_pocket, d_xh_lig, d_xh_pocket);
}
int dsbdd_train_net_backward(dsbdd_train_net* net, void* stream, const dsbdd_train_graph* g, const float* const* params,
                             float* const* grads, void* pack, size_t pack_bytes, void* ws, size_t ws_bytes,
                             int64_t e_upd, const float* d_eps_lig, const float* d_eps_pocket, float* d_xh_lig,
                             float* d_xh_pocket) {
  return tn_backward(net, stream, g, params, grads, nullptr, pack, pack_bytes, ws, ws_bytes, e_upd, d_eps_lig, d_eps_pocket,
                     d_xh_lig, d_xh_pocket);
}
int dsbdd_train_net_backward_acc(dsbdd_train_net* net, void* stream, const dsbdd_train_graph* g, const float* const* params,
                                 float* const* grads, const uint8_t* accumulate, void* pack, size_t pack_bytes, void* ws,
                                 size_t ws_bytes, int64_t e_upd, const float* d_eps_lig, const float* d_eps_pocket,
                                 float* d_xh_lig, float* d_xh_pocket) {
  if (!net) return fail(DSBDD_ERR_ARG, "null handle");
  if (!accumulate) return fail(DSBDD_ERR_ARG, "null accumulate table (one flag per parameter slot)");
  return tn_backward(net, stream, g, params, grads, accumulate, pack, pack_bytes, ws, ws_bytes, e_upd, d_eps_lig, d_eps_pocket,
                     d_xh_lig, d_xh_pocket);
}

// ---- loss terms (loss_head.h) -------------------------------------------------------------------------------------------
int dsbdd_edge_capacity(void* stream, const int64_t* lig_mask, int64_t n_lig, const int64_t* pocket_mask, int64_t n_pocket,
                        int64_t batch, int64_t* out) {
  StreamDevice stream_device_(stream);
  if (!out || batch < 1 || n_lig < 0 || n_pocket < 0 || (n_lig > 0 && !lig_mask) || (n_pocket > 0 && !pocket_mask))
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(edge_capacity_kernel, dim3(1), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(lig_mask), (int)n_lig, reinterpret_cast<const long long*>(pocket_mask),
                     (int)n_pocket, (int)batch, reinterpret_cast<long long*>(out));
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_loss_rows(void) { return LS_ROWS; }
int dsbdd_loss_out_rows(void) { return LO_ROWS; }

int dsbdd_loss_cond_pre(void* stream, const dsbdd_loss_cfg* cfg, const float* lig_x, const float* lig_h, const int64_t* lig_mask,
                        const float* pocket_x, const float* pocket_h, const int64_t* pocket_mask, const float* eps,
                        const float* t_int, const float* gamma_table, const float* logpn_table, float* z_t, float* xh_pocket,
                        float* per_sample, float* lig_x_norm, float* lig_h_norm, float* pocket_x_norm, float* pocket_h_norm) {
  StreamDevice stream_device_(stream);
  if (!loss_cfg_ok(cfg) || !t_int || !gamma_table || !per_sample || (cfg->n_lig > 0 && (!lig_x || !lig_h || !lig_mask || !eps || !z_t)) ||
      (cfg->n_pocket > 0 && (!pocket_x || !pocket_h || !pocket_mask || !xh_pocket)) || (logpn_table && (cfg->n1_tab < 1 || cfg->n2_tab < 1)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(loss_cond_pre_kernel, dim3((unsigned)cfg->batch), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), lig_x, lig_h, reinterpret_cast<const long long*>(lig_mask), pocket_x, pocket_h,
                     reinterpret_cast<const long long*>(pocket_mask), eps, t_int, gamma_table, logpn_table, z_t, xh_pocket, per_sample,
                     lig_x_norm, lig_h_norm, pocket_x_norm, pocket_h_norm);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_loss_cond_post(void* stream, const dsbdd_loss_cfg* cfg, const float* net, const float* eps, const float* z_t,
                         const float* lig_h, const int64_t* lig_mask, const float* per_sample, float* xh_hat, float* out) {
  StreamDevice stream_device_(stream);
  if (!loss_cfg_ok(cfg) || !per_sample || !out || (cfg->n_lig > 0 && (!net || !eps || !z_t || !lig_h || !lig_mask || !xh_hat)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(loss_cond_post_kernel, dim3((unsigned)cfg->batch), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), net, eps, z_t, lig_h, reinterpret_cast<const long long*>(lig_mask), per_sample, xh_hat, out);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_loss_cond_post_backward(void* stream, const dsbdd_loss_cfg* cfg, const float* net, const float* eps, const float* lig_h,
                                  const int64_t* lig_mask, const float* per_sample, const float* g_err, const float* g_l0x,
                                  const float* g_hat, float* d_net) {
  StreamDevice stream_device_(stream);
  if (!loss_cfg_ok(cfg) || !per_sample || (cfg->n_lig > 0 && (!net || !eps || !lig_h || !lig_mask || !d_net)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  if (cfg->n_lig == 0) return DSBDD_OK;
  const size_t n = (size_t)cfg->n_lig * (3 + cfg->atom_nf);
  unsigned grid = (unsigned)((n + kLossThreads - 1) / kLossThreads);
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(loss_cond_post_bwd_kernel, dim3(grid), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), net, eps, lig_h, reinterpret_cast<const long long*>(lig_mask), per_sample, g_err, g_l0x,
                     g_hat, d_net);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

// the joint model: both node sets are noised and scored (cfg->remove_com and cfg->vnode_idx are not read)
int dsbdd_loss_joint_out_rows(void) { return LJ_ROWS; }

int dsbdd_loss_joint_pre(void* stream, const dsbdd_loss_cfg* cfg, const float* lig_x, const float* lig_h, const int64_t* lig_mask,
                         const float* pocket_x, const float* pocket_h, const int64_t* pocket_mask, const float* noise_lig,
                         const float* noise_pocket, const float* t_int, const float* gamma_table, const float* logpn_table,
                         float* eps_lig, float* eps_pocket, float* z_lig, float* z_pocket, float* per_sample, float* lig_x_norm,
                         float* lig_h_norm, float* pocket_x_norm, float* pocket_h_norm) {
  StreamDevice stream_device_(stream);
  if (!loss_cfg_ok(cfg) || !t_int || !gamma_table || !per_sample ||
      (cfg->n_lig > 0 && (!lig_x || !lig_h || !lig_mask || !noise_lig || !eps_lig || !z_lig)) ||
      (cfg->n_pocket > 0 && (!pocket_x || !pocket_h || !pocket_mask || !noise_pocket || !eps_pocket || !z_pocket)) ||
      (logpn_table && (cfg->n1_tab < 1 || cfg->n2_tab < 1)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(loss_joint_pre_kernel, dim3((unsigned)cfg->batch), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), lig_x, lig_h, reinterpret_cast<const long long*>(lig_mask), pocket_x, pocket_h,
                     reinterpret_cast<const long long*>(pocket_mask), noise_lig, noise_pocket, t_int, gamma_table, logpn_table,
                     eps_lig, eps_pocket, z_lig, z_pocket, per_sample, lig_x_norm, lig_h_norm, pocket_x_norm, pocket_h_norm);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_loss_joint_post(void* stream, const dsbdd_loss_cfg* cfg, const float* net_lig, const float* net_pocket,
                          const float* eps_lig, const float* eps_pocket, const float* z_lig, const int64_t* lig_mask,
                          const int64_t* pocket_mask, const float* per_sample, float* xh_lig_hat, float* out) {
  StreamDevice stream_device_(stream);
  if (!loss_cfg_ok(cfg) || !per_sample || !out ||
      (cfg->n_lig > 0 && (!net_lig || !eps_lig || !z_lig || !lig_mask || !xh_lig_hat)) ||
      (cfg->n_pocket > 0 && (!net_pocket || !eps_pocket || !pocket_mask)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(loss_joint_post_kernel, dim3((unsigned)cfg->batch), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), net_lig, net_pocket, eps_lig, eps_pocket, z_lig, reinterpret_cast<const long long*>(lig_mask),
                     reinterpret_cast<const long long*>(pocket_mask), per_sample, xh_lig_hat, out);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_loss_joint_post_backward(void* stream, const dsbdd_loss_cfg* cfg, const float* net_lig, const float* net_pocket,
                                   const float* eps_lig, const float* eps_pocket, const int64_t* lig_mask,
                                   const int64_t* pocket_mask, const float* per_sample, const float* g_err_lig,
                                   const float* g_err_pocket, const float* g_l0x_lig, const float* g_l0x_pocket,
                                   const float* g_xh_lig_hat, float* d_net_lig, float* d_net_pocket) {
  StreamDevice stream_device_(stream);
  if (!loss_cfg_ok(cfg) || !per_sample || (cfg->n_lig > 0 && (!net_lig || !eps_lig || !lig_mask || !d_net_lig)) ||
      (cfg->n_pocket > 0 && (!net_pocket || !eps_pocket || !pocket_mask || !d_net_pocket)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  const size_t n = (size_t)cfg->n_lig * (3 + cfg->atom_nf) + (size_t)cfg->n_pocket * (3 + cfg->residue_nf);
  if (n == 0) return DSBDD_OK;
  unsigned grid = (unsigned)((n + kLossThreads - 1) / kLossThreads);
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(loss_joint_post_bwd_kernel, dim3(grid), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), net_lig, net_pocket, eps_lig, eps_pocket, reinterpret_cast<const long long*>(lig_mask),
                     reinterpret_cast<const long long*>(pocket_mask), per_sample, g_err_lig, g_err_pocket, g_l0x_lig, g_l0x_pocket,
                     g_xh_lig_hat, d_net_lig, d_net_pocket);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

// ---- likelihood bound of given ligands (score.h) --------------------------------------------------------------------------
// the chunk of the four score entry points: DSBDD_OK and *ch, or the error
static int score_chunk_of(const dsbdd_loss_cfg* c, int32_t n_slots, int64_t first_state, int64_t chunk_states, int64_t cap_lig,
                          int64_t cap_pocket, ScoreChunk* ch) {
  const int64_t n_states = loss_cfg_ok(c) ? (int64_t)c->batch * n_slots : 0;
  if (!loss_cfg_ok(c) || c->vnode_idx >= 0 || n_slots < 2 || n_states >= (1ll << 31) || first_state < 0 || chunk_states < 1 ||
      first_state + chunk_states > n_states || cap_lig < 0 || cap_pocket < 0 || cap_lig >= (1ll << 24) || cap_pocket >= (1ll << 24))
    return fail(DSBDD_ERR_ARG, "bad configuration or chunk (virtual atoms are not supported; n_slots >= 2; the chunk lies inside "
                               "the batch * n_slots states)");
  *ch = ScoreChunk{n_slots, (int)first_state, (int)n_states, (int)cap_lig, (int)cap_pocket};
  return DSBDD_OK;
}

int dsbdd_score_rows(int32_t which) { return which == 0 ? SS_ROWS : which == 1 ? SL_ROWS : which == 2 ? SO_ROWS : 0; }

int dsbdd_score_cond_pre(void* stream, const dsbdd_loss_cfg* cfg, int32_t n_slots, int64_t first_state, int64_t chunk_states,
                         int64_t cap_lig, int64_t cap_pocket, const float* lig_x, const float* lig_h, const int64_t* lig_mask,
                         const float* pocket_x, const float* pocket_h, const int64_t* pocket_mask, const float* eps,
                         const float* t_int, const float* gamma_table, const float* logpn_table, float* z, float* xh_pocket,
                         int64_t* mask_lig_out, int64_t* mask_pocket_out, float* t_out, float* per_state, float* per_ligand) {
  StreamDevice stream_device_(stream);
  ScoreChunk ch;
  if (const int err = score_chunk_of(cfg, n_slots, first_state, chunk_states, cap_lig, cap_pocket, &ch)) return err;
  if (!t_int || !gamma_table || !logpn_table || cfg->n1_tab < 1 || cfg->n2_tab < 1 || !t_out || !per_state || !per_ligand ||
      (cfg->n_lig > 0 && (!lig_x || !lig_h || !lig_mask || !eps || !z || !mask_lig_out)) ||
      (cfg->n_pocket > 0 && (!pocket_x || !pocket_h || !pocket_mask || !xh_pocket || !mask_pocket_out)))
    return fail(DSBDD_ERR_ARG, "null argument");
  hipLaunchKernelGGL(score_cond_pre_kernel, dim3((unsigned)chunk_states), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), ch, lig_x, lig_h, reinterpret_cast<const long long*>(lig_mask), pocket_x, pocket_h,
                     reinterpret_cast<const long long*>(pocket_mask), eps, t_int, gamma_table, logpn_table, z, xh_pocket,
                     reinterpret_cast<long long*>(mask_lig_out), reinterpret_cast<long long*>(mask_pocket_out), t_out, per_state,
                     per_ligand);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_score_cond_post(void* stream, const dsbdd_loss_cfg* cfg, int32_t n_slots, int64_t first_state, int64_t chunk_states,
                          int64_t cap_lig, int64_t cap_pocket, const float* lig_h, const int64_t* lig_mask,
                          const int64_t* pocket_mask, const float* net, const float* eps, const float* z, float* per_state) {
  StreamDevice stream_device_(stream);
  ScoreChunk ch;
  if (const int err = score_chunk_of(cfg, n_slots, first_state, chunk_states, cap_lig, cap_pocket, &ch)) return err;
  if (!per_state || (cfg->n_lig > 0 && (!lig_h || !lig_mask || !net || !eps || !z)) || (cfg->n_pocket > 0 && !pocket_mask))
    return fail(DSBDD_ERR_ARG, "null argument");
  hipLaunchKernelGGL(score_cond_post_kernel, dim3((unsigned)chunk_states), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), ch, lig_h, reinterpret_cast<const long long*>(lig_mask),
                     reinterpret_cast<const long long*>(pocket_mask), net, eps, z, per_state);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_score_reduce(void* stream, int64_t batch, int32_t n_slots, const float* weights, const float* per_state,
                       const float* per_ligand, float* out) {
  StreamDevice stream_device_(stream);
  if (batch < 1 || n_slots < 2 || batch * n_slots >= (1ll << 31) || !weights || !per_state || !per_ligand || !out)
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream),
                     (int)batch, (int)n_slots, weights, per_state, per_ligand, out);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

// ---- the same bound under the joint model: both node sets noised and scored (score_joint.h) ---------------------------------
int dsbdd_score_joint_rows(int32_t which) { return which == 0 ? SJ_ROWS : which == 1 ? SL_ROWS : which == 2 ? SJO_ROWS : 0; }

int dsbdd_score_joint_pre(void* stream, const dsbdd_loss_cfg* cfg, int32_t n_slots, int64_t first_state, int64_t chunk_states,
                          int64_t cap_lig, int64_t cap_pocket, int32_t center, const float* lig_x, const float* lig_h,
                          const int64_t* lig_mask, const float* pocket_x, const float* pocket_h, const int64_t* pocket_mask,
                          const float* noise_lig, const float* noise_pocket, const float* t_int, const float* gamma_table,
                          const float* logpn_table, float* eps_lig, float* eps_pocket, float* z_lig, float* z_pocket,
                          int64_t* mask_lig_out, int64_t* mask_pocket_out, float* t_out, float* per_state, float* per_ligand) {
  StreamDevice stream_device_(stream);
  ScoreChunk ch;
  if (const int err = score_chunk_of(cfg, n_slots, first_state, chunk_states, cap_lig, cap_pocket, &ch)) return err;
  if (!t_int || !gamma_table || !logpn_table || cfg->n1_tab < 1 || cfg->n2_tab < 1 || !t_out || !per_state || !per_ligand ||
      (cfg->n_lig > 0 && (!lig_x || !lig_h || !lig_mask || !noise_lig || !eps_lig || !z_lig || !mask_lig_out)) ||
      (cfg->n_pocket > 0 && (!pocket_x || !pocket_h || !pocket_mask || !noise_pocket || !eps_pocket || !z_pocket ||
                             !mask_pocket_out)))
    return fail(DSBDD_ERR_ARG, "null argument");
  hipLaunchKernelGGL(score_joint_pre_kernel, dim3((unsigned)chunk_states), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), ch, (int)(center != 0), lig_x, lig_h, reinterpret_cast<const long long*>(lig_mask), pocket_x,
                     pocket_h, reinterpret_cast<const long long*>(pocket_mask), noise_lig, noise_pocket, t_int, gamma_table,
                     logpn_table, eps_lig, eps_pocket, z_lig, z_pocket, reinterpret_cast<long long*>(mask_lig_out),
                     reinterpret_cast<long long*>(mask_pocket_out), t_out, per_state, per_ligand);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_score_joint_post(void* stream, const dsbdd_loss_cfg* cfg, int32_t n_slots, int64_t first_state, int64_t chunk_states,
                           int64_t cap_lig, int64_t cap_pocket, const float* lig_h, const int64_t* lig_mask, const float* pocket_h,
                           const int64_t* pocket_mask, const float* net_lig, const float* net_pocket, const float* eps_lig,
                           const float* eps_pocket, const float* z_lig, const float* z_pocket, float* per_state) {
  StreamDevice stream_device_(stream);
  ScoreChunk ch;
  if (const int err = score_chunk_of(cfg, n_slots, first_state, chunk_states, cap_lig, cap_pocket, &ch)) return err;
  if (!per_state || (cfg->n_lig > 0 && (!lig_h || !lig_mask || !net_lig || !eps_lig || !z_lig)) ||
      (cfg->n_pocket > 0 && (!pocket_h || !pocket_mask || !net_pocket || !eps_pocket || !z_pocket)))
    return fail(DSBDD_ERR_ARG, "null argument");
  hipLaunchKernelGGL(score_joint_post_kernel, dim3((unsigned)chunk_states), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), ch, lig_h, reinterpret_cast<const long long*>(lig_mask), pocket_h,
                     reinterpret_cast<const long long*>(pocket_mask), net_lig, net_pocket, eps_lig, eps_pocket, z_lig, z_pocket,
                     per_state);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_score_joint_reduce(void* stream, int64_t batch, int32_t n_slots, const float* weights, const float* per_state,
                             const float* per_ligand, float* out) {
  StreamDevice stream_device_(stream);
  if (batch < 1 || n_slots < 2 || batch * n_slots >= (1ll << 31) || !weights || !per_state || !per_ligand || !out)
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(score_joint_reduce_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream),
                     (int)batch, (int)n_slots, weights, per_state, per_ligand, out);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

}  // extern "C"

struct dsbdd_optim {
  dsbdd_optim_cfg cfg;
  std::vector<int64_t> numel, offset;     // per tensor; offsets into the flat m / v / vmax buffers (multiples of 4)
  std::vector<int> chunk_first;           // first chunk of every tensor, [n + 1]
  std::vector<OptimChunk> chunks;
  int64_t flat_elems = 0;
  float *m = nullptr, *v = nullptr, *vmax = nullptr;
  OptimChunk* d_chunks = nullptr;
  float** d_params = nullptr;
  double *d_partial = nullptr, *d_queue = nullptr, *d_scratch = nullptr;
  bool bound = false, has_params = false;
  int64_t n_steps = 0;                    // optimiser steps so far: its parity selects the queue that is read
  int n_cu = 256;
};

struct OptimWs { size_t chunks, params, partial, queue, scratch, total; };
static OptimWs optim_carve(const dsbdd_optim* o) {
  OptimWs w;
  size_t off = 0;
  w.chunks = off; off += al256(o->chunks.size() * sizeof(OptimChunk));
  w.params = off; off += al256(o->numel.size() * sizeof(float*));
  w.partial = off; off += al256(o->chunks.size() * sizeof(double));
  w.queue = off; off += al256(2 * kQueueStride * sizeof(double));
  w.scratch = off; off += 256;
  w.total = off;
  return w;
}

extern "C" {

int dsbdd_optim_create(const dsbdd_optim_cfg* cfg, int32_t n_tensors, const int64_t* numel, dsbdd_optim** out) {
  if (!cfg || !numel || !out || n_tensors < 1) return fail(DSBDD_ERR_ARG, "bad argument");
  if (!(cfg->lr >= 0.0) || !(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0) || !(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0) ||
      !(cfg->eps >= 0.0) || !(cfg->weight_decay >= 0.0))
    return fail(DSBDD_ERR_ARG, "bad hyper-parameter");
  if (1.0 - cfg->beta1 >= 0.5) return fail(DSBDD_ERR_ARG, "beta1 must be above 0.5 (lerp branch of the update kernel)");
  dsbdd_optim* o = new dsbdd_optim();
  o->cfg = *cfg;
  int64_t flat = 0;
  for (int i = 0; i < n_tensors; ++i) {
    if (numel[i] < 1) { delete o; return fail(DSBDD_ERR_ARG, "empty tensor " + std::to_string(i)); }
    o->numel.push_back(numel[i]);
    o->offset.push_back(flat);
    o->chunk_first.push_back((int)o->chunks.size());
    for (int64_t e = 0; e < numel[i]; e += kOptimChunk) {
      const int64_t cnt = numel[i] - e < kOptimChunk ? numel[i] - e : kOptimChunk;
      if (flat + e + cnt >= (1ll << 31)) { delete o; return fail(DSBDD_ERR_ARG, "more than 2^31 parameters"); }
      o->chunks.push_back(OptimChunk{i, (int)e, (int)cnt, (int)(flat + e)});
    }
    flat += (numel[i] + 3) & ~(int64_t)3;
  }
  o->chunk_first.push_back((int)o->chunks.size());
  o->flat_elems = flat;
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
    o->n_cu = prop.multiProcessorCount;
  else
    (void)hipGetLastError();
  *out = o;
  return DSBDD_OK;
}

void dsbdd_optim_destroy(dsbdd_optim* o) { delete o; }

int64_t dsbdd_optim_state_elems(const dsbdd_optim* o) { return o ? o->flat_elems : 0; }
int64_t dsbdd_optim_state_offset(const dsbdd_optim* o, int32_t tensor) {
  return (o && tensor >= 0 && tensor < (int)o->offset.size()) ? o->offset[tensor] : -1;
}
size_t dsbdd_optim_workspace_bytes(const dsbdd_optim* o) { return o ? optim_carve(o).total : 0; }

static void optim_queue_image(double* q, const double* items, int n, double clips, double steps) {
  for (int i = 0; i < kQueueStride; ++i) q[i] = 0.0;
  for (int i = 0; i < n; ++i) q[i] = items[n - 1 - i];         // items arrive newest first (utils.Queue.items); slot 0 = oldest
  q[QS_LEN] = (double)n;
  q[QS_HEAD] = (double)(n == kQueueLen ? 0 : n);
  q[QS_CLIPS] = clips;
  q[QS_STEPS] = steps;
}

int dsbdd_optim_bind(dsbdd_optim* o, void* stream, float* m, float* v, float* vmax, void* ws, size_t ws_bytes) {
  StreamDevice stream_device_(stream);
  if (!o || !m || !v || !vmax || !ws) return fail(DSBDD_ERR_ARG, "null argument");
  if ((reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(vmax)) & 15)
    return fail(DSBDD_ERR_ARG, "state buffers must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(DSBDD_ERR_ARG, "workspace must be 256-byte aligned");
  const OptimWs w = optim_carve(o);
  if (ws_bytes < w.total) return fail(DSBDD_ERR_CAPACITY, "workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* b = static_cast<char*>(ws);
  o->m = m; o->v = v; o->vmax = vmax;
  o->d_chunks = reinterpret_cast<OptimChunk*>(b + w.chunks);
  o->d_params = reinterpret_cast<float**>(b + w.params);
  o->d_partial = reinterpret_cast<double*>(b + w.partial);
  o->d_queue = reinterpret_cast<double*>(b + w.queue);
  o->d_scratch = reinterpret_cast<double*>(b + w.scratch);
  double q[2 * kQueueStride];
  const double first = 3000.0;                                  // "Add large value that will be flushed."
  optim_queue_image(q, &first, 1, 0.0, 0.0);
  optim_queue_image(q + kQueueStride, &first, 1, 0.0, 0.0);
  HIP_TRY(hipMemcpyAsync(o->d_chunks, o->chunks.data(), o->chunks.size() * sizeof(OptimChunk), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(o->d_queue, q, sizeof(q), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(o->d_partial, 0, o->chunks.size() * sizeof(double), s));
  HIP_TRY(hipMemsetAsync(o->d_scratch, 0, 256, s));
  HIP_TRY(hipStreamSynchronize(s));                             // the sources are host temporaries
  o->n_steps = 0;
  o->bound = true;
  o->has_params = false;
  return DSBDD_OK;
}

int dsbdd_optim_set_params(dsbdd_optim* o, void* stream, float* const* params) {
  StreamDevice stream_device_(stream);
  if (!o || !params) return fail(DSBDD_ERR_ARG, "null argument");
  if (!o->bound) return fail(DSBDD_ERR_STATE, "optimiser state not bound");
  for (size_t i = 0; i < o->numel.size(); ++i)
    if (!params[i] || (reinterpret_cast<uintptr_t>(params[i]) & 3))
      return fail(DSBDD_ERR_ARG, "parameter " + std::to_string(i) + " is null or misaligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpyAsync(o->d_params, params, o->numel.size() * sizeof(float*), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  o->has_params = true;
  return DSBDD_OK;
}

// R == nullptr: launch 1 is optim_norm_kernel on the caller's gradients (skipped without clipping); else
// optim_reduce_norm_kernel folds the ranks' buckets into R->out first (always launched: the reduce is needed either way)
static int optim_step_impl(dsbdd_optim* o, void* stream, const float* const* grads, const int32_t* steps, double lr,
                           const OptimRanks* R) {
  StreamDevice stream_device_(stream);
  if (!o || !grads || !steps) return fail(DSBDD_ERR_ARG, "null argument");
  if (!o->bound || !o->has_params) return fail(DSBDD_ERR_STATE, "optimiser state or parameters not bound");
  if (!(lr >= 0.0)) return fail(DSBDD_ERR_ARG, "bad learning rate");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = (int)o->numel.size();
  const dsbdd_optim_cfg& c = o->cfg;
  OptimLaunch L{};
  L.chunks = o->d_chunks; L.n_chunks = (int)o->chunks.size(); L.params = o->d_params;
  L.m = o->m; L.v = o->v; L.vmax = o->vmax; L.partial = o->d_partial; L.queue = o->d_queue; L.scratch = o->d_scratch;
  L.parity = (int)(o->n_steps & 1); L.clip = c.clip_grad ? 1 : 0;
  // the scalars torch derives in Python doubles and hands to float32 kernels
  L.decay = (float)(1.0 - lr * c.weight_decay); L.w1 = (float)(1.0 - c.beta1); L.beta2 = (float)c.beta2;
  L.w2 = (float)(1.0 - c.beta2); L.eps = (float)c.eps;
  for (int pass = (c.clip_grad || R) ? 0 : 1; pass < 2; ++pass) {
    for (int lo = 0; lo < n; lo += kOptimTensors) {
      const int hi = lo + kOptimTensors < n ? lo + kOptimTensors : n;
      OptimStepArgs A{};
      for (int i = lo; i < hi; ++i) {
        A.grad[i - lo] = grads[i];
        if (!grads[i]) continue;
        if (steps[i] < 1) return fail(DSBDD_ERR_ARG, "step count of tensor " + std::to_string(i) + " must be >= 1");
        if (reinterpret_cast<uintptr_t>(grads[i]) & 3) return fail(DSBDD_ERR_ARG, "misaligned gradient");
        const double bc1 = 1.0 - std::pow(c.beta1, (double)steps[i]), bc2 = 1.0 - std::pow(c.beta2, (double)steps[i]);
        A.step_size_neg[i - lo] = (float)(-(lr / bc1));
        A.bc2_sqrt[i - lo] = (float)std::pow(bc2, 0.5);
      }
      L.tensor_lo = lo; L.chunk_lo = o->chunk_first[lo]; L.chunk_hi = o->chunk_first[hi]; L.first = lo == 0;
      int grid = L.chunk_hi - L.chunk_lo;
      if (grid > 2 * o->n_cu) grid = 2 * o->n_cu;
      if (grid < 1) grid = 1;
      if (pass == 0 && R) hipLaunchKernelGGL(optim_reduce_norm_kernel, dim3(grid), dim3(kOptimThreads), 0, s, L, A, *R);
      else if (pass == 0) hipLaunchKernelGGL(optim_norm_kernel, dim3(grid), dim3(kOptimThreads), 0, s, L, A);
      else hipLaunchKernelGGL(optim_update_kernel, dim3(grid), dim3(kOptimThreads), 0, s, L, A);
      HIP_TRY(hipGetLastError());
    }
  }
  if (c.clip_grad) ++o->n_steps;
  return DSBDD_OK;
}

int dsbdd_optim_step(dsbdd_optim* o, void* stream, const float* const* grads, const int32_t* steps, double lr) {
  return optim_step_impl(o, stream, grads, steps, lr, nullptr);
}

int dsbdd_optim_step_ranks(dsbdd_optim* o, void* stream, const float* gathered, int64_t rank_stride, int32_t n_ranks,
                           float* out_flat, const float* const* grads, const int32_t* steps, double lr) {
  if (!o || !gathered || !out_flat || !grads) return fail(DSBDD_ERR_ARG, "null argument");
  if (n_ranks < 1 || n_ranks > 4096) return fail(DSBDD_ERR_ARG, "n_ranks must be 1 to 4096");
  if (n_ranks > 1 && rank_stride < o->flat_elems) return fail(DSBDD_ERR_ARG, "rank_stride is shorter than one bucket");
  if ((reinterpret_cast<uintptr_t>(gathered) | reinterpret_cast<uintptr_t>(out_flat)) & 3) return fail(DSBDD_ERR_ARG, "misaligned bucket");
  for (size_t i = 0; i < o->numel.size(); ++i)
    if (grads[i] && grads[i] != out_flat + o->offset[i])
      return fail(DSBDD_ERR_ARG, "gradient " + std::to_string(i) + " is not its region of out_flat (dsbdd_optim_state_offset)");
  const OptimRanks R{gathered, (long long)rank_stride, (int)n_ranks, out_flat};
  return optim_step_impl(o, stream, grads, steps, lr, &R);
}

int dsbdd_optim_state_read(dsbdd_optim* o, void* stream, double* out, int32_t capacity) {
  StreamDevice stream_device_(stream);
  if (!o || !out || capacity < kQueueStride) return fail(DSBDD_ERR_ARG, "bad argument");
  if (!o->bound) return fail(DSBDD_ERR_STATE, "optimiser state not bound");
  hipStream_t s = static_cast<hipStream_t>(stream);
  double q[kQueueStride];
  HIP_TRY(hipMemcpyAsync(q, o->d_queue + (o->n_steps & 1) * kQueueStride, sizeof(q), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // out: [0] number of entries, [1 .. 50] the entries newest first, then clips, last norm, last threshold, steps, last coefficient
  int len = (int)q[QS_LEN], head = (int)q[QS_HEAD];
  if (len < 0 || len > kQueueLen || head < 0 || head >= kQueueLen) return fail(DSBDD_ERR_STATE, "corrupt queue record");
  for (int i = 0; i < kQueueStride; ++i) out[i] = 0.0;
  out[0] = (double)len;
  for (int i = 0; i < len; ++i) out[1 + i] = q[(head - 1 - i + 2 * kQueueLen) % kQueueLen];
  out[51] = q[QS_CLIPS]; out[52] = q[QS_LAST_NORM]; out[53] = q[QS_LAST_MAX]; out[54] = q[QS_STEPS]; out[55] = q[QS_LAST_COEF];
  return DSBDD_OK;
}

int dsbdd_optim_state_write(dsbdd_optim* o, void* stream, const double* items, int32_t n_items, double clips, double steps) {
  StreamDevice stream_device_(stream);
  if (!o || !items || n_items < 1 || n_items > kQueueLen) return fail(DSBDD_ERR_ARG, "the queue holds 1 to 50 entries");
  if (!o->bound) return fail(DSBDD_ERR_STATE, "optimiser state not bound");
  hipStream_t s = static_cast<hipStream_t>(stream);
  double q[kQueueStride];
  optim_queue_image(q, items, n_items, clips, steps);
  HIP_TRY(hipMemcpyAsync(o->d_queue + (o->n_steps & 1) * kQueueStride, q, sizeof(q), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DSBDD_OK;
}

int dsbdd_lj_potential(void* stream, const float* xh, int32_t ld, int32_t n_types, const int64_t* mask, int64_t n, int64_t batch,
                       const double* sigma, double clamp, int32_t has_clamp, int32_t* type_scratch, float* u, float* dx) {
  StreamDevice stream_device_(stream);
  if (batch < 1 || n < 0 || n >= (1ll << 30) || n_types < 1 || ld < 3 + n_types || !sigma || !u ||
      (n > 0 && (!xh || !mask || !type_scratch || !dx)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  LjArgs a{xh, ld, n_types, reinterpret_cast<const long long*>(mask), (int)n, (int)batch, sigma, clamp, has_clamp, type_scratch, u, dx};
  hipLaunchKernelGGL(lj_potential_kernel, dim3((unsigned)batch), dim3(kLjThreads), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

}  // extern "C"
