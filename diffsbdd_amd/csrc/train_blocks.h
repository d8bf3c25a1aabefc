// Training-step building blocks (host side of csrc/train.h and csrc/wgrad.h; included by engine.hip in front of
// train_net.h): weight gradients, the edge-stage scratch, side streams, and the forward / backward of one message or
// coordinate stage.  The dsbdd_train_* entry points over them are in train_api.h.
#pragma once

// out[i] = sum_p part[p * stride + i] in a fixed order (two levels above 64 parts); tmp: ceil(n_part / 32) * width floats.
// acc: out[i] += that sum, folded into the LAST level's store (the accumulating parameter gradients of train_net.h)
static hipError_t reduce_parts(hipStream_t s, const float* part, int n_part, size_t stride, int width, float* out,
                               float* tmp, bool acc = false) {
  const int bx = (width + 255) / 256;
  if (n_part <= 96) {
    hipLaunchKernelGGL(partial_reduce_kernel, dim3(bx, 1), dim3(256), 0, s, part, n_part, stride, width,
                       n_part > 0 ? n_part : 1, out, (size_t)0, acc ? 1 : 0);
    return hipGetLastError();
  }
  const int groups = (n_part + 31) / 32;
  hipLaunchKernelGGL(partial_reduce_kernel, dim3(bx, groups), dim3(256), 0, s, part, n_part, stride, width, 32, tmp,
                     (size_t)width, 0);
  hipLaunchKernelGGL(partial_reduce_kernel, dim3(bx, 1), dim3(256), 0, s, (const float*)tmp, groups, (size_t)width,
                     width, groups, out, (size_t)0, acc ? 1 : 0);
  return hipGetLastError();
}

struct WgradPlan { int chunks, kc; size_t floats; };
// upper bound of the chunk count of wgrad_plan(K', M, N) for every K' <= K: min(ceil(K / min_kc), cap), at least 1
static int64_t wgrad_chunk_bound(int64_t K, int64_t M, int64_t N) {
  // short chunks for the node-level gradients (K = a few thousand rows: the launch is a latency chain), at most
  // 256 / tiles chunks for the edge-level ones: <= 96 partial slabs reduce in ONE ordered launch (round 6: 768 -> 256,
  // 14.46 -> 14.03 ms per training step, profiles/r6_train_step.md; round 4's sweep had preferred 768 when the reduction
  // was two launches either way)
  static const int min_kc = env_int_in("DSBDD_WGRAD_MINKC", 32, INT_MAX, 64);      // (read once, on first use)
  static const int max_wg = env_int_in("DSBDD_WGRAD_MAXWG", 1, INT_MAX, 256);
  const int64_t tiles = ((M + 127) / 128) * ((N + 127) / 128);
  const int64_t cap = max_wg / tiles > 1 ? max_wg / tiles : 1;
  int64_t chunks = (K + min_kc - 1) / min_kc;
  if (chunks > cap) chunks = cap;
  return chunks < 1 ? 1 : chunks;
}
static WgradPlan wgrad_plan(int64_t K, int64_t M, int64_t N) {
  int64_t chunks = wgrad_chunk_bound(K, M, N);
  int64_t kc = ((K + chunks - 1) / chunks + 31) / 32 * 32;
  if (kc < 32) kc = 32;
  chunks = (K + kc - 1) / kc;
  if (chunks < 1) chunks = 1;
  WgradPlan p{(int)chunks, (int)kc, 0};
  p.floats = (size_t)chunks * M * N + (size_t)((chunks + 31) / 32) * M * N;
  return p;
}
// Scratch floats that cover wgrad_plan(K, M, N) for EVERY K <= K_max.  The plan is not monotonic in K (kc is rounded up
// to a multiple of 32 after the chunk cap, so a smaller K can end with more chunks: K = 160 000 -> 186, K = 30 000 -> 188
// at 256 x 256), but its chunk count never exceeds the bound above, which is.  (the coordinate
// stage's backward calls wgrad with K = e_upd < E on a scratch sized for E.)
static size_t wgrad_floats_upto(int64_t K_max, int64_t M, int64_t N) {
  const int64_t chunks = wgrad_chunk_bound(K_max, M, N);
  return (size_t)chunks * M * N + (size_t)((chunks + 31) / 32) * M * N;
}

static int wgrad_impl(hipStream_t s, const float* A, int lda, const float* B, int ldb, int64_t K, int M, int N, float* C,
                      float* scratch, size_t scratch_floats, bool acc = false) {
  const WgradPlan pl = wgrad_plan(K, M, N);
  if (pl.floats > scratch_floats) return fail(DSBDD_ERR_CAPACITY, "weight-gradient scratch too small for this plan");
  WgradArgs a{A, lda, B, ldb, (int)K, M, N, scratch, pl.kc};
  hipLaunchKernelGGL(wgrad_kernel, dim3((M + 127) / 128, (N + 127) / 128, pl.chunks), dim3(kThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(reduce_parts(s, scratch, pl.chunks, (size_t)M * N, M * N, C, scratch + (size_t)pl.chunks * M * N, acc));
  return DSBDD_OK;
}

struct TrainScratch {
  float *dz2, *a1, *dz1, *partA, *partB, *rtmp, *wg, *gd, *gxr, *gxc, *gm, *agg_head, *xagg, *xagg_head, *vec;
  size_t bytes, wg_floats;
};
static int train_grid(int64_t E) {
  // persistent workgroups of the backward edge kernels per CU (DSBDD_TRAIN_WG_PER_CU, default 1; the kernels fit two:
  // 256 VGPRs, 74 KB of LDS)
  static const int per_cu = env_int_in("DSBDD_TRAIN_WG_PER_CU", 1, 4, 1);
  return persistent_grid((E + 127) / 128, device_cus(), per_cu, 0, 1);
}
static TrainScratch carve_train(char* base, int H, int64_t N, int64_t E) {
  TrainScratch t{};
  Carver cv{base};
  const size_t EH = (size_t)(E > 0 ? E : 1) * H, E3 = 3 * (size_t)E + 4, tiles = (size_t)((E + 31) / 32 + 2);
  const size_t slots = 256 * 8, PH = (size_t)kPartAll * H;
  t.dz2 = cv.f(EH); t.a1 = cv.f(EH); t.dz1 = cv.f(EH);
  t.partA = cv.f(slots * PH); t.partB = t.partA;          // one [8][H] slot per workgroup for both kernels
  t.rtmp = cv.f((slots / 32 + 1) * PH);
  t.wg_floats = wgrad_floats_upto(E > N ? E : N, H, H);   // any K <= max(E, N): the coordinate stage runs on an edge prefix
  t.wg = cv.f(t.wg_floats);
  t.gd = cv.f(E + 1); t.gxr = cv.f(E3); t.gxc = cv.f(E3); t.gm = cv.f(E3);
  t.agg_head = cv.f(tiles * H);
  t.xagg = cv.f(2 * (3 * (size_t)N + 4)); t.xagg_head = cv.f(2 * 4 * tiles);   // one sum per MLP (pass split)
  t.vec = cv.f(8 * (size_t)H);
  t.bytes = cv.off;
  return t;
}

static hipError_t launch_bwd_a(int H, hipStream_t s, int mode, const TrainEdgeArgs& a, int grid) {
  return with_hidden(H, [&](auto h) {
    constexpr int HH = decltype(h)::value;
    if (mode == MODE_GCL) hipLaunchKernelGGL((edge_bwd_a_kernel<HH, MODE_GCL>), dim3(grid), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((edge_bwd_a_kernel<HH, MODE_COORD>), dim3(grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
  });
}
static hipError_t launch_bwd_b(int H, hipStream_t s, const TrainEdgeArgs& a, int grid) {
  return with_hidden(H, [&](auto h) {
    hipLaunchKernelGGL((edge_bwd_b_kernel<decltype(h)::value>), dim3(grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
  });
}
static hipError_t launch_bwd_e(int H, hipStream_t s, int mode, const TrainEdgeArgs& a, const float* z2, int grid) {
  return with_hidden(H, [&](auto h) {
    constexpr int HH = decltype(h)::value;
    if (mode == MODE_GCL) hipLaunchKernelGGL((edge_bwd_e_kernel<HH, MODE_GCL>), dim3(grid), dim3(kThreadsE), 0, s, a, z2);
    else hipLaunchKernelGGL((edge_bwd_e_kernel<HH, MODE_COORD>), dim3(grid), dim3(kThreadsE), 0, s, a, z2);
    return hipGetLastError();
  });
}

static bool graph_ok(const dsbdd_train_graph* g) {
  return g && g->erow && g->ecol && g->ed0 && g->row_ptr && g->deg && g->node_batch && g->lig_off && g->poc_off &&
         g->n_nodes > 0 && g->n_edges >= 0 && g->batch > 0 && g->n_lig >= 0 && g->n_lig <= g->n_nodes;
}
static bool mlp_ok(const dsbdd_train_mlp* m) {
  return m && m->P && m->Q && m->wd && m->wd0 && m->tab && m->W2 && m->W2T && m->b2 && (m->ldpq & 3) == 0;
}

// Side streams of the training backward (round 6, dsbdd_train_net_backward only).  The weight gradients leave the
// dependency chain of the input gradients, and the two edge MLPs of a coordinate stage are independent of each other:
// `wg` takes the weight-gradient launches, `co` the second MLP's chain, fork / join by events.  Every kernel and every
// reduction order is the one of the single-stream sequence (DSBDD_TRAIN_STREAMS=0), so the gradients keep their bits.
enum { SIDE_CO = 1, SIDE_NODE_WG = 2, SIDE_COORD_WG = 4, SIDE_GCL_WG = 8 };
struct TrainSide {
  hipStream_t wg = nullptr, co = nullptr;
  int mask = 0;                  // SIDE_* : what runs beside the main chain
  int device = -1;               // the device the streams live on (a module moved to another GPU gets new ones)
  hipEvent_t w2_done[2] = {nullptr, nullptr};   // after the last W2 weight gradient queued on `wg` that reads scratch set q
  bool w2_valid[2] = {false, false};
  std::vector<hipEvent_t> ev;
  size_t next = 0;
  // everything queued on `to` after this call starts after everything queued on `from` before it
  hipError_t link(hipStream_t from, hipStream_t to) {
    hipEvent_t e = ev[next++ % ev.size()];
    const hipError_t r = hipEventRecord(e, from);
    return r != hipSuccess ? r : hipStreamWaitEvent(to, e, 0);
  }
  hipError_t create() {
    hipError_t r = hipGetDevice(&device);
    if (r == hipSuccess) r = hipStreamCreateWithFlags(&wg, hipStreamNonBlocking);
    if (r == hipSuccess) r = hipStreamCreateWithFlags(&co, hipStreamNonBlocking);
    ev.resize(32);
    for (size_t i = 0; r == hipSuccess && i < ev.size(); ++i) r = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
    for (int q = 0; r == hipSuccess && q < 2; ++q) r = hipEventCreateWithFlags(&w2_done[q], hipEventDisableTiming);
    w2_valid[0] = w2_valid[1] = false;
    return r;
  }
  void destroy() {
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    ev.clear();
    for (int q = 0; q < 2; ++q) { if (w2_done[q]) (void)hipEventDestroy(w2_done[q]); w2_done[q] = nullptr; w2_valid[q] = false; }
    if (wg) (void)hipStreamDestroy(wg);
    if (co) (void)hipStreamDestroy(co);
    wg = co = nullptr;
  }
};

// the backward of ONE edge MLP: kernel A / E -> weight gradient -> kernel B -> node gathers; returns the per-edge gradient
// w.r.t. the current squared distance in ts.gd.  `o.side` (optional) -- what waits for what:
//   * kernel A / E overwrites ts.dz2 / ts.a1 of scratch set `o.scratch_set`: it waits for the last W2 weight gradient that read this
//     set on the side stream (its own event), NOT for the whole side stream -- the node-level weight gradients queued there
//     keep running beside the memory-bound kernel E (waiting for them cost the main chain 60 - 70 us per stage);
//   * the message stage's W2 gradient stays on this stream and is preceded by a FULL join of the side stream: it streams
//     373 MB and runs 1.6 x longer with anything beside it, and the join is the one point per block that covers the
//     caller's hazards: the node-level weight and bias gradients that TrainBackward (train_net.h) queued on the side
//     streams read dout, dz / xcat and d_pq / d_pq4.  dout is overwritten by the message stage's last tn_lin, dz / xcat
//     by the next sublayer, d_pq / d_pq4 by the node gathers below -- all of them after this join;
//   * a coordinate stage's W2 gradient goes to the side stream and records the set's event.
struct MlpBwdOpts {
  TrainSide* side = nullptr;      // the side streams, or none
  bool already_linked = false;    // the caller joined / forked the side streams itself (coordinate stage)
  const float* z2 = nullptr;      // the second-layer pre-activations the forward pass kept, or null: recompute (kernel A)
  int scratch_set = 0;            // which of the two scratch sets `ts` is (the W2 gradient's event)
  bool acc_w2 = false;            // out->d_W2 += the gradient instead of = (dsbdd_train_net_backward_acc)
};
static int mlp_backward(hipStream_t s, int H, int mode, const dsbdd_train_graph* g, const dsbdd_train_mlp* m, const float* x,
                        int64_t E, TrainEdgeArgs a, const dsbdd_train_mlp_grad* out, const TrainScratch& ts,
                        const MlpBwdOpts& o = {}) {
  TrainSide* const sd = o.side;
  const int grid = train_grid(E);
  const bool side_w = sd && (sd->mask & (mode == MODE_GCL ? SIDE_GCL_WG : SIDE_COORD_WG));
  const bool late_join = sd && mode == MODE_GCL && !side_w;      // the full join sits in front of the W2 gradient instead
  if (sd && !o.already_linked && !late_join) { HIP_TRY(sd->link(sd->wg, s)); HIP_TRY(sd->link(sd->co, s)); }
  if (sd && sd->w2_valid[o.scratch_set]) HIP_TRY(hipStreamWaitEvent(s, sd->w2_done[o.scratch_set], 0));
  const int slots = grid;                  // one partial-vector slot per workgroup
  a.erow = g->erow; a.ecol = g->ecol; a.ed0 = g->ed0; a.E = (int)E; a.x = x; a.n_lig = (int)g->n_lig;
  a.n_nodes = (int)g->n_nodes; a.P = m->P; a.Q = m->Q; a.ldpq = m->ldpq; a.wd = m->wd; a.wd0 = m->wd0; a.table = m->tab;
  a.b2 = m->b2; a.head = m->head; a.head_b = m->head_b;
  a.a1_out = ts.a1; a.gxr = ts.gxr; a.gxc = ts.gxc; a.gd = ts.gd; a.gd0 = out->gd0;
  // A: dz2, a1, partial bias / head vectors
  a.Bmat = m->W2T; a.dz_out = ts.dz2; a.part = ts.partA;
  if (o.z2) HIP_TRY(launch_bwd_e(H, s, mode, a, o.z2, grid));     // the forward pass kept z2: no H x H layer here
  else HIP_TRY(launch_bwd_a(H, s, mode, a, grid));
  // dW2[f][i] = sum_e dz2[e][f] a1[e][i]
  if (side_w) HIP_TRY(sd->link(s, sd->wg));
  if (late_join) { HIP_TRY(sd->link(sd->wg, s)); HIP_TRY(sd->link(sd->co, s)); }
  RC_TRY(wgrad_impl(side_w ? sd->wg : s, ts.dz2, H, ts.a1, H, E, H, H, out->d_W2, ts.wg, ts.wg_floats, o.acc_w2));
  if (side_w) { HIP_TRY(hipEventRecord(sd->w2_done[o.scratch_set], sd->wg)); sd->w2_valid[o.scratch_set] = true; }
  // B: dz1, partial first-layer vectors, per-edge distance gradients
  a.Bmat = m->W2; a.dz_in = ts.dz2; a.dz_out = ts.dz1; a.part = ts.partB;
  HIP_TRY(launch_bwd_b(H, s, a, grid));
  // ONE ordered reduction for both kernels' partial vectors (they share the grid and the [8][H] slots) -> d_vec [8][H]
  HIP_TRY(reduce_parts(s, ts.partB, slots, (size_t)kPartAll * H, kPartAll * H, out->d_vec, ts.rtmp));
  // dP / dQ
  const int N = (int)g->n_nodes;
  hipLaunchKernelGGL(rows_gather_kernel, dim3((N + 3) / 4), dim3(kThreads), 0, s, (const float*)ts.dz1, H, g->row_ptr,
                     g->deg, g->rev, (int)E, N, out->dP, out->dQ, out->ldo);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

// per-sample mean of x over the ligand and pocket rows of every sample (fixed order) -> mean [B][3]
static int sample_mean_impl(hipStream_t s, const float* x, const dsbdd_train_graph* g, float* mean) {
  hipLaunchKernelGGL(sample_mean_kernel, dim3((unsigned)g->batch), dim3(kThreads), 0, s, x, g->lig_off, g->poc_off,
                     (int)g->n_lig, mean);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}
// d_x[i] = sum over the edges at node i of the per-edge gradients gd w.r.t. the squared distances (ordered gather)
static int radial_backward_impl(hipStream_t s, const dsbdd_train_graph* g, const float* x, const float* gd, float* d_x) {
  const int N = (int)g->n_nodes;
  hipLaunchKernelGGL(edge_to_node3_kernel, dim3((N + 3) / 4), dim3(kThreads), 0, s, gd, (const float*)nullptr,
                     (const float*)nullptr, x, g->ecol, g->row_ptr, g->deg, g->rev, (int)g->n_edges, N, d_x, 0);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

static int gcl_forward_impl(void* stream, int32_t H, const dsbdd_train_graph* g, const dsbdd_train_mlp* m, const float* x,
                            float norm_factor, float* agg, void* scratch, size_t scratch_bytes, float* z2_store) {
  StreamDevice stream_device_(stream);
  if (!hidden_nf_ok(H) || !graph_ok(g) || !mlp_ok(m) || !x || !agg || !scratch) return fail(DSBDD_ERR_ARG, "bad argument");
  const TrainScratch ts = carve_train(static_cast<char*>(scratch), H, g->n_nodes, g->n_edges);
  if (ts.bytes > scratch_bytes) return fail(DSBDD_ERR_CAPACITY, "scratch too small (dsbdd_train_scratch_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int N = (int)g->n_nodes;
  EdgeArgs ea{};
  ea.erow = g->erow; ea.ecol = g->ecol; ea.ed0 = g->ed0; ea.e_count = g->row_ptr + N; ea.e_cap = (int)g->n_edges;
  ea.x = x; ea.n_lig = (int)g->n_lig; ea.n_nodes = N; ea.ldpq = m->ldpq;
  ea.mlp[0] = EdgeMlpW{m->P, m->Q, m->wd, m->wd0, m->tab, m->W2T, m->b2, nullptr};
  ea.mlp[1] = ea.mlp[0];
  ea.att_w = m->head; ea.att_b = m->head_b; ea.attention = m->head != nullptr;
  ea.agg = agg; ea.agg_head = ts.agg_head; ea.norm_factor = norm_factor; ea.z2_out = z2_store;
  if (g->n_edges > 0) HIP_TRY(launch_edge_plain(H, s, MODE_GCL, ea, g->n_edges));
  hipLaunchKernelGGL(agg_complete_kernel, dim3((N + 3) / 4), dim3(kThreads), 0, s, agg, (const float*)ts.agg_head,
                     g->row_ptr, g->deg, N, (int)H, (int)((g->n_edges + 31) / 32 + 1), 5);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

static int gcl_backward_impl(void* stream, int32_t H, const dsbdd_train_graph* g, const dsbdd_train_mlp* m, const float* x,
                             float norm_factor, const float* d_agg, const dsbdd_train_mlp_grad* out, float* d_x,
                             void* scratch, size_t scratch_bytes, TrainSide* sd, const float* z2 = nullptr,
                             bool acc_w2 = false) {
  StreamDevice stream_device_(stream);
  if (!hidden_nf_ok(H) || !graph_ok(g) || !g->rev || !mlp_ok(m) || !x || !d_agg || !out || !out->dP || !out->dQ ||
      !out->d_vec || !out->d_W2 || !out->gd0 || (out->ldo & 3) || !d_x || !scratch)
    return fail(DSBDD_ERR_ARG, "bad argument");
  const TrainScratch ts = carve_train(static_cast<char*>(scratch), H, g->n_nodes, g->n_edges);
  if (ts.bytes > scratch_bytes) return fail(DSBDD_ERR_CAPACITY, "scratch too small (dsbdd_train_scratch_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  TrainEdgeArgs a{};
  a.d_agg = d_agg; a.norm_factor = norm_factor;
  MlpBwdOpts o;
  o.side = sd; o.z2 = z2; o.acc_w2 = acc_w2;
  RC_TRY(mlp_backward(s, H, MODE_GCL, g, m, x, g->n_edges, a, out, ts, o));
  return radial_backward_impl(s, g, x, ts.gd, d_x);
}

static int coord_forward_impl(void* stream, int32_t H, const dsbdd_train_graph* g, const dsbdd_train_mlp* m, int32_t n_mlp,
                              const float* x, const float* mean, int64_t n_upd, float norm_constant, float coords_range,
                              int32_t use_tanh, float norm_factor, float* x_out, void* scratch, size_t scratch_bytes,
                              float* z2_store, size_t z2_stride) {
  StreamDevice stream_device_(stream);
  if (!hidden_nf_ok(H) || !graph_ok(g) || n_mlp < 1 || n_mlp > 2 || !mlp_ok(m) || (n_mlp == 2 && (!mlp_ok(m + 1) || !mean)) ||
      !m->head || !x || !x_out || n_upd < 0 || n_upd > g->n_nodes || !scratch)
    return fail(DSBDD_ERR_ARG, "bad argument");
  const TrainScratch ts = carve_train(static_cast<char*>(scratch), H, g->n_nodes, g->n_edges);
  if (ts.bytes > scratch_bytes) return fail(DSBDD_ERR_CAPACITY, "scratch too small (dsbdd_train_scratch_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int N = (int)g->n_nodes;
  HIP_TRY(hipMemcpyAsync(x_out, x, (size_t)N * 12, hipMemcpyDeviceToDevice, s));
  if (n_upd == 0 || g->n_edges == 0) return DSBDD_OK;
  EdgeArgs ea{};
  ea.erow = g->erow; ea.ecol = g->ecol; ea.ed0 = g->ed0; ea.e_count = g->row_ptr + n_upd; ea.e_cap = (int)g->n_edges;
  ea.x = x; ea.n_lig = (int)g->n_lig; ea.n_nodes = N; ea.ldpq = m->ldpq;
  for (int q = 0; q < 2; ++q) {
    const dsbdd_train_mlp& mq = m[q < n_mlp ? q : 0];
    ea.mlp[q] = EdgeMlpW{mq.P, mq.Q, mq.wd, mq.wd0, mq.tab, mq.W2T, mq.b2, nullptr};
  }
  ea.w3 = m->head; ea.node_batch = g->node_batch; ea.mean = mean; ea.norm_constant = norm_constant;
  ea.coords_range = coords_range; ea.use_tanh = use_tanh; ea.n_mlp = n_mlp; ea.xagg = ts.xagg; ea.xagg_head = ts.xagg_head;
  ea.xagg_stride = (size_t)N * 3; ea.xhead_stride = 4 * (size_t)((g->n_edges + 31) / 32 + 2); ea.norm_factor = norm_factor;
  ea.z2_out = z2_store; ea.z2_stride = z2_stride;
  // two MLPs: alternate workgroups take one MLP of a tile each (the updated rows' edge prefix is a fraction of a tile per
  // CU: twice as many, half as long work items), one coordinate sum per MLP, added by coord_update_kernel
  ea.pass_split = n_mlp == 2 ? 1 : 0;
  HIP_TRY(launch_edge_plain(H, s, MODE_COORD, ea, g->n_edges));
  const CoordSums sums{ts.xagg, ts.xagg_head, ea.pass_split ? 2 : 1, ea.xagg_stride, ea.xhead_stride, g->row_ptr, g->deg,
                       (int)((g->n_edges + 31) / 32 + 1), 5};
  return launch_1d(coord_update_kernel, (size_t)(3 * n_upd), s, x_out, sums, (int)(3 * n_upd));
}

static int coord_backward_impl(void* stream, int32_t H, const dsbdd_train_graph* g, const dsbdd_train_mlp* m, int32_t n_mlp,
                               const float* x, const float* mean, int64_t n_upd, int64_t e_upd, float norm_constant,
                               float coords_range, int32_t use_tanh, float norm_factor, const float* d_xout,
                               const dsbdd_train_mlp_grad* out, float* d_x, float* d_mean, void* scratch,
                               size_t scratch_bytes, TrainSide* sd, const float* z2 = nullptr, size_t z2_stride = 0,
                               const bool* acc_w2 = nullptr) {      // acc_w2 [n_mlp]: out[q].d_W2 accumulates
  StreamDevice stream_device_(stream);
  if (!hidden_nf_ok(H) || !graph_ok(g) || !g->rev || n_mlp < 1 || n_mlp > 2 || !mlp_ok(m) ||
      (n_mlp == 2 && (!mlp_ok(m + 1) || !mean || !d_mean)) || !m->head || !x || !d_xout || !out || !d_x || n_upd < 0 ||
      n_upd > g->n_nodes || e_upd < 0 || e_upd > g->n_edges || !scratch)
    return fail(DSBDD_ERR_ARG, "bad argument");
  for (int q = 0; q < n_mlp; ++q)
    if (!out[q].dP || !out[q].dQ || !out[q].d_vec || !out[q].d_W2 || !out[q].gd0 || (out[q].ldo & 3))
      return fail(DSBDD_ERR_ARG, "bad gradient destination");
  const TrainScratch ts = carve_train(static_cast<char*>(scratch), H, g->n_nodes, g->n_edges);
  if (ts.bytes > scratch_bytes) return fail(DSBDD_ERR_CAPACITY, "scratch too small (dsbdd_train_scratch_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int N = (int)g->n_nodes;
  // with side streams and two MLPs the second chain (kernel A .. node gathers) runs on sd->co out of its own scratch
  // (the second half of `scratch`, 2 x dsbdd_train_scratch_bytes) while the first runs here; d_x is still added in the
  // order q = 0, 1 on this stream
  const bool two = sd && (sd->mask & SIDE_CO) && n_mlp == 2 && scratch_bytes >= 2 * ts.bytes;
  const TrainScratch ts1 = two ? carve_train(static_cast<char*>(scratch) + ts.bytes, H, g->n_nodes, g->n_edges) : ts;
  if (two) HIP_TRY(sd->link(s, sd->co));
  for (int q = 0; q < n_mlp; ++q) {
    TrainEdgeArgs a{};
    a.d_xagg = d_xout; a.node_batch = g->node_batch; a.mean = mean; a.norm_constant = norm_constant;
    a.coords_range = coords_range; a.use_tanh = use_tanh; a.which = q; a.norm_factor = norm_factor;
    const TrainScratch& tq = q == 1 ? ts1 : ts;
    a.gm = q == 1 ? tq.gm : nullptr;
    dsbdd_train_mlp mq = m[q];
    mq.head = m[0].head;                      // the output layer is shared by both MLPs (egnn_new.py:78,85,91)
    hipStream_t sq = two && q == 1 ? sd->co : s;
    MlpBwdOpts o;
    o.side = sd; o.already_linked = true; o.z2 = z2 ? z2 + (size_t)q * z2_stride : nullptr; o.scratch_set = two && q == 1 ? 1 : 0;
    o.acc_w2 = acc_w2 && acc_w2[q];
    RC_TRY(mlp_backward(sq, H, MODE_COORD, g, &mq, x, e_upd, a, out + q, tq, o));
    if (sq != s) HIP_TRY(sd->link(sq, s));
    hipLaunchKernelGGL(edge_to_node3_kernel, dim3((N + 3) / 4), dim3(kThreads), 0, s, (const float*)tq.gd,
                       (const float*)tq.gxr, (const float*)tq.gxc, x, g->ecol, g->row_ptr, g->deg, g->rev, (int)e_upd, N,
                       d_x, q);
    HIP_TRY(hipGetLastError());
    if (q == 1) {
      hipLaunchKernelGGL(sample_edge_sum3_kernel, dim3((unsigned)g->batch), dim3(kThreads), 0, s, (const float*)tq.gm,
                         g->row_ptr, g->lig_off, g->poc_off, (int)g->n_lig, (int)e_upd, d_mean);
      HIP_TRY(hipGetLastError());
    }
  }
  return DSBDD_OK;
}
