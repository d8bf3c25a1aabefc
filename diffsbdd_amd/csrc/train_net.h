// The training step of EGNNDynamics as ONE launch sequence per direction (round 6).
//
// Reference: lightning_modules.py:337-363 (training_step) -> conditional_model.py:202-330 / en_diffusion.py:336-469
// (ddpm.forward) -> dynamics.py:87-167 (EGNNDynamics.forward) -> egnn_new.py:225-244, 163-184, 31-58, 96-122 under autograd.
//
// Rounds 4 - 5 composed the differentiable forward from ~60 torch.autograd.Function nodes (train_hip.py): every node
// called one or two HIP kernels through the C-ABI and left the residual adds, SiLUs, concatenations, weight transposes,
// first-layer re-layouts and gradient accumulations to ~470 small aten launches per step (profiles/r6_train_kernel_stats.md).
// Here the whole network is walked in C++: dsbdd_train_net_forward / dsbdd_train_net_backward enqueue every launch of a
// direction on the caller's stream -- no host synchronisation, no tensor library in between -- and PyTorch sees ONE autograd
// node (train_net.py).  What the sequence consists of:
//   * one batched re-layout launch per step for ALL weights (tn_pack_kernel over a descriptor table: the transposes the
//     GEMM kernels want as B operand, the first edge-MLP layer split into per-node projections / distance columns) + one
//     for the edge-type tables; the packed copies live in a caller-provided persistent buffer,
//   * the existing kernels of the edge stages (edge_wave.h forward; train.h kernel A / wgrad / kernel B / gathers) and of the
//     node level (node_linear.h GEMMs with fused bias / residual; ordered split-K weight gradients; ordered column sums),
//   * a handful of elementwise kernels (SiLU and its derivative on the saved pre-activations, input split, output
//     assembly, per-sample mean backward),
//   * the parameter gradients written in nn.Linear layout [out][in] straight into the caller's gradient tensors; what the
//     factorised first layer produces in pieces (d W_pq, d w_d, d w_d0, d tab) is assembled by one batched launch at the
//     end of the backward pass (tn_unpack_kernel).
// Every sum has a fixed order (no atomics): gradients stay bitwise reproducible.  Activations are kept in a caller-provided
// workspace between the two calls (per block: h, the projections, the aggregate, the node MLP's pre-activation and
// activation, the coordinates); nothing of size [E][H] is kept (the edge activations are recomputed, train.h).
//
// The kernels and descriptor tables of this file's own launches are in train_kernels.h; the stages of one message or
// coordinate layer in train_blocks.h (included in front of this file); the entry points in train_api.h.
#pragma once

// ---- the parameter list -------------------------------------------------------------------------------------------------
// Where every parameter tensor sits in the caller's `params` / `grads` arrays: the order of EGNNDynamics' own construction
// (diffsbdd_amd/synthetic.dynamics_param_shapes).  The aliased cross_product_mlp.4.weight is NOT listed: it IS
// coord_mlp.4.weight (egnn_new.py:78,85,91), `head_w` of both coordinate MLPs.
struct TnLinIx { int w, b; };
struct TnSubIx { int e1_w, e1_b, e2_w, e2_b, n1_w, n1_b, n2_w, n2_b, att_w, att_b; };   // att_*: -1 without attention
struct TnEqMlpIx { int l1_w, l1_b, l2_w, l2_b; };
struct TnEqIx { TnEqMlpIx mlp[2]; int head_w; };       // mlp[0] coord_mlp, mlp[1] cross_product_mlp (n_mlp == 2 only)
struct TnParamIndex {
  TnLinIx ae0, ae2, ad0, ad2, re0, re2, rd0, rd2;      // atom / residue encoders and decoders
  int emb_tab;                                         // edge_embedding.weight or -1
  TnLinIx emb, emb_out;
  std::vector<TnSubIx> subs;                           // message stage g = block * inv_sublayers + sublayer
  std::vector<TnEqIx> eqs;                             // per block
  int att, n_mlp;
  int n;
};
static TnParamIndex tn_index(const dsbdd_config& c) {
  TnParamIndex p{};
  int i = 0;
  auto next = [&] { return i++; };
  auto lin = [&] { const int w = next(); return TnLinIx{w, next()}; };
  p.ae0 = lin(); p.ae2 = lin(); p.ad0 = lin(); p.ad2 = lin(); p.re0 = lin(); p.re2 = lin(); p.rd0 = lin(); p.rd2 = lin();
  p.emb_tab = c.edge_embedding_dim > 0 ? next() : -1;
  p.emb = lin(); p.emb_out = lin();
  p.att = c.attention ? 1 : 0; p.n_mlp = c.reflection_equivariant ? 1 : 2;
  for (int b = 0; b < c.n_layers; ++b) {
    for (int sl = 0; sl < c.inv_sublayers; ++sl) {
      TnSubIx u{next(), next(), next(), next(), next(), next(), next(), next(), -1, -1};
      if (p.att) { u.att_w = next(); u.att_b = next(); }
      p.subs.push_back(u);
    }
    TnEqIx e{{{next(), next(), next(), next()}, {-1, -1, -1, -1}}, -1};
    e.head_w = next();
    if (p.n_mlp == 2) e.mlp[1] = TnEqMlpIx{next(), next(), next(), next()};
    p.eqs.push_back(e);
  }
  p.n = i;
  return p;
}

static const int kTnSideDefault = SIDE_CO | SIDE_NODE_WG | SIDE_COORD_WG;     // DSBDD_TRAIN_STREAMS (bit mask of SIDE_*, train_blocks.h) overrides
struct dsbdd_train_net {
  dsbdd_config cfg;
  TnParamIndex ix;
  // cached descriptor tables (device copies live at the head of the caller's pack buffer)
  std::vector<const float*> last_params;
  void* last_pack = nullptr;
  int n_pack = 0, n_tab = 0;
  // side streams of the backward (TrainSide, train_blocks.h), created on the first backward call; DSBDD_TRAIN_STREAMS=0: none
  TrainSide side;
  bool side_ready = false;
  int side_mask = 0;
  // The forward pass keeps z2 [E][H] of every edge MLP for the backward pass (4 E H bytes each: 93 MB at the reference
  // batch) instead of recomputing the H x H layer there; DSBDD_TRAIN_STORE_Z2=0: recompute (kernel A, rounds 4-5)
  bool store_z2 = true;
};
static dsbdd_train_net* tn_create(const dsbdd_config& cfg) {
  auto* n = new dsbdd_train_net();
  long long v;
  n->cfg = cfg; n->ix = tn_index(cfg);
  n->side_mask = env_int("DSBDD_TRAIN_STREAMS", &v) ? (int)v & 15 : kTnSideDefault;
  n->store_z2 = !(env_int("DSBDD_TRAIN_STORE_Z2", &v) && v == 0);
  return n;
}
// the side streams of the backward on the CURRENT device, or null when they are switched off
static int tn_side_streams(dsbdd_train_net* net, TrainSide** out) {
  if (net->side_ready) {
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != net->side.device) { net->side.destroy(); net->side_ready = false; }
  }
  if (net->side_mask && !net->side_ready) {
    HIP_TRY(net->side.create());
    net->side.mask = net->side_mask;
    net->side_ready = true;
  }
  *out = net->side_mask ? &net->side : nullptr;
  return DSBDD_OK;
}

// sizes of one call
struct TnDims {
  int a, r, J, D, JP, H, L, S, G, M, A, enf;
  int64_t n_l, n_p, N, B, E;
  size_t E1;      // max(E, 1): the stride of the per-edge buffers
};
static TnDims tn_dims(const dsbdd_config& c, const dsbdd_train_graph* g) {
  TnDims d{};
  d.a = c.atom_nf; d.r = c.residue_nf; d.J = c.joint_nf; d.D = d.J + 1; d.JP = pad4(d.D); d.H = c.hidden_nf;
  d.L = c.n_layers; d.S = c.inv_sublayers; d.G = d.L * d.S; d.M = c.reflection_equivariant ? 1 : 2;
  d.enf = c.edge_embedding_dim > 0 ? c.edge_embedding_dim : 0; d.A = 2 + d.enf;
  d.n_l = g->n_lig; d.N = g->n_nodes; d.n_p = d.N - d.n_l; d.B = g->batch; d.E = g->n_edges;
  d.E1 = (size_t)(d.E > 0 ? d.E : 1);
  return d;
}

// ---- the persistent pack buffer: descriptor tables + every re-laid-out weight -------------------------------------
// an nn.Linear [out][in]: WT [in][ldT] (forward B operand), Wp [out][ldP] (dX B operand)
struct TnLin { int out, in; float* WT; int ldT; float* Wp; int ldP; };
struct TnEdgeMlp { float *wd, *wd0, *tab, *W2T; };
struct TnPack {
  TnPackDesc* d_pack; TnTabDesc* d_tab;      // device descriptor tables
  TnLin ae0, ae2, ad0, ad2, re0, re2, rd0, rd2, emb, emb_out;
  std::vector<float*> WpqT, Wpq;             // per message stage g: [H][2H], [2H][H]
  std::vector<TnEdgeMlp> gcl;                // per g
  std::vector<TnLin> n1, n2;                 // node MLP layers per g
  std::vector<float*> W4T, W4;               // per block: [H][2H M], [2H M][H]
  std::vector<TnEdgeMlp> eqm;                // per block x MLP
  size_t bytes;
};
static const int kTnMaxDesc = 1024, kTnMaxTab = 256;
static TnPack tn_carve_pack(char* base, const dsbdd_config& c) {
  TnPack p{};
  const int a = c.atom_nf, r = c.residue_nf, J = c.joint_nf, D = J + 1, H = c.hidden_nf, L = c.n_layers, S = c.inv_sublayers;
  const int M = c.reflection_equivariant ? 1 : 2;
  const size_t HH = (size_t)H * H;
  Carver cv{base};
  p.d_pack = reinterpret_cast<TnPackDesc*>(cv.bytes(sizeof(TnPackDesc) * kTnMaxDesc));
  p.d_tab = reinterpret_cast<TnTabDesc*>(cv.bytes(sizeof(TnTabDesc) * kTnMaxTab));
  auto lin = [&](int out, int in) {
    TnLin l{out, in, nullptr, pad4(out), nullptr, pad4(in)};
    l.WT = cv.f((size_t)in * l.ldT); l.Wp = cv.f((size_t)out * l.ldP);
    return l;
  };
  auto edge_mlp = [&] { return TnEdgeMlp{cv.f(H), cv.f(H), cv.f(3 * (size_t)H), cv.f(HH)}; };
  p.ae0 = lin(2 * a, a); p.ae2 = lin(J, 2 * a); p.ad0 = lin(2 * a, J); p.ad2 = lin(a, 2 * a);
  p.re0 = lin(2 * r, r); p.re2 = lin(J, 2 * r); p.rd0 = lin(2 * r, J); p.rd2 = lin(r, 2 * r);
  p.emb = lin(H, D); p.emb_out = lin(D, H);
  for (int g = 0; g < L * S; ++g) {
    p.WpqT.push_back(cv.f(2 * HH)); p.Wpq.push_back(cv.f(2 * HH));
    p.gcl.push_back(edge_mlp());
    p.n1.push_back(lin(H, 2 * H)); p.n2.push_back(lin(H, H));
  }
  for (int b = 0; b < L; ++b) {
    p.W4T.push_back(cv.f(2 * HH * M)); p.W4.push_back(cv.f(2 * HH * M));
    for (int q = 0; q < M; ++q) p.eqm.push_back(edge_mlp());
  }
  p.bytes = cv.off;
  return p;
}

// ---- the per-call workspace: graph-sized activations and gradients --------------------------------------------------
struct TnWs {
  float *x0, *hf_l, *hf_p, *ze_l, *ae_l, *ze_p, *ae_p, *h0, *hout, *zd_l, *ad_l, *zd_p, *ad_p, *eh_l, *eh_p, *vel, *meanv;
  std::vector<float*> h, x, mean, pq, agg, z, act, pq4;       // h [G + 1], x [L + 1], mean [L], pq/agg/z/act [G], pq4 [L]
  std::vector<float*> z2, z2c;                                // z2 [G] x [E][H], z2c [L] x [M][E][H]: the edge MLPs' second-layer pre-activations
  // backward
  float *d_vel, *deh_l, *deh_p, *d_h[2], *d_x[2], *d_xg, *d_pq4, *d_pq, *da, *dz, *d_agg, *xcat, *d_hout, *d_h0, *d_hf_l, *d_hf_p,
      *d_small, *gd0, *gd0_tot, *d_mean, *colscr, *dWpq, *d_vec, *demb_part, *wg;
  size_t wg_floats;
  char* scratch; size_t scratch_bytes;
  size_t bytes;
};
// (every buffer holds at least one element: Carver::f1)
static TnWs tn_carve_ws(char* base, const TnDims& d, bool store_z2) {
  TnWs w{};
  Carver cv{base};
  const size_t N = (size_t)d.N, H = d.H, nl = (size_t)d.n_l, np = (size_t)d.n_p, JP = d.JP;
  const size_t N3 = 3 * N, B3 = 3 * (size_t)d.B, NH = N * H, NJ = N * JP, EH = d.E1 * H, PQ4 = NH * 2 * d.M;
  const size_t la = nl * d.a, pr = np * d.r;          // ligand x atom features, pocket x residue features
  const size_t mx2 = 2 * (size_t)(d.a > d.r ? d.a : d.r);
  const size_t n_mlp = (size_t)(d.G + d.L * d.M);     // edge MLPs of the network
  w.x0 = cv.f1(N3); w.hf_l = cv.f1(la); w.hf_p = cv.f1(pr);
  w.ze_l = cv.f1(2 * la); w.ae_l = cv.f1(2 * la); w.ze_p = cv.f1(2 * pr); w.ae_p = cv.f1(2 * pr);
  w.h0 = cv.f1(NJ); w.hout = cv.f1(NJ);
  w.zd_l = cv.f1(2 * la); w.ad_l = cv.f1(2 * la); w.zd_p = cv.f1(2 * pr); w.ad_p = cv.f1(2 * pr);
  w.eh_l = cv.f1(la); w.eh_p = cv.f1(pr); w.vel = cv.f1(N3); w.meanv = cv.f1(B3);
  for (int g = 0; g <= d.G; ++g) w.h.push_back(cv.f1(NH));
  for (int b = 0; b <= d.L; ++b) w.x.push_back(cv.f1(N3));
  for (int b = 0; b < d.L; ++b) { w.mean.push_back(cv.f1(B3)); w.pq4.push_back(cv.f1(PQ4)); }
  for (int g = 0; g < d.G; ++g) { w.pq.push_back(cv.f1(2 * NH)); w.agg.push_back(cv.f1(NH)); w.z.push_back(cv.f1(NH)); w.act.push_back(cv.f1(NH)); }
  for (int g = 0; g < d.G; ++g) w.z2.push_back(store_z2 ? cv.f1(EH) : nullptr);
  for (int b = 0; b < d.L; ++b) w.z2c.push_back(store_z2 ? cv.f1(EH * d.M) : nullptr);
  w.d_vel = cv.f1(N3); w.deh_l = cv.f1(la); w.deh_p = cv.f1(pr);
  w.d_h[0] = cv.f1(NH); w.d_h[1] = cv.f1(NH); w.d_x[0] = cv.f1(N3); w.d_x[1] = cv.f1(N3); w.d_xg = cv.f1(N3);
  w.d_pq4 = cv.f1(PQ4); w.d_pq = cv.f1(2 * NH); w.da = cv.f1(NH); w.dz = cv.f1(NH); w.d_agg = cv.f1(NH);
  w.xcat = cv.f1(2 * NH); w.d_hout = cv.f1(NJ); w.d_h0 = cv.f1(NJ);
  w.d_hf_l = cv.f1(la); w.d_hf_p = cv.f1(pr); w.d_small = cv.f1((nl > np ? nl : np) * mx2 * 2);
  w.gd0 = cv.f1(2 * d.E1); w.gd0_tot = cv.f1(d.E1); w.d_mean = cv.f1(B3);
  w.colscr = cv.f1(((N + 31) / 32 + 1) * (2 * H > JP ? 2 * H : JP));
  w.dWpq = cv.f1((size_t)(d.G * 2 + d.L * 2 * d.M) * H * H);
  w.d_vec = cv.f1(n_mlp * 8 * H);
  w.demb_part = cv.f1(n_mlp * 3 * (d.enf > 0 ? d.enf : 1));
  {   // the largest split-K plan over the node-level weight gradients of this network (K <= N rows)
    const int m2 = (int)mx2;
    const int shapes[][2] = {{d.H, d.H}, {d.H, 2 * d.H}, {2 * d.H, d.H}, {2 * d.H * d.M, d.H}, {d.D, d.H}, {d.H, d.D}, {d.J, m2},
                             {m2, d.J}, {m2, m2}};
    w.wg_floats = 0;
    for (const auto& sh : shapes) { const size_t f = wgrad_floats_upto((int64_t)N, sh[0], sh[1]); if (f > w.wg_floats) w.wg_floats = f; }
  }
  w.wg = cv.f1(w.wg_floats);
  // (two scratch sets when a coordinate stage has two edge MLPs: their backward chains run side by side)
  w.scratch_bytes = carve_train(nullptr, d.H, d.N, d.E).bytes * (d.M == 2 ? 2 : 1);
  w.scratch = cv.bytes(w.scratch_bytes);
  w.bytes = cv.off;
  return w;
}

// y = [x | x2] W^T (+ b) (+ R) through node_linear: x [M][lda] (K columns), x2 likewise or none, WT [K + K2][ldT]
static int tn_lin(hipStream_t s, const float* x, int lda, int K, const float* WT, int ldT, const float* bias, const float* R,
                  int ldr, float* y, int ldc, int64_t M, int Nout, const float* x2 = nullptr, int lda2 = 0, int K2 = 0) {
  if (M <= 0) return DSBDD_OK;
  HIP_TRY(nl(s, x, lda, K, x2, lda2, K2, WT, ldT, bias, R, ldr, y, ldc, M, Nout, 0));
  return DSBDD_OK;
}
// (acc: dW / db += the gradient; a gradient of zeros then adds nothing instead of clearing)
static int tn_wgrad(hipStream_t s, const float* dy, int ldy, const float* x, int ldx, int64_t K, int M, int Nn, float* dW,
                    const TnWs& w, bool acc = false) {
  if (K <= 0) { if (!acc) HIP_TRY(hipMemsetAsync(dW, 0, (size_t)M * Nn * 4, s)); return DSBDD_OK; }
  return wgrad_impl(s, dy, ldy, x, ldx, K, M, Nn, dW, w.wg, w.wg_floats, acc);
}
static int tn_colsum(hipStream_t s, const float* dy, int ldy, int64_t M, int Nn, float* db, const TnWs& w, bool acc = false) {
  if (M <= 0) { if (!acc) HIP_TRY(hipMemsetAsync(db, 0, (size_t)Nn * 4, s)); return DSBDD_OK; }
  HIP_TRY(reduce_parts(s, dy, (int)M, (size_t)ldy, Nn, db, w.colscr, acc));
  return DSBDD_OK;
}

// ---- the edge MLPs as the stages of train_blocks.h take them ------------------------------------------------------------
// P | Q in columns [col, col + 2H) of pq [N][ld] (pq null: the weights only, tn_prepare_pack)
static dsbdd_train_mlp tn_mlp(const float* pq, int col, int ld, int H, const TnEdgeMlp& m, const float* W2, const float* b2,
                              const float* head, const float* head_b) {
  dsbdd_train_mlp t{};
  t.P = pq ? pq + col : nullptr; t.Q = pq ? pq + col + H : nullptr; t.ldpq = ld;
  t.wd = m.wd; t.wd0 = m.wd0; t.tab = m.tab; t.W2 = W2; t.W2T = m.W2T; t.b2 = b2; t.head = head; t.head_b = head_b;
  return t;
}
// message stage gi over pq [N][2H]; the head is the attention layer
static dsbdd_train_mlp tn_msg_mlp(const TnParamIndex& ix, const float* const* P, const TnPack& pk, int gi, int H, const float* pq) {
  const TnSubIx& u = ix.subs[gi];
  return tn_mlp(pq, 0, 2 * H, H, pk.gcl[gi], P[u.e2_w], P[u.e2_b], ix.att ? P[u.att_w] : nullptr, ix.att ? P[u.att_b] : nullptr);
}
// the coordinate stage of block b over pq4 [N][2H M]: MLP q in columns [2H q, 2H q + 2H), one output layer for both
static void tn_coord_mlps(const TnParamIndex& ix, const float* const* P, const TnPack& pk, int b, int H, const float* pq4,
                          dsbdd_train_mlp mm[2]) {
  const TnEqIx& e = ix.eqs[b];
  const int M = ix.n_mlp;
  for (int q = 0; q < M; ++q)
    mm[q] = tn_mlp(pq4, 2 * H * q, 2 * H * M, H, pk.eqm[b * M + q], P[e.mlp[q].l2_w], P[e.mlp[q].l2_b], P[e.head_w], nullptr);
}

// the pack buffer holds the re-laid-out copies of exactly these tensors (their VALUES are the caller's business)
static bool tn_pack_matches(const dsbdd_train_net* net, const float* const* P, const char* pack_base) {
  bool same = net->last_pack == pack_base && (int)net->last_params.size() == net->ix.n;
  for (int i = 0; same && i < net->ix.n; ++i) same = net->last_params[i] == P[i];
  return same;
}
// descriptor tables of the weight re-layout; uploaded when the parameter / pack pointers changed
static int tn_prepare_pack(dsbdd_train_net* net, hipStream_t s, const float* const* P, char* pack_base, const TnPack& pk) {
  const dsbdd_config& c = net->cfg;
  const TnParamIndex& ix = net->ix;
  const int H = c.hidden_nf, L = c.n_layers, S = c.inv_sublayers;
  const int M = ix.n_mlp, enf = c.edge_embedding_dim > 0 ? c.edge_embedding_dim : 0, ld1 = 2 * H + 2 + enf;
  if (!tn_pack_matches(net, P, pack_base)) {
    std::vector<TnPackDesc> pd;
    std::vector<TnTabDesc> td;
    auto lin = [&](TnLinIx i, const TnLin& l) { pd.push_back(TnPackDesc{P[i.w], l.in, l.out, l.in, l.WT, l.ldT, l.ldT, l.Wp, l.ldP}); };
    auto lin_T = [&](int wi, const TnLin& l) { pd.push_back(TnPackDesc{P[wi], l.in, l.out, l.in, l.WT, l.ldT, l.ldT, nullptr, 0}); };
    lin(ix.ae0, pk.ae0); lin(ix.ae2, pk.ae2); lin(ix.ad0, pk.ad0); lin(ix.ad2, pk.ad2);
    lin(ix.re0, pk.re0); lin(ix.re2, pk.re2); lin(ix.rd0, pk.rd0); lin(ix.rd2, pk.rd2);
    lin(ix.emb, pk.emb); lin(ix.emb_out, pk.emb_out);
    const float* emb = ix.emb_tab >= 0 ? P[ix.emb_tab] : nullptr;
    // first layer of an edge MLP W1 [H][2H + A]: the two [H][H] blocks as columns [c0, c0 + H) / [c0 + H, c0 + 2H) of
    // WT [H][ldT] (rows = k) and as rows [c0, c0 + H) / [c0 + H, c0 + 2H) of Wp [.][H]; the distance columns; the table.
    // Second layer: the transpose, where the stages will look for it (m.W2T).
    auto edge_mlp = [&](int w1, int b1, float* WT, int ldT, int c0, float* Wp, const TnEdgeMlp& dst, const dsbdd_train_mlp& m) {
      const float* W1 = P[w1];
      pd.push_back(TnPackDesc{W1, ld1, H, H, WT + c0, ldT, 0, Wp + (size_t)c0 * H, H});
      pd.push_back(TnPackDesc{W1 + H, ld1, H, H, WT + c0 + H, ldT, 0, Wp + (size_t)(c0 + H) * H, H});
      pd.push_back(TnPackDesc{W1 + 2 * H, ld1, H, 1, dst.wd, H, 0, nullptr, 0});
      pd.push_back(TnPackDesc{W1 + 2 * H + 1, ld1, H, 1, dst.wd0, H, 0, nullptr, 0});
      td.push_back(TnTabDesc{W1, ld1, 2 * H + 2, P[b1], emb, enf, dst.tab, H});
      pd.push_back(TnPackDesc{m.W2, H, H, H, dst.W2T, H, 0, nullptr, 0});
    };
    for (int b = 0; b < L; ++b) {
      for (int sl = 0; sl < S; ++sl) {
        const int g = b * S + sl;
        const TnSubIx& u = ix.subs[g];
        edge_mlp(u.e1_w, u.e1_b, pk.WpqT[g], 2 * H, 0, pk.Wpq[g], pk.gcl[g], tn_msg_mlp(ix, P, pk, g, H, nullptr));
        lin_T(u.n1_w, pk.n1[g]); lin_T(u.n2_w, pk.n2[g]);
      }
      dsbdd_train_mlp mm[2];
      tn_coord_mlps(ix, P, pk, b, H, nullptr, mm);
      for (int q = 0; q < M; ++q)
        edge_mlp(ix.eqs[b].mlp[q].l1_w, ix.eqs[b].mlp[q].l1_b, pk.W4T[b], 2 * H * M, 2 * H * q, pk.W4[b], pk.eqm[b * M + q], mm[q]);
    }
    if ((int)pd.size() > kTnMaxDesc || (int)td.size() > kTnMaxTab) return fail(DSBDD_ERR_CAPACITY, "too many layers for the descriptor tables");
    HIP_TRY(hipMemcpyAsync(pk.d_pack, pd.data(), pd.size() * sizeof(TnPackDesc), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(pk.d_tab, td.data(), td.size() * sizeof(TnTabDesc), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));        // (the host vectors go out of scope; once per set of pointers)
    net->n_pack = (int)pd.size(); net->n_tab = (int)td.size();
    net->last_params.assign(P, P + ix.n); net->last_pack = pack_base;
  }
  hipLaunchKernelGGL(tn_pack_kernel, dim3(32, net->n_pack), dim3(256), 0, s, (const TnPackDesc*)pk.d_pack);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(tn_tab_kernel, dim3(net->n_tab), dim3(256), 0, s, (const TnTabDesc*)pk.d_tab);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

// ---- one call --------------------------------------------------------------------------------------------------------
// y = W1 SiLU(W0 x + b0) + b1: an encoder or decoder (dynamics.py:96-97, 147-149) with what the forward pass keeps of it
struct TnMlp2 {
  TnLinIx i0, i1;      // parameter slots of the two layers
  TnLin l0, l1;        // their packed copies
  float *z, *act;      // [rows][l0.out]: pre-activation and activation
};

// What both directions of a call share: the handle, the stream, the graph, the carved buffers and the sizes.
struct TrainCall {
  dsbdd_train_net* const net;
  const hipStream_t s;
  const dsbdd_train_graph* const g;
  const float* const* const P;
  const dsbdd_config& c;
  const TnParamIndex& ix;
  const TnDims d;
  const TnPack pk;
  const TnWs w;
  char* const pack_base;
  const int H, a, r, J, JP, N, n_l, n_p, M;
  const int64_t E, n_upd;      // n_upd: the leading rows whose coordinates move (all, or the ligand's)
  const size_t N3, NH;
  const TnMlp2 enc_l, enc_p, dec_l, dec_p;

  TrainCall(dsbdd_train_net* net_, void* stream, const dsbdd_train_graph* g_, const float* const* params, void* pack, void* ws)
      : net(net_), s(static_cast<hipStream_t>(stream)), g(g_), P(params), c(net_->cfg), ix(net_->ix), d(tn_dims(c, g_)),
        pk(tn_carve_pack(static_cast<char*>(pack), c)), w(tn_carve_ws(static_cast<char*>(ws), d, net_->store_z2)),
        pack_base(static_cast<char*>(pack)), H(d.H), a(d.a), r(d.r), J(d.J), JP(d.JP), N((int)d.N), n_l((int)d.n_l),
        n_p((int)d.n_p), M(d.M), E(d.E), n_upd(c.update_pocket_coords ? d.N : d.n_l), N3(3 * (size_t)d.N), NH((size_t)d.N * d.H),
        enc_l{ix.ae0, ix.ae2, pk.ae0, pk.ae2, w.ze_l, w.ae_l}, enc_p{ix.re0, ix.re2, pk.re0, pk.re2, w.ze_p, w.ae_p},
        dec_l{ix.ad0, ix.ad2, pk.ad0, pk.ad2, w.zd_l, w.ad_l}, dec_p{ix.rd0, ix.rd2, pk.rd0, pk.rd2, w.zd_p, w.ad_p} {}
  // the pocket rows of a node matrix with ld floats per row
  template <class T> T* pocket(T* m, int ld) const { return m + (size_t)n_l * ld; }
};

// The forward pass (dynamics.py:87-167 over egnn_new.py:225-244).  Every stage runs on `s`; what it leaves in the
// workspace is what TrainBackward reads.
struct TrainForward : TrainCall {
  using TrainCall::TrainCall;

  // writes m.z, m.act and y [rows][ldc]
  int mlp2(const TnMlp2& m, const float* x, int lda, float* y, int ldc, int64_t rows) {
    if (rows <= 0) return DSBDD_OK;
    const int mid = m.l0.out;
    RC_TRY(tn_lin(s, x, lda, m.l0.in, m.l0.WT, m.l0.ldT, P[m.i0.b], nullptr, 0, m.z, mid, rows, mid));
    RC_TRY(launch_1d(tn_silu_kernel, (size_t)rows * mid, s, m.z, m.act, (size_t)rows * mid));
    return tn_lin(s, m.act, mid, mid, m.l1.WT, m.l1.ldT, P[m.i1.b], nullptr, 0, y, ldc, rows, m.l1.out);
  }

  // dynamics.py:89-111, egnn_new.py:233: split, encoders, time feature, embedding.  Writes x0, hf_*, h0, h[0], x[0].
  int inputs_and_encoders(const float* xh_lig, const float* xh_pocket, const float* t, int64_t t_count) {
    RC_TRY(launch_1d(tn_split_inputs_kernel, N, s, xh_lig, 3 + a, xh_pocket, 3 + r, n_l, n_p, w.x0, w.hf_l, w.hf_p));
    RC_TRY(mlp2(enc_l, w.hf_l, a, w.h0, JP, n_l));
    RC_TRY(mlp2(enc_p, w.hf_p, r, pocket(w.h0, JP), JP, n_p));
    RC_TRY(launch_1d(tn_time_col_kernel, N, s, w.h0, JP, J, t, (int)t_count, g->node_batch, N));
    RC_TRY(tn_lin(s, w.h0, JP, d.D, pk.emb.WT, pk.emb.ldT, P[ix.emb.b], nullptr, 0, w.h[0], H, N, H));
    HIP_TRY(hipMemcpyAsync(w.x[0], w.x0, (size_t)N * 12, hipMemcpyDeviceToDevice, s));
    return DSBDD_OK;
  }

  // egnn_new.py:31-58 at the coordinates x[b].  Reads h[gi]; writes pq[gi], agg[gi], z[gi], act[gi], z2[gi], h[gi + 1].
  int sublayer(int b, int sl) {
    const int gi = b * d.S + sl;
    const TnSubIx& u = ix.subs[gi];
    const float* hin = w.h[gi];
    RC_TRY(tn_lin(s, hin, H, H, pk.WpqT[gi], 2 * H, nullptr, nullptr, 0, w.pq[gi], 2 * H, N, 2 * H));
    const dsbdd_train_mlp m = tn_msg_mlp(ix, P, pk, gi, H, w.pq[gi]);
    RC_TRY(gcl_forward_impl(s, H, g, &m, w.x[b], c.normalization_factor, w.agg[gi], w.scratch, w.scratch_bytes, w.z2[gi]));
    // node MLP (egnn_new.py:53-58): h + W2 SiLU(W1 [h | agg] + b1) + b2
    RC_TRY(tn_lin(s, hin, H, H, pk.n1[gi].WT, pk.n1[gi].ldT, P[u.n1_b], nullptr, 0, w.z[gi], H, N, H, w.agg[gi], H, H));
    RC_TRY(launch_1d(tn_silu_kernel, NH, s, w.z[gi], w.act[gi], NH));
    return tn_lin(s, w.act[gi], H, H, pk.n2[gi].WT, pk.n2[gi].ldT, P[u.n2_b], hin, H, w.h[gi + 1], H, N, H);
  }

  // coordinate update (egnn_new.py:96-122).  Reads the block's last h, x[b], mean[b]; writes pq4[b], z2c[b], x[b + 1].
  int coord_stage(int b) {
    RC_TRY(tn_lin(s, w.h[(b + 1) * d.S], H, H, pk.W4T[b], 2 * H * M, nullptr, nullptr, 0, w.pq4[b], 2 * H * M, N, 2 * H * M));
    dsbdd_train_mlp mm[2];
    tn_coord_mlps(ix, P, pk, b, H, w.pq4[b], mm);
    return coord_forward_impl(s, H, g, mm, M, w.x[b], M == 2 ? w.mean[b] : nullptr, n_upd, c.norm_constant, c.coords_range,
                              c.use_tanh, c.normalization_factor, w.x[b + 1], w.scratch, w.scratch_bytes, w.z2c[b], d.E1 * H);
  }

  // egnn_new.py:241-243, dynamics.py:136-167.  Reads h[G], x[L], x0; writes hout, the decoders' z / act, eh_*, vel, meanv.
  int decoders_and_output(int32_t zero_nan, float* eps_lig, float* eps_pocket, int32_t* status) {
    RC_TRY(tn_lin(s, w.h[d.G], H, H, pk.emb_out.WT, pk.emb_out.ldT, P[ix.emb_out.b], nullptr, 0, w.hout, JP, N, d.D));
    RC_TRY(mlp2(dec_l, w.hout, JP, w.eh_l, a, n_l));
    RC_TRY(mlp2(dec_p, pocket(w.hout, JP), JP, w.eh_p, r, n_p));
    RC_TRY(launch_1d(tn_vel_kernel, N3, s, w.x[d.L], w.x0, w.vel, 3 * N, (int)zero_nan, status));
    if (c.update_pocket_coords) RC_TRY(sample_mean_impl(s, w.vel, g, w.meanv));
    return launch_1d(tn_out_kernel, N, s, w.vel, c.update_pocket_coords ? w.meanv : nullptr, g->node_batch, w.eh_l, a, w.eh_p, r,
                     n_l, n_p, eps_lig, eps_pocket);
  }

  // pack_is_current: the pack buffer already holds these weights (an accumulation window: they cannot have changed
  // since the window's first forward) -- the two re-layout launches are skipped
  int run(const float* xh_lig, const float* xh_pocket, const float* t, int64_t t_count, int32_t zero_nan, float* eps_lig,
          float* eps_pocket, int32_t* status, bool pack_is_current = false) {
    if (pack_is_current && !tn_pack_matches(net, P, pack_base))
      return fail(DSBDD_ERR_STATE, "the pack buffer does not hold these parameter tensors");
    if (!pack_is_current) RC_TRY(tn_prepare_pack(net, s, P, pack_base, pk));
    RC_TRY(inputs_and_encoders(xh_lig, xh_pocket, t, t_count));
    for (int b = 0; b < d.L; ++b) {
      if (M == 2) RC_TRY(sample_mean_impl(s, w.x[b], g, w.mean[b]));      // the cross product is taken about it
      for (int sl = 0; sl < d.S; ++sl) RC_TRY(sublayer(b, sl));
      RC_TRY(coord_stage(b));
    }
    return decoders_and_output(zero_nan, eps_lig, eps_pocket, status);
  }
};

// The backward pass: the stages of TrainForward in reverse.  The chain of the input gradients runs on `s`; with side
// streams (TrainSide, train_blocks.h) the node-level weight gradients of the blocks go to `sw` and their bias gradients
// to `sb`, forked from `s` where their operands are complete.  Parameter gradients go straight to G[...]; what the
// factorised first layers produce in pieces is noted in `ud` / `cd` and assembled at the end.
// Accumulation (dsbdd_train_net_backward_acc): slot i with A[i] != 0 receives G[i] += g_i, folded into the LAST store of
// that gradient -- the final level of reduce_parts, tn_unpack / tn_copy / tn_sum_parts -- on the stream where the
// overwriting store runs; the scratch in between (dWpq, d_vec, demb_part) is overwritten per call either way.
struct TrainBackward : TrainCall {
  float* const* const G;
  const uint8_t* const A;             // per parameter slot: accumulate (null: overwrite everything)
  const int64_t e_upd;                // the edge prefix of the rows whose coordinates move
  const bool want_in;                 // the caller asked for input gradients
  TrainSide* sd = nullptr;
  hipStream_t sw, sb;                 // == s without side streams
  const float* const emb;             // edge-type embedding or null
  // the running gradients: d_h / d_x w.r.t. the h / x the walk has reached, and the buffer the next stage writes its own to
  float *d_h, *d_h_next, *d_x, *d_x_next;
  int n_edge_mlps = 0;                // edge MLPs walked so far; MLP k owns slot k of d_vec / demb_part
  std::vector<TnUnpackDesc> ud;       // gradient-assembly tables, launched at the end (by value, see TnUnpackTable)
  std::vector<TnCopyDesc> cd;

  TrainBackward(dsbdd_train_net* net_, void* stream, const dsbdd_train_graph* g_, const float* const* params, float* const* grads,
                const uint8_t* accumulate, void* pack, void* ws, int64_t e_upd_, bool want_in_)
      : TrainCall(net_, stream, g_, params, pack, ws), G(grads), A(accumulate), e_upd(e_upd_), want_in(want_in_), sw(s), sb(s),
        emb(ix.emb_tab >= 0 ? P[ix.emb_tab] : nullptr), d_h(w.d_h[0]), d_h_next(w.d_h[1]), d_x(w.d_x[0]), d_x_next(w.d_x[1]) {}

  bool acc(int slot) const { return A && A[slot]; }
  float* vec_of(int k) const { return w.d_vec + (size_t)k * 8 * H; }      // [8][H]: d_wd, d_wd0, d_tab[0..2], d_b2, d head, d head_b
  int fork_w() { if (sw != s) HIP_TRY(sd->link(s, sd->wg)); return DSBDD_OK; }
  int fork_b() { if (sb != s) HIP_TRY(sd->link(s, sd->co)); return DSBDD_OK; }
  // d W = dy^T x and d b = the column sums of dy, for y = x W^T + b over `rows` rows.  beside: on the side streams, forked here
  int lin_grads(bool beside, const float* dy, int ldy, const float* x, int ldx, int64_t rows, int out, int in, TnLinIx i) {
    if (beside) RC_TRY(fork_w());
    RC_TRY(tn_wgrad(beside ? sw : s, dy, ldy, x, ldx, rows, out, in, G[i.w], w, acc(i.w)));
    if (beside) RC_TRY(fork_b());
    return tn_colsum(beside ? sb : s, dy, ldy, rows, out, G[i.b], w, acc(i.b));
  }
  int add_gd0(const float* gd) {      // the input distances d0 collect a gradient from every edge MLP
    if (!want_in || E <= 0) return DSBDD_OK;
    return launch_1d(tn_add_kernel, (size_t)E, s, w.gd0_tot, gd, (size_t)E);
  }
  // notes the assembly of edge MLP k's first layer (d W1, d b1, its share of d emb) and the copy of d b2
  void edge_mlp_grads(int k, int l1_w, int l1_b, int l2_b, const float* dWpq) {
    ud.push_back(TnUnpackDesc{G[l1_w], 2 * H + d.A, G[l1_b], emb ? w.demb_part + (size_t)k * 3 * d.enf : nullptr, dWpq, H, vec_of(k),
                              P[l1_w], emb, d.enf, H, acc(l1_w), acc(l1_b)});
    cd.push_back(TnCopyDesc{G[l2_b], vec_of(k) + 5 * H, nullptr, H, acc(l2_b)});
  }

  // Reads dy [rows][lddy], x [rows][ldx] and m.z / m.act; writes both layers' gradients and, if asked, dx.  w.d_small is
  // its scratch.
  int mlp2_bwd(const TnMlp2& m, const float* dy, int lddy, const float* x, int ldx, float* dx, int lddx, int64_t rows, bool want_dx) {
    const int in = m.l0.in, mid = m.l0.out, out = m.l1.out;
    float* dact = w.d_small;
    float* dzz = w.d_small + (size_t)(rows > 0 ? rows : 0) * mid;
    RC_TRY(lin_grads(false, dy, lddy, m.act, mid, rows, out, mid, m.i1));
    if (rows > 0) {
      RC_TRY(tn_lin(s, dy, lddy, out, m.l1.Wp, m.l1.ldP, nullptr, nullptr, 0, dact, mid, rows, mid));
      RC_TRY(launch_1d(tn_silu_bwd_kernel, (size_t)rows * mid, s, dact, m.z, dzz, (size_t)rows * mid));
    }
    RC_TRY(lin_grads(false, dzz, mid, x, ldx, rows, mid, in, m.i0));
    if (want_dx && rows > 0) RC_TRY(tn_lin(s, dzz, mid, mid, m.l0.Wp, m.l0.ldP, nullptr, nullptr, 0, dx, lddx, rows, in));
    return DSBDD_OK;
  }

  // dynamics.py:136-167, egnn_new.py:241-243 backward.  Reads the output gradients; writes d_vel, the decoders' and
  // embedding_out's gradients, d_h (w.r.t. h[G]) and d_x (w.r.t. x[L], which enters vel only); clears gd0_tot.
  int output_and_decoders(const float* d_eps_lig, const float* d_eps_pocket) {
    RC_TRY(launch_1d(tn_split_grads_kernel, N, s, d_eps_lig, a, d_eps_pocket, r, n_l, n_p, w.d_vel, w.deh_l, w.deh_p));
    if (c.update_pocket_coords) {          // vel - mean(vel): the same projection on the gradient
      RC_TRY(sample_mean_impl(s, w.d_vel, g, w.meanv));
      RC_TRY(launch_1d(tn_sub_mean_kernel, N3, s, w.d_vel, w.meanv, g->node_batch, N));
    }
    RC_TRY(mlp2_bwd(dec_l, w.deh_l, a, w.hout, JP, w.d_hout, JP, n_l, true));
    RC_TRY(mlp2_bwd(dec_p, w.deh_p, r, pocket(w.hout, JP), JP, pocket(w.d_hout, JP), JP, n_p, true));
    RC_TRY(launch_1d(tn_clear_cols_kernel, N, s, w.d_hout, JP, J, N));
    RC_TRY(lin_grads(false, w.d_hout, JP, w.h[d.G], H, N, d.D, H, ix.emb_out));
    RC_TRY(tn_lin(s, w.d_hout, JP, d.D, pk.emb_out.Wp, pk.emb_out.ldP, nullptr, nullptr, 0, d_h, H, N, H));
    HIP_TRY(hipMemcpyAsync(d_x, w.d_vel, (size_t)N * 12, hipMemcpyDeviceToDevice, s));
    if (want_in) HIP_TRY(hipMemsetAsync(w.gd0_tot, 0, d.E1 * 4, s));
    return DSBDD_OK;
  }

  // Coordinate update backward.  Reads d_x (w.r.t. x[b + 1]) and d_h (w.r.t. the block's last h); leaves d_x w.r.t. x[b]
  // and adds the stage's share to d_h.  Overwrites d_pq4, gd0 and the edge scratch.  The W4 gradient goes to `sw`.
  int coord_stage(int b) {
    const TnEqIx& e = ix.eqs[b];
    dsbdd_train_mlp mm[2];
    tn_coord_mlps(ix, P, pk, b, H, w.pq4[b], mm);
    const int k0 = n_edge_mlps;
    n_edge_mlps += M;
    float* dW4 = w.dWpq + (size_t)(d.G * 2 + b * 2 * M) * H * H;       // [2H M][H]
    dsbdd_train_mlp_grad og[2];
    bool acc_w2[2] = {false, false};
    for (int q = 0; q < M; ++q) {
      acc_w2[q] = acc(e.mlp[q].l2_w);
      og[q].dP = w.d_pq4 + 2 * H * q; og[q].dQ = w.d_pq4 + 2 * H * q + H; og[q].ldo = 2 * H * M;
      og[q].d_vec = vec_of(k0 + q); og[q].d_W2 = G[e.mlp[q].l2_w]; og[q].gd0 = w.gd0 + (size_t)q * d.E1;
    }
    if (e_upd > 0 && n_upd > 0) {
      if (want_in) HIP_TRY(hipMemsetAsync(w.gd0, 0, 2 * d.E1 * 4, s));
      RC_TRY(coord_backward_impl(s, H, g, mm, M, w.x[b], M == 2 ? w.mean[b] : nullptr, n_upd, e_upd, c.norm_constant, c.coords_range,
                                 c.use_tanh, c.normalization_factor, d_x, og, d_x_next, M == 2 ? w.d_mean : nullptr, w.scratch,
                                 w.scratch_bytes, sd, w.z2c[b], d.E1 * H, acc_w2));
      for (int q = 0; q < M; ++q) RC_TRY(add_gd0(og[q].gd0));
      RC_TRY(launch_1d(tn_add_kernel, N3, s, d_x_next, d_x, N3));        // identity path x -> x_out
      if (M == 2) RC_TRY(launch_1d(tn_mean_bwd_kernel, N3, s, d_x_next, w.d_mean, g->node_batch, g->lig_off, g->poc_off, N));
      // d_h += d_pq4 W4; d W4 = d_pq4^T h
      RC_TRY(tn_lin(s, w.d_pq4, 2 * H * M, 2 * H * M, pk.W4[b], H, nullptr, d_h, H, d_h_next, H, N, H));
      std::swap(d_h, d_h_next);
      RC_TRY(fork_w());
      RC_TRY(tn_wgrad(sw, w.d_pq4, 2 * H * M, w.h[(b + 1) * d.S], H, N, 2 * H * M, H, dW4, w));
    } else {                             // no row moves: the stage is the identity on x, its parameters get zeros (accumulating: nothing)
      HIP_TRY(hipMemcpyAsync(d_x_next, d_x, (size_t)N * 12, hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemsetAsync(dW4, 0, (size_t)2 * H * M * H * 4, s));
      for (int q = 0; q < M; ++q) {
        HIP_TRY(hipMemsetAsync(vec_of(k0 + q), 0, (size_t)8 * H * 4, s));
        if (!acc_w2[q]) HIP_TRY(hipMemsetAsync(og[q].d_W2, 0, (size_t)H * H * 4, s));
      }
    }
    std::swap(d_x, d_x_next);
    for (int q = 0; q < M; ++q) edge_mlp_grads(k0 + q, e.mlp[q].l1_w, e.mlp[q].l1_b, e.mlp[q].l2_b, dW4 + (size_t)q * 2 * H * H);
    cd.push_back(TnCopyDesc{G[e.head_w], vec_of(k0) + 6 * H, M == 2 ? vec_of(k0 + 1) + 6 * H : nullptr, H, acc(e.head_w)});   // d w3 (shared head)
    return DSBDD_OK;
  }

  // One sublayer backward: node MLP, then message stage.  Reads d_h (w.r.t. h[gi + 1]), leaves it w.r.t. h[gi]; adds the
  // message stage's coordinate gradient to d_x.  Overwrites da, dz, xcat, d_agg, d_pq, d_xg, gd0 and the edge scratch.
  // The weight gradients go to `sw`, the bias gradients to `sb`; they read dout, dz, xcat and d_pq, which nothing
  // overwrites before the join inside the NEXT message stage (mlp_backward, train_blocks.h) or the one in run().
  int sublayer(int b, int sl) {
    const int gi = b * d.S + sl;
    const TnSubIx& u = ix.subs[gi];
    const float* hin = w.h[gi];
    float* dout = d_h;
    RC_TRY(lin_grads(true, dout, H, w.act[gi], H, N, H, H, TnLinIx{u.n2_w, u.n2_b}));
    RC_TRY(tn_lin(s, dout, H, H, P[u.n2_w], H, nullptr, nullptr, 0, w.da, H, N, H));
    RC_TRY(launch_1d(tn_silu_bwd_kernel, NH, s, w.da, w.z[gi], w.dz, NH));
    RC_TRY(launch_1d(tn_cat_kernel, 2 * NH, s, hin, w.agg[gi], w.xcat, N, H));
    RC_TRY(lin_grads(true, w.dz, H, w.xcat, 2 * H, N, H, 2 * H, TnLinIx{u.n1_w, u.n1_b}));
    // d_hin = dz W1[:, :H] + d_out (residual);  d_agg = dz W1[:, H:]
    RC_TRY(tn_lin(s, w.dz, H, H, P[u.n1_w], 2 * H, nullptr, dout, H, d_h_next, H, N, H));
    RC_TRY(tn_lin(s, w.dz, H, H, P[u.n1_w] + H, 2 * H, nullptr, nullptr, 0, w.d_agg, H, N, H));
    std::swap(d_h, d_h_next);
    // message stage backward
    const dsbdd_train_mlp m = tn_msg_mlp(ix, P, pk, gi, H, w.pq[gi]);
    const int k = n_edge_mlps++;
    float* dWpq = w.dWpq + (size_t)gi * 2 * H * H;
    dsbdd_train_mlp_grad o{};
    o.dP = w.d_pq; o.dQ = w.d_pq + H; o.ldo = 2 * H; o.d_vec = vec_of(k); o.d_W2 = G[u.e2_w]; o.gd0 = w.gd0;
    if (want_in) HIP_TRY(hipMemsetAsync(w.gd0, 0, d.E1 * 4, s));
    RC_TRY(gcl_backward_impl(s, H, g, &m, w.x[b], c.normalization_factor, w.d_agg, &o, w.d_xg, w.scratch, w.scratch_bytes, sd, w.z2[gi], acc(u.e2_w)));
    RC_TRY(add_gd0(w.gd0));
    RC_TRY(launch_1d(tn_add_kernel, N3, s, d_x, w.d_xg, N3));
    RC_TRY(tn_lin(s, w.d_pq, 2 * H, 2 * H, pk.Wpq[gi], H, nullptr, d_h, H, d_h_next, H, N, H));
    std::swap(d_h, d_h_next);
    RC_TRY(fork_w());
    RC_TRY(tn_wgrad(sw, w.d_pq, 2 * H, hin, H, N, 2 * H, H, dWpq, w));
    edge_mlp_grads(k, u.e1_w, u.e1_b, u.e2_b, dWpq);
    if (ix.att) {
      cd.push_back(TnCopyDesc{G[u.att_w], vec_of(k) + 6 * H, nullptr, H, acc(u.att_w)});
      cd.push_back(TnCopyDesc{G[u.att_b], vec_of(k) + 7 * H, nullptr, 1, acc(u.att_b)});
    }
    return DSBDD_OK;
  }

  // egnn_new.py:233, dynamics.py:96-111 backward.  Reads d_h (w.r.t. h[0]); writes d_h0 and, if asked, d_hf_*.
  int embedding_and_encoders() {
    RC_TRY(lin_grads(false, d_h, H, w.h0, JP, N, H, d.D, ix.emb));
    RC_TRY(tn_lin(s, d_h, H, H, pk.emb.Wp, pk.emb.ldP, nullptr, nullptr, 0, w.d_h0, JP, N, d.D));
    RC_TRY(mlp2_bwd(enc_l, w.d_h0, JP, w.hf_l, a, w.d_hf_l, a, n_l, want_in));
    return mlp2_bwd(enc_p, pocket(w.d_h0, JP), JP, w.hf_p, r, w.d_hf_p, r, n_p, want_in);
  }

  // one workgroup row (grid y) per descriptor, as many launches as the by-value table needs
  template <class Table, class Desc>
  int launch_tables(void (*kernel)(Table), unsigned grid_x, const std::vector<Desc>& descs) {
    const size_t per = sizeof(Table::d) / sizeof(Desc);
    for (size_t o = 0; o < descs.size(); o += per) {
      Table tab{};
      const size_t n = std::min(per, descs.size() - o);
      std::copy_n(descs.begin() + o, n, tab.d);
      hipLaunchKernelGGL(kernel, dim3(grid_x, (unsigned)n), dim3(256), 0, s, tab);
      HIP_TRY(hipGetLastError());
    }
    return DSBDD_OK;
  }

  // the assembled first layers, the copied vectors, the edge-type embedding: reads dWpq, d_vec; writes demb_part and G[...]
  int assemble_grads() {
    RC_TRY(launch_tables(tn_unpack_kernel, 64, ud));
    RC_TRY(launch_tables(tn_copy_kernel, 1, cd));
    if (emb) {
      hipLaunchKernelGGL(tn_sum_parts_kernel, dim3(1), dim3(256), 0, s, (const float*)w.demb_part, n_edge_mlps, 3 * d.enf, 3 * d.enf,
                         G[ix.emb_tab], (int)acc(ix.emb_tab));
      HIP_TRY(hipGetLastError());
    }
    return DSBDD_OK;
  }

  // x enters through the first block (d_x), the velocity (- d_vel) and the input distances d0 of every edge MLP (gd0_tot)
  int input_grads(float* d_xh_lig, float* d_xh_pocket) {
    if (E > 0) {
      RC_TRY(radial_backward_impl(s, g, w.x0, w.gd0_tot, w.d_xg));
      RC_TRY(launch_1d(tn_add_kernel, N3, s, d_x, w.d_xg, N3));
    }
    RC_TRY(launch_1d(tn_sub_kernel, N3, s, d_x, w.d_vel, N3));
    return launch_1d(tn_join_grads_kernel, N, s, d_x, w.d_hf_l, a, w.d_hf_p, r, n_l, n_p, d_xh_lig, d_xh_pocket);
  }

  int run(const float* d_eps_lig, const float* d_eps_pocket, float* d_xh_lig, float* d_xh_pocket) {
    RC_TRY(tn_side_streams(net, &sd));
    if (sd && (sd->mask & SIDE_NODE_WG)) {
      // The bias gradients (ordered column sums, w.colscr) of the sublayers go to the OTHER side stream, idle outside the
      // coordinate stages: the weight-gradient chain of a sublayer (3 GEMMs + their reductions + 2 two-stage column sums)
      // was longer than the main chain's node work beside it, and the main chain waited for it in front of the W2 gradient
      sw = sd->wg; sb = sd->co;       // (w.wg / w.colscr are their scratch there)
    }
    RC_TRY(output_and_decoders(d_eps_lig, d_eps_pocket));
    for (int b = d.L - 1; b >= 0; --b) {
      RC_TRY(coord_stage(b));
      for (int sl = d.S - 1; sl >= 0; --sl) RC_TRY(sublayer(b, sl));
    }
    if (sd) { HIP_TRY(sd->link(sd->wg, s)); HIP_TRY(sd->link(sd->co, s)); }      // every weight / bias gradient of the blocks is complete from here on
    RC_TRY(embedding_and_encoders());
    RC_TRY(assemble_grads());
    return want_in ? input_grads(d_xh_lig, d_xh_pocket) : DSBDD_OK;
  }
};
