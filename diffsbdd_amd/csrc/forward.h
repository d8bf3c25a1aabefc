// The launch sequence of one EGNNDynamics.forward (enqueue only; host side, included by engine.hip): the per-call plan
// (pocket frame, level pruning, forward cone) and the stages that are enqueued from it.
#pragma once

// the arguments of one dsbdd_dynamics_forward call
struct ForwardArgs {
  const float *xh_lig, *xh_pocket, *t;
  int64_t t_count;
  const int64_t *mask_lig, *mask_pocket;
  int64_t n_lig, n_pocket, batch;
  const int32_t *ext_row, *ext_col;
  int64_t ext_n_edges;
  float *eps_lig, *eps_pocket;
  int32_t* status;
};

// whether the engine's pocket frame applies to a call (its sizes are the frame's, no teacher-forced edges)
static bool frame_applies(const dsbdd_engine* e, const ForwardArgs& a) {
  return e->frame && !e->cfg.update_pocket_coords && !a.ext_row && a.n_lig == e->frame_nlig &&
         a.n_pocket == e->frame_npoc && a.batch == e->frame_batch;
}

// the residue encoder (dynamics.py:97) on the call's pocket features -> pocket rows of h0[:, 0:J]
static Mlp2Problem residue_encoder(const dsbdd_engine* e, const ForwardArgs& a) {
  const dsbdd_config& c = e->cfg;
  const int r = c.residue_nf, J = c.joint_nf, JP = pad4(J + 1);
  const float* const* W = e->slots.data();
  return Mlp2Problem{a.xh_pocket + 3, 3 + r, r, W[DSBDD_G_RES_ENC_W0T], pad4(2 * r), W[DSBDD_G_RES_ENC_B0], 2 * r,
                     W[DSBDD_G_RES_ENC_W1T], pad4(J), W[DSBDD_G_RES_ENC_B1], J, e->h0 + (size_t)a.n_lig * JP, JP,
                     (int)a.n_pocket};
}

// what one stage leaves for the next: which projections of the new h are already in place
struct StageState {
  bool pqg_ready = false;       // the next message stage's P|Q is in pqg
  bool chained_pq = false;      // ... produced by the node-phase launch of the stage before
  bool chained_coord = false;   // the coordinate projections rode in the block's last node-phase launch
};

// Per-call context: everything that is decided once at the top of a call, and the stages as functions over it.
struct Forward : ForwardArgs {
  dsbdd_engine* const e;
  const hipStream_t s;
  const bool ext = ext_row != nullptr;
  const dsbdd_config& c = e->cfg;
  const int H = c.hidden_nf, J = c.joint_nf, JP = pad4(J + 1);
  const int a = c.atom_nf, r = c.residue_nf, dl = 3 + a, dp = 3 + r;
  const int LE = pad4(2 * (a > r ? a : r));
  const int nlig = (int)n_lig, N = (int)(n_lig + n_pocket), B = (int)batch;
  const int n_mlp = c.reflection_equivariant ? 1 : 2;
  const int PQ = (c.reflection_equivariant ? 2 : 4) * H;
  const float* const* W = e->slots.data();
  // pocket-conditioning mode: the coordinate MLPs only touch edges whose row is a ligand
  // node, so their first-layer projections are needed for a subset of the nodes only
  const bool subset = !c.update_pocket_coords;

  // Pocket frame (pocket-conditioning chains): block 0's first message stage runs on the edges with a
  // ligand endpoint; the pocket-pocket part comes from the static list built by set_pocket_frame.
  const bool split0 = frame_applies(e, *this);
  // Ligand output only (eps_pocket == nullptr) in pocket-conditioning mode: the stages evaluate the rows the
  // ligand output depends on, prefixes of the level-ordered list (level_list.h)
  const bool prune = e->prune && subset && !ext && !eps_pocket && !e->trace_h && !e->trace_x && nlig > 0;
  const int G_stages = c.n_layers * c.inv_sublayers;
  // Forward cone (identical pockets, one t for the batch): after message stage g only the nodes within g + 1 hops of
  // a ligand node can differ from the ligand-free ("canonical") pocket network, which is evaluated once, on the ghost
  // rows N .. N + n_ghost (its stage-0 messages are the frame's pocket-pocket launch).  Stage g then computes the
  // rows of level <= min(g + 1, G - g); the rows the next stage reads beyond those get the canonical values.
  // Cost model: the canonical network is extra work -- its G/2 ascending stages on every ghost row (the frame's pockets:
  // frame_n3 rows, one per group of identical pockets) -- against the rows the cone's first stages skip.  On the
  // benchmark pocket the skipped part is (1 - 0.28) + (1 - 0.69) + (1 - 0.97) = 1.06 edge lists per call and the
  // pocket-pocket edges of the ghosts are 0.83 of a list per stage, so by edge counts the cone pays while the frame holds less
  // than 1.06 / (3 x 0.83) = 0.43 of the batch's pocket rows: this rule (option value 1) is kept for direct C-API callers.
  // MEASURED at B = 64 (profiles/r4n_cone_rule.md) the break-even is lower -- 12 distinct pockets of 64: 8.8 ms per chain
  // and ghost pocket (the ascending stages' short launches run at 0.63 instead of 0.75 of the peak) against 1.7 ms saved
  // per sample -- and a size-dependent rule inside the engine would let a batch and its half take different modes; the
  // DDPM modules therefore decide per chain from the pocket groups (5 groups <= batch) and pass 0 / 2.
  const bool cone_pays = e->cone >= 2 || 5 * e->frame_n3 <= 2 * (int64_t)n_pocket;
  const bool cone = prune && split0 && e->cone && cone_pays && t_count == 1 && G_stages >= 2;
  // with a frame, the frame's pockets are the ghost rows N .. N + n_frame_rows; in the level-ordered list they own the
  // first n_ghost entries of lvl_list and the first ghost_slots edge slots
  const int n_frame_rows = split0 ? (int)e->frame_n3 : 0;
  const int n_ghost = (split0 && prune) ? n_frame_rows : 0;
  const int64_t ghost_slots = (split0 && prune) ? e->ghost_slots : 0;
  // (the ghost rows are kept valid by frame_upkeep, which also covers the calls that replay a graph)
  static constexpr int LV = kLevels - 1;                // "everything"
  // ghost rows are evaluated while a later stage still reads canonical values: the ascending part of the radii
  const int g_ghost_last = ghost_last();
  int64_t edge_bound = e->cap_edges;           // edge_list(): the external list's length
  bool mean_in_levels = false;                 // edge_list(): block 0's sample mean was computed by levels_kernel
  // the list the stages after block 0's split run on
  const int* L_row = prune ? e->erowL : e->erow;
  const int* L_col = prune ? e->ecolL : e->ecol;
  const float* L_d0 = prune ? e->ed0L : e->ed0;
  const int* L_ptr = prune ? e->row_ptrL : e->row_ptr;
  const int L_cap = prune ? (int)e->cap_edgesL : (int)e->cap_edges;
  int64_t L_bound() const { return prune ? e->cap_edgesL : edge_bound; }
  // active nodes of the coordinate projections (ligand nodes + pocket nodes with a ligand neighbour) = the nodes of
  // level <= 1: with the level list they are its prefix (after the ghost entries), otherwise a scan + compaction
  const int* act_rows = prune ? e->lvl_list + n_ghost : e->act_list;
  const int* act_count = prune ? e->lvl_cnt + kLevels + 1 : e->act_ptr + N;
  const int n_upd = c.update_pocket_coords ? N : nlig;   // update_coords_mask, dynamics.py:130-132
  const int* e_all = prune ? e->lvl_end + kLevels + LV : e->row_ptr + N;   // (counted from the end of the ghost segment)
  const int* e_upd = prune ? e->lvl_end + kLevels : e->row_ptr + n_upd;    // edges are row-sorted: a prefix (level 0 = ligand rows)
  const bool can_sk = w2_enabled(e, W2_SPLITK);     // the split-K masks apply (hidden_nf 256, not emulated)
  // packed weights of the row-owning node-phase kernel: per (block, sublayer) node MLP layer 1 [2H -> H], layer 2
  // [H -> H] and the message stage's first-layer projection [H -> 2H]; per block the coordinate projections [H -> PQ]
  const bool use_chain = e->chain && (H == 256 || H == 192 || H == 128) && N >= e->chain_min_rows;
  const size_t chain_blk = (size_t)c.inv_sublayers * 5 * H * H + (size_t)H * PQ;

  Forward(dsbdd_engine* e_, hipStream_t s_, const ForwardArgs& args) : ForwardArgs(args), e(e_), s(s_) {}

  int radius_of(int g) const {
    const int bw = G_stages - g, fw = g + 1;
    const int r = cone ? (bw < fw ? bw : fw) : bw;
    return r < LV ? r : LV;
  }
  int ghost_last() const {
    int last = -1;
    if (cone)
      for (int g = 0; g + 1 < G_stages; ++g) {
        const int rd = radius_of(g + 1) + 1 < LV ? radius_of(g + 1) + 1 : LV;
        if (rd > radius_of(g)) last = g;
      }
    return last;
  }
  // Shell (DSBDD_OPT_SHELL): the same argument edge by edge.  In an ascending stage g >= 1 the rows of level g + 1 -- the
  // stage's shell -- still hold canonical h (and P|Q), and so do their neighbours of level >= g + 1; pocket-pocket distances
  // do not depend on the ligand.  The message of an edge (shell row, column of level >= g + 1) is therefore the one the
  // ghost rows compute for the twin edge in the same launch, and every sample would compute it again.  Such a stage runs
  // list A = [ghost segment | rows of level <= g] of the main list and list B = the stage's shell list (level_list.h: the shell
  // rows' edges from columns of level <= g) in one persistent grid, the ghost tiles keep their messages, and
  // agg_complete_shell_kernel adds them to the shell rows' own sums in a fixed order.  Only for exact levels (g + 1 < LV)
  // and the default exact kernel at hidden_nf 256; the kernel variants of the 16-edge / split-K masks and the emulated
  // path run their stages as before.  Never switched by size: a sample's bits do not depend on its batch.
  bool shell_stage(int g) const {
    return cone && e->shell && g > 0 && g <= g_ghost_last && radius_of(g) == g + 1 && g + 1 < LV && g <= kShellLists &&
           H == 256 && !e->emu && w2_enabled(e, W2_PERM);
  }
  int n_shell() const {                        // shell lists to build: list g - 1 serves stage g
    int n = 0;
    for (int g = 1; g <= kShellLists && g < G_stages; ++g) if (shell_stage(g)) n = g;
    return n;
  }
  // rows of the nodes of level <= r (r >= kLevels - 1: everything), with or without the ghost rows in front
  // (the all-row stages keep the natural row order: walking the level list there as well, so that the coordinate
  //  projections ride in every stage's node-phase launch, was measured 0.5 % slower, profiles/r4f_ab.md)
  void rows_of(int r, bool ghost, NodeLinearArgs& a) const {
    if (!prune || (r >= LV && !ghost)) return;
    if (r > LV) r = LV;
    a.row_idx = ghost ? e->lvl_list : e->lvl_list + n_ghost;
    a.m_count = ghost ? e->lvl_cnt + r : e->lvl_cnt + kLevels + r;
    a.M = N + n_ghost;
  }
  const float* chain_w(int blk, int sub, int which) const {   // which: 0 N1, 1 N2, 2 E1 (P|Q), 3 coordinate (sub ignored)
    const float* base = e->wchain + (size_t)blk * chain_blk;
    if (which == 3) return base + (size_t)c.inv_sublayers * 5 * H * H;
    return base + (size_t)sub * 5 * H * H + (which == 0 ? 0 : (which == 1 ? 2 * H * H : 3 * H * H));
  }
  // P | Q projections of the first layer of message stage (blk, sub)'s edge MLP
  NodeLinearArgs gcl_pq(int blk, int sub) const {
    NodeLinearArgs a{e->h, H, H, nullptr, 0, 0, W[gcl_slot(c, blk, sub, DSBDD_GCL_E1_WT)], 2 * H, nullptr,
                     nullptr, 0, e->pqg, 2 * H, (int)N, 2 * H, 0, nullptr, nullptr};
    const int g = blk * c.inv_sublayers + sub;
    rows_of(radius_of(g) + 1, g <= g_ghost_last && g > 0, a);    // the stage reads its neighbours one level out
    return a;
  }
  // second-layer weights of one edge MLP, with every derived copy the engine's options enable
  EdgeMlpW edge_mlp(const float* P, const float* Q, const float* wd, const float* wd0, const float* tab, const float* W2T,
                    const float* b2, int blk, int which) const {
    return EdgeMlpW{P, Q, wd, wd0, tab, W2T, b2,
                    static_cast<const float*>(w2_copy(e, W2_PERM, blk, which)),
                    static_cast<const float*>(w2_copy(e, W2_PERM16, blk, which)), w2_copy(e, W2_EMU, blk, which),
                    static_cast<const float*>(w2_copy(e, W2_SPLITK, blk, which))};
  }

  // what dsbdd_engine_last_plan reports: radius and ghost use of every message stage, level of the timed launches
  void plan() {
    e->plan_radius.assign(G_stages, LV); e->plan_ghost.assign(G_stages, 0);
    e->plan_timed_level = LV;
    if (prune) {
      int rt = 0;
      for (int g = 0; g < G_stages; ++g) {
        e->plan_radius[g] = radius_of(g); e->plan_ghost[g] = g <= g_ghost_last;
        if (!(split0 && g == 0) && radius_of(g) > rt) rt = radius_of(g);
      }
      e->plan_timed_level = rt;
    }
  }

  // The two-layer MLPs of the two node sets (ligand, pocket): the first n in ONE launch when both fit mlp2_kernel;
  // otherwise each one that has an output as two node_linear launches through its part of enc_tmp.
  int mlp2_pair(const Mlp2Problem (&p)[2], int n) {
    if (mlp2_fits(p[0]) && mlp2_fits(p[1])) {
      HIP_TRY(launch_mlp2(s, p, n));
      return DSBDD_OK;
    }
    for (int k = 0; k < 2; ++k) {
      const Mlp2Problem& q = p[k];
      if (!q.out) continue;
      float* tmp = e->enc_tmp + (k ? (size_t)n_lig * LE : 0);
      HIP_TRY(nl(s, q.in, q.ld_in, q.K0, nullptr, 0, 0, q.W0T, q.ldw0, q.b0, nullptr, 0, tmp, LE, q.rows, q.M1, 1));
      HIP_TRY(nl(s, tmp, LE, q.M1, nullptr, 0, 0, q.W1T, q.ldw1, q.b1, nullptr, 0, q.out, q.ld_out, q.rows, q.n_out, 0));
    }
    return DSBDD_OK;
  }

  int assemble_and_encode() {
    // ---- masks -> offsets, split inputs ---------------------------------------
    {
      int work = N > B + 1 ? N : B + 1;
      if (work < 2 * B) work = 2 * B;
      hipLaunchKernelGGL(prep_assemble_kernel, dim3((work + 255) / 256), dim3(256), 0, s, mask_lig, nlig, mask_pocket,
                         (int)n_pocket, B, e->node_batch, e->lig_off, e->poc_off, e->tile_ctr, xh_lig, dl, xh_pocket, dp,
                         t, (int)t_count, e->x, e->x_in, e->h0, J, JP);
      HIP_TRY(hipGetLastError());
    }
    // (The encoder / embedding chain below needs only the assembled inputs and the edge list only the coordinates, but
    //  they stay on one stream: as parallel branches of the captured graph they cost 40 us per call more than the 46 us
    //  of serial kernels the fork hides, profiles/r4g_fork_ab.md.)
    // ---- encoders (dynamics.py:96-97) -> h0[:, 0:J] ----------------------------
    const Mlp2Problem enc[2] = {
        {xh_lig + 3, dl, a, W[DSBDD_G_ATOM_ENC_W0T], pad4(2 * a), W[DSBDD_G_ATOM_ENC_B0], 2 * a,
         W[DSBDD_G_ATOM_ENC_W1T], pad4(J), W[DSBDD_G_ATOM_ENC_B1], J, e->h0, JP, (int)n_lig},
        residue_encoder(e, *this)};
    // With a pocket frame the pocket's encoding is a constant of the chain: frame_upkeep computed it before this call
    // (eagerly, so that replayed graphs find it too)
    RC_TRY(mlp2_pair(enc, (split0 && e->h0_pocket_valid) ? 1 : 2));
    // ---- embedding (egnn_new.py:233) ---------------------------------------------
    HIP_TRY(nl(s, e->h0, JP, JP, nullptr, 0, 0, W[DSBDD_G_EMB_WT], H, W[DSBDD_G_EMB_B], nullptr, 0, e->h, H, N, H, 0));
    if (split0) {   // the ghost rows start from the embedded features of the pockets they stand for
      hipLaunchKernelGGL(gather_rows_kernel, dim3((e->frame_n3 + 3) / 4), dim3(kThreads), 0, s, e->h + (size_t)N * H,
                         (const float*)(e->h + (size_t)nlig * H), (const int*)e->frame_rows, (int)e->frame_n3, H);
      HIP_TRY(hipGetLastError());
    }
    return DSBDD_OK;
  }

  // ---- edges (dynamics.py:114, 169-187): the external list or the radius graph, then the level ordering --------------
  int edge_list() {
    if (ext) {
      HIP_TRY(zero_async(e->deg, (size_t)N * 4, s));
      if (ext_n_edges > 0) {
        hipLaunchKernelGGL(ext_edges_kernel, dim3((int)((ext_n_edges + 255) / 256)), dim3(256), 0, s, ext_row,
                           ext_col, (int)ext_n_edges, (const float*)e->x, e->erow, e->ecol, e->ed0, e->deg);
        HIP_TRY(hipGetLastError());
      }
      hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, (const int*)e->deg, e->row_ptr, N, SegAlign{},
                         (const int*)nullptr, (int*)nullptr, SegAlign{});
      HIP_TRY(hipGetLastError());
      edge_bound = ext_n_edges > 0 ? ext_n_edges : 1;
      if (subset) {
        hipLaunchKernelGGL(ext_flags_init_kernel, dim3((N + 255) / 256), dim3(256), 0, s, e->act_flag, nlig, N);
        HIP_TRY(hipGetLastError());
        if (ext_n_edges > 0) {
          hipLaunchKernelGGL(ext_flags_kernel, dim3((int)((ext_n_edges + 255) / 256)), dim3(256), 0, s, ext_row,
                             ext_col, (int)ext_n_edges, nlig, e->act_flag);
          HIP_TRY(hipGetLastError());
        }
      }
    } else {
      EdgeList2 l2{e->deg2, e->row_ptr2, e->erow2, e->ecol2, e->ed02, (int)e->cap_edges,
                   SegAlign{e->node_batch, e->lig_off, e->poc_off, nlig, B, e->scan_tmp2, e->seg_base2}};
      int rc = build_edges_impl(s, e->x, nlig, N, B, c, e->node_batch, e->lig_off, e->poc_off, e->deg,
                                e->row_ptr, e->erow, e->ecol, e->ed0, e->cap_edges, status,
                                subset ? e->act_flag : nullptr, e->scan_tmp, e->seg_base,
                                split0 ? &l2 : nullptr, 0, prune ? e->lvl : nullptr);
      if (rc) return rc;
      if (prune) {
        LevelArgs la{e->node_batch, e->lig_off, e->poc_off, nlig, B, e->lvl, e->deg, e->row_ptr, e->erow, e->ecol,
                     e->ed0, e->seg_rows, e->seg_edges, e->node_base, e->edge_base, e->lvl_cnt, e->lvl_end,
                     e->lvl_list, e->row_ptrL, e->erowL, e->ecolL, e->ed0L, (int)e->cap_edgesL, e->lvl_stats,
                     n_ghost, (int)ghost_slots, (int)e->cap_edges, nullptr, nullptr};
        // block 0's per-sample mean (coord2cross) rides in the levels launch: one launch less per pruned call
        mean_in_levels = e->fold_scan && n_mlp == 2;
        if (mean_in_levels) { la.mean_x = e->x; la.mean_out = e->mean; }
        // the shell lists ride in the level launches: levels_kernel counts, level_place_kernel places and writes them
        la.n_shell = e->shell_mem ? n_shell() : 0;         // (shell_memory ran in frame_upkeep; message_stage insists on it)
        la.sh_seg = e->sh_seg; la.sh_deg = e->sh_deg; la.sh_ptr = e->sh_ptr; la.sh_row = e->sh_row; la.sh_col = e->sh_col;
        la.sh_d0 = e->sh_d0; la.sh_cap = (int)e->cap_shell; la.sh_cnt = e->sh_cnt; la.sh_stats = e->sh_stats;
        if (!e->lvl_stats_zeroed) {
          HIP_TRY(zero_async(e->lvl_stats, 128, s));
          e->lvl_stats_zeroed = true;
        }
        hipLaunchKernelGGL(levels_kernel, dim3(B), dim3(kThreads), 0, s, la);
        HIP_TRY(hipGetLastError());
        if (!e->fold_scan) {
          hipLaunchKernelGGL(level_scan_kernel, dim3(1), dim3(1024), 0, s, la, N);
          HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(level_place_kernel, dim3(B), dim3(kThreads), 0, s, la, e->fold_scan ? 1 : 0);
        HIP_TRY(hipGetLastError());
        int64_t cb = (e->cap_edges + 255) / 256;
        if (cb > 2048) cb = 2048;
        if (cb < 1) cb = 1;
        hipLaunchKernelGGL(level_copy_kernel, dim3((int)cb), dim3(256), 0, s, la, N);
        HIP_TRY(hipGetLastError());
      }
    }
    if (subset && !prune) {   // sorted list of active nodes; its length stays on the device (act_ptr[N])
      hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, (const int*)e->act_flag, e->act_ptr, N, SegAlign{},
                         (const int*)nullptr, (int*)nullptr, SegAlign{});
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(compact_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const int*)e->act_flag,
                         (const int*)e->act_ptr, e->act_list, N);
      HIP_TRY(hipGetLastError());
    }
    return DSBDD_OK;
  }

  // the packed copies of the weights that are not current: the W2^T kinds (engine_state.h), the node-chain weights
  int derived_weights() {
    const int rc = w2_pack_missing(e, s);
    if (rc) return rc;
    if (use_chain && !e->derived.chain) {
      auto pack = [&](const float* WT, int ldw, int K, int Ncols, const float* dst) {
        hipLaunchKernelGGL(pack_b16_kernel, dim3((K * Ncols + 255) / 256), dim3(256), 0, s, WT, ldw, K, Ncols,
                           const_cast<float*>(dst));
      };
      for (int blk = 0; blk < c.n_layers; ++blk) {
        for (int sub = 0; sub < c.inv_sublayers; ++sub) {
          pack(W[gcl_slot(c, blk, sub, DSBDD_GCL_N1_WT)], H, 2 * H, H, chain_w(blk, sub, 0));
          pack(W[gcl_slot(c, blk, sub, DSBDD_GCL_N2_WT)], H, H, H, chain_w(blk, sub, 1));
          pack(W[gcl_slot(c, blk, sub, DSBDD_GCL_E1_WT)], 2 * H, H, 2 * H, chain_w(blk, sub, 2));
        }
        pack(W[eq_slot(c, blk, DSBDD_EQ_C1_WT)], PQ, H, PQ, chain_w(blk, 0, 3));
      }
      HIP_TRY(hipGetLastError());
      e->derived.chain = true;
    }
    return DSBDD_OK;
  }

  // One message stage (GCL, egnn_new.py:31-66): P|Q, edge launch, completion of the aggregates, node phase.
  int message_stage(int blk, int sub, StageState& st) {
    auto G = [&](int which) { return W[gcl_slot(c, blk, sub, which)]; };
    const bool first_split = split0 && blk == 0 && sub == 0;     // block 0's two-list launch of a framed call
    // P | Q projections of the edge MLP's first layer (those of a block's first sublayer
    // were launched together with the previous block's coordinate projections)
    if (sub > 0 && st.chained_pq) st.pqg_ready = true;           // produced by the previous sublayer's node-phase launch
    if (!st.pqg_ready) {
      NodeLinearArgs grp0[2];
      if (first_split) {
        // pocket frame: block 0 reads P|Q only at the active nodes (ligand nodes + pocket nodes with a ligand
        // neighbour: the endpoints of the ligand-endpoint list) and at the ghost rows (the frame's pockets)
        grp0[0] = gcl_pq(blk, sub);
        grp0[0].row_idx = act_rows; grp0[0].m_count = act_count; grp0[0].M = N;
        grp0[1] = gcl_pq(blk, sub);
        grp0[1].A1 = e->h + (size_t)N * H; grp0[1].C = e->pqg + (size_t)N * 2 * H; grp0[1].M = n_frame_rows;
        grp0[1].row_idx = nullptr; grp0[1].m_count = nullptr;
      }
      if (!(first_split && launch_node_group(s, grp0, 2) == hipSuccess)) {
        (void)hipGetLastError();
        HIP_TRY(launch_node_linear(s, gcl_pq(blk, sub)));
        if (first_split) HIP_TRY(launch_node_linear(s, grp0[1]));       // the ghost rows separately
      }
    }
    st.pqg_ready = false;
    const int g = blk * c.inv_sublayers + sub;
    const int radius = radius_of(g);               // this stage computes the nodes of level <= radius
    const bool ghost = g <= g_ghost_last;          // ... and the ghost rows of the canonical pocket
    const bool all_rows = !prune || radius >= LV;
    // list range of the stage: from the ghost segment or from its end, up to the end of level `radius`
    const int64_t begin = ghost ? 0 : ghost_slots;
    EdgeArgs ea{};
    ea.erow = L_row + begin; ea.ecol = L_col + begin; ea.ed0 = L_d0 + begin;
    ea.e_count = !prune ? e_all : (ghost ? e->lvl_end + radius : e->lvl_end + kLevels + radius);
    ea.e_cap = L_cap - (int)begin; ea.wt_base = (int)(begin / 32); ea.x = e->x;
    ea.n_lig = nlig; ea.n_nodes = N + n_frame_rows; ea.ldpq = 2 * H;
    ea.mlp[0] = edge_mlp(e->pqg, e->pqg + H, G(DSBDD_GCL_E1_WD), G(DSBDD_GCL_E1_WD0), G(DSBDD_GCL_E1_TAB),
                         G(DSBDD_GCL_E2_WT), G(DSBDD_GCL_E2_B), blk, sub);
    ea.mlp[1] = ea.mlp[0];
    // 16-edge-granule variant of this stage (engine option; never for block 0's two-list launch of a framed call)
    // (no emulated 16-edge kernel: with DSBDD_OPT_EMU the mask is ignored, a chain never mixes exact and emulated stages)
    const bool g16 = ((e->granule16 >> (g & 15)) & 1u) && !first_split && !e->emu;
    // split-K variant of this stage (engine option; takes precedence over the 16-edge mask; block 0's two-list launch too)
    const bool gsk = ((e->splitk >> (g & 15)) & 1u) && can_sk;
    ea.att_w = G(DSBDD_GCL_ATT_W); ea.att_b = G(DSBDD_GCL_ATT_B); ea.attention = c.attention;
    ea.agg = e->agg; ea.agg_head = e->agg_head; ea.tile_ctr = e->tile_ctr;
    ea.norm_factor = c.normalization_factor;
    if (first_split) {
      // (A) edges with a ligand endpoint, current coordinates -> agg / agg_head
      EdgeArgs a2 = ea;
      a2.erow = e->erow2; a2.ecol = e->ecol2; a2.ed0 = e->ed02; a2.e_count = e->row_ptr2 + N;
      a2.e_cap = (int)e->cap_edges; a2.wt_base = 0;          // (lists 2 and 3 count their wave tiles from 0)
      // (B) pocket-pocket edges of the frame (all samples, or the representative of identical pockets),
      //     raw pocket coordinates -> aggB / agg_headB.  (Running the small launch (B) on a second stream
      //     beside (A) was measured: 29.13 vs 29.42 ligands/s -- no gain, removed.)
      EdgeArgs a3 = ea;
      a3.erow = e->erow3; a3.ecol = e->ecol3; a3.ed0 = e->ed03; a3.e_count = e->row_ptr3 + e->frame_n3;
      a3.agg = e->aggB; a3.agg_head = e->agg_headB; a3.e_cap = (int)e->cap_edges; a3.wt_base = 0;   // (x: the ghost rows of e->x)
      // one launch: (B)'s few tiles ride behind (A)'s in the same persistent grid instead of paying a launch of
      // single-occupancy tile latency of their own (45 us for 35 tiles)
      a2.erow_b = a3.erow; a2.ecol_b = a3.ecol; a2.ed0_b = a3.ed0; a2.e_count_b = a3.e_count; a2.e_cap_b = a3.e_cap;
      a2.wt_base_b = a3.wt_base; a2.agg_b = a3.agg; a2.agg_head_b = a3.agg_head;
      HIP_TRY(launch_edge(e, s, MODE_GCL, a2, edge_bound + ((e->frame_cap3 + 127) / 128) * 128, false, gsk));
      hipLaunchKernelGGL(agg_complete2_kernel, dim3((N + n_ghost + 3) / 4), dim3(kThreads), 0, s, e->agg,
                         (const float*)e->agg_head, (const int*)e->row_ptr2, (const int*)e->deg2,
                         (const float*)e->aggB, (const float*)e->agg_headB, (const int*)e->row_ptr3,
                         (const int*)e->deg3, (const int*)e->twin, N, nlig, N, H, cone ? n_ghost : 0, (int)e->cap_tiles - 1);
      HIP_TRY(hipGetLastError());
    } else if (shell_stage(g) && !g16 && !gsk) {
      // shell stage: list A = [ghost segment | level <= g], list B = the shell rows' edges from columns of level <= g; the
      // shell rows are no rows of list A, so both lists write agg, and B's head slots are block 0's, free since its
      // completion.  Not bracketed by the profiling events: the timed launches stay whole prefixes of the main list.
      const int sl = g - 1;
      if (!e->msg_buf || e->msg_cap < ghost_slots) return fail(DSBDD_ERR_STATE, "shell stage without a message buffer");
      ea.e_count = e->lvl_end + (radius - 1);
      ea.erow_b = e->sh_row + (size_t)sl * e->cap_shell; ea.ecol_b = e->sh_col + (size_t)sl * e->cap_shell;
      ea.ed0_b = e->sh_d0 + (size_t)sl * e->cap_shell; ea.e_count_b = e->sh_cnt + sl; ea.e_cap_b = (int)e->cap_shell;
      ea.wt_base_b = 0; ea.agg_b = e->agg; ea.agg_head_b = e->agg_headB;
      ea.msg_out = e->msg_buf; ea.msg_tiles = (int)(ghost_slots / 32);
      HIP_TRY(launch_edge(e, s, MODE_GCL, ea, L_bound() + 128));
      const int n_rows = N + n_ghost;
      hipLaunchKernelGGL(agg_complete_shell_kernel, dim3((n_rows + 3) / 4), dim3(kThreads), 0, s, e->agg,
                         (const float*)e->agg_head, L_ptr, (const int*)e->deg, n_rows, H, (int)e->cap_tiles - 1,
                         (const int*)e->lvl, radius, nlig, N, (const float*)e->agg_headB, (const int*)e->sh_ptr,
                         (const int*)e->sh_deg, (const int*)e->row_ptr, (const int*)e->ecol, (int)e->cap_edges,
                         (const int*)e->twin, (const int*)(e->row_ptrL + N), (const float*)e->msg_buf, (int)ghost_slots,
                         1.0f / c.normalization_factor);
      HIP_TRY(hipGetLastError());
    } else {
      // (timed: the launches over the whole list only, so that every timed launch is the same work)
      // (a stage that would run a shell list but for its kernel variant is not timed either: `timed` is decided by the plan)
      const bool timed = e->time_now && (all_rows || radius == e->plan_timed_level) && !shell_stage(g) &&
                         e->ev_used + 2 <= e->ev.size();
      if (timed) HIP_TRY(hipEventRecord(e->ev[e->ev_used], s));
      HIP_TRY(launch_edge(e, s, MODE_GCL, ea, L_bound(), g16 && !gsk, gsk));
      if (timed) {
        HIP_TRY(hipEventRecord(e->ev[e->ev_used + 1], s));
        e->ev_used += 2;
      }
      // complete the rows whose edges span several wave tiles (ordered head partial sums, edge_mlp.h)
      const int n_rows = N + (ghost ? n_ghost : 0);
      hipLaunchKernelGGL(agg_complete_kernel, dim3((n_rows + 3) / 4), dim3(kThreads), 0, s, e->agg,
                         (const float*)e->agg_head, L_ptr, (const int*)e->deg, n_rows, H,
                         (int)((g16 && !gsk) ? e->cap_tiles16 : e->cap_tiles) - 1, (g16 && !gsk) ? 4 : 5);
      HIP_TRY(hipGetLastError());
    }
    return node_phase(blk, sub, radius, ghost, st);
  }

  // node MLP (egnn_new.py:21-24,56-57): h += W4 SiLU(W3 [h, agg] + b3) + b4, with the projections of the new h that can
  // ride in the same launch, then the canonical values of the rows the next stage reads beyond this one's
  int node_phase(int blk, int sub, int radius, bool ghost, StageState& st) {
    auto G = [&](int which) { return W[gcl_slot(c, blk, sub, which)]; };
    const int g = blk * c.inv_sublayers + sub;
    NodeLinearArgs n1{e->h, H, H, e->agg, H, H, G(DSBDD_GCL_N1_WT), H, G(DSBDD_GCL_N1_B), nullptr, 0, e->t1, H,
                      (int)N, H, 1, nullptr, nullptr};
    NodeLinearArgs n2{e->t1, H, H, nullptr, 0, 0, G(DSBDD_GCL_N2_WT), H, G(DSBDD_GCL_N2_B), e->h, H, e->h, H,
                      (int)N, H, 0, nullptr, nullptr};
    rows_of(radius, ghost, n1); rows_of(radius, ghost, n2);
    st.chained_pq = false; st.chained_coord = false;
    bool fill_pq = false;
    if (use_chain) {
      // one launch: the node MLP and every projection of the new h whose rows are a contiguous part of the MLP's
      // row list (node_chain.h) -- the coordinate projections (after the block's last sublayer), the next message
      // stage's P|Q when it reads exactly the rows this stage computes
      NodeChainArgs ca{};
      ca.row_idx = n1.row_idx; ca.m_count = n1.m_count; ca.M = n1.M; ca.do_mlp = 1;
      ca.h = e->h; ca.agg = e->agg;
      ca.W1p = chain_w(blk, sub, 0); ca.b1 = G(DSBDD_GCL_N1_B);
      ca.W2p = chain_w(blk, sub, 1); ca.b2 = G(DSBDD_GCL_N2_B);
      const bool last_sub = sub + 1 == c.inv_sublayers;
      const int first = ghost ? n_ghost : 0;               // the ghost rows lead the list of a ghost stage
      if (last_sub) {
        const int QW = n_mlp * H;
        const float* wc = chain_w(blk, 0, 3);
        if (!subset) {
          ca.proj[ca.n_proj++] = ChainProj{wc, e->pq, PQ, PQ, nullptr, 0};
          st.chained_coord = true;
        } else if (prune && n1.row_idx) {                  // active / ligand rows = prefixes of the level list
          ca.proj[ca.n_proj++] = ChainProj{wc, e->pq, PQ, QW, act_count, first};
          ca.proj[ca.n_proj++] = ChainProj{wc + (size_t)(QW / 16) * (H / 16) * 256, e->pq + QW, PQ, QW,
                                           e->lvl_cnt + kLevels, first};
          st.chained_coord = true;
        }
      }
      const bool has_next = !last_sub || blk + 1 < c.n_layers;
      if (has_next) {
        const int nb = last_sub ? blk + 1 : blk, ns = last_sub ? 0 : sub + 1;
        const NodeLinearArgs nx = gcl_pq(nb, ns);
        // the next stage's P|Q rides along when it reads exactly the rows this stage computes -- or, in a ghost stage,
        // those plus rows that are about to take the canonical values: the ghost rows' P|Q is computed here and
        // copied together with their h (canon_fill_kernel)
        const bool same_rows = nx.row_idx == n1.row_idx && nx.m_count == n1.m_count && nx.M == n1.M;
        if (same_rows || ghost) {
          ca.proj[ca.n_proj++] = ChainProj{chain_w(nb, ns, 2), e->pqg, 2 * H, 2 * H, nullptr, 0};
          st.chained_pq = true;
          fill_pq = ghost && !same_rows;
        }
      }
      ca.deal = e->chain_deal;
      HIP_TRY(launch_node_chain(s, ca, H, e->n_cu));
    } else {
      HIP_TRY(launch_node_linear(s, n1));
      HIP_TRY(launch_node_linear(s, n2));
    }
    if (ghost) {
      // the rows the next stage reads but this one did not compute: canonical values (and their P|Q, see above)
      const int hi = radius_of(g + 1) + 1 < LV ? radius_of(g + 1) + 1 : LV;
      if (hi > radius) {
        hipLaunchKernelGGL(canon_fill_kernel, dim3((N - nlig + 3) / 4), dim3(kThreads), 0, s, e->h,
                           (const int*)e->lvl, (const int*)e->twin, nlig, N, N, radius, hi, H,
                           fill_pq ? e->pqg : (float*)nullptr, 2 * H);
        HIP_TRY(hipGetLastError());
      }
    }
    return DSBDD_OK;
  }

  // The coordinate stage of a block (EquivariantUpdate, egnn_new.py:96-122): projections, edge launch, update.
  int coord_stage(int blk, StageState& st) {
    auto Q = [&](int which) { return W[eq_slot(c, blk, which)]; };
    // first-layer projections, column order [Q_coord | Q_cross | P_coord | P_cross]; the next
    // block's GCL P|Q projection reads the same h and shares the launch when it can
    const int QW = n_mlp * H;   // width of the Q (column-node) part
    NodeLinearArgs grp[kMaxGroup];
    int ng = 0;
    if (!st.chained_coord) {
      if (subset) {
        grp[ng++] = NodeLinearArgs{e->h, H, H, nullptr, 0, 0, Q(DSBDD_EQ_C1_WT), PQ, nullptr, nullptr, 0, e->pq, PQ,
                                   (int)N, QW, 0, act_rows, act_count};
        grp[ng++] = NodeLinearArgs{e->h, H, H, nullptr, 0, 0, Q(DSBDD_EQ_C1_WT) + QW, PQ, nullptr, nullptr, 0,
                                   e->pq + QW, PQ, (int)n_lig, QW, 0, nullptr, nullptr};
      } else {
        grp[ng++] = NodeLinearArgs{e->h, H, H, nullptr, 0, 0, Q(DSBDD_EQ_C1_WT), PQ, nullptr, nullptr, 0, e->pq, PQ,
                                   (int)N, PQ, 0, nullptr, nullptr};
      }
    }
    const int n_coord = ng;
    const bool want_next = blk + 1 < c.n_layers && !st.chained_pq;
    if (st.chained_pq && blk + 1 < c.n_layers) st.pqg_ready = true;
    if (want_next && use_chain) {
      // the next stage reads more rows than this one computed (ascending radii of the forward cone: the rest were
      // filled with canonical values above): its P|Q as a launch of its own, rows streamed from global memory
      const NodeLinearArgs nx = gcl_pq(blk + 1, 0);
      NodeChainArgs ca{};
      ca.row_idx = nx.row_idx; ca.m_count = nx.m_count; ca.M = nx.M; ca.do_mlp = 0; ca.h = e->h;
      ca.n_proj = 1;
      ca.proj[0] = ChainProj{chain_w(blk + 1, 0, 2), e->pqg, 2 * H, 2 * H, nullptr, 0};
      ca.deal = e->chain_deal;
      HIP_TRY(launch_node_chain(s, ca, H, e->n_cu));
      st.pqg_ready = true;
    } else if (want_next) {
      grp[ng++] = gcl_pq(blk + 1, 0);
    }
    if (ng > 0) {
      if (e->node_group && launch_node_group(s, grp, ng) == hipSuccess) {
        if (ng > n_coord) st.pqg_ready = true;
      } else {
        (void)hipGetLastError();
        for (int i = 0; i < n_coord; ++i) HIP_TRY(launch_node_linear(s, grp[i]));   // the coordinate projections only
      }
    }
    st.chained_pq = false;
    const int S = c.inv_sublayers;   // the coord / cross matrices follow the block's GCL ones in the derived copies
    EdgeArgs ea{};
    ea.erow = L_row + ghost_slots; ea.ecol = L_col + ghost_slots; ea.ed0 = L_d0 + ghost_slots; ea.e_count = e_upd;
    ea.e_cap = L_cap - (int)ghost_slots; ea.wt_base = (int)(ghost_slots / 32); ea.x = e->x;
    ea.n_lig = nlig; ea.n_nodes = N + n_frame_rows; ea.ldpq = PQ;
    ea.mlp[0] = edge_mlp(e->pq + QW, e->pq, Q(DSBDD_EQ_C_WD), Q(DSBDD_EQ_C_WD0), Q(DSBDD_EQ_C_TAB),
                         Q(DSBDD_EQ_C_W2T), Q(DSBDD_EQ_C_B2), blk, S);
    if (n_mlp == 2)
      ea.mlp[1] = edge_mlp(e->pq + QW + H, e->pq + H, Q(DSBDD_EQ_X_WD), Q(DSBDD_EQ_X_WD0), Q(DSBDD_EQ_X_TAB),
                           Q(DSBDD_EQ_X_W2T), Q(DSBDD_EQ_X_B2), blk, S + 1);
    else
      ea.mlp[1] = ea.mlp[0];
    ea.w3 = Q(DSBDD_EQ_W3); ea.node_batch = e->node_batch; ea.mean = e->mean;
    ea.norm_constant = c.norm_constant; ea.coords_range = c.coords_range; ea.use_tanh = c.use_tanh;
    ea.n_mlp = n_mlp; ea.xagg = e->xagg; ea.xagg_head = e->xagg_head;
    const bool csk = ((e->splitk >> (16 + (blk & 15))) & 1u) && can_sk;        // split-K variant of this stage (one sum per MLP)
    const bool c16 = ((e->granule16 >> (16 + (blk & 15))) & 1u) && !e->emu && !csk;   // 16-edge-granule variant of this stage
    ea.xagg_stride = (size_t)N * 3; ea.xhead_stride = (size_t)(c16 ? e->cap_tiles16 : e->cap_tiles) * 4;
    ea.tile_ctr = e->tile_ctr; ea.norm_factor = c.normalization_factor;
    ea.pass_split = (c16 || csk) ? 1 : e->coord_split;
    if (e->ts_buf && e->ts_next < e->ts_cap) ea.ts = e->ts_buf + (size_t)(e->ts_next++) * 1024;
    HIP_TRY(launch_edge(e, s, MODE_COORD, ea, L_bound(), c16, csk));
    const int n_q = ((e->coord_split || c16 || csk) && n_mlp == 2) ? 2 : 1;   // (the 16-edge / split-K kernels keep one sum per MLP)
    const int c_shift = c16 ? 4 : 5, c_max = (int)(c16 ? e->cap_tiles16 : e->cap_tiles) - 1;
    // few updated rows (the ligand's): one workgroup per sample updates them and reduces the next block's mean;
    // all rows updated (joint model): the wide per-component kernel, the mean stays a launch of its own
    const bool next_mean = subset && n_mlp == 2 && blk + 1 < c.n_layers;
    const CoordSums sums{e->xagg, e->xagg_head, n_q, ea.xagg_stride, ea.xhead_stride, L_ptr, e->deg, c_max, c_shift};
    if (!subset) {
      if (n_upd > 0) {
        hipLaunchKernelGGL(coord_update_kernel, dim3((3 * n_upd + 255) / 256), dim3(256), 0, s, e->x, sums, 3 * n_upd);
        HIP_TRY(hipGetLastError());
      }
    } else if (n_upd > 0 || next_mean) {
      hipLaunchKernelGGL(coord_update_mean_kernel, dim3(B), dim3(kThreads), 0, s, e->x, sums, n_upd,
                         (const int*)e->lig_off, (const int*)e->poc_off, nlig, next_mean ? e->mean : (float*)nullptr);
      HIP_TRY(hipGetLastError());
    }
    return DSBDD_OK;
  }

  // ---- embedding_out, decoders (egnn_new.py:241, dynamics.py:147-153) --------
  int output_head() {
    // ligand output only, pocket-conditioning mode: embedding_out + atom decoder + velocity + NaN flag in ONE launch
    // (csrc/lig_head.h; DSBDD_LIG_HEAD=0: the three launches below)
    LigHeadArgs lh{e->h, H, W[DSBDD_G_EMBOUT_WT], JP, W[DSBDD_G_EMBOUT_B], J,
                   W[DSBDD_G_ATOM_DEC_W0T], pad4(2 * a), W[DSBDD_G_ATOM_DEC_B0], 2 * a,
                   W[DSBDD_G_ATOM_DEC_W1T], pad4(a), W[DSBDD_G_ATOM_DEC_B1], a,
                   e->x, e->x_in, nlig, N, eps_lig, dl, status};
    if (e->lig_head && !eps_pocket && !c.update_pocket_coords && lig_head_fits(lh)) {
      HIP_TRY(launch_lig_head(s, lh));
      return DSBDD_OK;
    }
    HIP_TRY(nl(s, e->h, H, H, nullptr, 0, 0, W[DSBDD_G_EMBOUT_WT], JP, W[DSBDD_G_EMBOUT_B], nullptr, 0, e->hout, JP,
               eps_pocket ? N : n_lig, JP, 0));
    const Mlp2Problem dec[2] = {
        {e->hout, JP, J, W[DSBDD_G_ATOM_DEC_W0T], pad4(2 * a), W[DSBDD_G_ATOM_DEC_B0], 2 * a,
         W[DSBDD_G_ATOM_DEC_W1T], pad4(a), W[DSBDD_G_ATOM_DEC_B1], a, eps_lig + 3, dl, (int)n_lig},
        {e->hout + (size_t)n_lig * JP, JP, J, W[DSBDD_G_RES_DEC_W0T], pad4(2 * r), W[DSBDD_G_RES_DEC_B0], 2 * r,
         W[DSBDD_G_RES_DEC_W1T], pad4(r), W[DSBDD_G_RES_DEC_B1], r, eps_pocket ? eps_pocket + 3 : nullptr, dp,
         (int)n_pocket}};
    RC_TRY(mlp2_pair(dec, eps_pocket ? 2 : 1));
    // ---- velocity, NaN guard, joint-mode COM removal (dynamics.py:136,155-164) --
    hipLaunchKernelGGL(finalize_kernel, dim3(B), dim3(kThreads), 0, s, (const float*)e->x, (const float*)e->x_in,
                       (const int*)e->lig_off, (const int*)e->poc_off, nlig, c.update_pocket_coords, eps_lig, dl,
                       eps_pocket, dp, status);
    HIP_TRY(hipGetLastError());
    return DSBDD_OK;
  }

  int run() {
    if (N == 0) return DSBDD_OK;
    plan();
    int rc = assemble_and_encode();
    if (rc == DSBDD_OK) rc = edge_list();
    if (rc == DSBDD_OK) rc = derived_weights();
    StageState st;
    for (int blk = 0; blk < c.n_layers && rc == DSBDD_OK; ++blk) {
      // coord2cross needs the per-sample mean of the block's input x (pocket-conditioning mode, later blocks: computed
      // by the previous block's coordinate update; block 0 of a pruned call: by levels_kernel)
      if (n_mlp == 2 && (blk == 0 || !subset) && !(blk == 0 && mean_in_levels)) {
        hipLaunchKernelGGL(sample_mean_kernel, dim3(B), dim3(kThreads), 0, s, (const float*)e->x,
                           (const int*)e->lig_off, (const int*)e->poc_off, nlig, e->mean);
        HIP_TRY(hipGetLastError());
      }
      for (int sub = 0; sub < c.inv_sublayers && rc == DSBDD_OK; ++sub) rc = message_stage(blk, sub, st);
      if (rc == DSBDD_OK) rc = coord_stage(blk, st);
      if (rc != DSBDD_OK) break;
      if (e->trace_h)
        HIP_TRY(hipMemcpyAsync(e->trace_h + (size_t)blk * N * H, e->h, (size_t)N * H * 4, hipMemcpyDeviceToDevice, s));
      if (e->trace_x)
        HIP_TRY(hipMemcpyAsync(e->trace_x + (size_t)blk * N * 3, e->x, (size_t)N * 12, hipMemcpyDeviceToDevice, s));
    }
    return rc == DSBDD_OK ? output_head() : rc;
  }
};

static int forward_impl(dsbdd_engine* e, hipStream_t s, const ForwardArgs& args) { return Forward(e, s, args).run(); }
