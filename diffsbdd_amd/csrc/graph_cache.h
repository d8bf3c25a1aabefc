// Around the forward (host side, included by engine.hip): upkeep of the pocket frame's ghost rows, and the hipGraph cache
// that captures the launch sequence of a call once per argument signature and replays it.
#pragma once

// Ghost rows N .. N + n3 (the frame's pockets as nodes of their own: coordinates, degrees, positions) and the front
// segment of the level-ordered list, from the pristine frame data (list 3, xframe).  Re-run whenever a call without
// the frame may have written over them.
static int ghost_setup(dsbdd_engine* e, hipStream_t s) {
  const int n3 = (int)e->frame_n3, N = (int)(e->frame_nlig + e->frame_npoc);
  int64_t gb = (e->frame_cap3 + 255) / 256;
  if (gb > 1024) gb = 1024;
  hipLaunchKernelGGL(ghost_setup_kernel, dim3((int)gb), dim3(256), 0, s, (const int*)e->erow3, (const int*)e->ecol3,
                     (const float*)e->ed03, (const int*)e->row_ptr3, (const int*)e->deg3, n3, N, N, e->erowL,
                     e->ecolL, e->ed0L, (int)e->cap_edgesL, e->deg, e->row_ptrL, e->lvl_list,
                     (const float*)e->xframe, e->x);
  HIP_TRY(hipGetLastError());
  e->ghost_dirty = false;
  return DSBDD_OK;
}

// The engine-owned memory of the cone's shell stages (engine_state.h: shell_mem): laid out for the bound capacities and
// the frame's ghost segment, zero-filled (the counters start with it); a block that still fits is kept.
static int shell_memory(dsbdd_engine* e, hipStream_t s) {
  const int64_t N = e->cap_lig + e->cap_poc, B = e->cap_batch, SL = e->cap_shell;
  if (e->shell_mem && e->shell_key[0] == N && e->shell_key[1] == B && e->shell_key[2] == SL && e->msg_cap >= e->ghost_slots)
    return DSBDD_OK;
  HIP_TRY(hipStreamSynchronize(s));
  e->drop_graphs();                          // captured graphs hold the old block's pointers
  if (e->shell_mem) (void)hipFree(e->shell_mem);
  e->shell_mem = nullptr; e->msg_cap = 0;
  auto lay = [&](Carver c) {
    auto ints = [&](size_t n) { return reinterpret_cast<int*>(c.bytes(n * 4)); };
    e->sh_seg = ints((size_t)kShellLists * B); e->sh_deg = ints((size_t)N); e->sh_ptr = ints((size_t)N); e->sh_cnt = ints(4);
    e->sh_stats = reinterpret_cast<unsigned long long*>(c.bytes(64));
    e->sh_row = ints((size_t)kShellLists * SL); e->sh_col = ints((size_t)kShellLists * SL); e->sh_d0 = c.f((size_t)kShellLists * SL);
    e->msg_buf = c.f1((size_t)e->ghost_slots * e->cfg.hidden_nf);
    return c.off;
  };
  const size_t total = lay(Carver{nullptr});
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->shell_mem), total));
  HIP_TRY(hipMemset(e->shell_mem, 0, total));
  lay(Carver{e->shell_mem});
  e->shell_key[0] = N; e->shell_key[1] = B; e->shell_key[2] = SL; e->msg_cap = e->ghost_slots;
  return DSBDD_OK;
}

// Ghost rows of a pocket frame (set once per chain) share the node arrays with the real nodes: a call the frame
// does not apply to (other sizes, teacher-forced edges) may write over them -- eagerly or through a replayed
// graph --, so they are re-written from the pristine frame data before the next framed call, whichever way it runs.
static int frame_upkeep(dsbdd_engine* e, hipStream_t s, const ForwardArgs& a) {
  if (!frame_applies(e, a)) {
    e->ghost_dirty = true;
    e->h0_pocket_valid = false;
    return DSBDD_OK;
  }
  if (e->ghost_dirty) {
    int rc = ghost_setup(e, s);
    if (rc) return rc;
  }
  if (Forward(e, s, a).n_shell() > 0) RC_TRY(shell_memory(e, s));
  if (!e->h0_pocket_valid) {
    // the residue encoder on the chain's pocket features, once per chain (and again after a call the frame does not
    // apply to overwrote the rows): dynamics.py:97
    Mlp2Problem enc = residue_encoder(e, a);
    if (mlp2_fits(enc)) {
      HIP_TRY(launch_mlp2(s, &enc, 1));
      e->h0_pocket_valid = true;
    }
  }
  return DSBDD_OK;
}

// the cache entry of a call's signature (pointers + sizes), created on first sight; bounded: the oldest entry goes
static dsbdd_engine::GraphEntry* graph_entry(dsbdd_engine* e, hipStream_t s, const ForwardArgs& a) {
  std::vector<uint64_t> key = {(uint64_t)(uintptr_t)a.xh_lig, (uint64_t)(uintptr_t)a.xh_pocket, (uint64_t)(uintptr_t)a.t,
                               (uint64_t)a.t_count, (uint64_t)(uintptr_t)a.mask_lig, (uint64_t)(uintptr_t)a.mask_pocket,
                               (uint64_t)a.n_lig, (uint64_t)a.n_pocket, (uint64_t)a.batch, (uint64_t)(uintptr_t)a.eps_lig,
                               (uint64_t)(uintptr_t)a.eps_pocket, (uint64_t)(uintptr_t)a.status,
                               (uint64_t)(uintptr_t)e->ws, (uint64_t)(uintptr_t)e->slots.data()[0],
                               (uint64_t)(uintptr_t)s, (uint64_t)e->frame};
  for (auto& ge : e->graphs)
    if (ge.key == key) return &ge;
  if (e->graphs.size() >= 8) {
    e->graphs.front().destroy();
    e->graphs.erase(e->graphs.begin());
  }
  e->graphs.emplace_back();
  e->graphs.back().key = std::move(key);
  return &e->graphs.back();
}

// Capture the call's launch sequence on the engine's capture stream and instantiate it into g.  Returns the forward's own
// result; without a graph (g->exec stays null) graphs are switched off for this engine and the caller launches plainly.
static int graph_capture(dsbdd_engine* e, const ForwardArgs& a, dsbdd_engine::GraphEntry* g) {
  // (pack kernels enqueued during a capture have not run if the capture fails: remember what was current before)
  const DerivedReady before = e->derived;
  HIP_TRY(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal));
  const int rc = forward_impl(e, e->cap_stream, a);
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  const hipError_t ec = hipStreamEndCapture(e->cap_stream, &graph);
  const bool ok = rc == DSBDD_OK && ec == hipSuccess && graph &&
                  hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess && exec;
  if (!ok) {
    if (graph) (void)hipGraphDestroy(graph);
    e->use_graph = 0;                  // do not try again; fall back to plain launches
    e->derived = before;
    return rc;
  }
  g->graph = graph;
  g->exec = exec;
  g->plan_radius = e->plan_radius; g->plan_ghost = e->plan_ghost; g->plan_timed_level = e->plan_timed_level;
  return DSBDD_OK;
}

// One forward call through the cache: the first call with a signature runs eagerly (warm-up), the second captures,
// every later one replays.
static int forward_cached(dsbdd_engine* e, hipStream_t s, const ForwardArgs& a) {
  dsbdd_engine::GraphEntry* g = graph_entry(e, s, a);
  if (g->exec) {
    ++e->n_replay;
    HIP_TRY(hipGraphLaunch(g->exec, s));
    e->plan_radius = g->plan_radius; e->plan_ghost = g->plan_ghost; e->plan_timed_level = g->plan_timed_level;
    return DSBDD_OK;
  }
  ++e->n_eager;
  if (g->seen++ == 0) return forward_impl(e, s, a);      // first sight of this signature: plain launches
  // second call with the same arguments: capture the sequence, then replay it
  if (!e->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
  const int rc = graph_capture(e, a, g);
  if (rc != DSBDD_OK) return rc;
  if (!g->exec) return forward_impl(e, s, a);
  ++e->n_capture;
  HIP_TRY(hipGraphLaunch(g->exec, s));
  return DSBDD_OK;
}
