// Engine state (host side, included by engine.hip): error plumbing, the workspace layout, struct dsbdd_engine, the derived
// copies of the W2^T matrices and the environment switches.
#pragma once

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess)                                                          \
      return fail(DSBDD_ERR_LAUNCH, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)
// the same for the int codes of the library's own helpers
#define RC_TRY(expr)                       \
  do {                                     \
    const int _rc = (expr);                \
    if (_rc != DSBDD_OK) return _rc;       \
  } while (0)

// Every entry point launches on the caller's stream: make that stream's device the current one for the duration of the
// call (a module living on a GPU that is not torch's current device must not launch through another device's
// context), and restore it afterwards.  The NULL stream belongs to the current device by definition.
struct StreamDevice {
  int prev = -1;
  bool switched = false;
  explicit StreamDevice(void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!s) return;
    hipDevice_t d = 0;
    int cur = 0;
    if (hipStreamGetDevice(s, &d) != hipSuccess || hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); return; }
    if ((int)d != cur) { prev = cur; switched = hipSetDevice((int)d) == hipSuccess; }
  }
  ~StreamDevice() { if (switched) (void)hipSetDevice(prev); }
  StreamDevice(const StreamDevice&) = delete;
  StreamDevice& operator=(const StreamDevice&) = delete;
};

static inline int pad4(int v) { return (v + 3) & ~3; }
static inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
// Hands out consecutive 256-byte aligned pieces of one buffer (the training step's pack buffer, workspace and scratch).
// base == nullptr: sizes only (`off` is the total), every pointer null.
struct Carver {
  char* base;
  size_t off = 0;
  char* bytes(size_t n) { char* q = base ? base + off : nullptr; off += al256(n); return q; }
  float* f(size_t floats) { return reinterpret_cast<float*>(bytes(floats * 4)); }
  float* f1(size_t floats) { return f(floats > 0 ? floats : 1); }      // an empty buffer still gets an address of its own
};

// The one list of supported hidden_nf: run-time H -> compile-time constant.  f is a generic callable taking
// std::integral_constant<int, H> and returning hipError_t.
template <class F>
static hipError_t with_hidden(int H, F&& f) {
  switch (H) {
    case 64: return f(std::integral_constant<int, 64>{});
    case 128: return f(std::integral_constant<int, 128>{});
    case 192: return f(std::integral_constant<int, 192>{});
    case 256: return f(std::integral_constant<int, 256>{});
  }
  return hipErrorInvalidValue;
}
static bool hidden_nf_ok(int H) { return with_hidden(H, [](auto) { return hipSuccess; }) == hipSuccess; }

// ---- derived copies of the W2^T matrices ------------------------------------------------------------------------------
// Every [H][H] second-layer matrix of the edge MLPs (per block: inv_sublayers GCL, coord, cross) has up to four derived
// copies (EdgeMlpW::W2TP / W2TP16 / W2E / W2SK).  They share one workspace buffer: the region of a kind follows the regions
// of the kinds before it in this table, and holds one slot of `bytes` x H x H per matrix.
enum { W2_PERM, W2_PERM16, W2_EMU, W2_SPLITK, W2_KINDS };
struct W2Kind {
  size_t bytes;      // per element of the H x H matrix
  void (*pack)(hipStream_t s, const float* src, void* dst, int H);
};
template <class T, void (*K)(const float*, T*, int)>
static void w2_pack(hipStream_t s, const float* src, void* dst, int H) {
  hipLaunchKernelGGL(K, dim3((H * H + 255) / 256), dim3(256), 0, s, src, static_cast<T*>(dst), H);
}
static const W2Kind kW2Kinds[W2_KINDS] = {
    {4, w2_pack<float, permute_w2t_kernel>},        // lane-grouped copy of the 32-edge kernels (edge_wave.h; packed in edge_mlp.h)
    {4, w2_pack<float, pack16_w2t_kernel>},         // lane-grouped copy of the 16-edge kernels (edge_wave16.h)
    {6, w2_pack<unsigned short, pack_w2e_kernel>},  // three bf16 planes of the emulated path (edge_wave.h)
    {4, w2_pack<float, pack_w2sk_kernel>}};         // per-wave rotated copy of the split-K kernels (edge_splitk.h)
static size_t w2_bytes_before(int kind) {      // of the kinds in front of `kind` (W2_KINDS: of all)
  size_t b = 0;
  for (int k = 0; k < kind; ++k) b += kW2Kinds[k].bytes;
  return b;
}
// which packed copies in the workspace are current (the W2^T kinds and the node-chain weights, node_chain.h)
struct DerivedReady { bool w2[W2_KINDS] = {}, chain = false; };

// ---- workspace ----------------------------------------------------------------------------------------------------------
// Every buffer of the bound workspace.  ws_carve() names each one once, in layout order.
struct Workspace {
  int *node_batch, *lig_off, *poc_off, *deg, *row_ptr, *erow, *ecol;
  int *act_flag, *act_ptr, *act_list;
  float *ed0, *x, *x_in, *xagg, *mean, *h0, *enc_tmp, *h, *t1, *agg, *pq, *pqg, *hout;
  char* w2copies;                       // the derived W2^T copies (kW2Kinds)
  float *agg_head, *xagg_head;          // partial sums of rows continuing from the previous wave tile
  int *scan_tmp, *seg_base, *tile_ctr;
  // second per-call list (edges with a ligand endpoint) and the static pocket-pocket list of the pocket frame
  int *erow2, *ecol2, *row_ptr2, *deg2, *scan_tmp2, *seg_base2;
  int *erow3, *ecol3, *row_ptr3, *deg3, *scan_tmp3, *seg_base3, *node_batch3, *lig_off3, *poc_off3, *twin;
  float *ed02, *ed03, *xframe, *aggB, *agg_headB;
  int* frame_rows;                      // pocket row (0-based in the pocket array) of every frame row
  // level-ordered list (level_list.h): pocket-conditioned calls that return the ligand part only
  int *lvl, *seg_rows, *seg_edges, *node_base, *edge_base, *lvl_cnt, *lvl_end, *lvl_list, *row_ptrL, *erowL, *ecolL;
  float* ed0L;
  unsigned long long* lvl_stats;
  float* wchain;                        // lane-major packed node-level weights of the row-owning node-phase kernel (node_chain.h)
  size_t total;                         // bytes
};

// The layout: every buffer is al256(size + 16) bytes, in this order.  base == nullptr: sizes only (total), no pointers.
static Workspace ws_carve(const dsbdd_config& c, int64_t nl, int64_t np, int64_t B, int64_t E, char* base) {
  const size_t N = (size_t)(nl + np), nB = (size_t)B, nE = (size_t)E;
  const size_t H = c.hidden_nf, JP = pad4(c.joint_nf + 1);
  const size_t LE = pad4(2 * (c.atom_nf > c.residue_nf ? c.atom_nf : c.residue_nf));
  const size_t PQ = (c.reflection_equivariant ? 2 : 4) * H;
  const size_t EL = 2 * nE + 32 * kLevels * nB;   // level-ordered list: ghost segment + one padded segment per (level, sample)
  const size_t NG = N + (size_t)np;               // + the ghost rows of a canonical pocket (forward cone)
  const size_t T = EL / 32 + 2;                   // wave tiles
  const size_t LB = kLevels * nB;                 // (level, sample) segments
  const size_t n_w2 = (size_t)c.n_layers * (c.inv_sublayers + 2);
  Workspace w{};
  size_t off = 0;
  auto take = [&](auto*& p, size_t count) {
    using T_ = std::remove_reference_t<decltype(*p)>;
    p = base ? reinterpret_cast<T_*>(base + off) : nullptr;
    off += al256(count * sizeof(T_) + 16);
  };
  take(w.node_batch, N); take(w.lig_off, nB + 1); take(w.poc_off, nB + 1);
  take(w.deg, NG); take(w.row_ptr, N + 1);           // (deg: + ghosts)
  take(w.erow, nE); take(w.ecol, nE); take(w.ed0, nE);
  take(w.x, NG * 3); take(w.x_in, N * 3); take(w.xagg, N * 6); take(w.mean, nB * 3);   // xagg[2]
  take(w.h0, N * JP); take(w.enc_tmp, N * LE);
  take(w.h, NG * H); take(w.t1, NG * H); take(w.agg, NG * H); take(w.pq, N * PQ); take(w.hout, N * JP);
  take(w.act_flag, N); take(w.act_ptr, N + 1); take(w.act_list, N);
  take(w.pqg, NG * 2 * H);                           // GCL P|Q
  take(w.w2copies, n_w2 * H * H * w2_bytes_before(W2_KINDS) + 4096);
  take(w.agg_head, 2 * T * H); take(w.xagg_head, 2 * T * 2 * 4);   // xagg_head[2][T][4] (16-edge tiles: 2 T slots)
  take(w.scan_tmp, N + 1); take(w.seg_base, 2 * nB + 1); take(w.tile_ctr, (size_t)kTileCtrInts);
  take(w.erow2, nE); take(w.ecol2, nE); take(w.ed02, nE); take(w.row_ptr2, N + 1); take(w.deg2, N);   // list 2
  take(w.scan_tmp2, N + 1); take(w.seg_base2, 2 * nB + 1);
  take(w.erow3, nE); take(w.ecol3, nE); take(w.ed03, nE); take(w.row_ptr3, N + 1); take(w.deg3, N);   // list 3
  take(w.scan_tmp3, N + 1); take(w.seg_base3, 2 * nB + 1);
  take(w.node_batch3, N); take(w.lig_off3, nB + 1); take(w.poc_off3, nB + 1); take(w.twin, N);
  take(w.xframe, N * 3); take(w.aggB, NG * H); take(w.agg_headB, T * H);   // aggB: ghost ids
  take(w.lvl, N); take(w.seg_rows, LB); take(w.seg_edges, LB);
  take(w.node_base, LB + 1); take(w.edge_base, LB + 1); take(w.lvl_cnt, 16); take(w.lvl_end, 16);
  take(w.lvl_list, NG); take(w.row_ptrL, NG + 1); take(w.erowL, EL); take(w.ecolL, EL); take(w.ed0L, EL);
  take(w.lvl_stats, 16); take(w.frame_rows, N);
  take(w.wchain, (size_t)c.n_layers * ((size_t)c.inv_sublayers * 5 * H * H + H * PQ) + 1024);
  w.total = off;
  return w;
}

struct dsbdd_engine : Workspace {
  dsbdd_config cfg;
  std::vector<const float*> slots;
  bool has_weights = false;
  // workspace (the buffers: struct Workspace)
  char* ws = nullptr;
  size_t ws_bytes = 0;
  int64_t cap_lig = 0, cap_poc = 0, cap_batch = 0, cap_edges = 0;
  bool lvl_stats_zeroed = false;
  int64_t cap_edgesL = 0;
  int prune = 1;                        // DSBDD_PRUNE=0: evaluate every row in every stage
  // forward cone (identical pockets): the first message stages evaluate only the rows the ligand can have influenced;
  // the rest take the values of the canonical pocket, computed once on ghost rows N .. N + n_ghost
  int cone = 1;                         // DSBDD_CONE=0: off, 1: when the cost model says it pays (default), 2: always
  int64_t ghost_slots = 0;              // slots of the ghost segment at the front of the level-ordered list
  int shell = 1;                        // DSBDD_OPT_SHELL: shell rows of the cone's ascending stages reuse the ghost rows' messages
  int tail = 1;                         // DSBDD_OPT_TAIL: the last round of the exact H = 256 message launches on quarter items (edge_wave.h);
                                        // 0 off, 1 on (default), n > 1: n in place of the resident workgroups in the rule (test hook); DSBDD_TAIL
  int chain_deal = 1;                   // DSBDD_OPT_CHAIN_DEAL: node_chain_kernel's rows by the min-max deal (chain_split.h ChainDeal); 0: ChainSplit; DSBDD_CHAIN_DEAL
  int64_t cap_shell = 0;                // slots of one shell list: a level's rows, one padded segment per sample
  // Memory of the shell stages: the shell lists (level_list.h, LevelArgs::sh_*) and the messages of the ghost segment,
  // [ghost_slots][H].  The bound workspace keeps its recorded layout and the message buffer's size is the frame's, not
  // known at bind time, so the engine owns this block: laid out by shell_memory (graph_cache.h) before the first call
  // that runs a shell stage -- eagerly, never inside a capture --, kept until the capacities or the frame outgrow it.
  char* shell_mem = nullptr;
  int64_t shell_key[3] = {0, 0, 0};     // node / batch / list capacity it was laid out for
  int *sh_seg = nullptr, *sh_deg = nullptr, *sh_ptr = nullptr, *sh_row = nullptr, *sh_col = nullptr, *sh_cnt = nullptr;
  float* sh_d0 = nullptr;
  unsigned long long* sh_stats = nullptr;
  float* msg_buf = nullptr;
  int64_t msg_cap = 0;                  // slots
  // plan of the last forward (host side): radius and ghost use of every message stage, level of the timed launches
  std::vector<int> plan_radius, plan_ghost;
  int plan_timed_level = kLevels - 1;
  // pocket frame of the running chain (dsbdd_engine_set_pocket_frame): raw pocket coordinates are rigid in
  // pocket-conditioning mode, so block 0's pocket-pocket messages are evaluated on them, separately
  bool frame = false;
  int64_t frame_nlig = 0, frame_npoc = 0, frame_batch = 0, frame_n3 = 0, frame_cap3 = 0;
  bool ghost_dirty = true;              // the ghost rows / ghost list segment must be (re)written before the next framed call
  bool h0_pocket_valid = false;         // the pocket rows of h0 hold this chain's encoded pocket features (a frame fixes the
                                        // pocket of a chain: coordinates up to translation AND features, which never change in
                                        // pocket-conditioning mode) -> framed calls after the first run the ligand encoder only
  int64_t cap_tiles = 0;                // wave tiles (32 edges) of the edge capacity
  int64_t cap_tiles16 = 0;              // the same in 16-edge tiles (edge_wave16.h)
  unsigned granule16 = 0;               // DSBDD_OPT_GRANULE16: bit g = message stage g, bit 16 + b = coordinate stage of block b
                                        // run on the 16-edge-granule kernels (default: none; DSBDD_GRANULE16=<mask> in the environment)
  unsigned splitk = 0;                  // DSBDD_OPT_SPLITK: the same bit layout -- stages that run on the split-K kernels (edge_splitk.h:
                                        // a workgroup owns 32 edges, wave w a quarter of the reduction dimension; hidden_nf 256 only)
  int emu = 0;                          // DSBDD_OPT_EMU: 0 = exact fp32 edge kernels (default), 6 / 9 = fp32 emulated on the bf16 matrix
                                        // cores with 6 / 9 partial products (edge_wave.h, "emulated path"); DSBDD_EMU=<k> in the environment
  DerivedReady derived;                 // which derived weight copies in the workspace are current
  float *trace_h = nullptr, *trace_x = nullptr;
  int n_cu = 256;
  int chain = 1;             // DSBDD_NODE_CHAIN=0: the three-launch node phase (node_linear.h) everywhere
  int64_t chain_min_rows = 0;      // (test hook; the choice of kernel must not depend on the batch size: bitwise batch invariance)
  int fold_scan = 1;   // DSBDD_FOLD_SCAN: 1 (default) = the level ordering's exclusive scans are computed by level_place_kernel
                       // itself (no single-workgroup level_scan_kernel launch) and the block-0 sample mean rides in levels_kernel;
                       // 0 = the separate launches.  (The same fold for the radius graph's own scan -- segment totals by
                       // integer atomics in the count pass -- was measured SLOWER in round 5, 19.8 k atomics on 128 counters:
                       // edges_kernel<false> 12 -> 129 us, profiles/r5k_*; its code was removed in round 6.)
  int lig_head = 1;    // DSBDD_LIG_HEAD=0: embedding_out / decoder / finalize as three launches also for ligand-only calls
  int edge_bperm = 1;  // edge_wave.h reads the B operand with 16-byte LDS loads from those copies (DSBDD_EDGE_BPERM=0: off)
  // optional timing of the dominant kernel (GCL edge stage) with HIP events
  int profile = 0;        // 0 off, k: the GCL launches of every k-th forward call are timed with HIP events
  int64_t prof_call = 0;
  bool time_now = false;
  std::vector<hipEvent_t> ev;   // pairs: start, stop
  size_t ev_used = 0;
  // hipGraph cache (graph_cache.h): the launch sequence of one dynamics call is captured once per argument
  // signature (pointers + sizes) and replayed; a sampling chain calls with identical
  // arguments every reverse step.  DSBDD_GRAPH=0 disables.
  struct GraphEntry {
    std::vector<uint64_t> key;
    int seen = 0;                 // 1st call runs eagerly (warm-up), 2nd captures, then replay
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::vector<int> plan_radius, plan_ghost;   // what dsbdd_engine_last_plan reports after a replay of this graph
    int plan_timed_level = 0;
    void destroy() { if (exec) (void)hipGraphExecDestroy(exec); if (graph) (void)hipGraphDestroy(graph); }
  };
  std::vector<GraphEntry> graphs;
  int use_graph = 1;
  int coord_split = 1; // edge_wave MODE_COORD: one workgroup per (tile, MLP) (DSBDD_COORD_SPLIT=0: per tile)
  int node_group = 1;  // coordinate projections + next block's P|Q in one launch (DSBDD_NODE_GROUP=0: separate)
  int edge_max_wg = 0;  // test hook (DSBDD_EDGE_MAX_WG): cap on the persistent edge grid, so that small problems
                        // run several tiles per workgroup (the path large batches take)
  int64_t n_replay = 0, n_capture = 0, n_eager = 0;
  unsigned long long* ts_buf = nullptr;   // -DDSBDD_TIMESTAMPS builds: [launches][64][16] marks of the edge kernels
  int ts_cap = 0, ts_next = 0;
  hipStream_t cap_stream = nullptr;   // capture happens here (the caller's stream may be the
                                      // legacy default stream, which cannot be captured)
  dsbdd_engine() : Workspace{} {}
  // captured graphs hold the raw weight / workspace pointers of the moment they were captured
  void drop_graphs() {
    for (GraphEntry& g : graphs) g.destroy();
    graphs.clear();
  }
  // new weights or a new workspace: every packed copy has to be made again
  void invalidate_derived() { derived = DerivedReady{}; }
  ~dsbdd_engine() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    drop_graphs();
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
    if (shell_mem) (void)hipFree(shell_mem);
  }
};

static int n_slots(const dsbdd_config& c) {
  return DSBDD_G_COUNT + c.n_layers * (c.inv_sublayers * DSBDD_GCL_COUNT + DSBDD_EQ_COUNT);
}
static int gcl_slot(const dsbdd_config& c, int block, int sub, int which) {
  return DSBDD_G_COUNT + block * (c.inv_sublayers * DSBDD_GCL_COUNT + DSBDD_EQ_COUNT) +
         sub * DSBDD_GCL_COUNT + which;
}
static int eq_slot(const dsbdd_config& c, int block, int which) {
  return DSBDD_G_COUNT + block * (c.inv_sublayers * DSBDD_GCL_COUNT + DSBDD_EQ_COUNT) +
         c.inv_sublayers * DSBDD_GCL_COUNT + which;
}

// whether the engine's options call for the copies of `kind`
static bool w2_enabled(const dsbdd_engine* e, int kind) {
  const int H = e->cfg.hidden_nf;
  switch (kind) {
    case W2_PERM: return e->edge_bperm && (H == 256 || H == 128);
    case W2_PERM16: return e->granule16 != 0;
    case W2_EMU: return e->emu != 0;
    // (edge_splitk.h: hidden_nf 256; no emulated form -- the mask is ignored with DSBDD_OPT_EMU)
    case W2_SPLITK: return e->splitk != 0 && H == 256 && !e->emu;
  }
  return false;
}
// the copy of `kind` of matrix `which` (0 .. inv_sublayers-1 GCL, then coord, cross) of block `blk`; nullptr: kind not enabled
static void* w2_copy(const dsbdd_engine* e, int kind, int blk, int which) {
  if (!w2_enabled(e, kind)) return nullptr;
  const dsbdd_config& c = e->cfg;
  const size_t HH = (size_t)c.hidden_nf * c.hidden_nf, n_w2 = (size_t)c.n_layers * (c.inv_sublayers + 2);
  return e->w2copies + n_w2 * HH * w2_bytes_before(kind) + ((size_t)blk * (c.inv_sublayers + 2) + which) * HH * kW2Kinds[kind].bytes;
}
// (re)pack every enabled kind that is not current (enqueue only)
static int w2_pack_missing(dsbdd_engine* e, hipStream_t s) {
  const dsbdd_config& c = e->cfg;
  for (int kind = W2_KINDS - 1; kind >= 0; --kind) {       // (last kind first: the order the launches have always had)
    if (!w2_enabled(e, kind) || e->derived.w2[kind]) continue;
    for (int blk = 0; blk < c.n_layers; ++blk)
      for (int which = 0; which < c.inv_sublayers + 2; ++which) {
        const float* src = which < c.inv_sublayers ? e->slots[gcl_slot(c, blk, which, DSBDD_GCL_E2_WT)]
                         : e->slots[eq_slot(c, blk, which == c.inv_sublayers ? DSBDD_EQ_C_W2T : DSBDD_EQ_X_W2T)];
        if (!src) continue;                                   // reflection-equivariant models have no cross MLP
        kW2Kinds[kind].pack(s, src, w2_copy(e, kind, blk, which), c.hidden_nf);
        HIP_TRY(hipGetLastError());
      }
    e->derived.w2[kind] = true;
  }
  return DSBDD_OK;
}

// ---- environment switches (README, "Switches") --------------------------------------------------------------------------
// false when NAME is unset; otherwise its value as atoi reads it, or (mask) as an unsigned C literal, base 0
static bool env_int(const char* name, long long* v, bool mask = false) {
  const char* s = getenv(name);
  if (!s) return false;
  *v = mask ? (long long)strtoul(s, nullptr, 0) : (long long)atoi(s);
  return true;
}
// NAME's value when it is set and lies in [lo, hi], otherwise dflt
static int env_int_in(const char* name, long long lo, long long hi, int dflt) {
  long long v;
  return env_int(name, &v) && v >= lo && v <= hi ? (int)v : dflt;
}
static void read_env_switches(dsbdd_engine* e) {
  long long v;
  const std::pair<const char*, int*> off_on_zero[] = {      // on by default; off only on a value that parses to 0
      {"DSBDD_GRAPH", &e->use_graph}, {"DSBDD_EDGE_BPERM", &e->edge_bperm}, {"DSBDD_COORD_SPLIT", &e->coord_split},
      {"DSBDD_NODE_GROUP", &e->node_group}, {"DSBDD_PRUNE", &e->prune}, {"DSBDD_LIG_HEAD", &e->lig_head},
      {"DSBDD_NODE_CHAIN", &e->chain}, {"DSBDD_CHAIN_DEAL", &e->chain_deal}};
  for (const auto& sw : off_on_zero) if (env_int(sw.first, &v) && v == 0) *sw.second = 0;
  if (env_int("DSBDD_FOLD_SCAN", &v)) e->fold_scan = v > 0 ? 1 : 0;
  if (env_int("DSBDD_GRANULE16", &v, true)) e->granule16 = (unsigned)v;
  if (env_int("DSBDD_SPLITK", &v, true)) e->splitk = (unsigned)v;
  if (env_int("DSBDD_EMU", &v)) e->emu = (v == 6 || v == 9) ? (int)v : 0;
  if (env_int("DSBDD_CONE", &v)) e->cone = v <= 0 ? 0 : (v >= 2 ? 2 : 1);
  if (env_int("DSBDD_NODE_CHAIN_MIN_ROWS", &v) && v >= 0) e->chain_min_rows = v;
  if (env_int("DSBDD_EDGE_MAX_WG", &v) && v > 0) e->edge_max_wg = (int)v;
  if (env_int("DSBDD_TAIL", &v) && v >= 0) e->tail = (int)v;
}
