/*
 * diffsbdd_hip.h -- C-ABI of libdiffsbdd_hip.so: the MI355X (gfx950) kernels for
 * DiffSBDD's DDPM denoising hot path.
 *
 * The reference (/root/reference) is pure Python/PyTorch and has no FFI; the
 * interface replaced here is the Python call boundary of
 *
 *   EGNNDynamics.forward                 equivariant_diffusion/dynamics.py:87-167
 *   EGNNDynamics.get_edges               equivariant_diffusion/dynamics.py:169-187
 *   EGNN / EquivariantBlock / GCL /
 *   EquivariantUpdate .forward           equivariant_diffusion/egnn_new.py:31-244
 *   ConditionalDDPM.sample_p_zs_given_zt equivariant_diffusion/conditional_model.py:432-464
 *   EnVariationalDiffusion
 *     .sample_p_zs_given_zt              equivariant_diffusion/en_diffusion.py:503-557
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *     nothing is allocated, freed or owned by the library except the opaque
 *     engine object (host memory); device workspaces are caller-provided.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *     work is enqueued asynchronously, no entry point synchronises.
 *   - all floating point is fp32, row-major; node masks are int64 as in the
 *     reference (constants.py:8-9) and must be sorted ascending (the reference
 *     builds them with repeat_interleave, utils.py:146-154).
 *   - return value: 0 = ok, negative = DSBDD_ERR_*.  Device-side conditions
 *     (NaN in the velocity, edge-capacity overflow) are reported through the
 *     `status` word (bit mask DSBDD_STATUS_*), never by a host sync.
 *
 * The Python binding is diffsbdd_amd/_lib.py (ctypes); INTEGRATION.md shows
 * the stub a reference maintainer would add.
 */
#ifndef DIFFSBDD_HIP_H
#define DIFFSBDD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSBDD_ABI_VERSION 6

enum {
  DSBDD_OK = 0,
  DSBDD_ERR_ARG = -1,         /* bad argument / unsupported configuration   */
  DSBDD_ERR_STATE = -2,       /* weights or workspace not bound             */
  DSBDD_ERR_CAPACITY = -3,    /* sizes exceed the bound workspace           */
  DSBDD_ERR_LAUNCH = -4       /* hip launch error (see dsbdd_last_error)    */
};

enum {
  DSBDD_STATUS_NAN = 1,            /* dynamics.py:155-159                   */
  DSBDD_STATUS_EDGE_OVERFLOW = 2   /* more edges than edge_capacity         */
};

/* EGNNDynamics constructor arguments that reach the kernels
 * (dynamics.py:11-19; lightning_modules.py:137-159). */
typedef struct dsbdd_config {
  int32_t atom_nf, residue_nf, joint_nf, hidden_nf;
  int32_t n_layers, inv_sublayers;
  int32_t attention, use_tanh, update_pocket_coords, reflection_equivariant;
  int32_t edge_embedding_dim;         /* 0 = no edge-type embedding         */
  int32_t has_cutoff_ligand, has_cutoff_pocket, has_cutoff_interaction;
  float cutoff_ligand, cutoff_pocket, cutoff_interaction;
  float norm_constant, normalization_factor, coords_range;
} dsbdd_config;

typedef struct dsbdd_engine dsbdd_engine;

/* ---- weight slots --------------------------------------------------------
 * Weights are passed as a table of device pointers in the order below.  All
 * matrices are stored TRANSPOSED with respect to nn.Linear ([in][out], out
 * contiguous) with the leading dimension padded up to a multiple of 4 floats;
 * vectors are unpadded.  `JP` = round_up(joint_nf+1, 4), `H` = hidden_nf.
 *
 * global slots (DSBDD_G_*), then per block b = 0..n_layers-1:
 *   inv_sublayers x DSBDD_GCL_* slots, then DSBDD_EQ_* slots.            */
enum {
  DSBDD_G_ATOM_ENC_W0T = 0, DSBDD_G_ATOM_ENC_B0, DSBDD_G_ATOM_ENC_W1T, DSBDD_G_ATOM_ENC_B1,
  DSBDD_G_RES_ENC_W0T, DSBDD_G_RES_ENC_B0, DSBDD_G_RES_ENC_W1T, DSBDD_G_RES_ENC_B1,
  DSBDD_G_ATOM_DEC_W0T, DSBDD_G_ATOM_DEC_B0, DSBDD_G_ATOM_DEC_W1T, DSBDD_G_ATOM_DEC_B1,
  DSBDD_G_RES_DEC_W0T, DSBDD_G_RES_DEC_B0, DSBDD_G_RES_DEC_W1T, DSBDD_G_RES_DEC_B1,
  DSBDD_G_EMB_WT,      /* [JP][H]   rows >= joint_nf+1 are zero                */
  DSBDD_G_EMB_B,       /* [H]                                                  */
  DSBDD_G_EMBOUT_WT,   /* [H][JP]   cols >= joint_nf+1 are zero                */
  DSBDD_G_EMBOUT_B,    /* [JP]                                                 */
  DSBDD_G_COUNT
};
enum {
  DSBDD_GCL_E1_WT = 0, /* [H][2H]: edge_mlp.0.weight[:, :H]^T | [:, H:2H]^T     */
  DSBDD_GCL_E1_WD,     /* [H]    : edge_mlp.0.weight[:, 2H]   (current |d|^2)   */
  DSBDD_GCL_E1_WD0,    /* [H]    : edge_mlp.0.weight[:, 2H+1] (input   |d|^2)   */
  DSBDD_GCL_E1_TAB,    /* [3][H] : bias + edge-type-embedding contribution      */
  DSBDD_GCL_E2_WT,     /* [H][H] */
  DSBDD_GCL_E2_B,      /* [H]    */
  DSBDD_GCL_ATT_W,     /* [H]    (unused if !attention)                         */
  DSBDD_GCL_ATT_B,     /* [1]    */
  DSBDD_GCL_N1_WT,     /* [2H][H]: node_mlp.0.weight^T                          */
  DSBDD_GCL_N1_B,      /* [H]    */
  DSBDD_GCL_N2_WT,     /* [H][H] */
  DSBDD_GCL_N2_B,      /* [H]    */
  DSBDD_GCL_COUNT
};
enum {
  DSBDD_EQ_C1_WT = 0,  /* [H][4H]: coord col | cross col | coord row | cross row parts of
                          {coord,cross_product}_mlp.0.weight^T ([H][2H]: coord col |
                          coord row if reflection_equivariant)                  */
  DSBDD_EQ_C_WD,       /* coord_mlp: same five slots as the GCL edge MLP        */
  DSBDD_EQ_C_WD0, DSBDD_EQ_C_TAB, DSBDD_EQ_C_W2T, DSBDD_EQ_C_B2,
  DSBDD_EQ_X_WD,       /* cross_product_mlp (ignored if reflection_equivariant) */
  DSBDD_EQ_X_WD0, DSBDD_EQ_X_TAB, DSBDD_EQ_X_W2T, DSBDD_EQ_X_B2,
  DSBDD_EQ_W3,         /* [H]: the shared bias-free output layer (egnn_new.py:78) */
  DSBDD_EQ_COUNT
};

/* ---- engine ---------------------------------------------------------------*/
int dsbdd_abi_version(void);
const char* dsbdd_last_error(void);

int dsbdd_engine_create(const dsbdd_config* cfg, dsbdd_engine** out);
void dsbdd_engine_destroy(dsbdd_engine* e);
int dsbdd_engine_weight_slots(const dsbdd_engine* e);
int dsbdd_engine_set_weights(dsbdd_engine* e, const float* const* slots_host, int n_slots);

/* Workspace for up to (n_lig, n_pocket) nodes, `batch` samples and
 * `edge_capacity` directed edges (self loops included). */
size_t dsbdd_engine_workspace_bytes(const dsbdd_engine* e, int64_t n_lig, int64_t n_pocket,
                                    int64_t batch, int64_t edge_capacity);
int dsbdd_engine_bind_workspace(dsbdd_engine* e, void* workspace, size_t bytes, int64_t n_lig,
                                int64_t n_pocket, int64_t batch, int64_t edge_capacity);

/* Pocket frame of a pocket-conditioned sampling chain (update_pocket_coords = 0).
 * During such a chain the pocket moves rigidly (the reverse step only translates it with the ligand's
 * centre of mass, conditional_model.py:688-696), so its pocket-pocket radius graph and distances are
 * constants of the chain.  With a frame set, block 0 of dsbdd_dynamics_forward evaluates
 *     agg[node] = [sum over the node's edges with a ligand endpoint] + [sum over its pocket-pocket edges]
 * with the second part taken from the frame: a static edge list built here ONCE from the raw coordinates of the
 * frame's pockets.  The frame holds one REPRESENTATIVE pocket per group of identical pockets of the batch
 * (identical atom features and coordinates, e.g. prepare_pocket(repeats = n_samples), lightning_modules.py:738-750:
 * one group; a batch packed from several pockets: one per pocket; nothing shared: every sample its own):
 *   x_frame    [n_frame][3]  raw coordinates of the representatives' atoms, sample after sample
 *   mask_frame [n_frame]     sample id 0 .. batch_frame-1 of every frame row (sorted)
 *   frame_rows [n_frame]     row of that atom in the call's pocket array (0-based)
 *   twin_local [n_pocket]    frame row that stands for pocket row i (its own group's representative)
 * The pocket-pocket messages of block 0 are the same in every sample of a group (same features, same time step,
 * same distances) and are evaluated once per representative -- 82 % of that stage's edges at the benchmark batch.
 * Every grouping gives bit-identical results: the association A + B and the raw-coordinate distances are the same.
 * The representatives are also the rows of the canonical (ligand-free) pocket network of the FORWARD CONE of the
 * ligand-output-only calls (eps_pocket == NULL, t_count == 1; see dsbdd_dynamics_forward): stage g then computes the
 * rows within min(g + 1, G - g) hops of a ligand atom only, the rest comes from the representative.
 * A frame also fixes the pocket FEATURES of the calls it applies to (the feature columns of xh_pocket never change in
 * pocket-conditioning mode): the residue encoder runs in the first such call only, later calls reuse its output.
 * Set a new frame (or clear it) before calling with other pocket features.
 * The frame lives in the workspace; it is dropped by bind_workspace and by dsbdd_engine_clear_pocket_frame,
 * and only applies to calls with exactly (n_lig, n_pocket, batch).  edge_bound_frame = upper bound on the
 * frame's edge count (sum of squared pocket sizes of the frame samples + 32 per sample).  This function
 * synchronises the stream once (it reads the frame's edge count back). */
int dsbdd_engine_set_pocket_frame(dsbdd_engine* e, void* stream, const float* x_frame, const int64_t* mask_frame,
                                  const int32_t* frame_rows, const int32_t* twin_local, int64_t n_lig,
                                  int64_t n_pocket, int64_t batch, int64_t n_frame, int64_t batch_frame,
                                  int64_t edge_bound_frame);
int dsbdd_engine_clear_pocket_frame(dsbdd_engine* e);

/* Optional per-block trace (debug / parity tests): after every EquivariantBlock
 * the node features h [N][H] and coordinates x [N][3] are copied to
 * trace_h + b*N*H / trace_x + b*N*3.  NULL disables. */
int dsbdd_engine_set_trace(dsbdd_engine* e, float* trace_h, float* trace_x);

/* EGNNDynamics.forward (dynamics.py:87-167).
 *   xh_lig    [n_lig][3+atom_nf]       xh_pocket [n_pocket][3+residue_nf]
 *   t         [t_count] with t_count == batch or 1 (dynamics.py:104-111)
 *   ext_row/ext_col: optional teacher-forced edge list (int32, sorted by
 *     (row,col), node numbering [ligand | pocket]); NULL -> radius graph is
 *     built on device as dynamics.py:169-187 does.
 *   eps_lig   [n_lig][3+atom_nf]       eps_pocket [n_pocket][3+residue_nf] (may be NULL)
 *   status    int32 device word, OR-ed with DSBDD_STATUS_* (caller zeroes it)
 * eps_pocket == NULL in pocket-conditioning mode (what ConditionalDDPM's chains need, conditional_model.py:268-272)
 * lets the engine skip every row the ligand output does not depend on: message stage g of G evaluates the nodes
 * within G - g hops of a ligand atom (csrc/level_list.h; dsbdd_engine_last_plan reports the
 * radii).  eps_lig is the same up to fp32 summation order (different wave-tile boundaries). */
int dsbdd_dynamics_forward(dsbdd_engine* e, void* stream, const float* xh_lig,
                           const float* xh_pocket, const float* t, int64_t t_count,
                           const int64_t* mask_lig, const int64_t* mask_pocket, int64_t n_lig,
                           int64_t n_pocket, int64_t batch, const int32_t* ext_row,
                           const int32_t* ext_col, int64_t ext_n_edges, float* eps_lig,
                           float* eps_pocket, int32_t* status);

/* Timing of the dominant kernel (the fused GCL edge stage): with enable = k > 0,
 * the largest launches of that kernel (all of them when every stage runs on the whole edge list) inside every
 * k-th dsbdd_dynamics_forward call are bracketed by hipEventRecord on the caller's stream (up to max_launches timed
 * launches between reads); those calls run eagerly, the others may replay their
 * captured graph.  enable = 1 times every call, 0 switches timing off.  dsbdd_engine_profile_read waits for the recorded events, returns
 * the summed kernel time and the number of timed launches, and resets. */
int dsbdd_engine_profile(dsbdd_engine* e, int enable, int max_launches);
int dsbdd_engine_profile_read(dsbdd_engine* e, double* total_ms, int64_t* launches);

/* hipGraph bookkeeping.  dsbdd_dynamics_forward captures its launch sequence into a
 * hipGraph the second time it is called with an identical argument signature
 * (pointers + sizes + stream) and replays it afterwards -- a sampling chain calls it
 * with identical arguments every reverse step.  Eager launches are used while the
 * timing / trace hooks are active, for teacher-forced edge lists, or with
 * DSBDD_GRAPH=0.  Counters: graph replays, captures, eager calls. */
int dsbdd_engine_graph_stats(const dsbdd_engine* e, int64_t* replays, int64_t* captures, int64_t* eager);

/* Which rows the message stages of the last forward evaluated (host-side bookkeeping, no sync): radius[g] = hop
 * level up to which stage g computed its rows (4 = every row), ghost[g] = 1 when the stage also evaluated the
 * canonical pocket (identical pockets, csrc/forward.h "Forward cone"), timed_level = radius of the launches that
 * dsbdd_engine_profile brackets.  All 4 / 0 unless the call was a ligand-output-only call in pocket-conditioning
 * mode (eps_pocket == NULL), see csrc/level_list.h. */
int dsbdd_engine_last_plan(const dsbdd_engine* e, int32_t* radius, int32_t* ghost, int32_t capacity,
                           int32_t* n_stages, int32_t* timed_level);

/* Switches of the dead-row elimination (environment: DSBDD_PRUNE, DSBDD_CONE).  DSBDD_OPT_PRUNE: 0 / 1.
 * DSBDD_OPT_CONE: 0 = never, 1 = when the engine's cost model says the canonical-pocket network pays (default: the
 * frame's representatives hold at most 0.4 of the batch's pocket rows; the DDPM modules decide per chain from the
 * pocket groups with the measured break-even 0.2 and pass 0 / 2), 2 = always.  Cone on / off agree to rounding.
 * DSBDD_OPT_GRANULE16: bit mask of the stages that run on the 16-edge-granule variant of the fused edge kernels
 * (csrc/edge_wave16.h: a wave owns 16 edges on v_mfma_f32_16x16x4_f32 instead of 32 on 32x32x2; half the work unit, for
 * launches too small to fill the SIMDs a whole number of times): bit g (g < 16) = message stage g (block * inv_sublayers +
 * sublayer), bit 16 + b = the coordinate stage of block b.  Default 0 (environment: DSBDD_GRANULE16=<mask>).  The two
 * variants agree to rounding (< 1e-6 relative measured); each is bitwise reproducible; the mask is never changed by the
 * engine itself.
 * DSBDD_OPT_SPLITK (round 6; environment DSBDD_SPLITK=<mask>): bit mask, same layout as DSBDD_OPT_GRANULE16, of the stages
 * that run on the split-K variant of the fused edge kernels (csrc/edge_splitk.h: a WORKGROUP owns 32 edges, wave w a
 * quarter of the reduction dimension of the H x H layer for all H columns, B operand straight from L2, the four partial
 * accumulators reduce-scattered through LDS): a quarter of the default kernel's work unit (7 instead of 27 us of matrix
 * time per wave) with the A operand still evaluated once per element -- for launches of fewer tiles than the chip has
 * resident workgroups (crossdock_ca_cond, the free-running full-atom chain).  hidden_nf = 256 only; elsewhere, and with
 * DSBDD_OPT_EMU != 0, the mask is ignored.  A stage named in both masks runs the split-K kernel.  Same aggregation
 * protocol (head slots per 32-edge tile); results differ from the default kernel in the association of the K sum only
 * (four partial sums); bitwise reproducible; the mask is never changed by the engine itself.
 * DSBDD_OPT_EMU (round 5; environment DSBDD_EMU): arithmetic of the H x H layer of the fused edge kernels.  0 (default) =
 * exact fp32 on v_mfma_f32_32x32x2_f32.  6 / 9 = fp32 EMULATED on the bf16 matrix cores: both operands split exactly into
 * three bf16 terms, the 6 largest (or all 9) partial products accumulated in fp32 by v_mfma_f32_32x32x16_bf16
 * (csrc/edge_wave.h, "emulated path").  Same inputs, same edge order, same aggregation protocol; the results differ from
 * the exact path in rounding only (error vs a float64 evaluation <= 2 x the exact path's own -- the tested bound,
 * tests/test_gpu_emu.py; measured <= 1.1 x: profiles/r5_emu_error.md) and every parity test of the exact path holds at
 * the same tolerance.  Part of a chain's definition like the granule mask: never changed by the engine.  The
 * 16-edge-granule kernels and the training kernels have no emulated form: with DSBDD_OPT_EMU != 0 the DSBDD_OPT_GRANULE16
 * mask is IGNORED (every edge stage of a forward call runs the emulated 32-edge kernel, so a chain never mixes exact and
 * emulated stages); the training step (dsbdd_train_*) always computes in exact fp32.
 * (Round 5 also made the fma of cond_update_kernel / cond_repaint_kernel explicit: the un-fused reverse-step path
 * differs from earlier rounds' results by up to 1 ulp.)
 * DSBDD_OPT_SHELL (0 / 1, default 1; no environment variable): in the ascending stages g >= 1 of the forward cone the rows
 * of level g + 1 (the stage's "shell") evaluate only their edges from columns of level <= g; the messages of their
 * other edges are the canonical pocket's and are gathered from the ghost rows' messages of the same launch
 * (csrc/forward.h, "Shell").  hidden_nf = 256 with the default exact kernel only: a stage named in the 16-edge or split-K
 * mask, and every stage with DSBDD_OPT_EMU != 0, runs as with 0.  0 = the launch sequence without it, bit for bit.  On / off
 * differ in rounding (association of the row sum; canonical messages evaluated on the frame's raw pocket coordinates).
 * Part of a chain's definition like DSBDD_OPT_CONE: never changed by the engine, a sample's bits do not depend on its batch.
 * Memory: the shell lists and the ghost segment's messages live in a device block the ENGINE owns (the bound workspace
 * keeps its layout; the message buffer's size is the frame's).  It is allocated by the first dsbdd_dynamics_forward that
 * runs a shell stage after dsbdd_engine_bind_workspace / dsbdd_engine_set_pocket_frame changed the capacities or enlarged
 * the ghost segment: that one call synchronises `stream`, drops the captured graphs and calls hipMalloc, so it must not be
 * issued while the caller is capturing `stream` (the engine's own graph cache runs its first call of a signature eagerly).
 * DSBDD_OPT_TAIL (environment DSBDD_TAIL; default 1): the exact message kernels at hidden_nf = 256 finish a launch's last, partly
 * filled round of 128-edge tiles on QUARTER items -- a 32-edge wave tile evaluated by all four waves of a workgroup, split
 * over the column tiles (csrc/edge_wave.h).  0 = whole items only (the launch sequence without the option), 1 = on,
 * n > 1 = on with n in place of the resident workgroup count in the rule that picks the split tiles (a test hook: a launch
 * of a few dozen tiles then holds whole rounds and a split remainder).  Every value gives the same bits: the split keeps
 * every output's fmaf chain and every sum's order.  The workspace layout does not depend on it.
 * DSBDD_OPT_CHAIN_DEAL (0 / 1, default 1; environment DSBDD_CHAIN_DEAL): how node_chain_kernel deals its 16-row tiles to the
 * workgroups (csrc/chain_split.h).  0 = ranges of equal planned cost, cut at the problems' boundaries only in launches of
 * >= 3 tiles per workgroup (ChainSplit).  1 = cut at every boundary at every launch size and the ranges chosen so that the
 * slowest workgroup EXECUTES the least (ChainDeal: the smallest bottleneck whose ranges fit the grid; DESIGN.md §5
 * "Min-max deal").  Both give the same bits: every output element is one fmaf chain over k that does not depend on the
 * row split.  Part of a chain's definition like DSBDD_OPT_TAIL: the engine never switches it by size. */
enum { DSBDD_OPT_PRUNE = 0, DSBDD_OPT_CONE = 1, DSBDD_OPT_GRANULE16 = 2, DSBDD_OPT_EMU = 3, DSBDD_OPT_SPLITK = 4,
       DSBDD_OPT_SHELL = 5, DSBDD_OPT_TAIL = 6, DSBDD_OPT_CHAIN_DEAL = 7 };
int dsbdd_engine_set_option(dsbdd_engine* e, int which, int value);
/* current value of an option (what the environment / set_option left); DSBDD_ERR_ARG (< 0) for an unknown id */
int dsbdd_engine_get_option(const dsbdd_engine* e, int which);

/* Introspection of the last forward (device pointers into the workspace). */
enum {
  DSBDD_BUF_EDGE_ROW = 0, DSBDD_BUF_EDGE_COL, DSBDD_BUF_EDGE_D0, DSBDD_BUF_ROW_PTR,
  DSBDD_BUF_H, DSBDD_BUF_X, DSBDD_BUF_NODE_BATCH, DSBDD_BUF_DEG,
  /* level-ordered list of the last ligand-output-only call in pocket-conditioning mode (csrc/level_list.h):
   * level[N], nodes by (level, id) [N], cumulative node counts [5], edge prefix ends [5], and the list */
  DSBDD_BUF_LEVEL, DSBDD_BUF_LEVEL_LIST, DSBDD_BUF_LEVEL_COUNT, DSBDD_BUF_LEVEL_END,
  DSBDD_BUF_LROW_PTR, DSBDD_BUF_LEDGE_ROW, DSBDD_BUF_LEDGE_COL, DSBDD_BUF_LEDGE_D0,
  /* uint64[16]: sums over the calls since the workspace was bound of the 5 node counts, the 5 list prefix
   * lengths, the 5 edge counts (level <= r), and the number of such calls */
  DSBDD_BUF_LEVEL_STATS
};
int dsbdd_engine_buffer(const dsbdd_engine* e, int which, void** ptr_out);

/* Read-out of the shell lists of the last forward-cone call (csrc/level_list.h, LevelArgs::sh_*; DSBDD_OPT_SHELL): copies
 * `count` elements to host memory (synchronises the device).  List s = 0, 1 holds the rows of level s + 2 with their edges
 * from columns of level <= s + 1.  STATS: uint64[8] sums over the calls that built the lists, [3 s] edges of list s,
 * [3 s + 1] its slots (32-aligned sample segments), [3 s + 2] the rows' other edges = references to the canonical pocket's
 * messages, [6] calls; COUNT: int32[2] slots of either list; ROW / COL: int32 entries of list `list` (padding: row -1);
 * PTR / DEG: int32 per node, position and degree of a row of level 2 or 3 in its list.  `list` is ignored elsewhere.
 * DSBDD_ERR_STATE before the first call that ran a shell stage (the memory is laid out then). */
enum { DSBDD_SHELL_STATS = 0, DSBDD_SHELL_COUNT, DSBDD_SHELL_ROW, DSBDD_SHELL_COL, DSBDD_SHELL_PTR, DSBDD_SHELL_DEG };
int dsbdd_engine_shell_read(const dsbdd_engine* e, int which, int list, void* dst, int64_t count);

/* Read-out of the second edge list of the last call that had a pocket frame (csrc/radius_graph.h EdgeList2: the edges with
 * a ligand endpoint): copies `count` int32 to host memory (synchronises the device).  DEG: per node, its edges in that
 * list; ROW_PTR: [n_nodes + 1] the first slot of a row (32-aligned (sample, node set) segments), then the padded total. */
enum { DSBDD_LIST2_DEG = 0, DSBDD_LIST2_ROW_PTR };
int dsbdd_engine_list2_read(const dsbdd_engine* e, int which, void* dst, int64_t count);

/* ---- DDPM reverse-step updates -------------------------------------------
 * ConditionalDDPM.sample_p_zs_given_zt after the dynamics call
 * (conditional_model.py:448-464): in place
 *   z_lig <- z_lig/alpha_ts - c_eps*eps_lig + sigma*noise ; then the ligand
 *   centre of mass of each sample is subtracted from its ligand AND pocket x.
 * remove_com = 0 reproduces SimpleConditionalDDPM (conditional_model.py:717-721). */
int dsbdd_cond_reverse_update(void* stream, float* z_lig, float* xh_pocket, const float* eps_lig,
                              const float* noise, const int64_t* mask_lig,
                              const int64_t* mask_pocket, int64_t n_lig, int64_t n_pocket,
                              int64_t batch, int32_t atom_nf, int32_t residue_nf, float alpha_ts,
                              float c_eps, float sigma, int32_t remove_com);

/* EnVariationalDiffusion.sample_p_zs_given_zt after the dynamics call
 * (en_diffusion.py:530-556): both node sets are updated and the joint COM is
 * removed.  center_noise != 0: the x part (first 3 columns) of noise_* is made
 * COM-free over the sample's ligand + pocket rows inside the kernel
 * (sample_center_gravity_zero_gaussian_batch, en_diffusion.py:932-942);
 * center_noise = 0: the caller passes noise that is already COM-free. */
int dsbdd_joint_reverse_update(void* stream, float* z_lig, float* z_pocket, const float* eps_lig,
                               const float* eps_pocket, const float* noise_lig,
                               const float* noise_pocket, const int64_t* mask_lig,
                               const int64_t* mask_pocket, int64_t n_lig, int64_t n_pocket,
                               int64_t batch, int32_t atom_nf, int32_t residue_nf, float alpha_ts,
                               float c_eps, float sigma, int32_t center_noise);

/* ---- the other per-step pieces of the sampling loops ------------------------
 * One workgroup per sample, fixed reduction order: every result is a pure function
 * of that sample's rows (bitwise reproducible, independent of the batch composition).
 *
 * out[b][0..2] = mean over the rows of sample b of x[:, 0..2] (x [n_rows][ld], mask sorted);
 * torch_scatter.scatter_mean semantics (count clamped to >= 1). */
int dsbdd_segment_mean3(void* stream, const float* x, int32_t ld, const int64_t* mask, int64_t n_rows,
                        int64_t batch, float* out);

/* ConditionalDDPM.sample_normal_zero_com / noised_representation / sample_p_zt_given_zs
 * (conditional_model.py:140-183,420-430), in place:
 *   z_lig <- a * z_lig + sigma * noise ; remove_com: ligand COM subtracted from ligand and pocket x. */
int dsbdd_cond_affine_noise(void* stream, float* z_lig, float* xh_pocket, const float* noise,
                            const int64_t* mask_lig, const int64_t* mask_pocket, int64_t n_lig,
                            int64_t n_pocket, int64_t batch, int32_t atom_nf, int32_t residue_nf, float a,
                            float sigma, int32_t remove_com);

/* EnVariationalDiffusion.sample_combined_position_feature_noise / noised_representation /
 * sample_p_zt_given_zs (en_diffusion.py:302-317,479-501,559-578), in place on both node sets:
 *   z <- a * z + sigma * noise, noise optionally COM-centred (x part), result optionally COM-free.
 *   a = 0, sigma = 1 draws z_T. */
int dsbdd_joint_affine_noise(void* stream, float* z_lig, float* z_pocket, const float* noise_lig,
                             const float* noise_pocket, const int64_t* mask_lig, const int64_t* mask_pocket,
                             int64_t n_lig, int64_t n_pocket, int64_t batch, int32_t atom_nf,
                             int32_t residue_nf, float a, float sigma, int32_t center_noise,
                             int32_t remove_com);

/* One RePaint iteration of ConditionalDDPM.inpaint after the reverse step
 * (conditional_model.py:600-660).  On entry z_lig = denoised state, xh_pocket = pocket moved by
 * that step.  Known part noised to level s around the moved pocket, COM of the fixed atoms of both
 * parts aligned, blend by `fixed`, optional q(z_t | z_s) resampling step; the pocket follows every
 * translation.  scratch_lig [n_lig][3 + atom_nf]; com_pocket0 [batch][3]; fixed [n_lig]. */
int dsbdd_cond_repaint_update(void* stream, float* z_lig, float* xh_pocket, float* scratch_lig,
                              const float* xh0_lig, const float* com_pocket0, const float* fixed,
                              const float* noise_known, const float* noise_resample, const int64_t* mask_lig,
                              const int64_t* mask_pocket, int64_t n_lig, int64_t n_pocket, int64_t batch,
                              int32_t atom_nf, int32_t residue_nf, float alpha_s, float sigma_s,
                              float alpha_ts, float sigma_ts, int32_t resample, int32_t remove_com);

/* One launch per reverse step of a pocket-conditioned chain drawn from the keyed generator (round 5; replaces
 * dsbdd_randn_keyed x 1-3 + dsbdd_cond_reverse_update [+ dsbdd_cond_repaint_update] + the fill of the denoiser's time
 * word): the posterior update of conditional_model.py:448-464 with the noise of draw `draw_index` evaluated in place;
 * repaint = 1: followed by the RePaint iteration of :600-660 (known part noised with draw + 1), 2: and the q(z_t | z_s)
 * jump (draw + 2).  alpha_ts / sigma_ts are shared by the update and the jump (the same step); alpha_s / sigma_s noise
 * the known part.  t_word (optional): device float that receives t_next at the end -- the `t` of the NEXT
 * dsbdd_dynamics_forward call.  Results are bitwise those of the separate entry points on dsbdd_randn_keyed's output. */
int dsbdd_cond_step_keyed(void* stream, float* z_lig, float* xh_pocket, const float* eps_lig, float* scratch_lig,
                          const float* xh0_lig, const float* com_pocket0, const float* fixed, const int64_t* mask_lig,
                          const int64_t* mask_pocket, int64_t n_lig, int64_t n_pocket, int64_t batch, int32_t atom_nf,
                          int32_t residue_nf, float alpha_ts, float c_eps, float sigma, int32_t repaint, float alpha_s,
                          float sigma_s, float sigma_ts, int32_t remove_com, uint64_t seed, uint64_t draw_index,
                          int64_t sample_offset, const int64_t* sample_ids, float* t_word, float t_next);

/* One RePaint iteration of EnVariationalDiffusion.inpaint after the reverse step
 * (en_diffusion.py:742-809): known part q(z_s | x) with COM-centred noise, COM alignment over the
 * fixed ligand + pocket nodes, blend, optional jump back q(z_t | z_s) + joint COM removal. */
int dsbdd_joint_repaint_update(void* stream, float* z_lig, float* z_pocket, float* scratch_lig,
                               float* scratch_pocket, const float* xh0_lig, const float* xh0_pocket,
                               const float* fixed_lig, const float* fixed_pocket, const float* noise_known_lig,
                               const float* noise_known_pocket, const float* noise_jump_lig,
                               const float* noise_jump_pocket, const int64_t* mask_lig,
                               const int64_t* mask_pocket, int64_t n_lig, int64_t n_pocket, int64_t batch,
                               int32_t atom_nf, int32_t residue_nf, float alpha_s, float sigma_s,
                               float alpha_ts, float sigma_ts, int32_t jump);

/* Counter-based Gaussian noise (Philox4x32-10 + Box-Muller), a pure function of
 * (seed, global sample id, row within the sample, column, draw index, stream id), so
 * that a chain's noise does not depend on how samples are sharded over GPUs or packed
 * into batches.  out [n_rows][n_cols]; global sample id of row i =
 * sample_ids[mask[i]] when sample_ids != NULL (int64 [batch], device), else
 * mask[i] + sample_offset.
 *
 * Key domain.  With gs the global sample id and e = row_in_sample * n_cols + col (32 bit), a value is Box-Muller
 * (u1 = ((w0 >> 8) + 1) / 2^24 in (0, 1], u2 = (w1 >> 8) / 2^24 in [0, 1), |z| <= sqrt(48 ln 2)) on words 0 and 1 of
 *   Philox4x32-10(counter = { gs_lo, e, draw_lo, draw_hi ^ stream_id * 0x9E3779B1 ^ gs_hi }, key = { seed_lo, seed_hi }).
 * Distinct (seed, draw_index, stream_id, sample id, element) give distinct (counter, key) pairs, hence unrelated
 * streams, as long as draw_index < 2^32 and the sample id < 2^32: there the last counter word is stream_id * 0x9E3779B1
 * alone (an odd multiplier: a bijection of the stream ids) and the other words are the inputs verbatim.  Outside that
 * domain the three terms of the last word alias: (draw_index + 2^32, gs) and (draw_index, gs + 2^32) are the SAME
 * stream, and a stream_id can cancel a high half likewise.  Every caller in this project stays inside the domain (draw
 * indices count the draws of one chain, sample ids the molecules of one run); a caller that does not must not rely
 * on independence.  oracle/keyed_noise.py restates the generator on the host; tests/test_keyed_noise.py pins both
 * statements. */
int dsbdd_randn_keyed(void* stream, float* out, const int64_t* mask, int64_t n_rows,
                      int32_t n_cols, int64_t batch, int64_t sample_offset,
                      const int64_t* sample_ids, uint64_t seed, uint64_t draw_index,
                      uint32_t stream_id);

/* ---- individual kernels (unit tests, building blocks) --------------------*/
/* C[M][N] = act([A1 | A2] @ WT + bias) (+ R);  WT is [K1+K2][ldw]. act: 0 none, 1 SiLU */
int dsbdd_node_linear(void* stream, const float* A1, int32_t lda1, int32_t K1, const float* A2,
                      int32_t lda2, int32_t K2, const float* WT, int32_t ldw, const float* bias,
                      const float* R, int32_t ldr, float* C, int32_t ldc, int64_t M, int32_t N,
                      int32_t act);

/* The row split of the node-chain kernel (csrc/chain_split.h) as compiled, for every workgroup of a launch
 * of `grid` workgroups: which 16-row tiles each one runs, in order.  Host only -- no GPU is touched, it works where the
 * library loads without one.  M: logical rows (what the kernel has after min(M, *m_count)); projection q of n_proj <= 3
 * has proj_N[q] columns and covers proj_count[q] rows from row proj_first[q] (count 0x7fffffff: all that follow; both are
 * clamped to M inside).  header: uint32[5] = (Mw rows with work, total cost, V ranges planned, Vs ranges dealt out, forced
 * cuts 0 / 1), all zero when nothing is dealt out; pieces: int32 [capacity][3] = (workgroup, first row, tiles <= 6),
 * workgroup by workgroup.  Returns the number of pieces there are (capacity 0: only counts), or DSBDD_ERR_ARG. */
int64_t dsbdd_chain_split_host(int32_t M, int32_t do_mlp, int32_t n_proj, const int32_t* proj_N,
                               const int32_t* proj_first, const int32_t* proj_count, int32_t H, int32_t grid,
                               uint32_t* header, int32_t* pieces, int64_t capacity);

/* The same split as the DEVICE computes it: one small launch of `grid` workgroups that read the device scalars through the
 * kernel's own lines (m_count: device int32 or NULL; proj_count: host array of n_proj device int32 pointers, NULL entry =
 * all rows that follow) and write header, pieces (layout as above, device memory) and n_pieces (device int64: the pieces
 * there are, of which the first `capacity` are written).  Same argument checks as the kernel's launcher: H in {64, 128,
 * 192, 256}, at most 3 projections, M <= 8 << 20. */
int dsbdd_chain_split_probe(void* stream, int32_t M, const int32_t* m_count, int32_t do_mlp, int32_t n_proj,
                            const int32_t* proj_N, const int32_t* proj_first, const int32_t* const* proj_count,
                            int32_t H, int32_t grid, uint32_t* header, int32_t* pieces, int64_t capacity,
                            int64_t* n_pieces);

/* The twins of the two entry points above for the second policy (ChainDeal, DSBDD_OPT_CHAIN_DEAL = 1): same arguments, same
 * checks, same piece layout.  header: uint32[5] = (Mw rows with work, B executed load of the slowest range, G ranges the
 * launch may hold: grid, or segments x grid in the fallback, Vs ranges dealt out, fallback 0 / 1), all zero when nothing is
 * dealt out. */
int64_t dsbdd_chain_deal_host(int32_t M, int32_t do_mlp, int32_t n_proj, const int32_t* proj_N,
                              const int32_t* proj_first, const int32_t* proj_count, int32_t H, int32_t grid,
                              uint32_t* header, int32_t* pieces, int64_t capacity);
int dsbdd_chain_deal_probe(void* stream, int32_t M, const int32_t* m_count, int32_t do_mlp, int32_t n_proj,
                           const int32_t* proj_N, const int32_t* proj_first, const int32_t* const* proj_count,
                           int32_t H, int32_t grid, uint32_t* header, int32_t* pieces, int64_t capacity,
                           int64_t* n_pieces);

/* Radius graph (dynamics.py:169-187) -> edge list sorted by (row, col).
 * x [n_lig+n_pocket][3]; scratch: node_batch [N], lig_off/poc_off [batch+1],
 * deg [N], row_ptr [N+1] (row_ptr[N] = number of edges). */
int dsbdd_build_edges(void* stream, const float* x, const int64_t* mask_lig,
                      const int64_t* mask_pocket, int64_t n_lig, int64_t n_pocket, int64_t batch,
                      const dsbdd_config* cfg, int32_t* node_batch, int32_t* lig_off,
                      int32_t* poc_off, int32_t* deg, int32_t* row_ptr, int32_t* edge_row,
                      int32_t* edge_col, float* edge_d0, int64_t edge_capacity, int32_t* status);

/* ---- training step: backward of the fused edge stages -------------------------------------------
 * The reference trains through `loss.backward()` over its eager op stream (lightning_modules.py:337-363 ->
 * conditional_model.py:202-330 / en_diffusion.py:336-469 -> dynamics.py:87-167 -> egnn_new.py:31-58,96-122).  These entry
 * points are the hand-written forward / backward pairs of the two fused edge stages and the weight-gradient GEMM; the
 * Python side (diffsbdd_amd/train_hip.py) wraps them as torch.autograd.Function objects behind EGNNDynamics.forward.
 * Nothing of size [n_edges][H] is kept from the forward pass: the backward recomputes the edge activations from the
 * per-node projections.  All sums over edges are taken in a fixed order (bitwise reproducible gradients, no atomics).
 *
 * graph: the (row, col)-sorted list of dsbdd_build_edges plus rev (dsbdd_train_edge_rev: index of the edge (col, row)). */
typedef struct dsbdd_train_graph {
  const int32_t *erow, *ecol; const float* ed0;     /* [n_edges]                                    */
  const int32_t *row_ptr, *deg;                     /* [n_nodes + 1], [n_nodes]                     */
  const int32_t* rev;                               /* [n_edges] (backward only)                    */
  const int32_t *node_batch, *lig_off, *poc_off;    /* [n_nodes], [batch + 1], [batch + 1]          */
  int64_t n_lig, n_nodes, n_edges, batch;
} dsbdd_train_graph;

/* one edge MLP in its factorised form (csrc/edge_mlp.h): z1 = P[row] + Q[col] + d wd + d0 wd0 + tab[type] */
typedef struct dsbdd_train_mlp {
  const float *P, *Q; int32_t ldpq;   /* [n_nodes][ldpq] first-layer projections of the row / column node             */
  const float *wd, *wd0, *tab;        /* [H], [H], [3][H]                                                             */
  const float *W2, *W2T, *b2;         /* second layer: nn.Linear layout [out][in], its transpose [in][out], bias [H]  */
  const float *head, *head_b;         /* GCL: att_mlp.0.weight [H] and bias [1] (head = NULL: no attention);
                                         coordinate MLPs: the bias-free output layer [H] (egnn_new.py:78)             */
} dsbdd_train_mlp;

/* gradient destinations of one edge MLP */
typedef struct dsbdd_train_mlp_grad {
  float *dP, *dQ; int32_t ldo;        /* [n_nodes][ldo]: every row is written                                         */
  float* d_vec;                       /* [8][H]: d_wd, d_wd0, d_tab[0..2], d_b2, d_head, d_head_b (element 0)         */
  float* d_W2;                        /* [H][H] nn.Linear layout                                                      */
  float* gd0;                         /* [n_edges] gradient w.r.t. ed0                                                */
} dsbdd_train_mlp_grad;

size_t dsbdd_train_scratch_bytes(int32_t H, int64_t n_nodes, int64_t n_edges);
/* scratch of dsbdd_train_wgrad: enough for every K' <= K (the split-K plan is not monotonic in K, so a scratch sized
   for an edge count E also serves the calls on an edge prefix); dsbdd_train_wgrad_plan_bytes = what a call with exactly
   this K uses (never more than the former; a call whose plan does not fit returns DSBDD_ERR_CAPACITY) */
size_t dsbdd_train_wgrad_scratch_bytes(int64_t K, int64_t M, int64_t N);
size_t dsbdd_train_wgrad_plan_bytes(int64_t K, int64_t M, int64_t N);
int dsbdd_train_edge_rev(void* stream, const dsbdd_train_graph* g, int32_t* rev);
/* mean[b] = mean position of ALL nodes of sample b (coord2cross, egnn_new.py:307-310) */
int dsbdd_train_sample_mean(void* stream, const float* x, const dsbdd_train_graph* g, float* mean);

/* GCL.edge_model + aggregation (egnn_new.py:31-52): agg [n_nodes][H] = sum over the row's edges of m * att / nf */
int dsbdd_train_gcl_forward(void* stream, int32_t H, const dsbdd_train_graph* g, const dsbdd_train_mlp* m,
                            const float* x, float norm_factor, float* agg, void* scratch, size_t scratch_bytes);
/* d_agg [n_nodes][H] -> gradients of the MLP's inputs and parameters; d_x [n_nodes][3] = gradient through |x_i - x_j|^2 */
int dsbdd_train_gcl_backward(void* stream, int32_t H, const dsbdd_train_graph* g, const dsbdd_train_mlp* m,
                             const float* x, float norm_factor, const float* d_agg,
                             const dsbdd_train_mlp_grad* out, float* d_x, void* scratch, size_t scratch_bytes);

/* EquivariantUpdate.coord_model (egnn_new.py:96-122): x_out = x + sum over the edges of rows < n_upd of
 * (u T(phi) + cross T(phi_x)) / nf; m[0] = coord_mlp, m[1] = cross_product_mlp (n_mlp = 2), m[0].head = the shared
 * output layer.  mean [batch][3] from dsbdd_train_sample_mean (n_mlp = 2 only). */
int dsbdd_train_coord_forward(void* stream, int32_t H, const dsbdd_train_graph* g, const dsbdd_train_mlp* m,
                              int32_t n_mlp, const float* x, const float* mean, int64_t n_upd, float norm_constant,
                              float coords_range, int32_t use_tanh, float norm_factor, float* x_out, void* scratch,
                              size_t scratch_bytes);
/* d_xout [n_nodes][3] -> out[0 .. n_mlp) and d_x [n_nodes][3] = the gradient through the geometry (u, cross,
 * |x_i - x_j|^2; the identity path x -> x_out is NOT included), d_mean [batch][3].  e_upd = row_ptr[n_upd] (host value).
 * out[1].d_vec row 6 (d_head) belongs to the shared output layer as well: the caller adds it to out[0]'s. */
int dsbdd_train_coord_backward(void* stream, int32_t H, const dsbdd_train_graph* g, const dsbdd_train_mlp* m,
                               int32_t n_mlp, const float* x, const float* mean, int64_t n_upd, int64_t e_upd,
                               float norm_constant, float coords_range, int32_t use_tanh, float norm_factor,
                               const float* d_xout, const dsbdd_train_mlp_grad* out, float* d_x, float* d_mean,
                               void* scratch, size_t scratch_bytes);

/* gradient of the squared edge lengths d_e = |x_row - x_col|^2 (the edge list's ed0 when x is the call's input):
 * d_x[i] = sum over row i's edges of 2 (gd[e] + gd[rev e]) (x_i - x_col) */
int dsbdd_train_radial_backward(void* stream, const dsbdd_train_graph* g, const float* x, const float* gd, float* d_x);

/* C[M][N] = sum_k A[k][m] B[k][n]  (A [K][lda], B [K][ldb]; the weight gradient dY^T X of a Linear layer), split-K with
 * an ordered reduction.  out[n] = sum_m A[m][n] (bias gradient); scratch >= 4 * ceil(M / 32) * N bytes. */
int dsbdd_train_wgrad(void* stream, const float* A, int32_t lda, const float* B, int32_t ldb, int64_t K, int32_t M,
                      int32_t N, float* C, void* scratch, size_t scratch_bytes);
int dsbdd_train_colsum(void* stream, const float* A, int32_t lda, int64_t M, int32_t N, float* out, void* scratch,
                       size_t scratch_bytes);

/* ---- the training step as ONE launch sequence per direction (round 6; csrc/train_net.h) ---------------------------
 * Replaces, for the training step, the composition of the building blocks above by PyTorch autograd nodes:
 * lightning_modules.py:337-363 -> conditional_model.py:202-330 / en_diffusion.py:336-469 -> EGNNDynamics.forward
 * (dynamics.py:87-167) under autograd.  The reference-side binding is ONE torch.autograd.Function.
 *
 * params / grads: the module's parameter tensors in nn.Linear layout [out][in], in the order
 *   {atom_encoder.0, atom_encoder.2, atom_decoder.0, atom_decoder.2, residue_encoder.0, residue_encoder.2,
 *    residue_decoder.0, residue_decoder.2}.{weight, bias}, [edge_embedding.weight], egnn.embedding.{weight, bias},
 *   egnn.embedding_out.{weight, bias}, then per block i: per sublayer s gcl_s.{edge_mlp.0, edge_mlp.2, node_mlp.0,
 *   node_mlp.2, [att_mlp.0]}.{weight, bias}, gcl_equiv.{coord_mlp.0, coord_mlp.2}.{weight, bias}, coord_mlp.4.weight,
 *   [cross_product_mlp.{0, 2}.{weight, bias}]
 * (dsbdd_train_net_param_count entries; the aliased cross_product_mlp.4.weight IS coord_mlp.4.weight and is not listed:
 * its gradient is the sum over both MLPs).  Every gradient tensor is OVERWRITTEN.
 * graph: dsbdd_build_edges + dsbdd_train_edge_rev on the call's input coordinates (n_edges is a host value).
 * pack: persistent caller-owned buffer (dsbdd_train_net_pack_bytes) for the re-laid-out weights, rewritten by every
 * forward; ws: per-call workspace (dsbdd_train_net_workspace_bytes) that carries the activations from forward to backward
 * -- including the second-layer pre-activation z2 [E][H] of every edge MLP (4 E H bytes each; DSBDD_TRAIN_STORE_Z2=0:
 * recomputed in the backward pass instead) -- and two scratch sets for the coordinate stage's two MLPs.
 * Nothing is allocated by the library; no host synchronisation inside (beyond the first call's descriptor upload).
 * Streams: everything is ordered on `stream` as seen by the caller.  Inside, the backward runs the second coordinate
 * MLP's chain and the node-level / coordinate weight gradients on two internal non-blocking streams of the handle
 * (created by the first backward call; fork / join by events, all joined before the call's last launches on `stream`;
 * same kernels and reduction orders, so the gradients are bitwise those of DSBDD_TRAIN_STREAMS=0, one stream).
 * zero_nan: training mode replaces NaN velocities by 0 (dynamics.py:155-159); otherwise bit 1 of *status is raised.
 * e_upd (backward): row_ptr[n_lig] as a host value (pocket-conditioned models; ignored when update_pocket_coords).
 * d_xh_lig / d_xh_pocket: gradients w.r.t. the inputs, or NULL. */
typedef struct dsbdd_train_net dsbdd_train_net;
int dsbdd_train_net_create(const dsbdd_config* cfg, dsbdd_train_net** out);
void dsbdd_train_net_destroy(dsbdd_train_net* net);
int dsbdd_train_net_param_count(const dsbdd_train_net* net);
size_t dsbdd_train_net_pack_bytes(const dsbdd_train_net* net);
size_t dsbdd_train_net_workspace_bytes(const dsbdd_train_net* net, const dsbdd_train_graph* g);
int dsbdd_train_net_forward(dsbdd_train_net* net, void* stream, const dsbdd_train_graph* g, const float* const* params,
                            void* pack, size_t pack_bytes, void* ws, size_t ws_bytes, const float* xh_lig,
                            const float* xh_pocket, const float* t, int64_t t_count, int32_t zero_nan, float* eps_lig,
                            float* eps_pocket, int32_t* status);
int dsbdd_train_net_backward(dsbdd_train_net* net, void* stream, const dsbdd_train_graph* g, const float* const* params,
                             float* const* grads, void* pack, size_t pack_bytes, void* ws, size_t ws_bytes,
                             int64_t e_upd, const float* d_eps_lig, const float* d_eps_pocket, float* d_xh_lig,
                             float* d_xh_pocket);
/* Gradient accumulation over the micro-batches of one optimiser step.
 * _backward_acc: `accumulate` holds one flag per parameter slot (never NULL).  Flag 0: grads[i] is overwritten as by
 * dsbdd_train_net_backward.  Flag 1: grads[i] = grads[i] + g_i, where g_i is bit for bit what dsbdd_train_net_backward
 * would have written: the complete new gradient is formed first, in its fixed order, and the old value is added last with
 * one rounding, inside the kernel that does the last store of that gradient (no staging copy, no extra launch; on the
 * side streams where the overwriting stores run).  The gradient tensors may be views of ONE contiguous bucket.
 * _forward_held: dsbdd_train_net_forward with a trailing pack_is_current.  Non-zero: the weights cannot have changed since
 * the previous forward (same accumulation window), the two re-layout launches are skipped and the pack buffer is used as
 * it is; DSBDD_ERR_STATE unless the handle last packed exactly these parameter tensors into exactly this buffer. */
int dsbdd_train_net_forward_held(dsbdd_train_net* net, void* stream, const dsbdd_train_graph* g, const float* const* params,
                                 void* pack, size_t pack_bytes, void* ws, size_t ws_bytes, const float* xh_lig,
                                 const float* xh_pocket, const float* t, int64_t t_count, int32_t zero_nan, float* eps_lig,
                                 float* eps_pocket, int32_t* status, int32_t pack_is_current);
int dsbdd_train_net_backward_acc(dsbdd_train_net* net, void* stream, const dsbdd_train_graph* g, const float* const* params,
                                 float* const* grads, const uint8_t* accumulate, void* pack, size_t pack_bytes, void* ws,
                                 size_t ws_bytes, int64_t e_upd, const float* d_eps_lig, const float* d_eps_pocket,
                                 float* d_xh_lig, float* d_xh_pocket);

/* ---- the loss terms of the pocket-conditioned training step --------------------------------------------
 * ConditionalDDPM.forward around the network call (conditional_model.py:202-330 -> en_diffusion.py:109-262 for the terms):
 * normalisation, ligand-COM removal, z_t = alpha_t xh0 + sigma_t eps (centred again), and the twelve per-sample terms.
 * The reference-side binding calls _pre, then EGNNDynamics.forward (dsbdd_train_net_forward), then _post inside ONE
 * torch.autograd.Function whose backward is _post_backward (diffsbdd_amd/loss_head.py).
 * Predefined noise schedules only (gamma_table [timesteps + 1], en_diffusion.py:1158-1190); training mode (t may be 0: the
 * L0 terms are evaluated on z_t and masked by [t = 0], conditional_model.py:285-302).
 *   lig_x [n_lig][3], lig_h [n_lig][atom_nf] (raw one-hot), lig_mask [n_lig] int64 sorted ascending; pocket likewise;
 *   eps [n_lig][3 + atom_nf] standard normal draws; t_int [batch] integer-valued floats in [0, timesteps];
 *   logpn_table [n1_tab][n2_tab] = log p(n_lig | n_pocket) or NULL.
 * _pre writes z_t [n_lig][3 + atom_nf], xh_pocket [n_pocket][3 + residue_nf] and per_sample [dsbdd_loss_rows()][batch]:
 *   rows t, gamma_t, gamma_s, alpha_t, sigma_t, SNR_weight, neg_log_constants, kl_prior, loss_0_h (x [t = 0]), log_pN,
 *   delta_log_px, [t = 0]; optionally (non-NULL) the normalised batch x / norm_value_x, (h - norm_bias_h) / norm_value_h that
 *   normalize() (en_diffusion.py:880-895) leaves in the caller's dictionaries.
 * _post writes xh_hat [n_lig][3 + atom_nf] and out [dsbdd_loss_out_rows()][batch]: error_t (x [t > 0]), loss_0_x (x [t = 0]),
 *   mean |net_x|, mean |net_h| per sample.  _post_backward: d_net from the gradients of error_t / loss_0_x (per sample) and of
 *   xh_hat (or NULL).  Every per-sample sum is taken in a fixed order (the reference's scatter_add uses atomics). */
typedef struct {
  int32_t batch, n_lig, n_pocket, atom_nf, residue_nf, timesteps;
  int32_t remove_com;     /* 1: ConditionalDDPM (ligand COM removed from ligand and pocket, dof = 3 (n - 1)); 0: SimpleConditionalDDPM */
  int32_t vnode_idx;      /* class index of the virtual atom (its coordinates do not enter the error terms) or -1 */
  float norm_value_x, norm_value_h, norm_bias_h;
  int32_t n1_tab, n2_tab;
} dsbdd_loss_cfg;
/* Upper bound on the edge list dsbdd_build_edges writes for these (sorted) batch masks, and their validity, in one launch:
 * out[0] = 1 when both masks are sorted ascending with ids in [0, batch), out[1] = sum over the samples of the complete
 * graph's edges (dynamics.py:170-172) with every (sample, node set) segment rounded up to 32.  The host reads both words
 * (diffsbdd_amd/engine.py edge_capacity). */
int dsbdd_edge_capacity(void* stream, const int64_t* lig_mask, int64_t n_lig, const int64_t* pocket_mask, int64_t n_pocket,
                        int64_t batch, int64_t* out);
int dsbdd_loss_rows(void);
int dsbdd_loss_out_rows(void);
int dsbdd_loss_cond_pre(void* stream, const dsbdd_loss_cfg* cfg, const float* lig_x, const float* lig_h, const int64_t* lig_mask,
                        const float* pocket_x, const float* pocket_h, const int64_t* pocket_mask, const float* eps,
                        const float* t_int, const float* gamma_table, const float* logpn_table, float* z_t, float* xh_pocket,
                        float* per_sample, float* lig_x_norm, float* lig_h_norm, float* pocket_x_norm, float* pocket_h_norm);
int dsbdd_loss_cond_post(void* stream, const dsbdd_loss_cfg* cfg, const float* net, const float* eps, const float* z_t,
                         const float* lig_h, const int64_t* lig_mask, const float* per_sample, float* xh_hat, float* out);
int dsbdd_loss_cond_post_backward(void* stream, const dsbdd_loss_cfg* cfg, const float* net, const float* eps, const float* lig_h,
                                  const int64_t* lig_mask, const float* per_sample, const float* g_err, const float* g_l0x,
                                  const float* g_hat, float* d_net);

/* ---- the loss terms of the joint training step -------------------------------------------------------------------------
 * EnVariationalDiffusion.forward around the network call (en_diffusion.py:336-469), training mode, predefined schedules:
 * the same three launches for the model that diffuses ligand and pocket together.  Same dsbdd_loss_cfg; its remove_com and
 * vnode_idx fields are IGNORED here (the joint model neither centres the data nor masks virtual atoms).  Inputs as above;
 *   noise_lig [n_lig][3 + atom_nf], noise_pocket [n_pocket][3 + residue_nf] standard normal draws, x part NOT centred;
 *   logpn_table [n1_tab][n2_tab] = log p(n_lig, n_pocket) (the joint categorical) or NULL.
 * _pre writes eps_lig / eps_pocket (the noise with its x part centred over the sample's ligand + pocket rows, count clamped
 *   to >= 1: en_diffusion.py:559-578), z_lig = alpha_t xh_lig + sigma_t eps_lig and z_pocket likewise (xh normalised, not
 *   centred), per_sample [dsbdd_loss_rows()][batch] with the rows listed above -- neg_log_constants and delta_log_px with
 *   dof = 3 (n_lig + n_pocket - 1), kl_prior over both node sets (en_diffusion.py:109-155), loss_0_h = - sum of the
 *   categorical log-likelihood of z_t over ligand rows (atom_nf classes) and pocket rows (residue_nf classes) (x [t = 0]) --
 *   and optionally (non-NULL) the normalised batch.
 * _post writes xh_lig_hat [n_lig][3 + atom_nf] and out [dsbdd_loss_joint_out_rows()][batch]: error_t_lig, error_t_pocket
 *   (x [t > 0]), loss_0_x_ligand, loss_0_x_pocket (x [t = 0]), and the per-sample means of |net_lig_x|, |net_lig_h|,
 *   |net_pocket_x|, |net_pocket_h|.  _post_backward: d_net_lig and d_net_pocket from the per-sample gradients of the four
 *   error terms (each may be NULL) and of xh_lig_hat (or NULL; ligand only).  Fixed-order sums, no atomics. */
int dsbdd_loss_joint_out_rows(void);
int dsbdd_loss_joint_pre(void* stream, const dsbdd_loss_cfg* cfg, const float* lig_x, const float* lig_h, const int64_t* lig_mask,
                         const float* pocket_x, const float* pocket_h, const int64_t* pocket_mask, const float* noise_lig,
                         const float* noise_pocket, const float* t_int, const float* gamma_table, const float* logpn_table,
                         float* eps_lig, float* eps_pocket, float* z_lig, float* z_pocket, float* per_sample, float* lig_x_norm,
                         float* lig_h_norm, float* pocket_x_norm, float* pocket_h_norm);
int dsbdd_loss_joint_post(void* stream, const dsbdd_loss_cfg* cfg, const float* net_lig, const float* net_pocket,
                          const float* eps_lig, const float* eps_pocket, const float* z_lig, const int64_t* lig_mask,
                          const int64_t* pocket_mask, const float* per_sample, float* xh_lig_hat, float* out);
int dsbdd_loss_joint_post_backward(void* stream, const dsbdd_loss_cfg* cfg, const float* net_lig, const float* net_pocket,
                                   const float* eps_lig, const float* eps_pocket, const int64_t* lig_mask,
                                   const int64_t* pocket_mask, const float* per_sample, const float* g_err_lig,
                                   const float* g_err_pocket, const float* g_l0x_lig, const float* g_l0x_pocket,
                                   const float* g_xh_lig_hat, float* d_net_lig, float* d_net_pocket);

/* ---- the likelihood bound of given ligands (csrc/score.h; diffsbdd_amd/score.py) --------------------------------------------
 * ConditionalDDPM.nll_given_pocket: the evaluation branch of ConditionalDDPM.forward (conditional_model.py:202-330) for K
 * integer times per ligand instead of one random time, with all (ligand, slot) states of a call evaluated by few large
 * network calls.  Pocket-conditioned models, predefined schedules, no virtual atoms (cfg->vnode_idx must be -1).
 *   States: g = b * n_slots + k with n_slots = K + 1; k < K are the time slots, k = K is the zero slot (t = 0).  A chunk is
 *   the states [first_state, first_state + chunk_states), one network call; it may begin and end inside a ligand's slots.
 *   cfg->batch = number of ligands B; cfg->n_lig / n_pocket, lig_* / pocket_* = the caller's batch as for dsbdd_loss_cond_pre
 *   (pocket b belongs to ligand b; masks sorted ascending); cfg->n1_tab / n2_tab + logpn_table (required) = log p(n_lig |
 *   n_pocket), every size of the batch inside the table.
 *   Chunk arrays: state g owns the ligand rows [P(g) - P(first_state), + n_lig(b)) with P(g) = n_slots * (first row of ligand
 *   b) + k * n_lig(b), and its pocket rows likewise.  cap_lig / cap_pocket = rows of the chunk arrays; a state that does not
 *   fit writes no row and NaN scalars.
 * _rows(which): number of rows of per_state (0), per_ligand (1), out (2).
 * _pre: eps [cap_lig][3 + atom_nf] standard normal draws in chunk layout; t_int [B * n_slots] integer-valued floats in
 *   [1, timesteps] (zero slots: not read).  Writes z [cap_lig][3 + atom_nf], xh_pocket [cap_pocket][3 + residue_nf] (each state
 *   its own centred copy), mask_lig_out / mask_pocket_out (int64, state ids local to the chunk, sorted), t_out [chunk_states]
 *   = t / timesteps, per_state [_rows(0)][B * n_slots]: rows t, gamma_t, alpha_t, sigma_t, SNR_weight (and, by _post, error_t,
 *   loss_0_x, loss_0_h) in column g, and -- on the state that is a ligand's slot 0 -- per_ligand [_rows(1)][B]: kl_prior,
 *   neg_log_constants, delta_log_px, log_pN.
 * _post: net = the network's output for (z, xh_pocket, t_out).  Time slots: error_t = sum over the ligand's rows and all
 *   columns of (eps - net)^2; zero slots: loss_0_x = 0.5 sum over the coordinates, loss_0_h = - sum log p(h | z_0).
 * _reduce: once per call after every chunk; weights [B * n_slots] (zero slots: not read).  out [_rows(2)][B]: nll, loss_t,
 *   loss_0_x, loss_0_h, neg_log_constants, kl_prior, delta_log_px, log_pN with
 *     loss_t = sum_k ((-0.5 w[b][k]) SNR_weight) error_t   (k ascending, float32)
 *     nll    = (((loss_t + ((loss_0_x + loss_0_h) + neg_log_constants)) + kl_prior) - delta_log_px) - log_pN.
 * Every sum is taken in a fixed order; no atomics. */
int dsbdd_score_rows(int32_t which);
int dsbdd_score_cond_pre(void* stream, const dsbdd_loss_cfg* cfg, int32_t n_slots, int64_t first_state, int64_t chunk_states,
                         int64_t cap_lig, int64_t cap_pocket, const float* lig_x, const float* lig_h, const int64_t* lig_mask,
                         const float* pocket_x, const float* pocket_h, const int64_t* pocket_mask, const float* eps,
                         const float* t_int, const float* gamma_table, const float* logpn_table, float* z, float* xh_pocket,
                         int64_t* mask_lig_out, int64_t* mask_pocket_out, float* t_out, float* per_state, float* per_ligand);
int dsbdd_score_cond_post(void* stream, const dsbdd_loss_cfg* cfg, int32_t n_slots, int64_t first_state, int64_t chunk_states,
                          int64_t cap_lig, int64_t cap_pocket, const float* lig_h, const int64_t* lig_mask,
                          const int64_t* pocket_mask, const float* net, const float* eps, const float* z, float* per_state);
int dsbdd_score_reduce(void* stream, int64_t batch, int32_t n_slots, const float* weights, const float* per_state,
                       const float* per_ligand, float* out);

/* ---- the same bound under the joint model (csrc/score_joint.h; diffsbdd_amd/score.py nll_of_complex) ------------------------
 * EnVariationalDiffusion.nll_of_complex: the evaluation branch of EnVariationalDiffusion.forward (en_diffusion.py:336-469)
 * for K integer times per complex.  States, chunks, row offsets, cfg and the refusals are those of the entry points above;
 * the joint model noises and scores BOTH node sets, so the chunk arrays of both hold noised rows, logpn_table is
 * log p(n_lig, n_pocket) and the degrees of freedom are 3 (n_lig + n_pocket - 1).  cfg->remove_com is not read.
 * _joint_rows(which): number of rows of per_state (0), per_ligand (1), out (2).
 * _joint_pre: noise_lig [cap_lig][3 + atom_nf], noise_pocket [cap_pocket][3 + residue_nf] = standard normal draws in chunk
 *   layout; their coordinate part is centred here over the state's ligand + pocket rows.  center != 0: the complex's mean of
 *   the normalised coordinates over ligand + pocket rows is subtracted first (the model's training data is centred that way;
 *   the reference's forward leaves it to the data set).  Writes eps_* (the centred noise), z_* = alpha_t xh + sigma_t eps,
 *   both masks (int64, state ids local to the chunk, sorted), t_out [chunk_states] = t / timesteps, per_state
 *   [_joint_rows(0)][B * n_slots]: rows t, gamma_t, alpha_t, sigma_t, SNR_weight (and, by _joint_post, error_t_lig,
 *   error_t_pocket, loss_0_x_ligand, loss_0_x_pocket, loss_0_h) in column g, and -- on the state that is a complex's slot 0 --
 *   per_ligand [_joint_rows(1)][B]: kl_prior, neg_log_constants, delta_log_px, log_pN.
 * _joint_post: net_* = the network's output for (z_lig, z_pocket, t_out).  Time slots: error_t_* = sum over the node set's
 *   rows and all its columns of (eps - net)^2; zero slots: loss_0_x_* = 0.5 sum over the coordinates, loss_0_h = - sum over
 *   both node sets of log p(h | z_0).
 * _joint_reduce: once per call after every chunk.  out [_joint_rows(2)][B]: nll, loss_t, loss_t_lig, loss_0_x_ligand,
 *   loss_0_x_pocket, loss_0_h, neg_log_constants, kl_prior, delta_log_px, log_pN with
 *     loss_t     = sum_k ((-0.5 w[b][k]) SNR_weight) (error_t_lig + error_t_pocket)   (k ascending, float32)
 *     loss_t_lig = the same sum over error_t_lig alone
 *     nll = (((loss_t + (((loss_0_x_ligand + loss_0_x_pocket) + loss_0_h) + neg_log_constants)) + kl_prior) - delta_log_px)
 *           - log_pN.
 * Every sum is taken in a fixed order; no atomics. */
int dsbdd_score_joint_rows(int32_t which);
int dsbdd_score_joint_pre(void* stream, const dsbdd_loss_cfg* cfg, int32_t n_slots, int64_t first_state, int64_t chunk_states,
                          int64_t cap_lig, int64_t cap_pocket, int32_t center, const float* lig_x, const float* lig_h,
                          const int64_t* lig_mask, const float* pocket_x, const float* pocket_h, const int64_t* pocket_mask,
                          const float* noise_lig, const float* noise_pocket, const float* t_int, const float* gamma_table,
                          const float* logpn_table, float* eps_lig, float* eps_pocket, float* z_lig, float* z_pocket,
                          int64_t* mask_lig_out, int64_t* mask_pocket_out, float* t_out, float* per_state, float* per_ligand);
int dsbdd_score_joint_post(void* stream, const dsbdd_loss_cfg* cfg, int32_t n_slots, int64_t first_state, int64_t chunk_states,
                           int64_t cap_lig, int64_t cap_pocket, const float* lig_h, const int64_t* lig_mask, const float* pocket_h,
                           const int64_t* pocket_mask, const float* net_lig, const float* net_pocket, const float* eps_lig,
                           const float* eps_pocket, const float* z_lig, const float* z_pocket, float* per_state);
int dsbdd_score_joint_reduce(void* stream, int64_t batch, int32_t n_slots, const float* weights, const float* per_state,
                             const float* per_ligand, float* out);

/* ---- the optimiser step of the native training loop (csrc/optim.h) --------------------------------------------------------
 * One step = configure_gradient_clipping (lightning_modules.py:874-899) + torch.optim.AdamW(amsgrad=True).step() of the
 * reference in two launches and without a device-to-host copy: per-chunk sums of g^2 in a fixed order; then every
 * workgroup derives the same global norm, threshold 1.5 mean + 2 std (population) of the last 50 norms and
 * clip_coef = min(1, max_norm / (norm + 1e-6)), and updates p, exp_avg, exp_avg_sq, max_exp_avg_sq with the gradient scaled
 * as it is read (the caller's gradient tensors are NOT scaled).  The queue lives on the device, double-buffered by step
 * parity, and starts with the single entry 3000.
 *   _create: host only; numel [n_tensors].  The optimiser state is three flat float buffers of _state_elems() elements in
 *     which tensor i starts at _state_offset(i) (a multiple of 4); the caller owns them (zero-initialised) and a workspace
 *     of _workspace_bytes(); _bind uploads the tables and resets the queue; _set_params uploads the parameter pointers
 *     (again whenever one changes).  _bind, _set_params, _state_read and _state_write synchronise the stream; _step does not.
 *   _step: grads [n_tensors] device pointers, NULL = no gradient at this step: that tensor is skipped entirely (no decay,
 *     no state update); steps [n_tensors] = the tensor's own step count INCLUDING this step (>= 1; ignored where grads is NULL).
 *   _state_read: out [64] doubles: [0] entries in the queue, [1 .. 50] the entries newest first, [51] clipped steps,
 *     [52] last norm, [53] last threshold, [54] steps, [55] last clip coefficient.  _state_write sets the queue (newest
 *     first) and the two counters.
 *   _step_ranks: the step of data-parallel ranks.  gathered: the flat gradient buckets of the n_ranks contributing ranks
 *     (each in the layout of _state_offset, rank r at gathered + r * rank_stride floats).  Launch 1 folds them per element in
 *     rank order, ((g0 + g1) + g2) + ..., float32 adds with one rounding each, stores the sum to out_flat (_state_elems()
 *     floats; may be one of the inputs) and forms the per-chunk sums of squares with the bits the norm launch of _step
 *     leaves on that sum; launch 2 is the update launch of _step on out_flat.  Without clipping launch 1 still reduces.
 *     grads [n_tensors]: NULL = no gradient (the tensor's region is neither read nor written in any bucket and may hold
 *     NaN), else exactly out_flat + _state_offset(i).  steps, lr: as for _step.  No atomics: bitwise reproducible. */
typedef struct {
  double lr, beta1, beta2, eps, weight_decay;
  int32_t clip_grad;      /* 0: plain AdamW, one launch */
} dsbdd_optim_cfg;
typedef struct dsbdd_optim dsbdd_optim;
int dsbdd_optim_create(const dsbdd_optim_cfg* cfg, int32_t n_tensors, const int64_t* numel, dsbdd_optim** out);
void dsbdd_optim_destroy(dsbdd_optim* o);
int64_t dsbdd_optim_state_elems(const dsbdd_optim* o);
int64_t dsbdd_optim_state_offset(const dsbdd_optim* o, int32_t tensor);
size_t dsbdd_optim_workspace_bytes(const dsbdd_optim* o);
int dsbdd_optim_bind(dsbdd_optim* o, void* stream, float* m, float* v, float* vmax, void* ws, size_t ws_bytes);
int dsbdd_optim_set_params(dsbdd_optim* o, void* stream, float* const* params);
int dsbdd_optim_step(dsbdd_optim* o, void* stream, const float* const* grads, const int32_t* steps, double lr);
int dsbdd_optim_step_ranks(dsbdd_optim* o, void* stream, const float* gathered, int64_t rank_stride, int32_t n_ranks,
                           float* out_flat, const float* const* grads, const int32_t* steps, double lr);
int dsbdd_optim_state_read(dsbdd_optim* o, void* stream, double* out, int32_t capacity);
int dsbdd_optim_state_write(dsbdd_optim* o, void* stream, const double* items, int32_t n_items, double clips, double steps);

/* ---- the auxiliary Lennard-Jones term of the training loss (csrc/lj_loss.h; lightning_modules.py:304-331) ----------------
 * xh [n][ld]: coordinates in columns 0-2, n_types feature columns from column 3 (type = argmax); mask [n] int64 sorted
 * ascending in [0, batch); sigma [n_types][n_types] doubles = 2^(-1/6) rm / 100 / norm_values[0].  One launch, one workgroup per
 * sample: u [batch] = sum over ordered pairs of min(4 ((sigma/r)^12 - (sigma/r)^6), clamp), dx [n][3] = d u[sample] / d x
 * (a clamped pair contributes none).  type_scratch [n] int32.  Rows whose mask is outside [0, batch) are not written. */
int dsbdd_lj_potential(void* stream, const float* xh, int32_t ld, int32_t n_types, const int64_t* mask, int64_t n, int64_t batch,
                       const double* sigma, double clamp, int32_t has_clamp, int32_t* type_scratch, float* u, float* dx);

/* ---- post-processing of a finished batch ------------------*/
/* Distance-based bond orders of a batch of molecules: replaces
 * get_bond_order_batch + the (X, A, E) step of make_mol_edm
 * (analysis/molecule_builder.py:30-55, :101-118).  x [N][3] in Angstrom,
 * atom_type [N] indices into the [n_types][n_types] single/double/triple
 * length tables (pm), mol_off [batch+1] first atom of each molecule.
 * order [batch][n_max][n_max] int8 receives the strictly lower triangle
 * (order[b][i][j], i > j: 0 none, 1 single, 2 double, 3 triple); everything
 * else is set to 0.  Molecules longer than n_max are truncated to n_max atoms. */
int dsbdd_bond_orders(void* stream, const float* x, const int32_t* atom_type,
                      const int32_t* mol_off, int64_t batch, int32_t n_types,
                      const float* bonds1, const float* bonds2, const float* bonds3,
                      float margin1, float margin2, float margin3, int32_t n_max,
                      int8_t* order);

/* Graph statistics of every molecule of such a batch (csrc/mol_metrics.h; the per-molecule part of the reference's
 * analysis/metrics.py:52-125): one wave per molecule, integers only, no atomics -- every output is a function of the
 * molecule alone.  order = what dsbdd_bond_orders wrote with the same n_max; n_max in [1, DSBDD_MOL_MAX_ATOMS], anything
 * larger is refused (a molecule longer than n_max is read as its first n_max atoms, as by dsbdd_bond_orders).
 * max_valence [n_types]: highest sum of bond orders per type, -1 = not checked.  orders_in_key = 0 treats every bond as a
 * single one in the keys (skeleton key).  Outputs: valence [N], label [N] (smallest atom index, within the molecule, of the
 * atom's fragment), stats [batch][DSBDD_MOL_STATS] = n_atoms, n_bonds, atoms over their valence, fragments, size and label
 * of the largest fragment (ties: smallest atom index; -1 for an empty molecule), 0, 0; keys [batch][2] = colour-refinement
 * keys of the largest fragment and of the whole sample (invariant under atom renumbering; equal keys mean
 * refinement-equivalent, not proven isomorphic); fingerprint [batch][64] = 2048 bits of the largest fragment (radius-2
 * environments); type_counts [batch][n_types].  batch = 0 launches nothing. */
#define DSBDD_MOL_MAX_ATOMS 128
#define DSBDD_MOL_STATS 8
int dsbdd_mol_graph_stats(void* stream, const int8_t* order, const int32_t* atom_type, const int32_t* mol_off,
                          int64_t batch, int32_t n_types, const int32_t* max_valence, int32_t n_max,
                          int32_t orders_in_key, int32_t* valence, int32_t* label, int32_t* stats, uint64_t* keys,
                          uint32_t* fingerprint, int32_t* type_counts);

/* Tanimoto distances inside groups of such fingerprints (the reference's calculate_diversity): fingerprint [M][64] (16-byte
 * aligned), group_off [n_groups+1] ascending row offsets.  sum [g] = sum over pairs i < j of the group of
 * 1 - |a & b| / |a | b| (0 for an empty union), float64 in a fixed order; pairs [g] = the number of pairs.  One workgroup
 * per group. */
int dsbdd_fp_diversity(void* stream, const uint32_t* fingerprint, const int32_t* group_off, int64_t n_groups, double* sum,
                       int64_t* pairs);

/* Pose checks of a batch of ligands against the heavy atoms of their pockets (csrc/pose_check.h), one launch, one
 * workgroup per molecule.  lig_x [N][3] (Angstrom) and lig_r [N] (van-der-Waals radii) hold the molecules one after the
 * other, mol_off [batch+1] their first rows (N = mol_off[batch]; empty molecules allowed), mol_group [batch] the pocket
 * group of every molecule in any order; poc_x [M][3], poc_r [M] the pocket atoms, group_off [n_groups+1] the first row of
 * every group (M = group_off[n_groups]; a pocket shared by many molecules is stored once, a group may be unused).
 * float32, every operation rounded on its own:  d = sqrt((dx dx + dy dy) + dz dz);  clash iff d < (r_i + r_j) - tol;
 * contact iff d < contact; both strict, false for NaN.
 * atom_out [N][4]: clashing pocket atoms, pocket atoms in contact, index within the group of the nearest pocket atom (ties:
 * the smallest index; -1 without one), bit pattern of its d (+inf without one).
 * mol_out [batch][8]: n_atoms, clash pairs, atoms with a clash, contact pairs, atoms with a contact, nonfinite (1 when a
 * coordinate of the molecule is NaN or +-inf), bit pattern of the smallest d, 0.
 * No atomics; the result does not depend on the order of anything.  Offsets and group ids are range-checked on the device:
 * a molecule whose rows or group fail the check is read as empty / as having an empty group.  batch = 0 launches nothing;
 * null pointers, negative counts and a non-finite or negative tol / contact are DSBDD_ERR_ARG. */
int dsbdd_pose_check(void* stream, const float* lig_x, const float* lig_r, const int32_t* mol_off, int64_t batch,
                     const int32_t* mol_group, const float* poc_x, const float* poc_r, const int32_t* group_off,
                     int64_t n_groups, float tol, float contact, int32_t* atom_out, int32_t* mol_out);

/* Vina-type interaction score of such a batch (csrc/vina_score.h; functional form and weights of Trott & Olson, J. Comput.
 * Chem. 31 (2010) 455, heavy atoms only -- NOT the output of smina or Vina: no hydrogens, no charges, no intramolecular
 * term).  Two launches: the typing of the ligand atoms from their bond orders, then the pair sum.
 *
 * Atom code, one int32 per atom: bits 0-3 the class (0 untyped, 1 C, 2 N, 3 O, 4 P, 5 S, 6 F, 7 Cl, 8 Br, 9 I, 10 metal;
 * 11-15 are read as untyped), bit 4 hydrophobic, bit 5 hydrogen-bond donor, bit 6 acceptor.  Untyped atoms take part in
 * no pair term; as neighbours in the typing rules they count as heteroatoms.
 *
 * dsbdd_vina_type: one wave per molecule, integers only.  order / atom_type / mol_off / n_max as for
 * dsbdd_mol_graph_stats (orders outside 1..3 are no bond; a molecule longer than n_max is read as its first n_max atoms,
 * the codes of the atoms after them are written 0); class_elem [n_types] the class of every atom type (a type id outside
 * [0, n_types) or a class outside the list is untyped).  With s = the sum of bond orders at the atom and a heteroatom
 * neighbour = any neighbour that is not carbon:  C hydrophobic iff it has no heteroatom neighbour;  F, Cl, Br, I
 * hydrophobic;  N donor iff s < 3, acceptor iff s = 3 and one of its bonds has order >= 2;  O acceptor, donor iff s < 2;
 * S, P no flags;  metal donor.  lig_code [N]; mol_int [batch][4] = typed atoms, untyped atoms, N_rot, 0, where N_rot = the
 * bonds of order 1 that are in no ring (their ends are not connected when the bond is removed) and whose two ends both have
 * heavy degree >= 2 (amide and conjugated bonds are not excluded).
 *
 * dsbdd_vina_score: one workgroup per molecule; lig_x / mol_off / mol_group / poc_x / group_off and every group
 * convention exactly as for dsbdd_pose_check, lig_code [N] and poc_code [M] atom codes, mol_int what dsbdd_vina_type wrote
 * (N_rot is read; a negative one as 0).  A pair of typed atoms counts iff its float32 distance r = sqrt((dx dx + dy dy) +
 * dz dz), every operation rounded on its own, is < 8.0, strictly.  With d = r - R_i - R_j (R by class: C 1.9, N 1.8, O 1.7,
 * P 2.1, S 2.0, F 1.5, Cl 1.8, Br 2.0, I 2.2, metal 1.2):
 *   gauss1 = exp(-(d / 0.5)^2);  gauss2 = exp(-((d - 3) / 2)^2);  repulsion = d^2 if d < 0, else 0;
 *   hydrophobic (both atoms hydrophobic) = 1 if d <= 0.5, 1.5 - d if 0.5 < d < 1.5, else 0;
 *   hbond (one atom donor and the other acceptor, once per pair) = 1 if d <= -0.7, -d / 0.7 if -0.7 < d < 0, else 0,
 * all evaluated and summed in float64 from the float32 r, stored as float32.
 * atom_out [N][5]: the unweighted sums of the five terms over the atom's pairs.  mol_out [batch][8]: the five sums T_k over
 * the molecule, inter = -0.035579 T_1 - 0.005156 T_2 + 0.840245 T_3 - 0.035069 T_4 - 0.587439 T_5,
 * score = inter / (1 + 0.05846 N_rot) in kcal/mol, 0.  mol_flag [batch]: 1 when a coordinate of the molecule is NaN or
 * +-inf; every float output of such a molecule, per atom and per molecule, is NaN.  An empty molecule or group gives zeros.
 * No atomics; the order of every sum is a function of the molecule and its group alone, so the outputs are bitwise
 * reproducible and do not depend on the rest of the batch.  Offsets, group ids, type ids and codes are range-checked on
 * the device (a molecule whose rows fail the check is read as empty and its rows are not written).  batch = 0 launches
 * nothing; null pointers, negative counts and an n_max outside [1, DSBDD_MOL_MAX_ATOMS] are DSBDD_ERR_ARG. */
int dsbdd_vina_type(void* stream, const int8_t* order, const int32_t* atom_type, const int32_t* mol_off, int64_t batch,
                    int32_t n_types, const int32_t* class_elem, int32_t n_max, int32_t* lig_code, int32_t* mol_int);
int dsbdd_vina_score(void* stream, const float* lig_x, const int32_t* lig_code, const int32_t* mol_off, int64_t batch,
                     const int32_t* mol_group, const int32_t* mol_int, const float* poc_x, const int32_t* poc_code,
                     const int32_t* group_off, int64_t n_groups, float* atom_out, float* mol_out, int32_t* mol_flag);

/* dsbdd_vina_score and the analytic gradient of `inter` with respect to the ligand coordinates from one sweep
 * (csrc/vina_grad.h), one launch, one workgroup per molecule.  Every input, convention and check of dsbdd_vina_score;
 * atom_out, mol_out and mol_flag are bit for bit what dsbdd_vina_score writes for the same inputs.
 * Per counted pair (i ligand atom, j pocket atom; counted as above: both typed, float32 r < 8): e = (dx, dy, dz) the three
 * float32 differences x_i - x_j the distance is formed from, r their float32 root, and from here on float64:
 * d = r - R_i - R_j, u = e / r (the float32 values converted, then divided), and the derivatives of the terms in d,
 *   gauss1' = -8 d exp(-4 d^2);  gauss2' = -c exp(-c^2) with c = (d - 3) / 2;  repulsion' = 2 d if d < 0, else 0;
 *   hydrophobic' (both atoms hydrophobic) = -1 if 0.5 < d < 1.5, else 0;
 *   hbond' (donor / acceptor pair) = -1 / 0.7 if -0.7 < d < 0, else 0,
 * one-sided at the kinks exactly as the terms are: at d = 0.5, 1.5, -0.7 and 0 the derivative is the 0 (or, for the
 * repulsion at d = 0, the 2 d = 0) of the branch the term itself takes there.  A pair with r == 0 (the atoms coincide) adds
 * to the five terms as in dsbdd_vina_score and adds ZERO to the gradient: its direction is undefined.  The cutoff at 8 A is
 * a jump of the score itself, as in Vina; the gradient ignores it (it is the gradient of the sum over the pairs counted at
 * x).  Typing is constant: codes and N_rot do not depend on x here.
 * atom_grad [N][3]: g_i = sum_j (sum_k w_k T_k'(d_ij)) u_ij = d inter / d x_i in kcal/mol/A, w the weights of `inter`;
 * 0 for an untyped atom and for the atoms of a molecule on an empty or invalid group.
 * mol_grad [batch][8]: [0:3] F = sum_i g_i;  [3:6] the moment about the centroid sum_i (x_i - c) x g_i, c the mean of all
 * n atoms of the molecule (sum x_i, sum g_i and sum x_i x g_i carried in float64, M - c x F formed once);  [6] max_i |g_i|
 * (the maximum of the float64 norms, then rounded);  [7] 1 / (1 + 0.05846 N_rot), the factor that turns d inter / d x into
 * d score / d x.  A molecule with a NaN or +-inf coordinate: NaN in every float of its rows of atom_grad and mol_grad, and
 * the flag.  Sums in float64 in the order of dsbdd_vina_score's, stored as float32; no atomics, bitwise reproducible,
 * independent of the rest of the batch; the same range checks.  batch = 0 launches nothing; null pointers and negative
 * counts are DSBDD_ERR_ARG. */
int dsbdd_vina_score_grad(void* stream, const float* lig_x, const int32_t* lig_code, const int32_t* mol_off, int64_t batch,
                          const int32_t* mol_group, const int32_t* mol_int, const float* poc_x, const int32_t* poc_code,
                          const int32_t* group_off, int64_t n_groups, float* atom_out, float* mol_out, int32_t* mol_flag,
                          float* atom_grad, float* mol_grad);

/* Rigid-body minimisation of every pose of such a batch under `inter` of dsbdd_vina_score, one launch (csrc/vina_minimize.h):
 * one workgroup per molecule runs the sweep of dsbdd_vina_score_grad once per evaluation and takes every decision on the
 * device.  Rigid ligand (no torsions), rigid protein, a local search by steepest descent in a scaled metric with
 * backtracking; no intramolecular term; NOT smina or qvina output.  Every input, convention and check of
 * dsbdd_vina_score_grad; lig_x is the input pose and is not written; lig_x and x_out MUST NOT alias (with batch > 0 the same
 * pointer is DSBDD_ERR_ARG; overlapping ranges are the caller's error).  Typing is done once, on the input pose, by dsbdd_vina_type.
 * Pose: c0 the mean of the molecule's n input coordinates, s_i = x0_i - c0 (float64), (T, q) a translation and a unit
 * quaternion (w first) from (0, identity); x_i = float32((c0 + T) + R(q) s_i), formed in float64 from the INPUT
 * coordinates at every evaluation and rounded once.  rho^2 = max(sum |s_i|^2 / n, 1), rho_max = max |s_i|.
 * An evaluation writes x(T, q) to x_out, sweeps, and reads back the stored float32 E = inter (mol_out[5]), F = net
 * gradient and M = its moment about the centroid (mol_grad[0..5]); every decision is a function of those and the pose:
 *   1. evaluate the input pose: E_start = E, L = step;
 *   2. u = |F| + rho_max |M| / rho^2; unless u > 0 stop with status 2;
 *   3. if L < tol stop with status 1; if max_evals evaluations were made stop with status 0; else alpha = L / u,
 *      T' = T - alpha F, q' = normalise(dq q) with dq the rotation by the vector -alpha M / rho^2 (about the centroid, in
 *      world axes; no atom moves more than L); evaluate; if E' < E (float32, strict) take the trial, L = min(2 L, step)
 *      and go to 2, else L = L / 2 and repeat 3;
 *   4. on a stop after a rejected trial the accepted pose is evaluated once more (counted in the evaluations; the only
 *      one beyond max_evals).
 * Outputs: atom_out, mol_out, mol_flag, atom_grad, mol_grad as dsbdd_vina_score_grad writes them for x_out, bit for bit;
 * x_out [N][3] the returned pose; mol_pose [B][8] = T (3), q (4), rho^2; mol_min [B][4] = E_start, E_final, the last accepted
 * L (0 if none), u at the returned pose; mol_stat [B][4] int32 = status (0 budget, 1 converged, 2 no gradient: no atoms, an
 * empty group, nothing typed, or a flat score; 3 not finite), evaluations, accepted steps, 0.  A molecule with a NaN or
 * +-inf coordinate: status 3, its x_out rows are the input's bit for bit, NaN in every other float it owns, mol_flag 1.
 * No atomics, bitwise reproducible, independent of the rest of the batch; the same range checks.  batch = 0 launches
 * nothing; null pointers, negative counts, step or tol not finite or <= 0 and max_evals outside [1, 4096] are
 * DSBDD_ERR_ARG. */
int dsbdd_vina_minimize(void* stream, const float* lig_x, const int32_t* lig_code, const int32_t* mol_off, int64_t batch,
                        const int32_t* mol_group, const int32_t* mol_int, const float* poc_x, const int32_t* poc_code,
                        const int32_t* group_off, int64_t n_groups, float* atom_out, float* mol_out, int32_t* mol_flag,
                        float* atom_grad, float* mol_grad, float step, float tol, int32_t max_evals, float* x_out,
                        float* mol_pose, float* mol_min, int32_t* mol_stat);

/* Torsion tree and intramolecular term of such a batch (csrc/vina_torsion.h, csrc/vina_intra.h): these two launches list
 * the rotatable bonds with their moving sides and evaluate the ligand-ligand term and its gradient at the pose given;
 * nothing is moved.  dsbdd_vina_flex (below) relaxes a pose over them.
 *
 * dsbdd_vina_torsions: one wave per molecule, integers only; order / atom_type / mol_off / n_types / class_elem / n_max
 * exactly as for dsbdd_vina_type.  A rotor is what N_rot counts: a bond (a, c), c < a, of order 1, both ends of heavy
 * degree >= 2, in no ring.  Rotors are enumerated in ascending (a, c); the first 32 are kept.
 * tor_int [batch][4] = rotors kept, rotors found (= mol_int[2] of dsbdd_vina_type on the same input), 0, 0; a molecule
 * longer than n_max keeps none (found is still counted on its first n_max atoms).
 * Moving side S_k of kept rotor k: of the two components its ends fall into when the bond is cut, the one with fewer atoms,
 * on a tie the one of the higher-index end.  tor_end [batch][32][2] = fixed end p_k, moving end m_k (m_k in S_k; atom
 * indices inside the molecule), -1 past the kept; tor_side [batch][32][4] = S_k as a 128-bit mask in four int32 words (atom
 * 32 w + b is bit b of word w), 0 past the kept.  Any two S_k are nested or disjoint: two sides of at most half a
 * component each cannot overlap without one containing the other.
 * pair_mask [N][4]: for atom i of its molecule the 128-bit mask of the atoms j of the same molecule with i != j, both typed
 * (class_elem of their type), more than 3 bonds apart or not connected, and exactly one of i, j in S_k for some kept k.
 * Symmetric; all zero for a molecule without kept rotors and for the atoms past n_max.  A molecule whose offsets fail the
 * range check is read as empty: zeros in tor_int, no row of pair_mask written.
 *
 * dsbdd_vina_intra: one workgroup per molecule, the sweep of dsbdd_vina_score_grad with the molecule's own atoms in place
 * of the pocket group, over the pairs set in pair_mask (what dsbdd_vina_torsions wrote; a bit at or above the molecule's
 * size is ignored).  The same float32 distance and strict cutoff r < 8, the same five terms, weights, radii and flags from
 * lig_code on both sides, the same one-sided derivatives; a pair with r == 0 adds to the terms and zero to the gradient.
 * atom_out [N][5]: the unweighted sums of the five terms over the atom's partners.  atom_grad [N][3]: g_i = sum_j (sum_k w_k
 * T_k'(d_ij)) u_ij = d intra / d x_i in kcal/mol/A.  mol_out [batch][8]: the five sums with every pair counted once (half
 * the sum over the atoms), intra = sum_k w_k T_k (no division by rotors), 0, 0.  mol_flag [batch]: 1 when a coordinate is
 * NaN or +-inf; every float the molecule owns in atom_out, mol_out and atom_grad is then NaN.  A molecule without kept rotors
 * gives exact zeros.  Sums in float64 in a fixed order, stored as float32; no atomics, bitwise reproducible, independent of
 * the rest of the batch; offsets range-checked as everywhere.  batch = 0 launches nothing; null pointers, negative counts
 * and an n_max outside [1, DSBDD_MOL_MAX_ATOMS] are DSBDD_ERR_ARG. */
int dsbdd_vina_torsions(void* stream, const int8_t* order, const int32_t* atom_type, const int32_t* mol_off, int64_t batch,
                        int32_t n_types, const int32_t* class_elem, int32_t n_max, int32_t* tor_int, int32_t* tor_end,
                        int32_t* tor_side, int32_t* pair_mask);
int dsbdd_vina_intra(void* stream, const float* lig_x, const int32_t* lig_code, const int32_t* mol_off, int64_t batch,
                     const int32_t* pair_mask, float* atom_out, float* mol_out, int32_t* mol_flag, float* atom_grad);

/* Flexible minimisation of every pose of such a batch under E = inter + intra, one launch (csrc/vina_flex.h) after
 * dsbdd_vina_type and dsbdd_vina_torsions: dsbdd_vina_minimize with the kept rotors as further degrees of freedom and the
 * term of dsbdd_vina_intra in the objective.  NOT smina or qvina output: steepest descent with backtracking and not BFGS, a
 * local search from one start, a rigid protein, heavy atoms only, typing and the torsion tree fixed on the input pose, amide
 * and conjugated bonds rotate, at most 32 rotors.  Every input, convention and check of dsbdd_vina_minimize; tor_int, tor_end,
 * tor_side and pair_mask what dsbdd_vina_torsions wrote.  They are range-checked on the device: the kept count is clamped
 * to [0, 32], a rotor whose ends are not two different atoms of the molecule is DROPPED (the molecule relaxes with the
 * others), side and pair bits at or above the molecule's size are ignored, a molecule longer than 128 atoms has no rotor.
 * dofs: bit 0 = the rigid body, bit 1 = the torsions (1, 2 or 3); a switched-off block is never stepped.
 * Coordinates, always from the input x0 in float64, rounded once: y = x0; for k in list order (a rotor with theta_k == 0 or
 * coinciding ends is skipped) the atoms of S_k turn by theta_k about the line from y[p_k] through y[m_k] as it stands
 * (Rodrigues); x_i = float32(t + R(q) y_i).  Start: theta = 0, t = 0, q = identity, so x = x0 bit for bit.  Because the S_k
 * are nested or disjoint the geometry does not depend on the list order in real arithmetic, and bond lengths, angles and
 * all distances inside a rigid piece are the input's up to one float32 rounding.
 * An evaluation writes x to x_out, runs the sweep of dsbdd_vina_score_grad and that of dsbdd_vina_intra on it, and reads
 * back E = (double)inter + (double)intra of the stored float32 values (compared with strict <), F and M (mol_grad[0..5]).
 * At every accepted pose, with c the mean of its float32 coordinates: rho^2 = max(mean |x_i - c|^2, 1), rho_max = max |x_i - c|;
 * per rotor a_k the unit vector from x[p_k] to x[m_k], tau_k = a_k . sum_{i in S_k} (x_i - x[m_k]) x (g_i^inter + g_i^intra)
 * (the stored float32 gradients, float64 sums), r_k = the largest distance of an atom of S_k from axis k,
 * rho_k^2 = max(mean over S_k of that distance squared, 1).  u = |F| + rho_max |M| / rho^2 + sum_k r_k |tau_k| / rho_k^2
 * (switched-off blocks left out), alpha = L / u, and the trial is q' = normalise(dq q), t' = c + R(dq)(t - c) - alpha F (dq
 * the rotation by -alpha M / rho^2: a rotation about c then a translation), theta_k' = theta_k - alpha tau_k / rho_k^2.  No atom
 * moves more than L in a trial.  Steps 1-4, tol, max_evals and the statuses are those of dsbdd_vina_minimize with this E, u.
 * Outputs, for the returned x_out: atom_out, mol_out, mol_flag, atom_grad, mol_grad bit for bit what dsbdd_vina_score_grad
 * writes on x_out; intra_atom, intra_mol, intra_flag, intra_grad bit for bit what dsbdd_vina_intra writes on x_out;
 * mol_pose [B][8] = t (3), q (4), rho^2 at the returned pose; mol_flex [B][8] = inter at the start, inter at the end, the last
 * accepted L (0 if none), u at the returned pose, intra at the start, intra at the end, E at the start, E at the end;
 * mol_stat as dsbdd_vina_minimize; theta, tau [B][32] in the slots of tor_end (0 where no valid kept rotor stands).  A
 * molecule with a NaN or +-inf coordinate: status 3, x_out the input's bits, NaN in every other float it owns, both flags 1.
 * No atomics, bitwise reproducible, independent of the rest of the batch.  batch = 0 launches nothing; the argument errors of
 * dsbdd_vina_minimize, and dofs outside [1, 3], are DSBDD_ERR_ARG. */
int dsbdd_vina_flex(void* stream, const float* lig_x, const int32_t* lig_code, const int32_t* mol_off, int64_t batch,
                    const int32_t* mol_group, const int32_t* mol_int, const float* poc_x, const int32_t* poc_code,
                    const int32_t* group_off, int64_t n_groups, const int32_t* tor_int, const int32_t* tor_end,
                    const int32_t* tor_side, const int32_t* pair_mask, int32_t dofs, float step, float tol, int32_t max_evals,
                    float* atom_out, float* mol_out, int32_t* mol_flag, float* atom_grad, float* mol_grad, float* intra_atom,
                    float* intra_mol, int32_t* intra_flag, float* intra_grad, float* x_out, float* mol_pose, float* mol_flex,
                    int32_t* mol_stat, float* theta, float* tau);

/* ---- ligands as input: the packed batch of the design front ends -------------*/
/* One launch that writes the ligand batch of substructure inpainting and of
 * diversification (inpaint.py:114-141, optimize.py:39-62 of the reference build
 * it on the host).  Templates: tmpl_x [tmpl_rows][3], tmpl_type [tmpl_rows]
 * class ids, tmpl_ptr [n_tmpl+1] first row of every template -- device memory,
 * e.g. the output of an earlier chain.  Slots: slot_tmpl [batch] template id,
 * slot_size [batch] rows of the slot (>= rows of its template, >= 1), slot_off
 * [batch+1] first output row (exclusive scan of slot_size; n_rows = the total) --
 * device memory as well, known to the host, which uploads them as one buffer.
 * Outputs: x [n_rows][3] and one_hot [n_rows][atom_nf] hold the template in the
 * first rows of every slot and zeros after, lig_fixed [n_rows] is 1 on the
 * template rows, mask [n_rows] the slot id, size [batch] = slot_size (int64).
 * Launch geometry depends on n_rows only; no host synchronisation.  Indices read
 * from device memory are range-checked: a row without a valid source is empty. */
int dsbdd_pack_ligands(void* stream, const float* tmpl_x, const int32_t* tmpl_type,
                       const int32_t* tmpl_ptr, int32_t n_tmpl, int64_t tmpl_rows,
                       const int32_t* slot_tmpl, const int32_t* slot_size,
                       const int32_t* slot_off, int64_t batch, int64_t n_rows,
                       int32_t atom_nf, float* x, float* one_hot, int64_t* lig_fixed,
                       int64_t* mask, int64_t* size);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSBDD_HIP_H */
