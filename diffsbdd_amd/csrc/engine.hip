// libdiffsbdd_hip.so -- C-ABI implementation (see include/diffsbdd_hip.h): the one translation unit of the library.
// Host-side orchestration of one EGNNDynamics.forward call
// (the reference's equivariant_diffusion/dynamics.py:87-167) as a fixed sequence
// of asynchronous launches on the caller's stream: no allocation, no host sync.
// This file holds the engine's entry points; the host code behind them lives in the units included below:
//   engine_state.h  error plumbing, struct dsbdd_engine, workspace layout, derived weight copies, environment switches
//   launch.h        H dispatch and persistent grid of the edge kernels, node GEMM helpers, radius-graph builder
//   forward.h       the per-call plan (pocket frame, level pruning, "forward cone") and the stages of one forward
//   graph_cache.h   ghost-row upkeep and the hipGraph capture / replay around the forward
//   capi_kernels.h  C-ABI wrappers of the stand-alone kernels
//   train_blocks.h  the training step's building blocks: weight gradients, scratch, side streams, one edge stage each way
//   train_net.h     the training step of the whole network: parameter index, pack buffer, workspace, the two walks
//   train_api.h     every dsbdd_train_* / dsbdd_loss_* / dsbdd_score_* / dsbdd_optim_* entry point
// (device code: the kernel headers included first; train_kernels.h holds the network walk's own kernels)
#include "../../include/diffsbdd_hip.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.h"
#include "ddpm.h"
#include "edge_mlp.h"
#include "edge_wave.h"
#include "edge_wave16.h"
#include "edge_splitk.h"
#include "graph_parts.h"
#include "radius_graph.h"
#include "level_list.h"
#include "geometry.h"
#include "lig_head.h"
#include "ligand_pack.h"
#include "molecule.h"
#include "mol_metrics.h"
#include "pose_check.h"
#include "vina_score.h"
#include "vina_grad.h"
#include "vina_minimize.h"
#include "vina_torsion.h"
#include "vina_intra.h"
#include "vina_flex.h"
#include "node_chain.h"
#include "node_linear.h"
#include "train.h"
#include "train_kernels.h"

using namespace dsbdd;

#include "engine_state.h"
#include "launch.h"
#include "forward.h"
#include "graph_cache.h"
#include "capi_kernels.h"
// the training step: building blocks, one launch sequence per direction, loss terms, optimiser and auxiliary loss
#include "train_blocks.h"
#include "train_net.h"
#include "loss_head.h"
#include "score.h"
#include "score_joint.h"
#include "optim.h"
#include "lj_loss.h"
#include "train_api.h"

extern "C" {

int dsbdd_abi_version(void) { return DSBDD_ABI_VERSION; }
const char* dsbdd_last_error(void) { return g_err.c_str(); }

int dsbdd_engine_create(const dsbdd_config* cfg, dsbdd_engine** out) {
  if (!cfg || !out) return fail(DSBDD_ERR_ARG, "null argument");
  if (!hidden_nf_ok(cfg->hidden_nf)) return fail(DSBDD_ERR_ARG, "hidden_nf must be one of 64, 128, 192, 256");
  if (cfg->n_layers < 1 || cfg->inv_sublayers < 1 || cfg->atom_nf < 1 || cfg->residue_nf < 1 ||
      cfg->joint_nf < 1 || cfg->edge_embedding_dim < 0)
    return fail(DSBDD_ERR_ARG, "bad layer/feature counts");
  if (!(cfg->normalization_factor > 0.f)) return fail(DSBDD_ERR_ARG, "normalization_factor must be > 0");
  dsbdd_engine* e = new dsbdd_engine();
  e->cfg = *cfg;
  e->slots.assign(n_slots(*cfg), nullptr);
  e->n_cu = device_cus();
  read_env_switches(e);
  *out = e;
  return DSBDD_OK;
}

void dsbdd_engine_destroy(dsbdd_engine* e) { delete e; }

int dsbdd_engine_weight_slots(const dsbdd_engine* e) { return e ? n_slots(e->cfg) : DSBDD_ERR_ARG; }

int dsbdd_engine_set_weights(dsbdd_engine* e, const float* const* slots_host, int n) {
  if (!e || !slots_host) return fail(DSBDD_ERR_ARG, "null argument");
  if (n != n_slots(e->cfg)) return fail(DSBDD_ERR_ARG, "wrong number of weight slots");
  const dsbdd_config& c = e->cfg;
  for (int i = 0; i < n; ++i) {
    const float* ptr = slots_host[i];
    bool optional = false;
    // slots that may legitimately be absent
    const int per = c.inv_sublayers * DSBDD_GCL_COUNT + DSBDD_EQ_COUNT;
    if (i >= DSBDD_G_COUNT) {
      const int r = (i - DSBDD_G_COUNT) % per;
      if (r < c.inv_sublayers * DSBDD_GCL_COUNT) {
        const int wch = r % DSBDD_GCL_COUNT;
        if (!c.attention && (wch == DSBDD_GCL_ATT_W || wch == DSBDD_GCL_ATT_B)) optional = true;
      } else {
        const int wch = r - c.inv_sublayers * DSBDD_GCL_COUNT;
        if (c.reflection_equivariant && wch >= DSBDD_EQ_X_WD && wch <= DSBDD_EQ_X_B2) optional = true;
      }
    }
    if (!ptr && !optional) return fail(DSBDD_ERR_ARG, "null weight slot " + std::to_string(i));
    if (ptr && (reinterpret_cast<uintptr_t>(ptr) & 15))
      return fail(DSBDD_ERR_ARG, "weight slot " + std::to_string(i) + " not 16-byte aligned");
    e->slots[i] = ptr;
  }
  e->drop_graphs();
  e->invalidate_derived();
  e->h0_pocket_valid = false;
  e->has_weights = true;
  return DSBDD_OK;
}

size_t dsbdd_engine_workspace_bytes(const dsbdd_engine* e, int64_t nl, int64_t np, int64_t B,
                                    int64_t E) {
  if (!e || nl < 0 || np < 0 || B < 1 || E < 0) return 0;
  return ws_carve(e->cfg, nl, np, B, E, nullptr).total;
}

int dsbdd_engine_bind_workspace(dsbdd_engine* e, void* ws, size_t bytes, int64_t nl, int64_t np,
                                int64_t B, int64_t E) {
  if (!e || !ws) return fail(DSBDD_ERR_ARG, "null argument");
  if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(DSBDD_ERR_ARG, "workspace must be 256-byte aligned");
  if ((nl + np) >= (1ll << 30) || E >= (1ll << 31) - 256) return fail(DSBDD_ERR_ARG, "problem too large for int32 indices");
  if (bytes < ws_carve(e->cfg, nl, np, B, E, nullptr).total) return fail(DSBDD_ERR_CAPACITY, "workspace too small");
  e->drop_graphs();
  static_cast<Workspace&>(*e) = ws_carve(e->cfg, nl, np, B, E, static_cast<char*>(ws));
  e->ws = static_cast<char*>(ws); e->ws_bytes = bytes;
  e->cap_lig = nl; e->cap_poc = np; e->cap_batch = B; e->cap_edges = E;
  e->cap_edgesL = 2 * E + 32 * kLevels * B;
  e->cap_tiles = e->cap_edgesL / 32 + 2;
  e->cap_shell = E + 32 * B;
  e->cap_tiles16 = e->cap_edgesL / 16 + 2;   // head slots of the 16-edge-granule kernels (edge_wave16.h); <= 2 * cap_tiles
  e->lvl_stats_zeroed = false;          // cleared by the first (eager) call that uses it
  e->frame = false;               // a pocket frame lives in the workspace
  e->ghost_dirty = true;
  e->h0_pocket_valid = false;
  e->invalidate_derived();
  return DSBDD_OK;
}

#ifdef DSBDD_TIMESTAMPS
// debug builds only (not part of the ABI header): device buffer of [capacity][64][16] uint64 marks
int dsbdd_debug_set_timestamps(dsbdd_engine* e, unsigned long long* buf, int capacity) {
  if (!e) return DSBDD_ERR_ARG;
  e->ts_buf = buf; e->ts_cap = capacity; e->ts_next = 0;
  return DSBDD_OK;
}
#endif

int dsbdd_engine_set_pocket_frame(dsbdd_engine* e, void* stream, const float* x_frame, const int64_t* mask_frame,
                                  const int32_t* frame_rows, const int32_t* twin_local, int64_t n_lig,
                                  int64_t n_pocket, int64_t batch, int64_t n_frame, int64_t batch_frame,
                                  int64_t edge_bound_frame) {
  StreamDevice stream_device_(stream);
  if (!e || !x_frame || !mask_frame || !frame_rows || !twin_local) return fail(DSBDD_ERR_ARG, "null argument");
  if (!e->ws) return fail(DSBDD_ERR_STATE, "workspace not bound");
  if (e->cfg.update_pocket_coords) return fail(DSBDD_ERR_STATE, "a pocket frame needs rigid pocket coordinates");
  if (n_lig < 0 || n_lig > e->cap_lig || n_pocket < 1 || n_pocket > e->cap_poc || batch < 1 || batch > e->cap_batch ||
      n_frame < 1 || n_frame > n_pocket || batch_frame < 1 || batch_frame > batch || edge_bound_frame < 1 ||
      edge_bound_frame > e->cap_edges)
    return fail(DSBDD_ERR_CAPACITY, "pocket frame exceeds the bound workspace");
  hipStream_t s = static_cast<hipStream_t>(stream);
  e->drop_graphs();
  e->frame = false;
  e->h0_pocket_valid = false;
  const int n3 = (int)n_frame, b3 = (int)batch_frame, N = (int)(n_lig + n_pocket);
  HIP_TRY(hipMemcpyAsync(e->xframe, x_frame, (size_t)n3 * 12, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(e->frame_rows, frame_rows, (size_t)n3 * 4, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(e->twin, twin_local, (size_t)n_pocket * 4, hipMemcpyDeviceToDevice, s));
  // the pocket-pocket radius graph of the frame: a pocket-only problem (no ligand nodes) whose nodes are the
  // ghost rows N .. N + n3 of the engine's node arrays
  const int work = n3 > b3 + 1 ? n3 : b3 + 1;
  hipLaunchKernelGGL(prep_kernel, dim3((work + 255) / 256), dim3(256), 0, s, (const int64_t*)nullptr, 0, mask_frame,
                     n3, b3, e->node_batch3, e->lig_off3, e->poc_off3, (int*)nullptr);
  HIP_TRY(hipGetLastError());
  int rc = build_edges_impl(s, x_frame, 0, n3, b3, e->cfg, e->node_batch3, e->lig_off3, e->poc_off3, e->deg3,
                            e->row_ptr3, e->erow3, e->ecol3, e->ed03, e->cap_edges, e->tile_ctr + 24, nullptr,
                            e->scan_tmp3, e->seg_base3, nullptr, N);
  if (rc) return rc;
  e->frame_nlig = n_lig; e->frame_npoc = n_pocket; e->frame_batch = batch;
  e->frame_n3 = n3; e->frame_cap3 = edge_bound_frame;
  rc = ghost_setup(e, s);
  if (rc) return rc;
  int slots = 0;                         // one host sync per chain (the chain start has one already)
  HIP_TRY(hipMemcpyAsync(&slots, e->row_ptr3 + n3, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (slots < 0 || slots > e->cap_edges || (slots & (kEdgeAlign - 1)))
    return fail(DSBDD_ERR_CAPACITY, "pocket frame: pocket-pocket list exceeds the edge capacity");
  e->ghost_slots = slots;
  e->frame = true;
  return DSBDD_OK;
}

int dsbdd_engine_clear_pocket_frame(dsbdd_engine* e) {
  if (!e) return fail(DSBDD_ERR_ARG, "null argument");
  if (e->frame) e->drop_graphs();
  e->frame = false;
  e->h0_pocket_valid = false;
  return DSBDD_OK;
}

int dsbdd_engine_last_plan(const dsbdd_engine* e, int32_t* radius, int32_t* ghost, int32_t capacity,
                           int32_t* n_stages, int32_t* timed_level) {
  if (!e || !radius || !ghost || !n_stages || !timed_level) return fail(DSBDD_ERR_ARG, "null argument");
  const int n = (int)e->plan_radius.size();
  if (capacity < n) return fail(DSBDD_ERR_CAPACITY, "plan arrays too short");
  for (int i = 0; i < n; ++i) { radius[i] = e->plan_radius[i]; ghost[i] = e->plan_ghost[i]; }
  *n_stages = n; *timed_level = e->plan_timed_level;
  return DSBDD_OK;
}

int dsbdd_engine_set_option(dsbdd_engine* e, int which, int value) {
  if (!e) return fail(DSBDD_ERR_ARG, "null argument");
  switch (which) {
    case DSBDD_OPT_PRUNE: e->prune = value ? 1 : 0; break;
    case DSBDD_OPT_CONE: e->cone = value <= 0 ? 0 : (value >= 2 ? 2 : 1); break;   // 0 off, 1 by the cost model, 2 always
    case DSBDD_OPT_GRANULE16: e->granule16 = (unsigned)value; break;               // bit g: message stage g, bit 16 + b: coordinate stage b
    case DSBDD_OPT_SPLITK: e->splitk = (unsigned)value; break;                     // the same layout: stages on the split-K kernels
    case DSBDD_OPT_EMU:                                                            // 0 exact fp32; 6 / 9: emulated on the bf16 matrix cores
      if (value != 0 && value != 6 && value != 9) return fail(DSBDD_ERR_ARG, "DSBDD_OPT_EMU takes 0, 6 or 9");
      e->emu = value; break;
    case DSBDD_OPT_SHELL: e->shell = value ? 1 : 0; break;
    case DSBDD_OPT_TAIL:                                                           // 0 off, 1 on, n > 1: n resident workgroups in the rule
      if (value < 0) return fail(DSBDD_ERR_ARG, "DSBDD_OPT_TAIL takes a value >= 0");
      e->tail = value; break;
    case DSBDD_OPT_CHAIN_DEAL: e->chain_deal = value ? 1 : 0; break;
    default: return fail(DSBDD_ERR_ARG, "unknown option");
  }
  e->drop_graphs();
  return DSBDD_OK;
}

int dsbdd_engine_get_option(const dsbdd_engine* e, int which) {
  if (!e) return fail(DSBDD_ERR_ARG, "null argument");
  switch (which) {
    case DSBDD_OPT_PRUNE: return e->prune;
    case DSBDD_OPT_CONE: return e->cone;
    case DSBDD_OPT_GRANULE16: return (int)e->granule16;
    case DSBDD_OPT_SPLITK: return (int)e->splitk;
    case DSBDD_OPT_EMU: return e->emu;
    case DSBDD_OPT_SHELL: return e->shell;
    case DSBDD_OPT_TAIL: return e->tail;
    case DSBDD_OPT_CHAIN_DEAL: return e->chain_deal;
  }
  return fail(DSBDD_ERR_ARG, "unknown option");
}

int dsbdd_engine_set_trace(dsbdd_engine* e, float* th, float* tx) {
  if (!e) return DSBDD_ERR_ARG;
  e->trace_h = th; e->trace_x = tx;
  return DSBDD_OK;
}

int dsbdd_engine_profile(dsbdd_engine* e, int enable, int max_launches) {
  if (!e || max_launches < 0) return fail(DSBDD_ERR_ARG, "bad argument");
  e->profile = enable < 0 ? 0 : enable;      // 0 off, k: the launches of every k-th forward call are timed
  e->prof_call = 0;
  e->ev_used = 0;
  while (e->profile && e->ev.size() < (size_t)2 * max_launches) {
    hipEvent_t a;
    HIP_TRY(hipEventCreate(&a));
    e->ev.push_back(a);
  }
  return DSBDD_OK;
}

int dsbdd_engine_profile_read(dsbdd_engine* e, double* total_ms, int64_t* launches) {
  if (!e || !total_ms || !launches) return fail(DSBDD_ERR_ARG, "null argument");
  double tot = 0.0;
  for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
    HIP_TRY(hipEventSynchronize(e->ev[i + 1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev[i], e->ev[i + 1]));
    tot += ms;
  }
  *total_ms = tot;
  *launches = (int64_t)(e->ev_used / 2);
  e->ev_used = 0;
  return DSBDD_OK;
}

int dsbdd_engine_graph_stats(const dsbdd_engine* e, int64_t* replays, int64_t* captures, int64_t* eager) {
  if (!e || !replays || !captures || !eager) return fail(DSBDD_ERR_ARG, "null argument");
  *replays = e->n_replay; *captures = e->n_capture; *eager = e->n_eager;
  return DSBDD_OK;
}

int dsbdd_engine_buffer(const dsbdd_engine* e, int which, void** out) {
  if (!e || !out || !e->ws) return fail(DSBDD_ERR_STATE, "no workspace bound");
  void* const buf[] = {e->erow, e->ecol, e->ed0, e->row_ptr, e->h, e->x, e->node_batch, e->deg, e->lvl, e->lvl_list, e->lvl_cnt,
                       e->lvl_end, e->row_ptrL, e->erowL, e->ecolL, e->ed0L, e->lvl_stats};     // in the order of DSBDD_BUF_*
  static_assert(DSBDD_BUF_LEVEL_STATS + 1 == sizeof(buf) / sizeof(buf[0]), "one pointer per DSBDD_BUF_* id");
  if (which < 0 || which > DSBDD_BUF_LEVEL_STATS) return fail(DSBDD_ERR_ARG, "unknown buffer id");
  *out = buf[which];
  return DSBDD_OK;
}

int dsbdd_engine_list2_read(const dsbdd_engine* e, int which, void* dst, int64_t count) {
  if (!e || !dst || count < 0) return fail(DSBDD_ERR_ARG, "bad argument");
  if (!e->ws) return fail(DSBDD_ERR_STATE, "no workspace bound");
  const int64_t N = e->cap_lig + e->cap_poc;
  const int* src = which == DSBDD_LIST2_DEG ? e->deg2 : (which == DSBDD_LIST2_ROW_PTR ? e->row_ptr2 : nullptr);
  if (!src) return fail(DSBDD_ERR_ARG, "unknown list-2 buffer");
  if (count > N + (which == DSBDD_LIST2_ROW_PTR ? 1 : 0)) return fail(DSBDD_ERR_CAPACITY, "list-2 read past the buffer");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(dst, src, (size_t)count * 4, hipMemcpyDeviceToHost));
  return DSBDD_OK;
}

int dsbdd_engine_shell_read(const dsbdd_engine* e, int which, int list, void* dst, int64_t count) {
  if (!e || !dst || count < 0) return fail(DSBDD_ERR_ARG, "bad argument");
  if (!e->shell_mem) return fail(DSBDD_ERR_STATE, "no shell stage has run on this engine");
  const int64_t N = e->shell_key[0], SL = e->shell_key[2];
  const void* src = nullptr;
  int64_t have = 0, size = 4;
  const bool lst = list >= 0 && list < kShellLists;
  switch (which) {
    case DSBDD_SHELL_STATS: src = e->sh_stats; have = 8; size = 8; break;
    case DSBDD_SHELL_COUNT: src = e->sh_cnt; have = kShellLists; break;
    case DSBDD_SHELL_ROW: if (lst) { src = e->sh_row + (size_t)list * SL; have = SL; } break;
    case DSBDD_SHELL_COL: if (lst) { src = e->sh_col + (size_t)list * SL; have = SL; } break;
    case DSBDD_SHELL_PTR: src = e->sh_ptr; have = N; break;
    case DSBDD_SHELL_DEG: src = e->sh_deg; have = N; break;
  }
  if (!src) return fail(DSBDD_ERR_ARG, "unknown shell buffer");
  if (count > have) return fail(DSBDD_ERR_CAPACITY, "shell read past the buffer");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(dst, src, (size_t)(count * size), hipMemcpyDeviceToHost));
  return DSBDD_OK;
}

int dsbdd_dynamics_forward(dsbdd_engine* e, void* stream, const float* xh_lig, const float* xh_pocket,
                           const float* t, int64_t t_count, const int64_t* mask_lig,
                           const int64_t* mask_pocket, int64_t n_lig, int64_t n_pocket, int64_t batch,
                           const int32_t* ext_row, const int32_t* ext_col, int64_t ext_n_edges,
                           float* eps_lig, float* eps_pocket, int32_t* status) {
  StreamDevice stream_device_(stream);
  if (!e || !xh_lig || !xh_pocket || !t || !mask_lig || !mask_pocket || !eps_lig || !status)
    return fail(DSBDD_ERR_ARG, "null argument");
  if (!e->has_weights) return fail(DSBDD_ERR_STATE, "weights not set");
  if (!e->ws) return fail(DSBDD_ERR_STATE, "workspace not bound");
  if (n_lig > e->cap_lig || n_pocket > e->cap_poc || batch > e->cap_batch || n_lig < 0 || n_pocket < 0 ||
      batch < 1)
    return fail(DSBDD_ERR_CAPACITY, "sizes exceed the bound workspace");
  if (t_count != 1 && t_count != batch) return fail(DSBDD_ERR_ARG, "t must have 1 or batch entries");
  if (ext_row && (!ext_col || ext_n_edges < 0 || ext_n_edges > e->cap_edges))
    return fail(DSBDD_ERR_CAPACITY, "external edge list exceeds edge capacity");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const ForwardArgs args{xh_lig, xh_pocket, t, t_count, mask_lig, mask_pocket, n_lig, n_pocket, batch,
                         ext_row, ext_col, ext_n_edges, eps_lig, eps_pocket, status};
  const int rc = frame_upkeep(e, s, args);
  if (rc) return rc;
  // eager path: graphs off, timing / tracing hooks active (they enqueue event records and
  // copies that must not be frozen into a graph), or teacher-forced edges (test-only)
  // kernel timing: the calls whose launches are bracketed by event records run eagerly, the others may replay
  e->time_now = e->profile > 0 && (e->prof_call++ % e->profile) == 0;
  if (!e->use_graph || e->time_now || e->trace_h || e->trace_x || ext_row) {
    ++e->n_eager;
    return forward_impl(e, s, args);
  }
  return forward_cached(e, s, args);
}

}  // extern "C"
