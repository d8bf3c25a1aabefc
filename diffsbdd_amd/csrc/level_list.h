// Level-ordered edge list (pocket-conditioning mode, ligand output only), its shell lists, and the ghost rows of the
// pocket frame.
//
// The caller of a pocket-conditioned denoiser step reads the LIGAND rows of the output only
// (conditional_model.py:268-272 discards the pocket part), and the pocket coordinates are never updated.
// Walking the network backwards, the last message stage therefore only has to produce h for the nodes the
// last coordinate stage reads -- the ligand nodes and their neighbours (hop <= 1) --, the stage before it
// for hop <= 2, and so on: stage g of G message stages computes the rows with hop <= G - g, and reads its
// neighbours' h at hop <= G - g + 1.  Everything else is dead code for this call and is not evaluated.
// (Exactly the same numbers come out for the ligand: no live value depends on a skipped one.)
//
// hop(i) = graph distance from node i to the nearest ligand node of its sample (0 for ligand nodes), through
// the edges of this call; level(i) = min(hop, kLevels - 1).  The edge list is re-ordered by
// (level, node set, sample, row): the rows a stage needs are then a PREFIX of the list (lvl_end[r], a device
// scalar, like the update_coords_mask prefix), and the same nodes a prefix of lvl_list (lvl_cnt[r]) for the
// node-level GEMMs.  Every (level, sample) segment starts at a wave-tile boundary and a row's position in
// its segment depends on its own sample only, so results stay independent of the batch composition.
//
//   levels_kernel   one workgroup per sample: hop levels 2, 3 by relaxation over the natural-order list
//                   (level 1 comes from the count pass), then rows / edges per (level, sample); the sample's
//                   levels are held in LDS and its pocket-row edges in registers, one thread per edge (row
//                   walk over global memory for a sample that does not fit)
//   level_scan_kernel   one workgroup: exclusive scans over the kLevels * B segments
//   level_place_kernel  one workgroup per sample, wave L places level L: new row_ptr, lvl_list, pads
//   level_copy_kernel   one thread per natural-list slot: move the edge to its new position (and to its shell list)
#pragma once
#include "common.h"
#include "graph_parts.h"

namespace dsbdd {

struct LevelArgs {
  const int* node_batch; const int* lig_off; const int* poc_off; int n_lig; int B;
  int* lvl;                 // [N]
  const int* deg;           // [N]
  const int* row_ptr_nat;   // [N + 1] natural-order list
  const int* erow_nat; const int* ecol_nat; const float* ed0_nat;
  int* seg_rows;            // [kLevels * B] rows of segment (L, b);   level 0 = the ligand rows of sample b
  int* seg_edges;           // [kLevels * B] edges (not padded)
  int* node_base;           // [kLevels * B + 1] exclusive scan of seg_rows
  int* edge_base;           // [kLevels * B + 1] exclusive scan of the padded seg_edges
  int* lvl_cnt;             // [2][kLevels] nodes with level <= r: entries of lvl_list / without the leading ghost rows
  int* lvl_end;             // [2][kLevels] end of the edges of the rows with level <= r (padded): list position / minus edge_off
  int* lvl_list;            // [node_off + N] ghost rows, then the nodes ordered by (level, node id)
  int* row_ptr;             // [N] level-ordered list (the total is lvl_end[kLevels - 1])
  int* erow; int* ecol; float* ed0; int e_cap;
  // running sums over calls (bench / tests): [0..5) nodes with level <= r, [5..10) list slots, [10..15) edges, [15] calls
  unsigned long long* stats;
  // "ghost" rows of the canonical pocket (forward.h, forward cone): node_off entries at the front of lvl_list and
  // edge_off slots (a multiple of kEdgeAlign) at the front of the edge list are theirs, written once per chain
  int node_off; int edge_off;
  int e_cap_nat;            // capacity of the natural-order list: never indexed past it, even when the radius graph
                            // overflowed (status bit 1 is then set by edges_kernel and the call's result is discarded)
  const float* mean_x; float* mean_out;   // optional: levels_kernel also writes the per-sample mean of mean_x (sample_mean_body)
  // Shell lists of the forward cone (forward.h, "shell"): list s = 0 .. n_shell - 1 holds the rows of level s + 2 with
  // only their edges from columns of level <= s + 1, laid out like the main list (sorted by (sample, row), a row's edges
  // contiguous in their natural column order, one 32-aligned segment per sample).  n_shell == 0: not built.
  int n_shell;
  int* sh_seg;              // [kShellLists][B] edges of list s in sample b (not padded)
  int* sh_deg; int* sh_ptr; // [N] a shell row's degree / position in its list (a row has one level: one array serves all lists)
  int* sh_row; int* sh_col; float* sh_d0; int sh_cap;   // [kShellLists][sh_cap]
  int* sh_cnt;              // [kShellLists] slots of list s (padded): device scalars
  // running sums over calls, per list: [3 s] edges of the list, [3 s + 1] its slots, [3 s + 2] edges of its rows that are
  // NOT in it (columns of level >= s + 2: references to the canonical pocket's messages); [3 kShellLists] calls
  unsigned long long* sh_stats;
};

// levels_kernel keeps a sample's pocket levels in LDS and its pocket-row edges in registers when they fit (a sample is
// a few hundred nodes and a few thousand edges); a larger sample takes the walk over global memory (levels_rows_global).
constexpr int kLvlRows = 2048;     // pocket rows of a sample held in LDS
constexpr int kLvlEdges = 8192;    // slots of the sample's pocket segment of the natural-order list held in registers

// One thread per pocket row, over global memory: the relaxation passes, then the row / edge / shell counts.
__device__ __forceinline__ void levels_rows_global(const LevelArgs& a, const SampleRows& r, int* s_rows, int* s_edges,
                                                   int* s_shell) {
  const int t = threadIdx.x;
  for (int k = 2; k < kLevels - 1; ++k) {
    __syncthreads();                       // level k-1 is final (global writes of this workgroup are visible to it)
    for (int i = r.p0 + t; i < r.p1; i += kThreads) {
      if (a.lvl[i] != kLevels - 1) continue;
      const int s = a.row_ptr_nat[i], d = a.deg[i];
      bool hit = false;
      for (int e = max(s, 0); e < min(s + d, a.e_cap_nat) && !hit; ++e) {
        const int j = a.ecol_nat[e];
        hit = j >= a.n_lig && a.lvl[j] == k - 1;     // (a ligand neighbour would have made it level 1)
      }
      if (hit) a.lvl[i] = k;               // readers of this pass test == k-1: no race
    }
  }
  __syncthreads();
  for (int i = r.p0 + t; i < r.p1; i += kThreads) {
    const int L = a.lvl[i];
    atomicAdd(&s_rows[L], 1);              // integer sums: order does not matter
    atomicAdd(&s_edges[L], a.deg[i]);
    if (L >= 2 && L - 2 < a.n_shell) {     // a shell row: its edges from columns one level further in
      const int s = a.row_ptr_nat[i], d = a.deg[i];
      int d2 = 0;
      for (int e = max(s, 0); e < min(s + d, a.e_cap_nat); ++e) {
        const int j = a.ecol_nat[e];
        d2 += (j < a.n_lig || a.lvl[j] < L) ? 1 : 0;
      }
      a.sh_deg[i] = d2;
      atomicAdd(&s_shell[L - 2], d2);
    }
  }
}

// The same results from LDS and registers, one thread per EDGE: the pocket rows of a sample own one contiguous piece
// [e0, e1) of the natural-order list (rows in node order, then the segment's padding).  levels_stage reads the piece
// once, coalesced, every load independent of the others, into (row, column) codes local to the sample that stay in the
// thread's registers (thread t owns slots t, t + kThreads, ...); levels_solve then runs the passes and the shell count
// on the sample's levels in LDS.  Entries that are no edge of this sample's pocket rows (padding; anything at all
// after an overflow of the list) get code -1 and are skipped.
constexpr int kLvlPer = kLvlEdges / kThreads;   // edge slots per thread
constexpr int kLvlBatch = 8;                     // slots whose LDS reads are issued together
constexpr int kLvlStage = 16;                    // slots whose global loads are issued together
constexpr int kLvlLig = 0xffff;                  // column code of a ligand node (its level is 0)
static_assert(kLvlPer % kLvlBatch == 0 && kLvlPer % kLvlStage == 0 && kLvlRows < kLvlLig, "codes: row << 16 | column");

__device__ __forceinline__ void levels_stage(const LevelArgs& a, const SampleRows& r, int e0, int ne, int (&code)[kLvlPer],
                                             int* s_lvl, int* s_deg, int* s_cnt) {
  const int t = threadIdx.x, np = r.p1 - r.p0;
  for (int i = t; i < np; i += kThreads) { s_lvl[i] = a.lvl[r.p0 + i]; s_deg[i] = a.deg[r.p0 + i]; s_cnt[i] = 0; }
#pragma unroll
  for (int u = 0; u < kLvlPer; ++u) code[u] = -1;
  if (ne <= 0) return;
#pragma unroll
  for (int g = 0; g < kLvlPer; g += kLvlStage) {
    if (g * kThreads >= ne) break;         // (the same for every thread)
    int row[kLvlStage], col[kLvlStage];
#pragma unroll
    for (int u = 0; u < kLvlStage; ++u) {  // unconditional loads (a slot past the end reads the last one): one latency
      const int q = min((g + u) * kThreads + t, ne - 1);
      row[u] = a.erow_nat[e0 + q];
      col[u] = a.ecol_nat[e0 + q];
    }
#pragma unroll
    for (int u = 0; u < kLvlStage; ++u) {
      const int i = row[u], j = col[u];
      const bool mine = (g + u) * kThreads + t < ne && i >= r.p0 && i < r.p1;
      const int jc = (j >= r.l0 && j < r.l1) ? kLvlLig : ((j >= r.p0 && j < r.p1) ? j - r.p0 : -1);
      code[g + u] = (mine && jc >= 0) ? (((i - r.p0) << 16) | jc) : -1;
    }
  }
}

__device__ __forceinline__ void levels_solve(const LevelArgs& a, const SampleRows& r, int ne, const int (&code)[kLvlPer],
                                             int* s_rows, int* s_edges, int* s_shell, int* s_lvl, const int* s_deg,
                                             int* s_cnt) {
  const int t = threadIdx.x, np = r.p1 - r.p0;
  for (int k = 2; k < kLevels - 1; ++k) {
    __syncthreads();                       // level k-1 is final
#pragma unroll
    for (int g = 0; g < kLvlPer; g += kLvlBatch) {
      if (g * kThreads >= ne) break;       // (the same for every thread)
      int li[kLvlBatch], lj[kLvlBatch];
#pragma unroll
      for (int u = 0; u < kLvlBatch; ++u) {
        // (reads at a safe index whatever the code, then the choice: nothing waits inside a branch)
        const int c = code[g + u], j = c & 0xffff;
        const bool pj = c >= 0 && j != kLvlLig;              // (a ligand neighbour would have made the row level 1)
        const int vi = s_lvl[c >= 0 ? c >> 16 : 0], vj = s_lvl[pj ? j : 0];
        li[u] = c >= 0 ? vi : -1;
        lj[u] = pj ? vj : -1;
      }
      // writers of this pass store k over kLevels-1 and readers test == k-1: no race
#pragma unroll
      for (int u = 0; u < kLvlBatch; ++u)
        if (li[u] == kLevels - 1 && lj[u] == k - 1) s_lvl[code[g + u] >> 16] = k;
    }
  }
  __syncthreads();                         // the levels are final
  if (a.n_shell > 0) {
#pragma unroll
    for (int g = 0; g < kLvlPer; g += kLvlBatch) {
      if (g * kThreads >= ne) break;
      int li[kLvlBatch], lj[kLvlBatch];
#pragma unroll
      for (int u = 0; u < kLvlBatch; ++u) {
        const int c = code[g + u], j = c & 0xffff;
        const bool pj = c >= 0 && j != kLvlLig;
        const int vi = s_lvl[c >= 0 ? c >> 16 : 0], vj = s_lvl[pj ? j : 0];
        li[u] = c >= 0 ? vi : -1;
        lj[u] = pj ? vj : 0;                                 // (a ligand column: level 0)
      }
      // a shell row's edges from columns one level further in
#pragma unroll
      for (int u = 0; u < kLvlBatch; ++u)
        if (li[u] >= 2 && li[u] - 2 < a.n_shell && lj[u] < li[u]) atomicAdd(&s_cnt[code[g + u] >> 16], 1);
    }
  }
  __syncthreads();
  for (int i = t; i < np; i += kThreads) {
    const int L = s_lvl[i];
    if (L >= 2 && L < kLevels - 1) a.lvl[r.p0 + i] = L;   // (the other levels are what edges_kernel wrote)
    atomicAdd(&s_rows[L], 1);              // integer sums: order does not matter
    atomicAdd(&s_edges[L], s_deg[i]);
    if (L >= 2 && L - 2 < a.n_shell) {
      a.sh_deg[r.p0 + i] = s_cnt[i];
      atomicAdd(&s_shell[L - 2], s_cnt[i]);
    }
  }
}

__global__ __launch_bounds__(kThreads) void levels_kernel(LevelArgs a) {
  __shared__ int s_rows[kLevels], s_edges[kLevels], s_shell[kShellLists];
  __shared__ float s_red[3][kThreads];
  __shared__ int s_lvl[kLvlRows], s_deg[kLvlRows], s_cnt[kLvlRows];
  const int b = blockIdx.x, t = threadIdx.x;
  const SampleRows r = sample_rows(a.lig_off, a.poc_off, a.n_lig, b);
  // the pocket rows' piece of the natural-order list (clipped like every walk over it)
  int e0 = 0, e1 = 0;
  if (r.p1 > r.p0) {
    e0 = max(a.row_ptr_nat[r.p0], 0);
    e1 = min(a.row_ptr_nat[r.p1 - 1] + a.deg[r.p1 - 1], a.e_cap_nat);
  }
  const int ne = max(e1 - e0, 0);
  const bool fits = r.p1 - r.p0 <= kLvlRows && ne <= kLvlEdges;   // (the same for every thread of the workgroup)
  int code[kLvlPer];
  if (fits) levels_stage(a, r, e0, ne, code, s_lvl, s_deg, s_cnt);    // (its loads are in flight during the mean)
  if (a.mean_out) sample_mean_body(a.mean_x, a.lig_off, a.poc_off, a.n_lig, a.mean_out, s_red);
  if (t < kLevels) { s_rows[t] = 0; s_edges[t] = 0; }
  if (t < kShellLists) s_shell[t] = 0;
  if (fits) levels_solve(a, r, ne, code, s_rows, s_edges, s_shell, s_lvl, s_deg, s_cnt);
  else levels_rows_global(a, r, s_rows, s_edges, s_shell);
  int le = 0;
  for (int i = r.l0 + t; i < r.l1; i += kThreads) le += a.deg[i];
  if (le) atomicAdd(&s_edges[0], le);
  __syncthreads();
  if (t < kLevels) {
    a.seg_rows[t * a.B + b] = t == 0 ? (r.l1 - r.l0) : s_rows[t];
    a.seg_edges[t * a.B + b] = s_edges[t];
  }
  if (t < a.n_shell) a.sh_seg[t * a.B + b] = s_shell[t];
}

// Level t ends at node cn of lvl_list and at slot ce of the list; ed = edges (without padding) of the rows with
// level <= t.  One thread per level writes the ends, with and without the ghost part in front, and the statistics.
__device__ __forceinline__ void level_end_write(const LevelArgs& a, int t, int cn, int ce, unsigned long long ed) {
  a.lvl_cnt[t] = cn; a.lvl_cnt[kLevels + t] = cn - a.node_off;
  a.lvl_end[t] = ce; a.lvl_end[kLevels + t] = ce - a.edge_off;
  if (a.stats) {
    a.stats[t] += (unsigned long long)(cn - a.node_off);
    a.stats[kLevels + t] += (unsigned long long)(ce - a.edge_off);
    a.stats[2 * kLevels + t] += ed;
    if (t == 0) a.stats[3 * kLevels] += 1ull;
  }
}

__global__ __launch_bounds__(1024) void level_scan_kernel(LevelArgs a, int n_nodes) {
  __shared__ int s_wave[16];
  __shared__ int s_tot;
  const int t = threadIdx.x, S = kLevels * a.B;
  int carry_n = 0, carry_e = 0;
  for (int base = 0; base < S; base += 1024) {
    const int k = base + t;
    const int r = k < S ? a.seg_rows[k] : 0;
    const int e = k < S ? align_edges(a.seg_edges[k]) : 0;
    const int xn = carry_n + block_scan_1024(r, s_wave, &s_tot);
    carry_n += s_tot;
    __syncthreads();
    const int xe = carry_e + block_scan_1024(e, s_wave, &s_tot);
    carry_e += s_tot;
    __syncthreads();
    if (k < S) { a.node_base[k] = a.node_off + xn; a.edge_base[k] = a.edge_off + xe; }
  }
  if (t == 0) { a.node_base[S] = a.node_off + carry_n; a.edge_base[S] = a.edge_off + carry_e; }
  __syncthreads();
  if (t < kLevels) {                        // cumulative ends of the levels
    const int cn = t == kLevels - 1 ? a.node_off + carry_n : a.node_base[(t + 1) * a.B];
    const int ce = t == kLevels - 1 ? a.edge_off + carry_e : a.edge_base[(t + 1) * a.B];
    unsigned long long ed = 0;
    if (a.stats) {
      int own = 0;                          // edges (without padding) of level t, then of the rows with level <= t
      for (int k = t * a.B; k < (t + 1) * a.B; ++k) own += a.seg_edges[k];
      s_wave[t] = own;
      __threadfence_block();
      __builtin_amdgcn_wave_barrier();
      for (int k = 0; k <= t; ++k) ed += (unsigned long long)s_wave[k];   // (same wave: LDS writes are in order)
    }
    level_end_write(a, t, cn, ce, ed);
  }
}

// exclusive position of segment k = (L, b) among the kLevels * B segments: nodes, padded edges (wave sums)
__device__ __forceinline__ void level_bases(const LevelArgs& a, int k, int lane, int& nb, int& eb) {
  int sn = 0, se = 0;
  for (int k0 = 0; k0 < k; k0 += 64) {
    const int kk = k0 + lane;
    if (kk < k) { sn += a.seg_rows[kk]; se += align_edges(a.seg_edges[kk]); }
  }
  nb = a.node_off + wave_sum_i(sn);
  eb = a.edge_off + wave_sum_i(se);
}

// fold_scan != 0: no level_scan_kernel launch in front -- every wave finds the bases of its own segment with
// two wave sums over the (level, sample) table, and workgroup 0 writes the per-level ends / counts / statistics
__global__ __launch_bounds__(kThreads) void level_place_kernel(LevelArgs a, int fold_scan = 0) {
  static_assert(kThreads / 64 >= kLevels - 1, "one wave per pocket level");
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (fold_scan && b == 0 && w == kThreads / 64 - 1) {
    // cumulative ends of the levels (what level_scan_kernel wrote): level t ends where segment (t + 1, 0) begins
    unsigned long long ed_run = 0;
    for (int t = 0; t < kLevels; ++t) {
      int cn, ce;
      level_bases(a, (t + 1) * a.B, lane, cn, ce);
      int own = 0;
      for (int k0 = t * a.B; k0 < (t + 1) * a.B; k0 += 64) { const int kk = k0 + lane; if (kk < (t + 1) * a.B) own += a.seg_edges[kk]; }
      ed_run += (unsigned long long)wave_sum_i(own);
      if (lane == 0) level_end_write(a, t, cn, ce, ed_run);
    }
  }
  if (w == 0) {                             // ligand rows keep their natural order
    const int l0 = a.lig_off[b], l1 = a.lig_off[b + 1];
    int nb, eb;
    if (fold_scan) level_bases(a, b, lane, nb, eb); else { nb = a.node_base[b]; eb = a.edge_base[b]; }
    const int s0 = l0 < l1 ? a.row_ptr_nat[l0] : 0;
    for (int i = l0 + lane; i < l1; i += 64) {
      a.lvl_list[nb + (i - l0)] = i;
      a.row_ptr[i] = eb + (a.row_ptr_nat[i] - s0);
    }
    pad_fill(eb + a.seg_edges[b], lane, a.erow, a.ecol, a.ed0, a.e_cap);
  }
  const int L = w + 1;                      // pocket level of this wave
  if (L >= kLevels) return;
  const int p0 = a.n_lig + a.poc_off[b], p1 = a.n_lig + a.poc_off[b + 1];
  int n_run, e_run;
  if (fold_scan) level_bases(a, L * a.B + b, lane, n_run, e_run);
  else { n_run = a.node_base[L * a.B + b]; e_run = a.edge_base[L * a.B + b]; }
  // this wave's level is a shell: the rows' second list (sample b's segment starts behind the padded ones before it)
  const int sl = L - 2;
  const bool shell = sl >= 0 && sl < a.n_shell;
  int s_run = 0;
  if (shell) {
    int sp = 0;
    for (int k0 = 0; k0 < b; k0 += 64) {
      const int kk = k0 + lane;
      if (kk < b) sp += align_edges(a.sh_seg[sl * a.B + kk]);
    }
    s_run = wave_sum_i(sp);
  }
  const int s_begin = s_run;
  for (int i0 = p0; i0 < p1; i0 += 64) {
    const int i = i0 + lane;
    const bool mine = i < p1 && a.lvl[i] == L;
    const int d = mine ? a.deg[i] : 0;
    const unsigned long long m = __ballot(mine);
    const int incl = wave_scan_incl(d, lane);   // of the degrees of this level's rows
    if (mine) {
      a.lvl_list[n_run + __popcll(m & ((1ull << lane) - 1ull))] = i;
      a.row_ptr[i] = e_run + incl - d;
    }
    n_run += __popcll(m);
    e_run += __shfl(incl, 63);
    if (shell) {
      const int d2 = mine ? a.sh_deg[i] : 0;
      const int incl2 = wave_scan_incl(d2, lane);
      if (mine) a.sh_ptr[i] = s_run + incl2 - d2;              // (level_copy_kernel moves the edges)
      s_run += __shfl(incl2, 63);
    }
  }
  pad_fill(e_run, lane, a.erow, a.ecol, a.ed0, a.e_cap);
  if (shell) {
    const size_t o = (size_t)sl * a.sh_cap;
    const int to = pad_fill(s_run, lane, a.sh_row + o, a.sh_col + o, a.sh_d0 + o, a.sh_cap);
    if (lane == 0) {
      if (b == a.B - 1) a.sh_cnt[sl] = to;
      if (a.sh_stats) {
        const int own = s_run - s_begin;
        atomicAdd(&a.sh_stats[3 * sl], (unsigned long long)own);
        atomicAdd(&a.sh_stats[3 * sl + 1], (unsigned long long)(to - s_begin));
        atomicAdd(&a.sh_stats[3 * sl + 2], (unsigned long long)(a.seg_edges[L * a.B + b] - own));
        if (b == 0 && sl == 0) atomicAdd(&a.sh_stats[3 * kShellLists], 1ull);
      }
    }
  }
}

__global__ void level_copy_kernel(LevelArgs a, int n_nodes) {
  const int total = min(a.row_ptr_nat[n_nodes], a.e_cap_nat);
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int i = a.erow_nat[e];
    if (i < 0 || i >= n_nodes) continue;    // padding of the natural-order list
    const int pos = a.row_ptr[i] + (e - a.row_ptr_nat[i]);
    if (pos >= 0 && pos < a.e_cap) { a.erow[pos] = i; a.ecol[pos] = a.ecol_nat[e]; a.ed0[pos] = a.ed0_nat[e]; }
    // a shell row's edge from a column of a lower level also goes to the row's shell list, behind the row's earlier
    // edges of that kind (the same test as levels_kernel's count; one thread per edge: a walk over the row's few edges
    // in front of it is cheaper here than a serial walk per row in level_place_kernel, 58 -> 10 us at the benchmark size)
    const int L = i >= a.n_lig ? a.lvl[i] : 0;
    if (L >= 2 && L - 2 < a.n_shell) {
      const int j = a.ecol_nat[e];
      if (j < a.n_lig || a.lvl[j] < L) {
        int rank = 0;
        for (int q = max(a.row_ptr_nat[i], 0); q < e; ++q) {
          const int jq = a.ecol_nat[q];
          rank += (jq < a.n_lig || a.lvl[jq] < L) ? 1 : 0;
        }
        const int ps = a.sh_ptr[i] + rank;
        const size_t o = (size_t)(L - 2) * a.sh_cap;
        if (ps >= 0 && ps < a.sh_cap) { a.sh_row[o + ps] = i; a.sh_col[o + ps] = j; a.sh_d0[o + ps] = a.ed0_nat[e]; }
      }
    }
  }
}

// Ghost rows of the canonical pocket: the static pocket-pocket list of the frame's representative (node ids
// id_src + i) becomes the front segment of the level-ordered list with node ids id_dst + i; their degrees,
// list positions and places at the front of lvl_list are static for the chain.
__global__ void ghost_setup_kernel(const int* erow3, const int* ecol3, const float* ed03, const int* row_ptr3,
                                   const int* deg3, int n3, int id_src, int id_dst, int* erow, int* ecol,
                                   float* ed0, int e_cap, int* deg, int* row_ptr, int* lvl_list,
                                   const float* xframe, float* x) {
  const int total = min(row_ptr3[n3], e_cap);
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
    const int r = erow3[p];
    erow[p] = r < 0 ? -1 : r - id_src + id_dst;
    ecol[p] = r < 0 ? 0 : ecol3[p] - id_src + id_dst;
    ed0[p] = ed03[p];
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n3; i += gridDim.x * blockDim.x) {
    deg[id_dst + i] = deg3[i];
    row_ptr[id_dst + i] = row_ptr3[i];
    lvl_list[i] = id_dst + i;
    x[3 * (id_dst + i)] = xframe[3 * i]; x[3 * (id_dst + i) + 1] = xframe[3 * i + 1];
    x[3 * (id_dst + i) + 2] = xframe[3 * i + 2];
  }
}

// dst[i][:] = src[rows[i]][:]  (one wave per row, 16-byte lanes): embedded features of the frame's pockets -> ghost rows
__global__ __launch_bounds__(kThreads) void gather_rows_kernel(float* dst, const float* src, const int* rows, int n,
                                                               int H) {
  const int i = (blockIdx.x * kThreads + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (i >= n) return;
  const float* a = src + (size_t)rows[i] * H;
  float* b = dst + (size_t)i * H;
  for (int k = 4 * lane; k < H; k += 256) *reinterpret_cast<float4*>(b + k) = ld4(a + k);
}

// h[i] <- h[ghost twin of i] for the pocket rows with lo < level <= hi: rows the next message stage reads but the
// ligand could not have influenced yet -- their value is the canonical pocket's (forward.h, forward cone).
__global__ __launch_bounds__(kThreads) void canon_fill_kernel(float* h, const int* lvl, const int* twin_local,
                                                              int n_lig, int n_nodes, int ghost_base, int lo,
                                                              int hi, int H, float* pq = nullptr, int ldpq = 0) {
  const int i = n_lig + ((blockIdx.x * kThreads + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (i >= n_nodes) return;
  const int L = lvl[i];
  if (L <= lo || L > hi) return;
  const int g = ghost_base + twin_local[i - n_lig];
  const float* src = h + (size_t)g * H;
  float* dst = h + (size_t)i * H;
  for (int k = 4 * lane; k < H; k += 256) *reinterpret_cast<float4*>(dst + k) = ld4(src + k);
  // pq: a projection of h that was computed for the ghost rows in the same launch as their h (the next message stage's
  // P|Q): a row that takes the canonical h takes the canonical projection too -- the same bits a GEMM over it would give
  if (pq)
    for (int k = 4 * lane; k < ldpq; k += 256)
      *reinterpret_cast<float4*>(pq + (size_t)i * ldpq + k) = ld4(pq + (size_t)g * ldpq + k);
}

}  // namespace dsbdd
