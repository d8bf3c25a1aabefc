// The edge list of EGNNDynamics.forward:
//   - sample offsets from the (sorted) batch masks
//   - radius graph -> edge list sorted by (row, col)      dynamics.py:169-187
//   - the teacher-forced list, and the compaction of the active nodes
// O(N * n_per_sample) integer/float byte work (HBM/latency bound, microseconds); one wave per row,
// ballot-compaction keeps the reference's (row, col) order without a sort.
#pragma once
#include "common.h"
#include "graph_parts.h"

namespace dsbdd {

struct Cutoffs {
  int has_l, has_p, has_i;
  float cl, cp, ci;
};

// Masks -> offsets, thread i = sample i: lig_off[b] / poc_off[b] = first ligand / pocket node of sample b (b = 0..B);
// the first kTileCtrInts threads also clear the work-queue counters of the edge kernels.
__device__ __forceinline__ void prep_offsets(int i, const int64_t* mask_lig, int n_lig, const int64_t* mask_poc,
                                             int n_poc, int B, int* lig_off, int* poc_off, int* tile_ctr) {
  if (tile_ctr && i < kTileCtrInts) tile_ctr[i] = 0;
  if (i <= B) {
    lig_off[i] = lower_bound_i64(mask_lig, n_lig, i);
    poc_off[i] = lower_bound_i64(mask_poc, n_poc, i);
  }
}
// ... and thread i = node i ([ligand | pocket] numbering, i < n_lig + n_poc): node_batch[i] = its sample id, returned
__device__ __forceinline__ int prep_node(int i, const int64_t* mask_lig, int n_lig, const int64_t* mask_poc,
                                         int* node_batch) {
  const int b = (int)(i < n_lig ? mask_lig[i] : mask_poc[i - n_lig]);
  node_batch[i] = b;
  return b;
}

__global__ void prep_kernel(const int64_t* mask_lig, int n_lig, const int64_t* mask_poc, int n_poc,
                            int B, int* node_batch, int* lig_off, int* poc_off, int* tile_ctr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  prep_offsets(i, mask_lig, n_lig, mask_poc, n_poc, B, lig_off, poc_off, tile_ctr);
  if (i < n_lig + n_poc) prep_node(i, mask_lig, n_lig, mask_poc, node_batch);
}

struct SegAlign {
  const int* node_batch; const int* lig_off; const int* poc_off;
  int n_lig; int B;
  int* scan_tmp;   // [n + 1] plain exclusive scan
  int* seg_base;   // [2B + 1]
};

// Optional second output of the radius graph: the edges that have a LIGAND endpoint (all edges of
// ligand rows + the ligand columns of pocket rows), in the same aligned layout with its own
// row_ptr / deg.  Block 0 of a pocket-conditioned chain evaluates the pocket-pocket messages
// separately (forward.h, "Pocket frame"), so its message stage runs on this list.
struct EdgeList2 {
  int* deg; int* row_ptr; int* erow; int* ecol; float* ed0; int e_cap;
  SegAlign seg;      // scan_tmp / seg_base of this list
};

// One wave per row node.  FILL=false counts neighbours (deg), FILL=true writes
// them at row_ptr[row].  Candidates are visited in index order (ligand nodes of
// the sample, then its pocket nodes) and compacted with ballot/popcount, so the
// output is sorted by (row, col) like torch.where(adj) (dynamics.py:185).
// Self loops are kept (distance 0 <= cutoff; dynamics.py never removes them).
template <bool FILL>
__global__ __launch_bounds__(kThreads) void edges_kernel(
    const float* __restrict__ x, const int* __restrict__ node_batch,
    const int* __restrict__ lig_off, const int* __restrict__ poc_off, int n_lig, int n_nodes,
    Cutoffs cut, int* __restrict__ deg, const int* __restrict__ row_ptr, int* __restrict__ erow,
    int* __restrict__ ecol, float* __restrict__ ed0, int e_cap, int* __restrict__ status,
    int* __restrict__ act_flag, SegAlign seg, int* __restrict__ row_ptr_out, EdgeList2 l2, int id_offset,
    int* __restrict__ lvl = nullptr) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  for (int i = wave; i < n_nodes; i += nwaves) {
    const int b = node_batch[i];
    const bool il = i < n_lig;
    const float xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
    // aligned layout: first edge of row i = base of its (sample, node set) segment + the edges of the
    // segment's earlier rows (plain scan differences); compact layout: the plain scan itself
    int base = 0;
    int base2 = 0;
    if (FILL) {
      if (seg.seg_base) {
        const int k = il ? b : seg.B + b;
        const int first = il ? lig_off[b] : n_lig + poc_off[b];
        base = seg.seg_base[k] + seg.scan_tmp[i] - seg.scan_tmp[first];
        if (lane == 0) row_ptr_out[i] = base;
      } else {
        base = row_ptr[i];
      }
    }
    if (FILL && l2.deg) {
      const int k = il ? b : l2.seg.B + b;
      const int first = il ? lig_off[b] : n_lig + poc_off[b];
      base2 = l2.seg.seg_base[k] + l2.seg.scan_tmp[i] - l2.seg.scan_tmp[first];
      if (lane == 0) l2.row_ptr[i] = base2;
    }
    int cnt = 0, cnt_lig = 0;
#pragma unroll 1
    for (int seg = 0; seg < 2; ++seg) {
      const int j_begin = seg == 0 ? lig_off[b] : n_lig + poc_off[b];
      const int j_end = seg == 0 ? lig_off[b + 1] : n_lig + poc_off[b + 1];
      const bool jl = seg == 0;
      const int has = (il && jl) ? cut.has_l : ((!il && !jl) ? cut.has_p : cut.has_i);
      const float c = (il && jl) ? cut.cl : ((!il && !jl) ? cut.cp : cut.ci);
      for (int j0 = j_begin; j0 < j_end; j0 += 64) {
        const int j = j0 + lane;
        const bool valid = j < j_end;
        float d2 = 0.f;
        if (valid) {
          const float dx = xi - x[3 * j], dy = yi - x[3 * j + 1], dz = zi - x[3 * j + 2];
          d2 = dx * dx + dy * dy + dz * dz;
        }
        // torch.cdist(...) <= cutoff  (dynamics.py:174-181), on the exact distance
        const bool pass = valid && (!has || __fsqrt_rn(d2) <= c);
        const unsigned long long m = __ballot(pass);
        if (FILL && pass) {
          const int pos = base + cnt + __popcll(m & ((1ull << lane) - 1ull));
          if (pos >= 0 && pos < e_cap) {   // (pos < 0 only with unsorted masks, which the host rejects)
            erow[pos] = i + id_offset; ecol[pos] = j + id_offset; ed0[pos] = d2;
          }
          if (l2.deg && (il || jl)) {     // ligand columns come first in a row: same running position
            const int pos2 = base2 + cnt + __popcll(m & ((1ull << lane) - 1ull));
            if (pos2 >= 0 && pos2 < l2.e_cap) { l2.erow[pos2] = i; l2.ecol[pos2] = j; l2.ed0[pos2] = d2; }
          }
        }
        cnt += __popcll(m);
      }
      if (seg == 0) cnt_lig = cnt;
    }
    if (!FILL && lane == 0) {
      deg[i] = cnt;
      if (l2.deg) l2.deg[i] = il ? cnt : cnt_lig;
      // "active" for the coordinate MLPs in pocket-conditioning mode: ligand nodes and
      // pocket nodes that are a column of some ligand-row edge (graph is symmetric)
      if (act_flag) act_flag[i] = (il || cnt_lig > 0) ? 1 : 0;
      // hop level of the node (level_list.h, levels_kernel): 0 ligand, 1 = pocket node with a ligand neighbour
      if (lvl) lvl[i] = il ? 0 : (cnt_lig > 0 ? 1 : kLevels - 1);
    }
    if (FILL && lane == 0 && base + cnt > e_cap) atomicOr(status, 2);
    if (FILL && seg.seg_base) {
      // the last row of a (sample, node set) segment pads the segment (pad_fill), see scan_kernel
      const int seg_last = (il ? lig_off[b + 1] : n_lig + poc_off[b + 1]) - 1;
      if (i == seg_last) {
        pad_fill(base + cnt, lane, erow, ecol, ed0, e_cap);
        if (l2.deg) pad_fill(base2 + (il ? cnt : cnt_lig), lane, l2.erow, l2.ecol, l2.ed0, l2.e_cap);
      }
    }
  }
}

// Exclusive scan of deg[0..n) -> row_ptr[0..n], row_ptr[n] = total.  One
// workgroup of 1024 threads (n is tens of thousands) walks tiles of 4096
// elements: coalesced 16-byte loads, 4-element serial prefix per lane, wave
// scan by lane shuffles, 16 wave totals through LDS, running carry in a register.
//
// With `seg` set, the edges of every (sample, node set) segment -- the rows of the ligand
// nodes of sample b, then the rows of its pocket nodes; 2B segments in node order -- start at
// a multiple of kEdgeAlign: row_ptr[i] = seg_base[segment of i] + (edges of the earlier rows
// of that segment) -- evaluated and stored by edges_kernel<true> from the plain scan and seg_base
// computed here --, row_ptr[n] = padded total, and the gaps are filled with inactive entries by
// edges_kernel<true>.  A wave tile of the edge kernels (32 consecutive edges) then never mixes
// samples and holds the same edges whatever else is in the batch, which makes every per-row sum
// independent of the batch composition (bitwise identical results for any sharding).
// A row's edge count stays in deg[]; row i owns [row_ptr[i], row_ptr[i] + deg[i]).
__device__ void scan_one(const int* deg, int* row_ptr, int n, SegAlign seg, int* s_wave, int* s_carry_p);

__global__ __launch_bounds__(1024) void scan_kernel(const int* deg, int* row_ptr, int n, SegAlign seg,
                                                    const int* deg_b, int* row_ptr_b, SegAlign seg_b) {
  __shared__ int s_wave[16];
  __shared__ int s_carry;
  // the second list of the same launch (EdgeList2) is workgroup 1's: the two scans share nothing (grid = 2 with deg_b)
  if (blockIdx.x == 0) scan_one(deg, row_ptr, n, seg, s_wave, &s_carry);
  else if (deg_b) scan_one(deg_b, row_ptr_b, n, seg_b, s_wave, &s_carry);
}

__device__ void scan_one(const int* deg, int* row_ptr, int n, SegAlign seg, int* s_wave, int* s_carry_p) {
  int& s_carry = *s_carry_p;
  const int t = threadIdx.x;
  int* out = seg.seg_base ? seg.scan_tmp : row_ptr;
  const bool vec = ((reinterpret_cast<uintptr_t>(deg) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  int carry = 0;
  for (int base = 0; base < n; base += 4096) {
    const int i0 = base + 4 * t;
    int v[4] = {0, 0, 0, 0};
    if (vec && i0 + 3 < n) {
      const int4 q = *reinterpret_cast<const int4*>(deg + i0);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (i0 + k < n) v[k] = deg[i0 + k];
    }
    const int mine = v[0] + v[1] + v[2] + v[3];
    int run = carry + block_scan_1024(mine, s_wave, s_carry_p);
    const int tile_total = s_carry;
    if (vec && i0 + 3 < n) {
      int4 o4;
      o4.x = run; o4.y = run + v[0]; o4.z = o4.y + v[1]; o4.w = o4.z + v[2];
      *reinterpret_cast<int4*>(out + i0) = o4;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) if (i0 + k < n) { out[i0 + k] = run; run += v[k]; }
    }
    carry += tile_total;
    __syncthreads();                                   // s_wave / s_carry are reused by the next tile
  }
  if (t == 0) out[n] = carry;
  if (!seg.seg_base) return;
  __syncthreads();                                     // the plain scan is visible to the whole workgroup
  // padded length of every segment -> exclusive scan -> seg_base
  const int S = 2 * seg.B;
  auto seg_begin = [&](int k) { return k < seg.B ? seg.lig_off[k] : seg.n_lig + seg.poc_off[k - seg.B]; };
  auto seg_end = [&](int k) { return k < seg.B ? seg.lig_off[k + 1] : seg.n_lig + seg.poc_off[k - seg.B + 1]; };
  carry = 0;
  for (int base = 0; base < S; base += 1024) {
    const int k = base + t;
    int len = 0;
    if (k < S) len = align_edges(max(out[seg_end(k)] - out[seg_begin(k)], 0));
    const int ex = carry + block_scan_1024(len, s_wave, s_carry_p);
    if (k < S) seg.seg_base[k] = ex;
    carry += s_carry;
    __syncthreads();
  }
  if (t == 0) {
    seg.seg_base[S] = carry;
    row_ptr[n] = carry;           // padded total; row_ptr[0 .. n) is written by edges_kernel<true>
  }
}

// Teacher-forced edge list: copy rows/cols, compute d0, build row_ptr counts.
__global__ void ext_edges_kernel(const int* row, const int* col, int E, const float* x, int* erow,
                                 int* ecol, float* ed0, int* deg) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int r = row[e], c = col[e];
  erow[e] = r; ecol[e] = c;
  const float dx = x[3 * r] - x[3 * c], dy = x[3 * r + 1] - x[3 * c + 1], dz = x[3 * r + 2] - x[3 * c + 2];
  ed0[e] = dx * dx + dy * dy + dz * dz;
  atomicAdd(&deg[r], 1);
}

// Active-node flags for a teacher-forced edge list: ligand nodes, plus every column
// of an edge whose row is a ligand node.
__global__ void ext_flags_init_kernel(int* flag, int n_lig, int n_nodes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_nodes) flag[i] = i < n_lig ? 1 : 0;
}
__global__ void ext_flags_kernel(const int* row, const int* col, int E, int n_lig, int* flag) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < E && row[e] < n_lig) flag[col[e]] = 1;   // benign race: all writers store 1
}
// list[ptr[i]] = i for flagged nodes (ptr = exclusive scan of flag): sorted node list.
__global__ void compact_kernel(const int* flag, const int* ptr, int* list, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flag[i]) list[ptr[i]] = i;
}

}  // namespace dsbdd
