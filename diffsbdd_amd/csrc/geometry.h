// Per-sample geometry of EGNNDynamics.forward:
//   - input assembly (split xh, time feature)             dynamics.py:89-111
//   - per-sample mean of x for coord2cross                egnn_new.py:307-310
//   - coordinate update, velocity / NaN guard / COM       dynamics.py:136,155-164
#pragma once
#include "common.h"
#include "graph_parts.h"
#include "radius_graph.h"   // prep_offsets, prep_node

namespace dsbdd {

// prep_kernel and the input assembly in one launch (thread i: node i and sample i): x[N][3] <- coordinates of both node
// sets; h0[:, J] <- t[sample]; pad columns of h0 (J+1..JP-1) <- 0 (dynamics.py:89-111).  The time feature is looked up
// through the masks themselves, so no thread depends on another one's node_batch entry.
__global__ void prep_assemble_kernel(const int64_t* mask_lig, int n_lig, const int64_t* mask_poc, int n_poc, int B,
                                     int* node_batch, int* lig_off, int* poc_off, int* tile_ctr, const float* xh_lig,
                                     int dl, const float* xh_poc, int dp, const float* t, int t_count, float* x,
                                     float* x_in, float* h0, int J, int JP) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  prep_offsets(i, mask_lig, n_lig, mask_poc, n_poc, B, lig_off, poc_off, tile_ctr);
  if (i >= n_lig + n_poc) return;
  const int b = prep_node(i, mask_lig, n_lig, mask_poc, node_batch);
  const float* src = i < n_lig ? xh_lig + (size_t)i * dl : xh_poc + (size_t)(i - n_lig) * dp;
  const float a0 = src[0], a1 = src[1], a2 = src[2];
  x[3 * i] = a0; x[3 * i + 1] = a1; x[3 * i + 2] = a2;
  x_in[3 * i] = a0; x_in[3 * i + 1] = a1; x_in[3 * i + 2] = a2;
  h0[(size_t)i * JP + J] = t[t_count == 1 ? 0 : b];
  for (int k = J + 1; k < JP; ++k) h0[(size_t)i * JP + k] = 0.f;
}

// mean[b] = mean of x over ALL nodes of sample b; one workgroup per sample.
__global__ __launch_bounds__(kThreads) void sample_mean_kernel(const float* x, const int* lig_off,
                                                               const int* poc_off, int n_lig,
                                                               float* mean) {
  __shared__ float red[3][kThreads];
  sample_mean_body(x, lig_off, poc_off, n_lig, mean, red);
}

// What the coordinate edge kernel leaves for the update: per MLP population q, the partial sum of the wave tile that
// holds the row's first edge in xagg[q][i] and the partial sums of the following tiles of a row that spans several
// in xhead[q][tile].
struct CoordSums {
  const float* xagg; const float* xhead; int n_q;
  size_t xagg_stride, xhead_stride;
  const int* row_ptr; const int* deg;
  int max_tile, shift;     // (see agg_complete_kernel)
};

// x[k] += (sum over the row's edges of trans) for component k = 3 i + c of node i: the partial sums are added in tile
// order (fixed summation order, no atomics).
__device__ __forceinline__ void coord_row_update(float* x, const CoordSums& p, int k) {
  const int i = k / 3, c = k - 3 * i;
  const int d = p.deg[i];
  if (d == 0) return;
  const int s = p.row_ptr[i], t0 = s >> p.shift, t1 = min((s + d - 1) >> p.shift, p.max_tile);
  float tot = 0.f;
  for (int q = 0; q < p.n_q; ++q) {
    float a = p.xagg[q * p.xagg_stride + k];
    for (int T = t0 + 1; T <= t1; ++T) a += p.xhead[q * p.xhead_stride + 4 * (size_t)T + c];
    tot += a;
  }
  x[k] += tot;
}

// The update of the nodes whose coordinates change (update_coords_mask, egnn_new.py:118-121; the first n_upd3 / 3 nodes),
// one thread per component.
__global__ void coord_update_kernel(float* x, CoordSums p, int n_upd3) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < n_upd3) coord_row_update(x, p, idx);
}

// The same update with one workgroup per sample, followed by the per-sample mean of the NEW coordinates (the next
// block's coord2cross reference point): one launch instead of two between two blocks.
__global__ __launch_bounds__(kThreads) void coord_update_mean_kernel(float* x, CoordSums p, int n_upd,
                                                                     const int* lig_off, const int* poc_off,
                                                                     int n_lig, float* mean) {
  __shared__ float red[3][kThreads];
  const SampleRows r = sample_rows(lig_off, poc_off, n_lig, blockIdx.x);
  for (int seg = 0; seg < 2; ++seg) {
    const int a = seg ? r.p0 : r.l0, e = min(seg ? r.p1 : r.l1, n_upd);
    for (int k = 3 * a + (int)threadIdx.x; k < 3 * e; k += kThreads) coord_row_update(x, p, k);
  }
  if (!mean) return;
  __syncthreads();
  sample_mean_body(x, lig_off, poc_off, n_lig, mean, red);
}

// vel = x_final - x_in (dynamics.py:136), NaN guard (dynamics.py:155-159: flag
// instead of a host sync), optional per-sample mean removal in joint mode
// (dynamics.py:161-164), scatter into eps[:, 0:3].  One workgroup per sample.
__global__ __launch_bounds__(kThreads) void finalize_kernel(
    const float* x, const float* x_in, const int* lig_off, const int* poc_off, int n_lig,
    int remove_mean, float* eps_lig, int dl, float* eps_poc, int dp, int* status) {
  __shared__ float red[3][kThreads];
  const int t = threadIdx.x;
  const SampleRows r = sample_rows(lig_off, poc_off, n_lig, blockIdx.x);
  float m0 = 0.f, m1 = 0.f, m2 = 0.f;
  bool nan = false;
  if (remove_mean) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int seg = 0; seg < 2; ++seg) {
      const int a = seg ? r.p0 : r.l0, e = seg ? r.p1 : r.l1;
      for (int i = a + t; i < e; i += kThreads) {
        s0 += x[3 * i] - x_in[3 * i]; s1 += x[3 * i + 1] - x_in[3 * i + 1]; s2 += x[3 * i + 2] - x_in[3 * i + 2];
      }
    }
    block_sum3(s0, s1, s2, red);
    const float cnt = (float)r.count();
    m0 = red[0][0] / cnt; m1 = red[1][0] / cnt; m2 = red[2][0] / cnt;
  }
  for (int seg = 0; seg < 2; ++seg) {
    const int a = seg ? r.p0 : r.l0, e = seg ? r.p1 : r.l1;
    for (int i = a + t; i < e; i += kThreads) {
      const float v0 = x[3 * i] - x_in[3 * i], v1 = x[3 * i + 1] - x_in[3 * i + 1],
                  v2 = x[3 * i + 2] - x_in[3 * i + 2];
      nan = nan || (v0 != v0) || (v1 != v1) || (v2 != v2);
      float* dst = nullptr;
      if (seg == 0) dst = eps_lig + (size_t)i * dl;
      else if (eps_poc) dst = eps_poc + (size_t)(i - n_lig) * dp;
      if (dst) { dst[0] = v0 - m0; dst[1] = v1 - m1; dst[2] = v2 - m2; }
    }
  }
  if (nan) atomicOr(status, 1);
}

}  // namespace dsbdd
