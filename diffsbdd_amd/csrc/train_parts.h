// The parts that the backward edge kernels of train.h share (kernel A and kernel B: lane = edge, 128-edge tiles on the
// matrix cores; kernel E: wave = edge, element-wise on the kept z2).  A kernel keeps its own tiling and its own
// epilogue; the rules of the backward pass's bitwise-reproducibility contract and of its agreement with the forward
// pass that can be stated once are stated here:
//
//   bwd_entry_active, bwd_lane_entry, bwd_edge_type      a list entry: which entries are active, what an inactive one
//                         reads as, the edge type
//   store_coord_pieces    the coordinate stage's per-edge gradient pieces -> gxr / gxc / gm
//   ld_cols, st_cols, wave_sum_f, first_layer_cols      kernel E: a lane's columns of a row, the element-wise first layer
//   fold_wave_partials    kernels A / B: the 8 (wave, half) partial vectors in LDS -> rows of the workgroup's [8][H] slot
//   fold16_wave_partials  kernel E: the 16 waves' partial vectors -> rows 5 .. 7 of the workgroup's slot
//
// Plain inline functions on the caller's registers: integer work, loads / stores and explicit fmaf chains only.
// |x_r - x_c|^2 and the geometry backward of the coordinate head (a * b + c * d expressions) stay written out in the
// kernels: the compiler contracts and pairs them by their surroundings; behind a call the last bit moved (profiles/train_parts.md).
#pragma once
#include "common.h"

namespace dsbdd {

// partial vectors of a workgroup, one [8][H] slot per workgroup (TrainEdgeArgs::part)
constexpr int kPartA = 3;   // kernel A: d_b2, d_head (att_w / w3), [0] = d_att_b
constexpr int kPartB = 5;   // kernel B: d_wd, d_wd0, d_tab[0..2]
constexpr int kPartAll = kPartA + kPartB;   // B's rows first = dsbdd_train_mlp_grad::d_vec: ONE ordered reduction serves both kernels

__device__ __forceinline__ float dsilu_from(float z, float sg) { return sg * (1.0f + z * (1.0f - sg)); }

// ---- a list entry ---------------------------------------------------------------------------------------------------
// THE activity rule: an entry counts when both ids are nodes.  Any other entry -- and, in the tiled kernels, a lane
// behind the list's end -- reads as r = c = 0, d0 = 0, d = 0, and the kernels write zero rows for it (the
// weight-gradient GEMM sums over every row of the list).
__device__ __forceinline__ bool bwd_entry_active(int r, int c, int n_nodes) {
  return !((unsigned)r >= (unsigned)n_nodes || (unsigned)c >= (unsigned)n_nodes);
}
// THE type rule (the row of the bias + edge-type table): 1 ligand-ligand, 2 pocket-pocket, 0 mixed
__device__ __forceinline__ int bwd_edge_type(int r, int c, int n_lig) {
  const bool rl = r < n_lig, cl = c < n_lig;
  return (rl && cl) ? 1 : ((!rl && !cl) ? 2 : 0);
}
// per-lane form (kernels A / B): entry e of a list of E entries -> r, c, d0; returns whether it is active.  (Kernel E
// reads the entry wave-uniformly into scalar registers itself and asks bwd_entry_active.)
__device__ __forceinline__ bool bwd_lane_entry(const int* erow, const int* ecol, const float* ed0, int E, int e, int n_nodes,
                                               int& r, int& c, float& d0) {
  bool active = e < E;
  r = 0; c = 0; d0 = 0.f;
  if (active) {
    r = erow[e]; c = ecol[e]; d0 = ed0[e];
    if (!bwd_entry_active(r, c, n_nodes)) { active = false; r = 0; c = 0; d0 = 0.f; }
  }
  return active;
}
// entry e's pieces -> gxr / gxc / gm [E][3] (gm: the second MLP only); the caller picks the one lane that stores
__device__ __forceinline__ void store_coord_pieces(float* gxr, float* gxc, float* gm, int e, const float (&ar)[3],
                                                   const float (&ac)[3], const float (&am)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gxr[3 * (size_t)e + k] = ar[k];
    gxc[3 * (size_t)e + k] = ac[k];
    if (gm) gm[3 * (size_t)e + k] = am[k];
  }
}

// ---- kernel E: wave = edge, lane l holds columns V l .. V l + V - 1 (V = H / 64), 16 waves per workgroup -----------------
constexpr int kThreadsE = 1024;
template <int V>
__device__ __forceinline__ void ld_cols(const float* row, int lane, float (&v)[V]) {
  if constexpr (V == 4) { const float4 q = *reinterpret_cast<const float4*>(row + 4 * lane); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
  else if constexpr (V == 2) { const float2 q = *reinterpret_cast<const float2*>(row + 2 * lane); v[0] = q.x; v[1] = q.y; }
  else {
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = row[V * lane + k];
  }
}
template <int V>
__device__ __forceinline__ void st_cols(float* row, int lane, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(row + 4 * lane) = float4{v[0], v[1], v[2], v[3]};
  else if constexpr (V == 2) *reinterpret_cast<float2*>(row + 2 * lane) = float2{v[0], v[1]};
  else {
#pragma unroll
    for (int k = 0; k < V; ++k) row[V * lane + k] = v[k];
  }
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// a1 = SiLU(z1), the first layer as kernel A evaluates it (first_layer_act4, edge_parts.h: the same fma nesting)
template <int V>
__device__ __forceinline__ void first_layer_cols(const float (&pv)[V], const float (&qv)[V], float d, float d0, int ty,
                                                 const float (&wd)[V], const float (&wd0)[V], const float (&tb)[3][V],
                                                 float (&a1)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) a1[k] = silu(fmaf(d0, wd0[k], fmaf(d, wd[k], pv[k] + qv[k])) + tb[ty][k]);
}
// Partial vectors of a 16-wave workgroup: the waves' sums of two [H] rows (and, PS, of one scalar) are added in wave
// order -> the kPartA rows at `slot` (row 2 = the scalar in column 0, zeros elsewhere).
template <int H, bool PS>
__device__ __forceinline__ void fold16_wave_partials(float (*sP)[2 * H + 4], int w, int lane, int t,
                                                     const float (&row0)[H / 64], const float (&row1)[H / 64], float ps,
                                                     float* slot) {
  st_cols<H / 64>(sP[w], lane, row0);
  st_cols<H / 64>(sP[w] + H, lane, row1);
  if (PS && lane == 0) sP[w][2 * H] = ps;
  __syncthreads();
  for (int i = t; i < kPartA * H; i += kThreadsE) {
    float v = 0.f;
    if (i < 2 * H) {
#pragma unroll
      for (int q = 0; q < kThreadsE / 64; ++q) v += sP[q][i];
    } else if (PS && i == 2 * H) {
#pragma unroll
      for (int q = 0; q < kThreadsE / 64; ++q) v += sP[q][2 * H];
    }
    slot[i] = v;
  }
}

// ---- kernels A / B: lane = edge, accumulator register q of a lane = row mfma_row(q, lane) of the wave's 32-edge tile ----
// (wave w, half h) has written its NP partial rows to s + (2 w + h) NP H; their sums in the order q = 0 .. 7 ->
// NP rows at `slot` (a workgroup's [8][H] slot: kernel B's rows first)
template <int NP>
__device__ __forceinline__ void fold_wave_partials(const float* s, int H, int t, float* slot) {
  __syncthreads();
  for (int i = t; i < NP * H; i += kThreads) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) v += s[(size_t)q * NP * H + i];
    slot[i] = v;
  }
}

}  // namespace dsbdd
