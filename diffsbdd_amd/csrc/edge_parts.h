// The parts that every variant of the fused edge-MLP kernels shares (edge_wave.h with its quarter items, edge_splitk.h,
// edge_wave16.h; the algorithm, the aggregation protocol and the reference citations are in edge_mlp.h).  A variant
// keeps its own tiling of the H x H layer, its W2^T stream and the rule which wave owns which columns; everything
// around that core is defined ONCE here, so that a rule of the bitwise-reproducibility contract -- which entries are
// inactive, in which order a row's messages are added, which segment goes to a head slot -- is changed in one place:
//
//   first_layer_act4      the A operand  SiLU((P + Q) + d wd + d0 wd0 + tab)  of four k
//   EdgeCursor            this lane's edge of the current tile and the prefetched edge of the next one
//   silu_tile, att_accumulate, gates_from_lds, scale_tile      messages and the attention gate
//   segmented_row_sums    per-row sums of a 32-edge tile's messages and their stores (agg / agg_head)
//   edge_translation, segmented_sum3      the coordinate stage's per-edge translation and its per-row sums (xagg / xagg_head)
//   xcd_range             the contiguous tile range of an XCD
//
// All of them are plain inline functions on the caller's registers: a 32-edge tile lives in a wave as lane = edge
// (l & 31), accumulator register rr of half-wave h = row 8 (rr >> 2) + 4 h + (rr & 3)  (mfma_row, common.h).
#pragma once
#include "common.h"
#include "edge_mlp.h"

namespace dsbdd {

__device__ __forceinline__ void wave_lds_fence() {
  // LDS operations of one wave complete in order; this only stops the compiler
  // from moving the later reads above the earlier writes.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- cross-lane helpers of the wave-private epilogue (gfx950: v_permlane{16,32}_swap, DPP) -----------------
// Lane exchanges never go through the LDS crossbar (ds_bpermute, what __shfl_xor compiles to): the two swaps move a
// whole 16- / 32-lane row between two registers in one VALU instruction, the rest are DPP operands.
__device__ __forceinline__ float dpp_xor1(float v) {   // quad_perm [1,0,3,2]
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_xor2(float v) {   // quad_perm [2,3,0,1]
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_half_mirror(float v) {   // lane i <-> 7 - i inside every group of 8
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_ror8(float v) {   // lane i <-> i ^ 8 inside every row of 16
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xF, 0xF, true));
}
// p: this lane keeps it when its row (16 lanes) is even; q: kept when odd.  Returns own kept value + the partner row's
// (lane ^ 16) value of the same register.
__device__ __forceinline__ float pair_sum_rows16(float p, float q) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(p), __float_as_uint(q), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// the same across the two 32-lane halves: half 0 gets p(own) + p(lane + 32), half 1 gets q(lane - 32) + q(own)
__device__ __forceinline__ float pair_sum_halves(float p, float q) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(p), __float_as_uint(q), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// Sum of 16 per-lane values over the 32 lanes of a half-wave as a reduce-scatter: every step halves the number of
// registers a lane carries (16 + 8 + 4 + 2 + 1 exchanges instead of 5 x 16 for a butterfly on every register).
// On return lane j of either half holds the total of register  rs_index(j) = j >> 1.
__device__ __forceinline__ float reduce16_half_wave(const float (&part)[16], int j) {
  float k8[8], k4[4], k2[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) k8[i] = pair_sum_rows16(part[i], part[i + 8]);          // lanes ^ 16: keep [8 b4, +8)
  const bool b3 = (j >> 3) & 1, b2 = (j >> 2) & 1, b1 = (j >> 1) & 1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {                                                       // lanes ^ 8: keep [.. + 4 b3, +4)
    const float send = b3 ? k8[i] : k8[i + 4], keep = b3 ? k8[i + 4] : k8[i];
    k4[i] = keep + dpp_ror8(send);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {                                                       // lane i <-> 7 - i: keep [.. + 2 b2, +2)
    const float send = b2 ? k4[i] : k4[i + 2], keep = b2 ? k4[i + 2] : k4[i];
    k2[i] = keep + dpp_half_mirror(send);
  }
  const float send = b1 ? k2[0] : k2[1], keep = b1 ? k2[1] : k2[0];                   // lanes ^ 2: keep [.. + b1]
  const float k1 = keep + dpp_xor2(send);
  return k1 + dpp_xor1(k1);                                                           // lanes ^ 1: both hold the total
}

// ---- first layer ---------------------------------------------------------------------------------------------------
// A operand of four consecutive k: SiLU((P + Q) + d wd + d0 wd0 + tab), two values per instruction (explicit fma: the
// same arithmetic in every kernel and instantiation).  pc / qc: the lane's chunks of its P / Q rows; dd / dz: |d|^2 and
// d0 of its edge; vk: the lane's first k in the kernel's per-MLP vectors (wd, wd0, tab0..2, b2, w-out), vt = vk + (2 + type) H; off: the group's k.
template <int H>
__device__ __forceinline__ f32x4 first_layer_act4(f32x4 pc, f32x4 qc, f32x2 dd, f32x2 dz, const float* vk,
                                                  const float* vt, int off) {
  const f32x4 wd4 = *reinterpret_cast<const f32x4*>(vk + off);
  const f32x4 wz4 = *reinterpret_cast<const f32x4*>(vk + H + off);
  const f32x4 tb4 = *reinterpret_cast<const f32x4*>(vt + off);
  f32x2 alo = pk_fma(dz, wz4.xy, pk_fma(dd, wd4.xy, pc.xy + qc.xy)) + tb4.xy;
  f32x2 ahi = pk_fma(dz, wz4.zw, pk_fma(dd, wd4.zw, pc.zw + qc.zw)) + tb4.zw;
  alo = silu2(alo);
  ahi = silu2(ahi);
  return f32x4{alo.x, alo.y, ahi.x, ahi.y};
}

// ---- this lane's edge (current tile) and the prefetched one (next tile) -----------------------------------------------
// request() only REQUESTS the next tile's indices; they are looked at later (resolve: range check, then the coordinates),
// so that no wave waits for a global load where it asks.  commit() makes the prefetched edge the current one.  Which
// list a tile belongs to and where its edges and its wave-tile slot are is the caller's arithmetic.
struct EdgeCursor {
  int my_r = -1, my_c = 0, my_ty = 0;
  float my_d = 0.f, my_d0 = 0.f, xr[3] = {0.f, 0.f, 0.f}, xc[3] = {0.f, 0.f, 0.f};
  int nx_r = -1, nx_c = 0;
  int my_prev = -1, nx_prev = -1;      // row of the edge just before this wave tile (wave-uniform)
  // my_wt / my_lb are what the caller handed to request(): the 32-edge kernels pass the tile's head slot and list,
  // which segmented_row_sums and the message store read.  edge_wave16.h passes 0 / false and takes its head slot from
  // its own 16-edge tile index: there these two members mean nothing and segmented_row_sums must not be called.
  int my_wt = 0, nx_wt = 0;            // global wave-tile index
  bool my_lb = false, nx_lb = false;   // the tile belongs to the stage's second list
  float nx_d0 = 0.f, nxr[3] = {0.f, 0.f, 0.f}, nxc[3] = {0.f, 0.f, 0.f};
  int vzero;                           // 0 in a vector register the compiler cannot see through
  __device__ __forceinline__ EdgeCursor() { asm volatile("v_mov_b32 %0, 0" : "=v"(vzero)); }

  // edges [e0, ..) of a list of El entries (er, ec, ed), this lane's is e; wt / lb: the tile's head slot and list
  __device__ __forceinline__ void request(const int* er, const int* ec, const float* ed, int e0, int e, int El, int wt,
                                          bool lb) {
    nx_r = -1; nx_c = 0; nx_d0 = 0.f; nx_prev = -1; nx_wt = wt; nx_lb = lb;
    if (e < El) { nx_r = er[e]; nx_c = ec[e]; nx_d0 = ed[e]; }
    if (e0 > 0 && e0 < El) nx_prev = er[e0 - 1 + vzero];   // (a per-lane load: nothing waits for it here)
  }
  __device__ __forceinline__ void resolve(const EdgeArgs& p) {
    // entries that do not name two rows of this call (stale workspace words after an overflowed build) are inactive
    if ((unsigned)nx_r >= (unsigned)p.n_nodes || (unsigned)nx_c >= (unsigned)p.n_nodes) { nx_r = -1; nx_c = 0; }
    if (nx_r >= 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { nxr[k] = p.x[3 * nx_r + k]; nxc[k] = p.x[3 * nx_c + k]; }
    }
  }
  __device__ __forceinline__ void commit(const EdgeArgs& p) {
    my_r = nx_r; my_c = nx_c; my_d0 = nx_d0; my_d = 0.f; my_ty = 0;
    my_prev = nx_prev; my_wt = nx_wt; my_lb = nx_lb;
#pragma unroll
    for (int k = 0; k < 3; ++k) { xr[k] = nxr[k]; xc[k] = nxc[k]; }
    if (my_r >= 0) {
      const float dx = xr[0] - xc[0], dy = xr[1] - xc[1], dz = xr[2] - xc[2];
      my_d = dx * dx + dy * dy + dz * dz;                  // coord2diff radial, egnn_new.py:298-299
      const bool rl = my_r < p.n_lig, cl = my_c < p.n_lig;
      my_ty = (rl && cl) ? 1 : ((!rl && !cl) ? 2 : 0);     // dynamics.py:119-124
    }
  }
};

// ---- messages and the attention gate on 32 x 32 accumulator tiles ------------------------------------------------------
// m = SiLU(acc)   (egnn_new.py:18-19; the bias is already in the accumulators), register pairs
__device__ __forceinline__ void silu_tile(f32x16& acc) {
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const f32x2 m2 = silu2(f32x2{acc[r], acc[r + 1]});
    acc[r] = m2.x; acc[r + 1] = m2.y;
  }
}
// att = sigmoid(w_a . m + b_a): one fma chain per row over the column tiles, in the order the caller enters them
__device__ __forceinline__ void att_accumulate(const f32x16& acc, float aw, f32x2 (&part2)[8]) {
  const f32x2 aw2 = splat2(aw);
#pragma unroll
  for (int r = 0; r < 8; ++r) part2[r] = pk_fma(f32x2{acc[2 * r], acc[2 * r + 1]}, aw2, part2[r]);
}
// reduce16_half_wave leaves the dot product of register j >> 1 in lane j, which takes ONE sigmoid and writes the gate
// to s[16 half + (j >> 1)]; the 16 gates of the half come back through 64 bytes of LDS (broadcast reads)
__device__ __forceinline__ void gates_from_lds(const float* s, int half, float (&part)[16]) {
#pragma unroll
  for (int q4 = 0; q4 < 4; ++q4) {
    const float4 g4 = *reinterpret_cast<const float4*>(s + 16 * half + 4 * q4);
    part[4 * q4] = g4.x; part[4 * q4 + 1] = g4.y; part[4 * q4 + 2] = g4.z; part[4 * q4 + 3] = g4.w;
  }
}
__device__ __forceinline__ void scale_tile(f32x16& acc, const float (&part)[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] *= part[r];          // mij * att, egnn_new.py:40
}

// ---- segmented sums over a tile's 32 rows, NT column tiles -----------------------------------------------------------------
// Accumulator register rr of half h is row 8*(rr>>2) + 4*h + (rr&3): the rows alternate between the halves in groups of
// 4.  Every half adds up ITS rows of the running segment in edge order; when the segment ends (row ids are wave-uniform
// scalars: a scalar branch) the two halves' partial sums are added (half 0's + half 1's) and half h receives and stores
// tile c + h NT/2 -- a fixed order that depends on the tile's edges only.
// Aggregation protocol (edge_mlp.h): the first segment of the tile goes to the tile's head slot when its row continues
// from the previous wave tile (agg_head[wt]), every other segment is the start of its row and goes to agg[row], either
// of the tile's list; plain stores, each address written by exactly one wave.  feat_of(c) is the feature of tile c.
// Even and odd rows of a half run in separate sums (the two words of a register pair) that meet at the flush: written
// as sum[c] += acc[c][r] the compiler pairs the adds ACROSS column tiles, whose accumulators are 16 registers apart --
// two v_mov per packed add.  aggregate / normalization_factor (egnn_new.py:328-329) is one multiply per flushed segment
// (<= 1 ulp from the reference's division).
template <int H, int NT, class FeatOf>
__device__ __forceinline__ void segmented_row_sums(const f32x16* acc, const EdgeArgs& p, const EdgeCursor& eg, int half,
                                                   FeatOf feat_of, float inv_norm) {
  static_assert(NT % 2 == 0, "column tiles are exchanged in pairs");
  const int my_r = eg.my_r;
  f32x2 sum2[NT];
#pragma unroll
  for (int c = 0; c < NT; ++c) sum2[c] = splat2(0.f);
  int cur = -1;
  const int row0 = __builtin_amdgcn_readlane(my_r, 0);
  bool to_head = row0 >= 0 && row0 == __builtin_amdgcn_readfirstlane(eg.my_prev);
  auto flush = [&]() {
    if (cur >= 0) {
      float* dst = to_head ? (eg.my_lb ? p.agg_head_b : p.agg_head) + (size_t)eg.my_wt * H
                           : (eg.my_lb ? p.agg_b : p.agg) + (size_t)cur * H;
#pragma unroll
      for (int c = 0; c < NT / 2; ++c) {
        const float tot = pair_sum_halves(sum2[c].x + sum2[c].y, sum2[c + NT / 2].x + sum2[c + NT / 2].y);
        dst[feat_of(c + half * (NT / 2))] = tot * inv_norm;
      }
      to_head = false;
    }
#pragma unroll
    for (int c = 0; c < NT; ++c) sum2[c] = splat2(0.f);
  };
#pragma unroll
  for (int gb = 0; gb < 8; ++gb) {
    const int hh = gb & 1;
#pragma unroll
    for (int ip = 0; ip < 4; ip += 2) {
      const int k = 4 * (gb >> 1) + ip;
      const int rn0 = __builtin_amdgcn_readlane(my_r, 4 * gb + ip);
      const int rn1 = __builtin_amdgcn_readlane(my_r, 4 * gb + ip + 1);
      if (rn0 != cur) {                                // scalar compare / branch
        flush();
        cur = rn0;
      }
      if (half == hh) {
#pragma unroll
        for (int c = 0; c < NT; ++c) sum2[c].x += acc[c][k];
      }
      if (rn1 != rn0) {
        flush();
        cur = rn1;
      }
      if (half == hh) {
#pragma unroll
        for (int c = 0; c < NT; ++c) sum2[c].y += acc[c][k + 1];
      }
    }
  }
  flush();
}

// ---- coordinate stage ------------------------------------------------------------------------------------------------
// trans = u*phi + cross*phi_x   (egnn_new.py:100-109, 296-316) of this lane's edge: the radial term (phi), the
// cross-product term (phi_x) or both, as the caller evaluates one MLP or both; an inactive edge moves nothing
__device__ __forceinline__ void edge_translation(const EdgeArgs& p, const EdgeCursor& eg, bool radial, bool cross,
                                                 float phi, float phi_x, float (&tr)[3]) {
  float tx = 0.f, ty = 0.f, tz = 0.f;
  if (eg.my_r >= 0) {
    const float* xr = eg.xr;
    const float* xc = eg.xc;
    if (radial) {
      const float dx = xr[0] - xc[0], dy = xr[1] - xc[1], dz = xr[2] - xc[2];
      const float den = sqrtf(eg.my_d + 1e-8f) + p.norm_constant;
      const float ux = dx / den, uy = dy / den, uz = dz / den;
      if (p.use_tanh) {
        const float th = tanhf(phi);
        tx = ux * th * p.coords_range; ty = uy * th * p.coords_range; tz = uz * th * p.coords_range;
      } else {
        tx = ux * phi; ty = uy * phi; tz = uz * phi;
      }
    }
    if (cross) {
      const int b = p.node_batch[eg.my_r];
      const float m0 = p.mean[3 * b], m1 = p.mean[3 * b + 1], m2 = p.mean[3 * b + 2];
      const float a0 = xr[0] - m0, a1 = xr[1] - m1, a2 = xr[2] - m2;
      const float b0 = xc[0] - m0, b1 = xc[1] - m1, b2 = xc[2] - m2;
      const float c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
      const float cden = sqrtf(c0 * c0 + c1 * c1 + c2 * c2) + p.norm_constant;
      float phx = phi_x;
      if (p.use_tanh) phx = tanhf(phx) * p.coords_range;
      tx += c0 / cden * phx; ty += c1 / cden * phx; tz += c2 / cden * phx;
    }
  }
  tr[0] = tx; tr[1] = ty; tr[2] = tz;
}

// Per-row sums of the translations of a tile's NE edges, lane c < 3 walks component c (trv: its NE values, in registers
// before the walk: read inside it, every step sat out an LDS round trip).  The aggregation protocol of the row sums
// above with xa[row][3] and the head slots xh[wt][4]; the reference's division is kept here.
template <int NE>
__device__ __forceinline__ void segmented_sum3(const float (&trv)[NE], int my_r, int my_prev, int lane, float* xa,
                                               float* xh, int wt, float norm_factor) {
  if (lane < 3) {
    const int row0 = __builtin_amdgcn_readlane(my_r, 0);
    bool to_head = row0 >= 0 && row0 == __builtin_amdgcn_readfirstlane(my_prev);
    int cur = -1;
    float sum = 0.f;
    auto put = [&]() {
      if (cur >= 0) {
        const float v = sum / norm_factor;
        if (to_head) xh[4 * (size_t)wt + lane] = v; else xa[(size_t)cur * 3 + lane] = v;
        to_head = false;
      }
    };
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int rn = __builtin_amdgcn_readlane(my_r, e);
      if (rn != cur) {
        put();
        cur = rn;
        sum = 0.f;
      }
      sum += trv[e];
    }
    put();
  }
}

// Tiles are dealt to the eight XCDs as contiguous ranges, the first ntiles % 8 of them one tile longer
__device__ __forceinline__ void xcd_range(int ntiles, int xcd, int& cbase, int& csize) {
  const int tq = ntiles / 8, tr = ntiles % 8;
  csize = tq + (xcd < tr ? 1 : 0);
  cbase = (xcd < tr) ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
}

}  // namespace dsbdd
