// Third structure of the fused edge-MLP kernels (same math and arguments as
// edge_mlp.h -- see there for the algorithm and the reference citations).  This file holds the tiling, the W2^T stream
// and the column ownership of the default kernel and of its quarter items; the parts it shares with edge_splitk.h and
// edge_wave16.h -- first-layer activation, edge prefetch, gate, segmented sums, translation -- are in edge_parts.h.
//
// What the hardware counters said about the LDS-tiled kernel (rocprofv3 --pmc,
// profiles/): matrix pipe 52 % busy; every wave parked 28 % of its time at
// barriers / waitcnt and issuing ~5 VALU + 2 LDS instructions per MFMA, most of
// it to move the *A operand* (gather -> SiLU -> transposed LDS write -> LDS read)
// and the tile metadata through LDS, with a workgroup barrier every 32 MFMAs.
//
// Here the MFMA A-operand layout is used the other way round:
//
//   * one wave owns 32 edges x ALL H features.  v_mfma_f32_32x32x2_f32 wants lane l
//     to supply A[i = l & 31][k = l >> 5]: so lane l simply *is* edge (l & 31); it
//     keeps that edge's P/Q row pointers, |d|^2, d0 and type in registers, loads
//     float4 chunks of its own P and Q rows straight from L2 and evaluates
//     a = SiLU(P + Q + d*wd + d0*wd0 + tab) in registers.  Half-wave h takes
//     k in {8g + 4h .. 8g + 4h + 3} of every group of 8 (any k pairing is legal as
//     long as B uses the same one).  No LDS, no transpose, no barrier for A.
//   * only W2^T goes through LDS (K slices of 32, double buffered, a continuous
//     stream across tiles): one workgroup barrier per 128 MFMAs per wave.  The slices
//     travel global -> staging registers -> LDS, a quarter per MFMA group (an LDS-DMA
//     stream makes the compiler drain it in front of every LDS read, see below).
//   * the epilogue is wave-private: attention dot as a reduce-scatter over each
//     half-wave (v_permlane16_swap + DPP; a half-wave holds complete rows), one
//     sigmoid per row, accumulators scaled in place; segmented row sums: every half
//     adds up its rows of the running segment (even / odd rows in the two words of a
//     register pair), the halves meet through v_permlane32_swap when a segment ends;
//     one plain store per (row segment, feature) following the aggregation protocol
//     of edge_mlp.h (no atomics).
//   * vector arithmetic is written on two-element vectors (v_pk_*_f32): beside an
//     fp32 MFMA stream no vector instruction is free (tools/mfma_shadow.hip).
//   * a stage that walks two edge lists (block 0 of a framed call) runs them in one
//     launch: the second list's tiles follow the first's (EdgeArgs::*_b).
//   * tiles are assigned round-robin inside each XCD's contiguous tile range.
//
// Structures that were built, measured and dropped -- a per-XCD work queue for the tiles, the W2^T stream by LDS-DMA
// (global_load_lds), scheduling fences / a one-step-ahead activation pipeline in the emulated path, the in-kernel
// timestamp / phase-clock / "no X" diagnostic builds -- live in tools/edge_wave_diag.h (the round-5 state of this file,
// used by the micro-benchmarks' A/B builds); their numbers are in profiles/README.md and DESIGN.md.
//
// Workgroup = 4 waves = 128 edges; LDS = 2 x 32 x H x 4 B (64 KB at H = 256) +
// vectors -> 2 workgroups per CU, which overlap each other's epilogues.
#pragma once
#include "common.h"
#include "edge_mlp.h"
#include "edge_parts.h"

namespace dsbdd {

// EMU = 0: exact fp32 (v_mfma_f32_32x32x2_f32).  EMU = 6 / 9: fp32 EMULATED on the bf16 matrix cores -- both operands of
// the H x H layer split into three bf16 terms (x = hi + mid + lo exactly), 6 (or all 9) partial products per k step on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulators; see "emulated path" below.
template <int H, int MODE, int EMU = 0>
struct WaveLayout {
  static constexpr int BK = EMU ? 16 : 32;
  // emulated path: a K slice holds the three bf16 planes of 16 k x H columns = 96 H bytes = 24 H floats
  static constexpr int B_BUF = EMU ? 24 * H : BK * H;
  static constexpr int NV = (MODE == MODE_GCL) ? 1 : 2;
  static constexpr int VEC_PER = 7 * H;
  // the per-MLP vectors come first: every in-loop read of them is then `base register + 16-bit immediate`
  // (behind the 64 KB of W2^T slices each read needed its own v_add)
  static constexpr int VEC_OFF = 0;
  static constexpr int SCR_OFF = VEC_OFF + NV * VEC_PER;
  static constexpr int SCR_PER = 32 * 3;                   // per wave: trans[32][3]; phi[32] uses the same words earlier
  static constexpr int B_OFF = (SCR_OFF + 4 * SCR_PER + 4 + 255) / 256 * 256;   // [2][BK][H], 1 KB aligned
  static constexpr int TOTAL = B_OFF + 2 * B_BUF;
};

// ---- emulated path (EMU = 6 / 9): fp32 on the bf16 matrix cores ------------------------------------------------------
// The fp32 MFMA runs at 1/16 of the bf16 MFMA rate on gfx950 (MI355X_MICROARCH.md), and it runs ON the vector ALUs.  The
// H x H layer  z2 = a1 W2^T  is therefore also available as
//     a1 = a_hi + a_mid + a_lo,   W2^T = b_hi + b_mid + b_lo     (bf16 terms, round-to-nearest splits: EXACT, 3 x 8 bits)
//     z2 ~= sum over k of  a_hi b_hi + a_hi b_mid + a_mid b_hi + a_hi b_lo + a_mid b_mid + a_lo b_hi   [+ the 3 terms <= 2^-24 |a||b|]
// every bf16 x bf16 product exact in fp32, accumulated in the fp32 accumulators of v_mfma_f32_32x32x16_bf16: 6 MFMAs of
// 32 cycles per 16 k instead of 8 MFMAs of 64 cycles -- 2.7 x less matrix time, and the vector ALUs are free beside it.
// Error (tools/emu_error_study.py, profiles/r5_emu_error.md): not larger than the exact fp32 chain's own rounding error
// (one rounding per 16-k partial sum instead of one per k).  Lane l of the MFMA supplies A[l & 31][8 (l >> 5) + i] as a
// bf16x8: the lane still IS edge l & 31 and evaluates its 8 activations of the k step from 32-byte chunks of its P / Q
// rows.  B: the three planes of W2^T are split ONCE (pack_w2e_kernel) into the MFMA's own operand layout
//     W2E[k step][column tile c][plane][lane l][i] = plane(W2T[16 ks + 8 (l >> 5) + i][32 c + (l & 31)]),
// a K slice (96 H bytes) is copied to LDS as it lies, and a lane's operand of (c, plane) is ONE ds_read_b128 at
// `lane base + immediate` -- 1 KiB contiguous per wave and read, conflict-free.  Same tile walk, same epilogue, same
// aggregation protocol as the exact path; results differ from it in rounding only (both are <= 1e-4 from the oracle).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf16_rne_f(float x) {     // nearest bf16 (ties to even) as a float; finite inputs
  unsigned u = __float_as_uint(x);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return __uint_as_float(u & 0xFFFF0000u);
}

// one thread per (k step, column tile, lane, i): the three bf16 planes of W2T[k][col] in the MFMA B-operand layout
__global__ __launch_bounds__(256) void pack_w2e_kernel(const float* __restrict__ W2T, unsigned short* __restrict__ out, int H) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= H * H) return;
  const int CT = H / 32;
  const int i = idx & 7, l = (idx >> 3) & 63, c = (idx >> 9) % CT, ks = (idx >> 9) / CT;
  const int k = 16 * ks + 8 * (l >> 5) + i, col = 32 * c + (l & 31);
  const float w = W2T[(size_t)k * H + col];
  const float hi = bf16_rne_f(w), r1 = w - hi, mid = bf16_rne_f(r1), lo = bf16_rne_f(r1 - mid);
  const size_t base = (((size_t)(ks * CT + c) * 3) * 64 + l) * 8 + i;
  out[base] = (unsigned short)(__float_as_uint(hi) >> 16);
  out[base + 512] = (unsigned short)(__float_as_uint(mid) >> 16);
  out[base + 1024] = (unsigned short)(__float_as_uint(lo) >> 16);
}

// ---- quarter items (exact message kernels, H = 256, lane-grouped B copy) ---------------------------------------------
// A launch costs the slowest CU's stack of whole 128-edge items, so the tiles of its last, partly filled round run as
// QUARTER items instead: one 32-edge wave tile evaluated by all four waves of a workgroup, wave w owning the accumulator
// tiles {2w, 2w + 1} of the eight.  Every output element keeps its fmaf chain over k and every sum its operands and
// order, so the result is the whole item's bit for bit:
//   * every wave evaluates the A operand of all k for the tile's 32 edges (the same function; the redundancy is
//     paid on these tiles only), the W2^T slices stream through LDS as in the main loop, a wave reads only its columns;
//   * the attention logit is ONE fma chain over the accumulator tiles c = 0 .. 7 per lane: wave w continues the chain
//     that wave w - 1 left in LDS (16 floats per lane, three hand-offs, a workgroup barrier each), wave 3 reduces, takes
//     the sigmoids and the gates go back to all waves through LDS;
//   * the segmented row sums are the main loop's function (segmented_row_sums, edge_parts.h) on the wave's two tiles: at a
//     flush the halves exchange the same two partial sums (half 0 ends with tile 2w, half 1 with tile 2w + 1) and store
//     them to the same address;
//   * the shell instantiation's message store writes the wave's columns of the same rows.
// Item u of the workgroup's share is wave tile (u & 3) of 128-edge tile tile0 + (u >> 2); u = u0, u0 + ustep, ... < nq.
// The second half of the W2^T double buffer carries the hand-off: nobody reads it between the last K step's barrier
// and the first K step of the next item.
template <int H, bool MSG>
__device__ __forceinline__ void edge_quarter_items(const EdgeArgs& p, float* smem, int u0, int ustep, int nq, int tile0,
                                                   int nt_a, int E, int E_b, float att_b, float inv_norm) {
  using L = WaveLayout<H, MODE_GCL, 0>;
  constexpr int BK = L::BK, NK = H / BK, CT = H / 32, BMW = 32, BMB = 128;
  constexpr int BI = BK * (H / 4) / kThreads;            // float4 units of a W2^T slice per thread
  static_assert(CT == 8 && NK % 2 == 0, "quarter items: H = 256");
  float* sB = smem + L::B_OFF;
  const float* vq = smem + L::VEC_OFF;
  float* s_hand = sB + L::B_BUF;                          // [4][64 lanes] float4: the attention chain between two waves
  float* s_gate = s_hand + 16 * 64;                       // [2 halves][16]
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int half = lane >> 5, j = lane & 31;
  const int swb = (j >> 3) & 1;                           // this lane reads its halves swapped (see the kernel)
  const int c0 = 2 * w;                                   // accumulator tiles c0, c0 + 1 of the whole item's eight
  const int feat0 = ((c0 ^ (4 * swb)) * 32) + j, feat1 = feat0 + 32;
  // word of accumulator tile c0 in the lane's group of CT: tiles 0..3 at [4 swb, +4), tiles 4..7 at [4 - 4 swb, +4)
  const int boff = j * CT + (w < 2 ? 4 * swb + c0 : 4 - 4 * swb + (c0 - 4));
  const float* W2 = p.mlp[0].W2TP;

  const auto feat_of = [&](int c) { return c ? feat1 : feat0; };
#pragma unroll 1
  for (int u = u0; u < nq; u += ustep) {
    const int tile = tile0 + (u >> 2), sub = u & 3;
    const bool lb = tile >= nt_a;                         // a tile of the second list
    const int tl = lb ? tile - nt_a : tile, El = lb ? E_b : E;
    const int e0 = tl * BMB + sub * BMW;
    if (e0 >= El) continue;                               // a wave tile behind the list's end: nothing to write
    EdgeCursor eg;
    eg.request(lb ? p.erow_b : p.erow, lb ? p.ecol_b : p.ecol, lb ? p.ed0_b : p.ed0, e0, e0 + j, El,
               (lb ? p.wt_base_b : p.wt_base) + tl * 4 + sub, lb);
    // first W2^T slice
    {
      f32x4 s0[BI];
#pragma unroll
      for (int i = 0; i < BI; ++i) s0[i] = ldv4(W2 + kThreads * 4 * i + t * 4);
#pragma unroll
      for (int i = 0; i < BI; ++i) *reinterpret_cast<f32x4*>(sB + kThreads * 4 * i + t * 4) = s0[i];
    }
    eg.resolve(p);
    eg.commit(p);
    const float* Pp = p.mlp[0].P + (size_t)(eg.my_r < 0 ? 0 : eg.my_r) * p.ldpq + 4 * half;
    const float* Qp = p.mlp[0].Q + (size_t)eg.my_c * p.ldpq + 4 * half;
    f32x4 pc = ldv4(Pp), qc = ldv4(Qp), pn = pc, qn4 = qc;
    f32x16 acc[2];
    __syncthreads();          // sV + slice 0 visible
    {
      const float b0 = vq[5 * H + feat0], b1 = vq[5 * H + feat1];
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[0][r] = b0; acc[1][r] = b1; }
    }
    const f32x2 dd = splat2(eg.my_d), dz = splat2(eg.my_d0);

#pragma unroll 1
    for (int kt = 0; kt < NK; ++kt) {
      const bool more = kt + 1 < NK;
      f32x4 stg[BI];
      if (more) {
        const float* src = W2 + (size_t)(kt + 1) * BK * H + t * 4;
#pragma unroll
        for (int i = 0; i < BI; ++i) stg[i] = ldv4(src + kThreads * 4 * i);
      }
      const float* bcur = sB + (kt & 1) * L::B_BUF + (4 * half) * H + boff;
      const float* vk = vq + kt * BK + 4 * half;           // this lane's k = kt*BK + 8g + 4*half + i
      const float* vt = vk + (2 + eg.my_ty) * H;
#pragma unroll
      for (int g = 0; g < BK / 8; ++g) {
        const int kb = kt * BK + 8 * g;
        if (g + 1 < BK / 8 || more) {
          pn = ldv4(Pp + kb + 8);
          qn4 = ldv4(Qp + kb + 8);
        }
        const f32x4 a = first_layer_act4<H>(pc, qc, dd, dz, vk, vt, 8 * g);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x2 bv = *reinterpret_cast<const f32x2*>(bcur + (8 * g + i) * H);
          acc[0] = mfma32(a[i], bv.x, acc[0]);
          acc[1] = mfma32(a[i], bv.y, acc[1]);
        }
        __builtin_amdgcn_s_setprio(0);
        pc = pn; qc = qn4;
      }
      if (more) {
        float* dst = sB + ((kt + 1) & 1) * L::B_BUF + t * 4;
#pragma unroll
        for (int i = 0; i < BI; ++i) *reinterpret_cast<f32x4*>(dst + kThreads * 4 * i) = stg[i];
      }
      __syncthreads();
    }

    // ---- epilogue: the main loop's, for accumulator tiles c0 and c0 + 1 ----
    silu_tile(acc[0]);
    silu_tile(acc[1]);
    if (p.attention) {
      float part[16];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (w == s) {                                      // (wave-uniform; the barrier below is outside)
          f32x2 part2[8];
          if (s == 0) {
#pragma unroll
            for (int r = 0; r < 8; ++r) part2[r] = splat2(0.f);
          } else {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
              const f32x4 h4 = *reinterpret_cast<const f32x4*>(s_hand + (q4 * 64 + lane) * 4);
              part2[2 * q4] = h4.xy; part2[2 * q4 + 1] = h4.zw;
            }
          }
          att_accumulate(acc[0], vq[6 * H + feat0], part2);
          att_accumulate(acc[1], vq[6 * H + feat1], part2);
          if (s < 3) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
              f32x4 h4;
              h4.xy = part2[2 * q4]; h4.zw = part2[2 * q4 + 1];
              *reinterpret_cast<f32x4*>(s_hand + (q4 * 64 + lane) * 4) = h4;
            }
          } else {
#pragma unroll
            for (int r = 0; r < 8; ++r) { part[2 * r] = part2[r].x; part[2 * r + 1] = part2[r].y; }
            s_gate[16 * half + (j >> 1)] = sigmoidf_fast(reduce16_half_wave(part, j) + att_b);
          }
        }
        __syncthreads();
      }
      gates_from_lds(s_gate, half, part);
      scale_tile(acc[0], part);
      scale_tile(acc[1], part);
    }
    if constexpr (MSG) {
      if (!lb && eg.my_wt < p.msg_tiles) {                 // (wt_base == 0: the list starts at slot 0)
        float* mb = p.msg_out + (size_t)e0 * H + (4 * half) * H;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 8 * (r >> 2) + 4 * half + (r & 3);
          if (e0 + row < E) {
            mb[(8 * (r >> 2) + (r & 3)) * H + feat0] = acc[0][r];
            mb[(8 * (r >> 2) + (r & 3)) * H + feat1] = acc[1][r];
          }
        }
      }
    }
    // half 0 ends with tile c0, half 1 with tile c0 + 1
    segmented_row_sums<H, 2>(acc, p, eg, half, feat_of, inv_norm);
  }
}

template <int H, int MODE, bool BPERM, int EMU = 0, bool STORE = false, bool MSG = false>
__global__ __launch_bounds__(kThreads, 2) void edge_wave_kernel(EdgeArgs p) {
  using L = WaveLayout<H, MODE, EMU>;
  static_assert(!STORE || (!BPERM && EMU == 0), "z2 is stored by the plain exact kernels only");
  static_assert(!MSG || (MODE == MODE_GCL && EMU == 0 && !STORE), "messages are kept by the exact message kernel only");
  constexpr int BK = L::BK;
  constexpr int CT = H / 32;            // 32-col MFMA tiles per wave (all features)
  constexpr int NK = H / BK;            // K slices per unit
  constexpr int NQ = H / 4;
  // staging units of a W2^T slice per thread: float4 (exact path; emulated path when the 96 H bytes of a slice split
  // evenly), else float2
  constexpr int UNIT = EMU ? (((6 * H) % kThreads == 0) ? 4 : 2) : 4;      // floats per unit
  constexpr int BI = EMU ? (24 * H) / (kThreads * UNIT) : BK * NQ / kThreads;
  constexpr int NG = EMU ? CT / 2 : BK / 8;                                // groups of a K step (staging cadence)
  constexpr int BMW = 32, BMB = 128;    // edges per wave / per workgroup
  static_assert(H % 64 == 0 && H <= 256, "hidden_nf must be 64,128,192 or 256");
  static_assert(EMU || (BK * NQ) % kThreads == 0, "B slice split");
  static_assert(!EMU || (24 * H) % (kThreads * UNIT) == 0, "emulated B slice split");
  static_assert(EMU == 0 || EMU == 6 || EMU == 9, "partial products of the emulated path");
  static_assert(!EMU || !BPERM, "the emulated path has its own B layout");
  // s_setprio 1 around every MFMA cluster: the two workgroups sharing a CU are in different
  // phases, so favouring the wave that has MFMAs ready keeps the matrix pipe fed (+2.7 %)
  constexpr bool SETPRIO = true;
  // B operand from the lane-grouped W2^T copy (EdgeMlpW::W2TP): lane j finds the values of all its
  // column tiles in CT consecutive words -> one (CT = 4) or two (CT = 8) ds_read_b128 per k step
  // instead of CT/2 ds_read2_b32.  For CT = 8 the two 16-byte halves are read in swapped order by
  // the lanes with bit 3 set, which spreads a ds_read_b128 lane group over all 16 slots of the
  // 256-byte bank row; accumulator tile c of such a lane then holds feature tile c ^ 4.
  static_assert(!BPERM || CT == 8 || CT == 4, "lane-grouped B reads need 4 or 8 column tiles");
  constexpr bool bperm = BPERM;

  __shared__ __attribute__((aligned(1024))) float smem[L::TOTAL];
  float* sB = smem + L::B_OFF;              // [2][BK][H]
  float* sV = smem + L::VEC_OFF;            // per MLP: wd, wd0, tab0..2, b2, w-out
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int half = lane >> 5, j = lane & 31;
  float* s_phi = smem + L::SCR_OFF + w * L::SCR_PER;   // [32]
  float* s_tr = s_phi;                                  // [32][3] (phi is consumed before trans is written)
  const bool split = MODE == MODE_COORD && p.pass_split && p.n_mlp == 2;
  const int qsel = split ? ((blockIdx.x >> 3) & 1) : 0;   // the MLP this workgroup evaluates when split
  const int n_pass = (MODE == MODE_GCL || split) ? 1 : p.n_mlp;

  for (int q = 0; q < n_pass; ++q) {
    const EdgeMlpW& mw = p.mlp[qsel + q];
    // per MLP: wd, wd0, tab0..2, b2, w-out.  Written out in each kernel on purpose: as a call to a shared function the
    // compiler orders the prologue another way, and every launch waits for its prologue (profiles/edge_parts.md)
    float* v = sV + q * L::VEC_PER;
    for (int i = t; i < H; i += kThreads) {
      v[i] = mw.wd[i];
      v[H + i] = mw.wd0[i];
      v[2 * H + i] = mw.table[i];
      v[3 * H + i] = mw.table[H + i];
      v[4 * H + i] = mw.table[2 * H + i];
      v[5 * H + i] = mw.b2[i];
      v[6 * H + i] = (MODE == MODE_GCL) ? (p.attention ? p.att_w[i] : 0.f) : p.w3[i];
    }
  }
  const float att_b = (MODE == MODE_GCL && p.attention) ? p.att_b[0] : 0.f;
  const float inv_norm = 1.0f / p.norm_factor;

  const int swb = (bperm && CT == 8) ? ((j >> 3) & 1) : 0;          // this lane reads its halves swapped
  auto feat = [&](int c) { return ((c ^ (4 * swb)) * 32) + j; };    // feature held by accumulator tile c

  const int E = min(*p.e_count, p.e_cap);
  const int nt_a = (E + BMB - 1) / BMB;
  const int E_b = (MODE == MODE_GCL && p.e_count_b) ? min(*p.e_count_b, p.e_cap_b) : 0;   // second list of the stage
  const int ntiles = nt_a + (E_b + BMB - 1) / BMB;
  const int xcd = blockIdx.x & 7;
  const int kx = split ? (blockIdx.x >> 4) : (blockIdx.x >> 3);
  const int gx = split ? (gridDim.x >> 4) : (gridDim.x >> 3);
  int cbase, csize_all;
  xcd_range(ntiles, xcd, cbase, csize_all);
  // Quarter items (edge_quarter_items above): the last `nsplit` tiles of the XCD's range run as 4 quarter items each,
  // behind the whole items.  With S = the resident workgroups of an XCD (EdgeArgs::tail_s / 8) and R = the XCD's tiles
  // mod S, the tiles of the last round: R <= S/4 -> all R (one quarter item per workgroup at most, where a whole item
  // would keep one CU busy for its full length); S/2 < R <= 3S/4 -> the last R - S/2 (the first S/2 fill every CU once,
  // the quarter items go to the other workgroups first: qoff); otherwise none -- two whole items per CU are the
  // steady state.  A pure function of the tile count and the grid, the same in every workgroup of the XCD.
  constexpr bool QT = H == 256 && MODE == MODE_GCL && BPERM && EMU == 0 && !STORE;
  int nsplit = 0, qoff = 0;
  if constexpr (QT) {
    if (p.tail_s > 0) {
      const int S = max(p.tail_s >> 3, 1), R = csize_all % S;
      if (4 * R <= S) nsplit = R;
      else if (2 * R > S && 4 * R <= 3 * S) { nsplit = R - S / 2; qoff = gx >> 1; }
    }
  }
  const int csize = csize_all - nsplit;                   // whole items of the XCD
  const int nq = 4 * nsplit;
  const int qu0 = kx >= qoff ? kx - qoff : kx - qoff + gx;   // this workgroup's first quarter item
  // Static round-robin over the XCD's tiles: local tiles kx, kx + gx, ... (with two resident workgroups per CU the static
  // order keeps the (kx, kx + n_CU) pairs of a CU balanced; a work queue measured 3 % slower, see the top of the file)
  if (kx >= csize) {
    if constexpr (QT) {
      if (qu0 < nq) edge_quarter_items<H, MSG>(p, smem, qu0, gx, nq, cbase + csize, nt_a, E, E_b, att_b, inv_norm);
    }
    return;
  }


  // ---- W2^T slice stream through staging registers --------------------------------------------------------
  // The compiler orders every LDS read behind ALL pending global_load_lds (it cannot tell the slice being filled
  // from the slice being read), so a DMA burst costs each wave one exposed L2 round trip per K step.  Plain loads
  // carry no such dependence: quarter g of the next slice is requested at the top of group g and written to LDS one
  // group later (its latency sits behind the 32 MFMAs in between); nobody reads that buffer before the barrier.
  constexpr int SG = EMU ? BI : (BI + 3) / 4;              // staging registers (units) per thread (emulated path: indexed by unit, the two halves of a slice reuse them)
  typedef float stg_t __attribute__((ext_vector_type(UNIT)));
  stg_t stg[SG];
  auto stage_lo = [](int g) { return BI * g / NG; };
  auto stage_load = [&](int q, int ks, int g) {
    const char* src = EMU ? reinterpret_cast<const char*>(p.mlp[qsel + q].W2E) + (size_t)ks * (96 * H)
                          : reinterpret_cast<const char*>((bperm ? p.mlp[qsel + q].W2TP : p.mlp[qsel + q].W2T) + (size_t)ks * BK * H);
    const unsigned toff = (unsigned)t * (4u * UNIT);
#pragma unroll
    for (int i = stage_lo(g); i < stage_lo(g + 1); ++i)
      stg[EMU ? i : i - stage_lo(g)] = *reinterpret_cast<const stg_t*>(src + (size_t)(kThreads * 4 * UNIT * i) + toff);
  };
  auto stage_store = [&](int buf, int g) {
    float* dst = sB + buf * L::B_BUF + t * UNIT;
#pragma unroll
    for (int i = stage_lo(g); i < stage_lo(g + 1); ++i)
      *reinterpret_cast<stg_t*>(dst + kThreads * UNIT * i) = stg[EMU ? i : i - stage_lo(g)];
  };

  // ---- this lane's edge (current unit) and the prefetched one (next tile): requested at the first K step of a unit,
  // resolved one K step later, so that no wave waits for a global load at the top of a K step
  EdgeCursor eg;
  auto request_tile = [&](int tile) {
    const bool lb = MODE == MODE_GCL && tile >= nt_a;     // a tile of the second list (wave-uniform)
    const int tl = lb ? tile - nt_a : tile, El = lb ? E_b : E;
    const int e0 = tl * BMB + w * BMW;
    eg.request(lb ? p.erow_b : p.erow, lb ? p.ecol_b : p.ecol, lb ? p.ed0_b : p.ed0, e0, e0 + j, El,
               (lb ? p.wt_base_b : p.wt_base) + tl * 4 + w, lb);
  };

  // B values of one MFMA step: column j of every column tile (plain layout: CT 4-byte reads at stride 32) or
  // the lane-grouped copy (one or two 16-byte reads)
  auto read_b = [&](const float* brow, float (&bv)[CT]) {
    if constexpr (BPERM) {
      const float4 lo = *reinterpret_cast<const float4*>(brow);
      bv[0] = lo.x; bv[1] = lo.y; bv[2] = lo.z; bv[3] = lo.w;
      if constexpr (CT == 8) {
        const float4 hi = *reinterpret_cast<const float4*>(brow + 4 - 8 * swb);
        bv[4] = hi.x; bv[5] = hi.y; bv[6] = hi.z; bv[7] = hi.w;
      }
    } else {
#pragma unroll
      for (int c = 0; c < CT; ++c) bv[c] = brow[c * 32];
    }
  };

  // prologue: first W2^T slice, first edge, first P/Q chunk
#pragma unroll
  for (int g = 0; g < NG; ++g) { stage_load(0, 0, g); stage_store(0, g); }
  request_tile(cbase + kx);
  eg.resolve(p);
  eg.commit(p);
  __syncthreads();          // sV + slice 0 visible
  int bslice = 0;           // running slice counter (buffer = bslice & 1)

  // this lane's k of a step: exact path 8 g + 4 half + i (float4 chunks), emulated path 16 kt + 8 half + i (two float4)
  constexpr int KH = EMU ? 8 : 4;
  const float* Pp = p.mlp[qsel].P + (size_t)(eg.my_r < 0 ? 0 : eg.my_r) * p.ldpq + KH * half;
  const float* Qp = p.mlp[qsel].Q + (size_t)eg.my_c * p.ldpq + KH * half;
  f32x4 pc = ldv4(Pp), qc = ldv4(Qp), pn = pc, qn4 = qc;
  f32x4 pc1 = pc, qc1 = qc;                                // emulated path: second half of the 8-float chunk
  if constexpr (EMU != 0) { pc1 = ldv4(Pp + 4); qc1 = ldv4(Qp + 4); }
  float phi0 = 0.f, phi1 = 0.f;

  bf16x8 a_h = {}, a_m = {}, a_l = {};                     // emulated path: the current k step's activations (three bf16 planes)
  (void)a_h; (void)a_m; (void)a_l;
  int li = kx, q = 0, next_li = 0;
  bool has_next = false;
#pragma unroll 1
  for (;;) {
    const float* vq = sV + q * L::VEC_PER;
    const bool tile_ends = q == n_pass - 1;
    const int qn = tile_ends ? 0 : q + 1;                  // MLP pass of the next unit

    // the accumulators start from the second layer's bias (one fmaf chain per output starting at b2: the bias add
    // of the epilogue costs nothing)
    f32x16 acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const float bv = vq[5 * H + feat(c)];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] = bv;
    }

#pragma unroll 1
    for (int kt = 0; kt < NK; ++kt) {
      const bool more = kt + 1 < NK;
      // next tile of this workgroup: its edge with two dependent loads, all behind the MFMAs of the current tile
      const int st = q * NK + kt;
      if (st == 0) {
        next_li = li + gx;
        has_next = next_li < csize;
        if (has_next) request_tile(cbase + next_li);
      }
      if (st == 1 && has_next) eg.resolve(p);
      // the next W2^T slice: a continuous stream across units (the last K step of a workgroup re-reads slice 0 of
      // its MLP: never used; unconditional, so that the compiler counts the loads in flight exactly)
      const int sq = more ? q : qn, sks = more ? kt + 1 : 0;
      const f32x2 dd = splat2(eg.my_d), dz = splat2(eg.my_d0);
      if constexpr (EMU != 0) {
        // ---- emulated path: one 16-k step = 8 activations per lane, split into three bf16x8, 6 (9) MFMAs per column tile.
        // Order of a step: the step's activations, the next P / Q chunk requested, then per pair of column tiles the three
        // B planes (lo: 1 product, mid: 2, hi: 3) and their MFMAs; the next W2E slice travels through staging registers in
        // two halves.  (B reads one pair ahead behind scheduling fences and the next step's activations one step ahead were
        // measured neutral to slower, profiles/r5_emu_microbench.md; those builds live in tools/edge_wave_diag.h.)
        constexpr int NG1 = (NG + 1) / 2;
        auto act8 = [&](int ks, bf16x8& o_h, bf16x8& o_m, bf16x8& o_l) {       // activations of k step ks from pc / qc
          const float* vk = vq + ks * 16 + 8 * half;       // this lane's k = 16 ks + 8 half + i
          const float* vt = vk + (2 + eg.my_ty) * H;
          const f32x4 a03 = first_layer_act4<H>(pc, qc, dd, dz, vk, vt, 0), a47 = first_layer_act4<H>(pc1, qc1, dd, dz, vk, vt, 4);
          const float av[8] = {a03.x, a03.y, a03.z, a03.w, a47.x, a47.y, a47.z, a47.w};
#pragma unroll
          for (int i = 0; i < 8; ++i) {                    // exact three-way split: v_cvt_pk_bf16_f32 rounds to nearest even
            const __bf16 h1 = (__bf16)av[i];
            const float r1 = av[i] - (float)h1;
            const __bf16 m1 = (__bf16)r1;
            const float r2 = r1 - (float)m1;
            o_h[i] = h1; o_m[i] = m1; o_l[i] = (__bf16)r2;
          }
        };
        auto load_pq = [&](int ks) {                       // this lane's P / Q chunk of k step ks (32 bytes of either row)
          pc = ldv4(Pp + 16 * ks); pc1 = ldv4(Pp + 16 * ks + 4);
          qc = ldv4(Qp + 16 * ks); qc1 = ldv4(Qp + 16 * ks + 4);
        };
        act8(kt, a_h, a_m, a_l);                           // the step's activations in front of its MFMAs
        load_pq(more ? kt + 1 : 0);
#pragma unroll
        for (int g = 0; g < NG1; ++g) stage_load(sq, sks, g);
        const float* bl = sB + (bslice & 1) * L::B_BUF + lane * 4;       // + (c * 3 + plane) * 256 floats
        bf16x8 bh[2], bm[2], blo[2];
        auto rdb = [&](int cp, int plane, bf16x8 (&dst)[2]) {
#pragma unroll
          for (int u = 0; u < 2; ++u)
            dst[u] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(bl + (2 * cp + u) * 768 + plane * 256));
        };
        rdb(0, 2, blo); rdb(0, 1, bm); rdb(0, 0, bh);
#define EMU_MM(a, b) do { _Pragma("unroll") for (int u = 0; u < 2; ++u) \
          acc[2 * cp + u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[u], acc[2 * cp + u], 0, 0, 0); } while (0)
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int cp = 0; cp < CT / 2; ++cp) {
          const bool nxt = cp + 1 < CT / 2;
          if constexpr (EMU == 9) { EMU_MM(a_l, blo); EMU_MM(a_m, blo); }
          EMU_MM(a_h, blo);
          if (nxt) rdb(cp + 1, 2, blo);
          if constexpr (EMU == 9) EMU_MM(a_l, bm);
          EMU_MM(a_m, bm); EMU_MM(a_h, bm);
          if (nxt) rdb(cp + 1, 1, bm);
          EMU_MM(a_l, bh); EMU_MM(a_m, bh); EMU_MM(a_h, bh);           // (the leading product last)
          if (nxt) rdb(cp + 1, 0, bh);
          if (NG > 1 && cp == CT / 4 - 1) {                // half way: first half of the slice -> LDS, request the second
#pragma unroll
            for (int g = 0; g < NG1; ++g) stage_store((bslice + 1) & 1, g);
#pragma unroll
            for (int g = NG1; g < NG; ++g) stage_load(sq, sks, g);
          }
        }
#undef EMU_MM
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int g = (NG > 1 ? NG1 : 0); g < NG; ++g) stage_store((bslice + 1) & 1, g);
      } else {
      const float* bcur = sB + (bslice & 1) * L::B_BUF + (4 * half) * H + (bperm ? j * CT + 4 * swb : j);
      const float* vk = vq + kt * BK + 4 * half;           // this lane's k = kt*BK + 8g + 4*half + i
      const float* vt = vk + (2 + eg.my_ty) * H;
#pragma unroll
      for (int g = 0; g < BK / 8; ++g) {
        const int kb = kt * BK + 8 * g;                    // this lane's k = kb + 4*half + i
        if (g > 0) stage_store((bslice + 1) & 1, g - 1);
        stage_load(sq, sks, g);
        if (g + 1 < BK / 8 || more) {                      // prefetch the next group's P/Q chunk
          pn = ldv4(Pp + kb + 8);
          qn4 = ldv4(Qp + kb + 8);
        }
        const f32x4 a = first_layer_act4<H>(pc, qc, dd, dz, vk, vt, 8 * g);
        if (SETPRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float* brow = bcur + (8 * g + i) * H;
          float bv[CT];
          read_b(brow, bv);
#pragma unroll
          for (int c = 0; c < CT; ++c) acc[c] = mfma32(a[i], bv[c], acc[c]);
        }
        if (SETPRIO) __builtin_amdgcn_s_setprio(0);
        pc = pn; qc = qn4;
      }
      stage_store((bslice + 1) & 1, BK / 8 - 1);
      }   // exact path
      ++bslice;
      __syncthreads();
    }

    const bool last_unit = tile_ends && !has_next;
    // first P/Q chunk of the NEXT unit: in flight during the epilogue
    if (!last_unit) {
      const int r_n = tile_ends ? eg.nx_r : eg.my_r, c_n = tile_ends ? eg.nx_c : eg.my_c;
      Pp = p.mlp[qsel + qn].P + (size_t)(r_n < 0 ? 0 : r_n) * p.ldpq + KH * half;
      Qp = p.mlp[qsel + qn].Q + (size_t)c_n * p.ldpq + KH * half;
      pc = ldv4(Pp); qc = ldv4(Qp);
      if constexpr (EMU != 0) { pc1 = ldv4(Pp + 4); qc1 = ldv4(Qp + 4); }
    }

    // ================= wave-private epilogue =================
    if constexpr (STORE) {
      // training forward: z2 (bias included) of the wave tile's valid slots, 128-byte row segments per half-wave
      const int e0 = (eg.my_wt - p.wt_base) * BMW;
      float* zb = p.z2_out + (MODE == MODE_COORD ? (size_t)(qsel + q) * p.z2_stride : (size_t)0) + (size_t)e0 * H + j;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 8 * (r >> 2) + 4 * half + (r & 3);
        if (e0 + row < E) {
#pragma unroll
          for (int c = 0; c < CT; ++c) zb[(size_t)row * H + 32 * c] = acc[c][r];
        }
      }
    }
    if (MODE == MODE_GCL) {
#pragma unroll
      for (int c = 0; c < CT; ++c) silu_tile(acc[c]);
      if (p.attention) {   // att = sigmoid(w_a . m + b_a); a half-wave holds complete rows
        f32x2 part2[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) part2[r] = splat2(0.f);
#pragma unroll
        for (int c = 0; c < CT; ++c) att_accumulate(acc[c], vq[6 * H + feat(c)], part2);
        float part[16];
#pragma unroll
        for (int r = 0; r < 8; ++r) { part[2 * r] = part2[r].x; part[2 * r + 1] = part2[r].y; }
        // reduce-scatter over the half-wave: lane j ends with the dot product of accumulator register j >> 1,
        // takes ONE sigmoid, and the 16 gates of the half come back through 64 bytes of LDS (broadcast reads)
        s_phi[16 * half + (j >> 1)] = sigmoidf_fast(reduce16_half_wave(part, j) + att_b);
        wave_lds_fence();
        gates_from_lds(s_phi, half, part);
        wave_lds_fence();   // the words are rewritten by the next tile
#pragma unroll
        for (int c = 0; c < CT; ++c) scale_tile(acc[c], part);
      }
      if constexpr (MSG) {
        // shell stage of the forward cone: the ghost segment's tiles of the first list keep the gated, un-normalised
        // messages of their valid slots (128-byte row segments per half-wave, like the z2 store above); the tile index
        // is wave-uniform (wt_base == 0: the list starts at slot 0)
        const int wt = __builtin_amdgcn_readfirstlane(eg.my_wt);
        if (!eg.my_lb && wt < p.msg_tiles) {
          const int e0 = wt * BMW;
          // feat(c) = 32 c + j, with the two halves of the column tiles swapped for the lanes that read B swapped
          // (CT == 8 only): two lane bases, every other offset a compile-time constant
          float* mb = p.msg_out + (size_t)e0 * H + (4 * half) * H + j;
          float* const mlo = mb + 128 * swb;
          float* const mhi = mb - 128 * swb;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = 8 * (r >> 2) + 4 * half + (r & 3);
            if (e0 + row < E) {
#pragma unroll
              for (int c = 0; c < CT; ++c)
                (c < 4 ? mlo : mhi)[(8 * (r >> 2) + (r & 3)) * H + 32 * c] = acc[c][r];
            }
          }
        }
      }
      segmented_row_sums<H, CT>(acc, p, eg, half, feat, inv_norm);
    } else {
      // scalar head: phi = w3 . SiLU(acc)   (egnn_new.py:80-92; the bias is already in the accumulators)
      f32x2 part2[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) part2[r] = splat2(0.f);
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        const f32x2 wv = splat2(vq[6 * H + feat(c)]);
#pragma unroll
        for (int r = 0; r < 8; ++r) part2[r] = pk_fma(silu2(f32x2{acc[c][2 * r], acc[c][2 * r + 1]}), wv, part2[r]);
      }
      float part[16];
#pragma unroll
      for (int r = 0; r < 8; ++r) { part[2 * r] = part2[r].x; part[2 * r + 1] = part2[r].y; }
      // lane j of a half ends with the total of accumulator register j >> 1 = edge mfma_row(j >> 1, lane)
      s_phi[mfma_row(j >> 1, lane)] = reduce16_half_wave(part, j);
      wave_lds_fence();
      const float ph = s_phi[j];                            // this lane's edge
      wave_lds_fence();
      if (qsel + q == 0) phi0 = ph; else phi1 = ph;

      if (tile_ends) {
        // lane = edge; a split launch's workgroup adds only its own MLP's term
        float tr[3];
        edge_translation(p, eg, !(split && qsel == 1), p.n_mlp == 2 && !(split && qsel == 0), phi0, phi1, tr);
        if (half == 0) { s_tr[3 * j] = tr[0]; s_tr[3 * j + 1] = tr[1]; s_tr[3 * j + 2] = tr[2]; }
        wave_lds_fence();
        float trv[32];
#pragma unroll
        for (int e = 0; e < 32; ++e) trv[e] = s_tr[3 * e + (lane < 3 ? lane : 0)];
        const int pop = split ? qsel : 0;
        segmented_sum3<32>(trv, eg.my_r, eg.my_prev, lane, p.xagg + pop * p.xagg_stride, p.xagg_head + pop * p.xhead_stride,
                           eg.my_wt, p.norm_factor);
        wave_lds_fence();   // scratch is reused by the next tile
      }
    }

    // advance to the next unit
    if (tile_ends) {
      if (last_unit) break;
      eg.commit(p);
      li = next_li;
      q = 0;
    } else {
      ++q;
    }
  }  // units
  // this workgroup's quarter items (every wave is behind the last K step's barrier: the W2^T buffers are free)
  if constexpr (QT) {
    if (qu0 < nq) edge_quarter_items<H, MSG>(p, smem, qu0, gx, nq, cbase + csize, nt_a, E, E_b, att_b, inv_norm);
  }
}

}  // namespace dsbdd
