// The parts that the graph and geometry kernels share (radius_graph.h, level_list.h, geometry.h; ddpm.h, loss_parts.h,
// loss_head.h, score.h and train.h take single pieces): the constants of the edge-list layout, the integer wave / workgroup scans,
// the three-component workgroup reduction with the per-sample mean built on it, a sample's row ranges, the pad fill
// of a list segment and the zero fill.  One definition each: "the same bits" and "the same layout" hold by
// construction at every site.
#pragma once
#include "common.h"

namespace dsbdd {

constexpr int kTileCtrInts = 32;   // 16 queue heads (8 XCDs x 2 MLP populations) + completion count
constexpr int kEdgeAlign = 32;     // edges of one (sample, node set) start at a multiple of a wave tile
constexpr int kLevels = 5;         // hop levels of the level-ordered edge list: 0 ligand, 1..3, 4 = farther
constexpr int kShellLists = 2;     // shell lists of the forward cone: rows of level 2 and of level 3 (the exact levels past 1)

// v rounded up to the next wave-tile boundary of the edge list
__host__ __device__ __forceinline__ int align_edges(int v) { return (v + kEdgeAlign - 1) & ~(kEdgeAlign - 1); }

// first index of the sorted a[0..n) whose entry is >= v (I: int64_t or long long, whichever the caller's masks are)
template <class I>
__device__ __forceinline__ int lower_bound_i64(const I* a, int n, long long v) {
  static_assert(sizeof(I) == 8, "64-bit masks");
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Row ranges of sample b: ligand rows [l0, l1), pocket rows [p0, p1).
struct SampleRows {
  int l0, l1, p0, p1;
  __device__ __forceinline__ int count() const { return max((l1 - l0) + (p1 - p0), 1); }   // nodes, clamped for a mean
};
// from the sorted batch masks; pocket rows numbered within the pocket array
__device__ __forceinline__ SampleRows sample_rows(const int64_t* mask_lig, int n_lig, const int64_t* mask_poc,
                                                  int n_poc, int b) {
  return SampleRows{lower_bound_i64(mask_lig, n_lig, b), lower_bound_i64(mask_lig, n_lig, b + 1),
                    lower_bound_i64(mask_poc, n_poc, b), lower_bound_i64(mask_poc, n_poc, b + 1)};
}
// from the offsets that prep_kernel made of them; pocket rows in the [ligand | pocket] node numbering
__device__ __forceinline__ SampleRows sample_rows(const int* lig_off, const int* poc_off, int n_lig, int b) {
  return SampleRows{lig_off[b], lig_off[b + 1], n_lig + poc_off[b], n_lig + poc_off[b + 1]};
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// inclusive prefix sum of v over the first W lanes of the wave
template <int W = 64>
__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
  for (int o = 1; o < W; o <<= 1) {
    const int u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

// exclusive prefix of `mine` over the 1024 threads of the workgroup; *s_total = sum
__device__ __forceinline__ int block_scan_1024(int mine, int* s_wave, int* s_total) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int incl = wave_scan_incl(mine, lane);
  if (lane == 63) s_wave[w] = incl;
  __syncthreads();
  if (w == 0) {
    const int tot = lane < 16 ? s_wave[lane] : 0;
    const int inc = wave_scan_incl<16>(tot, lane);
    if (lane < 16) s_wave[lane] = inc - tot;
    if (lane == 15) *s_total = inc;
  }
  __syncthreads();
  return s_wave[w] + incl - mine;
}

// Sums of three values per thread over the kThreads threads of the workgroup, one fixed halving tree: the totals are
// red[0..2][0] once it returns.  Every per-sample mean of coordinates goes through this tree, so a mean has the same
// bits whichever kernel reduces it.
__device__ __forceinline__ void block_sum3(float s0, float s1, float s2, float (*red)[kThreads]) {
  const int t = threadIdx.x;
  red[0][t] = s0; red[1][t] = s1; red[2][t] = s2;
  __syncthreads();
  for (int o = kThreads / 2; o >= 64; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; red[2][t] += red[2][t + o]; }
    __syncthreads();
  }
  // the steps o = 32 .. 1 stay inside wave 0: the same pairs (t, t + o) in the same order, by lane shuffles, no barriers
  if (t < 64) {
    float x0 = red[0][t], x1 = red[1][t], x2 = red[2][t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { x0 += __shfl_down(x0, o); x1 += __shfl_down(x1, o); x2 += __shfl_down(x2, o); }
    if (t == 0) { red[0][0] = x0; red[1][0] = x1; red[2][0] = x2; }
  }
  __syncthreads();
}

// first index of the sorted a[0..n) whose entry is >= v, found by the 64 lanes of a wave together: every round probes 64
// evenly spaced entries and keeps the gap the answer lies in -- 3 dependent loads for 2^18 entries, where the bisection of
// lower_bound_i64 takes 18.  The same integer.
template <class I>
__device__ __forceinline__ int lower_bound_wave(const I* a, int n, long long v, int lane) {
  static_assert(sizeof(I) == 8, "64-bit masks");
  int lo = 0, hi = n;
  while (lo < hi) {
    const int step = (hi - lo + 63) / 64;
    const int idx = lo + lane * step;
    const int c = __popcll(__ballot(idx < hi && a[idx] < v));   // sorted: the probes below v are the first c
    if (c == 0) return lo;
    const int last = lo + (c - 1) * step;                        // a[last] < v <= a[last + step] (or the end)
    hi = min(last + step, hi);
    lo = last + 1;
  }
  return lo;
}

// sample_rows from the masks by the four waves of a workgroup at once (wave w finds bound w); s_rows: 4 ints of LDS
__device__ __forceinline__ SampleRows sample_rows_wg(const int64_t* mask_lig, int n_lig, const int64_t* mask_poc,
                                                     int n_poc, int b, int* s_rows) {
  static_assert(kThreads == 256, "one wave per bound");
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = w < 2 ? lower_bound_wave(mask_lig, n_lig, b + (w & 1), lane)
                      : lower_bound_wave(mask_poc, n_poc, b + (w & 1), lane);
  if (lane == 0) s_rows[w] = r;
  __syncthreads();
  return SampleRows{s_rows[0], s_rows[1], s_rows[2], s_rows[3]};
}

// mean[b] = mean of x over ALL nodes of sample b = blockIdx.x (egnn_new.py:307-310): the body of sample_mean_kernel, of
// the tail of coord_update_mean_kernel and of levels_kernel (block 0's mean of a pruned call rides in the levels launch)
__device__ __forceinline__ void sample_mean_body(const float* x, const int* lig_off, const int* poc_off, int n_lig,
                                                 float* mean, float (*red)[kThreads]) {
  const int b = blockIdx.x, t = threadIdx.x;
  const SampleRows r = sample_rows(lig_off, poc_off, n_lig, b);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int i = r.l0 + t; i < r.l1; i += kThreads) { s0 += x[3 * i]; s1 += x[3 * i + 1]; s2 += x[3 * i + 2]; }
  for (int i = r.p0 + t; i < r.p1; i += kThreads) { s0 += x[3 * i]; s1 += x[3 * i + 1]; s2 += x[3 * i + 2]; }
  block_sum3(s0, s1, s2, red);
  if (t < 3) mean[3 * b + t] = red[t][0] / (float)r.count();
  __syncthreads();
}

// The lanes of a wave fill a list segment that ends at `from` up to the next wave-tile boundary with inactive entries
// (row = -1); returns that boundary.
__device__ __forceinline__ int pad_fill(int from, int lane, int* erow, int* ecol, float* ed0, int cap) {
  const int to = align_edges(from), pos = from + lane;
  if (pos >= 0 && pos < to && pos < cap) { erow[pos] = -1; ecol[pos] = 0; ed0[pos] = 0.f; }
  return to;
}

// Zero fill as an ordinary kernel on the caller's stream.  hipMemsetAsync is avoided inside
// dsbdd_dynamics_forward: its blit submissions were observed to lose their ordering against launches
// of a captured graph on the same stream (profiles/README.md, "eager calls between graph replays").
__global__ void zero_kernel(uint4* p, size_t n16, unsigned char* tail, int n_tail) {
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x)
    p[i] = z;
  if (blockIdx.x == 0 && (int)threadIdx.x < n_tail) tail[threadIdx.x] = 0;
}

// ptr must be 16-byte aligned (every workspace buffer is 256-byte aligned)
inline hipError_t zero_async(void* ptr, size_t bytes, hipStream_t s) {
  if (bytes == 0) return hipSuccess;
  const size_t n16 = bytes / 16;
  const int n_tail = (int)(bytes % 16);
  size_t blocks = (n16 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(zero_kernel, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<uint4*>(ptr), n16,
                     static_cast<unsigned char*>(ptr) + n16 * 16, n_tail);
  return hipGetLastError();
}

}  // namespace dsbdd
