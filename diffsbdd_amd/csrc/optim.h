// Gradient norm, adaptive clipping and AdamW(amsgrad) as two launches without a host round trip.
//
// One optimiser step of the reference is configure_gradient_clipping (lightning_modules.py:874-899: a queue of the
// last 50 gradient norms, threshold 1.5 mean + 2 std, clip_grad_norm_) followed by torch.optim.AdamW(amsgrad=True).
// Here:
//   launch 1  optim_norm_kernel    per-chunk sums of g^2 (double) -> partial[chunk]; workgroup 0 evaluates the
//                                  threshold from the queue of parity p and writes it to the scratch record
//   launch 2  optim_update_kernel  EVERY workgroup reduces the same partials in the same order and derives the same
//                                  clip coefficient; then p, m, v, vmax of its chunks are updated with the gradient
//                                  scaled as it is read; workgroup 0 writes the queue of parity p ^ 1 and the counters
// Data-parallel ranks (dsbdd_optim_step_ranks): launch 1 is optim_reduce_norm_kernel instead, which folds the ranks' gradient
// buckets in rank order as it reads them and leaves the same partials; launch 2 is unchanged.
// The queue is double-buffered by step parity: within one launch no workgroup reads what another one writes.
// No floating-point atomics: every sum has a fixed order, the result is bitwise reproducible.
// Gradient pointers change every step (fresh allocations of the backward pass) and travel BY VALUE in the kernel
// arguments together with the per-tensor scalars the host derives from the per-tensor step counts in double, as
// torch does (bias corrections); kOptimTensors tensors per launch, more tensors -> more launches.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dsbdd {

constexpr int kOptimThreads = 256;
constexpr int kOptimChunk = 8192;      // elements of one tensor per chunk (multiple of 4 * kOptimThreads)
constexpr int kOptimTensors = 200;     // tensors per launch: 200 * 16 B of kernel arguments (limit 4 KB)
constexpr int kQueueLen = 50;          // utils.Queue(max_len=50)
constexpr int kQueueStride = 64;       // doubles per parity: ring[50] + the record below
enum { QS_LEN = 50, QS_HEAD, QS_CLIPS, QS_LAST_NORM, QS_LAST_MAX, QS_STEPS, QS_LAST_COEF };

struct OptimChunk {
  int tensor;     // index into the parameter table
  int offset;     // first element of the chunk within its tensor
  int count;      // elements
  int flat;       // first element in the flat m / v / vmax buffers
};

struct OptimStepArgs {
  const float* grad[kOptimTensors];      // NULL: the tensor has no gradient at this step and is skipped entirely
  float step_size_neg[kOptimTensors];    // -lr / (1 - beta1^step)
  float bc2_sqrt[kOptimTensors];         // sqrt(1 - beta2^step)
};

struct OptimLaunch {
  const OptimChunk* chunks;
  int chunk_lo, chunk_hi;      // this launch's chunks (tensors tensor_lo .. tensor_lo + kOptimTensors)
  int n_chunks;                // all chunks (= length of partial[])
  int tensor_lo;
  float* const* params;
  float *m, *v, *vmax;
  double* partial;
  double* queue;               // [2][kQueueStride]
  double* scratch;             // [0] threshold of this step
  int parity;                  // the queue this step reads
  int clip;                    // 0: plain AdamW
  int first;                   // this launch owns the queue / threshold writes
  float decay, w1, beta2, w2, eps;
};

__device__ inline double wave_sum_f64(double x) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) x += __shfl_xor(x, o, 64);     // butterfly: every lane ends with the same bits
  return x;
}

// sum over the workgroup in a fixed order; every thread receives the same value
__device__ inline double block_sum_f64(double x, double* lds) {
  x = wave_sum_f64(x);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[w] = x;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < kOptimThreads / 64; ++i) s += lds[i];
  return s;
}

// threshold 1.5 mean + 2 std (population) of the queue, one lane, double
__device__ inline double queue_threshold(const double* q) {
  int len = (int)q[QS_LEN];
  len = len < 1 ? 1 : (len > kQueueLen ? kQueueLen : len);
  double s = 0.0;
  for (int i = 0; i < len; ++i) s += q[i];
  const double mean = s / len;
  double d2 = 0.0;
  for (int i = 0; i < len; ++i) { const double d = q[i] - mean; d2 += d * d; }
  return 1.5 * mean + 2.0 * sqrt(d2 / len);
}

__global__ __launch_bounds__(kOptimThreads) void optim_norm_kernel(OptimLaunch L, OptimStepArgs A) {
  __shared__ double lds[kOptimThreads / 64];
  if (L.first && blockIdx.x == 0 && threadIdx.x == 0) L.scratch[0] = queue_threshold(L.queue + L.parity * kQueueStride);
  for (int c = L.chunk_lo + blockIdx.x; c < L.chunk_hi; c += gridDim.x) {
    const OptimChunk ch = L.chunks[c];
    const float* g = A.grad[ch.tensor - L.tensor_lo];
    double acc = 0.0;
    if (g) {
      g += ch.offset;
      const int n = ch.count;
      if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const int n4 = n >> 2;
        const float4* g4 = reinterpret_cast<const float4*>(g);
        for (int i = threadIdx.x; i < n4; i += kOptimThreads) {
          const float4 q = g4[i];
          acc += (double)q.x * q.x; acc += (double)q.y * q.y; acc += (double)q.z * q.z; acc += (double)q.w * q.w;
        }
        for (int i = (n4 << 2) + threadIdx.x; i < n; i += kOptimThreads) acc += (double)g[i] * g[i];
      } else {
        for (int i = threadIdx.x; i < n; i += kOptimThreads) acc += (double)g[i] * g[i];
      }
    }
    const double s = block_sum_f64(acc, lds);
    if (threadIdx.x == 0) L.partial[c] = s;
  }
}

// Data-parallel ranks: the flat gradient buckets of n_ranks ranks (layout of the m / v / vmax buffers, OptimChunk::flat),
// `stride` floats apart, folded in rank order into `out` (which may be one of them).
struct OptimRanks {
  const float* gathered;
  long long stride;
  int n_ranks;
  float* out;
};

// Launch 1 of a data-parallel step: s = ((g[0] + g[1]) + g[2]) + ... per element in float32 (one rounding per add, rank
// order), s -> out, and the per-chunk sums of s^2 with the thread <- element assignment, the per-thread order and the
// block_sum_f64 of optim_norm_kernel's 16-byte path: partial[c] has the bits optim_norm_kernel leaves on the reduced
// bucket.  Every element is read (all ranks) and written by one thread only, so `out` may alias a rank's bucket.
// A tensor without a gradient is neither read nor written (its region may hold NaN).
__global__ __launch_bounds__(kOptimThreads) void optim_reduce_norm_kernel(OptimLaunch L, OptimStepArgs A, OptimRanks R) {
  __shared__ double lds[kOptimThreads / 64];
  if (L.clip && L.first && blockIdx.x == 0 && threadIdx.x == 0)
    L.scratch[0] = queue_threshold(L.queue + L.parity * kQueueStride);
  // float4 accesses need every rank's copy of a chunk 16-byte aligned: flat is a multiple of 4 elements
  const bool vec = ((reinterpret_cast<uintptr_t>(R.gathered) | reinterpret_cast<uintptr_t>(R.out)) & 15) == 0 &&
                   (R.n_ranks == 1 || (R.stride & 3) == 0);
  for (int c = L.chunk_lo + blockIdx.x; c < L.chunk_hi; c += gridDim.x) {
    const OptimChunk ch = L.chunks[c];
    double acc = 0.0;
    if (A.grad[ch.tensor - L.tensor_lo]) {
      const float* g = R.gathered + ch.flat;
      float* o = R.out + ch.flat;
      const int n = ch.count;
      const int n4 = n >> 2;
      if (vec) {
        for (int i = threadIdx.x; i < n4; i += kOptimThreads) {
          float4 q = reinterpret_cast<const float4*>(g)[i];
          for (int r = 1; r < R.n_ranks; ++r) {
            const float4 a = reinterpret_cast<const float4*>(g + r * R.stride)[i];
            q.x = q.x + a.x; q.y = q.y + a.y; q.z = q.z + a.z; q.w = q.w + a.w;
          }
          reinterpret_cast<float4*>(o)[i] = q;
          acc += (double)q.x * q.x; acc += (double)q.y * q.y; acc += (double)q.z * q.z; acc += (double)q.w * q.w;
        }
      } else {
        for (int i = threadIdx.x; i < n4; i += kOptimThreads) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int e = 4 * i + k;
            float q = g[e];
            for (int r = 1; r < R.n_ranks; ++r) q = q + g[r * R.stride + e];
            o[e] = q;
            acc += (double)q * q;
          }
        }
      }
      for (int e = (n4 << 2) + threadIdx.x; e < n; e += kOptimThreads) {
        float q = g[e];
        for (int r = 1; r < R.n_ranks; ++r) q = q + g[r * R.stride + e];
        o[e] = q;
        acc += (double)q * q;
      }
    }
    const double s = block_sum_f64(acc, lds);
    if (threadIdx.x == 0) L.partial[c] = s;
  }
}

struct OptimScal {
  float coef, decay, w1, beta2, w2, eps, step_size_neg, bc2_sqrt;
};

// torch.optim.AdamW(amsgrad=True), operation order of torch/optim/adam.py: decay, exp_avg lerp, exp_avg_sq, running
// max, sqrt / bias_correction2_sqrt + eps, addcdiv.  The gradient is scaled as it is read (clip_grad_norm_ scales it in place).
__device__ inline void adamw_elem(float& p, float gr, float& m, float& v, float& vm, const OptimScal& s) {
  const float g = gr * s.coef;
  p = p * s.decay;
  m = m + s.w1 * (g - m);                       // lerp, |weight| < 0.5
  v = v * s.beta2;
  v = v + s.w2 * (g * g);                       // addcmul
  vm = (v > vm || v != v) ? v : vm;             // torch.maximum (propagates NaN)
  const float denom = sqrtf(vm) / s.bc2_sqrt + s.eps;
  p = p + s.step_size_neg * (m / denom);        // addcdiv
}

__global__ __launch_bounds__(kOptimThreads) void optim_update_kernel(OptimLaunch L, OptimStepArgs A) {
  __shared__ double lds[kOptimThreads / 64];
  float coef = 1.f;
  if (L.clip) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < L.n_chunks; i += kOptimThreads) acc += L.partial[i];
    const double sum = block_sum_f64(acc, lds);
    const float normf = (float)sqrt(sum);                      // the reference holds the norm as a float32 tensor
    const double thr = L.scratch[0];
    // clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1, in float32
    coef = (1.0f / (normf + 1e-6f)) * (float)thr;
    coef = coef < 1.0f ? coef : 1.0f;
    if (L.first && blockIdx.x == 0 && threadIdx.x == 0) {
      const double* q = L.queue + L.parity * kQueueStride;
      double* o = L.queue + (L.parity ^ 1) * kQueueStride;
      const double norm = (double)normf;
      const bool clipped = norm > thr;
      int len = (int)q[QS_LEN], head = (int)q[QS_HEAD];
      if (head < 0 || head >= kQueueLen) head = 0;             // device memory is never trusted as an index
      len = len < 0 ? 0 : len;
      for (int i = 0; i < kQueueLen; ++i) o[i] = q[i];
      o[head] = clipped ? thr : norm;                          // the entry appended is min(grad_norm, max_norm)
      head = head + 1 == kQueueLen ? 0 : head + 1;
      if (len < kQueueLen) ++len;
      o[QS_LEN] = (double)len;
      o[QS_HEAD] = (double)head;
      o[QS_CLIPS] = q[QS_CLIPS] + (clipped ? 1.0 : 0.0);
      o[QS_LAST_NORM] = norm;
      o[QS_LAST_MAX] = thr;
      o[QS_STEPS] = q[QS_STEPS] + 1.0;
      o[QS_LAST_COEF] = (double)coef;
    }
  }
  OptimScal s{coef, L.decay, L.w1, L.beta2, L.w2, L.eps, 0.f, 1.f};
  for (int c = L.chunk_lo + blockIdx.x; c < L.chunk_hi; c += gridDim.x) {
    const OptimChunk ch = L.chunks[c];
    const int t = ch.tensor - L.tensor_lo;
    const float* g = A.grad[t];
    if (!g) continue;                                          // no gradient: no decay, no state, no step count
    g += ch.offset;
    s.step_size_neg = A.step_size_neg[t];
    s.bc2_sqrt = A.bc2_sqrt[t];
    float* p = L.params[ch.tensor] + ch.offset;
    float* m = L.m + ch.flat;
    float* v = L.v + ch.flat;
    float* vm = L.vmax + ch.flat;
    const int n = ch.count;
    int done = 0;
    if (((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(p)) & 15) == 0) {   // m / v / vmax: flat is a multiple of 4
      const int n4 = n >> 2;
      const float4* g4 = reinterpret_cast<const float4*>(g);
      float4* p4 = reinterpret_cast<float4*>(p);
      float4* m4 = reinterpret_cast<float4*>(m);
      float4* v4 = reinterpret_cast<float4*>(v);
      float4* vm4 = reinterpret_cast<float4*>(vm);
      for (int i = threadIdx.x; i < n4; i += kOptimThreads) {
        const float4 gg = g4[i];
        float4 pp = p4[i], mm = m4[i], vv = v4[i], xx = vm4[i];
        adamw_elem(pp.x, gg.x, mm.x, vv.x, xx.x, s);
        adamw_elem(pp.y, gg.y, mm.y, vv.y, xx.y, s);
        adamw_elem(pp.z, gg.z, mm.z, vv.z, xx.z, s);
        adamw_elem(pp.w, gg.w, mm.w, vv.w, xx.w, s);
        p4[i] = pp; m4[i] = mm; v4[i] = vv; vm4[i] = xx;
      }
      done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < n; i += kOptimThreads) {
      float pp = p[i], mm = m[i], vv = v[i], xx = vm[i];
      adamw_elem(pp, g[i], mm, vv, xx, s);
      p[i] = pp; m[i] = mm; v[i] = vv; vm[i] = xx;
    }
  }
}

}  // namespace dsbdd
