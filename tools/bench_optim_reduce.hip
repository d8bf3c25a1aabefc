// Times the first launch of the optimiser step on a gradient bucket by device events: optim_norm_kernel (one GPU) and
// optim_reduce_norm_kernel (data-parallel ranks, the rank buffers emulated in this process) at n_ranks = 1, 2, 8, the
// versions alternating inside every round.  profiles/data_parallel.md is written from its output.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/bench_optim_reduce.hip -o bench_optim_reduce
//   bench_optim_reduce numel.txt [rounds]        numel.txt: one tensor size per line (tools/bucket_numel.py)
#include "../diffsbdd_amd/csrc/optim.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace dsbdd;

#define CHECK(x)                                                                                   \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
  } while (0)

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s numel.txt [rounds]\n", argv[0]); return 2; }
  const int rounds = argc > 2 ? std::atoi(argv[2]) : 200;
  std::vector<long long> numel;
  if (FILE* f = std::fopen(argv[1], "r")) {
    long long v;
    while (std::fscanf(f, "%lld", &v) == 1) if (v > 0) numel.push_back(v);
    std::fclose(f);
  }
  if (numel.empty() || rounds < 1) { std::fprintf(stderr, "no tensor sizes\n"); return 2; }
  // the chunk table of dsbdd_optim_create
  std::vector<OptimChunk> chunks;
  std::vector<int> chunk_first;
  std::vector<long long> offset;
  long long flat = 0, elements = 0;
  for (size_t i = 0; i < numel.size(); ++i) {
    offset.push_back(flat);
    chunk_first.push_back((int)chunks.size());
    for (long long e = 0; e < numel[i]; e += kOptimChunk)
      chunks.push_back(OptimChunk{(int)i, (int)e, (int)std::min<long long>(kOptimChunk, numel[i] - e), (int)(flat + e)});
    flat += (numel[i] + 3) & ~3ll;
    elements += numel[i];
  }
  chunk_first.push_back((int)chunks.size());
  if (flat >= (1ll << 31)) { std::fprintf(stderr, "bucket too large\n"); return 2; }
  const int max_ranks = 8;
  const long long stride = flat;                     // (a multiple of 4: the 16-byte path)
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int n_cu = prop.multiProcessorCount;

  float *gathered = nullptr, *out = nullptr;
  OptimChunk* d_chunks = nullptr;
  double *partial = nullptr, *queue = nullptr, *scratch = nullptr;
  CHECK(hipMalloc(&gathered, (size_t)max_ranks * stride * sizeof(float)));
  CHECK(hipMalloc(&out, (size_t)flat * sizeof(float)));
  CHECK(hipMalloc(&d_chunks, chunks.size() * sizeof(OptimChunk)));
  CHECK(hipMalloc(&partial, chunks.size() * sizeof(double)));
  CHECK(hipMalloc(&queue, 2 * kQueueStride * sizeof(double)));
  CHECK(hipMalloc(&scratch, 256));
  std::vector<float> host((size_t)max_ranks * stride);
  unsigned s = 12345u;
  for (float& v : host) { s = s * 1664525u + 1013904223u; v = ((int)(s >> 8) % 2001 - 1000) * 1e-3f; }
  CHECK(hipMemcpy(gathered, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(out, host.data(), (size_t)flat * sizeof(float), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_chunks, chunks.data(), chunks.size() * sizeof(OptimChunk), hipMemcpyHostToDevice));
  std::vector<double> q(2 * kQueueStride, 0.0);
  q[0] = q[kQueueStride] = 3000.0;
  q[QS_LEN] = q[kQueueStride + QS_LEN] = 1.0;
  CHECK(hipMemcpy(queue, q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice));

  // variant 0: optim_norm_kernel on `out`; variants 1..3: optim_reduce_norm_kernel, n_ranks 1, 2, 8, gathered -> out
  const int ranks_of[4] = {0, 1, 2, 8};
  auto run = [&](int variant) -> hipError_t {
    const int n = (int)numel.size();
    for (int lo = 0; lo < n; lo += kOptimTensors) {
      const int hi = std::min(lo + kOptimTensors, n);
      OptimLaunch L{};
      L.chunks = d_chunks; L.n_chunks = (int)chunks.size(); L.partial = partial; L.queue = queue; L.scratch = scratch;
      L.clip = 1; L.first = lo == 0; L.tensor_lo = lo; L.chunk_lo = chunk_first[lo]; L.chunk_hi = chunk_first[hi];
      OptimStepArgs A{};
      for (int i = lo; i < hi; ++i) A.grad[i - lo] = out + offset[i];
      int grid = std::max(1, std::min(L.chunk_hi - L.chunk_lo, 2 * n_cu));
      if (variant == 0) {
        hipLaunchKernelGGL(optim_norm_kernel, dim3(grid), dim3(kOptimThreads), 0, 0, L, A);
      } else {
        const OptimRanks R{gathered, stride, ranks_of[variant], out};
        hipLaunchKernelGGL(optim_reduce_norm_kernel, dim3(grid), dim3(kOptimThreads), 0, 0, L, A, R);
      }
    }
    return hipGetLastError();
  };
  hipEvent_t t0, t1;
  CHECK(hipEventCreate(&t0));
  CHECK(hipEventCreate(&t1));
  for (int w = 0; w < 20; ++w)
    for (int v = 0; v < 4; ++v) CHECK(run(v));
  CHECK(hipDeviceSynchronize());
  std::vector<float> ms[4];
  for (int r = 0; r < rounds; ++r)
    for (int k = 0; k < 4; ++k) {
      const int v = (r & 1) ? 3 - k : k;             // the order turns round every round
      CHECK(hipEventRecord(t0, 0));
      CHECK(run(v));
      CHECK(hipEventRecord(t1, 0));
      CHECK(hipEventSynchronize(t1));
      float t = 0.f;
      CHECK(hipEventElapsedTime(&t, t0, t1));
      ms[v].push_back(t);
    }
  const int launches = ((int)numel.size() + kOptimTensors - 1) / kOptimTensors;
  std::printf("{\"device\": \"%s\", \"tensors\": %zu, \"elements\": %lld, \"bucket_bytes\": %lld, \"chunks\": %zu, "
              "\"launches\": %d, \"rounds\": %d}\n", prop.name, numel.size(), elements, flat * 4, chunks.size(), launches, rounds);
  for (int v = 0; v < 4; ++v) {
    std::sort(ms[v].begin(), ms[v].end());
    const double med = ms[v][ms[v].size() / 2], lo = ms[v][ms[v].size() / 10], hi = ms[v][ms[v].size() * 9 / 10];
    const double read = (double)elements * 4 * (v == 0 ? 1 : ranks_of[v]), written = v == 0 ? 0.0 : (double)elements * 4;
    std::printf("{\"kernel\": \"%s\", \"n_ranks\": %d, \"median_us\": %.2f, \"p10_us\": %.2f, \"p90_us\": %.2f, "
                "\"bytes_read\": %.0f, \"bytes_written\": %.0f, \"read_GBps\": %.1f}\n",
                v == 0 ? "optim_norm_kernel" : "optim_reduce_norm_kernel", ranks_of[v], med * 1e3, lo * 1e3, hi * 1e3, read,
                written, read / (med * 1e-3) * 1e-9);
  }
  return 0;
}
