// The auxiliary Lennard-Jones term of the training loss (LigandPocketDDPM.lj_potential, lightning_modules.py:304-331):
// for every ordered pair i != j of ligand atoms of one sample  4 ((sigma / r)^12 - (sigma / r)^6), clamped from above,
// summed per sample -- and, in the same pass, its derivative with respect to the coordinates.
// One launch, one workgroup per sample.  Atom types are the argmax of the feature columns (no gradient); a clamped
// pair contributes no gradient.  The pair terms are evaluated and summed in double in a fixed order (thread t owns
// atoms t, t + 256, ..., inner loop over j ascending, then a fixed-order workgroup sum): bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "optim.h"   // block_sum_f64

namespace dsbdd {

constexpr int kLjThreads = kOptimThreads;

struct LjArgs {
  const float* xh;          // [n][ld]: coordinates in columns 0-2, features in columns 3 .. 3 + n_types
  int ld, n_types;
  const long long* mask;    // [n] sample of every atom, sorted ascending
  int n, batch;
  const double* sigma;      // [n_types][n_types] = 2^(-1/6) rm / 100 / norm_values[0]
  double clamp;
  int has_clamp;
  int* type;                // [n] scratch: argmax per atom
  float* u;                 // [batch]
  float* dx;                // [n][3] dU_sample / dx
};

__device__ inline int lj_lower_bound(const long long* a, int n, long long key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kLjThreads) void lj_potential_kernel(LjArgs a) {
  __shared__ double lds[kLjThreads / 64];
  __shared__ int range[2];
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    range[0] = lj_lower_bound(a.mask, a.n, b);
    range[1] = lj_lower_bound(a.mask, a.n, (long long)b + 1);
  }
  __syncthreads();
  const int r0 = range[0], r1 = range[1];
  for (int i = r0 + threadIdx.x; i < r1; i += kLjThreads) {
    const float* h = a.xh + (size_t)i * a.ld + 3;
    int best = 0;
    float bv = h[0];
    for (int k = 1; k < a.n_types; ++k) {          // first maximum, as torch.argmax
      const float v = h[k];
      if (v > bv) { bv = v; best = k; }
    }
    a.type[i] = best;
  }
  __syncthreads();                                  // the types of this sample were written by this workgroup
  double usum = 0.0;
  for (int i = r0 + threadIdx.x; i < r1; i += kLjThreads) {
    const float* xi = a.xh + (size_t)i * a.ld;
    const double x0 = xi[0], x1 = xi[1], x2 = xi[2];
    const double* srow = a.sigma + (size_t)a.type[i] * a.n_types;
    double ui = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int j = r0; j < r1; ++j) {
      if (j == i) continue;
      const float* xj = a.xh + (size_t)j * a.ld;
      const double d0 = x0 - xj[0], d1 = x1 - xj[1], d2 = x2 - xj[2];
      const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
      const double sg = srow[a.type[j]];
      const double s2 = sg * sg / r2;
      const double s6 = s2 * s2 * s2, s12 = s6 * s6;
      double e = 4.0 * (s12 - s6);
      double w = 4.0 * (6.0 * s6 - 12.0 * s12) / r2;     // (dE / dr) / r
      if (a.has_clamp && e > a.clamp) { e = a.clamp; w = 0.0; }
      ui += e;
      g0 += w * d0; g1 += w * d1; g2 += w * d2;
    }
    usum += ui;
    // the pair (i, j) enters the sum twice (ordered pairs): both copies depend on x_i
    a.dx[(size_t)i * 3 + 0] = (float)(2.0 * g0);
    a.dx[(size_t)i * 3 + 1] = (float)(2.0 * g1);
    a.dx[(size_t)i * 3 + 2] = (float)(2.0 * g2);
  }
  const double s = block_sum_f64(usum, lds);
  if (threadIdx.x == 0) a.u[b] = (float)s;
}

}  // namespace dsbdd
