// Packed ligand batch of the design front ends (substructure inpainting, diversification): every batch slot takes
// the atoms of one template in its first rows and is padded with empty rows up to the slot's size.  The reference
// builds this on the host: inpaint.py:114-141 (a loop over samples with three masked read-modify-writes each, every
// one a synchronising boolean index) and optimize.py:39-62,210-222 (one concatenation of host conformers per
// generation).  Here it is ONE launch, one thread per output row: the slot of a row is found by bisection over the
// slot offsets (a few hundred integers, cache resident), the row is copied from its template or zeroed, and the
// templates may be the device output of an earlier chain -- no coordinate crosses the host between generations.
// Plain loads and stores, no atomics; every index that comes from device memory is range-checked before use.
#pragma once
#include "common.h"

namespace dsbdd {

struct PackArgs {
  const float* tmpl_x;       // [M][3]
  const int* tmpl_type;      // [M] class ids
  const int* tmpl_ptr;       // [n_tmpl + 1] first row of every template
  const int* slot_tmpl;      // [B] template of every slot
  const int* slot_size;      // [B] rows of every slot (>= rows of its template)
  const int* slot_off;       // [B + 1] first output row of every slot
  int n_tmpl, m_rows, batch, n_rows, atom_nf;
  float* x;                  // [N][3]
  float* one_hot;            // [N][atom_nf]
  long long* fixed;          // [N] 1 = template row
  long long* mask;           // [N] slot id
  long long* size;           // [B]
};

__global__ __launch_bounds__(kThreads) void pack_ligands_kernel(PackArgs p) {
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r < p.batch) p.size[r] = p.slot_size[r];                 // (n_rows >= batch: every slot has a row)
  if (r >= p.n_rows) return;
  int lo = 0, hi = p.batch - 1;                                // last slot with slot_off[slot] <= r
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.slot_off[mid] <= r) lo = mid; else hi = mid - 1;
  }
  const int k = r - p.slot_off[lo];                            // row inside the slot
  const int t = p.slot_tmpl[lo];
  int src = -1;
  if (t >= 0 && t < p.n_tmpl && k >= 0) {
    const int t0 = p.tmpl_ptr[t], len = p.tmpl_ptr[t + 1] - t0;
    if (k < len && k < p.slot_size[lo] && t0 >= 0 && t0 + k < p.m_rows) src = t0 + k;
  }
  float vx = 0.0f, vy = 0.0f, vz = 0.0f;
  int type = -1;
  if (src >= 0) {
    vx = p.tmpl_x[3 * src];
    vy = p.tmpl_x[3 * src + 1];
    vz = p.tmpl_x[3 * src + 2];
    type = p.tmpl_type[src];
  }
  p.x[3 * (size_t)r] = vx;
  p.x[3 * (size_t)r + 1] = vy;
  p.x[3 * (size_t)r + 2] = vz;
  float* h = p.one_hot + (size_t)r * p.atom_nf;
  for (int c = 0; c < p.atom_nf; ++c) h[c] = c == type ? 1.0f : 0.0f;
  p.fixed[r] = src >= 0 ? 1 : 0;
  p.mask[r] = lo;
}

}  // namespace dsbdd
