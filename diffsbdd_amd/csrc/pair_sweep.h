// What the ligand-pocket pair kernels share (pose_check_kernel in pose_check.h, vina_score_kernel in vina_score.h,
// vina_grad_kernel in vina_grad.h, and vina_intra_kernel in vina_intra.h, whose "group" is the molecule itself), defined once: the batch, its range check, the squared distance, and the sweep of a molecule's atoms over its pocket group.
//
// pair_sweep: one workgroup per molecule.  The pocket atoms of the molecule's group pass through LDS in tiles of kPairTile
// (x, y, z and one word of the policy's as one float4 each: lane j reads 16 contiguous bytes, conflict free); wave w takes
// the ligand atoms w, w + 4, ..., its lanes stride over the tile (j ascends in steps of 64), a butterfly of wave shuffles
// (o = 32, 16, ..., 1) folds the lanes.  Neither the molecule nor the group has a size limit below int32: a molecule
// longer than the workgroup is a longer atom loop, a group larger than a tile is a longer tile loop, and an atom's
// running record between tiles lives in its output row (written and read back by lane 0 of the one wave that owns the
// atom).  On the last tile lane 0 adds the atom to its wave's totals; those meet in LDS and thread 0 folds them in wave
// order.  No atomics, and the order of every reduction is a function of the molecule and its group alone: the outputs
// are bitwise reproducible and do not depend on what else is in the batch.  Every offset and group id read from device
// memory is range-checked before it is used (pair_rows): what fails the check is an empty molecule / an empty group.
//
// A policy is a plain struct of inline functions on the caller's registers (no virtuals, no function pointers): its types
// Atom (a ligand atom with the policy's own columns), Record (the atom's running record) and Total (a wave's totals) with
// zero() and zero_total(), `part` = Total[kThreads / 64] in LDS declared by the kernel, tile_word(r) = the fourth float4
// component of pocket row r, atom(r, x, y, z) = the ligand atom of row r, and the calls marked below.
#pragma once
#include "common.h"

namespace dsbdd {

constexpr int kPairTile = 1024;     // pocket atoms per LDS tile (16 KiB)

struct PairBatch {
  const float* lig_x;      // [N][3] Angstrom
  const int* mol_off;      // [B+1] first row of every molecule (N = mol_off[B])
  const int* mol_group;    // [B] pocket group of every molecule
  const float* poc_x;      // [M][3]
  const int* group_off;    // [G+1] first pocket row of every group (M = group_off[G])
  int batch, n_groups;
};

struct PairRows { int lo, n, glo, m; };     // the molecule's ligand rows [lo, lo + n), its group's pocket rows [glo, glo + m)

// the rows of molecule b and of its group, range-checked against the totals the offset arrays end in
__device__ inline PairRows pair_rows(const PairBatch& p, int b) {
  const int n_total = p.mol_off[p.batch], m_total = p.group_off[p.n_groups];
  const int lo = p.mol_off[b], hi = p.mol_off[b + 1];
  const int n = (lo >= 0 && hi >= lo && hi <= n_total) ? hi - lo : 0;
  const int g = p.mol_group[b];
  int glo = 0, m = 0;
  if (g >= 0 && g < p.n_groups) {
    glo = p.group_off[g];
    const int ghi = p.group_off[g + 1];
    m = (glo >= 0 && ghi >= glo && ghi <= m_total) ? ghi - glo : 0;
  }
  return {lo, n, glo, m};
}

// (dx dx + dy dy) + dz dz in float32, five roundings.  The toolkit's __fadd_rn / __fmul_rn are the plain operators unless
// OCML_BASIC_ROUNDED_OPERATIONS is defined, so the roundings are enforced here: floating-point contraction is off (no
// fused multiply-add).  Its root is taken with sqrtf, which hipcc rounds correctly.
__device__ inline float pair_dist2(float xi, float yi, float zi, float xj, float yj, float zj) {
#pragma clang fp contract(off)
  const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  return (xx + yy) + zz;
}
__device__ inline bool pose_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

template <class Policy>
__device__ inline void pair_sweep(const PairBatch& p, const PairRows& rows, Policy& pol) {
  constexpr int kWaves = kThreads / 64;
  __shared__ float4 tile[kPairTile];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lo = rows.lo, n = rows.n, glo = rows.glo, m = rows.m;
  typename Policy::Total w_total = Policy::zero_total();           // of the atoms this wave owns (lane 0 keeps it)
  const int n_tiles = m > 0 ? (m - 1) / kPairTile + 1 : 1;         // an empty group: one pass over an empty tile
  for (int t = 0; t < n_tiles; ++t) {
    const int base = t * kPairTile, cnt = min(kPairTile, m - base);
    if (t) __syncthreads();                                        // the previous tile has been read
    for (int j = tid; j < cnt; j += kThreads) {
      const size_t r = (size_t)glo + base + j;
      tile[j] = make_float4(p.poc_x[3 * r], p.poc_x[3 * r + 1], p.poc_x[3 * r + 2], pol.tile_word(r));
    }
    __syncthreads();
    const bool last = t == n_tiles - 1;
    for (int a = wave; a < n; a += kWaves) {
      const size_t r = (size_t)lo + a;
      const typename Policy::Atom atom = pol.atom(r, p.lig_x[3 * r], p.lig_x[3 * r + 1], p.lig_x[3 * r + 2]);
      typename Policy::Record rec = Policy::zero();
      if (!pol.skip(atom)) {                                       // wave-uniform: an atom that meets no pocket atom
        for (int j = lane; j < cnt; j += 64) pol.pair(rec, atom, tile[j], base + j);     // the (base + j)-th of the group
        for (int o = 32; o; o >>= 1) pol.fold(rec, o);             // the record of lane ^ o joins this lane's
      }
      if (lane == 0) {
        if (t) pol.carry(rec, r);                                  // the record of the tiles before, from output row r
        pol.store(rec, r);                                         // the output row
        if (last) pol.total(w_total, rec, atom);                   // the atom joins its wave's totals
      }
    }
  }
  if (lane == 0) pol.part[wave] = w_total;
  __syncthreads();
  if (tid == 0) {
    typename Policy::Total s = Policy::zero_total();
    for (int w = 0; w < kWaves; ++w) Policy::merge(s, pol.part[w]);     // in wave order
    pol.finish(b, n, s);                                           // the row of molecule b (n atoms)
  }
}

}  // namespace dsbdd
