// Pose checks of a batch of ligands against the heavy atoms of their pockets (diffsbdd_amd/pose.py): per ligand atom the
// number of pocket atoms it clashes with (d < r_i + r_j - tol), the number in contact (d < contact), the nearest pocket
// atom and its distance; per molecule the totals.  One launch, no host round trip: the sampled coordinates are on the
// device before a molecule is built.
//
// pose_check_kernel is pair_sweep (pair_sweep.h: the tiles, the waves, the carry between tiles, the range checks) under
// PosePolicy; the fourth tile component is the pocket atom's radius.  Every reduction is an integer sum, a minimum, or
// an arg-min whose ties go to the smallest index -- all of them independent of the order and of the mapping, which is
// what makes the numpy restatement (_pose_check_host) exact.
//
// Arithmetic: float32, every operation rounded to nearest on its own (molecule.h:37-38 names the roundings the same way);
// pair_dist2 and pose_clash_limit are compiled with floating-point contraction off, the root is a correctly rounded sqrtf.
#pragma once
#include "common.h"
#include "pair_sweep.h"

namespace dsbdd {

constexpr int kPoseAtomOut = 4;     // ints per ligand atom: n_clash, n_contact, nearest, bits of the smallest d
constexpr int kPoseMolOut = 8;      // ints per molecule: n_atoms, clash pairs, clash atoms, contact pairs, contact atoms, nonfinite, bits of the smallest d, 0

struct PoseArgs {
  PairBatch pairs;
  const float* lig_r;      // [N] van-der-Waals radius
  const float* poc_r;      // [M]
  float tol, contact;
  int* atom_out;           // [N][kPoseAtomOut]
  int* mol_out;            // [B][kPoseMolOut]
};

// d = sqrt((dx dx + dy dy) + dz dz), five roundings and a correctly rounded root
__device__ inline float pose_distance(float xi, float yi, float zi, float xj, float yj, float zj) {
  return sqrtf(pair_dist2(xi, yi, zi, xj, yj, zj));
}
// (r_i + r_j) - tol
__device__ inline float pose_clash_limit(float ri, float rj, float tol) {
#pragma clang fp contract(off)
  const float sum = ri + rj;
  return sum - tol;
}
// (d, index) records: the smaller d wins, ties go to the smaller index; (+inf, -1) is "none" and never wins
__device__ inline bool pose_closer(float d, int i, float than_d, int than_i) {
  return d < than_d || (d == than_d && i < than_i);
}

struct PosePolicy {
  struct Atom { float x, y, z, r; };
  struct Record { int n_clash, n_contact, near; float best; };
  struct Total { int sum[4], nonfinite; float min_d; };            // clash pairs, clash atoms, contact pairs, contact atoms
  const PoseArgs& p;
  Total* part;             // [kThreads / 64] in LDS

  __device__ static Record zero() { return {0, 0, -1, __builtin_inff()}; }
  __device__ static Total zero_total() { return {{0, 0, 0, 0}, 0, __builtin_inff()}; }
  __device__ float tile_word(size_t r) const { return p.poc_r[r]; }
  __device__ Atom atom(size_t r, float x, float y, float z) const { return {x, y, z, p.lig_r[r]}; }
  __device__ static bool skip(const Atom&) { return false; }
  __device__ void pair(Record& c, const Atom& a, const float4 q, int index) const {
    const float d = pose_distance(a.x, a.y, a.z, q.x, q.y, q.z);
    c.n_clash += d < pose_clash_limit(a.r, q.w, p.tol);             // strict; false for NaN
    c.n_contact += d < p.contact;
    if (d < c.best) { c.best = d; c.near = index; }                 // the index ascends: the first of equal distances stays
  }
  __device__ static void join(Record& c, int n_clash, int n_contact, int near, float best) {
    c.n_clash += n_clash;
    c.n_contact += n_contact;
    if (pose_closer(best, near, c.best, c.near)) { c.best = best; c.near = near; }
  }
  __device__ static void fold(Record& c, int o) {
    join(c, __shfl_xor(c.n_clash, o), __shfl_xor(c.n_contact, o), __shfl_xor(c.near, o), __shfl_xor(c.best, o));
  }
  __device__ void carry(Record& c, size_t r) const {
    const int* out = p.atom_out + kPoseAtomOut * r;
    join(c, out[0], out[1], out[2], __int_as_float(out[3]));
  }
  __device__ void store(const Record& c, size_t r) const {
    int* out = p.atom_out + kPoseAtomOut * r;
    out[0] = c.n_clash; out[1] = c.n_contact; out[2] = c.near; out[3] = __float_as_int(c.best);
  }
  __device__ static void merge(Total& s, const Total& o) {
    for (int k = 0; k < 4; ++k) s.sum[k] += o.sum[k];
    s.nonfinite |= o.nonfinite;
    if (o.min_d < s.min_d) s.min_d = o.min_d;
  }
  __device__ static void total(Total& w, const Record& c, const Atom& a) {
    merge(w, {{c.n_clash, c.n_clash > 0, c.n_contact, c.n_contact > 0},
              pose_nonfinite(a.x) || pose_nonfinite(a.y) || pose_nonfinite(a.z), c.best});
  }
  __device__ void finish(int b, int n, const Total& s) const {
    int* out = p.mol_out + (size_t)kPoseMolOut * b;
    out[0] = n; out[1] = s.sum[0]; out[2] = s.sum[1]; out[3] = s.sum[2]; out[4] = s.sum[3]; out[5] = s.nonfinite;
    out[6] = __float_as_int(s.min_d); out[7] = 0;
  }
};

__global__ __launch_bounds__(kThreads) void pose_check_kernel(PoseArgs p) {
  __shared__ PosePolicy::Total part[kThreads / 64];
  PosePolicy pol{p, part};
  pair_sweep(p.pairs, pair_rows(p.pairs, blockIdx.x), pol);
}

}  // namespace dsbdd
