// Vina-type interaction score of a batch of ligand poses against the heavy atoms of their pockets (diffsbdd_amd/vina.py;
// the functional form and weights of Trott & Olson, J. Comput. Chem. 31 (2010) 455, heavy atoms only).  Two launches on
// what the samplers and bond_orders_kernel (molecule.h) leave on the device, no host round trip:
//
// vina_type_kernel: one wave per molecule, integers only.  The molecule's lower-triangular order matrix is staged in LDS,
// every atom gets its adjacency as a 128-bit mask (n <= kMolMaxAtoms), and from the masks: the sum of orders, the highest
// order, the heavy degree, "has a neighbour that is not carbon" (one AND with the ballot mask of the carbons), hence the
// atom code; a single bond whose ends both have degree >= 2 is a rotor unless its ends stay connected without it, which
// a frontier expansion on the masks decides (each atom is expanded at most once per bond).
//
// vina_score_kernel: a scan of the molecule's coordinates (one that is not finite ends the workgroup: the flag, and NaN
// in every float the molecule owns), then pair_sweep (pair_sweep.h: the tiles, the waves, the carry between tiles, the
// order of every sum) under VinaPolicy; the fourth tile component is the bits of the pocket atom's code, and a ligand
// atom without a class meets no pocket atom.
//
// Arithmetic: the distance r is the float32 root of pair_dist2, as the pose check rounds it, and the pair counts iff r < 8
// (decided on r^2 < 64 before the root: a correctly rounded root of a float32 below 64 is below 8).  From r on everything
// is float64 -- the surface distance, the five terms, the lane and wave sums -- and is rounded to float32 where it is
// stored, so the only error against the float64 restatement (_vina_score_host) beyond those roundings is that of r.
// Every offset, group id, type id and code read from device memory is range-checked before it is used.
#pragma once
#include "common.h"
#include "mol_metrics.h"
#include "pair_sweep.h"

namespace dsbdd {

constexpr int kVinaTerms = 5;       // gauss1, gauss2, repulsion, hydrophobic, hbond
constexpr int kVinaMolOut = 8;      // floats per molecule: the five sums, inter, score, 0
constexpr int kVinaMolInt = 4;      // ints per molecule: typed atoms, untyped atoms, rotors, 0

// atom code: bits 0-3 class, bit 4 hydrophobic, bit 5 donor, bit 6 acceptor
enum VinaClass { kVinaNone = 0, kVinaC, kVinaN, kVinaO, kVinaP, kVinaS, kVinaF, kVinaCl, kVinaBr, kVinaI, kVinaMetal, kVinaClasses };
constexpr int kVinaHydrophobic = 16, kVinaDonor = 32, kVinaAcceptor = 64;

__device__ inline int vina_class_of(int code) {
  const int c = code & 15;
  return c < kVinaClasses ? c : kVinaNone;
}
__device__ inline double vina_radius(int cls) {     // cls in [0, kVinaClasses)
  constexpr double kRadius[kVinaClasses] = {0.0, 1.9, 1.8, 1.7, 2.1, 2.0, 1.5, 1.8, 2.0, 2.2, 1.2};
  return kRadius[cls];
}

// ---- typing ------------------------------------------------------------------------------------------------------------
struct VinaTypeArgs {
  const signed char* order;   // [B][n_max][n_max] strictly lower triangular (bond_orders_kernel)
  const int* atom_type;       // [N]
  const int* mol_off;         // [B+1]
  const int* class_elem;      // [n_types] class of every atom type
  int batch, n_types, n_max;
  int* lig_code;              // [N]
  int* mol_int;               // [B][kVinaMolInt]
};

struct VinaMask {             // 128 atoms
  mm_u64 w[2];
  __device__ bool any() const { return (w[0] | w[1]) != 0; }
  __device__ bool has(int a) const { return ((a < 64 ? w[0] : w[1]) >> (a & 63)) & 1ull; }
  __device__ void set(int a) { const mm_u64 bit = 1ull << (a & 63); w[0] |= a < 64 ? bit : 0; w[1] |= a < 64 ? 0 : bit; }
  __device__ void clear(int a) { const mm_u64 bit = 1ull << (a & 63); w[0] &= a < 64 ? ~bit : ~0ull; w[1] &= a < 64 ? ~0ull : ~bit; }
  __device__ int count() const { return __popcll(w[0]) + __popcll(w[1]); }
};

// are a and c connected when the bond between them is left out?  adj: [n] masks in LDS
__device__ inline bool vina_bond_in_ring(const VinaMask* adj, int a, int c) {
  VinaMask seen{{0, 0}}, front{{0, 0}};
  seen.set(a);
  front.set(a);
  for (;;) {
    VinaMask next{{0, 0}};
    for (int k = 0; k < 2; ++k) {
      mm_u64 f = front.w[k];
      while (f) {
        const int u = 64 * k + __ffsll((long long)f) - 1;
        f &= f - 1;
        VinaMask row = adj[u];
        if (u == a) row.clear(c);
        next.w[0] |= row.w[0];
        next.w[1] |= row.w[1];
      }
    }
    next.w[0] &= ~seen.w[0];
    next.w[1] &= ~seen.w[1];
    if (next.has(c)) return true;
    if (!next.any()) return false;
    seen.w[0] |= next.w[0];
    seen.w[1] |= next.w[1];
    front = next;
  }
}

__global__ __launch_bounds__(64) void vina_type_kernel(VinaTypeArgs p) {
  __shared__ signed char ord[kMolMaxAtoms * kMolMaxAtoms];     // the molecule's [n][n] block, row stride n
  __shared__ VinaMask adj[kMolMaxAtoms];
  __shared__ int cls[kMolMaxAtoms];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n_max = p.n_max;
  const int n_total = p.mol_off[p.batch];
  const int lo = p.mol_off[b], hi = p.mol_off[b + 1];
  const int size = (lo >= 0 && hi >= lo && hi <= n_total) ? hi - lo : 0;
  const int n = min(size, n_max);
  const signed char* src = p.order + (size_t)b * n_max * n_max;
  for (int idx = lane; idx < n * n; idx += 64) {
    const int a = idx / n, c = idx - a * n;
    ord[idx] = c < a ? src[a * n_max + c] : 0;
  }
  for (int a = lane; a < kMolMaxAtoms; a += 64) {
    int k = kVinaNone;
    if (a < n) {
      const int t = p.atom_type[(size_t)lo + a];
      if (t >= 0 && t < p.n_types) k = vina_class_of(p.class_elem[t]);
    }
    cls[a] = k;
  }
  for (int a = n_max + lane; a < size; a += 64) p.lig_code[(size_t)lo + a] = 0;     // past n_max: not read, untyped
  __syncthreads();
  // lanes own the atoms lane and lane + 64
  VinaMask carbon;
  carbon.w[0] = __ballot(cls[lane] == kVinaC);
  carbon.w[1] = __ballot(cls[lane + 64] == kVinaC);
  VinaMask single[2] = {{{0, 0}}, {{0, 0}}};
  int n_typed = 0, n_untyped = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int a = lane + 64 * h;
    if (a >= n) continue;
    VinaMask m{{0, 0}};
    int sum = 0, top = 0;
    for (int c = 0; c < n; ++c) {
      const int o = c < a ? ord[a * n + c] : ord[c * n + a];
      if (o >= 1 && o <= 3) {
        m.set(c);
        if (o == 1) single[h].set(c);
        sum += o;
        top = max(top, o);
      }
    }
    adj[a] = m;
    const int k = cls[a];
    int code = k;
    if (k == kVinaC) {
      if (!((m.w[0] & ~carbon.w[0]) | (m.w[1] & ~carbon.w[1]))) code |= kVinaHydrophobic;
    } else if (k == kVinaF || k == kVinaCl || k == kVinaBr || k == kVinaI) {
      code |= kVinaHydrophobic;
    } else if (k == kVinaN) {
      if (sum < 3) code |= kVinaDonor;
      if (sum == 3 && top >= 2) code |= kVinaAcceptor;
    } else if (k == kVinaO) {
      code |= kVinaAcceptor;
      if (sum < 2) code |= kVinaDonor;
    } else if (k == kVinaMetal) {
      code |= kVinaDonor;
    }
    p.lig_code[(size_t)lo + a] = code;
    n_typed += k != kVinaNone;
    n_untyped += k == kVinaNone;
  }
  __syncthreads();
  // rotors: the single bonds (a, c), c < a, of the lane's atoms
  int n_rot = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int a = lane + 64 * h;
    if (a >= n || adj[a].count() < 2) continue;
    for (int k = 0; k < 2; ++k) {
      mm_u64 f = single[h].w[k];
      while (f) {
        const int c = 64 * k + __ffsll((long long)f) - 1;
        f &= f - 1;
        if (c < a && adj[c].count() >= 2 && !vina_bond_in_ring(adj, a, c)) ++n_rot;
      }
    }
  }
  n_typed = mm_wave_sum(n_typed);
  n_untyped = mm_wave_sum(n_untyped);
  n_rot = mm_wave_sum(n_rot);
  if (lane == 0) {
    int* out = p.mol_int + (size_t)kVinaMolInt * b;
    out[0] = n_typed; out[1] = n_untyped; out[2] = n_rot; out[3] = 0;
  }
}

// ---- scoring -------------------------------------------------------------------------------------------------------------
struct VinaScoreArgs {
  PairBatch pairs;
  const int* lig_code;     // [N]
  const int* mol_int;      // [B][kVinaMolInt]: the rotors are read
  const int* poc_code;     // [M]
  float* atom_out;         // [N][kVinaTerms] unweighted terms
  float* mol_out;          // [B][kVinaMolOut]
  int* mol_flag;           // [B] nonfinite
};

constexpr double kVinaWeight[kVinaTerms] = {-0.035579, -0.005156, 0.840245, -0.035069, -0.587439};
constexpr double kVinaRotWeight = 0.05846;

// the five terms of one pair at surface distance d, added to t
__device__ inline void vina_pair_terms(double d, bool hydrophobic, bool hbond, double* t) {
  const double a = d * 2.0, c = (d - 3.0) * 0.5;
  t[0] += exp(-(a * a));
  t[1] += exp(-(c * c));
  if (d < 0.0) t[2] += d * d;
  if (hydrophobic) t[3] += d <= 0.5 ? 1.0 : (d < 1.5 ? 1.5 - d : 0.0);
  if (hbond) t[4] += d <= -0.7 ? 1.0 : (d < 0.0 ? -d / 0.7 : 0.0);
}

// 1 + 0.05846 N_rot of molecule b (a negative N_rot as 0)
__device__ inline double vina_rot_divisor(const int* mol_int, int b) {
  const int n_rot = max(mol_int[(size_t)kVinaMolInt * b + 2], 0);
  return 1.0 + kVinaRotWeight * (double)n_rot;
}

// every sum in float64, in the order pair_sweep fixes; the tiles before join before the store rounds, `inter` in term order
struct VinaPolicy {
  struct Atom { float x, y, z; int code, cls; double radius; };
  struct Record { double t[kVinaTerms]; };     // walked by fully unrolled loops only: it stays in registers
  struct Pair { float s, r; double d; bool hyd, hb; };
  using Total = Record;
  const VinaScoreArgs& p;
  Total* part;             // [kThreads / 64] in LDS

  __device__ static Record zero() { return {{0, 0, 0, 0, 0}}; }
  __device__ static Total zero_total() { return zero(); }
  __device__ float tile_word(size_t r) const { return __int_as_float(p.poc_code[r]); }
  __device__ Atom atom(size_t r, float x, float y, float z) const {
    const int code = p.lig_code[r], cls = vina_class_of(code);
    return {x, y, z, code, cls, vina_radius(cls)};
  }
  __device__ static bool skip(const Atom& a) { return a.cls == kVinaNone; }
  // does the pair count?  then its float32 squared distance and root, its surface distance and the terms that apply
  __device__ static bool counted(const Atom& a, const float4 q, Pair& v) {
    const int cj = __float_as_int(q.w), kj = vina_class_of(cj);
    if (kj == kVinaNone) return false;
    v.s = pair_dist2(a.x, a.y, a.z, q.x, q.y, q.z);
    if (!(v.s < 64.0f)) return false;                               // r < 8, strictly; false for NaN
    v.r = sqrtf(v.s);
    v.d = (double)v.r - a.radius - vina_radius(kj);
    v.hyd = (a.code & cj & kVinaHydrophobic) != 0;
    v.hb = ((a.code & kVinaDonor) && (cj & kVinaAcceptor)) || ((a.code & kVinaAcceptor) && (cj & kVinaDonor));
    return true;
  }
  __device__ static void pair(Record& acc, const Atom& a, const float4 q, int) {
    Pair v;
    if (counted(a, q, v)) vina_pair_terms(v.d, v.hyd, v.hb, acc.t);
  }
  __device__ static void fold(Record& acc, int o) {
    for (int k = 0; k < kVinaTerms; ++k) acc.t[k] += __shfl_xor(acc.t[k], o);
  }
  __device__ void carry(Record& acc, size_t r) const {
    const float* out = p.atom_out + kVinaTerms * r;
    for (int k = 0; k < kVinaTerms; ++k) acc.t[k] += (double)out[k];
  }
  __device__ void store(const Record& acc, size_t r) const {
    float* out = p.atom_out + kVinaTerms * r;
    for (int k = 0; k < kVinaTerms; ++k) out[k] = (float)acc.t[k];
  }
  __device__ static void merge(Total& s, const Total& o) {
    for (int k = 0; k < kVinaTerms; ++k) s.t[k] += o.t[k];
  }
  __device__ static void total(Total& w, const Record& acc, const Atom&) { merge(w, acc); }
  __device__ void finish(int b, int, const Total& s) const {
    float* mol = p.mol_out + (size_t)kVinaMolOut * b;
    double inter = 0.0;
    for (int k = 0; k < kVinaTerms; ++k) {
      mol[k] = (float)s.t[k];
      inter += kVinaWeight[k] * s.t[k];
    }
    mol[5] = (float)inter;
    mol[6] = (float)(inter / vina_rot_divisor(p.mol_int, b));
    mol[7] = 0.0f;
    p.mol_flag[b] = 0;
  }
};

// a molecule with a coordinate that is not finite: the flag, and NaN in every float it owns (the whole workgroup calls it
// and gets the same answer)
__device__ inline bool vina_nonfinite(const VinaScoreArgs& p, const PairRows& rows, int b) {
  const int tid = threadIdx.x;
  int bad = 0;
  for (int k = tid; k < 3 * rows.n; k += kThreads) bad |= pose_nonfinite(p.pairs.lig_x[3 * (size_t)rows.lo + k]);
  if (!__syncthreads_or(bad)) return false;
  const float nan = __builtin_nanf("");
  for (int k = tid; k < kVinaTerms * rows.n; k += kThreads) p.atom_out[kVinaTerms * (size_t)rows.lo + k] = nan;
  if (tid < kVinaMolOut) p.mol_out[(size_t)kVinaMolOut * b + tid] = nan;
  if (tid == 0) p.mol_flag[b] = 1;
  return true;
}

__global__ __launch_bounds__(kThreads) void vina_score_kernel(VinaScoreArgs p) {
  __shared__ VinaPolicy::Total part[kThreads / 64];
  const int b = blockIdx.x;
  const PairRows rows = pair_rows(p.pairs, b);
  if (vina_nonfinite(p, rows, b)) return;
  VinaPolicy pol{p, part};
  pair_sweep(p.pairs, rows, pol);
}

}  // namespace dsbdd
