// Intramolecular term of the Vina-type score: the five terms of vina_score.h and their gradient (vina_grad.h) over the
// ligand-ligand pairs that vina_torsion_kernel listed (vina_torsion.h: both typed, more than 3 bonds apart, separated by a
// kept rotor).  One launch, one workgroup per molecule, pair_sweep (pair_sweep.h) with the molecule's own rows as its
// "pocket group": the tile holds the molecule's coordinates and codes, and the policy counts a pair only if the bit of the
// tile index pair() receives is set in the atom's 128-bit mask (an index at or above 128 is never set).  Everything else is
// VinaGradPolicy's: the same float32 distance and strict cutoff r < 8, the same terms, weights, radii, flags and one-sided
// derivatives in float64, a pair with r = 0 adds to the terms and nothing to the gradient.
//
// Per atom: the five unweighted sums over its partners and g_i = sum_j (sum_k w_k T_k'(d_ij)) u_ij.  Per molecule: half the
// sum over the atoms of each term (every pair is met from both of its ends, the halving is exact), and intra = sum_k w_k T_k.
// Sums in float64 in the order pair_sweep fixes, stored as float32; no atomics, bitwise reproducible, independent of the
// batch.  A molecule with a coordinate that is not finite: the flag, NaN in every float it owns, as vina_grad_kernel.
#pragma once
#include "vina_grad.h"
#include "vina_torsion.h"

namespace dsbdd {

struct VinaIntraArgs {
  VinaGradArgs out;        // score.pairs: lig_x and mol_off on both sides; score.poc_code = score.lig_code; score.atom_out [N][5],
                           // score.mol_out [B][8] = the five sums, intra, 0, 0, score.mol_flag [B], atom_grad [N][3] are
                           // written; score.mol_int and mol_grad are not read or written
  const int* pair_mask;    // [N][kVinaMaskWords]
};

// the molecule's rows as both sides of the sweep, range-checked as pair_rows checks them
__device__ inline PairRows intra_rows(const PairBatch& p, int b) {
  const int n_total = p.mol_off[p.batch];
  const int lo = p.mol_off[b], hi = p.mol_off[b + 1];
  const int n = (lo >= 0 && hi >= lo && hi <= n_total) ? hi - lo : 0;
  return {lo, n, lo, n};
}

struct VinaIntraPolicy {
  struct Atom { VinaPolicy::Atom a; VinaMask mask; };
  using Record = VinaGradPolicy::Record;
  using Total = VinaPolicy::Total;
  const VinaIntraArgs& p;
  const VinaGradPolicy grad;   // on p.out: the records go through its calls
  Total* part;                 // [kThreads / 64] in LDS

  __device__ static Record zero() { return VinaGradPolicy::zero(); }
  __device__ static Total zero_total() { return VinaPolicy::zero_total(); }
  __device__ float tile_word(size_t r) const { return __int_as_float(p.out.score.lig_code[r]); }
  __device__ Atom atom(size_t r, float x, float y, float z) const {
    return {grad.atom(r, x, y, z), vina_mask_load(p.pair_mask + kVinaMaskWords * r)};
  }
  __device__ static bool skip(const Atom& a) { return VinaPolicy::skip(a.a) || !a.mask.any(); }
  __device__ static void pair(Record& acc, const Atom& a, const float4 q, int j) {
    if (j < kMolMaxAtoms && a.mask.has(j)) VinaGradPolicy::pair(acc, a.a, q, j);
  }
  __device__ static void fold(Record& acc, int o) { VinaGradPolicy::fold(acc, o); }
  __device__ void carry(Record& acc, size_t r) const { grad.carry(acc, r); }
  __device__ void store(const Record& acc, size_t r) const { grad.store(acc, r); }
  __device__ static void merge(Total& s, const Total& o) { VinaPolicy::merge(s, o); }
  __device__ static void total(Total& w, const Record& acc, const Atom&) { VinaPolicy::merge(w, acc.t); }
  __device__ void finish(int b, int, const Total& s) const {
    float* mol = p.out.score.mol_out + (size_t)kVinaMolOut * b;
    double intra = 0.0;
    for (int k = 0; k < kVinaTerms; ++k) {
      const double t = 0.5 * s.t[k];                                // every pair was met from both ends
      mol[k] = (float)t;
      intra += kVinaWeight[k] * t;
    }
    mol[5] = (float)intra;
    mol[6] = mol[7] = 0.0f;
    p.out.score.mol_flag[b] = 0;
  }
};

// the whole workgroup: NaN rows and the flag for a molecule that is not finite (true), else the sweep
__device__ inline bool vina_intra_nonfinite(const VinaIntraArgs& p, const PairRows& rows, int b) {
  if (!vina_nonfinite(p.out.score, rows, b)) return false;
  const float nan = __builtin_nanf("");
  for (int k = threadIdx.x; k < 3 * rows.n; k += kThreads) p.out.atom_grad[3 * (size_t)rows.lo + k] = nan;
  return true;
}

__global__ __launch_bounds__(kThreads) void vina_intra_kernel(VinaIntraArgs p) {
  __shared__ VinaIntraPolicy::Total part[kThreads / 64];
  const int b = blockIdx.x;
  const PairRows rows = intra_rows(p.out.score.pairs, b);
  if (vina_intra_nonfinite(p, rows, b)) return;
  VinaIntraPolicy pol{p, {p.out, {p.out.score, nullptr}, nullptr}, part};
  pair_sweep(p.out.score.pairs, rows, pol);
}

}  // namespace dsbdd
