// The torsion tree of a batch of ligands and the pair list of their intramolecular term, from the inputs of vina_type_kernel
// (vina_score.h): one launch, one wave per molecule, integers only, on the 128-bit adjacency masks of the typing kernel.
//
// Rotors are what vina_type_kernel counts as N_rot: a bond (a, c), c < a, of order 1, both ends of heavy degree >= 2, whose
// ends are not connected once it is cut.  They are enumerated in ascending (a, c); the first kVinaMaxTorsions are kept,
// and `found` is the number of all of them (= mol_int[2] of vina_type_kernel on the same input).  A molecule longer than
// n_max keeps none: it is a rigid body to everything that reads the tree, and its pair masks are empty.
//
// Moving side S_k of rotor k: cut the bond; of the two components that hold its ends, the one with fewer atoms, on a tie
// the one of the higher-index end a.  Stored as a 128-bit mask with the pair (p_k, m_k) = (fixed end, moving end in S_k).
// Any two sides are nested or disjoint.  Rotors of different connected components have disjoint sides.  Two rotors j, k of
// one component of n_c atoms cut it into X - j - Y - k - Z with X, Y, Z not empty; the only choice that overlaps without
// nesting is S_j = Y + Z and S_k = X + Y, which needs |Y| + |Z| <= |X| and |X| + |Y| <= |Z|, hence 2 |Y| <= 0.  So the rotors
// form a forest by inclusion, and a rotation about one axis moves every axis inside its side rigidly along with it.
//
// Pair mask of atom i, 128 bits: j is set iff i != j, both are typed (class_elem of their type, as vina_type_kernel reads
// it), j is more than 3 bonds from i or not connected to it, and some kept rotor has exactly one of i, j in its side.
// Symmetric by construction; empty for every atom of a molecule without kept rotors.
//
// Masks are written as four int32 words, atom 32 w + b = bit b of word w.
#pragma once
#include "vina_score.h"

namespace dsbdd {

constexpr int kVinaMaxTorsions = 32;
constexpr int kVinaTorInt = 4;      // ints per molecule: rotors kept, rotors found, 0, 0
constexpr int kVinaMaskWords = 4;   // int32 words of a 128-bit mask

struct VinaTorsionArgs {
  const signed char* order;   // as VinaTypeArgs
  const int* atom_type;
  const int* mol_off;
  const int* class_elem;
  int batch, n_types, n_max;
  int* tor_int;               // [B][kVinaTorInt]
  int* tor_end;               // [B][kVinaMaxTorsions][2]: fixed end, moving end (atoms of the molecule); -1 past the kept
  int* tor_side;              // [B][kVinaMaxTorsions][kVinaMaskWords]: S_k; 0 past the kept
  int* pair_mask;             // [N][kVinaMaskWords]
};

__device__ inline void vina_mask_store(int* out, const VinaMask& m) {
  out[0] = (int)(unsigned)m.w[0]; out[1] = (int)(unsigned)(m.w[0] >> 32);
  out[2] = (int)(unsigned)m.w[1]; out[3] = (int)(unsigned)(m.w[1] >> 32);
}
__device__ inline VinaMask vina_mask_load(const int* in) {
  return {{(mm_u64)(unsigned)in[0] | ((mm_u64)(unsigned)in[1] << 32), (mm_u64)(unsigned)in[2] | ((mm_u64)(unsigned)in[3] << 32)}};
}
// the first n atoms
__device__ inline VinaMask vina_mask_first(int n) {
  VinaMask m;
  m.w[0] = n >= 64 ? ~0ull : (n > 0 ? (1ull << n) - 1 : 0);
  m.w[1] = n >= 128 ? ~0ull : (n > 64 ? (1ull << (n - 64)) - 1 : 0);
  return m;
}
// the union of the rows of `adj` over the atoms base + (the set bits of f)
__device__ inline void vina_join_rows(VinaMask& out, const VinaMask* adj, mm_u64 f, int base) {
  while (f) {
    const int u = base + __ffsll((long long)f) - 1;
    f &= f - 1;
    out.w[0] |= adj[u].w[0];
    out.w[1] |= adj[u].w[1];
  }
}
// the union of the rows of `adj` over the atoms of `of` (the two words by name: a mask indexed by a loop variable would
// live in scratch)
__device__ inline VinaMask vina_neighbours(const VinaMask* adj, const VinaMask& of) {
  VinaMask out{{0, 0}};
  vina_join_rows(out, adj, of.w[0], 0);
  vina_join_rows(out, adj, of.w[1], 64);
  return out;
}
// the atoms connected to a when the bond (a, c) is left out (a itself included)
__device__ inline VinaMask vina_cut_side(const VinaMask* adj, int a, int c) {
  VinaMask seen{{0, 0}}, front{{0, 0}};
  seen.set(a);
  front = adj[a];
  front.clear(c);
  front.clear(a);
  while (front.any()) {
    seen.w[0] |= front.w[0];
    seen.w[1] |= front.w[1];
    VinaMask next = vina_neighbours(adj, front);
    next.w[0] &= ~seen.w[0];
    next.w[1] &= ~seen.w[1];
    front = next;
  }
  return seen;
}

__global__ __launch_bounds__(64) void vina_torsion_kernel(VinaTorsionArgs p) {
  __shared__ signed char ord[kMolMaxAtoms * kMolMaxAtoms];     // the molecule's [n][n] block, row stride n
  __shared__ VinaMask adj[kMolMaxAtoms];
  __shared__ VinaMask rot[kMolMaxAtoms];                       // the lower ends c of the rotors (a, c) of atom a
  __shared__ VinaMask side[kVinaMaxTorsions];
  __shared__ int cls[kMolMaxAtoms];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n_max = p.n_max;
  const int n_total = p.mol_off[p.batch];
  const int lo = p.mol_off[b], hi = p.mol_off[b + 1];
  const bool valid = lo >= 0 && hi >= lo && hi <= n_total;
  const int size = valid ? hi - lo : 0;
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
  __syncthreads();
  // lanes own the atoms lane and lane + 64
  VinaMask typed;
  typed.w[0] = __ballot(cls[lane] != kVinaNone);
  typed.w[1] = __ballot(cls[lane + 64] != kVinaNone);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int a = lane + 64 * h;
    VinaMask m{{0, 0}};
    if (a < n)
      for (int c = 0; c < n; ++c) {
        const int o = c < a ? ord[a * n + c] : ord[c * n + a];
        if (o >= 1 && o <= 3) m.set(c);
      }
    adj[a] = m;
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int a = lane + 64 * h;
    VinaMask r{{0, 0}};
    if (a < n && adj[a].count() >= 2)
      for (int c = 0; c < a; ++c)                                   // the bonds of order 1 to a lower atom, read from `ord` again
        if (ord[a * n + c] == 1 && adj[c].count() >= 2 && !vina_bond_in_ring(adj, a, c)) r.set(c);
    rot[a] = r;
  }
  if (lane < kVinaMaxTorsions) side[lane] = VinaMask{{0, 0}};
  __syncthreads();
  // the place of every rotor in ascending (a, c): the rotors of the atoms before a, then those of a with a lower c
  int found = 0;
  for (int a = 0; a < n; ++a) found += rot[a].count();
  const int kept = size > n_max ? 0 : min(found, kVinaMaxTorsions);
  int* ends = p.tor_end + (size_t)2 * kVinaMaxTorsions * b;
  int* sides = p.tor_side + (size_t)kVinaMaskWords * kVinaMaxTorsions * b;
  if (lane < kVinaMaxTorsions) {
    ends[2 * lane] = ends[2 * lane + 1] = -1;
    for (int w = 0; w < kVinaMaskWords; ++w) sides[kVinaMaskWords * lane + w] = 0;
  }
  if (lane == 0) {
    int* out = p.tor_int + (size_t)kVinaTorInt * b;
    out[0] = kept; out[1] = found; out[2] = 0; out[3] = 0;
  }
  __syncthreads();                                                  // the -1 and 0 rows, before a lane writes a kept rotor's
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int a = lane + 64 * h;
    if (a >= n) continue;
    int at = 0;
    for (int e = 0; e < a; ++e) at += rot[e].count();
    for (int k = 0; k < 2 && at < kept; ++k) {
      mm_u64 f = rot[a].w[k];
      while (f && at < kept) {
        const int c = 64 * k + __ffsll((long long)f) - 1;
        f &= f - 1;
        const VinaMask of_a = vina_cut_side(adj, a, c), of_c = vina_cut_side(adj, c, a);
        const bool a_moves = of_a.count() <= of_c.count();          // on a tie the side of the higher-index end
        side[at] = VinaMask{{a_moves ? of_a.w[0] : of_c.w[0], a_moves ? of_a.w[1] : of_c.w[1]}};     // word by word: no struct behind a pointer
        ends[2 * at] = a_moves ? c : a;
        ends[2 * at + 1] = a_moves ? a : c;
        vina_mask_store(sides + kVinaMaskWords * at, side[at]);
        ++at;
      }
    }
  }
  __syncthreads();
  // pair masks
  const VinaMask all = vina_mask_first(n);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int a = lane + 64 * h;
    if (a >= n) continue;
    VinaMask m{{0, 0}};
    if (cls[a] != kVinaNone && kept > 0) {
      VinaMask cut{{0, 0}};                                         // atoms a kept rotor separates from a
      for (int k = 0; k < kept; ++k) {
        const VinaMask s = side[k];
        const mm_u64 flip = s.has(a) ? ~0ull : 0ull;                // a inside: the atoms outside
        cut.w[0] |= s.w[0] ^ flip;
        cut.w[1] |= s.w[1] ^ flip;
      }
      VinaMask near{{0, 0}};                                        // a and the atoms within 3 bonds of it
      near.set(a);
      for (int d = 0; d < 3; ++d) {
        const VinaMask next = vina_neighbours(adj, near);
        near.w[0] |= next.w[0];
        near.w[1] |= next.w[1];
      }
      m.w[0] = cut.w[0] & ~near.w[0] & typed.w[0] & all.w[0];
      m.w[1] = cut.w[1] & ~near.w[1] & typed.w[1] & all.w[1];
    }
    vina_mask_store(p.pair_mask + kVinaMaskWords * ((size_t)lo + a), m);
  }
  for (int a = n_max + lane; a < size; a += 64)                     // past n_max: no pairs
    for (int w = 0; w < kVinaMaskWords; ++w) p.pair_mask[kVinaMaskWords * ((size_t)lo + a) + w] = 0;
}

}  // namespace dsbdd
