// Graph statistics of a batch of molecules, and the pair distances of their fingerprints: what the molecule-set metrics
// (diffsbdd_amd/metrics.py; the reference's analysis/metrics.py:52-125 and calculate_diversity) need of every sample, from
// the bond-order matrices that bond_orders_kernel (molecule.h) leaves on the device.
//
// mol_graph_kernel: one wave owns one molecule, all per-molecule state in LDS (dynamic, sized by n_max <= kMolMaxAtoms).
// Integer arithmetic only, no atomics; every output is a function of the molecule alone, so it is bitwise reproducible
// and does not depend on what else is in the batch or on n_max.  The numpy restatement in metrics.py is the specification;
// the two agree bit for bit.
//
// The graph key is a colour-refinement hash (uint64, wrapping):
//   c[a]  = mix(type[a] + 1), then for d = 1, 2, ...: c[a] = mix(c[a] ^ (d << 32 | #atoms at graph distance d of a))
//   n rounds r = 0..n-1:  c'[a] = mix(c[a] ^ mix(sum_b mix(4 c[b] + w(a,b)) + r))     b over a's neighbours
//   key(S) = mix(sum_{a in S} mix(c[a]) ^ |S|)
// w = bond order, or 1 with orders_in_key = 0.  The largest fragment's key is taken after |fragment| rounds and the whole
// sample's after n, so a fragment's key is the key of the same molecule generated alone.  Equal keys mean
// "refinement-equivalent": graphs that colour refinement cannot tell apart (prism / K3,3) share a key.
#pragma once
#include "common.h"

namespace dsbdd {

constexpr int kMolMaxAtoms = 128;   // largest supported n_max of mol_graph_kernel
constexpr int kMolStats = 8;        // ints per molecule: n_atoms, n_bonds, n_over_valence, n_fragments, largest size, largest label, 0, 0
constexpr int kFpWords = 64;        // 2048-bit fingerprint

typedef unsigned long long mm_u64;

struct MolGraphArgs {
  const signed char* order;   // [B][n_max][n_max] strictly lower triangular (bond_orders_kernel)
  const int* atom_type;       // [N]
  const int* mol_off;         // [B+1]
  const int* max_valence;     // [n_types], -1 = not checked
  int n_types, n_max, orders_in_key;
  int* valence;               // [N] sum of bond orders
  int* label;                 // [N] smallest atom index (within the molecule) of the atom's fragment
  int* stats;                 // [B][kMolStats]
  mm_u64* keys;               // [B][2]: largest fragment, whole sample
  unsigned* fp;               // [B][kFpWords]
  int* type_counts;           // [B][n_types]
};

// words per adjacency row: odd, so that consecutive rows start on different LDS banks
__host__ __device__ inline int mol_row_words(int n_max) { const int w = (n_max + 3) / 4; return w | 1; }
__host__ __device__ inline size_t mol_graph_lds_bytes(int n_max) {
  return (size_t)n_max * (2 * sizeof(mm_u64) + 2 * 4 * mol_row_words(n_max) + 5 * sizeof(int));
}

// splitmix64: the increment and the finaliser (mix(0) != 0)
__host__ __device__ inline mm_u64 mm_mix(mm_u64 x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ inline mm_u64 mm_wave_sum(mm_u64 v) {
  for (int o = 32; o; o >>= 1) v += (mm_u64)__shfl_xor((long long)v, o);
  return v;
}
__device__ inline int mm_wave_sum(int v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ inline int mm_wave_max(int v) {
  for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// f(b, order) for every neighbour b of the atom whose adjacency row (bytes, 4 per word) is `row`
template <class F>
__device__ inline void mm_for_neighbours(const unsigned* row, int n_words, F f) {
  for (int k = 0; k < n_words; ++k) {
    unsigned w = row[k];
    while (w) {
      const int byte = (__ffs((int)w) - 1) >> 3;
      f(4 * k + byte, (int)((w >> (8 * byte)) & 0xffu));
      w &= ~(0xffu << (8 * byte));
    }
  }
}

__global__ __launch_bounds__(64) void mol_graph_kernel(MolGraphArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mm_lds[];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n_max = p.n_max, ws = mol_row_words(n_max);
  const int lo = p.mol_off[b], n = max(min(p.mol_off[b + 1] - lo, n_max), 0);
  const int nw = (n + 3) / 4;
  // carve (every array n_max entries; 8-byte items first)
  mm_u64* cur = reinterpret_cast<mm_u64*>(mm_lds);
  mm_u64* nxt = cur + n_max;
  unsigned* adj = reinterpret_cast<unsigned*>(nxt + n_max);      // [n][ws] words = 4 orders each
  unsigned* dist = adj + (size_t)n_max * ws;                     // [n][ws] words = 4 BFS distances each (0xff = unreached)
  int* type = reinterpret_cast<int*>(dist + (size_t)n_max * ws);
  int* val = type + n_max;
  int* lab = val + n_max;
  int* fsize = lab + n_max;
  int* deg = fsize + n_max;
  const signed char* ord = p.order + (size_t)b * n_max * n_max;

  // the symmetric order matrix, four entries per word; entries past n are 0
  for (int idx = lane; idx < n * nw; idx += 64) {
    const int a = idx / nw, k = idx - a * nw;
    unsigned w = 0;
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * k + j;
      if (c < n && c != a) {
        const int o = a > c ? ord[a * n_max + c] : ord[c * n_max + a];
        if (o > 0) w |= (unsigned)o << (8 * j);
      }
    }
    adj[a * ws + k] = w;
    dist[a * ws + k] = 0xffffffffu;
  }
  for (int a = lane; a < n; a += 64) type[a] = p.atom_type[lo + a];
  __syncthreads();

  // valence, degree, one BFS per atom (its row of `dist` is the lane's own): fragment label and size, shell-profile seed
  int my_bonds = 0, my_over = 0;
  for (int a = lane; a < n; a += 64) {
    int v = 0, dg = 0;
    mm_for_neighbours(adj + a * ws, nw, [&](int, int o) { v += o; ++dg; });
    const int t = type[a];
    const int lim = (t >= 0 && t < p.n_types) ? p.max_valence[t] : -1;
    val[a] = v;
    deg[a] = dg;
    my_bonds += dg;
    my_over += lim >= 0 && v > lim;
    unsigned char* drow = reinterpret_cast<unsigned char*>(dist + a * ws);
    drow[a] = 0;
    mm_u64 c = mm_mix((mm_u64)(long long)t + 1ull);
    int reached = 1;
    for (int d = 0;; ++d) {
      int shell = 0;
      for (int u = 0; u < n; ++u)
        if (drow[u] == d)
          mm_for_neighbours(adj + u * ws, nw, [&](int v2, int) {
            if (drow[v2] == 0xff) { drow[v2] = (unsigned char)(d + 1); ++shell; }
          });
      if (!shell) break;
      reached += shell;
      c = mm_mix(c ^ (((mm_u64)(d + 1) << 32) | (mm_u64)shell));
    }
    int first = 0;
    while (drow[first] == 0xff) ++first;
    lab[a] = first;
    fsize[a] = reached;
    cur[a] = c;
    p.valence[lo + a] = v;
    p.label[lo + a] = first;
  }
  const int n_bonds = mm_wave_sum(my_bonds) / 2, n_over = mm_wave_sum(my_over);
  // fragments: the roots; the largest by (size, then smallest root)
  int my_roots = 0, my_best = -1;
  for (int a = lane; a < n; a += 64)
    if (lab[a] == a) { ++my_roots; my_best = max(my_best, fsize[a] * 256 + (255 - a)); }
  const int n_frags = mm_wave_sum(my_roots), best = mm_wave_max(my_best);
  const int big_size = best < 0 ? 0 : best >> 8, big_label = best < 0 ? -1 : 255 - (best & 255);
  __syncthreads();

  // the key: n rounds of colour refinement, the fragment's sum taken after big_size rounds
  mm_u64 frag_part = 0;
  for (int r = 0; r < n; ++r) {
    for (int a = lane; a < n; a += 64) {
      mm_u64 s = 0;
      mm_for_neighbours(adj + a * ws, nw, [&](int c, int o) { s += mm_mix(4ull * cur[c] + (mm_u64)(p.orders_in_key ? o : 1)); });
      nxt[a] = mm_mix(cur[a] ^ mm_mix(s + (mm_u64)r));
    }
    __syncthreads();
    mm_u64* t = cur; cur = nxt; nxt = t;
    if (r + 1 == big_size)
      for (int a = lane; a < n; a += 64)
        if (lab[a] == big_label) frag_part += mm_mix(cur[a]);
  }
  mm_u64 whole_part = 0;
  for (int a = lane; a < n; a += 64) whole_part += mm_mix(cur[a]);
  const mm_u64 key_frag = mm_mix(mm_wave_sum(frag_part) ^ (mm_u64)big_size);
  const mm_u64 key_whole = mm_mix(mm_wave_sum(whole_part) ^ (mm_u64)n);
  __syncthreads();

  // the fingerprint: colours of rounds 0, 1, 2 of a plain refinement seeded with (element, degree, valence); lane = word
  unsigned word = 0;
  for (int a = lane; a < n; a += 64)
    cur[a] = mm_mix((mm_u64)(long long)type[a] + 1ull + ((mm_u64)deg[a] << 16) + ((mm_u64)val[a] << 32));
  __syncthreads();
  for (int r = 0;; ++r) {
    for (int a = 0; a < n; ++a)
      if (lab[a] == big_label) {
        const unsigned bit = (unsigned)(cur[a] & 2047ull);
        if ((int)(bit >> 5) == lane) word |= 1u << (bit & 31u);
      }
    if (r == 2) break;
    for (int a = lane; a < n; a += 64) {
      mm_u64 s = 0;
      mm_for_neighbours(adj + a * ws, nw, [&](int c, int o) { s += mm_mix(4ull * cur[c] + (mm_u64)o); });
      nxt[a] = mm_mix(cur[a] ^ mm_mix(s + (mm_u64)(r + 1)));
    }
    __syncthreads();
    mm_u64* t = cur; cur = nxt; nxt = t;
  }
  p.fp[(size_t)b * kFpWords + lane] = word;

  for (int t = lane; t < p.n_types; t += 64) {
    int c = 0;
    for (int a = 0; a < n; ++a) c += type[a] == t;
    p.type_counts[(size_t)b * p.n_types + t] = c;
  }
  if (lane == 0) {
    int* st = p.stats + (size_t)b * kMolStats;
    st[0] = n; st[1] = n_bonds; st[2] = n_over; st[3] = n_frags; st[4] = big_size; st[5] = big_label; st[6] = 0; st[7] = 0;
    p.keys[2 * (size_t)b] = key_frag;
    p.keys[2 * (size_t)b + 1] = key_whole;
  }
}

// Tanimoto distances inside groups of fingerprints: one workgroup per group; wave w takes rows i = 1 + w, 5 + w, ..., a lane
// the partners j = lane, lane + 64, ... < i.  Every thread adds its pairs in that order, the 256 partial sums are folded by a
// fixed tree: the float64 sum is the same in every run.
__global__ __launch_bounds__(kThreads) void fp_diversity_kernel(const uint4* fp, const int* group_off, double* sum,
                                                                long long* pairs) {
  __shared__ double part[kThreads];
  const int g = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lo = group_off[g], m = max(group_off[g + 1] - lo, 0);
  double acc = 0.0;
  for (int i = 1 + wave; i < m; i += kThreads / 64) {
    const uint4* a = fp + (size_t)(lo + i) * (kFpWords / 4);
    for (int j = lane; j < i; j += 64) {
      const uint4* q = fp + (size_t)(lo + j) * (kFpWords / 4);
      int inter = 0, uni = 0;
#pragma unroll
      for (int k = 0; k < kFpWords / 4; ++k) {
        const uint4 x = a[k], y = q[k];
        inter += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
        uni += __popc(x.x | y.x) + __popc(x.y | y.y) + __popc(x.z | y.z) + __popc(x.w | y.w);
      }
      acc += uni ? 1.0 - (double)inter / (double)uni : 0.0;
    }
  }
  part[tid] = acc;
  __syncthreads();
  for (int s = kThreads / 2; s; s >>= 1) {
    if (tid < s) part[tid] += part[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    sum[g] = part[0];
    pairs[g] = (long long)m * (m - 1) / 2;
  }
}

}  // namespace dsbdd
