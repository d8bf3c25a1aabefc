// Cost-weighted split of node_chain_kernel's row list (node_chain.h) into ranges of 16-row tiles: pure integer
// bookkeeping, identical in every workgroup, written once for both compilers -- the kernel builds it from its device
// scalars, dsbdd_chain_split_host and tools/chain_split_host.cpp run the same text on a CPU.  No HIP include, no HIP
// builtin; everything is inlined and the tables are only indexed by fully unrolled loops, so on the device they stay in
// scalar registers (out-of-line range functions measured slower).
// Cost of a row, in units of H*H/16 MAC: 48 for the node MLP + N_p / H * 16 for every projection that covers it.
// All of it in 32-bit arithmetic on wave-uniform values (rows x 240 units < 2^31: launch_node_chain rejects more than 8 M
// rows): round 3's 64-bit version -- bisection of the cumulative cost, 64-bit divisions -- cost every workgroup 7 us
// before its first load (in-kernel timeline, profiles/r4h_node_chain_timeline.md).
#pragma once

#ifdef __HIPCC__
#define CHAIN_SPLIT_FN __host__ __device__ __forceinline__
#else
#define CHAIN_SPLIT_FN inline
#endif
namespace dsbdd {
constexpr int kChainRowsMax = 96;      // rows a workgroup holds in LDS at a time (6 row tiles)
constexpr int kChainMaxProj = 3;
constexpr int kChainAllRows = 0x7fffffff;      // ChainSplitIn::count: the problem covers all rows that follow `first`
constexpr int kChainBreaks = 2 * kChainMaxProj + 3;
template <class T> CHAIN_SPLIT_FN T chain_min(T a, T b) { return b < a ? b : a; }
template <class T> CHAIN_SPLIT_FN T chain_max(T a, T b) { return a < b ? b : a; }
// ceil(a j / n) = (a / n) j + ceil((a % n) j / n): no 64-bit division
CHAIN_SPLIT_FN unsigned chain_share(unsigned a, unsigned j, unsigned n) { return a / n * j + (a % n * j + n - 1) / n; }

// What the kernel knows after reading its device scalars.
struct ChainSplitIn {
  int M;                          // logical rows, already min(M, *m_count)
  int do_mlp, n_proj;
  int N[kChainMaxProj];           // columns of projection q; it covers the logical rows [first, first + count)
  int first[kChainMaxProj];
  int count[kChainMaxProj];       // kChainAllRows: all that follow.  first / count are clamped to M here
  int H, grid;
};

struct ChainSplit {
  int cnt[kChainMaxProj], fst[kChainMaxProj];      // the clamped problems (chain_range needs cnt)
  unsigned wgt[kChainMaxProj], w_mlp;
  int n_proj, do_mlp, M;
  int Mw;                         // rows behind the last problem's end have no work
  unsigned total;                 // cost of [0, Mw)
  unsigned V, Vs;                 // ranges: planned (a multiple of the grid), and dealt out (forced: may differ)
  bool forced;
  int bpv[kChainBreaks];          // where the slope of the cumulative cost F changes, sorted ...
  unsigned Fb[kChainBreaks];      // ... and F there
  // forced only: the cuts in tiles, F at the cuts, ranges of the segment that starts at cut a
  int Tt, cut[kChainBreaks];
  unsigned fcut[kChainBreaks], nrg[kChainBreaks];

  // cumulative cost of the logical rows [0, r)
  CHAIN_SPLIT_FN unsigned cost_to(int r) const {
    unsigned f = w_mlp * (unsigned)chain_min(r, Mw);
#pragma unroll
    for (int q = 0; q < kChainMaxProj; ++q) f += wgt[q] * (unsigned)chain_max(0, chain_min(r - fst[q], cnt[q]));
    return f;
  }

  // The <= 8 places where a problem starts or ends, with 0 and `end` around them, sorted: in rows (the breakpoints of F)
  // or in TILES (the forced cuts: a start rounded down to a tile, an end rounded up, empty problems left out).
  template <bool TILES>
  CHAIN_SPLIT_FN void breaks(int (&b)[kChainBreaks], int end) const {
    int nb = 0;
    b[nb++] = 0;
#pragma unroll
    for (int q = 0; q < kChainMaxProj; ++q) {
      const bool on = q < n_proj && (!TILES || cnt[q] > 0);
      b[nb++] = on ? chain_min(end, TILES ? fst[q] >> 4 : fst[q]) : end;
      b[nb++] = on ? chain_min(end, TILES ? (fst[q] + cnt[q] + 15) >> 4 : fst[q] + cnt[q]) : end;
    }
    b[nb++] = do_mlp ? chain_min(end, TILES ? (M + 15) >> 4 : M) : end;
    b[nb++] = end;
#pragma unroll
    for (int a2 = 1; a2 < kChainBreaks; ++a2)              // insertion sort, fully unrolled (the array stays in registers)
#pragma unroll
      for (int b2 = kChainBreaks - 1; b2 > 0; --b2)
        if (b2 <= a2 && b[b2] < b[b2 - 1]) { const int tmp = b[b2]; b[b2] = b[b2 - 1]; b[b2 - 1] = tmp; }
  }

  CHAIN_SPLIT_FN explicit ChainSplit(const ChainSplitIn& in) {
    n_proj = in.n_proj; do_mlp = in.do_mlp; M = in.M;
    Mw = 0; total = 0; V = 0; Vs = 0; forced = false;
    if (M <= 0) return;
    w_mlp = do_mlp ? 48u : 0u;
    int M_work = do_mlp ? M : 0;
#pragma unroll
    for (int q = 0; q < kChainMaxProj; ++q) {              // (an unused slot: an empty problem of weight 0 at row 0)
      const bool on = q < n_proj;
      fst[q] = on ? chain_min(M, in.first[q]) : 0;
      cnt[q] = on ? chain_max(chain_min(M - fst[q], in.count[q]), 0) : 0;
      wgt[q] = on ? (unsigned)(in.N[q] * 16 / in.H) : 0u;
      M_work = chain_max(M_work, fst[q] + cnt[q]);
    }
    if (M_work <= 0) return;
    Mw = M_work;
    // F is piecewise linear: its slope only changes where a problem starts or ends
    breaks<false>(bpv, Mw);
#pragma unroll
    for (int a2 = 0; a2 < kChainBreaks; ++a2) Fb[a2] = cost_to(bpv[a2]);
    total = Fb[kChainBreaks - 1];
    if (total == 0) { Mw = 0; return; }                    // (no row has work: nothing is dealt out, as for M <= 0)
    // the cheapest row of the list = the smallest positive slope of a piece
    unsigned w_min = ~0u;
#pragma unroll
    for (int a2 = 0; a2 < kChainBreaks - 1; ++a2) {
      const int len = bpv[a2 + 1] - bpv[a2];
      if (len > 0 && Fb[a2 + 1] > Fb[a2]) w_min = chain_min(w_min, (Fb[a2 + 1] - Fb[a2]) / (unsigned)len);
    }
    if (w_min == ~0u || w_min == 0) w_min = 1;
    // number of ranges: a multiple of the grid, large enough that a range of the cheapest rows fits kChainRowsMax (the
    // boundaries are rounded UP to tiles, so a range has floor or ceil of (rows per range / 16) tiles, never more)
    const unsigned per_max = (unsigned)kChainRowsMax * w_min;
    V = (total + per_max - 1) / per_max;
    V = (V + (unsigned)in.grid - 1) / (unsigned)in.grid * (unsigned)in.grid;
    Vs = V;
    // Only for launches of >= 3 row tiles per workgroup: below that the ranges are 1 - 2 tiles, nothing straddles for long,
    // and the extra arithmetic (1.5 us) is what shows (measured: 19.8 k rows 165.5 -> 153.9 us, 11.5 k 109.6 -> 111.5,
    // 3.6 k 54.9 -> 57.8).
    Tt = (Mw + 15) >> 4;
    forced = Tt >= 3 * in.grid;
    if (forced) force_cuts();
  }

  // Forced cuts (round 4).  A range that STRADDLES the end of a projection problem multiplies all its row tiles for a
  // projection that covers some of them -- it was the slowest workgroup of every launch (171 vs 153 us in the timeline).
  // The row list is therefore cut at every problem's start (rounded down to a tile) and end (rounded up), and every
  // segment between two cuts gets its share of the V ranges by cost and splits them with the same inversion of F.
  CHAIN_SPLIT_FN void force_cuts() {
    constexpr int NC = kChainBreaks, kTilesMax = kChainRowsMax / 16;
    breaks<true>(cut, Tt);
#pragma unroll
    for (int a2 = 0; a2 < NC; ++a2) fcut[a2] = cost_to(chain_min(Mw, cut[a2] << 4));
    Vs = 0;
    int big = 0; unsigned cbig = 0;
#pragma unroll
    for (int a2 = 0; a2 < NC - 1; ++a2) {
      const unsigned c = fcut[a2 + 1] - fcut[a2];
      const int tiles = cut[a2 + 1] - cut[a2];
      unsigned n = 0;
      if (tiles > 0) {
        // the only floating-point step: a product, a correctly rounded division and a sum, which nothing can contract
        n = (unsigned)((float)c * (float)V / (float)total + 0.5f);
        n = chain_max(n, (unsigned)((tiles + kTilesMax - 1) / kTilesMax));      // every range fits the LDS panels
        n = chain_min(chain_max(n, 1u), (unsigned)tiles);
        if (c > cbig) { cbig = c; big = a2; }
      }
      nrg[a2] = n; Vs += n;
    }
    nrg[NC - 1] = 0;
    // the ranges left over (or borrowed) by the rounding go to (come from) the most expensive segment
#pragma unroll
    for (int a2 = 0; a2 < NC - 1; ++a2)
      if (a2 == big && Vs != V) {
        const int tiles = cut[a2 + 1] - cut[a2];
        const int lo_n = (tiles + kTilesMax - 1) / kTilesMax;
        int n = (int)nrg[a2] + (int)V - (int)Vs;
        n = chain_min(chain_max(n, chain_max(lo_n, 1)), tiles);
        Vs = Vs - nrg[a2] + (unsigned)n;
        nrg[a2] = (unsigned)n;
      }
  }

  // first row (multiple of 16) whose cumulative cost reaches y: F inverted piece by piece, one 32-bit division
  CHAIN_SPLIT_FN int row_at(unsigned y) const {
    constexpr int NB = kChainBreaks;
    if (y == 0) return 0;
    if (y > total) return (Mw + 15) / 16 * 16;
    // the piece [b[a], b[a + 1]) with F(b[a]) < y <= F(b[a + 1]): the first a whose end reaches y (F is non-decreasing,
    // F(b[0]) = 0 < y); pieces of zero length or zero slope can never be it
    int base = bpv[NB - 2], bnext = bpv[NB - 1];
    unsigned fbase = Fb[NB - 2], fnext = Fb[NB - 1];
    bool found = false;
#pragma unroll
    for (int a2 = 0; a2 < NB - 1; ++a2)
      if (!found && Fb[a2 + 1] >= y) { found = true; base = bpv[a2]; bnext = bpv[a2 + 1]; fbase = Fb[a2]; fnext = Fb[a2 + 1]; }
    const int len = bnext - base;
    int r = bnext;
    if (len > 0 && fnext > fbase) {
      const unsigned slope = (fnext - fbase) / (unsigned)len;   // exact: the cost per row is constant inside a piece
      r = base + (int)((y - fbase + slope - 1) / slope);
    }
    return (r + 15) / 16 * 16;
  }

  // (Mw, total, V, Vs, forced) as the entry points report it; all zero when nothing is dealt out
  CHAIN_SPLIT_FN void report(unsigned* h) const { h[0] = (unsigned)Mw; h[1] = total; h[2] = V; h[3] = Vs; h[4] = forced; }

  // Rows [r0, r1) of range v (both multiples of 16; r1 <= r0: nothing).  False past the last range.
  CHAIN_SPLIT_FN bool range(unsigned v, int& r0, int& r1) const {
    if (v >= Vs) return false;
    if (!forced) {
      r0 = v == 0 ? 0 : row_at(chain_share(total, v, V));
      r1 = v + 1 == V ? (Mw + 15) / 16 * 16 : row_at(chain_share(total, v + 1, V));
      return true;
    }
    // segment and position of range v
    unsigned j = v, ns = 1, f0 = 0, cseg = 0;
    int b0 = 0, b1 = Tt;
    bool found = false;
#pragma unroll
    for (int a2 = 0; a2 < kChainBreaks - 1; ++a2) {
      if (!found && j < nrg[a2]) { found = true; ns = nrg[a2]; f0 = fcut[a2]; cseg = fcut[a2 + 1] - fcut[a2]; b0 = cut[a2]; b1 = cut[a2 + 1]; }
      if (!found) j -= nrg[a2];
    }
    if (!found) return false;
    r0 = j == 0 ? (b0 << 4) : chain_min(chain_max(row_at(f0 + chain_share(cseg, j, ns)), b0 << 4), b1 << 4);
    r1 = j + 1 == ns ? (b1 << 4) : chain_min(chain_max(row_at(f0 + chain_share(cseg, j + 1, ns)), b0 << 4), b1 << 4);
    return true;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// Second policy (DSBDD_OPT_CHAIN_DEAL, DESIGN.md §5 "Min-max deal"): the same inputs, dealt by the load a workgroup EXECUTES.
// chain_range multiplies all tiles of a piece for every projection the piece touches, so the tile list is cut at every
// problem's start (rounded down to a tile) and end (rounded up) at every launch size, and inside a segment between two cuts
// every tile costs the same: u = 48 (node MLP) + N_p * 16 / H for every problem whose tile range holds the segment, x 16
// rows.  Every range is k_s consecutive tiles of one segment (the segment's last range: what is left).
//   * FALLBACK, a pure function of the launch's counts (Tt tiles, S segments with tiles, grid): with 8 S > grid and
//     Tt >= 3 grid ChainSplit deals the launch (its forced path: the same cuts, several ranges per workgroup).  One range
//     per workgroup cannot balance S segments over fewer than 8 S workgroups as well as that does (measured on the listed
//     cases of tests/_chain_split_cases.py: up to 2.5 x its slowest load at grid 2 / 3 / 8, never above it from grid 104);
//     no engine launch is that narrow;
//   * at most `grid` tiles: every tile is a range of its own.  The same where the segments outnumber the workgroups
//     (S > grid, so grid < 8) in a launch too small for the fallback: workgroup w then takes the tiles w, w + grid, ...;
//   * else the smallest bottleneck b for which sum_s ceil(T_s / floor(b / u_s)) ranges fit the grid: b starts at the
//     lower bound max(u_max, ceil(sum T_s u_s / grid)) and steps through the values at which some floor(b / u_s) grows --
//     the only values at which the sum can change -- so the first b that fits is the optimum (1 + 2 S divisions to start,
//     one per step; about S^2 Tt / grid^2 + S steps).  One range per workgroup; ranges of more than kChainRowsMax rows go
//     on as pieces (chain_pieces);
//   * ranges that do not fill the grid leave workgroups idle: by the minimality of b no further cut lowers the bottleneck.
// 32-bit arithmetic on wave-uniform values: sum T_s u_s <= tiles x 240 < 2^32 up to 17.8 M tiles (286 M rows; the entry
// points and launch_node_chain stop at 8 M rows).  The tables are only indexed by fully unrolled loops.
constexpr int kDealCuts = 2 * kChainMaxProj + 2;      // 0, the problems' starts and ends, the last tile's end
constexpr int kChainSegs = kDealCuts - 1;

struct ChainDeal {
  int cnt[kChainMaxProj];         // the clamped counts, as ChainSplit has them (chain_range needs them)
  int Mw, Tt;                     // rows with work (as ChainSplit::Mw) and their tiles
  int cut[kDealCuts];             // the cuts in tiles, sorted
  unsigned k[kChainSegs];         // tiles per range of the segment that starts at cut a
  unsigned nrg[kChainSegs];       // its ranges
  unsigned B;                     // the slowest range's executed load (units of H*H/16 MAC)
  unsigned Vs;                    // ranges dealt out
  bool fallback;                  // nothing is dealt out here: ChainSplit deals this launch (ChainDealt)

  CHAIN_SPLIT_FN explicit ChainDeal(const ChainSplitIn& in) {
    Mw = 0; Tt = 0; B = 0; Vs = 0; fallback = false;
#pragma unroll
    for (int q = 0; q < kChainMaxProj; ++q) cnt[q] = 0;
    const int M = in.M;
    if (M <= 0) return;
    const unsigned w_mlp = in.do_mlp ? 48u : 0u;
    int M_work = in.do_mlp ? M : 0;
    bool work = in.do_mlp != 0;
    unsigned wgt[kChainMaxProj];
    int lo[kChainMaxProj];
#pragma unroll
    for (int q = 0; q < kChainMaxProj; ++q) {              // (an unused slot: an empty problem of weight 0 at row 0)
      const bool on = q < in.n_proj;
      lo[q] = on ? chain_max(in.first[q], 0) : 0;
      const int fst = chain_min(M, lo[q]);
      cnt[q] = on ? chain_max(chain_min(M - fst, in.count[q]), 0) : 0;
      wgt[q] = on ? (unsigned)(in.N[q] * 16 / in.H) : 0u;
      M_work = chain_max(M_work, fst + cnt[q]);
      work = work || (wgt[q] > 0 && cnt[q] > 0);
    }
    if (M_work <= 0 || !work) return;                      // (no row has work: nothing is dealt out, as in ChainSplit)
    Mw = M_work;
    Tt = (Mw + 15) >> 4;
    // the tiles chain_range multiplies for problem q: those that touch [first, first + cnt) -- for an EMPTY problem whose
    // first is no multiple of 16 still the tile around it (chain_range does not look at the count alone)
    int t0[kChainMaxProj], t1[kChainMaxProj];
#pragma unroll
    for (int q = 0; q < kChainMaxProj; ++q) {
      const int l = chain_min(lo[q], Tt << 4);
      t0[q] = chain_min(Tt, l >> 4);
      t1[q] = chain_min(Tt, (l + cnt[q] + 15) >> 4);
    }
    {
      int nb = 0;
      cut[nb++] = 0;
#pragma unroll
      for (int q = 0; q < kChainMaxProj; ++q) { cut[nb++] = t0[q]; cut[nb++] = t1[q]; }
      cut[nb++] = Tt;
#pragma unroll
      for (int a2 = 1; a2 < kDealCuts; ++a2)               // insertion sort, fully unrolled (the array stays in registers)
#pragma unroll
        for (int b2 = kDealCuts - 1; b2 > 0; --b2)
          if (b2 <= a2 && cut[b2] < cut[b2 - 1]) { const int tmp = cut[b2]; cut[b2] = cut[b2 - 1]; cut[b2 - 1] = tmp; }
    }
    // cost of a tile of every segment (/ 16), segments with tiles, their sum and their most expensive tile
    unsigned u[kChainSegs], S = 0, total = 0, u_max = 0;
#pragma unroll
    for (int a2 = 0; a2 < kChainSegs; ++a2) {
      const unsigned T = (unsigned)(cut[a2 + 1] - cut[a2]);
      unsigned c = w_mlp;
#pragma unroll
      for (int q = 0; q < kChainMaxProj; ++q) c += cut[a2] >= t0[q] && cut[a2] < t1[q] ? wgt[q] : 0u;      // (every t0, t1 is a cut)
      u[a2] = c; k[a2] = 1; nrg[a2] = T;
      S += T > 0; total += T * c;
      if (T > 0) u_max = chain_max(u_max, c);
    }
    const unsigned G = (unsigned)in.grid;
    fallback = 8 * S > G && (unsigned)Tt >= 3 * G;
    if (fallback) return;
    if ((unsigned)Tt <= G || S > G) { Vs = (unsigned)Tt; B = 16 * u_max; return; }      // every tile a range of its own
    // many tiles: the smallest bottleneck b (/ 16) whose ranges fit the grid
    unsigned b = chain_max(u_max, (total + G - 1) / G);
    Vs = 0;
#pragma unroll
    for (int a2 = 0; a2 < kChainSegs; ++a2) {
      const unsigned T = (unsigned)(cut[a2 + 1] - cut[a2]);
      if (T > 0) {
        k[a2] = u[a2] > 0 ? chain_min(b / u[a2], T) : T;   // (a segment without work: one range)
        nrg[a2] = (T + k[a2] - 1) / k[a2];
        Vs += nrg[a2];
      }
    }
#pragma unroll 1
    while (Vs > G) {
      unsigned nb = ~0u;
#pragma unroll
      for (int a2 = 0; a2 < kChainSegs; ++a2)
        if (k[a2] < (unsigned)(cut[a2 + 1] - cut[a2])) nb = chain_min(nb, (k[a2] + 1) * u[a2]);
      b = nb;
#pragma unroll
      for (int a2 = 0; a2 < kChainSegs; ++a2) {
        const unsigned T = (unsigned)(cut[a2 + 1] - cut[a2]);
        if (k[a2] < T && (k[a2] + 1) * u[a2] == b) {
          Vs -= nrg[a2];
          k[a2] += 1;
          nrg[a2] = (T + k[a2] - 1) / k[a2];
          Vs += nrg[a2];
        }
      }
    }
    (void)b;
#pragma unroll
    for (int a2 = 0; a2 < kChainSegs; ++a2)
      if (cut[a2 + 1] > cut[a2]) B = chain_max(B, 16 * u[a2] * chain_min(k[a2], (unsigned)(cut[a2 + 1] - cut[a2])));
  }


  // Rows [r0, r1) of range v (both multiples of 16).  False past the last range.  No division.  With more ranges than
  // workgroups every range is a single tile, range v = tile v (node_chain_kernel relies on it for its later rounds).
  CHAIN_SPLIT_FN bool range(unsigned v, int& r0, int& r1) const {
    if (v >= Vs) return false;
    unsigned j = v, kk = 1;
    int b0 = 0, b1 = 0;
    bool found = false;
#pragma unroll
    for (int a2 = 0; a2 < kChainSegs; ++a2) {
      if (!found && j < nrg[a2]) { found = true; kk = k[a2]; b0 = cut[a2]; b1 = cut[a2 + 1]; }
      if (!found) j -= nrg[a2];
    }
    if (!found) return false;
    r0 = (b0 + (int)(j * kk)) << 4;
    r1 = chain_min(b1, b0 + (int)((j + 1) * kk)) << 4;
    return true;
  }
};

// What a launch with the option at 1 runs, for the entry points (node_chain_kernel does the same with shorter lifetimes):
// ChainDeal, or ChainSplit where that falls back.
struct ChainDealt {
  ChainDeal dl;
  ChainSplit sp;
  unsigned Vs, grid;
  CHAIN_SPLIT_FN explicit ChainDealt(const ChainSplitIn& in) : dl(in), sp(dl.fallback ? in : ChainSplitIn{}) {
    Vs = dl.fallback ? sp.Vs : dl.Vs; grid = (unsigned)in.grid;
  }
  CHAIN_SPLIT_FN bool range(unsigned v, int& r0, int& r1) const { return dl.fallback ? sp.range(v, r0, r1) : dl.range(v, r0, r1); }
  // (Mw, B executed load of the slowest range -- 0 in the fallback --, grid, Vs, fallback); all zero when nothing is dealt out
  CHAIN_SPLIT_FN void report(unsigned* h) const {
    h[0] = (unsigned)dl.Mw; h[1] = dl.B; h[2] = dl.Mw > 0 ? grid : 0u; h[3] = Vs; h[4] = dl.fallback;
  }
};

// The pieces of at most kChainRowsMax rows a workgroup walks for the rows [r0, r1): piece(first row, tiles).
// (At most one piece unless the rounding overshoots.)
template <class F>
CHAIN_SPLIT_FN void chain_pieces(int r0, int r1, F&& piece) {
  for (int nt = (r1 - r0) / 16, rs = r0; nt > 0;) {
    const int take = nt > kChainRowsMax / 16 ? kChainRowsMax / 16 : nt;
    piece(rs, take);
    rs += 16 * take; nt -= take;
  }
}

// A split (ChainSplit or ChainDealt) as the entry points report it: the (workgroup, first row, tiles) triples of the
// workgroups [0, wg_end) of a launch of `grid`, workgroup by workgroup; those of workgroup `own` (~0u: of all) are written to pieces[capacity][3].
// Returns the number of pieces of [0, wg_end).
template <class Split>
CHAIN_SPLIT_FN long long chain_split_list(const Split& sp, unsigned grid, unsigned wg_end, unsigned own, int* pieces,
                                          long long capacity) {
  long long n = 0;
  for (unsigned wg = 0; wg < wg_end; ++wg)
    for (unsigned v = wg; v < sp.Vs; v += grid) {
      int r0, r1;
      if (!sp.range(v, r0, r1)) break;
      chain_pieces(r0, r1, [&](int rs, int take) {
        if ((own == ~0u || own == wg) && n < capacity) { pieces[3 * n] = (int)wg; pieces[3 * n + 1] = rs; pieces[3 * n + 2] = take; }
        ++n;
      });
    }
  return n;
}

}  // namespace dsbdd
