// The node chain's row split (csrc/chain_split.h) as a stand-alone host program: the header includes nothing of HIP, so
// this builds with any C++17 compiler -- in particular with the sanitizers that cannot run on device code:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/chain_split_host.cpp -o tools/bin/chain_split_host
//   (clang++: add -fsanitize=unsigned-integer-overflow to see where the 32-bit products wrap)
//
// stdin: one case per line, 14 integers: M grid H do_mlp n_proj, then (N count first) for three projection slots
// (count 2147483647 = all rows that follow; tests/_chain_split_cases.case_row writes this format).
// stdout: "case Mw total V Vs forced n_pieces", then n_pieces lines "workgroup first_row tiles" --
// what tests/golden/make_golden_chain_split.py reads back.  With the argument `deal` the second policy (ChainDealt) runs
// instead and the case line reads "case Mw B grid Vs fallback n_pieces".
// Host code only: no GPU is involved, and it is not part of the test suite.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../diffsbdd_amd/csrc/chain_split.h"

template <class Split>
static void print_split(const dsbdd::ChainSplitIn& in) {
  const Split sp(in);
  unsigned header[5];
  sp.report(header);
  const long long n = dsbdd::chain_split_list(sp, in.grid, in.grid, ~0u, nullptr, 0);
  std::vector<int> pieces(3 * (size_t)n + 3);
  dsbdd::chain_split_list(sp, in.grid, in.grid, ~0u, pieces.data(), n);
  printf("case %u %u %u %u %u %lld\n", header[0], header[1], header[2], header[3], header[4], n);
  for (long long k = 0; k < n; ++k) printf("%d %d %d\n", pieces[3 * k], pieces[3 * k + 1], pieces[3 * k + 2]);
}

int main(int argc, char** argv) {
  const bool deal = argc > 1 && !strcmp(argv[1], "deal");
  int c[14];
  for (;;) {
    for (int k = 0; k < 14; ++k)
      if (scanf("%d", &c[k]) != 1) return 0;
    if (c[1] < 1 || c[2] < 1 || c[4] < 0 || c[4] > dsbdd::kChainMaxProj) { fprintf(stderr, "bad case\n"); return 1; }
    dsbdd::ChainSplitIn in{};
    in.M = c[0]; in.grid = c[1]; in.H = c[2]; in.do_mlp = c[3]; in.n_proj = c[4];
    for (int q = 0; q < dsbdd::kChainMaxProj; ++q) { in.N[q] = c[5 + 3 * q]; in.count[q] = c[6 + 3 * q]; in.first[q] = c[7 + 3 * q]; }
    if (deal) print_split<dsbdd::ChainDealt>(in);
    else print_split<dsbdd::ChainSplit>(in);
  }
}
