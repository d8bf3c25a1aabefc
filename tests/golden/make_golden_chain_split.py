"""Records tests/golden/chain_split_parent.npz: the row split of node_chain_kernel as the commit BEFORE csrc/chain_split.h
computed it -- per case the inputs, the header (Mw, total, V, Vs, forced; zeros when the kernel returns before the split)
and the flat list of (workgroup, first row, tiles) pieces; for the five large cases a SHA-256 of the list instead.

The split has no GPU dependency, so it is recorded on a CPU from the parent's own text, never from the code under test:
lines 369-557 of that commit's csrc/node_chain.h (from the read of *m_count to the end of the range loop) are taken out
of git and compiled UNCHANGED inside the host shim below -- std::min / std::max, blockIdx / gridDim as arguments,
chain_range replaced by a print, no floating-point contraction:

    python tests/golden/make_golden_chain_split.py [parent commit, default 0e8fbe8] [out.npz]

The shim reads and prints the text format of tools/chain_split_host.cpp, so the same cases can be piped through that
program (a sanitizer build of the header) and compared line by line."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHIM = r"""
#include <algorithm>
#include <cstdio>
#include <vector>
using std::min; using std::max;
constexpr int kChainMaxProj = 3, kChainRowsMax = 96;
struct Proj { int N; const int* count; int first; };
struct Args { const int* m_count; int M; int do_mlp; int n_proj; Proj proj[kChainMaxProj]; };
struct Dim { unsigned x; };
struct Out { unsigned hdr[5] = {0, 0, 0, 0, 0}; std::vector<int> pieces; };
static Out* g_out; static unsigned g_wg;
#define CHAIN_NOTE(slot, v) do { } while (0)
static unsigned long long wall_clock64() { return 0; }
template <int H, int RT> static void chain_range(const Args&, int r0, int, float*, const int*) {
  g_out->pieces.insert(g_out->pieces.end(), {(int)g_wg, r0, RT});
}
template <int H> static void body(Args p, Dim blockIdx, Dim gridDim) {
  float* smem = nullptr;
#include "parent_body.inc"
  const unsigned h[5] = {(unsigned)Mw, total, V, Vs, (unsigned)forced};
  for (int k = 0; k < 5; ++k) g_out->hdr[k] = h[k];
}
int main() {
  int c[14];
  for (;;) {
    for (int k = 0; k < 14; ++k) if (scanf("%d", &c[k]) != 1) return 0;
    Args p{nullptr, c[0], c[3], c[4], {}};
    for (int q = 0; q < 3; ++q) p.proj[q] = Proj{c[5 + 3 * q], c[6 + 3 * q] == 0x7fffffff ? nullptr : &c[6 + 3 * q], c[7 + 3 * q]};
    Out out; g_out = &out;
    for (g_wg = 0; g_wg < (unsigned)c[1]; ++g_wg) {
      if (c[2] == 256) body<256>(p, Dim{g_wg}, Dim{(unsigned)c[1]});
      else if (c[2] == 192) body<192>(p, Dim{g_wg}, Dim{(unsigned)c[1]});
      else if (c[2] == 128) body<128>(p, Dim{g_wg}, Dim{(unsigned)c[1]});
      else body<64>(p, Dim{g_wg}, Dim{(unsigned)c[1]});
    }
    printf("case %u %u %u %u %u %zu\n", out.hdr[0], out.hdr[1], out.hdr[2], out.hdr[3], out.hdr[4], out.pieces.size() / 3);
    for (size_t k = 0; k < out.pieces.size(); k += 3) printf("%d %d %d\n", out.pieces[k], out.pieces[k + 1], out.pieces[k + 2]);
  }
}
"""


def build_parent_shim(commit, workdir):
    src = subprocess.run(["git", "show", f"{commit}:diffsbdd_amd/csrc/node_chain.h"], cwd=ROOT, check=True,
                         capture_output=True, text=True).stdout.split("\n")
    body = src[368:557]
    assert body[0].lstrip().startswith("const int M = p.m_count") and body[-1] == "  }", (body[0], body[-1])
    with open(os.path.join(workdir, "parent_body.inc"), "w") as f:
        f.write("\n".join(body) + "\n")
    with open(os.path.join(workdir, "shim.cpp"), "w") as f:
        f.write(SHIM)
    exe = os.path.join(workdir, "shim")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "shim.cpp", "-o", exe],
                   cwd=workdir, check=True)
    return exe


def run_split_program(exe, rows):
    """Pipe cases (tests/_chain_split_cases.case_row) through a split program; returns [(header, pieces [n][3])]."""
    text = "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
    res, i = [], 0
    for _ in rows:
        head = out[i].split()
        assert head[0] == "case", out[i]
        n = int(head[6])
        pieces = np.array([ln.split() for ln in out[i + 1:i + 1 + n]], dtype=np.int32).reshape(n, 3)
        res.append((tuple(int(v) for v in head[1:6]), pieces))
        i += 1 + n
    return res


def main():
    from tests import _chain_split_cases as cs
    commit = sys.argv[1] if len(sys.argv) > 1 else "0e8fbe8"
    out = sys.argv[2] if len(sys.argv) > 2 else cs.GOLDEN
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_parent_shim(commit, tmp)
        rows = [cs.case_row(*c, H) for H in cs.HS for c in cs.listed_cases()]
        large = [cs.case_row(*c, H) for H in cs.HS for c in cs.LARGE]
        res, res_large = run_split_program(exe, rows), run_split_program(exe, large)
    off = np.cumsum([0] + [len(p) for _, p in res]).astype(np.int64)
    np.savez_compressed(out, cases=np.array(rows, dtype=np.int32), header=np.array([h for h, _ in res], dtype=np.int64),
                        piece_off=off, pieces=np.concatenate([p for _, p in res]),
                        large_cases=np.array(large, dtype=np.int32),
                        large_header=np.array([h for h, _ in res_large], dtype=np.int64),
                        large_pieces=np.array([len(p) for _, p in res_large], dtype=np.int64),
                        large_digest=np.array([cs.digest(p) for _, p in res_large]))
    forced = sum(h[4] for h, _ in res)
    print(f"wrote {len(rows)} + {len(large)} cases ({forced} forced, {off[-1]} pieces) of {commit} to {out}, "
          f"{os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
