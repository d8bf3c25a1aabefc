"""Records tests/golden/small_kernels_parent.json: what the small kernels of a sampling call produced BEFORE they were
rewritten -- eps_lig of one ligand-output-only call (lig_head_kernel) and z_lig / xh_pocket after one keyed reverse step
(cond_step_keyed_kernel) -- as SHA-256 digests of the float32 bytes plus the first rows.

Run on a GPU against a build of the parent commit, never against the code under test:

    DSBDD_LIB=/path/to/parent/libdiffsbdd_hip.so python tests/golden/make_golden_small_kernels.py [out.json]

(the parent's kernels with the read-out entry point dsbdd_engine_list2_read added, which the binding expects).  The
inputs are the seeded problems of tests/test_gpu_small_kernels.py, which compares the same calls against this file."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    if not os.environ.get("DSBDD_LIB"):
        raise SystemExit("set DSBDD_LIB to a build of the parent commit")
    from tests import test_gpu_small_kernels as t
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    rec = {name: t.digest(a) for name, a in t.parent_cases().items()}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(rec)} entries to {out}")


if __name__ == "__main__":
    main()
