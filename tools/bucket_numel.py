"""Writes the sizes of the trainable tensors of a workload's network, one per line: the layout of the optimiser's gradient
bucket, as tools/bench_optim_reduce.hip reads it.  No GPU needed.
    python tools/bucket_numel.py crossdock_fullatom_cond > numel.txt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import weights as W  # noqa: E402


def main(arch):
    from diffsbdd_amd.dynamics import EGNNDynamics
    cfg, _ = W.arch_cfg(arch)
    for p in EGNNDynamics(**cfg, device="cpu").parameters():
        if p.requires_grad:
            print(p.numel())


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "crossdock_fullatom_cond")
