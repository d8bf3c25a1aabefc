#!/usr/bin/env python
"""Golden vector of the learned noise schedule from the REAL reference: `GammaNetwork` (en_diffusion.py:1030-1102)
built under torch.manual_seed(3) -- its state_dict, gamma(t) at 17 random t and gamma(k / 40) for k = 0..40.
Run in the build container only:   python tests/golden/make_golden_gamma.py

  gamma_learned.npz   sd/<name> (the reference's parameters under its own names), t, gamma_t, gamma_table"""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle.ref_shim import import_reference  # noqa: E402

_, ref_ed, _, _ = import_reference()
torch.manual_seed(3)
with redirect_stdout(io.StringIO()):
    ref = ref_ed.GammaNetwork()
t = torch.rand(17, 1)
with torch.no_grad():
    out = {"sd/" + k: v.numpy() for k, v in ref.state_dict().items()}
    out.update(t=t.numpy(), gamma_t=ref(t).numpy(), gamma_table=ref(torch.arange(41).float().view(-1, 1) / 40).view(-1).numpy())
np.savez(os.path.join(HERE, "gamma_learned.npz"), **out)
print("gamma_learned.npz:", sorted(out))
