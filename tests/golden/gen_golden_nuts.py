"""Writes tests/golden/chains_normal3_nuts.npz from the NUTS checker (tests/nuts_oracle.c): 4 chains x 30 kept steps
of NUTS() on v ~ Normal(1, 2), d = 3, seed 1, with epsilon and ndoublings.  Run from the repository root:
    python tests/golden/gen_golden_nuts.py
tests/test_nuts.py checks the fixture against the checker (CPU) and against the HIP kernels (GPU)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "mcmc.jl_amd"), os.path.join(ROOT, "tests")]

import mcmchip as mc  # noqa: E402
import nuts_ref as nr  # noqa: E402

SEED = 1
m = mc.model(mc.NormalDSL(1, 2), v=np.ones(3), gradient=True)
out = nr.NutsChains(m, mc.NUTS(), 4, seed=SEED).run(mc.SerialMC(steps=30))
np.savez_compressed(os.path.join(HERE, "chains_normal3_nuts.npz"), seed=np.int64(SEED), samples=out["samples"],
                    grads=out["grads"], accept=out["accept"], epsilon=out["epsilon"], ndoublings=out["ndoublings"])
print("wrote chains_normal3_nuts.npz", out["samples"].shape)
