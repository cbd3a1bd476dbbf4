#!/usr/bin/env python3
"""Dev probe (GPU): PMALA against SMMALA on the logistic model of test/test_syntax.jl's shape (n = 1 000, d = 10,
link_sign = -1, the `binomial` bench shape), CHAINS chains, STEPS steps per repetition after WARMUP steps.  Reports, per
sampler, the HIP-event time of the step kernels (mcmc_outputs.kernel_ms) of REPS repetitions: median and spread,
chain-steps/s, acceptance, and the fp64 work against the 78.6 TF fp64 matrix peak: per evaluation SMMALA's pass counts
2 n d_pad^2 + 4 n d flop (tensor, eta, gradient); PMALA's second pass (invG X', eta, X' (w o qf)) counts the same again.
The second pass's 16 reduction MFMAs a tile (A = 1) are not counted as work.

  CHAINS=65536 STEPS=100 WARMUP=100 REPS=5 python scripts/pmala_probe.py
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc.jl_amd"))
import mcmchip as mc  # noqa: E402

FP64_MFMA_PEAK_TF = 78.6    # MI355X fp64 matrix, spec

n, d, d_pad = int(os.environ.get("N", "1000")), int(os.environ.get("D", "10")), 16
C = int(os.environ.get("CHAINS", 1 << 16))
steps = int(os.environ.get("STEPS", "100"))
warmup = int(os.environ.get("WARMUP", "100"))
reps = int(os.environ.get("REPS", "5"))
h = float(os.environ.get("H", "0.5"))

rng = np.random.default_rng(0)
X = np.hstack([np.ones((n, 1)), rng.standard_normal((n, d - 1))])
beta = rng.standard_normal(d) * 0.5
Y = (rng.random(n) < 1.0 / (1.0 + np.exp(X @ beta))).astype(np.float64)
m = mc.model(mc.LogisticRegression(X, Y, link_sign=-1.0), vars=np.zeros(d), gradient=True, tensor=True, dtensor=True)

res = {"n": n, "d": d, "chains": C, "steps": steps, "warmup": warmup, "reps": reps, "h": h}
for name, sp, passes in (("pmala", mc.PMALA(h), 2), ("smmala", mc.SMMALA(h), 1)):
    t = (m * sp * mc.SerialMC(steps=warmup, burnin=warmup - 1)).batch(C, seed=1)
    mc.run(t)
    t.runner = mc.SerialMC(steps=steps, burnin=steps - 1)          # one kept step: the timing is the step kernels'
    ts, acc = [], []
    for _ in range(reps):
        ch = mc.run(t)
        ts.append(ch.kernel_ms)
        acc.append(float(ch.diagnostics["accept"].mean()))
    ms = statistics.median(ts)
    flop = C * steps * passes * (2 * n * d_pad * d_pad + 4 * n * d)
    res[name] = {"kernel": t.step_kernel, "ms_median": round(ms, 3), "ms_all": [round(v, 3) for v in ts],
                 "spread": round((max(ts) - min(ts)) / ms, 4), "chain_steps_per_s": round(C * steps / ms * 1e3, 1),
                 "accept_last_step": round(statistics.mean(acc), 3), "fp64_TFLOPs": round(flop / ms / 1e9, 3),
                 "fraction_of_fp64_mfma_peak": round(flop / ms / 1e9 / FP64_MFMA_PEAK_TF, 4)}
res["pmala_over_smmala"] = round(res["pmala"]["ms_median"] / res["smmala"]["ms_median"], 3)
print(json.dumps(res), flush=True)
