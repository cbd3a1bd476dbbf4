#!/usr/bin/env python3
"""Dev probe (GPU): RMHMC against PMALA on the logistic model of test/test_syntax.jl's shape (n = 1 000, d = 10,
link_sign = -1, the `binomial` bench shape), CHAINS chains, STEPS steps per repetition after WARMUP steps.  Reports, per
sampler, the HIP-event time of the step kernels (mcmc_outputs.kernel_ms) of REPS repetitions: median and spread,
chain-steps/s and acceptance; for RMHMC also the leapfrogs a repetition took (mcmc_chains_evals), leapfrogs/s and the
cost of one leapfrog in PMALA steps.  PMALA(H) is the yardstick, from the same script on the same build.

  CHAINS=65536 STEPS=100 WARMUP=100 REPS=5 python scripts/rmhmc_probe.py
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc.jl_amd"))
import mcmchip as mc  # noqa: E402

n, d = int(os.environ.get("N", "1000")), int(os.environ.get("D", "10"))
C = int(os.environ.get("CHAINS", 1 << 16))
steps = int(os.environ.get("STEPS", "100"))
warmup = int(os.environ.get("WARMUP", "100"))
reps = int(os.environ.get("REPS", "5"))
h = float(os.environ.get("H", "0.5"))
nleaps, leapstep, nnewton = int(os.environ.get("NLEAPS", "6")), float(os.environ.get("LEAPSTEP", "0.5")), \
    int(os.environ.get("NNEWTON", "4"))

rng = np.random.default_rng(0)
X = np.hstack([np.ones((n, 1)), rng.standard_normal((n, d - 1))])
beta = rng.standard_normal(d) * 0.5
Y = (rng.random(n) < 1.0 / (1.0 + np.exp(X @ beta))).astype(np.float64)
m = mc.model(mc.LogisticRegression(X, Y, link_sign=-1.0), vars=np.zeros(d), gradient=True, tensor=True, dtensor=True)

res = {"n": n, "d": d, "chains": C, "steps": steps, "warmup": warmup, "reps": reps, "h": h,
       "rmhmc_args": [nleaps, leapstep, nnewton]}
for name, sp in (("rmhmc", mc.RMHMC(nleaps, leapstep, nnewton)), ("pmala", mc.PMALA(h))):
    t = (m * sp * mc.SerialMC(steps=warmup, burnin=warmup - 1)).batch(C, seed=1)
    mc.run(t)
    t.runner = mc.SerialMC(steps=steps, burnin=steps - 1)          # one kept step: the timing is the step kernels'
    ts, acc, leaps = [], [], []
    for _ in range(reps):
        e0 = t.evals
        ch = mc.run(t)
        ts.append(ch.kernel_ms)
        acc.append(float(ch.diagnostics["accept"].mean()))
        leaps.append(t.evals - e0)
    ms = statistics.median(ts)
    res[name] = {"kernel": t.step_kernel, "ms_median": round(ms, 3), "ms_all": [round(v, 3) for v in ts],
                 "spread": round((max(ts) - min(ts)) / ms, 4), "chain_steps_per_s": round(C * steps / ms * 1e3, 1),
                 "accept_last_step": round(statistics.mean(acc), 3)}
    if name == "rmhmc":
        lf = statistics.median(leaps)
        res[name]["leapfrogs_per_rep"] = lf
        res[name]["leapfrogs_per_s"] = round(lf / ms * 1e3, 1)
r, p = res["rmhmc"], res["pmala"]
res["rmhmc_leapfrog_in_pmala_steps"] = round((r["ms_median"] / r["leapfrogs_per_rep"]) / (p["ms_median"] / (C * steps)), 3)
print(json.dumps(res), flush=True)
