#!/usr/bin/env python3
"""Dev probe (GPU): ERMLMC and RMLMC against RMHMC at equal nLeaps on the logistic model of test/test_syntax.jl's shape
(n = 1 000, d = 10, link_sign = -1, the `binomial` bench shape), CHAINS chains, STEPS steps per repetition after WARMUP
steps.  Reports, per sampler, the HIP-event time of the step kernels (mcmc_outputs.kernel_ms) of REPS repetitions:
median and spread, chain-steps/s, acceptance, the leapfrogs a repetition took (mcmc_chains_evals), leapfrogs/s, and the
passes over X one leapfrog makes (lmc.hip's and rmhmc.hip's headers: ERMLMC 6, RMLMC nNewton + 4, RMHMC 2 nNewton + 2).
RMHMC(NLEAPS, LEAPSTEP, NNEWTON), `rm_step`, is the yardstick, from the same script on the same build.

  CHAINS=65536 STEPS=100 WARMUP=100 REPS=5 python scripts/lmc_probe.py
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
nleaps, leapstep, nnewton = int(os.environ.get("NLEAPS", "6")), float(os.environ.get("LEAPSTEP", "0.5")), \
    int(os.environ.get("NNEWTON", "4"))

rng = np.random.default_rng(0)
X = np.hstack([np.ones((n, 1)), rng.standard_normal((n, d - 1))])
beta = rng.standard_normal(d) * 0.5
Y = (rng.random(n) < 1.0 / (1.0 + np.exp(X @ beta))).astype(np.float64)
m = mc.model(mc.LogisticRegression(X, Y, link_sign=-1.0), vars=np.zeros(d), gradient=True, tensor=True, dtensor=True)

res = {"n": n, "d": d, "chains": C, "steps": steps, "warmup": warmup, "reps": reps,
       "args": [nleaps, leapstep, nnewton]}
samplers = (("ermlmc", mc.ERMLMC(nleaps, leapstep), 6), ("rmlmc", mc.RMLMC(nleaps, leapstep, nnewton), nnewton + 4),
            ("rmhmc", mc.RMHMC(nleaps, leapstep, nnewton), 2 * nnewton + 2))
for name, sp, passes in samplers:
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
    lf = statistics.median(leaps)
    res[name] = {"kernel": t.step_kernel, "ms_median": round(ms, 3), "ms_all": [round(v, 3) for v in ts],
                 "spread": round((max(ts) - min(ts)) / ms, 4), "chain_steps_per_s": round(C * steps / ms * 1e3, 1),
                 "accept_last_step": round(statistics.mean(acc), 3), "leapfrogs_per_rep": lf,
                 "leapfrogs_per_s": round(lf / ms * 1e3, 1), "passes_per_leapfrog": passes}
for name in ("ermlmc", "rmlmc"):
    res[name + "_leapfrog_in_rmhmc_leapfrogs"] = round(
        (res[name]["ms_median"] / res[name]["leapfrogs_per_rep"]) /
        (res["rmhmc"]["ms_median"] / res["rmhmc"]["leapfrogs_per_rep"]), 3)
print(json.dumps(res), flush=True)
