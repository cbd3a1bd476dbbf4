#!/usr/bin/env python3
"""Dev probe (GPU): describe on device-resident arrays, beside mcmc_stats_ess on the same arrays in the same session.
Fills samples [NKEPT][D][CHAINS] with a synthetic AR(1) draw per series (so Geyer's scan runs a few pairs, as on real
chains), then for each shape times with HIP events, WARMUP calls first, the median of REPS:

  ess           mcmc_stats_ess (IMSE)                                      -- the yardstick
  per_chain     mcmc_stats_describe, the per-chain table alone             -- the fused per-series pass
  pooled_noq    mcmc_stats_describe, pooled rows alone, no quantiles       -- the pass (5 workspace columns) + reduction
  pooled_q      the same with PROBS quantiles                              -- ... + the radix select
  select        pooled_q - pooled_noq: 8 passes over the samples

and reports bytes over time as a fraction of HBM peak.  A time is that of the whole Python call (the library runs on its
own stream and synchronises before returning, so the events bracket host-serialised time): it includes torch.empty of the
outputs and, with the pooled table, the workspace's hipMalloc / hipFree inside mcmc_stats_describe.  Writes OUT (default profiles/describe_probe.json).

  python scripts/describe_probe.py                       # the metric's 2^20 x 32 x 90, and d = 3
  SHAPES=65536x32x90 python scripts/describe_probe.py
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mcmc.jl_amd"))
import mcmchip as mc  # noqa: E402

HBM_PEAK_TBS = 8.0          # MI355X HBM3E, spec
PASSES = 8                  # k_desc_hist: 8 digits of 8 bits

shapes = [tuple(int(v) for v in s.split("x")) for s in
          os.environ.get("SHAPES", f"{1 << 20}x32x90,{1 << 20}x3x90").split(",")]
reps = int(os.environ.get("REPS", "5"))
warmup = int(os.environ.get("WARMUP", "2"))
probs = tuple(float(p) for p in os.environ.get("PROBS", "0.025,0.5,0.975").split(","))
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "describe_probe.json"))
dev = torch.device("cuda", 0)


def timed(fn):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), [round(t, 3) for t in ts]


results = []
for C, d, n in shapes:
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    x = torch.empty((n, d, C), dtype=torch.float64, device=dev)
    x[0].normal_(0.0, 1.0, generator=gen)
    for t in range(1, n):                                # row by row: no temporaries of the array's size
        x[t].normal_(0.0, 0.6, generator=gen)
        x[t].add_(x[t - 1], alpha=0.8)
    torch.cuda.synchronize()
    arr, col = x.numel() * 8, d * C * 8
    legs = {
        "ess": (lambda: mc.stats.ess_device(x, "imse"), arr + col),
        "per_chain": (lambda: mc.stats.describe_device(x, probs=(), pooled=False), arr + 6 * col),
        "pooled_noq": (lambda: mc.stats.describe_device(x, probs=(), per_chain=False), arr + 10 * col),
        "pooled_q": (lambda: mc.stats.describe_device(x, probs=probs, per_chain=False), arr + 10 * col + PASSES * arr),
    }
    res = {"chains": C, "d": d, "nkept": n, "reps": reps, "warmup": warmup, "probs": probs,
           "array_GB": round(arr / 1e9, 3)}
    ms = {}
    for name, (fn, nbytes) in legs.items():
        ms[name], all_ms = timed(fn)
        res[name] = {"ms_median": round(ms[name], 3), "ms_all": all_ms, "algorithmic_GB": round(nbytes / 1e9, 3),
                     "hbm_fraction": round(nbytes / ms[name] / 1e9 / HBM_PEAK_TBS, 3)}
    sel = ms["pooled_q"] - ms["pooled_noq"]
    res["per_chain_over_ess_time"] = round(ms["per_chain"] / ms["ess"], 3)
    res["per_chain_over_ess_bytes"] = round((arr + 6 * col) / (arr + col), 3)
    res["select"] = {"ms": round(sel, 3), "passes": PASSES, "algorithmic_GB": round(PASSES * arr / 1e9, 3),
                     "hbm_fraction": round(PASSES * arr / sel / 1e9 / HBM_PEAK_TBS, 3) if sel > 0 else None}
    r = mc.stats.describe_device(x, probs=probs)
    res["pooled_mean_first"] = float(r.pooled["mean"][0].item())
    res["rhat_first"] = float(r.pooled["rhat"][0].item())
    res["nbad_total"] = int(r.nbad.sum().item())
    print(json.dumps(res), flush=True)
    results.append(res)
    del x, r
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
