#!/usr/bin/env python3
"""Dev probe (GPU): the ZV kernel on device-resident arrays.  Fills samples and gradients [NKEPT][D][CHAINS] with
synthetic draws (a correlated Gaussian and a noisy, slightly non-linear gradient: the kernel's cost does not depend on
the values), runs mcmc_stats_zv WARMUP times, then times REPS calls with HIP events and reports the median: time,
algorithmic bytes (three reads of x and g, one write of zv) over time as a fraction of HBM peak, and the Gram pass's
fp64 MFMA work over the whole call's time (the kernel is fused, so this is a lower bound on that pass's rate).

  ORDER=1 D=32 NKEPT=90 CHAINS=1048576 python scripts/zv_probe.py     # the ESS leg's series shape
  ORDER=2 D=8 python scripts/zv_probe.py
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
FP64_MFMA_PEAK_TF = 78.6    # MI355X fp64 matrix, spec

order = int(os.environ.get("ORDER", "1"))
d = int(os.environ.get("D", "32"))
n = int(os.environ.get("NKEPT", "90"))
C = int(os.environ.get("CHAINS", 1 << 20))
reps = int(os.environ.get("REPS", "7"))
warmup = int(os.environ.get("WARMUP", "2"))
k = d * (d + 3) // 2 if order == 2 else d
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev)
gen.manual_seed(3)
x = torch.empty((n, d, C), dtype=torch.float64, device=dev)
g = torch.empty((n, d, C), dtype=torch.float64, device=dev)
for t in range(n):                                   # row by row: no temporaries of the arrays' size
    x[t].normal_(0.5, 1.0, generator=gen)
    g[t].normal_(0.0, 0.1, generator=gen)
    g[t].sub_(x[t] - 0.5).add_(0.3 * torch.tanh(x[t]))
torch.cuda.synchronize()
for _ in range(warmup):
    z, info = mc.stats.zv_device((x, g), order=order, return_info=True)
torch.cuda.synchronize()
ts = []
for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    z = mc.stats.zv_device((x, g), order=order)
    e1.record()
    torch.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
ms = statistics.median(ts)
arr = x.numel() * 8
bytes_alg = 7 * arr                                   # x and g read in each of three passes, zv written once
tiles = sum(1 for ti in range(-(-k // 16) + -(-d // 16)) for tj in range(-(-k // 16)) if tj <= ti)
gram_flop = C * tiles * -(-n // 4) * 2 * 16 * 16 * 4  # MFMAs issued by pass 2, padded tiles included
res = {"order": order, "d": d, "k": k, "nkept": n, "chains": C, "reps": reps, "ms_median": round(ms, 3),
       "ms_all": [round(t, 3) for t in ts], "array_GB": round(arr / 1e9, 3), "algorithmic_GB": round(bytes_alg / 1e9, 3),
       "TBps": round(bytes_alg / ms / 1e9, 3), "hbm_fraction": round(bytes_alg / ms / 1e9 / HBM_PEAK_TBS, 3),
       "gram_TFLOPs_over_whole_call": round(gram_flop / ms / 1e9, 2),
       "gram_fraction_of_fp64_mfma_peak": round(gram_flop / ms / 1e9 / FP64_MFMA_PEAK_TF, 3),
       "singular_chains": int((info != 0).sum().item()), "zv_finite": bool(torch.isfinite(z[:, :, :4096]).all().item())}
print(json.dumps(res), flush=True)
