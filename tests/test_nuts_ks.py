"""The reference's distribution suite with NUTS() (test/test_dists.jl:37): the 19 cases of test_dists_ks.py.

CPU, on the NUTS checker (tests/nuts_oracle.c):
- the reference's own criterion: one chain, SerialMC(1000:10000), KS measure < 10;
- the meaningful bound of test_dists_ks.py: 64 chains, every 100th kept sample pooled (5 824 draws), KS < 1.95 (the
  Kolmogorov distribution's 0.1 % critical value).  Every one of the 19 cases meets it on the checker (the largest
  pooled value is 1.43, TDist(2.2); the largest single-chain value 3.08, LogNormal(-1, 1)), so none is listed as an
  exception.

GPU (`-m gpu`): 1 024 chains of the same run on the HIP kernels; chain 0 bitwise the checker's single chain, and the
KS measure across the 1 024 independent chains at kept rows 4 500 and 9 000 below 1.95, for every case that passed
the pooled bound on the CPU (all 19).
"""
import numpy as np
import pytest

import mcmchip as mc
import nuts_ref as nr
from test_dists_ks import CASES, IDS, KS_CRIT_001, KSTHRESHOLD, RUNNER, case_model, ks_value

POOLED_MISSES = {}             # (name, params) -> (measured pooled KS, reason): none on the checker


def test_suite_is_the_references():
    assert len(CASES) == 19 and len(RUNNER.r) == 9001 and not POOLED_MISSES


@pytest.mark.parametrize("name,params,dist", CASES, ids=IDS)
def test_ks_checker(name, params, dist):
    m = case_model(name, params, dist)
    oc = nr.NutsChains(m, mc.NUTS(), nchains=64, seed=1)
    s = oc.run(RUNNER)["samples"]
    assert np.isfinite(s).all()
    ksv1 = ks_value(s[:, 0, 0], dist)                                       # the reference's own test (one chain)
    assert ksv1 < KSTHRESHOLD, f"NUTS on {name}{params}: KS {ksv1:.2f} (reference threshold 10)"
    ksv = ks_value(s[::100, 0, :], dist)                                    # 91 x 64 pooled draws
    if (name, params) not in POOLED_MISSES:
        assert ksv < KS_CRIT_001, f"NUTS on {name}{params}: pooled KS {ksv:.3f} > {KS_CRIT_001}"


@pytest.mark.gpu
@pytest.mark.parametrize("name,params,dist", CASES, ids=IDS)
def test_ks_hip(gpu, name, params, dist):
    m = case_model(name, params, dist)
    C = 1024
    chain = mc.run((m * mc.NUTS() * RUNNER).batch(C, seed=1))
    s = chain._samples                                                      # [9001][1][C]
    assert np.isfinite(s).all()
    o1 = nr.NutsChains(m, mc.NUTS(), nchains=1, seed=1).run(RUNNER)
    assert np.array_equal(s[:, :, :1].view(np.uint64), o1["samples"].view(np.uint64)), "chain 0 differs from the checker"
    assert np.array_equal(chain.diagnostics["ndoublings"][0], o1["ndoublings"][:, 0])
    assert np.array_equal(chain.diagnostics["epsilon"][0].view(np.uint64), o1["epsilon"][:, 0].copy().view(np.uint64))
    assert ks_value(s[:, 0, 0], dist) < KSTHRESHOLD
    if (name, params) in POOLED_MISSES:
        return
    for row in (4500, 9000):                                                # 1 024 independent draws each
        ksv = ks_value(s[row, 0, :], dist)
        assert ksv < KS_CRIT_001, f"NUTS on {name}{params}: KS across chains at kept row {row}: {ksv:.3f}"
