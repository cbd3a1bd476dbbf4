"""What the host runtime reads from its sampler table and chain-state table (csrc/host/tables.hpp): the refusal
messages in full, and mcmc_chains_fork's copy of every live buffer for the samplers no other fork test covers."""
import ctypes as ct
import functools

import numpy as np
import pytest

import mcmchip as mc
import smmala_cases as sc
from mcmchip import _lib

pytestmark = pytest.mark.gpu
R = mc.SerialMC(steps=4)


@functools.lru_cache(maxsize=None)
def logistic3():
    """logistic d = 3, n = 8, with gradient, tensor and tensor derivatives"""
    X, Y = sc.data(8, 3, 1)
    return mc.model(mc.LogisticRegression(X, Y), vars=np.zeros(3), gradient=True, tensor=True, dtensor=True)


SAMPLERS = {"RWM": lambda: mc.RWM(0.1), "SMMALA": lambda: mc.SMMALA(0.5), "PMALA": lambda: mc.PMALA(0.5),
            "RMHMC": lambda: mc.RMHMC(), "ERMLMC": lambda: mc.ERMLMC(), "RMLMC": lambda: mc.RMLMC()}


def task(name):
    return (logistic3() * SAMPLERS[name]() * R).batch(16, seed=1)


def last_error():
    return _lib.load().mcmc_last_error().decode()


SEQMC_REFUSALS = {
    "SMMALA": "SeqMC does not run SMMALA targets: the sampler's reset hook keeps invG and firstTerm of the chain's "
              "previous position (SMMALA.jl:54-57)",
    "PMALA": "SeqMC does not run PMALA targets: the sampler's reset hook keeps invG, firstTerm and secondTerm of the "
             "chain's previous position (PMALA.jl:63-66)",
    "RMHMC": "SeqMC does not run RMHMC targets: the population runner's device path is built for the samplers without "
             "a metric tensor",
    "ERMLMC": "SeqMC does not run ERMLMC targets: the sampler's reset hook keeps invG, cholG, traceInvGxdG, dphi and C "
              "of the chain's previous position (ERMLMC.jl:64-67), which mcmc_chains_set_state does not",
    "RMLMC": "SeqMC does not run RMLMC targets: the sampler's reset hook keeps invG, cholG, traceInvGxdG, dphi and C "
             "of the chain's previous position (ERMLMC.jl:64-67), which mcmc_chains_set_state does not",
}


@pytest.mark.parametrize("name", list(SEQMC_REFUSALS))
def test_seqmc_refusal_message(gpu, name):
    t = task(name)
    targets = (ct.c_void_p * 1)(t.handle())
    cfg = (ct.c_char * 24)()                               # mcmc_seqmc_cfg: steps 2, burnin 0, trigger 0.1
    ct.memmove(cfg, (ct.c_int64 * 2)(2, 0), 16)
    ct.memmove(ct.addressof(cfg) + 16, ct.addressof(ct.c_double(0.1)), 8)
    parts = np.zeros((3, 16))
    rc = _lib.load().mcmc_run_seqmc(targets, 1, 16, parts.ctypes.data, ct.addressof(cfg), ct.c_uint64(1), 0, None, None,
                                    None, None)
    assert rc == _lib.MCMC_E_UNSUPPORTED
    assert last_error() == SEQMC_REFUSALS[name]


LEAPS_REFUSALS = {
    "RMHMC": (_lib.MCMC_E_UNSUPPORTED, "storeLeaps is not built for RMHMC: the reference's RMHMC keeps no leapfrog "
                                       "record (RMHMC.jl:120-155)"),
    "ERMLMC": (_lib.MCMC_E_UNSUPPORTED, "storeLeaps is not built for ERMLMC: the reference's sampler keeps no leapfrog "
                                        "record (ERMLMC.jl:114-152)"),
    "RMLMC": (_lib.MCMC_E_UNSUPPORTED, "storeLeaps is not built for RMLMC: the reference's sampler keeps no leapfrog "
                                       "record (ERMLMC.jl:114-152)"),
    "RWM": (_lib.MCMC_E_INVALID_ARG, "storeLeaps needs an HMC or HMCDA sampler"),
}


@pytest.mark.parametrize("name", list(LEAPS_REFUSALS))
def test_store_leaps_refusal_message(gpu, name):
    t = task(name)
    buf = np.zeros(2 * 3 * 16)
    nl = np.zeros(16, dtype=np.int32)
    rc = _lib.load().mcmc_chains_store_leaps(t.handle(), 1, _lib.dptr(buf), _lib.dptr(buf), _lib.dptr(buf),
                                             _lib.dptr(buf), _lib.dptr(buf), nl.ctypes.data)
    assert (rc, last_error()) == LEAPS_REFUSALS[name]


def test_manifold_state_refusal_messages(gpu):
    g = np.zeros((3, 16))
    lib = _lib.load()
    rc = lib.mcmc_chains_manifold_state(task("RWM").handle(), _lib.dptr(g), None, None, None, None)
    assert (rc, last_error()) == (_lib.MCMC_E_INVALID_ARG, "chains do not run the SMMALA or PMALA sampler")
    rc = lib.mcmc_chains_manifold_state(task("SMMALA").handle(), None, None, None, None, _lib.dptr(g))
    assert (rc, last_error()) == (_lib.MCMC_E_INVALID_ARG, "SMMALA keeps no drift correction")


# ------------------------------------------------------------------ fork
def _tuner():
    return mc.EmpiricalMCMCTuner(0.7, adaptStep=2, maxStep=6)


FORK_SAMPLERS = {"mala_tuned": lambda: mc.MALA(0.4, _tuner()), "hmc_tuned": lambda: mc.HMC(3, 0.3, _tuner()),
                 "hmcda": lambda: mc.HMCDA(len=0.6, max_leaps=20), "ram": lambda: mc.RAM(0.3)}


@functools.lru_cache(maxsize=None)
def fork_model(layout):
    if layout == "lane":
        return mc.model(mc.IsoNormalDot(), init=np.ones(3), grad=True)
    if layout == "wave":
        return mc.model(mc.IsoNormalDot(), init=np.ones(40), grad=True)
    d = 5 if layout == "regression" else 40                # regression40: RAM's wave factor on a regression target
    X, Y = sc.data(12, d, 3)
    return mc.model(mc.LogisticRegression(X, Y), vars=np.zeros(d), gradient=True)


def _run(handle, steps, d, C):
    """steps more steps of a chain batch: samples [steps][d][C], accept [steps][C]"""
    samples = np.empty((steps, d, C))
    words = np.zeros((steps, (C + 63) // 64), dtype=np.uint64)
    out = _lib.Outputs()
    out.samples = samples.ctypes.data
    out.accept_bits = words.ctypes.data
    rc = _lib.RunnerCfg(0, 1, steps)
    _lib.check(_lib.load().mcmc_run_serialmc(handle, ct.byref(rc), ct.byref(out)))
    acc = (words[:, np.arange(C) // 64] >> (np.arange(C) % 64).astype(np.uint64)) & np.uint64(1)
    return samples, acc.astype(bool)


FORK_CASES = [(s, L) for L in ("lane", "wave", "regression") for s in FORK_SAMPLERS] + [("ram", "regression40")]


@pytest.mark.parametrize("sname,layout", FORK_CASES)
def test_fork_continues_its_chains_bitwise(gpu, sname, layout):
    """130 chains, 5 steps (the tuners adapt twice), fork chains [70, 121) -- off the 64-chain tile boundaries at both
    ends, where RAM's lane-layout factor is re-tiled -- then 7 steps on both: the fork's samples and accept bits are the
    source's columns 70..120, bit for bit"""
    C, first, count = 130, 70, 51
    m = fork_model(layout)
    d = {"lane": 3, "wave": 40, "regression": 5, "regression40": 40}[layout]
    t = (m * FORK_SAMPLERS[sname]() * mc.SerialMC(steps=5, burnin=4)).batch(C, seed=3)
    mc.run(t)
    h = ct.c_void_p()
    _lib.check(_lib.load().mcmc_chains_fork(t.handle(), first, count, ct.byref(h)))
    try:
        fs, fa = _run(h, 7, d, count)
    finally:
        _lib.load().mcmc_chains_destroy(h)
    ss, sa = _run(t.handle(), 7, d, C)
    assert np.isfinite(ss).all()
    assert sa.any(), "no chain moved"
    assert np.array_equal(fs.view(np.uint64), ss[:, :, first:first + count].view(np.uint64)), "samples"
    assert np.array_equal(fa, sa[:, first:first + count]), "accept bits"
