"""ctypes harness for tests/stemp_oracle.c -- TEST INFRASTRUCTURE ONLY.

The SerialTempMC checker: tests/stemp_oracle.c includes oracle/oracle.c unchanged and adds the per-walker restatement
of run_serialtempmc (SerialTempMC.jl:31-85).  It is built with oracle/Makefile's CC and CFLAGS into tests/_build/ on
first use, or when a source is newer than the library.  `serialtempmc` runs it on oracle_ref.OracleChains, whose state
and step counters it advances, so that a second call continues them as a second library run does.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

import checker_build
from oracle_ref import D, OModel, OSampler, OState, _d


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = checker_build.load("stemp_oracle.c", "libstemp_oracle.so")
        i64, P, V = ct.c_int64, ct.POINTER, ct.c_void_p
        L.orc_serialtempmc.restype = None
        L.orc_serialtempmc.argtypes = [V, V, V, i64, V, V, V, ct.c_int, i64, i64, i64, i64, D, ct.c_uint64, D,
                                       P(ct.c_int32), P(ct.c_uint8), P(ct.c_int32), P(i64)]
        L.orc_stemp_draws.restype = None
        L.orc_stemp_draws.argtypes = [ct.c_uint64, ct.c_uint32, ct.c_uint32, D]
        L.orc_stemp_exp.restype = ct.c_double
        L.orc_stemp_exp.argtypes = [ct.c_double]
        L.orc_stemp_pick.restype = ct.c_int32
        L.orc_stemp_pick.argtypes = [ct.c_double, ct.c_int32, ct.c_int32]
        # oracle.c's own entry points, from this library (the literal transcription steps its tasks with them)
        L.orc_run.restype = None
        L.orc_run.argtypes = [P(OModel), P(OSampler), ct.c_uint64, i64, i64, i64, i64, i64, i64, i64, i64, P(OState),
                              D, D, P(ct.c_uint8), ct.c_int, ct.c_int]
        _lib = L
    return _lib


def draws(seed: int, chain: int, i: int):
    """(u, u2) of walker `chain` at runner step i"""
    u = np.empty(2)
    lib().orc_stemp_draws(ct.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), chain, i, _d(u))
    return float(u[0]), float(u[1])


def det_exp(x: float) -> float:
    return lib().orc_stemp_exp(x)


def pick(u: float, K: int, at: int) -> int:
    return lib().orc_stemp_pick(u, K, at)


def serialtempmc(chains, steps, burnin, swap_period, logW, seed):
    """orc_serialtempmc over OracleChains `chains` (one per target, equal C and chain offset).  Returns dict(samples
    [steps-burnin][d][C], mod [steps-burnin][C], swap [steps-burnin][C] bool, final_at [C], counters dict)."""
    K, C, d = len(chains), chains[0].C, chains[0].om.size
    assert all(c.C == C and c.chain0 == chains[0].chain0 for c in chains)
    models = (ct.POINTER(OModel) * K)(*[ct.pointer(c.om.s) for c in chains])
    samplers = (ct.POINTER(OSampler) * K)(*[ct.pointer(c.os) for c in chains])
    states = (ct.POINTER(OState) * K)(*[ct.pointer(c.st) for c in chains])
    seeds = (ct.c_uint64 * K)(*[c.seed for c in chains])
    done = (ct.c_int64 * K)(*[c.steps_done for c in chains])
    orders = (ct.c_int * K)(*[c.order for c in chains])
    w = np.zeros(K) if logW is None else np.ascontiguousarray(logW, dtype=np.float64)
    nst = steps - burnin
    out = {"samples": np.full((nst, d, C), np.nan), "mod": np.full((nst, C), -1, dtype=np.int32),
           "final_at": np.full(C, -1, dtype=np.int32)}
    swaps = np.zeros((nst, C), dtype=np.uint8)
    cnt = np.zeros(4 + K, dtype=np.int64)
    lib().orc_serialtempmc(models, samplers, seeds, chains[0].chain0, states, done, orders, K, C, steps, burnin,
                           swap_period, _d(w), ct.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), _d(out["samples"]),
                           out["mod"].ctypes.data_as(ct.POINTER(ct.c_int32)),
                           swaps.ctypes.data_as(ct.POINTER(ct.c_uint8)),
                           out["final_at"].ctypes.data_as(ct.POINTER(ct.c_int32)),
                           cnt.ctypes.data_as(ct.POINTER(ct.c_int64)))
    for c, n in zip(chains, done):
        c.steps_done = int(n)
    out["swap"] = swaps.astype(bool)
    out["counters"] = {"proposed": int(cnt[0]), "accepted": int(cnt[1]), "rejected": int(cnt[2]), "nan": int(cnt[3]),
                       "visits": [int(v) for v in cnt[4:]]}
    return out
