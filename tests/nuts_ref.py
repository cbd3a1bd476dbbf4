"""ctypes harness for tests/nuts_oracle.c -- TEST INFRASTRUCTURE ONLY.

The NUTS checker: tests/nuts_oracle.c includes oracle/oracle.c unchanged and adds the recursive restatement of
NUTS.jl.  It is built by checker_build.load.  NutsChains is the checker's twin of an MCMCTask running NUTS, like oracle_ref.OracleChains.
"""
from __future__ import annotations

import ctypes as ct
import os

import numpy as np

import checker_build
import oracle_ref as orc
from oracle_ref import D, OModel, OState, OracleModel, _d, _i

COUNTERS = ("outer_uturn", "inner_uturn", "leaf_fail", "maxdoublings", "zero_merges", "dir_plus", "dir_minus")

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = checker_build.load("nuts_oracle.c", "libnuts_oracle.so")
        i64, P = ct.c_int64, ct.POINTER
        L.orc_nuts_init.restype = i64
        L.orc_nuts_init.argtypes = [P(OModel), ct.c_uint64, i64, i64, P(OState), D, ct.c_int]
        L.orc_nuts_set_state.restype = None
        L.orc_nuts_set_state.argtypes = [P(OModel), i64, P(OState), D, ct.c_int]
        L.orc_nuts_run.restype = None
        L.orc_nuts_run.argtypes = [P(OModel), ct.c_int, ct.c_uint64, i64, i64, i64, i64, i64, i64, i64, i64,
                                   P(OState), D, D, D, P(ct.c_uint8), D, P(ct.c_int32), ct.c_int, ct.c_int, P(i64)]
        L.orc_nuts_exp.restype = ct.c_double
        L.orc_nuts_exp.argtypes = [ct.c_double]
        _lib = L
    return _lib


class NutsChains:
    """The checker's NUTS chains: per-chain state (position, log-target, epsilon, hbar, log epsilon_bar, mu, the step
    counter) kept between runs; `counters` accumulates the coverage counters of every run."""

    def __init__(self, m, sampler, nchains, seed=1, chain_offset=0, init_x=None, order=None):
        self.model = m
        self.om = OracleModel(m)
        self.maxdoublings = int(sampler.maxdoublings)
        self.C = int(nchains)
        self.seed = int(seed)
        self.chain0 = int(chain_offset)
        self.order = int(orc.kernel_order(m) if order is None else order)
        self.init_x = init_x
        self.counters = dict.fromkeys(COUNTERS, 0)
        self.reset()

    def reset(self):
        d, C = self.om.size, self.C
        if self.init_x is None:
            self.x = np.ascontiguousarray(np.repeat(self.om.init[:, None], C, axis=1))
        else:
            self.x = np.ascontiguousarray(np.asarray(self.init_x, dtype=np.float64).reshape(d, C))
        self.lp = np.zeros(C)
        self.eps = np.zeros(C)
        self.lebar = np.zeros(C)
        self.hbar = np.zeros(C)
        self.mu = np.zeros(C)
        self.n_evals = np.zeros(C, dtype=np.int64)
        self._z32 = np.zeros(C, dtype=np.int32)
        self._z = np.zeros(1)
        self.st = OState(_d(self.x), _d(self.lp), _d(self.eps), _d(self.lebar), _d(self.hbar), _i(self._z32),
                         _i(self._z32), _i(self._z32), self.n_evals.ctypes.data_as(ct.POINTER(ct.c_int64)),
                         _d(self._z))
        bad = lib().orc_nuts_init(ct.byref(self.om.s), ct.c_uint64(self.seed), self.chain0, C, ct.byref(self.st),
                                  _d(self.mu), self.order)
        if bad:
            raise AssertionError("Initial values out of model support, try other values")
        self.steps_done = 0

    def set_state(self, x):
        """the :reset hook (NUTS.jl:61-63): position and evaluation only"""
        xx = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(self.om.size, self.C))
        lib().orc_nuts_set_state(ct.byref(self.om.s), self.C, ct.byref(self.st), _d(xx), self.order)
        return self.lp.copy()

    def run(self, runner, nthreads=None, c_begin=0, c_end=None):
        """-> dict(samples, grads [nkept][d][C]; accept, epsilon, ndoublings [nkept][C])"""
        d, C = self.om.size, self.C
        nk = len(runner.r)
        out = {"samples": np.full((nk, d, C), np.nan), "grads": np.full((nk, d, C), np.nan),
               "accept": np.zeros((nk, C), dtype=np.uint8), "epsilon": np.full((nk, C), np.nan),
               "ndoublings": np.zeros((nk, C), dtype=np.int32)}
        if nthreads is None:
            nthreads = min(8, os.cpu_count() or 1)
        cnt = np.zeros(len(COUNTERS), dtype=np.int64)
        lib().orc_nuts_run(ct.byref(self.om.s), self.maxdoublings, ct.c_uint64(self.seed), self.chain0, C, c_begin,
                           C if c_end is None else c_end, self.steps_done, runner.burnin, runner.thinning, runner.len,
                           ct.byref(self.st), _d(self.mu), _d(out["samples"]), _d(out["grads"]),
                           out["accept"].ctypes.data_as(ct.POINTER(ct.c_uint8)), _d(out["epsilon"]),
                           _i(out["ndoublings"]), self.order, nthreads,
                           cnt.ctypes.data_as(ct.POINTER(ct.c_int64)))
        self.steps_done += runner.len
        for k, v in zip(COUNTERS, cnt):
            self.counters[k] += int(v)
        return out

    def tuner_state(self):
        """the library's mcmc_chains_tuner_state for NUTS: step = epsilon, step_bar = exp(log epsilon_bar)"""
        return {"step": self.eps.copy(), "step_bar": np.array([lib().orc_nuts_exp(v) for v in self.lebar])}

    @property
    def evals(self) -> int:
        return int(self.n_evals.sum())
