"""ctypes harness for tests/rmhmc_oracle.c -- TEST INFRASTRUCTURE ONLY.

The RMHMC checker: tests/rmhmc_oracle.c includes tests/pmala_oracle.c (and through it smmala_oracle.c and
oracle/oracle.c) unchanged and adds the two fused tensor terms, the Cholesky solve and the sampler in the kernels'
documented order.  Built like pmala_ref's library into tests/_build/ on first use, or when a source is newer than the
library.  RmhmcChains is the checker's twin of an MCMCTask running RMHMC; its `counters` say what the steps it ran
covered.
"""
from __future__ import annotations

import ctypes as ct
import os
import subprocess

import numpy as np

import nuts_ref
import oracle_ref as orc
import pmala_ref
import smmala_ref
from oracle_ref import D, OModel, OSampler, OracleModel, _d, _i

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "rmhmc_oracle.c")
BUILD_DIR = os.path.join(HERE, "_build")
LIB = os.path.join(BUILD_DIR, "librmhmc_oracle.so")

_lib = None
unpack = smmala_ref.unpack


class RmState(ct.Structure):
    _fields_ = [("x", D), ("lp", D), ("g", D), ("t_step", D), ("t_leaps", ct.POINTER(ct.c_int32)),
                ("t_acc", ct.POINTER(ct.c_int32)), ("t_prop", ct.POINTER(ct.c_int32)),
                ("n_evals", ct.POINTER(ct.c_int64))]


class RmCounters(ct.Structure):
    _fields_ = [("n_plus", ct.c_int64), ("n_minus", ct.c_int64), ("nrl_min", ct.c_int64), ("nrl_max", ct.c_int64),
                ("n_failed", ct.c_int64), ("n_zero", ct.c_int64), ("n_adapt", ct.c_int64)]


def build() -> None:
    cc, cflags = nuts_ref._make_vars()
    os.makedirs(BUILD_DIR, exist_ok=True)
    tmp = LIB + f".{os.getpid()}.tmp"
    subprocess.run([cc, *cflags, "-shared", "-o", tmp, SRC, "-lm"], check=True, cwd=HERE)
    os.replace(tmp, LIB)


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [SRC, pmala_ref.SRC, smmala_ref.SRC] + [os.path.join(orc.ORACLE_DIR, f) for f in os.listdir(orc.ORACLE_DIR)
                                                   if f.endswith((".c", ".h", ".inc"))]
    return any(os.path.getmtime(p) > t for p in deps)


def lib():
    global _lib
    if _lib is None:
        if _stale():
            build()
        L = ct.CDLL(LIB)
        i64, P = ct.c_int64, ct.POINTER
        L.orc_rm_init.restype = i64
        L.orc_rm_init.argtypes = [P(OModel), P(OSampler), i64, P(RmState)]
        L.orc_rm_set_state.restype = None
        L.orc_rm_set_state.argtypes = [P(OModel), i64, P(RmState), D]
        L.orc_rm_run.restype = None
        L.orc_rm_run.argtypes = [P(OModel), P(OSampler), ct.c_uint64, i64, i64, i64, i64, i64, i64, i64, i64, i64,
                                 P(RmState), D, D, P(ct.c_uint8), P(RmCounters), ct.c_int]
        L.orc_rm_terms.restype = None
        L.orc_rm_terms.argtypes = [P(OModel), D, D, D, D, D]
        L.orc_rm_solve.restype = ct.c_int
        L.orc_rm_solve.argtypes = [ct.c_int, D, D, D]
        L.orc_rm_draws.restype = None
        L.orc_rm_draws.argtypes = [ct.c_uint64, ct.c_uint32, ct.c_uint32, ct.c_int, D, D, D, D]
        L.orc_rm_energy_error.restype = ct.c_double
        L.orc_rm_energy_error.argtypes = [P(OModel), D, D, ct.c_double, i64, ct.c_int]
        L.orc_pm_evalalldt.restype = None
        L.orc_pm_evalalldt.argtypes = [P(OModel), i64, D, D, D, D, D]
        L.orc_pm_inverse.restype = None
        L.orc_pm_inverse.argtypes = [ct.c_int, i64, D, D]
        _lib = L
    return _lib


def terms(m, x, invG, v):
    """the checker's fused terms of one point: x [d], packed invG [nr], v [d] -> (X' (w o qf), X' (w o (X v)^2))"""
    om = OracleModel(m)
    d = m.size
    xa, iG, va = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, invG, v))
    u, u2 = np.empty(d), np.empty(d)
    lib().orc_rm_terms(ct.byref(om.s), _d(xa), _d(iG), _d(va), _d(u), _d(u2))
    return u, u2


def solve(Gp, b, d):
    """packed G [nr] \\ b [d] by the kernels' Cholesky route (None on a failed pivot)"""
    Gp, b = np.ascontiguousarray(Gp, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    out = np.empty(d)
    return out if lib().orc_rm_solve(d, _d(Gp), _d(b), _d(out)) else None


def draws(seed, chain, step, d):
    """the build's draws of (chain, step): normals z [d], the accept uniform, the leaps' uniform, the sign's normal"""
    z, a, u, n = np.empty(d), np.empty(1), np.empty(1), np.empty(1)
    lib().orc_rm_draws(ct.c_uint64(seed), chain, step, d, _d(z), _d(a), _d(u), _d(n))
    return z, float(a[0]), float(u[0]), float(n[0])


def energy_error(m, x, mom, eps, nleaps, n_newton):
    """H_end - H_start of nleaps generalised leapfrogs of step eps (timeStep = +1) from (x, mom) on the checker"""
    om = OracleModel(m)
    xa, ma = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, mom))
    return float(lib().orc_rm_energy_error(ct.byref(om.s), _d(xa), _d(ma), float(eps), int(nleaps), int(n_newton)))


def evalalldt(m, x):
    """the checker's evalalldt (pmala_oracle.c's): x [d, C] -> lp [C], grad [d, C], G packed [nr, C], dG [d, nr, C]"""
    om = OracleModel(m)
    d = m.size
    nr = d * (d + 1) // 2
    xa = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(d, -1))
    C = xa.shape[1]
    lp, g, G, dG = np.empty(C), np.empty((d, C)), np.empty((nr, C)), np.empty((d, nr, C))
    lib().orc_pm_evalalldt(ct.byref(om.s), C, _d(xa), _d(lp), _d(g), _d(G), _d(dG))
    return lp, g, G, dG


def inverse(Gp, d):
    """packed G [nr, C] -> packed inverse by the kernels' Cholesky route"""
    Gp = np.ascontiguousarray(Gp, dtype=np.float64)
    out = np.empty_like(Gp)
    lib().orc_pm_inverse(d, Gp.shape[1], _d(Gp), _d(out))
    return out


class RmhmcChains:
    """The checker's RMHMC chains: the state (pars, logTarget, grad), the tuner's state, the step counter and the
    counters of what the steps covered, kept between runs."""

    def __init__(self, m, sampler, nchains, seed=1, chain_offset=0, init_x=None):
        self.model = m
        self.om = OracleModel(m)
        self.os = orc.oracle_sampler(sampler)
        self.C = int(nchains)
        self.seed = int(seed)
        self.chain0 = int(chain_offset)
        self.init_x = init_x
        self.tuner_burnin = -1
        self.reset()

    def reset(self):
        d, C = self.om.size, self.C
        if self.init_x is None:
            self.x = np.ascontiguousarray(np.repeat(self.om.init[:, None], C, axis=1))
        else:
            self.x = np.ascontiguousarray(np.asarray(self.init_x, dtype=np.float64).reshape(d, C))
        self.lp = np.zeros(C)
        self.g = np.zeros((d, C))
        self.t_step = np.full(C, np.nan)
        self.t_leaps = np.zeros(C, dtype=np.int32)
        self.t_acc = np.zeros(C, dtype=np.int32)
        self.t_prop = np.zeros(C, dtype=np.int32)
        self.n_evals = np.zeros(C, dtype=np.int64)
        self.counters = RmCounters(0, 0, 1 << 62, -1, 0, 0, 0)
        self.st = RmState(_d(self.x), _d(self.lp), _d(self.g), _d(self.t_step), _i(self.t_leaps), _i(self.t_acc),
                          _i(self.t_prop), self.n_evals.ctypes.data_as(ct.POINTER(ct.c_int64)))
        bad = lib().orc_rm_init(ct.byref(self.om.s), ct.byref(self.os), C, ct.byref(self.st))
        if bad:
            raise AssertionError("Initial values out of model support, try other values")
        self.steps_done = 0

    def set_state(self, x):
        """the :reset hook (RMHMC.jl:74-77): pars, logTarget and grad at x"""
        xx = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(self.om.size, self.C))
        lib().orc_rm_set_state(ct.byref(self.om.s), self.C, ct.byref(self.st), _d(xx))
        return self.lp.copy()

    def run(self, runner, nthreads=None, c_begin=0, c_end=None):
        """-> (samples, grads [nkept][d][C], accept [nkept][C])"""
        d, C = self.om.size, self.C
        nk = len(runner.r)
        samples = np.full((nk, d, C), np.nan)
        grads = np.full((nk, d, C), np.nan)
        acc = np.zeros((nk, C), dtype=np.uint8)
        if nthreads is None:
            nthreads = min(8, os.cpu_count() or 1)
        tb = self.tuner_burnin if self.tuner_burnin >= 0 else runner.burnin
        lib().orc_rm_run(ct.byref(self.om.s), ct.byref(self.os), ct.c_uint64(self.seed), self.chain0, C, c_begin,
                         C if c_end is None else c_end, self.steps_done, runner.burnin, runner.thinning, runner.len,
                         tb, ct.byref(self.st), _d(samples), _d(grads),
                         acc.ctypes.data_as(ct.POINTER(ct.c_uint8)), ct.byref(self.counters), nthreads)
        self.steps_done += runner.len
        return samples, grads, acc

    @property
    def evals(self) -> int:
        return int(self.n_evals.sum())
