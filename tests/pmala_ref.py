"""ctypes harness for tests/pmala_oracle.c -- TEST INFRASTRUCTURE ONLY.

The PMALA checker: tests/pmala_oracle.c includes tests/smmala_oracle.c (and through it oracle/oracle.c) unchanged and
adds the tensor's derivatives, the fused drift correction and the sampler in the kernels' documented order.  Built like
smmala_ref's library into tests/_build/ on first use, or when a source is newer than the library.  PmalaChains is the
checker's twin of an MCMCTask running PMALA.
"""
from __future__ import annotations

import ctypes as ct
import os
import subprocess

import numpy as np

import nuts_ref
import oracle_ref as orc
import smmala_ref
from oracle_ref import D, OModel, OSampler, OracleModel, _d, _i

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "pmala_oracle.c")
BUILD_DIR = os.path.join(HERE, "_build")
LIB = os.path.join(BUILD_DIR, "libpmala_oracle.so")

_lib = None
unpack = smmala_ref.unpack


class PmState(ct.Structure):
    _fields_ = [("x", D), ("lp", D), ("g", D), ("G", D), ("invG", D), ("ft", D), ("c", D), ("t_step", D),
                ("t_acc", ct.POINTER(ct.c_int32)), ("t_prop", ct.POINTER(ct.c_int32)),
                ("n_evals", ct.POINTER(ct.c_int64))]


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
    deps = [SRC, smmala_ref.SRC] + [os.path.join(orc.ORACLE_DIR, f) for f in os.listdir(orc.ORACLE_DIR)
                                    if f.endswith((".c", ".h", ".inc"))]
    return any(os.path.getmtime(p) > t for p in deps)


def lib():
    global _lib
    if _lib is None:
        if _stale():
            build()
        L = ct.CDLL(LIB)
        i64, P = ct.c_int64, ct.POINTER
        L.orc_pm_evalalldt.restype = None
        L.orc_pm_evalalldt.argtypes = [P(OModel), i64, D, D, D, D, D]
        L.orc_pm_inverse.restype = None
        L.orc_pm_inverse.argtypes = [ct.c_int, i64, D, D]
        L.orc_pm_corr.restype = None
        L.orc_pm_corr.argtypes = [P(OModel), i64, D, D, D]
        L.orc_pm_init.restype = i64
        L.orc_pm_init.argtypes = [P(OModel), P(OSampler), i64, P(PmState)]
        L.orc_pm_set_state.restype = None
        L.orc_pm_set_state.argtypes = [P(OModel), i64, P(PmState), D]
        L.orc_pm_run.restype = None
        L.orc_pm_run.argtypes = [P(OModel), P(OSampler), ct.c_uint64, i64, i64, i64, i64, i64, i64, i64, i64, i64,
                                 P(PmState), D, D, P(ct.c_uint8), ct.c_int]
        L.orc_smm_draws.restype = None
        L.orc_smm_draws.argtypes = [ct.c_uint64, ct.c_uint32, ct.c_uint32, ct.c_int, D, D]
        _lib = L
    return _lib


def evalalldt(m, x):
    """the checker's mcmc_model_eval_dtensor: x [d, C] -> lp [C], grad [d, C], G packed [nr, C], dG packed [d, nr, C]"""
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


def corr(m, x, invG):
    """the checker's fused drift correction at x [d, C] with packed invG [nr, C] -> c [d, C]"""
    om = OracleModel(m)
    d = m.size
    xa = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(d, -1))
    iG = np.ascontiguousarray(invG, dtype=np.float64)
    c = np.empty_like(xa)
    lib().orc_pm_corr(ct.byref(om.s), xa.shape[1], _d(xa), _d(iG), _d(c))
    return c


def draws(seed, chain, step, d):
    """the build's normals and accept uniform of (chain, step)"""
    z, u = np.empty(d), np.empty(1)
    lib().orc_smm_draws(ct.c_uint64(seed), chain, step, d, _d(z), _d(u))
    return z, float(u[0])


class PmalaChains:
    """The checker's PMALA chains: the seven state members (pars, logTarget, grad, G, invG, firstTerm, c), the tuner's
    state and the step counter kept between runs."""

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
        nr = d * (d + 1) // 2
        if self.init_x is None:
            self.x = np.ascontiguousarray(np.repeat(self.om.init[:, None], C, axis=1))
        else:
            self.x = np.ascontiguousarray(np.asarray(self.init_x, dtype=np.float64).reshape(d, C))
        self.lp = np.zeros(C)
        self.g = np.zeros((d, C))
        self.G = np.zeros((nr, C))
        self.invG = np.zeros((nr, C))
        self.ft = np.zeros((d, C))
        self.c = np.zeros((d, C))
        self.t_step = np.full(C, np.nan)
        self.t_acc = np.zeros(C, dtype=np.int32)
        self.t_prop = np.zeros(C, dtype=np.int32)
        self.n_evals = np.zeros(C, dtype=np.int64)
        self.st = PmState(_d(self.x), _d(self.lp), _d(self.g), _d(self.G), _d(self.invG), _d(self.ft), _d(self.c),
                          _d(self.t_step), _i(self.t_acc), _i(self.t_prop),
                          self.n_evals.ctypes.data_as(ct.POINTER(ct.c_int64)))
        bad = lib().orc_pm_init(ct.byref(self.om.s), ct.byref(self.os), C, ct.byref(self.st))
        if bad:
            raise AssertionError("Initial values out of model support, try other values")
        self.steps_done = 0

    def set_state(self, x):
        """the :reset hook as written (PMALA.jl:63-66): invG, firstTerm and c stay those of the previous position"""
        xx = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(self.om.size, self.C))
        lib().orc_pm_set_state(ct.byref(self.om.s), self.C, ct.byref(self.st), _d(xx))
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
        lib().orc_pm_run(ct.byref(self.om.s), ct.byref(self.os), ct.c_uint64(self.seed), self.chain0, C, c_begin,
                         C if c_end is None else c_end, self.steps_done, runner.burnin, runner.thinning, runner.len,
                         tb, ct.byref(self.st), _d(samples), _d(grads),
                         acc.ctypes.data_as(ct.POINTER(ct.c_uint8)), nthreads)
        self.steps_done += runner.len
        return samples, grads, acc

    @property
    def evals(self) -> int:
        return int(self.n_evals.sum())
