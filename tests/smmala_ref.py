"""ctypes harness for tests/smmala_oracle.c -- TEST INFRASTRUCTURE ONLY.

The SMMALA checker: tests/smmala_oracle.c includes oracle/oracle.c unchanged and adds the metric tensor, the small SPD
algebra and the sampler in the kernels' documented order.  Built with oracle/Makefile's CC and CFLAGS into
tests/_build/ on first use, or when a source is newer than the library.  SmmalaChains is the checker's twin of an
MCMCTask running SMMALA, like oracle_ref.OracleChains.
"""
from __future__ import annotations

import ctypes as ct
import os
import subprocess

import numpy as np

import nuts_ref
import oracle_ref as orc
from oracle_ref import D, OModel, OSampler, OracleModel, _d, _i

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "smmala_oracle.c")
BUILD_DIR = os.path.join(HERE, "_build")
LIB = os.path.join(BUILD_DIR, "libsmmala_oracle.so")

_lib = None


class SmmState(ct.Structure):
    _fields_ = [("x", D), ("lp", D), ("g", D), ("G", D), ("invG", D), ("ft", D), ("t_step", D),
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
    deps = [SRC] + [os.path.join(orc.ORACLE_DIR, f) for f in os.listdir(orc.ORACLE_DIR)
                    if f.endswith((".c", ".h", ".inc"))]
    return any(os.path.getmtime(p) > t for p in deps)


def lib():
    global _lib
    if _lib is None:
        if _stale():
            build()
        L = ct.CDLL(LIB)
        i64, P = ct.c_int64, ct.POINTER
        L.orc_smm_evalallt.restype = None
        L.orc_smm_evalallt.argtypes = [P(OModel), i64, D, D, D, D]
        L.orc_smm_init.restype = i64
        L.orc_smm_init.argtypes = [P(OModel), P(OSampler), i64, P(SmmState)]
        L.orc_smm_set_state.restype = None
        L.orc_smm_set_state.argtypes = [P(OModel), i64, P(SmmState), D]
        L.orc_smm_run.restype = None
        L.orc_smm_run.argtypes = [P(OModel), P(OSampler), ct.c_uint64, i64, i64, i64, i64, i64, i64, i64, i64, i64,
                                  P(SmmState), D, D, P(ct.c_uint8), ct.c_int]
        L.orc_smm_draws.restype = None
        L.orc_smm_draws.argtypes = [ct.c_uint64, ct.c_uint32, ct.c_uint32, ct.c_int, D, D]
        _lib = L
    return _lib


def unpack(Gp, d):
    """packed lower rows [d(d+1)/2, C] -> symmetric [d, d, C]"""
    Gp = np.asarray(Gp)
    G = np.empty((d, d) + Gp.shape[1:])
    for r in range(d):
        for c in range(r + 1):
            G[r, c] = G[c, r] = Gp[r * (r + 1) // 2 + c]
    return G


def evalallt(m, x):
    """the checker's mcmc_model_eval_tensor: x [d, C] -> lp [C], grad [d, C], G packed [d(d+1)/2, C]"""
    om = OracleModel(m)
    d = m.size
    xa = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(d, -1))
    C = xa.shape[1]
    lp, g, G = np.empty(C), np.empty((d, C)), np.empty((d * (d + 1) // 2, C))
    lib().orc_smm_evalallt(ct.byref(om.s), C, _d(xa), _d(lp), _d(g), _d(G))
    return lp, g, G


def draws(seed, chain, step, d):
    """the build's normals and accept uniform of (chain, step)"""
    z, u = np.empty(d), np.empty(1)
    lib().orc_smm_draws(ct.c_uint64(seed), chain, step, d, _d(z), _d(u))
    return z, float(u[0])


class SmmalaChains:
    """The checker's SMMALA chains: the six state members (pars, logTarget, grad, G, invG, firstTerm), the tuner's
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
        self.t_step = np.full(C, np.nan)
        self.t_acc = np.zeros(C, dtype=np.int32)
        self.t_prop = np.zeros(C, dtype=np.int32)
        self.n_evals = np.zeros(C, dtype=np.int64)
        self.st = SmmState(_d(self.x), _d(self.lp), _d(self.g), _d(self.G), _d(self.invG), _d(self.ft),
                           _d(self.t_step), _i(self.t_acc), _i(self.t_prop),
                           self.n_evals.ctypes.data_as(ct.POINTER(ct.c_int64)))
        bad = lib().orc_smm_init(ct.byref(self.om.s), ct.byref(self.os), C, ct.byref(self.st))
        if bad:
            raise AssertionError("Initial values out of model support, try other values")
        self.steps_done = 0

    def set_state(self, x):
        """the :reset hook as written (SMMALA.jl:54-57): invG and firstTerm stay those of the previous position"""
        xx = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(self.om.size, self.C))
        lib().orc_smm_set_state(ct.byref(self.om.s), self.C, ct.byref(self.st), _d(xx))
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
        lib().orc_smm_run(ct.byref(self.om.s), ct.byref(self.os), ct.c_uint64(self.seed), self.chain0, C, c_begin,
                          C if c_end is None else c_end, self.steps_done, runner.burnin, runner.thinning, runner.len,
                          tb, ct.byref(self.st), _d(samples), _d(grads),
                          acc.ctypes.data_as(ct.POINTER(ct.c_uint8)), nthreads)
        self.steps_done += runner.len
        return samples, grads, acc

    @property
    def evals(self) -> int:
        return int(self.n_evals.sum())
