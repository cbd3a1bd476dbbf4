"""ctypes harness for tests/lmc_oracle.c -- TEST INFRASTRUCTURE ONLY.

The ERMLMC / RMLMC checker: tests/lmc_oracle.c includes tests/rmhmc_oracle.c (and through it pmala_oracle.c,
smmala_oracle.c and oracle/oracle.c) unchanged and adds the weighted Gram matrix, the factor of G + c vxC and both
samplers in the kernels' documented order.  Built like rmhmc_ref's library into tests/_build/ on first use, or when a
source is newer than the library.  LmcChains is the checker's twin of an MCMCTask running ERMLMC or RMLMC; its
`counters` say what the steps it ran covered.
"""
from __future__ import annotations

import ctypes as ct
import os
import subprocess

import numpy as np

import nuts_ref
import oracle_ref as orc
import pmala_ref
import rmhmc_ref
import smmala_ref
from oracle_ref import D, OModel, OSampler, OracleModel, _d, _i
from rmhmc_ref import RmState

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "lmc_oracle.c")
BUILD_DIR = os.path.join(HERE, "_build")
LIB = os.path.join(BUILD_DIR, "liblmc_oracle.so")

_lib = None
unpack = smmala_ref.unpack


class LmcCounters(ct.Structure):
    _fields_ = [("nrl_min", ct.c_int64), ("nrl_max", ct.c_int64), ("n_failed", ct.c_int64), ("n_zero", ct.c_int64),
                ("n_adapt", ct.c_int64)]


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
    deps = [SRC, rmhmc_ref.SRC, pmala_ref.SRC, smmala_ref.SRC]
    deps += [os.path.join(orc.ORACLE_DIR, f) for f in os.listdir(orc.ORACLE_DIR) if f.endswith((".c", ".h", ".inc"))]
    return any(os.path.getmtime(p) > t for p in deps)


def lib():
    global _lib
    if _lib is None:
        if _stale():
            build()
        L = ct.CDLL(LIB)
        i64, P = ct.c_int64, ct.POINTER
        L.orc_lmc_init.restype = i64
        L.orc_lmc_init.argtypes = [P(OModel), P(OSampler), i64, P(RmState)]
        L.orc_lmc_set_state.restype = None
        L.orc_lmc_set_state.argtypes = [P(OModel), i64, P(RmState), D]
        L.orc_lmc_run.restype = None
        L.orc_lmc_run.argtypes = [P(OModel), P(OSampler), ct.c_uint64, i64, i64, i64, i64, i64, i64, i64, i64, i64,
                                  P(RmState), D, D, P(ct.c_uint8), P(LmcCounters), ct.c_int]
        L.orc_lmc_gram.restype = None
        L.orc_lmc_gram.argtypes = [P(OModel), D, D, D, D]
        L.orc_lmc_factor.restype = ct.c_int
        L.orc_lmc_factor.argtypes = [ct.c_int, D, D, ct.c_double, D, D, D]
        L.orc_lmc_leap.restype = ct.c_double
        L.orc_lmc_leap.argtypes = [P(OModel), ct.c_int, ct.c_int, ct.c_double, D, D]
        L.orc_lmc_draws.restype = None
        L.orc_lmc_draws.argtypes = [ct.c_uint64, ct.c_uint32, ct.c_uint32, ct.c_int, D, D, D]
        L.orc_pm_evalalldt.restype = None
        L.orc_pm_evalalldt.argtypes = [P(OModel), i64, D, D, D, D, D]
        _lib = L
    return _lib


def pack(M):
    """symmetric [d, d] -> packed lower rows [d (d + 1) / 2]"""
    d = M.shape[0]
    return np.array([M[r, c] for r in range(d) for c in range(r + 1)], dtype=np.float64)


def unpack1(Mp, d):
    """packed lower rows [nr] -> symmetric [d, d]"""
    return unpack(np.ascontiguousarray(Mp, dtype=np.float64).reshape(-1, 1), d)[:, :, 0]


def gram(m, x, v):
    """the checker's weighted Gram matrix of one point: x [d], v [d] -> (vxC(v) [d, d] = 0.5 X' diag(w o X v) X,
    vxC(v) v [d] = 0.5 X' (w o (X v)^2))"""
    om = OracleModel(m)
    d = m.size
    xa, va = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, v))
    K, u2 = np.empty(d * (d + 1) // 2), np.empty(d)
    lib().orc_lmc_gram(ct.byref(om.s), _d(xa), _d(va), _d(K), _d(u2))
    return 0.5 * unpack1(K, d), 0.5 * u2


def factor(G, vxC, c, b=None):
    """logdet and (with b) the solve of G + c vxC ([d, d] each) from the packed Cholesky factor, the kernels' route;
    (None, None) on a failed pivot"""
    d = G.shape[0]
    Gp, Kp = pack(G), pack(2.0 * vxC)
    hl, out = np.empty(1), np.empty(d)
    bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    ok = lib().orc_lmc_factor(d, _d(Gp), _d(Kp), 0.5 * c, None if bb is None else _d(bb), _d(hl), _d(out))
    if not ok:
        return None, None
    return 2.0 * float(hl[0]), (out if b is not None else None)


def leap(m, kind, x, v, h, n_newton=0):
    """one leapfrog of ERMLMC ("ermlmc") or RMLMC ("rmlmc") on the checker from (x, v): -> (x', v', the change of
    deltaLogDet), None when the trajectory fails"""
    om = OracleModel(m)
    xa, va = (np.array(a, dtype=np.float64) for a in (x, v))
    dl = float(lib().orc_lmc_leap(ct.byref(om.s), int(kind == "rmlmc"), int(n_newton), float(h), _d(xa), _d(va)))
    return None if np.isnan(dl) else (xa, va, dl)


def draws(seed, chain, step, d):
    """the build's draws of (chain, step): normals z [d], the accept uniform, the leaps' uniform"""
    z, a, u = np.empty(d), np.empty(1), np.empty(1)
    lib().orc_lmc_draws(ct.c_uint64(seed), chain, step, d, _d(z), _d(a), _d(u))
    return z, float(a[0]), float(u[0])


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


class LmcChains:
    """The checker's ERMLMC / RMLMC chains: the state (pars, logTarget, grad), the tuner's state, the step counter and
    the counters of what the steps it ran covered, kept between runs."""

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
        self.counters = LmcCounters(1 << 62, -1, 0, 0, 0)
        self.st = RmState(_d(self.x), _d(self.lp), _d(self.g), _d(self.t_step), _i(self.t_leaps), _i(self.t_acc),
                          _i(self.t_prop), self.n_evals.ctypes.data_as(ct.POINTER(ct.c_int64)))
        bad = lib().orc_lmc_init(ct.byref(self.om.s), ct.byref(self.os), C, ct.byref(self.st))
        if bad:
            raise AssertionError("Initial values out of model support, try other values")
        self.steps_done = 0

    def set_state(self, x):
        """pars, logTarget and grad at x; the next step recomputes all geometry from it (a stated departure from the
        reset hooks ERMLMC.jl:64-67 / RMLMC.jl:69-72)"""
        xx = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(self.om.size, self.C))
        lib().orc_lmc_set_state(ct.byref(self.om.s), self.C, ct.byref(self.st), _d(xx))
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
        lib().orc_lmc_run(ct.byref(self.om.s), ct.byref(self.os), ct.c_uint64(self.seed), self.chain0, C, c_begin,
                          C if c_end is None else c_end, self.steps_done, runner.burnin, runner.thinning, runner.len,
                          tb, ct.byref(self.st), _d(samples), _d(grads),
                          acc.ctypes.data_as(ct.POINTER(ct.c_uint8)), ct.byref(self.counters), nthreads)
        self.steps_done += runner.len
        return samples, grads, acc

    @property
    def evals(self) -> int:
        return int(self.n_evals.sum())
