"""ctypes harness for tests/manifold_oracle.c -- TEST INFRASTRUCTURE ONLY.

The checker of the metric-tensor samplers: tests/manifold_oracle.c includes oracle/oracle.c unchanged, then its parts
(smmala_oracle.c: the tensor and the small SPD algebra; pmala_oracle.c: the tensor's derivatives, the fused drift
correction and the SMMALA / PMALA driver; rmhmc_oracle.c: the fused tensor terms, the Cholesky solve, the trajectory
samplers' frame and RMHMC; lmc_oracle.c: ERMLMC and RMLMC), all in the kernels' documented order.  checker_build.load
builds it into tests/_build/libmanifold_oracle.so.  SmmalaChains, PmalaChains, RmhmcChains and LmcChains are the
checker's twins of an MCMCTask running those samplers, like oracle_ref.OracleChains.
"""
from __future__ import annotations

import ctypes as ct
import os

import numpy as np

import checker_build
import oracle_ref as orc
from oracle_ref import D, OModel, OSampler, OracleModel, _d

PARTS = ("smmala_oracle.c", "pmala_oracle.c", "rmhmc_oracle.c", "lmc_oracle.c")
_I32, _I64 = ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int64)

_lib = None


class PmState(ct.Structure):
    """pm_state: SMMALA's and PMALA's chains (c is NULL for SMMALA)"""
    _fields_ = [("x", D), ("lp", D), ("g", D), ("G", D), ("invG", D), ("ft", D), ("c", D), ("t_step", D),
                ("t_acc", _I32), ("t_prop", _I32), ("n_evals", _I64)]


class RmState(ct.Structure):
    """rm_state: RMHMC's, ERMLMC's and RMLMC's chains"""
    _fields_ = [("x", D), ("lp", D), ("g", D), ("t_step", D), ("t_leaps", _I32), ("t_acc", _I32), ("t_prop", _I32),
                ("n_evals", _I64)]


class Counters(ct.Structure):
    """mf_counters: what the steps of the trajectory samplers covered (n_plus and n_minus are RMHMC's)"""
    _fields_ = [(k, ct.c_int64) for k in ("n_plus", "n_minus", "nrl_min", "nrl_max", "n_failed", "n_zero", "n_adapt")]


def lib():
    global _lib
    if _lib is None:
        L = checker_build.load("manifold_oracle.c", "libmanifold_oracle.so", PARTS)
        i64, P, V = ct.c_int64, ct.POINTER, ct.c_void_p
        for name, res, args in (
                ("orc_smm_evalallt", None, [P(OModel), i64, D, D, D, D]),
                ("orc_pm_evalalldt", None, [P(OModel), i64, D, D, D, D, D]),
                ("orc_pm_inverse", None, [ct.c_int, i64, D, D]),
                ("orc_pm_corr", None, [P(OModel), i64, D, D, D]),
                ("orc_rm_terms", None, [P(OModel), D, D, D, D, D]),
                ("orc_rm_solve", ct.c_int, [ct.c_int, D, D, D]),
                ("orc_rm_energy_error", ct.c_double, [P(OModel), D, D, ct.c_double, i64, ct.c_int]),
                ("orc_lmc_gram", None, [P(OModel), D, D, D, D]),
                ("orc_lmc_factor", ct.c_int, [ct.c_int, D, D, ct.c_double, D, D, D]),
                ("orc_lmc_leap", ct.c_double, [P(OModel), ct.c_int, ct.c_int, ct.c_double, D, D]),
                ("orc_manifold_draws", None, [ct.c_uint64, ct.c_uint32, ct.c_uint32, ct.c_int, D, D, D, D]),
                ("orc_pm_init", i64, [P(OModel), P(OSampler), i64, P(PmState)]),
                ("orc_pm_set_state", None, [P(OModel), i64, P(PmState), D]),
                ("orc_hmc_init", i64, [P(OModel), P(OSampler), i64, P(RmState)]),
                ("orc_hmc_set_state", None, [P(OModel), i64, P(RmState), D]),
                ("orc_manifold_run", None, [P(OModel), P(OSampler), ct.c_uint64, i64, i64, i64, i64, i64, i64, i64, i64,
                                            i64, V, D, D, P(ct.c_uint8), P(Counters), ct.c_int])):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _lib = L
    return _lib


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def unpack(Gp, d):
    """packed lower rows [d(d+1)/2, C] -> symmetric [d, d, C]"""
    Gp = np.asarray(Gp)
    G = np.empty((d, d) + Gp.shape[1:])
    for r in range(d):
        for c in range(r + 1):
            G[r, c] = G[c, r] = Gp[r * (r + 1) // 2 + c]
    return G


def pack(M):
    """symmetric [d, d] -> packed lower rows [d (d + 1) / 2]"""
    d = M.shape[0]
    return np.array([M[r, c] for r in range(d) for c in range(r + 1)], dtype=np.float64)


def evalalldt(m, x):
    """the checker's mcmc_model_eval_dtensor: x [d, C] -> lp [C], grad [d, C], G packed [nr, C], dG packed [d, nr, C]"""
    om = OracleModel(m)
    d = m.size
    nr = d * (d + 1) // 2
    xa = _f64(np.asarray(x, dtype=np.float64).reshape(d, -1))
    C = xa.shape[1]
    lp, g, G, dG = np.empty(C), np.empty((d, C)), np.empty((nr, C)), np.empty((d, nr, C))
    lib().orc_pm_evalalldt(ct.byref(om.s), C, _d(xa), _d(lp), _d(g), _d(G), _d(dG))
    return lp, g, G, dG


def evalallt(m, x):
    """the checker's mcmc_model_eval_tensor: x [d, C] -> lp [C], grad [d, C], G packed [d(d+1)/2, C]"""
    om = OracleModel(m)
    d = m.size
    xa = _f64(np.asarray(x, dtype=np.float64).reshape(d, -1))
    C = xa.shape[1]
    lp, g, G = np.empty(C), np.empty((d, C)), np.empty((d * (d + 1) // 2, C))
    lib().orc_smm_evalallt(ct.byref(om.s), C, _d(xa), _d(lp), _d(g), _d(G))
    return lp, g, G


def inverse(Gp, d):
    """packed G [nr, C] -> packed inverse by the kernels' Cholesky route"""
    Gp = _f64(Gp)
    out = np.empty_like(Gp)
    lib().orc_pm_inverse(d, Gp.shape[1], _d(Gp), _d(out))
    return out


def corr(m, x, invG):
    """the checker's fused drift correction at x [d, C] with packed invG [nr, C] -> c [d, C]"""
    om = OracleModel(m)
    xa = _f64(np.asarray(x, dtype=np.float64).reshape(m.size, -1))
    iG = _f64(invG)
    c = np.empty_like(xa)
    lib().orc_pm_corr(ct.byref(om.s), xa.shape[1], _d(xa), _d(iG), _d(c))
    return c


def terms(m, x, invG, v):
    """the checker's fused terms of one point: x [d], packed invG [nr], v [d] -> (X' (w o qf), X' (w o (X v)^2))"""
    om = OracleModel(m)
    xa, iG, va = _f64(x), _f64(invG), _f64(v)
    u, u2 = np.empty(m.size), np.empty(m.size)
    lib().orc_rm_terms(ct.byref(om.s), _d(xa), _d(iG), _d(va), _d(u), _d(u2))
    return u, u2


def solve(Gp, b, d):
    """packed G [nr] \\ b [d] by the kernels' Cholesky route (None on a failed pivot)"""
    Gp, b = _f64(Gp), _f64(b)
    out = np.empty(d)
    return out if lib().orc_rm_solve(d, _d(Gp), _d(b), _d(out)) else None


def gram(m, x, v):
    """the checker's weighted Gram matrix of one point: x [d], v [d] -> (vxC(v) [d, d] = 0.5 X' diag(w o X v) X,
    vxC(v) v [d] = 0.5 X' (w o (X v)^2))"""
    om = OracleModel(m)
    d = m.size
    xa, va = _f64(x), _f64(v)
    K, u2 = np.empty(d * (d + 1) // 2), np.empty(d)
    lib().orc_lmc_gram(ct.byref(om.s), _d(xa), _d(va), _d(K), _d(u2))
    return 0.5 * unpack(K.reshape(-1, 1), d)[:, :, 0], 0.5 * u2


def factor(G, vxC, c, b=None):
    """logdet and (with b) the solve of G + c vxC ([d, d] each) from the packed Cholesky factor, the kernels' route;
    (None, None) on a failed pivot"""
    d = G.shape[0]
    Gp, Kp = pack(G), pack(2.0 * vxC)
    hl, out = np.empty(1), np.empty(d)
    bb = None if b is None else _f64(b)
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


def energy_error(m, x, mom, eps, nleaps, n_newton):
    """H_end - H_start of nleaps generalised leapfrogs of step eps (timeStep = +1) from (x, mom) on the checker"""
    om = OracleModel(m)
    xa, ma = _f64(x), _f64(mom)
    return float(lib().orc_rm_energy_error(ct.byref(om.s), _d(xa), _d(ma), float(eps), int(nleaps), int(n_newton)))


def draws(seed, chain, step, d, family="mala"):
    """the build's draws of (chain, step): normals z [d] and the accept uniform; for "rmhmc" also the leaps' uniform and
    the sign's normal, for "lmc" also the leaps' uniform"""
    z, a, rm, u = np.empty(d), np.empty(1), np.empty(2), np.empty(1)
    lib().orc_manifold_draws(ct.c_uint64(seed), chain, step, d, _d(z), _d(a), _d(rm), _d(u))
    extra = {"mala": (), "rmhmc": (float(rm[0]), float(rm[1])), "lmc": (float(u[0]),)}[family]
    return (z, float(a[0])) + extra


class ManifoldChains:
    """The checker's chains of one sampler of the family: the state members (x and VECTORS [d][C], MATRICES packed
    [nr][C], lp [C]), the tuner's state and the step counter kept between runs.  A subclass names the state struct (a
    member it does not hold stays NULL), the init and set_state entry points, and whether the run counts what its
    steps covered (`counters`)."""
    STRUCT, INIT, SET_STATE, COUNTERS = None, None, None, False
    VECTORS, MATRICES = ("g",), ()

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
            self.x = _f64(np.asarray(self.init_x, dtype=np.float64).reshape(d, C))
        self.lp = np.zeros(C)
        for name in self.VECTORS:
            setattr(self, name, np.zeros((d, C)))
        for name in self.MATRICES:
            setattr(self, name, np.zeros((d * (d + 1) // 2, C)))
        self.t_step = np.full(C, np.nan)
        for name, ctype in self.STRUCT._fields_:
            if ctype is _I32:                      # the tuner's counts (and nLeaps)
                setattr(self, name, np.zeros(C, dtype=np.int32))
        self.n_evals = np.zeros(C, dtype=np.int64)
        self.counters = Counters(0, 0, 1 << 62, -1, 0, 0, 0) if self.COUNTERS else None
        self.st = self.STRUCT(**{name: getattr(self, name).ctypes.data_as(ctype)
                                 for name, ctype in self.STRUCT._fields_ if hasattr(self, name)})
        bad = getattr(lib(), self.INIT)(ct.byref(self.om.s), ct.byref(self.os), C, ct.byref(self.st))
        if bad:
            raise AssertionError("Initial values out of model support, try other values")
        self.steps_done = 0

    def set_state(self, x):
        """the sampler's :reset hook: pars, logTarget and grad (the MALA pair: and G) at x; what the hook leaves stale
        stays"""
        xx = _f64(np.asarray(x, dtype=np.float64).reshape(self.om.size, self.C))
        getattr(lib(), self.SET_STATE)(ct.byref(self.om.s), self.C, ct.byref(self.st), _d(xx))
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
        lib().orc_manifold_run(ct.byref(self.om.s), ct.byref(self.os), ct.c_uint64(self.seed), self.chain0, C, c_begin,
                               C if c_end is None else c_end, self.steps_done, runner.burnin, runner.thinning,
                               runner.len, tb, ct.byref(self.st), _d(samples), _d(grads),
                               acc.ctypes.data_as(ct.POINTER(ct.c_uint8)),
                               ct.byref(self.counters) if self.COUNTERS else None, nthreads)
        self.steps_done += runner.len
        return samples, grads, acc

    @property
    def evals(self) -> int:
        return int(self.n_evals.sum())


class PmalaChains(ManifoldChains):
    """PMALA: pars, logTarget, grad, G, invG, firstTerm and c.  set_state is the hook as written (PMALA.jl:63-66):
    invG, firstTerm and c stay those of the previous position"""
    STRUCT, INIT, SET_STATE = PmState, "orc_pm_init", "orc_pm_set_state"
    VECTORS, MATRICES = ("g", "ft", "c"), ("G", "invG")


class SmmalaChains(PmalaChains):
    """SMMALA: PMALA's members without c (SMMALA.jl:54-57 for set_state)"""
    VECTORS = ("g", "ft")


class RmhmcChains(ManifoldChains):
    """RMHMC: pars, logTarget, grad; `counters` say what the steps it ran covered.  set_state: RMHMC.jl:74-77"""
    STRUCT, INIT, SET_STATE, COUNTERS = RmState, "orc_hmc_init", "orc_hmc_set_state", True


class LmcChains(RmhmcChains):
    """ERMLMC / RMLMC, by the sampler given: RMHMC's state.  set_state re-evaluates at x and the next step recomputes all
    geometry from it (a stated departure from the reset hooks ERMLMC.jl:64-67 / RMLMC.jl:69-72)"""
