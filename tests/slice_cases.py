"""The slice sampler's case table and the checker's wrapper -- TEST INFRASTRUCTURE ONLY.

A case is (model, widths, nchains, keywords).  Unless it says otherwise it runs 6 iterations after burnin 2 under seed
1.  run_checker runs tests/slice_oracle.c (three plain while loops per chain on the oracle's eval); the CPU tests hold
it against the literal transcription (slice_ref.py), the GPU tests hold the kernels against it.
"""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import checker_build
import mcmchip as mc
import oracle_ref as orc

NITER, BURNIN, SEED = 6, 2, 1
DEFAULT_EVALS = 4096
CENSUS = ("left0", "left1", "right0", "right1", "shrink_left", "shrink_right", "first_accept", "neg_inf", "max_evals",
          "updates", "stopped")


@dataclass
class Case:
    id: str
    make: object                       # () -> model
    widths: Optional[object] = None    # None: ones
    C: int = 65
    kw: dict = field(default_factory=dict)      # niter, burnin, step_out, max_evals, chain_offset, iter_begin, seed
    per_chain_init: bool = False       # a per-chain init_x, jittered about model.init
    out_of_support: bool = False
    starved: bool = False


def _iso(d):
    return lambda: mc.model(mc.IsoNormalDot(), init=np.linspace(0.3, 1.1, d))


def _dist(name, *p, x):
    return lambda: mc.model(mc.DistDSL(name, *p), init=np.array([x]))


def _distobs():
    v = np.random.default_rng(3).normal(1.0, 0.5, 40)
    return mc.model(mc.DistObsDSL("Normal", 0.5, 1.5, v=v), init=np.array([0.7]))


def _ou():
    m = mc.model(mc.OrnsteinUhlenbeck(mc.ou_series(60)), init=np.array([5.0, 0.5, 5.0]))
    return m


CASES = [
    Case("iso3", _iso(3), C=65),
    Case("iso16", _iso(16), C=64),
    Case("iso17", _iso(17), C=63),                       # the pair split S = 12 < d
    Case("iso24", _iso(24), C=65),
    Case("iso32", _iso(32), C=33),
    Case("iso3-one-chain", _iso(3), C=1),
    Case("iso24-one-chain", _iso(24), C=1),
    Case("iso3-130-offset-init", _iso(3), C=130, kw={"chain_offset": 1000}, per_chain_init=True),
    Case("iso17-130-offset-init", _iso(17), C=130, kw={"chain_offset": 77}, per_chain_init=True),
    Case("normal5", lambda: mc.model(mc.NormalDSL(1.0, 2.0), init=np.full(5, 0.5)),
         widths=[0.5, 1.0, 2.0, 4.0, 8.0], C=65),
    Case("uniform01", _dist("Uniform", 0.0, 1.0, x=0.5), C=65),
    Case("exponential2", _dist("Exponential", 2.0, x=1.0), C=65),
    Case("cauchy01", _dist("Cauchy", 0.0, 1.0, x=0.3), C=65),
    Case("beta23", _dist("Beta", 2.0, 3.0, x=0.4), C=65),
    Case("absnormal2", lambda: mc.model(mc.AbsNormalDSL(1.0, 0.5), init=np.array([0.8, -1.2])), C=65),
    Case("distobs40", _distobs, C=65),
    Case("ou60", _ou, widths=[20.0, 0.5, 5.0], C=64),
    Case("iso3-no-step-out", _iso(3), widths=[50.0] * 3, C=65, kw={"step_out": False}),
    Case("iso3-narrow", _iso(3), widths=[0.05] * 3, C=65),
    Case("iso17-narrow", _iso(17), widths=[0.05] * 17, C=34),
    Case("iso3-two-launches", _iso(3), C=65, kw={"burnin": 255}),        # 261 iterations: launches of 256 + 5
    Case("iso3-starved", _iso(3), widths=[0.01] * 3, C=65, kw={"max_evals": 3}, starved=True),
    Case("uniform01-out-of-support", _dist("Uniform", 0.0, 1.0, x=0.5), C=3, out_of_support=True),
]
BY_ID = {c.id: c for c in CASES}
ORDINARY = [c for c in CASES if not c.starved and not c.out_of_support]


def case_args(case: Case):
    """(model, init_x [d][C], widths [d], keywords with every default filled in)"""
    m = case.make()
    d, C = m.size, case.C
    init = np.repeat(m.init[:, None], C, axis=1)
    if case.per_chain_init:
        init = init + 0.25 * np.random.default_rng(11).standard_normal((d, C))
    if case.out_of_support:
        init[0, C - 1] = 1.5
    w = np.ones(d) if case.widths is None else np.asarray(case.widths, dtype=np.float64)
    kw = dict(niter=NITER, burnin=BURNIN, step_out=True, max_evals=0, chain_offset=0, iter_begin=0, seed=SEED)
    kw.update(case.kw)
    return m, np.ascontiguousarray(init), w, kw


_lib = None


def checker():
    global _lib
    if _lib is None:
        L = checker_build.load("slice_oracle.c", "libslice_oracle.so")
        D, I32, I64 = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int32), ct.POINTER(ct.c_int64)
        L.orc_slice.restype = ct.c_int
        L.orc_slice.argtypes = [ct.POINTER(orc.OModel), ct.c_int, ct.c_int64, ct.c_int64, ct.c_uint64, D, D, ct.c_int64,
                                ct.c_int64, ct.c_int64, ct.c_int, ct.c_int64, D, D, D, I32, I64, I64, I32]
        L.orc_slice_draw.restype = ct.c_double
        L.orc_slice_draw.argtypes = [ct.c_uint64, ct.c_uint32, ct.c_uint32, ct.c_uint32, ct.c_uint32]
        L.orc_slice_log.restype = ct.c_double
        L.orc_slice_log.argtypes = [ct.c_double]
        _lib = L
    return _lib


@dataclass
class Result:
    rc: int
    samples: np.ndarray
    final_x: np.ndarray
    final_lp: np.ndarray
    info: np.ndarray
    evals: int
    census: dict
    upd_evals: Optional[np.ndarray] = None


def run_checker(m, init, widths, niter=NITER, burnin=BURNIN, step_out=True, max_evals=0, chain_offset=0, iter_begin=0,
                seed=SEED, want_upd=False, want_samples=True) -> Result:
    d, C = init.shape
    om = orc.OracleModel(m)
    samples = np.empty((niter, d, C)) if want_samples else None
    fx, flp, info = np.empty((d, C)), np.empty(C), np.empty(C, dtype=np.int32)
    ev = ct.c_int64(0)
    census = np.zeros(len(CENSUS), dtype=np.int64)
    upd = np.zeros((burnin + niter, d, C), dtype=np.int32) if want_upd else None
    init = np.ascontiguousarray(init, dtype=np.float64)
    w = np.ascontiguousarray(widths, dtype=np.float64)
    P = lambda a, t: None if a is None else a.ctypes.data_as(ct.POINTER(t))  # noqa: E731
    rc = checker().orc_slice(ct.byref(om.s), orc.kernel_order(m), C, chain_offset, ct.c_uint64(seed),
                             P(init, ct.c_double), P(w, ct.c_double), niter, burnin, iter_begin, int(step_out),
                             max_evals or DEFAULT_EVALS, P(samples, ct.c_double), P(fx, ct.c_double),
                             P(flp, ct.c_double), P(info, ct.c_int32), ct.byref(ev), P(census, ct.c_int64),
                             P(upd, ct.c_int32))
    return Result(rc, samples, fx, flp, info, ev.value, dict(zip(CENSUS, census.tolist())), upd)


_cache: dict = {}


def checker_result(case: Case) -> Result:
    """the checker's run of a case, computed once and shared (left unchanged by the tests)"""
    if case.id not in _cache:
        m, init, w, kw = case_args(case)
        _cache[case.id] = run_checker(m, init, w, **kw)
    return _cache[case.id]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
