"""Shared PMALA cases (test_pmala_cpu.py, test_pmala_gpu.py): smmala_cases' five shapes as models with tensor
derivatives, and the closed forms of the tensor and its derivatives in numpy / scipy."""
import functools

import numpy as np

import mcmchip as mc
import smmala_cases as sc
from mcmchip import _lib

SHAPES = sc.SHAPES
points = sc.points


def _with_dtensor(m):
    return mc.model(m.target, vars=np.zeros(m.size), gradient=True, tensor=True, dtensor=True)


@functools.lru_cache(maxsize=None)
def model(name):
    """smmala_cases.model(name) with has_gradient == 3: the same data, init and prior"""
    return _with_dtensor(sc.model(name))


@functools.lru_cache(maxsize=None)
def logistic_40_10():
    return _with_dtensor(sc.logistic_40_10())


def weights(m, x):
    """(v, w = dv / d eta) of every observation at x [d], from scipy / numpy: the probit example's tensor and
    deriv_tensor as written (examples/probit_regression.jl:44-49, 52-68); the logistic p (1 - p) and its derivative"""
    t = m.target
    eta = t.X @ x
    if t.kind == _lib.MODEL_PROBIT:
        from scipy.stats import norm
        lc, lcm = norm.logcdf(eta), norm.logcdf(-eta)
        v = np.exp(-eta ** 2 - lc - lcm - np.log(2 * np.pi))
        vector01 = np.exp(-eta ** 2 - 2 * lc - lcm - np.log(2 * np.pi))
        w = vector01 * (np.exp(-(eta ** 2 + np.log(2 * np.pi)) / 2 - lcm) - 2 * (norm.pdf(eta) + eta * norm.cdf(eta)))
        return v, w
    s = getattr(t, "link_sign", 1.0)
    p = 1.0 / (1.0 + np.exp(-s * eta))
    return p * (1.0 - p), s * p * (1.0 - p) * (1.0 - 2.0 * p)


def closed_G(m, x):
    t = m.target
    v, _ = weights(m, x)
    return t.X.T @ (v[:, None] * t.X) + np.eye(m.size) / t.prior_sigma ** 2


def closed_dG(m, x):
    """output[:, :, i] = X' diag(w o X[:, i]) X"""
    t = m.target
    _, w = weights(m, x)
    d = m.size
    out = np.empty((d, d, d))
    for i in range(d):
        out[:, :, i] = t.X.T @ ((w * t.X[:, i])[:, None] * t.X)
    return out
