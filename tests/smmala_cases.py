"""Shared SMMALA cases (test_smmala_cpu.py, test_smmala_gpu.py): the five (kind, n, d, C) shapes of the tensor and
sampler parity tests, with fixed seeded data."""
import functools
import os

import numpy as np

import mcmchip as mc

VASO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vaso.txt")

# name -> (kind, n, d, C, h): h = 1.0, 0.5 at d = 16
SHAPES = {
    "probit_vaso": ("vaso", 39, 3, 8, 1.0),
    "logistic_n16_d1": ("logistic", 16, 1, 1, 1.0),
    "logistic_n17_d5": ("logistic", 17, 5, 70, 1.0),
    "logistic_neg_n33_d16": ("logistic_neg", 33, 16, 100, 0.5),
    "probit_n40_d10": ("probit", 40, 10, 17, 1.0),
}


def data(n, d, seed):
    """X with a leading column of ones, Y drawn from the logistic model at a fixed beta"""
    rng = np.random.default_rng(seed)
    X = np.hstack([np.ones((n, 1)), rng.standard_normal((n, d - 1))]) if d > 1 else rng.standard_normal((n, 1))
    beta = rng.standard_normal(d) * 0.5
    Y = (rng.random(n) < 1.0 / (1.0 + np.exp(-X @ beta))).astype(np.float64)
    return np.ascontiguousarray(X), Y


@functools.lru_cache(maxsize=None)
def model(name, tensor=True):
    kind, n, d, _, _ = SHAPES[name]
    if kind == "vaso":
        X, Y = mc.vaso_data(VASO)
        return mc.model(mc.ProbitRegression(X, Y), vars=np.zeros(3), gradient=True, tensor=tensor)
    X, Y = data(n, d, 100 + n)
    if kind == "probit":
        return mc.model(mc.ProbitRegression(X, Y), vars=np.zeros(d), gradient=True, tensor=tensor)
    t = mc.LogisticRegression(X, Y, link_sign=-1.0) if kind == "logistic_neg" else mc.LogisticRegression(X, Y)
    return mc.model(t, vars=np.zeros(d), gradient=True, tensor=tensor)


@functools.lru_cache(maxsize=None)
def logistic_40_10(tensor=True):
    X, Y = data(40, 10, 7)
    return mc.model(mc.LogisticRegression(X, Y), vars=np.zeros(10), gradient=True, tensor=tensor)


def points(name):
    """evaluation points [d, C]: seeded normals of scale 0.5"""
    _, n, d, C, _ = SHAPES[name]
    return np.random.default_rng(n * 31 + d).standard_normal((d, C)) * 0.5
