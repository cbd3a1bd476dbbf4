"""ctypes harness for tests/zv_oracle.c -- TEST INFRASTRUCTURE ONLY.

The ZV checker: a scalar C restatement of the arithmetic kernels/zv.hip documents.  It is built with
oracle/Makefile's CC and CFLAGS into tests/_build/ on first use, or when its source is newer than the library.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

import checker_build


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = checker_build.load("zv_oracle.c", "libzv_oracle.so")
        i64, D = ct.c_int64, ct.POINTER(ct.c_double)
        L.orc_zv.restype = ct.c_int
        L.orc_zv.argtypes = [ct.c_int, D, D, i64, i64, i64, D, D, ct.POINTER(ct.c_int32)]
        _lib = L
    return _lib


def k_of(order: int, d: int) -> int:
    return d * (d + 3) // 2 if order == 2 else d


def zv(order, samples, grads):
    """samples, grads [nkept][d][C] (the C-ABI layout) -> (zv [nkept][d][C], coef [k][d][C], info [C])"""
    x = np.ascontiguousarray(samples, dtype=np.float64)
    g = np.ascontiguousarray(grads, dtype=np.float64)
    assert x.ndim == 3 and x.shape == g.shape
    n, d, C = x.shape
    out = np.empty((n, d, C))
    coef = np.empty((k_of(order, d), d, C))
    info = np.empty(C, dtype=np.int32)
    D = ct.POINTER(ct.c_double)
    rc = lib().orc_zv(order, x.ctypes.data_as(D), g.ctypes.data_as(D), n, d, C, out.ctypes.data_as(D),
                      coef.ctypes.data_as(D), info.ctypes.data_as(ct.POINTER(ct.c_int32)))
    if rc:
        raise ValueError("zv_oracle: bad argument")
    return out, coef, info
