"""ctypes harness for tests/describe_oracle.c -- TEST INFRASTRUCTURE ONLY.

The describe checker: a scalar C restatement of mcmc_stats_describe on top of the oracle's orc_ess_one (DESIGN.md §4,
§5.5).  Built with oracle/Makefile's CC and CFLAGS into tests/_build/ on first use, or when its source (or the oracle's)
is newer than the library.  Also the shared cases of test_describe_cpu.py and test_describe_gpu.py.
"""
from __future__ import annotations

import ctypes as ct
import functools

import numpy as np

import checker_build
import ess_cases as ec

NPOOLED = 6
PROBS = (0.0, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0)

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = checker_build.load("describe_oracle.c", "libdescribe_oracle.so")
        i64, D = ct.c_int64, ct.c_void_p
        L.orc_describe.restype = ct.c_int
        L.orc_describe.argtypes = [D, i64, i64, i64, i64, D, D, ct.c_int32, D, D]
        _lib = L
    return _lib


def describe(samples, probs=PROBS, maxlag=0):
    """samples [n][d][C] -> (per_chain [6][d][C], pooled [6 + nprobs][d], nbad [d])"""
    x = np.ascontiguousarray(samples, dtype=np.float64)
    n, d, C = x.shape
    p = np.array(probs, dtype=np.float64)
    per = np.empty((6, d, C))
    pooled = np.empty((NPOOLED + len(p), d))
    nbad = np.empty(d, dtype=np.int64)
    rc = lib().orc_describe(x.ctypes.data, n, d, C, maxlag, per.ctypes.data, p.ctypes.data if len(p) else None, len(p),
                            pooled.ctypes.data, nbad.ctypes.data)
    if rc:
        raise ValueError("describe_oracle: bad argument")
    return per, pooled, nbad


@functools.lru_cache(maxsize=None)
def reference(key):
    """the checker's tables of a named batch, computed once and read-only"""
    out = describe(batch(key))
    for a in out:
        a.setflags(write=False)
    return out


def quantile_rule(values, p):
    """the issue's rule on np.sort: h = (N - 1) p, lo = floor(h), v[lo] + (h - lo) (v[min(lo + 1, N - 1)] - v[lo])"""
    v = np.sort(np.asarray(values, dtype=np.float64).ravel() + 0.0)        # -0 -> +0; NaN sorts last
    N = len(v)
    h = np.float64(N - 1) * np.float64(p)
    lo = int(np.floor(h))
    f = h - np.floor(h)
    with np.errstate(all="ignore"):
        return v[lo] + f * (v[min(lo + 1, N - 1)] - v[lo])


# ------------------------------------------------------------------ the batches both test files use
SERIES_N = (2, 3, 90, 96, 97, 618, 619, 700)               # both sides of every size-class edge
SERIES_D = (1, 3, 32)
SERIES_C = (1, 63, 64, 65, 200)


def series_shapes():
    """every n with a (d, C) pair that walks through the d and C lists, plus the full (d, C) grid at n = 90"""
    out = [(n, SERIES_D[i % 3], SERIES_C[i % 5]) for i, n in enumerate(SERIES_N)]
    out += [(n, SERIES_D[(i + 1) % 3], SERIES_C[(i + 2) % 5]) for i, n in enumerate(SERIES_N)]
    out += [(90, d, C) for d in SERIES_D for C in SERIES_C]
    return sorted(set(out))


def never_moved_batch():
    """n = 90, d = 2, C = 70: the chains of STUCK never moved in parameter 0 (one value, so ss = 0 and varimse = 0/0
    or 0: the reference arithmetic alone marks them; the other chains are positively correlated series, whose IMSE
    variance is positive); parameter 1 is constant in EVERY chain (W = 0: rhat NaN)"""
    c = ec.Case("never-moved", 90, 2, 70, 89, 0, ("ar95", "ramp", "slowsin", "step", "white"), 0)
    x = ec.samples(c).copy()
    for ch in STUCK:
        x[:, 0, ch] = 0.5 + ch
    x[:, 1, :] = -3.25
    return x


STUCK = (0, 5, 63, 64, 69)

# Many chains, restated from the shapes alone: the pooled sums go over blocks of 4096 chains (nb = ceil(C / 4096) block
# sums added left to right) and a histogram block of the radix select owns 256 chains.  One chain past a block
# (nb = 2; 17 histogram blocks, the last with one chain), a ragged tail (nb = 3; 36 histogram blocks), and a last pool
# block that holds one chain (nb = 4: every lane but one of that block has no chain).
POOL_KEYS = (("pool", 6, 2, 4097), ("pool", 5, 2, 9000), ("pool", 8, 1, 12289))

# maxlag below n - 1, even and odd, one n a size class: the scan's `pair > k` end in each of the three kernels
MAXLAG_CASES = ((90, 2, 65, 7), (90, 2, 65, 40), (97, 1, 63, 1), (97, 1, 63, 50), (97, 1, 63, 94), (619, 1, 64, 6),
                (619, 1, 64, 301))


@functools.lru_cache(maxsize=None)
def batch(key):
    kind = key[0]
    if kind == "series":
        _, n, d, C = key
        x = ec.samples(ec.Case(f"desc-n{n}-d{d}-C{C}", n, d, C, n - 1, 0, ec.MIXED, 0))
    elif kind == "pool":                                    # short series, many chains: the cross-block paths
        _, n, d, C = key
        x = ec.samples(ec.Case(f"desc-pool-n{n}-d{d}-C{C}", n, d, C, n - 1, 0, ec.MIXED, 0))
    elif kind == "poison":                                # const and NaN series among the others
        _, n = key
        x = ec.samples(ec.Case(f"desc-poison-n{n}", n, 1, 130, n - 1, 0, ec.POISONED, 0))
    elif kind == "stuck":
        x = never_moved_batch()
    elif kind == "quant":
        x = quantile_batch(key[1])
    else:
        raise KeyError(key)
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


QUANT_CASES = ("ties", "equal", "zeros", "inf", "denormal", "signs", "lowdigit", "N2", "many")


def quantile_batch(name):
    """[n][d][C] batches for the radix select (n >= 2 always: N = 1 is not reachable through nkept >= 2, the rule's
    N = 2 is the smallest)"""
    rng = np.random.default_rng([7, QUANT_CASES.index(name)])
    if name == "ties":                                     # eleven distinct values among 90 x 2 x 67
        return rng.integers(-5, 6, size=(90, 2, 67)).astype(np.float64) / 4
    if name == "equal":
        return np.full((5, 2, 33), 1.75)
    if name == "zeros":                                    # +0 and -0 only, and a few +-tiny
        x = np.where(rng.random((7, 1, 65)) < 0.5, 0.0, -0.0)
        x[3, 0, ::9] = 5e-324
        x[4, 0, ::11] = -5e-324
        return x
    if name == "inf":
        x = rng.normal(size=(6, 2, 40))
        x[0, :, :3] = np.inf
        x[1, :, 5:9] = -np.inf
        return x
    if name == "denormal":
        return rng.integers(-2000, 2000, size=(9, 1, 70)).astype(np.float64) * 5e-324
    if name == "signs":
        return rng.normal(size=(33, 3, 129)) * np.exp(rng.normal(size=(33, 3, 129)) * 20)
    if name == "lowdigit":                                 # keys that differ in the last 8 bits only
        base = np.float64(1.0).view(np.uint64)
        return (base + rng.integers(0, 256, size=(10, 2, 77)).astype(np.uint64)).view(np.float64)
    if name == "N2":
        return np.array([[[2.0]], [[-1.0]]])
    if name == "many":                                     # four histogram blocks of 256 chains a parameter merge, the
        return rng.normal(size=(90, 3, 1000))              # last one ragged (232 chains); POOL_KEYS go further
    raise KeyError(name)
