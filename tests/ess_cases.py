"""Shared cases for the device ESS kernels of kernels/stats.hip (k_ess_reg<32|64|96>, k_ess_tile, k_ess_col):
test_ess_cpu.py (CPU: the table's census -- where Geyer's scan ends for every series -- the oracle against the numpy
twin, exact scaling, NaN positions) and test_ess_gpu.py (GPU: bitwise against the oracle).

The kernels, restated here from the shapes alone (not read from the library):
  imse / ipse, n <= 96        k_ess_reg<N>, N = 32, 64, 96: one lane per series, 256 series a block
  n <= 618 otherwise          k_ess_tile: 32 series a block, 4 lanes a series; pairs 0-3 in round 0, then rounds of
                              sixteen pairs (round r >= 1: pairs 4 + 16 (r - 1) .. 19 + 16 (r - 1))
  n >= 619                    k_ess_col: one thread per series, 64 series a block
Batch means (bm) at n <= 618 always take k_ess_tile.

Series are closed forms of (n, index), the index counting the series of one family within a case; only `white`, `ar95` and `nan` draw from a seeded generator.  A
case lays its families out by series index, so consecutive chains of one parameter cycle through them and every
4-lane group's wave, 32-series tile and 256-thread block holds series that end their scan in different rounds.
"""
import functools
from collections import namedtuple

import numpy as np

REG_MAX_N = 96
TILE_MAX_N = 618
VTYPES = {"imse": 1, "ipse": 2, "bm": 3}


def kernel_of(n, vtype):
    if vtype != "bm" and n <= REG_MAX_N:
        return "reg32" if n <= 32 else "reg64" if n <= 64 else "reg96"
    return "tile" if n <= TILE_MAX_N else "col"


def k_of(maxlag):
    """Geyer's last pair index: k = floor((maxlag - 1) / 2); pairs 0 .. k"""
    return (maxlag - 1) // 2


def round_of(pair):
    """k_ess_tile's round that holds `pair`"""
    return 0 if pair <= 3 else 1 + (pair - 4) // 16


# ------------------------------------------------------------------ series families
def _chirp(n, i, amp=0.05):
    t = np.arange(n, dtype=np.float64)
    return amp * np.sin(0.37 * t * t + 0.1 * i)


def _wiggle(n, i):
    t = np.arange(n, dtype=np.float64)
    return 0.01 * np.sin(1.3 * t + i)


def alt(n, i):
    """every Geyer pair positive: the scan runs to k"""
    t = np.arange(n, dtype=np.float64)
    return (-1.0) ** t * (1.0 + 0.001 * t / n) + _chirp(n, i)


def altstop_pair(n, i):
    """the pair at which `altstop` series i of length n ends its scan (None: n too short, the series is `alt`):
    consecutive i walk through k_ess_tile's rounds, at a varying place inside the round"""
    k = k_of(n - 1)
    if k < 2:
        return None
    nbins = round_of(k - 1) + 1
    b = i % nbins
    p = 1 + i % 3 if b == 0 else 4 + 16 * (b - 1) + (7 * i) % 16
    return min(p, k - 1)


def altstop(n, i):
    """`alt` with two spikes 2p + 1 steps apart: lag 2p + 1 gains their product, which makes pair p the first
    non-positive one (p = altstop_pair)"""
    p = altstop_pair(n, i)
    x = alt(n, i)
    if p is None:
        return alt(n, 500 + i)                                # another phase than any `alt` series of the case
    t0 = i % 3
    for t in (t0, t0 + 2 * p + 1):
        x[t] += 2.0 * (-1.0) ** t
    return x


def ramp(n, i):
    return np.arange(n, dtype=np.float64) + _wiggle(n, i)


def slowsin(n, i):
    t = np.arange(n, dtype=np.float64)
    return np.sin(2.0 * np.pi * t / n + 0.05 * (i % 16)) + _wiggle(n, i)


def step(n, i):
    return np.where(np.arange(n) < n // 2, 1.0, -1.0) + _wiggle(n, i)


def white(n, i):
    return np.random.default_rng([n, i]).normal(size=n)


def ar95(n, i):
    e = np.random.default_rng([n, i, 95]).normal(size=n)
    x = np.empty(n)
    x[0] = e[0]
    for t in range(1, n):
        x[t] = 0.95 * x[t - 1] + 0.1 * e[t]
    return x


def const(n, i):
    return np.full(n, (0.0, 1.5, -2.0)[i % 3])


def nan(n, i):
    x = white(n, i)
    x[n // 2] = np.nan
    return x


FAMILIES = {f.__name__: f for f in (alt, altstop, ramp, slowsin, step, white, ar95, const, nan)}
DETERMINISTIC = ("alt", "altstop", "ramp", "slowsin", "step")
POISON = ("const", "nan")                                     # ESS is NaN: 0/0, or NaN all the way

MIXED = ("alt", "white", "altstop", "ramp", "ar95", "altstop", "slowsin", "step")
POISONED = ("alt", "const", "altstop", "nan", "white", "ramp", "altstop", "const", "ar95", "nan", "step")
CAPPED = ("alt", "alt", "alt", "white")
SCALED = ("ramp", "alt", "altstop", "step", "slowsin")

# name, n, d, C, maxlag (always explicit), batchlen (0: no bm), layout, log2 of the scale
Case = namedtuple("Case", "name n d C maxlag batchlen layout scale")


def case_id(c):
    return c.name


def vtypes(c):
    return ("imse", "ipse") + (("bm",) if c.batchlen else ())


def family_of(c, j, ch):
    """the family of parameter j, chain ch: consecutive chains cycle through the layout, every parameter from
    another place in it"""
    return c.layout[(ch + 3 * j) % len(c.layout)]


@functools.lru_cache(maxsize=None)
def _samples(c, clean):
    x = np.empty((c.n, c.d, c.C))
    seen = {}
    for j in range(c.d):
        for ch in range(c.C):
            fam = family_of(c, j, ch)
            i = seen.get(fam, 0)                              # the family's index: its how-manieth series of the case
            seen[fam] = i + 1
            if clean and fam in POISON:
                fam, i = "white", 10000 + j * c.C + ch        # no other series changes
            x[:, j, ch] = FAMILIES[fam](c.n, i)
    if c.scale:
        x = x * 2.0 ** c.scale                                # exact
    x.setflags(write=False)
    return x


def samples(c, clean=False):
    """the case's batch [n][d][C] (read-only, shared); clean: the const / nan series replaced by white noise"""
    return _samples(c, bool(clean))


def poison_mask(c):
    """[d][C]: the series whose ESS is NaN"""
    return np.array([[family_of(c, j, ch) in POISON for ch in range(c.C)] for j in range(c.d)])


def family_mask(c, fams):
    return np.array([[family_of(c, j, ch) in fams for ch in range(c.C)] for j in range(c.d)])


# ------------------------------------------------------------------ where the scan ends (numpy, plain dot products)
def pair_sums(x, k):
    """(g[0 .. k], acv0) of one series: g[j] = acv[2j] + acv[2j + 1], acv[L] = sum_t z_t z_{t+L} / n"""
    n = len(x)
    z = x - x.sum() / n
    g = np.empty(k + 1)
    for j in range(k + 1):
        L = 2 * j
        g[j] = (np.dot(z[:n - L], z[L:]) + (np.dot(z[:n - L - 1], z[L + 1:]) if L + 1 < n else 0.0)) / n
    return g, np.dot(z, z) / n


def stop_pair(x, maxlag):
    """(e, margin): e the first pair with g <= 0, or k + 1 when every pair up to k is positive; margin the
    smallest |g[j]| / acv0 over the pairs the scan looks at, j <= min(e, k) (None when it looks at none or acv0 is
    not a positive number).  k_ess_tile ends the scan in round_of(e)."""
    k = k_of(maxlag)
    if k < 0:
        return 0, None
    g, a0 = pair_sums(x, k)
    nz = np.nonzero(~(g > 0.0))[0]
    e = int(nz[0]) if len(nz) else k + 1
    margin = float(np.min(np.abs(g[:min(e, k) + 1])) / a0) if a0 > 0.0 else None
    return e, margin


@functools.lru_cache(maxsize=None)
def census(c):
    """[(j, ch, family, e, margin)] (stop_pair) of every series of the case that is not const / nan"""
    x = samples(c)
    out = []
    for j in range(c.d):
        for ch in range(c.C):
            fam = family_of(c, j, ch)
            if fam in POISON:
                continue
            e, r = stop_pair(x[:, j, ch], c.maxlag)
            out.append((j, ch, fam, e, r))
    return out


def clamp_count(x, maxlag):
    """how many pairs of a series take IMSE's clamp g[j] > g[j-1] before the scan ends"""
    k = k_of(maxlag)
    g, _ = pair_sums(x, k)
    e, _ = stop_pair(x, maxlag)
    g = g[:min(e, k + 1)]
    return int(np.sum(g[1:] > np.minimum.accumulate(g)[:-1]))


# ------------------------------------------------------------------ the table
SHAPE_D = (1, 3)
SHAPE_C = (1, 31, 33, 65, 130)             # one series, partial tile, one past a tile, one past a wave, several tiles
SHAPE_N = (33, 101, 619)                   # one n a kernel family
REG_N = (2, 3, 32, 33, 64, 65, 95, 96)
TILE_N = (97, 98, 99, 100, 101, 102, 103, 104, 192, 193, 240, 241, 617, 618)
COL_N = (619, 1000)
CAP_N = (300, 1000)


def cap_maxlags(n):
    """k on both sides of the round edges at pairs 3|4, 19|20, 35|36 and at the end"""
    return (1, 2, 7, 8, 9, 39, 40, 41, 71, 72, 73, n - 2, n - 1)


BM_CASES = ((4, 2), (33, 16), (618, 20), (618, 309), (1000, 7))
POISON_N = ((96, 0), (33, 16), (618, 20), (619, 20))          # (n, batchlen)
SCALED_N = (96, 618, 619)


def _cases():
    out = []
    for n in SHAPE_N:
        for d in SHAPE_D:
            for C in SHAPE_C:
                out.append(Case(f"shape-n{n}-d{d}-C{C}", n, d, C, n - 1, 0, MIXED, 0))
    for n in REG_N:
        out.append(Case(f"reg-n{n}", n, 2, 130, n - 1, 0, MIXED, 0))
    for n in TILE_N:
        out.append(Case(f"tile-n{n}", n, 1, 130, n - 1, 0, MIXED, 0))
    for n in COL_N:
        out.append(Case(f"col-n{n}", n, 1, 130, n - 1, 0, MIXED, 0))
    for n in CAP_N:
        for ml in cap_maxlags(n):
            out.append(Case(f"cap-n{n}-maxlag{ml}", n, 1, 33, ml, 0, CAPPED, 0))
    for n, bl in BM_CASES:
        out.append(Case(f"bm-n{n}-bl{bl}", n, 2, 65, n - 1, bl, MIXED, 0))
    for n, bl in POISON_N:
        out.append(Case(f"poison-n{n}" + (f"-bl{bl}" if bl else ""), n, 1, 130, n - 1, bl, POISONED, 0))
    for n in SCALED_N:
        for s in (0, 400, -400):
            out.append(Case(f"scaled-n{n}-2^{s}", n, 1, 33, n - 1, 20, SCALED, s))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# cases that also go through the device-pointer path (a tensor in and out, no variance): one a kernel at least
DEVICE_POINTER_CASES = ("reg-n32", "reg-n64", "reg-n96", "tile-n618", "col-n1000", "bm-n33-bl16", "poison-n618-bl20")


def is_finite_case(c):
    return not any(f in POISON for f in c.layout)


def unscaled(c):
    """the scale-0 twin of a scaled case"""
    return BY_NAME[f"scaled-n{c.n}-2^0"]


# ------------------------------------------------------------------ the oracle's result, computed once a case
@functools.lru_cache(maxsize=None)
def reference(c, vtype, clean=False):
    """orc_ess of the case: (ess [d][C], var [d][C]), read-only"""
    import oracle_ref as orc
    e, v = orc.ess(samples(c, clean), VTYPES[vtype], c.maxlag, c.batchlen)
    e.setflags(write=False)
    v.setflags(write=False)
    return e, v


def same_bits(a, b):
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def same_bits_or_nan(a, b):
    """bitwise equal, NaN matching NaN of any payload"""
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
