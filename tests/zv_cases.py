"""Case tables of the ZV kernel tests -- TEST INFRASTRUCTURE ONLY: plain data and input builders, no device.

tests/test_zv_cases_cpu.py runs every table through the checker (zv_ref.zv) and asserts its premises; tests/test_zv_gpu.py
runs the same tables through kernels/zv.hip.  A failure on the device is then a kernel finding, never a case whose
premise was wrong.
"""
import functools

import numpy as np

import zv_ref
from test_zv import synthetic

# the five instances of k_zv<F, NTK, NTD>: (order, smallest d, largest d, NTK, NTD), as mcmc_launch_zv chooses them
INSTANCES = ((1, 1, 16, 1, 1), (1, 17, 32, 2, 2), (2, 1, 4, 1, 1), (2, 5, 6, 2, 1), (2, 7, 8, 3, 1))
TT = 16                                    # kept steps per staged block (kZvTt)


def instance_of(order, d):
    """(order, NTK, NTD) of the instance mcmc_launch_zv picks: linear by d, quadratic by k = d (d + 3) / 2"""
    k = zv_ref.k_of(order, d)
    if order == 1:
        assert 1 <= d <= 32
        return (1, 1, 1) if d <= 16 else (1, 2, 2)
    assert order == 2 and 1 <= d <= 8
    return (2, 1, 1) if k <= 16 else (2, 2, 1) if k <= 32 else (2, 3, 1)


def seed_of(order, d):
    return 100 * order + d


@functools.lru_cache(maxsize=None)
def case(order, d, C, n):
    """inputs and the checker's answer, computed once and left unchanged"""
    x, g = synthetic(d, C, n, seed=seed_of(order, d))
    out = zv_ref.zv(order, x, g)
    for v in (x, g) + out:
        v.setflags(write=False)
    return x, g, out


# ---- PARITY: (order, d, C, nkept).  Every width takes every allowed count of kept steps: the minimum k + 1, k + 2, and
# the staging block's multiples with the counts one below and one above.  63 is added where k >= 31, where 15 and 31 are
# not allowed and the class "a multiple of 16 minus 1" would otherwise be empty.  C rotates within an instance, so every
# instance meets every C.
WIDTHS = tuple((2, d) for d in range(1, 9)) + tuple((1, d) for d in (1, 2, 15, 16, 17, 31, 32))
NKEPT = (15, 16, 17, 31, 32, 33, 48, 61, 64, 65)
CHAINS = (1, 15, 16, 17, 33, 70)


def nkept_of(order, d):
    k = zv_ref.k_of(order, d)
    return sorted({k + 1, k + 2} | {n for n in NKEPT + ((63,) if k >= 31 else ()) if n > k})


def _parity():
    out, met = [], {}
    for order, d in WIDTHS:
        inst = instance_of(order, d)
        for n in nkept_of(order, d):
            i = met.get(inst, 0)
            met[inst] = i + 1
            out.append((order, d, CHAINS[i % len(CHAINS)], n))
    return tuple(out)


PARITY = _parity()

# ---- chains that fail inside the factorisation, at pivot j + 1 >= 1, with n - 1 moves
BAD_C = 33
# chains 3 and 11 share a solve block (waves wc and wc + 8, one after the other): bad then good, good then bad, bad
# then bad; chain 16 is the first of the second tile, chain 32 alone in a ragged tile
PLACEMENTS = ((3,), (11,), (3, 11, 16, 32))
_PIVOT_AT = ((1, 3, (0, 1, 2)), (1, 17, (0, 8, 16)), (1, 32, (0, 16, 31)),
             (2, 3, (0, 1, 2)), (2, 5, (0, 2, 4)), (2, 8, (0, 4, 7)))
# (order, d, j, chains)
PIVOT = tuple((o, d, j, p) for o, d, js in _PIVOT_AT for j in js for p in PLACEMENTS)
NONFINITE_VALUES = (float("nan"), float("inf"), 1e200)             # the last overflows the Gram diagonal
# (order, d, j, index into NONFINITE_VALUES, chains)
NONFINITE = tuple((o, d, j, v, p) for o, d in ((1, 3), (1, 20), (2, 3), (2, 6)) for j in (0, d - 1)
                  for v in range(len(NONFINITE_VALUES)) for p in PLACEMENTS)
DUPLICATE = ((1, 3), (1, 20), (2, 3))                              # (order, d); chain 3 of BAD_C
DUPLICATE_CHAIN = 3


def bad_n(order, d):
    return max(61, zv_ref.k_of(order, d) + 5)


def healthy(order, d):
    """the unmodified inputs of the PIVOT / NONFINITE / DUPLICATE cases and the checker's answer"""
    return case(order, d, BAD_C, bad_n(order, d))


def pivot_inputs(order, d, j, chains):
    """gradient coordinate j of `chains` held at its first value: control variate j centres to exact zeros, so pivot
    j is exactly 0 while the chain has n - 1 moves"""
    x, g, _ = healthy(order, d)
    x, g = x.copy(), g.copy()
    for c in chains:
        g[:, j, c] = g[0, j, c]
    return x, g


def nonfinite_inputs(order, d, j, v, chains):
    x, g, _ = healthy(order, d)
    x, g = x.copy(), g.copy()
    for c in chains:
        g[7, j, c] = NONFINITE_VALUES[v]
    return x, g


def duplicate_inputs(order, d):
    """coordinate 1 of one chain a copy of coordinate 0: G is exactly singular, its second pivot rounding residue"""
    x, g, _ = healthy(order, d)
    x, g = x.copy(), g.copy()
    c = DUPLICATE_CHAIN
    x[:, 1, c] = x[:, 0, c]
    g[:, 1, c] = g[:, 0, c]
    return x, g


# ---- BOUNDARY_MOVES: order 1, d = 3 (k = 3), n = 64; chain -> (the only kept steps at which it changes, info or None
# for "whatever the factorisation finds").  Only at t = 16, 32, 48 does `prev`, carried from one staged block to the
# next, decide the move count.  A healthy chain lies between each of them.
BOUNDARY_ORDER, BOUNDARY_D, BOUNDARY_N, BOUNDARY_C = 1, 3, 64, 9
BOUNDARY_MOVES = {1: ((16, 32, 48), None), 3: ((16, 32), 3), 5: ((15, 17), 3), 7: ((63,), 2)}


def boundary_inputs():
    x, g = synthetic(BOUNDARY_D, BOUNDARY_C, BOUNDARY_N, seed=seed_of(BOUNDARY_ORDER, BOUNDARY_D))
    for c, (at, _) in BOUNDARY_MOVES.items():
        state = np.searchsorted(np.asarray(at), np.arange(BOUNDARY_N), side="right")    # 0 .. len(at), held in stretches
        x[:, :, c] = x[state, :, c]
        g[:, :, c] = g[state, :, c]
    return x, g


# ---- MANY_TILES: (order, d, C, n): the grid index and the ragged last tile at a block count well above the CU count
MANY_TILES = ((1, 1, 16 * 1024 + 1, 3), (2, 1, 4097, 3))
