"""The premises of the ZV kernel cases (tests/zv_cases.py), asserted with the checker alone (tests/zv_oracle.c through
zv_ref.zv): every kernel instance and every class of kept-step count is met, the failing chains fail at the stated
pivot with NaN in zv and coef, and their neighbours equal the checker's answer for the unmodified inputs bit for bit.
tests/test_zv_gpu.py then runs the same tables on the device.
"""
import functools

import numpy as np
import pytest

import mcmchip as mc
import oracle_ref as orc
import zv_cases as zc
import zv_ref


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_instance_of_restates_the_dispatch():
    assert len(set((o, ntk, ntd) for o, _, _, ntk, ntd in zc.INSTANCES)) == len(zc.INSTANCES) == 5
    for order, dmax in ((1, 32), (2, 8)):
        for d in range(1, dmax + 1):
            rows = [(o, ntk, ntd) for o, lo, hi, ntk, ntd in zc.INSTANCES if o == order and lo <= d <= hi]
            assert rows == [zc.instance_of(order, d)], (order, d)
            _, ntk, ntd = rows[0]
            k = zv_ref.k_of(order, d)
            assert ntk == -(-k // 16) and ntd >= -(-d // 16), (order, d)       # the MFMA tiles hold k and d


def test_parity_meets_every_instance_width_and_count():
    seen = {}
    for order, d, C, n in zc.PARITY:
        assert n > zv_ref.k_of(order, d) and C in zc.CHAINS
        assert n in zc.NKEPT + (63, zv_ref.k_of(order, d) + 1, zv_ref.k_of(order, d) + 2)
        seen.setdefault((order, d), set()).add(n)
    assert len(set(zc.PARITY)) == len(zc.PARITY)
    assert set(seen) == {(2, d) for d in range(1, 9)} | {(1, d) for d in (1, 2, 15, 16, 17, 31, 32)}
    for (order, d), ns in seen.items():
        k = zv_ref.k_of(order, d)
        assert k + 1 in ns and k + 2 in ns, (order, d)
        assert {n for n in zc.NKEPT if n > k} <= ns, (order, d)
        for r in (0, zc.TT - 1, 1):                                 # a multiple of 16, one below, one above
            assert any(n % zc.TT == r for n in ns), (order, d, r)
    for order, lo, hi, ntk, ntd in zc.INSTANCES:                    # all five, at their smallest and largest d
        inst = (order, ntk, ntd)
        assert zc.instance_of(order, lo) == zc.instance_of(order, hi) == inst
        assert (order, lo) in seen and (order, hi) in seen, inst
        cs = {C for o, d, C, _ in zc.PARITY if zc.instance_of(o, d) == inst}
        assert cs == set(zc.CHAINS), inst


@pytest.mark.parametrize("order,d", zc.WIDTHS)
def test_parity_widths_factorise_on_33_chains(order, d):
    for n in zc.nkept_of(order, d):
        z, a, info = zc.case(order, d, 33, n)[2]
        assert not info.any(), (n, info)
        assert np.isfinite(z).all() and np.isfinite(a).all(), n


def test_parity_cases_factorise():
    for order, d, C, n in zc.PARITY:
        z, a, info = zc.case(order, d, C, n)[2]
        assert not info.any() and np.isfinite(z).all() and np.isfinite(a).all(), (order, d, C, n)


def check_bad(order, d, x, g, chains, want_info):
    """the bad chains: info and NaN; every other chain: finite, and the checker's answer for the unmodified inputs"""
    z, a, info = zv_ref.zv(order, x, g)
    z0, a0, i0 = zc.healthy(order, d)[2]
    assert not i0.any()
    good = np.setdiff1d(np.arange(zc.BAD_C), chains)
    assert (info[list(chains)] == want_info).all(), info[list(chains)]
    assert np.isnan(z[:, :, chains]).all() and np.isnan(a[:, :, chains]).all()
    assert not info[good].any() and np.isfinite(z[:, :, good]).all() and np.isfinite(a[:, :, good]).all()
    assert np.array_equal(bits(z[:, :, good]), bits(z0[:, :, good]))
    assert np.array_equal(bits(a[:, :, good]), bits(a0[:, :, good]))


def test_placements_cover_the_tile():
    assert zc.PLACEMENTS == ((3,), (11,), (3, 11, 16, 32)) and zc.BAD_C == 33
    assert 3 % 8 == 11 % 8 and 3 // 16 == 11 // 16                  # one solve block, one after the other


@pytest.mark.parametrize("order,d,j,chains", zc.PIVOT)
def test_pivot_cases_fail_at_their_pivot(order, d, j, chains):
    x, g = zc.pivot_inputs(order, d, j, chains)
    n, k = x.shape[0], zv_ref.k_of(order, d)
    assert n == max(61, k + 5) and 1 <= j + 1 <= k
    for c in chains:                                                # n - 1 moves: not the counting rule
        assert (np.abs(np.diff(x[:, :, c], axis=0)).max(axis=1) > 0).all()
    check_bad(order, d, x, g, chains, j + 1)


@pytest.mark.parametrize("order,d,j,v,chains", zc.NONFINITE)
def test_nonfinite_cases_fail_at_their_pivot(order, d, j, v, chains):
    x, g = zc.nonfinite_inputs(order, d, j, v, chains)
    check_bad(order, d, x, g, chains, j + 1)


def test_nonfinite_table():
    assert len(zc.NONFINITE) == 24 * len(zc.PLACEMENTS)
    assert np.isnan(zc.NONFINITE_VALUES[0]) and zc.NONFINITE_VALUES[1:] == (np.inf, 1e200)
    assert {zc.instance_of(o, d) for o, d, *_ in zc.NONFINITE} == {(1, 1, 1), (1, 2, 2), (2, 1, 1), (2, 2, 1)}
    assert {zc.instance_of(o, d) for o, d, *_ in zc.PIVOT} == {(o, ntk, ntd) for o, _, _, ntk, ntd in zc.INSTANCES}


@pytest.mark.parametrize("order,d", zc.DUPLICATE)
def test_duplicate_cases(order, d):
    """G is exactly singular, the second pivot rounding residue: whether it factorises is not a premise (measured with
    the checker on these inputs: info 0, 0, 2 -- in both linear cases the residue is positive and factorises, to
    coefficients of ordinary size, max |a| 2.3 and 2.5 beside the unmodified chain's 2.2 and 2.4); the neighbours are"""
    x, g = zc.duplicate_inputs(order, d)
    z, a, info = zv_ref.zv(order, x, g)
    print(f"order {order} d {d}: info {info[zc.DUPLICATE_CHAIN]}")
    assert info[zc.DUPLICATE_CHAIN] in (0, 2)
    z0, a0, _ = zc.healthy(order, d)[2]
    good = np.delete(np.arange(zc.BAD_C), zc.DUPLICATE_CHAIN)
    assert not info[good].any()
    assert np.array_equal(bits(z[:, :, good]), bits(z0[:, :, good]))
    assert np.array_equal(bits(a[:, :, good]), bits(a0[:, :, good]))
    bad = info[zc.DUPLICATE_CHAIN] != 0
    assert np.isnan(z[:, :, zc.DUPLICATE_CHAIN]).all() == np.isnan(a[:, :, zc.DUPLICATE_CHAIN]).all() == bad


def test_boundary_moves():
    x, g = zc.boundary_inputs()
    assert x.shape == (64, 3, 9) and zv_ref.k_of(zc.BOUNDARY_ORDER, zc.BOUNDARY_D) == 3
    z, a, info = zv_ref.zv(zc.BOUNDARY_ORDER, x, g)
    for c in range(zc.BOUNDARY_C):
        moved = np.flatnonzero((np.diff(x[:, :, c], axis=0) != 0).any(axis=1) |
                               (np.diff(g[:, :, c], axis=0) != 0).any(axis=1)) + 1
        if c in zc.BOUNDARY_MOVES:
            at, want = zc.BOUNDARY_MOVES[c]
            assert tuple(moved) == at
            if want is not None:
                assert info[c] == want == len(at) + 1
        else:
            assert len(moved) == 63 and info[c] == 0 and np.isfinite(z[:, :, c]).all()
        assert np.isnan(z[:, :, c]).all() == np.isnan(a[:, :, c]).all() == (info[c] != 0)
    assert zc.BOUNDARY_MOVES[1][0] == (16, 32, 48) and len(zc.BOUNDARY_MOVES[1][0]) == 3      # = k: factorised


@pytest.mark.parametrize("order,d,C,n", zc.MANY_TILES)
def test_many_tiles_cases(order, d, C, n):
    x, g, (z, a, info) = zc.case(order, d, C, n)
    assert n == zv_ref.k_of(order, d) + (2 if order == 1 else 1) and C % 16 == 1 and C // 16 >= 256
    assert x.nbytes <= 512 * 1024
    assert ((info != 0) == np.isnan(z).all(axis=(0, 1))).all() and ((info != 0) == np.isnan(a).all(axis=(0, 1))).all()
    assert np.isfinite(z[:, :, info == 0]).all() and (info == 0).sum() >= C // 2


@functools.lru_cache(maxsize=None)
def normal_hmc_d5():
    """the CPU oracle's HMC run on NormalDSL(1, 2), d = 5, 70 chains: (samples, grads) [60][5][70]"""
    m = mc.model(mc.NormalDSL(1, 2), v=np.ones(5), gradient=True)
    s, g, _ = orc.OracleChains(m, mc.HMC(), 70, seed=1).run(mc.SerialMC(steps=60))
    s.setflags(write=False)
    g.setflags(write=False)
    return s, g


def moves_of(s, g):
    """per chain, the kept steps that differ from the one before"""
    return ((np.diff(s, axis=0) != 0) | (np.diff(g, axis=0) != 0)).any(axis=1).sum(axis=0)


def test_quadratic_run_on_the_two_tile_instance():
    """what the oracle's run says about info: a chain with fewer than k = 20 moves has info = moves + 1"""
    s, g = normal_hmc_d5()
    assert s.shape == (60, 5, 70) and zc.instance_of(2, 5) == (2, 2, 1)
    moves = moves_of(s, g)
    z, a, info = zv_ref.zv(2, s, g)
    print(f"moves {moves.min()} .. {moves.max()}, info != 0 on {np.count_nonzero(info)} chains")
    few = moves < 20
    assert np.array_equal(info[few], moves[few] + 1)
    assert ((info != 0) == np.isnan(z).all(axis=(0, 1))).all()
