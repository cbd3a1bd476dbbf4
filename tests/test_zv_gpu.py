"""Zero-variance estimators on the device (kernels/zv.hip, mcmc_stats_zv) against the checker (tests/zv_oracle.c),
bit for bit on zv, coef and info: the MFMA row-tile edge d = 16 | 17, ragged chain tiles, the minimum nkept = k + 1,
a remainder of the MFMA k = 4 and an odd staging tail, a singular chain inside a tile, the device-pointer path, a real
run, and the refusals.

The tables of tests/zv_cases.py (their premises asserted with the checker alone in tests/test_zv_cases_cpu.py) add:
every one of the five instances k_zv<F, NTK, NTD> at its smallest and largest width -- <ZvQuadratic, 2, 1> (d = 5, 6)
among them -- with nkept at, one below and one above the multiples of the 16-step staging block; chains whose
factorisation fails inside zv_solve at the pivot of the first, a middle and the last gradient coordinate (an exact zero,
NaN, +inf, an overflowing Gram diagonal), placed before, after and beside a healthy chain of the same solve block, at a tile's first chain and in a
ragged tile, with every other chain equal to a run of the unmodified inputs; a duplicated coordinate, whose pivot is
rounding residue; chains whose only moves lie on the staging block's boundaries; a grid of a thousand tiles; the
device-pointer path and a real quadratic run on the two-tile instance.
"""
import ctypes as ct
import functools

import numpy as np
import pytest

import mcmchip as mc
import zv_cases as zc
import zv_ref
from mcmchip import _lib, stats
from test_zv import STUCK, normal_hmc, stuck_inputs
from test_zv_cases_cpu import moves_of, normal_hmc_d5

# a pairwise-sparse subset of d x C x nkept (nkept: 0 -> d + 1, 1 -> d + 2, else itself): every d meets every kind of
# nkept, every C every d class
LINEAR = [(1, 1, 0), (1, 17, 1), (1, 70, 61), (3, 17, 0), (3, 70, 1), (3, 1, 61), (16, 70, 0), (16, 1, 1),
          (16, 17, 61), (17, 17, 0), (17, 70, 1), (17, 1, 61), (32, 1, 0), (32, 17, 1), (32, 70, 61)]
QUADRATIC = [(d, 17, nk) for d in (1, 2, 3, 8) for nk in (0, 61)]        # 0 -> k + 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _n(order, d, nk):
    k = zv_ref.k_of(order, d)
    return k + 1 if nk == 0 else k + 2 if nk == 1 else nk


case = zc.case          # (order, d, C, n) -> inputs (seed 100 order + d) and the checker's answer, computed once


def device_zv(order, x, g, coef=True, info=True):
    """mcmc_stats_zv on host arrays [n][d][C] -> (zv, coef, info) in the same layout"""
    n, d, C = x.shape
    z = np.empty((n, d, C))
    a = np.empty((zv_ref.k_of(order, d), d, C)) if coef else None
    i = np.empty(C, dtype=np.int32) if info else None
    from mcmchip.api import _ctx
    _lib.check(_lib.load().mcmc_stats_zv(_ctx(0), order, x.ctypes.data, g.ctypes.data, n, d, C, 0, z.ctypes.data,
                                         a.ctypes.data if coef else None, i.ctypes.data if info else None))
    return z, a, i


def assert_same(got, want, what=""):
    assert np.array_equal(got[2], want[2]), what + ": info"
    assert np.array_equal(bits(got[1]), bits(want[1])), what + ": coef"
    assert np.array_equal(bits(got[0]), bits(want[0])), what + ": zv"


@pytest.mark.gpu
@pytest.mark.parametrize("d,C,nk", LINEAR)
def test_linear_matches_checker(gpu, d, C, nk):
    x, g, want = case(1, d, C, _n(1, d, nk))
    assert_same(device_zv(1, x, g), want)
    assert not want[2].any()


@pytest.mark.gpu
@pytest.mark.parametrize("d,C,nk", QUADRATIC)
def test_quadratic_matches_checker(gpu, d, C, nk):
    x, g, want = case(2, d, C, _n(2, d, nk))
    assert_same(device_zv(2, x, g), want)


@pytest.mark.gpu
def test_singular_chain_leaves_its_tile_alone(gpu):
    x0, g0, want0 = case(1, 3, 17, 61)
    x, g = x0.copy(), g0.copy()
    x[:, :, 5] = x[0, :, 5]
    g[:, :, 5] = g[0, :, 5]
    z, a, info = device_zv(1, x, g)
    assert info[5] == 1 and not np.delete(info, 5).any()
    assert np.isnan(z[:, :, 5]).all() and np.isnan(a[:, :, 5]).all()
    z0, a0, _ = device_zv(1, x0, g0)
    assert np.array_equal(bits(np.delete(z, 5, axis=2)), bits(np.delete(z0, 5, axis=2)))
    assert np.array_equal(bits(np.delete(a, 5, axis=2)), bits(np.delete(a0, 5, axis=2)))
    assert_same((z, a, info), zv_ref.zv(1, x, g), "against the checker")


@pytest.mark.gpu
@pytest.mark.parametrize("order,d", STUCK)
def test_stuck_chains_are_marked_whatever_their_value(gpu, order, d):
    """chains that never moved (several constants) and chains with too few moves, at the small widths and at one width of
    every kernel instance: info, NaN and the healthy neighbours as the checker has them"""
    x, g, want = stuck_inputs(order, d)
    got = device_zv(order, x, g)
    for c, w in enumerate(want):
        if w is not None:
            assert got[2][c] == w, (c, got[2][c], w)
    assert np.isnan(got[0][:, :, 1:1 + 7]).all() and got[2][0] == 0
    assert_same(got, zv_ref.zv(order, x, g))


@pytest.mark.gpu
def test_device_pointers_and_null_outputs(gpu):
    import torch
    x, g, want = case(2, 3, 17, 61)
    dev = torch.device("cuda", 0)
    tx, tg = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(g.copy()).to(dev)
    z, a, i = stats.zv_device((tx, tg), order=2, return_coef=True, return_info=True)
    assert z.device == tx.device and z.shape == tx.shape
    assert_same((z.cpu().numpy(), a.cpu().numpy(), i.cpu().numpy()), want, "device tensors")
    only = stats.zv_device((tx, tg), order=2)                          # coef = NULL, info = NULL
    assert np.array_equal(bits(only.cpu().numpy()), bits(want[0]))
    zh, _, _ = device_zv(2, x, g, coef=False, info=False)
    assert np.array_equal(bits(zh), bits(want[0]))
    e = stats.ess_device(only)                                         # straight into the ESS kernel
    assert e.shape == (3, 17) and bool(torch.isfinite(e).all())


@pytest.mark.gpu
def test_end_to_end_on_a_real_run(gpu):
    m = mc.model(mc.NormalDSL(1, 2), v=np.ones(3), gradient=True)
    ch = mc.run((m * mc.HMC() * mc.SerialMC(steps=60)).batch(70, seed=1))
    z, a, info = stats.zv_device(ch, return_coef=True, return_info=True)
    want = zv_ref.zv(1, ch._samples, ch._gradients)
    assert z.shape == ch.samples.shape == (70, 60, 3)
    assert_same((z.transpose(1, 2, 0), a.transpose(1, 2, 0), info), want)
    s, g = normal_hmc()
    assert np.array_equal(bits(ch._samples), bits(s)) and np.array_equal(bits(ch._gradients), bits(g))
    assert np.abs(z - 1.0).max() <= 1e-10                              # exact on a Normal target


@pytest.mark.gpu
def test_refusals_and_argument_errors(gpu):
    def call(order, d, n, C=2):
        x = np.zeros((n, d, C))
        with pytest.raises(_lib.MCMCError) as e:
            device_zv(order, x, x)
        return e.value
    e = call(1, 33, 40)
    assert e.code == _lib.MCMC_E_UNSUPPORTED and "d <= 32" in str(e)
    e = call(2, 9, 60)
    assert e.code == _lib.MCMC_E_UNSUPPORTED and "d <= 8" in str(e)
    assert call(1, 3, 3).code == _lib.MCMC_E_INVALID_ARG               # nkept = k
    assert call(2, 3, 9).code == _lib.MCMC_E_INVALID_ARG
    assert call(3, 3, 40).code == _lib.MCMC_E_INVALID_ARG              # unknown order
    from mcmchip.api import _ctx
    z = np.zeros((5, 1, 1))
    assert _lib.load().mcmc_stats_zv(_ctx(0), 1, None, z.ctypes.data, 5, 1, 1, 0, z.ctypes.data, None,
                                     None) == _lib.MCMC_E_INVALID_ARG
    assert _lib.load().mcmc_stats_zv(_ctx(0), 1, z.ctypes.data, z.ctypes.data, 5, 1, 0, 0, z.ctypes.data, None,
                                     None) == _lib.MCMC_E_INVALID_ARG
    m = mc.model(mc.NormalDSL(1, 2), v=np.ones(3), gradient=True)
    ch = mc.run((m * mc.RWM(0.5) * mc.SerialMC(steps=20)).batch(4, seed=1))
    with pytest.raises(ValueError, match="gradients"):
        stats.zv_device(ch)
    with pytest.raises(ValueError, match="gradients"):
        stats.linear_zv(ch)


# ---- the tables of zv_cases.py: every instance, the staging block's edges, chains that fail inside zv_solve


@pytest.mark.gpu
@pytest.mark.parametrize("order,d,C,n", zc.PARITY)
def test_every_instance_matches_checker(gpu, order, d, C, n):
    x, g, want = zc.case(order, d, C, n)
    assert_same(device_zv(order, x, g), want)
    assert not want[2].any()


@functools.lru_cache(maxsize=None)
def device_healthy(order, d):
    """the device's answer for the unmodified inputs of the PIVOT / NONFINITE / DUPLICATE cases, computed once"""
    x, g, want = zc.healthy(order, d)
    got = device_zv(order, x, g)
    assert_same(got, want, "unmodified inputs")
    for v in got:
        v.setflags(write=False)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("order,d,j,v,chains", [(o, d, j, None, p) for o, d, j, p in zc.PIVOT] + list(zc.NONFINITE))
def test_failing_pivot_marks_its_chain_only(gpu, order, d, j, v, chains):
    """pivot j + 1 of a chain with n - 1 moves is an exact zero (v None: PIVOT) or not finite (NONFINITE: one gradient
    entry NaN, +inf or 1e200, the last overflowing the Gram diagonal): zv_solve's failing return, which leaves a partly
    factorised block to the next chain of the solve batch.  NaN out, info = j + 1, every other chain as if nothing
    had failed."""
    x, g = zc.pivot_inputs(order, d, j, chains) if v is None else zc.nonfinite_inputs(order, d, j, v, chains)
    got = device_zv(order, x, g)
    z, a, info = got
    bad = list(chains)
    assert (info[bad] == j + 1).all() and not np.delete(info, bad).any(), info
    assert np.isnan(z[:, :, bad]).all() and np.isnan(a[:, :, bad]).all()
    assert_same(got, zv_ref.zv(order, x, g), "against the checker")
    z0, a0, _ = device_healthy(order, d)
    assert np.array_equal(bits(np.delete(z, bad, axis=2)), bits(np.delete(z0, bad, axis=2)))
    assert np.array_equal(bits(np.delete(a, bad, axis=2)), bits(np.delete(a0, bad, axis=2)))


@pytest.mark.gpu
@pytest.mark.parametrize("order,d", zc.DUPLICATE)
def test_duplicate_coordinate_factorises_like_the_checker(gpu, order, d):
    """an exactly singular G whose second pivot is rounding residue: any change in the order of operations shows"""
    x, g = zc.duplicate_inputs(order, d)
    got = device_zv(order, x, g)
    assert_same(got, zv_ref.zv(order, x, g))
    z0, a0, _ = device_healthy(order, d)
    c = zc.DUPLICATE_CHAIN
    assert np.array_equal(bits(np.delete(got[0], c, axis=2)), bits(np.delete(z0, c, axis=2)))
    assert np.array_equal(bits(np.delete(got[1], c, axis=2)), bits(np.delete(a0, c, axis=2)))


@pytest.mark.gpu
def test_moves_on_staging_block_boundaries(gpu):
    x, g = zc.boundary_inputs()
    got = device_zv(zc.BOUNDARY_ORDER, x, g)
    for c in range(zc.BOUNDARY_C):
        want = zc.BOUNDARY_MOVES[c][1] if c in zc.BOUNDARY_MOVES else 0
        if want is not None:
            assert got[2][c] == want, (c, got[2][c], want)
    assert_same(got, zv_ref.zv(zc.BOUNDARY_ORDER, x, g))


@pytest.mark.gpu
@pytest.mark.parametrize("order,d,C,n", zc.MANY_TILES)
def test_many_tiles(gpu, order, d, C, n):
    x, g, want = zc.case(order, d, C, n)
    assert_same(device_zv(order, x, g), want)


@pytest.mark.gpu
def test_device_pointers_and_null_outputs_two_tile_instance(gpu):
    import torch
    x, g, want = zc.case(2, 6, 17, 33)
    assert zc.instance_of(2, 6) == (2, 2, 1)
    dev = torch.device("cuda", 0)
    tx, tg = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(g.copy()).to(dev)
    z, a, i = stats.zv_device((tx, tg), order=2, return_coef=True, return_info=True)
    assert z.device == tx.device and z.shape == tx.shape and a.shape == (27, 6, 17) and i.shape == (17,)
    assert_same((z.cpu().numpy(), a.cpu().numpy(), i.cpu().numpy()), want, "device tensors")
    only = stats.zv_device((tx, tg), order=2)                          # coef = NULL, info = NULL
    assert np.array_equal(bits(only.cpu().numpy()), bits(want[0]))
    assert np.array_equal(bits(tx.cpu().numpy()), bits(x)) and np.array_equal(bits(tg.cpu().numpy()), bits(g))


@pytest.mark.gpu
def test_end_to_end_quadratic_on_the_two_tile_instance(gpu):
    m = mc.model(mc.NormalDSL(1, 2), v=np.ones(5), gradient=True)
    ch = mc.run((m * mc.HMC() * mc.SerialMC(steps=60)).batch(70, seed=1))
    z, a, info = stats.zv_device(ch, order=2, return_coef=True, return_info=True)
    want = zv_ref.zv(2, ch._samples, ch._gradients)
    assert z.shape == ch.samples.shape == (70, 60, 5) and a.shape == (70, 20, 5)
    assert_same((z.transpose(1, 2, 0), a.transpose(1, 2, 0), info), want)
    s, g = normal_hmc_d5()                                             # the CPU oracle's run says what info must be
    assert np.array_equal(bits(ch._samples), bits(s)) and np.array_equal(bits(ch._gradients), bits(g))
    moves = moves_of(s, g)
    few = moves < 20
    assert np.array_equal(info[few], moves[few] + 1)
