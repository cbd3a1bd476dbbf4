"""Zero-variance estimators (reference src/stats/zv.jl:8-68) -- the CPU side: the checker (tests/zv_oracle.c through
zv_ref, a scalar restatement of the arithmetic kernels/zv.hip documents) against the literal numpy transcription
(mcmchip.stats.linear_zv / quadratic_zv: np.cov + np.linalg.inv), and the properties that make ZV worth having.

Measured here (gcc, numpy 2.x): checker vs transcription 4e-16 .. 3e-15 on a and 8e-16 .. 1.1e-14 on
zv, relative to max |a| / max |zv|, at Gram condition numbers 1 .. 22; |zv - 1| <= 2.7e-15 on the Normal target;
across-chain variance of the logistic MALA posterior mean shrinks to 0.58 - 1.1 % (linear ZV) of the plain mean's.
"""
import functools

import numpy as np
import pytest

import glm_cases
import mcmchip as mc
import oracle_ref as orc
import zv_ref
from mcmchip import stats

PARITY_BOUND = 1e-10                       # the project's stated parity bound
# (order, d, nkept): the Gram matrix cov(w) of every chain has condition number <= 100 (asserted)
SYNTHETIC = ((1, 1, 50), (1, 3, 200), (1, 32, 400), (2, 1, 50), (2, 3, 400))


def synthetic(d, C, n, seed=7):
    """Correlated Gaussian draws and the gradient of a nearby, slightly non-Gaussian log-density plus noise, in the
    C-ABI layout [n][d][C]: neither exactly affine (ZV would be exact) nor degenerate."""
    rng = np.random.default_rng(seed)
    A = np.eye(d) + 0.3 * rng.standard_normal((d, d)) / np.sqrt(d)
    x = rng.standard_normal((n, C, d)) @ A.T + 0.5
    P = np.eye(d) + 0.2 * np.ones((d, d)) / d
    g = -(x - 0.5) @ P + 0.3 * np.tanh(x) + 0.1 * rng.standard_normal((n, C, d))
    return np.ascontiguousarray(x.transpose(0, 2, 1)), np.ascontiguousarray(g.transpose(0, 2, 1))


def control_variates(order, x, g):
    """[n, k] control variates of one chain, written out independently of stats.py: x, g [n, d]"""
    z = -g / 2
    if order == 1:
        return z
    d = x.shape[1]
    cols = [z, 2 * z * x - 1]
    cols += [(x[:, i] * z[:, j] + x[:, j] * z[:, i])[:, None] for i in range(d - 1) for j in range(i + 1, d)]
    return np.column_stack(cols)


@pytest.mark.parametrize("order,d,n", SYNTHETIC)
def test_checker_matches_literal_transcription(order, d, n):
    C = 5
    x, g = synthetic(d, C, n)
    for c in range(C):
        cond = np.linalg.cond(np.atleast_2d(np.cov(control_variates(order, x[:, :, c], g[:, :, c]), rowvar=False)))
        assert cond <= 100, (c, cond)
    zo, ao, info = zv_ref.zv(order, x, g)
    f = stats.linear_zv if order == 1 else stats.quadratic_zv
    zl, al = f(x.transpose(2, 0, 1), g.transpose(2, 0, 1))
    assert not info.any()
    assert zl.shape == (C, n, d) and al.shape == (C, zv_ref.k_of(order, d), d)
    ea = np.abs(ao.transpose(2, 0, 1) - al).max() / np.abs(al).max()
    ez = np.abs(zo.transpose(2, 0, 1) - zl).max() / np.abs(zl).max()
    print(f"order {order} d {d} n {n}: a {ea:.2e} zv {ez:.2e}")
    assert ea <= PARITY_BOUND and ez <= PARITY_BOUND


@functools.lru_cache(maxsize=None)
def normal_hmc():
    """the checker's HMC run on NormalDSL(1, 2), d = 3, 70 chains: (samples, grads) [60][3][70]"""
    m = mc.model(mc.NormalDSL(1, 2), v=np.ones(3), gradient=True)
    s, g, _ = orc.OracleChains(m, mc.HMC(), 70, seed=1).run(mc.SerialMC(steps=60))
    s.setflags(write=False)
    g.setflags(write=False)
    return s, g


def test_linear_zv_is_exact_on_a_normal_target():
    """z = (x - 1) / 8 is affine in x, so a = -8 I and every ZV draw is the target mean"""
    s, g = normal_hmc()
    assert np.ptp(s, axis=0).min() > 0                                  # every chain moved
    zo, ao, info = zv_ref.zv(1, s, g)
    assert not info.any()
    assert np.abs(zo - 1.0).max() <= 1e-10
    assert np.abs(ao - (-8.0 * np.eye(3))[:, :, None]).max() <= 1e-10 * 8
    zl, _ = stats.linear_zv(s.transpose(2, 0, 1), g.transpose(2, 0, 1))
    assert np.abs(zl - 1.0).max() <= 1e-10


def test_zv_reduces_the_variance_of_a_posterior_mean():
    """logistic regression (40 observations, d = 3), MALA, 64 chains, 200 kept: the across-chain variance of the
    per-chain ZV mean is below the plain mean's for every coordinate (measured ratios: linear 0.0058 .. 0.011,
    quadratic 0.0013 .. 0.0016)"""
    m = glm_cases.make_model("logistic", 40, 3)
    s, g, _ = orc.OracleChains(m, mc.MALA(0.1), 64, seed=1).run(mc.SerialMC(steps=400, burnin=200))
    assert s.shape == (200, 3, 64)
    plain = s.mean(axis=0).var(axis=1, ddof=1)
    for order in (1, 2):
        z, _, info = zv_ref.zv(order, s, g)
        assert not info.any()
        v = z.mean(axis=0).var(axis=1, ddof=1)
        print(f"order {order}: variance ratios {v / plain}")
        assert (v < plain).all()
    zl, _ = stats.linear_zv(s.transpose(2, 0, 1), g.transpose(2, 0, 1))
    assert (zl.mean(axis=1).var(axis=0, ddof=1) < plain).all()


def test_quadratic_column_order():
    """d = 3, k = 9: z1 z2 z3 | 2 z_j x_j - 1 | (1,2) (1,3) (2,3), zv.jl:46-53.  With a = e_i e_0^T the estimator
    returns x_0 + w_i, which exposes column i of both implementations."""
    rng = np.random.default_rng(11)
    n = 40
    x, g = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    z = -g / 2
    want = np.column_stack([z[:, 0], z[:, 1], z[:, 2],
                            2 * z[:, 0] * x[:, 0] - 1, 2 * z[:, 1] * x[:, 1] - 1, 2 * z[:, 2] * x[:, 2] - 1,
                            x[:, 0] * z[:, 1] + x[:, 1] * z[:, 0], x[:, 0] * z[:, 2] + x[:, 2] * z[:, 0],
                            x[:, 1] * z[:, 2] + x[:, 2] * z[:, 1]])
    assert want.shape == (n, 9) == (n, zv_ref.k_of(2, 3))
    assert np.array_equal(control_variates(2, x, g), want)
    for impl in ("checker", "numpy"):
        if impl == "checker":
            zc, a, _ = zv_ref.zv(2, x[:, :, None], g[:, :, None])
            zc, a = zc[:, :, 0], a[:, :, 0]
        else:
            zc, a = stats.quadratic_zv(x[None], g[None])
            zc, a = zc[0], a[0]
        assert a.shape == (9, 3)
        assert np.allclose(zc, x + want @ a, rtol=0, atol=1e-12), impl          # the columns, in this order
        # and a solves the normal equations of exactly these columns
        cov = np.cov(np.column_stack([want, x]), rowvar=False)
        assert np.allclose(cov[:9, :9] @ a, -cov[:9, 9:], rtol=0, atol=1e-12), impl


def test_python_surface():
    assert {"linear_zv", "quadratic_zv", "zv_device"} <= set(stats.__all__)
    assert mc.linear_zv is stats.linear_zv and mc.quadratic_zv is stats.quadratic_zv and mc.zv_device is stats.zv_device
    from mcmchip import _lib
    assert "mcmc_stats_zv" in _lib.EXPORTED_SYMBOLS and (_lib.ZV_LINEAR, _lib.ZV_QUADRATIC) == (1, 2)
    with pytest.raises(ValueError, match="Unknown ZV order"):
        stats.zv_device((np.zeros((5, 1, 1)), np.zeros((5, 1, 1))), order=3)


# (order, d): the small widths, where a stuck chain's rounding residue most often factorises "successfully", then the
# largest width of the one-tile quadratic instance and one width for each kernel instance the small ones do not select
STUCK = ((1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (1, 8), (1, 17), (2, 4), (2, 5), (2, 7))
STUCK_VALUES = (0.0, 1.0, -1e-3, 0.1, 57.3, 1e4 / 3, 1e-300)


def stuck_inputs(order, d, n=61):
    """[n][d][C]: chain 0 healthy, then for every constant in STUCK_VALUES a chain that never moved (x = the constant
    times 1 + j / 7, its own gradient), then chains with 1 .. k - 1 moves (too few for rank k) and one with exactly k
    moves.  Returns (x, g, expected info: a number, or None for "whatever the factorisation finds")."""
    k = zv_ref.k_of(order, d)
    C = 1 + len(STUCK_VALUES) + k
    x, g = synthetic(d, C, n, seed=31 * order + d)
    want = [0]
    for c, v in enumerate(STUCK_VALUES, start=1):
        x[:, :, c] = v * (1 + np.arange(d) / 7)
        g[:, :, c] = (0.3 - v) * (1 + np.arange(d) / 3)
        want.append(1)
    for moves in range(1, k + 1):                    # `moves` changes of state, spread over the kept steps
        c = len(STUCK_VALUES) + moves
        state = (np.arange(n) * (moves + 1)) // n    # 0 .. moves, each held for a stretch
        x[:, :, c] = x[state, :, c]
        g[:, :, c] = g[state, :, c]
        want.append(moves + 1 if moves < k else None)
    return x, g, want


@pytest.mark.parametrize("order,d", STUCK)
def test_checker_marks_stuck_chains_whatever_their_value(order, d):
    """a chain that never moved always gets info = 1, one with fewer than k moves info = moves + 1, NaN in both; the
    healthy chain beside them is not touched"""
    x, g, want = stuck_inputs(order, d)
    z, a, info = zv_ref.zv(order, x, g)
    for c, w in enumerate(want):
        if w is not None:
            assert info[c] == w, (c, info[c], w)
        assert np.isnan(z[:, :, c]).all() == np.isnan(a[:, :, c]).all() == (info[c] != 0)
    assert info[0] == 0
    z1, a1, i1 = zv_ref.zv(order, x[:, :, :1], g[:, :, :1])
    assert np.array_equal(z1[:, :, 0], z[:, :, 0]) and np.array_equal(a1[:, :, 0], a[:, :, 0])


def test_checker_marks_a_constant_chain():
    x, g = synthetic(3, 4, 30)
    x[:, :, 2] = x[0, :, 2]
    g[:, :, 2] = g[0, :, 2]
    z, a, info = zv_ref.zv(1, x, g)
    assert info.tolist() == [0, 0, 1, 0]
    assert np.isnan(z[:, :, 2]).all() and np.isnan(a[:, :, 2]).all()
    assert np.isfinite(np.delete(z, 2, axis=2)).all() and np.isfinite(np.delete(a, 2, axis=2)).all()
