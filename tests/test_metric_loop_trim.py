"""The d = 32 RWM step loop after its instruction trim: bitwise parity on the GPU, and the accept screen on the CPU.

The trim changes how the pair kernels `lpp_rwm` broadcast the accept uniform (one swap pair per two
steps: a launch's even step keeps half 1's uniform for its odd step), how they form the Box-Muller radius index and
the angle polynomials' constants, and the single-precision screen of `ratio > log(rand())` that every RWM / MALA
kernel shares (`detmath.hpp` `gt_det_log`).  None of it may change a bit of the output:

- the GPU tests compare samples, accept bits, final state and lp with `oracle_ref.OracleChains` for the d = 32
  iso-Normal under RWM(0.1) at C in {1, 31, 33, 257} (C <= 64 runs the look-ahead kernel `lpc_rwm_la`, which shares
  the radius and angle code; 65 and 97 are added so that the pair kernel itself runs with a dead half-wave -- 97
  chains are three full waves and one chain -- and 257 is a full block and one chain), runs of 7 and 8 steps with
  burnin 1 and thinning 2, and `steps_per_launch` in {0, 1, 3}: launches of odd length, which draw a pair and drop
  its second uniform, and launches that begin on an odd step index;
- one case at d = 20, the instance with per-coordinate validity masks, which shares the accept draw and the screen;
- the CPU test runs a numpy twin of the screen over a grid of uniforms and ratios placed just outside and just
  inside the undecided band, and checks every decided lane against `ratio > log(u)`.
"""
import numpy as np
import pytest

import mcmchip as mc
import oracle_ref as orc


def _model(d):
    return mc.model(mc.IsoNormalDot(), init=np.ones(d))          # bench.py's RWM model (README.md:60)


def _kernel(d, C):
    nb = (d + 3) // 4
    if C <= 64:
        return f"lpc_rwm_la<{nb}, IsoDot, true>"
    full = "true" if d % 8 == 0 else "false"
    return f"lpp_rwm<{(nb + 1) // 2}, {full}, IsoDot, true>"


def _run_and_compare(d, C, steps, spl):
    m = _model(d)
    r = mc.SerialMC(steps=steps, burnin=1, thinning=2)
    t = (m * mc.RWM(0.1) * r).batch(C, seed=5, steps_per_launch=spl)
    ch = mc.run(t)
    assert t.step_kernel == _kernel(d, C)
    oc = orc.OracleChains(m, mc.RWM(0.1), nchains=C, seed=5)
    s_ref, _, acc_ref = oc.run(r)
    assert ch._samples.shape == s_ref.shape
    assert np.array_equal(ch._samples.view(np.uint64), s_ref.view(np.uint64)), "samples not bit-identical"
    assert np.array_equal(ch.diagnostics["accept"].T, acc_ref.astype(bool)), "accept bits differ"
    assert np.array_equal(ch.final_x.view(np.uint64), oc.x.view(np.uint64)), "final state not bit-identical"
    assert np.array_equal(ch.final_lp.view(np.uint64), oc.lp.view(np.uint64)), "final lp not bit-identical"


@pytest.mark.gpu
@pytest.mark.parametrize("spl", [0, 1, 3])
@pytest.mark.parametrize("steps", [7, 8])
@pytest.mark.parametrize("C", [1, 31, 33, 65, 97, 257])
def test_metric_rwm_parity(gpu, C, steps, spl):
    _run_and_compare(32, C, steps, spl)


@pytest.mark.gpu
@pytest.mark.parametrize("spl", [0, 3])
def test_masked_pair_instance_parity(gpu, spl):
    """d = 20: `lpp_rwm<3, false, ...>`, three waves a SIMD, per-coordinate validity masks"""
    _run_and_compare(20, 257, 7, spl)


# ---------------------------------------------------------------------------------------------- the screen, on the CPU
LN2 = float.fromhex("0x1.62e42fefa39efp-1")


def _screen(ratio, u, ulp_shift=0):
    """gt_det_log's screen in numpy, operation for operation: L = RN(double(log2f(float(u))) ln2), d = RN(ratio - L),
    E = fma(|L|, 2^-16, 2^-16); returns (decided, accept).  ulp_shift moves the single-precision log2 by that many
    float ulps (the hardware's is within one of the correctly rounded value).  |L| 2^-16 is exact (a power-of-two
    scale), so the fma is the one rounding of the sum that the addition here performs."""
    with np.errstate(divide="ignore", invalid="ignore"):
        lf = np.log2(np.asarray(u, dtype=np.float64).astype(np.float32))
        for _ in range(abs(ulp_shift)):
            lf = np.nextafter(lf, np.float32(np.inf if ulp_shift > 0 else -np.inf))
        L = lf.astype(np.float64) * LN2
        d = ratio - L
        E = np.abs(L) * 2.0 ** -16 + 2.0 ** -16
        return np.abs(d) > E, d > 0.0


def _uniform_grid():
    rng = np.random.default_rng(7)
    edge = [2.0 ** -52, 2.0 ** -51, 3 * 2.0 ** -52, 2.0 ** -30, 1e-5, 0.25, 0.5, 1 - 2.0 ** -10, 1 - 2.0 ** -24,
            1 - 2.0 ** -25, 1 - 2.0 ** -26, 1 - 2.0 ** -52, 1 - 2.0 ** -53]
    k = rng.integers(1, 2 ** 52, 4000).astype(np.float64) * 2.0 ** -52      # rand()'s own grid
    near1 = 1 - rng.integers(1, 2 ** 30, 500).astype(np.float64) * 2.0 ** -53
    small = rng.integers(1, 2 ** 20, 500).astype(np.float64) * 2.0 ** -52
    return np.concatenate([np.array(edge), k, near1, small])


@pytest.mark.parametrize("ulp_shift", [-1, 0, 1])
def test_accept_screen_agrees_with_exact_test(ulp_shift):
    u = _uniform_grid()
    exact_log = np.log(u)
    with np.errstate(divide="ignore"):
        lf = np.log2(u.astype(np.float32))
    L = lf.astype(np.float64) * LN2
    E = np.abs(L) * 2.0 ** -16 + 2.0 ** -16
    n_dec = n_und = 0
    for sign in (1.0, -1.0):
        for f in (1 + 2.0 ** -20, 1 - 2.0 ** -20, 4.0, 0.0, 0.5):
            ratio = L + sign * E * f
            decided, acc = _screen(ratio, u, ulp_shift)
            want = ratio > exact_log
            assert np.array_equal(acc[decided], want[decided]), (sign, f)
            if ulp_shift == 0:
                # just outside the band every lane is decided; inside it none is
                if f > 1:
                    assert decided.all(), (sign, f)
                elif f < 1:
                    assert not decided.any(), (sign, f)
            n_dec += int(decided.sum())
            n_und += int((~decided).sum())
    assert n_dec > 0 and n_und > 0
    # ratios unrelated to L: the common case, all decided except by coincidence, all right
    rng = np.random.default_rng(11)
    ratio = -rng.exponential(3.0, u.size)
    decided, acc = _screen(ratio, u, ulp_shift)
    assert decided.mean() > 0.99
    assert np.array_equal(acc[decided], (ratio > exact_log)[decided])


def test_accept_screen_special_values():
    # u = 0: L = -inf, d = +inf and E = +inf (or d NaN for ratio = -inf): never decided, the exact test runs
    for ratio in (-1.0, -1e300, -np.inf, 0.0):
        decided, _ = _screen(np.float64(ratio), np.array([0.0]))
        assert not decided.any()
    # NaN ratio: undecided; ratio = -inf against a finite L: decided, rejected (as -inf > log(u) is)
    decided, _ = _screen(np.float64(np.nan), np.array([0.3, 2.0 ** -52, 1 - 2.0 ** -53]))
    assert not decided.any()
    decided, acc = _screen(np.float64(-np.inf), np.array([0.3, 2.0 ** -52, 1 - 2.0 ** -53]))
    assert decided.all() and not acc.any()
