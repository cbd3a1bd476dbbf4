"""ERMLMC and RMLMC without a GPU: the constructor forms, the C ABI's validation and the Python refusals, the symmetry
identity vxC(v) = 0.5 X' diag(w o X v) X against the literal C built from the checker's own dG slabs, logdet and solve
of G +- c vxC from the packed factor, the checker's samplers against a literal numpy transcription of
ERMLMC.jl:84-179 and RMLMC.jl:89-179, ERMLMC's volume correction against a finite-difference Jacobian, and the
checker's ERMLMC posterior means against SMMALA's."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import lmc_cases as lc
import manifold_harness as mh
import manifold_ref as lr
import mcmchip as mc
import pmala_cases as pc
import smmala_cases as sc
from mcmchip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNER = mc.EmpiricalMCMCTuner(0.8)


def test_ermlmc_constructor_forms():
    """ERMLMC.jl:37-41"""
    def f(sp):
        return sp.nLeaps, sp.leapStep, sp.tuner
    assert f(mc.ERMLMC()) == (10, 0.1, None)
    assert f(mc.ERMLMC(7)) == (7, 0.1, None)
    assert f(mc.ERMLMC(7, 0.3)) == (7, 0.3, None)
    assert f(mc.ERMLMC(0.3)) == (10, 0.3, None)
    assert f(mc.ERMLMC(0.3, TUNER)) == (10, 0.3, TUNER)
    assert f(mc.ERMLMC(0.3, None)) == (10, 0.3, None)
    assert f(mc.ERMLMC(7, TUNER)) == (7, 0.1, TUNER)
    assert f(mc.ERMLMC(TUNER)) == (10, 0.1, TUNER)
    assert f(mc.ERMLMC(7, 0.3, TUNER)) == (7, 0.3, TUNER)
    assert f(mc.ERMLMC(7, 0.3, None)) == (7, 0.3, None)
    assert f(mc.ERMLMC(init=4, scale=0.2, tuner=TUNER)) == (4, 0.2, TUNER)
    assert f(mc.ERMLMC(scale=0.2)) == (10, 0.2, None)
    assert f(mc.ERMLMC(tuner=TUNER)) == (10, 0.1, TUNER)
    for bad in ((1.0, 2.0), (1, 2), (0.5, 1), (1, 0.5, 2), (1, 0.5, TUNER, 3), (7, None)):
        with pytest.raises(TypeError):
            mc.ERMLMC(*bad)
    with pytest.raises(TypeError):
        mc.ERMLMC(3, scale=0.2)
    with pytest.raises(AssertionError, match="Number of leapfrog steps should be > 0"):
        mc.ERMLMC(0, 0.5)
    with pytest.raises(AssertionError, match="Leapfrog step size should be > 0"):
        mc.ERMLMC(3, 0.0)
    with pytest.raises(AssertionError, match="Leapfrog step size should be > 0"):
        mc.ERMLMC(-0.5)


def test_rmlmc_constructor_forms():
    """RMLMC.jl:40-46, each with and without a trailing tuner"""
    def f(sp):
        return sp.nLeaps, sp.leapStep, sp.nNewton
    for tail, tn in (((), None), ((TUNER,), TUNER), ((None,), None)):
        assert f(mc.RMLMC(*tail)) == (6, 0.5, 4) and mc.RMLMC(*tail).tuner is tn
        assert f(mc.RMLMC(5, *tail)) == (5, 3 / 5, 4)
        assert f(mc.RMLMC(5, 0.25, *tail)) == (5, 0.25, 4)
        assert f(mc.RMLMC(5, 3, *tail)) == (5, 3 / 5, 3)
        assert f(mc.RMLMC(0.7, *tail)) == (4, 0.7, 4)                  # floor(3 / 0.7) = 4
        assert f(mc.RMLMC(0.7, 2, *tail)) == (4, 0.7, 2)
        assert f(mc.RMLMC(7, 0.1, 2, *tail)) == (7, 0.1, 2) and mc.RMLMC(7, 0.1, 2, *tail).tuner is tn
    assert mc.RMLMC(tuner=TUNER).tuner is TUNER
    for bad in ((1.0, 2.0), (1, 2, 3), (0.5, 1, 2), (1, 0.5, 2.0), (1, 0.5, 2, 3)):
        with pytest.raises(TypeError, match="RMLMC"):
            mc.RMLMC(*bad)
    with pytest.raises(AssertionError, match="Number of leapfrog steps should be > 0"):
        mc.RMLMC(0, 0.5, 4)
    with pytest.raises(AssertionError, match="Leapfrog step size should be > 0"):
        mc.RMLMC(3, 0.0)
    with pytest.raises(AssertionError, match="Number of Newton steps should be > 0"):
        mc.RMLMC(3, 0)


def test_validation_and_t0_round_trip():
    lib = _lib.load()
    cfg = mc.RMLMC(7, 0.1, 3, TUNER).cfg()
    assert (cfg.kind, cfg.n_leaps, cfg.leap_step, cfg.t0, cfg.tuner) == (11, 7, 0.1, 3.0, 1)
    assert lib.mcmc_sampler_validate(ct.byref(cfg)) == 0
    cfg = mc.ERMLMC(7, 0.1, TUNER).cfg()
    assert (cfg.kind, cfg.n_leaps, cfg.leap_step, cfg.t0, cfg.tuner) == (10, 7, 0.1, 0.0, 1)
    assert lib.mcmc_sampler_validate(ct.byref(cfg)) == 0
    header = open(os.path.join(ROOT, "include", "mcmc_hip.h")).read()
    assert re.search(r"MCMC_ERMLMC = 10\b", header) and re.search(r"MCMC_RMLMC = 11\b", header)
    assert re.search(r"#define MCMC_ABI_VERSION 1\b", header)
    assert (_lib.SAMPLER_ERMLMC, _lib.SAMPLER_RMLMC) == (10, 11)

    def refused(make, field, value, code, text):
        c = make().cfg()
        setattr(c, field, value)
        assert lib.mcmc_sampler_validate(ct.byref(c)) == code, (field, value)
        assert text in lib.mcmc_last_error(), lib.mcmc_last_error()
    for make in (lambda: mc.ERMLMC(7, 0.1), lambda: mc.RMLMC(7, 0.1, 3)):
        refused(make, "n_leaps", 0, _lib.MCMC_E_INVALID_ARG, b"Number of leapfrog steps should be > 0")
        refused(make, "leap_step", 0.0, _lib.MCMC_E_INVALID_ARG, b"Leapfrog step size should be > 0")
        refused(make, "leap_step", float("nan"), _lib.MCMC_E_INVALID_ARG, b"Leapfrog step size should be > 0")
        refused(make, "n_leaps", (1 << 20) + 1, _lib.MCMC_E_UNSUPPORTED, b"nLeaps <= 2^20")
        c = make().cfg()
        c.tuner, c.adapt_step, c.max_step, c.target_rate = 1, 0, 10, 0.5
        assert lib.mcmc_sampler_validate(ct.byref(c)) == _lib.MCMC_E_INVALID_ARG
    make = lambda: mc.RMLMC(7, 0.1, 3)
    refused(make, "t0", 0.0, _lib.MCMC_E_INVALID_ARG, b"Number of Newton steps should be > 0")
    refused(make, "t0", -1.0, _lib.MCMC_E_INVALID_ARG, b"Number of Newton steps should be > 0")
    refused(make, "t0", float("nan"), _lib.MCMC_E_INVALID_ARG, b"Number of Newton steps should be > 0")
    refused(make, "t0", 2.5, _lib.MCMC_E_INVALID_ARG, b"t0 carries nNewton")
    refused(make, "t0", 2.0 ** 31, _lib.MCMC_E_INVALID_ARG, b"t0 carries nNewton")
    c = make().cfg()
    c.t0 = 2.0 ** 31 - 1
    assert lib.mcmc_sampler_validate(ct.byref(c)) == 0


@pytest.mark.parametrize("cls", [mc.ERMLMC, mc.RMLMC])
def test_python_refusals(cls):
    """gradient, tensor, dtensor, in that order, without a device"""
    nm = cls.__name__
    mh.python_refusals(nm, cls)
    pc.model("probit_vaso") * cls(0.5, TUNER) * mc.SerialMC(steps=10)
    from mcmchip import api
    assert nm in api.__all__ and getattr(mc, nm) is cls


def test_texts_name_the_new_samplers():
    header = open(os.path.join(ROOT, "include", "mcmc_hip.h")).read()
    hook, mod = mh.julia_texts()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "t0: RMLMC's nNewton" in header and "ERMLMC.jl:64-67" in header
    assert re.search(r"hip_sampler\(s::ERMLMC\) = hip_cfg\(10, 0\., 0\., s\.nLeaps, s\.leapStep", hook)
    assert re.search(r"hip_sampler\(s::RMLMC\) = hip_cfg\(11, 0\., 0\., s\.nLeaps, s\.leapStep", hook)
    assert re.search(r"isa\(s, ERMLMC\)", hook) and re.search(r"isa\(s, RMLMC\)", hook)
    assert re.search(r"const ERMLMC_K = 10\b", mod) and re.search(r"const RMLMC_K = 11\b", mod)
    assert "ermlmc(" in mod and "rmlmc(" in mod
    assert "### 5.12" in design and "TAG_LMC" in design and "lmc_step" in design
    assert "ERMLMC" in readme and "RMLMC" in readme and "ERMLMC" in integ and "RMLMC" in integ


@pytest.mark.parametrize("kind", ["logistic", "logistic_neg", "probit"])
@pytest.mark.parametrize("d", [1, 3, 5, 10, 16])
def test_symmetry_identity(kind, d):
    """the checker's vxC(v) = 0.5 X' diag(w o X v) X and vxC(v) v = 0.5 X' (w o (X v)^2) against the literal
    C = 0.5 (permutedims(dG, [3 2 1]) + permutedims(dG, [1 3 2]) - dG) and vxC[k, :] = v' C[:, :, k] from its own
    evalalldt slabs, at 6 points: 1e-10 relative to the largest entry"""
    n = 37
    X, Y = sc.data(n, d, 300 + d)
    tgt = mc.ProbitRegression(X, Y) if kind == "probit" else \
        mc.LogisticRegression(X, Y, link_sign=-1.0 if kind == "logistic_neg" else 1.0)
    m = mc.model(tgt, vars=np.zeros(d), gradient=True, tensor=True, dtensor=True)
    rng = np.random.default_rng(d)
    x = rng.standard_normal((d, 6)) * 0.5
    _, _, _, dGp = lr.evalalldt(m, x)
    worst = 0.0
    for c in range(6):
        v = rng.standard_normal(d)
        dG = mh.slabs(dGp, c, d)
        Cl = lc.literal_C(dG)
        vxC = lc.literal_vxC(v, Cl)
        got, gotv = lr.gram(m, x[:, c], v)
        for a, b in ((got, vxC), (gotv, vxC @ v)):
            scale = np.abs(b).max()
            dev = np.abs(a - b).max()
            worst = max(worst, dev / scale)
            assert dev <= 1e-10 * scale, (kind, d, c, dev, scale)
    print(kind, d, "worst deviation from the literal C", worst)


@pytest.mark.parametrize("d", [1, 3, 5, 10, 16])
def test_logdet_and_solve(d):
    """logdet and the solve of G +- c vxC from the packed factor against np.linalg.slogdet and np.linalg.solve
    (G = A' A + I, vxC a symmetric perturbation a tenth its size: well conditioned, 1e-10 relative); an indefinite matrix
    reports failure"""
    rng = np.random.default_rng(60 + d)
    A = rng.standard_normal((2 * d + 3, d))
    G = A.T @ A + np.eye(d)
    B = rng.standard_normal((d, d))
    vxC = 0.1 * (B + B.T)
    b = rng.standard_normal(d)
    for c in (0.25, -0.25):
        M = G + c * vxC
        ld, sol = lr.factor(G, vxC, c, b)
        sign, ref = np.linalg.slogdet(M)
        assert sign > 0
        assert abs(ld - ref) <= 1e-10 * max(1.0, abs(ref)), (d, c, ld, ref)
        rs = np.linalg.solve(M, b)
        assert np.abs(sol - rs).max() <= 1e-10 * np.abs(rs).max()
    big = 100.0 * np.abs(np.linalg.eigvalsh(G)).max() / max(np.abs(np.linalg.eigvalsh(vxC)).max(), 1e-300)
    for c in (big, -big):
        M = G + c * vxC
        if np.linalg.eigvalsh(M).min() < 0:                            # indefinite (at d = 1: negative for one sign)
            assert lr.factor(G, vxC, c, b) == (None, None), (d, c)
    assert any(np.linalg.eigvalsh(G + c * vxC).min() < 0 for c in (big, -big))


# leapStep 0.2 and seed 3: chosen on the CPU so that the transcription itself meets no failed trajectory (at 0.3 the
# tuned RMLMC run on probit_vaso grows its step until G + h vxC has a negative determinant), no draw of 0 and no accept
# test nearer a tie than the bound below
@pytest.mark.parametrize("kind", ["ermlmc", "rmlmc"])
@pytest.mark.parametrize("which,tuned,seed", [("vaso", False, 3), ("vaso", True, 3), ("logistic", False, 3),
                                              ("logistic", True, 3)])
def test_checker_against_literal_transcription(which, tuned, seed, kind):
    """20 steps of 8 chains: identical accept decisions, at least one accept, no failed trajectory and no draw of 0;
    kept samples and gradients within the project's standing 1e-10 relative bound; the nearest accept test farther from
    a tie than both 1e-6 and 10^3 times the measured deviation, so that gap cannot flip an accept"""
    m = pc.model("probit_vaso") if which == "vaso" else pc.logistic_40_10()
    tn = mc.EmpiricalMCMCTuner(0.7, adaptStep=5, maxStep=6, targetPath=2.0) if tuned else None
    sp = mc.ERMLMC(6, 0.2, tn) if kind == "ermlmc" else mc.RMLMC(6, 0.2, 4, tn)
    r = mc.SerialMC(steps=20, burnin=15)
    oc = lr.LmcChains(m, sp, 8, seed=seed)
    s, g, a = oc.run(mc.SerialMC(steps=20, burnin=0), nthreads=1) if not tuned else mh.run_all(oc, r)
    ls, lg, la, margin = lc.literal(m, sp, 8, 20, seed, 15)
    scale = np.abs(ls).max()
    gscale = np.abs(lg).max()
    dev = max(np.abs(s - ls).max() / scale, np.abs(g - lg).max() / gscale)
    print(kind, which, tuned, "max deviation", dev, "margin", margin, "acceptance", la.mean(), "adaptations",
          oc.counters.n_adapt)
    assert oc.counters.n_failed == 0 and oc.counters.n_zero == 0
    assert oc.counters.n_adapt == (3 * 8 if tuned else 0)
    assert margin > 1e-6 and margin > 1e3 * dev, (margin, dev)
    assert np.array_equal(a.astype(bool), la)
    assert la.any()
    assert dev <= 1e-10


def test_ermlmc_volume_correction():
    """exp(deltaLogDet) of one ERMLMC leapfrog on the checker against the determinant of the Jacobian of its map
    (pars, v) -> (pars', v') at d = 3 (probit_vaso, leapStep 0.5), the Jacobian by central differences of step
    delta = 1e-5 in each of the 6 inputs.

    Bound.  A central difference of a smooth map has truncation error delta^2 |f'''| / 6 and rounding error
    eps_f / delta, eps_f the absolute error of the map's outputs.  Here the outputs are O(1) and come out of a few
    hundred fp64 operations, eps_f <= 1e-13; the third derivatives of the leapfrog map at leapStep 0.5 on this model are
    O(10), so each entry of J carries at most 1e-10 * 10 / 6 + 1e-13 / 1e-5 < 2e-8.  A relative perturbation E of
    J changes det J by a factor within 1 +- 6 |J^-1| |E| to first order; the test measures cond(J), asserts it below
    1e2, and so bounds the relative error of the determinant by 6 * 1e2 * 2e-8 < 2e-5.  A misplaced or mis-signed
    logdet term changes deltaLogDet by the size of a single term, asserted to be above 1e-3 in magnitude here: fifty
    times the bound."""
    m = pc.model("probit_vaso")
    d, h, delta = 3, 0.5, 1e-5
    rng = np.random.default_rng(5)
    x0 = np.array([-0.3, 0.4, 0.2])
    G = pc.closed_G(m, x0)
    v0 = np.linalg.cholesky(np.linalg.inv(G)) @ rng.standard_normal(d)

    def F(y):
        out = lr.leap(m, "ermlmc", y[:d], y[d:], h)
        assert out is not None
        return np.concatenate([out[0], out[1]]), out[2]
    y0 = np.concatenate([x0, v0])
    _, dl = F(y0)
    J = np.empty((2 * d, 2 * d))
    for k in range(2 * d):
        e = np.zeros(2 * d)
        e[k] = delta
        J[:, k] = (F(y0 + e)[0] - F(y0 - e)[0]) / (2 * delta)
    detJ = np.linalg.det(J)
    cond = np.linalg.cond(J)
    # the four terms on their own, from the checker's Gram matrix: each is far above the bound
    vxC, _ = lr.gram(m, x0, v0)
    term, _ = lr.factor(G, vxC, 0.5 * h)
    print("det J", detJ, "exp(deltaLogDet)", np.exp(dl), "relative gap", detJ / np.exp(dl) - 1, "cond", cond,
          "deltaLogDet", dl, "first term's change of logdet", term - np.linalg.slogdet(G)[1])
    assert cond < 1e2
    assert abs(dl) > 1e-3 and abs(term - np.linalg.slogdet(G)[1]) > 1e-3
    assert abs(detJ / np.exp(dl) - 1) <= 2e-5


def test_checker_ermlmc_posterior_agrees_with_smmala():
    """the GPU test's posterior check on the checker alone, 256 chains each of ERMLMC(3, 0.5) and SMMALA(0.5) on
    logistic_40_10, 100 kept steps after 100: per coordinate the grand means within 5 standard errors of their
    difference (the errors scale with the chain count, so the bound is the GPU test's at 4 096 chains).  The same
    comparison for RMLMC(3, 0.5, 4), whose energy carries the other sign of the log-determinant, is recorded in
    DESIGN.md §10 and is not a gate."""
    C = 256
    r = mc.SerialMC(steps=200, burnin=100)
    m = pc.logistic_40_10()
    a, _, acc = lr.LmcChains(m, mc.ERMLMC(3, 0.5), C, seed=21).run(r)
    b, _, _ = lr.SmmalaChains(sc.logistic_40_10(), mc.SMMALA(0.5), C, seed=22).run(r)
    z, ma, mb, se = mh.posterior_z(a, b, C)
    print("z", z, "acceptance", acc.mean())
    assert (z < 5).all(), (ma, mb, se)
