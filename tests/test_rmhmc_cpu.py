"""RMHMC without a GPU: the constructor forms, the C ABI's validation and the Python refusals, the checker's two fused
tensor terms against their literal forms built from its own dG slabs, the Cholesky solve, the checker's sampler against
a literal numpy transcription of RMHMC.jl:53-183, the generalised leapfrog's second order, and the checker's posterior
means against SMMALA's at the leapStep and nNewton the GPU test uses."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import manifold_harness as mh
import manifold_ref as rr
import mcmchip as mc
import pmala_cases as pc
import smmala_cases as sc
from mcmchip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNER = mc.EmpiricalMCMCTuner(0.8)
sr = rr          # the tensor is the same checker's


def test_constructor_forms():
    """RMHMC.jl:42-48, each with and without a trailing tuner"""
    def f(sp):
        return sp.nLeaps, sp.leapStep, sp.nNewton
    for tail, tn in (((), None), ((TUNER,), TUNER), ((None,), None)):
        assert f(mc.RMHMC(*tail)) == (6, 0.5, 4) and mc.RMHMC(*tail).tuner is tn
        assert f(mc.RMHMC(5, *tail)) == (5, 3 / 5, 4)
        assert f(mc.RMHMC(5, 0.25, *tail)) == (5, 0.25, 4)
        assert f(mc.RMHMC(5, 3, *tail)) == (5, 3 / 5, 3)
        assert f(mc.RMHMC(0.7, *tail)) == (4, 0.7, 4)                  # floor(3 / 0.7) = 4
        assert f(mc.RMHMC(0.7, 2, *tail)) == (4, 0.7, 2)
        assert f(mc.RMHMC(7, 0.1, 2, *tail)) == (7, 0.1, 2) and mc.RMHMC(7, 0.1, 2, *tail).tuner is tn
    assert mc.RMHMC(tuner=TUNER).tuner is TUNER
    for bad in ((1.0, 2.0), (1, 2, 3), (0.5, 1, 2), (1, 0.5, 2.0), (1, 0.5, 2, 3)):
        with pytest.raises(TypeError):
            mc.RMHMC(*bad)
    with pytest.raises(AssertionError, match="Number of leapfrog steps should be > 0"):
        mc.RMHMC(0, 0.5, 4)
    with pytest.raises(AssertionError, match="Number of leapfrog steps should be > 0"):
        mc.RMHMC(4.0)                                                  # floor(3 / 4.0) = 0
    with pytest.raises(AssertionError, match="Leapfrog step size should be > 0"):
        mc.RMHMC(3, 0.0)
    with pytest.raises(AssertionError, match="Leapfrog step size should be > 0"):
        mc.RMHMC(-0.5)
    with pytest.raises(AssertionError, match="Number of Newton steps should be > 0"):
        mc.RMHMC(3, 0)


def test_validation_and_t0_round_trip():
    lib = _lib.load()
    cfg = mc.RMHMC(7, 0.1, 3, TUNER).cfg()
    assert (cfg.kind, cfg.n_leaps, cfg.leap_step, cfg.t0, cfg.tuner) == (9, 7, 0.1, 3.0, 1)
    assert lib.mcmc_sampler_validate(ct.byref(cfg)) == 0
    header = open(os.path.join(ROOT, "include", "mcmc_hip.h")).read()
    assert re.search(r"MCMC_RMHMC = 9\b", header) and _lib.SAMPLER_RMHMC == 9

    def refused(field, value, code, text):
        c = mc.RMHMC(7, 0.1, 3).cfg()
        setattr(c, field, value)
        assert lib.mcmc_sampler_validate(ct.byref(c)) == code, (field, value)
        assert text in lib.mcmc_last_error(), lib.mcmc_last_error()
    refused("n_leaps", 0, _lib.MCMC_E_INVALID_ARG, b"Number of leapfrog steps should be > 0")
    refused("leap_step", 0.0, _lib.MCMC_E_INVALID_ARG, b"Leapfrog step size should be > 0")
    refused("t0", 0.0, _lib.MCMC_E_INVALID_ARG, b"Number of Newton steps should be > 0")
    refused("t0", -1.0, _lib.MCMC_E_INVALID_ARG, b"Number of Newton steps should be > 0")
    refused("t0", 2.5, _lib.MCMC_E_INVALID_ARG, b"t0 carries nNewton")
    refused("t0", 2.0 ** 31, _lib.MCMC_E_INVALID_ARG, b"t0 carries nNewton")
    refused("t0", float("nan"), _lib.MCMC_E_INVALID_ARG, b"Number of Newton steps should be > 0")
    refused("n_leaps", (1 << 20) + 1, _lib.MCMC_E_UNSUPPORTED, b"nLeaps <= 2^20")
    c = mc.RMHMC(7, 0.1, 3).cfg()
    c.t0 = 2.0 ** 31 - 1
    assert lib.mcmc_sampler_validate(ct.byref(c)) == 0
    c = mc.RMHMC(7, 0.1, 3).cfg()
    c.tuner, c.adapt_step, c.max_step, c.target_rate = 1, 0, 10, 0.5
    assert lib.mcmc_sampler_validate(ct.byref(c)) == _lib.MCMC_E_INVALID_ARG


def test_python_refusals():
    mh.python_refusals("RMHMC", mc.RMHMC)
    pc.model("probit_vaso") * mc.RMHMC(0.5, TUNER) * mc.SerialMC(steps=10)                 # the example's line spins without a device


def test_texts_name_the_new_limits():
    header = open(os.path.join(ROOT, "include", "mcmc_hip.h")).read()
    hook, mod = mh.julia_texts()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "t0: RMHMC's nNewton" in header and "2^31 - 1" in header
    assert re.search(r"hip_sampler\(s::RMHMC\) = hip_cfg\(9, 0\., 0\., s\.nLeaps, s\.leapStep", hook)
    assert "float64(s.nNewton)" in hook and re.search(r"isa\(s, RMHMC\)", hook)
    assert re.search(r"const RMHMC_K = 9\b", mod) and "rmhmc(" in mod
    assert "### 5.11" in design and "TAG_RMHMC" in design and "rm_step" in design
    assert "RMHMC" in readme and "RMHMC(0.5, EmpMCTuner(0.8" in integ


@pytest.mark.parametrize("kind", ["logistic", "probit"])
@pytest.mark.parametrize("d", [1, 3, 5, 10, 16])
def test_fused_terms_against_literal(kind, d):
    """the checker's X' (w o qf) and 0.5 X' (w o t^2) against trace(invG dG_r) and 0.5 p' invG dG_r invG p from its
    own evalalldt slabs and inverse, at 6 points: 1e-10 relative to the largest term"""
    n = 37
    X, Y = sc.data(n, d, 300 + d)
    tgt = mc.ProbitRegression(X, Y) if kind == "probit" else mc.LogisticRegression(X, Y, link_sign=-1.0 if d == 5 else 1.0)
    m = mc.model(tgt, vars=np.zeros(d), gradient=True, tensor=True, dtensor=True)
    rng = np.random.default_rng(d)
    x = rng.standard_normal((d, 6)) * 0.5
    _, _, Gp, dGp = rr.evalalldt(m, x)
    iGp = rr.inverse(Gp, d)
    invG = rr.unpack(iGp, d)
    worst = 0.0
    for c in range(6):
        p = rng.standard_normal(d) * 3.0
        iG = invG[:, :, c]
        v = iG @ p
        u, u2 = rr.terms(m, x[:, c], iGp[:, c], v)
        dG = mh.slabs(dGp, c, d)
        tr = np.array([np.trace(iG @ dG[:, :, r]) for r in range(d)])
        mt = np.array([0.5 * (p @ (iG @ dG[:, :, r]) @ (iG @ p)) for r in range(d)])
        for got, lit in ((u, tr), (0.5 * u2, mt)):
            scale = np.abs(lit).max()
            dev = np.abs(got - lit).max()
            worst = max(worst, dev / scale)
            assert dev <= 1e-10 * scale, (kind, d, c, dev, scale)
    print(kind, d, "worst fused-term deviation", worst)


@pytest.mark.parametrize("d", [1, 3, 5, 10, 16])
def test_solve(d):
    """G \\ b by the factor's substitutions against np.linalg.solve: G = X' X + I is well conditioned, 1e-10 relative"""
    rng = np.random.default_rng(40 + d)
    A = rng.standard_normal((2 * d + 3, d))
    G = A.T @ A + np.eye(d)
    b = rng.standard_normal(d)
    Gp = np.array([G[r, c] for r in range(d) for c in range(r + 1)])
    got = rr.solve(Gp, b, d)
    ref = np.linalg.solve(G, b)
    assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max()
    Gp[0] = -1.0
    assert rr.solve(Gp, b, d) is None                                  # a failed pivot


def _literal(m, sp, C, steps, seed, burnin):
    """RMHMC.jl:53-183 transcribed with numpy (np.linalg.inv / cholesky / solve, libm / scipy), driven by the build's
    draws; also the smallest margin |ratio - log u| (|ratio| where no uniform is drawn) of the accept tests"""
    d = m.size
    tn = sp.tuner

    def evalallg(x):
        lp, g, _ = sr.evalallt(m, x.reshape(d, 1))
        return lp[0], g[:, 0]
    samples, grads, accs = np.empty((steps, d, C)), np.empty((steps, d, C)), np.zeros((steps, C), dtype=bool)
    margin = np.inf
    invGxdG = np.empty((d, d, d))
    traceInvGxdG = np.empty(d)
    momentumTerm = np.empty(d)
    for c in range(C):
        pars = m.init.copy()
        logTarget, grad = evalallg(pars)
        t_nLeaps, t_leapStep, accepted, proposed = sp.nLeaps, sp.leapStep, 0, 0
        for i in range(1, steps + 1):
            if tn is not None:
                proposed += 1
                nLeaps, leapStep = t_nLeaps, t_leapStep
            else:
                nLeaps, leapStep = sp.nLeaps, sp.leapStep
            z, u_acc, u_leaps, nz = rr.draws(seed, c, i, d, "rmhmc")
            proposedPars = pars.copy()
            G = pc.closed_G(m, proposedPars)
            invG = np.linalg.inv(G)
            cholG = np.linalg.cholesky(G).T
            momentum = cholG.T @ z
            H = -logTarget + 0.5 * (np.log(2) + d * np.log(np.pi) + 2 * np.sum(np.log(np.diag(cholG)))) \
                + (momentum @ (invG @ momentum)) / 2
            dG = pc.closed_dG(m, proposedPars)
            for j in range(d):
                invGxdG[:, :, j] = invG @ dG[:, :, j]
                traceInvGxdG[j] = np.trace(invGxdG[:, :, j])
            timeStep = 1.0 if nz > 0.5 else -1.0
            nRandomLeaps = int(np.ceil(u_leaps * nLeaps))
            assert nRandomLeaps > 0
            for j in range(nRandomLeaps):
                _, leapGrad = evalallg(proposedPars)
                leapMomentum = momentum.copy()
                for k in range(sp.nNewton):
                    invGMomentum01 = invG @ leapMomentum
                    for r in range(d):
                        momentumTerm[r] = 0.5 * (leapMomentum @ invGxdG[:, :, r] @ invGMomentum01)
                    leapMomentum = momentum + timeStep * (leapStep / 2) * (leapGrad - 0.5 * traceInvGxdG + momentumTerm)
                momentum = leapMomentum.copy()
                invGMomentum02 = invG @ momentum
                leapPars = proposedPars.copy()
                for k in range(sp.nNewton):
                    G = pc.closed_G(m, leapPars)
                    invGMomentum01 = np.linalg.solve(G, momentum)
                    leapPars = proposedPars + (timeStep * (leapStep / 2)) * (invGMomentum01 + invGMomentum02)
                proposedPars = leapPars.copy()
                G = pc.closed_G(m, proposedPars)
                invG = np.linalg.inv(G)
                dG = pc.closed_dG(m, proposedPars)
                for k in range(d):
                    invGxdG[:, :, k] = invG @ dG[:, :, k]
                    traceInvGxdG[k] = np.trace(invGxdG[:, :, k])
                invGMomentum01 = invG @ momentum
                for k in range(d):
                    momentumTerm[k] = 0.5 * (momentum @ invGxdG[:, :, k] @ invGMomentum01)
                _, proposedGrad = evalallg(proposedPars)
                momentum = momentum + timeStep * (leapStep / 2) * (proposedGrad - 0.5 * traceInvGxdG + momentumTerm)
            proposedLogTarget, _ = evalallg(proposedPars)
            proposedH = -proposedLogTarget \
                + 0.5 * (np.log(2) + d * np.log(np.pi) + 2 * np.sum(np.log(np.diag(np.linalg.cholesky(G).T)))) \
                + (momentum @ (invG @ momentum)) / 2
            ratio = H - proposedH
            margin = min(margin, abs(ratio) if ratio > 0 else abs(ratio - np.log(u_acc)))
            if ratio > 0 or ratio > np.log(u_acc):
                pars, logTarget, grad = proposedPars.copy(), proposedLogTarget, proposedGrad.copy()
                accs[i - 1, c] = True
                if tn is not None:
                    accepted += 1
            samples[i - 1, :, c], grads[i - 1, :, c] = pars, grad
            if tn is not None and i <= burnin and i % tn.adaptStep == 0:    # adapt!(tune, tuner), HMC.jl:165-169
                rate = accepted / proposed
                t_leapStep *= 1 / (1 + np.exp(-11 * (rate - tn.targetRate))) + 0.5
                t_nLeaps = min(tn.maxStep, int(np.ceil(tn.targetPath / t_leapStep)))
                accepted, proposed = 0, 0
    return samples, grads, accs, margin


@pytest.mark.parametrize("which,tuned,seed", [("vaso", False, 3), ("vaso", True, 3), ("logistic", False, 3),
                                              ("logistic", True, 3)])
def test_checker_against_literal_transcription(which, tuned, seed):
    """20 steps of 8 chains: identical accept decisions; kept samples and gradients within the project's standing 1e-10
    relative bound; the nearest accept test farther from a tie than 1e-6, four orders above the measured deviation,
    so that gap cannot flip an accept"""
    m = pc.model("probit_vaso") if which == "vaso" else pc.logistic_40_10()
    tn = mc.EmpiricalMCMCTuner(0.7, adaptStep=5, maxStep=6, targetPath=2.0) if tuned else None
    sp = mc.RMHMC(6, 0.5, 4, tn)                                      # the reference's defaults (RMHMC.jl:42)
    r = mc.SerialMC(steps=20, burnin=15)
    oc = rr.RmhmcChains(m, sp, 8, seed=seed)
    s, g, a = oc.run(mc.SerialMC(steps=20, burnin=0), nthreads=1) if not tuned else mh.run_all(oc, r)
    ls, lg, la, margin = _literal(m, sp, 8, 20, seed, 15)
    scale = np.abs(ls).max()
    gscale = np.abs(lg).max()
    dev = max(np.abs(s - ls).max() / scale, np.abs(g - lg).max() / gscale)
    print(which, tuned, "max deviation", dev, "margin", margin, "acceptance", la.mean(), "adaptations",
          oc.counters.n_adapt)
    assert oc.counters.n_failed == 0 and oc.counters.n_zero == 0
    assert oc.counters.n_adapt == (3 * 8 if tuned else 0)
    assert margin > 1e-6 and margin > 1e3 * dev, (margin, dev)
    assert np.array_equal(a.astype(bool), la)
    assert la.any()
    assert dev <= 1e-10


def test_generalised_leapfrog_is_second_order():
    """on the checker, with nNewton = 30 (both fixed points converged to rounding), the energy error after a path of
    length 1.6 falls by about 4 each time leapStep halves: a ratio in [3, 5] over three halvings from 0.4"""
    m = pc.logistic_40_10()
    rng = np.random.default_rng(11)
    x = rng.standard_normal(10) * 0.2
    G = pc.closed_G(m, x)
    mom = np.linalg.cholesky(G) @ rng.standard_normal(10)
    errs = [abs(rr.energy_error(m, x, mom, 0.4 / 2 ** k, 4 * 2 ** k, 30)) for k in range(4)]
    ratios = [errs[k] / errs[k + 1] for k in range(3)]
    print("energy errors", errs, "ratios", ratios)
    assert all(np.isfinite(errs)) and errs[-1] > 1e-9               # far above rounding
    assert all(3.0 <= q <= 5.0 for q in ratios), ratios


def test_checker_posterior_agrees_with_smmala():
    """the GPU test's posterior check on the checker alone, 256 chains each of RMHMC(3, 0.5, 4) and SMMALA(0.5) on
    logistic_40_10, 100 kept steps after 100: per coordinate the grand means within 5 standard errors of their
    difference (the errors scale with the chain count, so the bound is the GPU test's at 4 096 chains)"""
    C = 256
    r = mc.SerialMC(steps=200, burnin=100)
    m = pc.logistic_40_10()
    a, _, acc = rr.RmhmcChains(m, mc.RMHMC(3, 0.5, 4), C, seed=21).run(r)
    b, _, _ = sr.SmmalaChains(sc.logistic_40_10(), mc.SMMALA(0.5), C, seed=22).run(r)
    z, ma, mb, se = mh.posterior_z(a, b, C)
    print("z", z, "acceptance", acc.mean())
    assert (z < 5).all(), (ma, mb, se)
