"""PMALA and the tensor's derivatives without a GPU: the C ABI's validation and the Python refusals, the checker's dG
against finite differences of its own G and against the probit example's deriv_tensor, the fused drift correction
against the literal sum over slabs, and the checker's sampler against a literal numpy transcription of PMALA.jl:70-141."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import manifold_harness as mh
import manifold_ref as pr
import mcmchip as mc
import pmala_cases as pc
import smmala_cases as sc
from mcmchip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sr = pr          # the tensor is the same checker's


def test_validation_and_symbols():
    lib = _lib.load()
    cfg = mc.PMALA(1.0).cfg()
    assert cfg.kind == 8 and lib.mcmc_sampler_validate(ct.byref(cfg)) == 0
    cfg.drift_step = 0.0
    assert lib.mcmc_sampler_validate(ct.byref(cfg)) == _lib.MCMC_E_INVALID_ARG
    assert lib.mcmc_last_error() == b"PMALA drift step should be > 0"
    cfg = mc.PMALA(1.0).cfg()
    cfg.tuner, cfg.adapt_step, cfg.max_step, cfg.target_rate = 1, 0, 10, 0.5
    assert lib.mcmc_sampler_validate(ct.byref(cfg)) == _lib.MCMC_E_INVALID_ARG
    header = open(os.path.join(ROOT, "include", "mcmc_hip.h")).read()
    assert re.search(r"MCMC_PMALA = 8\b", header) and _lib.SAMPLER_PMALA == 8
    for sym in ("mcmc_model_eval_dtensor", "mcmc_chains_manifold_state"):
        assert sym in header and sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym)
    # the model descriptor: 3 = gradient, tensor and tensor derivatives
    assert pc.model("probit_vaso")._desc().has_gradient == 3
    assert sc.model("probit_vaso")._desc().has_gradient == 2
    assert sc.model("probit_vaso", False)._desc().has_gradient == 1
    assert mc.model(sc.model("probit_vaso").target, vars=np.zeros(3))._desc().has_gradient == 0


def test_python_refusals():
    with pytest.raises(AssertionError, match="PMALA drift step should be > 0"):
        mc.PMALA(0.0)
    assert mc.PMALA().driftStep == 1.0 and mc.PMALA().tuner is None
    assert mc.PMALA(scale=0.3).driftStep == 0.3
    tuned = mc.PMALA(mc.EmpiricalMCMCTuner(0.6))                    # the intended PMALA(1.0, tuner), PMALA.jl:36
    assert tuned.driftStep == 1.0 and tuned.cfg().tuner == 1
    assert mc.PMALA(0.5, mc.EmpiricalMCMCTuner(0.6)).cfg().drift_step == 0.5
    t = sc.model("probit_vaso").target
    with pytest.raises(AssertionError, match="needs its tensor function"):
        mc.model(t, vars=np.zeros(3), gradient=True, dtensor=True)
    r = mc.SerialMC(steps=10)
    mh.python_refusals("PMALA", lambda: mc.PMALA(1.0))
    pc.model("probit_vaso") * mc.PMALA(1.0) * r                     # spins without a device
    pc.model("probit_vaso") * mc.SMMALA(1.0) * r                    # a dtensor model serves SMMALA too


@pytest.mark.parametrize("name", list(pc.SHAPES))
def test_checker_dG_finite_differences(name):
    """every slab against the central difference of the checker's own G, delta = 1e-5: truncation O(delta^2), rounding
    O(2^-53 / delta) ~ 1e-11 relative, the bound 1e-6 max|dG|; a wrong derivative formula shows at order 1"""
    m = pc.model(name)
    x = pc.points(name)
    d, C = x.shape
    _, _, _, dG = pr.evalalldt(m, x)
    delta = 1e-5
    worst = 0.0
    for i in range(d):
        e = np.zeros((d, 1))
        e[i] = delta
        Gp = sr.evalallt(m, x + e)[2]
        Gm = sr.evalallt(m, x - e)[2]
        fd = (Gp - Gm) / (2 * delta)
        for c in range(C):
            scale = np.abs(dG[:, :, c]).max()
            err = np.abs(dG[i, :, c] - fd[:, c]).max()
            worst = max(worst, err / scale)
            assert err <= 1e-6 * scale, (name, i, c, err, scale)
    print(name, "worst finite-difference deviation / max|dG|", worst)


@pytest.mark.parametrize("name", ["probit_vaso", "probit_n40_d10"])
def test_checker_dG_probit_literal(name):
    """against deriv_tensor transcribed with scipy (examples/probit_regression.jl:52-68): 1e-10 relative"""
    m = pc.model(name)
    x = pc.points(name)
    d, C = x.shape
    _, _, _, dGp = pr.evalalldt(m, x)
    for c in range(C):
        ref = pc.closed_dG(m, x[:, c])
        got = mh.slabs(dGp, c, d)
        assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), (name, c)


@pytest.mark.parametrize("name", list(pc.SHAPES))
def test_fused_correction_against_literal(name):
    """c = invG X' (w o qf) against sum_i (invG dG_i) invG[:, i] from the checker's own dG and invG: 1e-10 relative"""
    m = pc.model(name)
    x = pc.points(name)
    d, C = x.shape
    _, _, Gp, dGp = pr.evalalldt(m, x)
    iGp = pr.inverse(Gp, d)
    fused = pr.corr(m, x, iGp)
    invG = pr.unpack(iGp, d)
    worst = 0.0
    for c in range(C):
        iG = invG[:, :, c]
        lit = np.zeros(d)
        for i in range(d):
            dGi = pr.unpack(dGp[i, :, c:c + 1], d)[:, :, 0]
            lit += (iG @ dGi) @ iG[:, i]
        scale = np.abs(lit).max()
        dev = np.abs(fused[:, c] - lit).max()
        worst = max(worst, dev / scale)
        assert dev <= 1e-10 * scale, (name, c, dev, scale)
    print(name, "worst fused-correction deviation", worst)


def _literal(m, h, C, steps, seed):
    """PMALA.jl:70-141 transcribed with numpy (np.linalg.inv / cholesky, libm / scipy), driven by the build's draws;
    also the smallest margin |ratio - log u| (|ratio| where no uniform is drawn) of the accept tests"""
    d = m.size

    def evalalldt(x):
        lp, g, _ = sr.evalallt(m, x.reshape(d, 1))
        return lp[0], g[:, 0], pc.closed_G(m, x), pc.closed_dG(m, x)

    def second(invG, dG):
        invGxdG = np.empty((d, d, d))
        secondTerm = np.empty((d, d))
        for i in range(d):
            invGxdG[:, :, i] = invG @ dG[:, :, i]
            secondTerm[:, i] = invGxdG[:, :, i] @ invG[:, i]
        return secondTerm
    samples, grads, accs = np.empty((steps, d, C)), np.empty((steps, d, C)), np.zeros((steps, C), dtype=bool)
    margin = np.inf
    for c in range(C):
        pars = m.init.copy()
        logTarget, grad, G, dG = evalalldt(pars)
        invG = np.linalg.inv(G)
        firstTerm = invG @ grad
        secondTerm = second(invG, dG)
        for i in range(1, steps + 1):
            z, u = pr.draws(seed, c, i, d)
            parsMean = pars + (h / 2) * (firstTerm - secondTerm.sum(axis=1))
            U = np.linalg.cholesky(h * invG).T
            prop = parsMean + U.T @ z
            pLT, pgrad, pG, dG = evalalldt(prop)
            e = parsMean - prop
            pNewOld = -np.sum(np.log(np.diag(U))) - 0.5 * e @ (G / h) @ e
            pinvG = np.linalg.inv(pG)
            pft = pinvG @ pgrad
            pst = second(pinvG, dG)
            pm2 = prop + (h / 2) * (pft - pst.sum(axis=1))
            e2 = pm2 - pars
            pOldNew = (-np.sum(np.log(np.diag(np.linalg.cholesky(h * np.eye(d) @ pinvG).T)))
                       - 0.5 * e2 @ (pG / h) @ e2)
            ratio = pLT + pOldNew - logTarget - pNewOld
            margin = min(margin, abs(ratio) if ratio > 0 else abs(ratio - np.log(u)))
            if ratio > 0 or ratio > np.log(u):
                pars, logTarget, grad, G, invG = prop, pLT, pgrad, pG, pinvG
                firstTerm, secondTerm = pft, pst
                accs[i - 1, c] = True
            samples[i - 1, :, c], grads[i - 1, :, c] = pars, grad
    return samples, grads, accs, margin


@pytest.mark.parametrize("which,h,seed", [("vaso", 1.0, 3), ("logistic", 0.5, 3)])
def test_checker_against_literal_transcription(which, h, seed):
    """20 steps of 8 chains: identical accept decisions, no accept test nearer than 1e-8 to a tie; kept samples and
    gradients within the project's standing 1e-10 relative bound"""
    m = pc.model("probit_vaso") if which == "vaso" else pc.logistic_40_10()
    r = mc.SerialMC(steps=20)
    oc = pr.PmalaChains(m, mc.PMALA(h), 8, seed=seed)
    s, g, a = oc.run(r, nthreads=1)
    ls, lg, la, margin = _literal(m, h, 8, 20, seed)
    scale = np.abs(ls).max()
    gscale = np.abs(lg).max()
    print("max deviation", np.abs(s - ls).max() / scale, np.abs(g - lg).max() / gscale, "margin", margin,
          "acceptance", la.mean())
    assert margin > 1e-8, margin
    assert np.array_equal(a.astype(bool), la)
    assert la.any() and not la.all()
    assert np.abs(s - ls).max() <= 1e-10 * scale
    assert np.abs(g - lg).max() <= 1e-10 * gscale


def test_julia_hook_text():
    hook, mod = mh.julia_texts()
    assert re.search(r"hip_sampler\(s::PMALA\) = hip_cfg\(8, 0\., s\.driftStep", hook)
    assert re.search(r"isa\(s, PMALA\)", hook) and re.search(r"const PMALA_K = 8\b", mod)
    assert re.search(r"hasdtensor", hook)
