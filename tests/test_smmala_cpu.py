"""SMMALA and the metric tensor without a GPU: the C ABI's validation and refusals, the checker's tensor against a
closed form, and the checker's sampler against a literal numpy transcription of SMMALA.jl:62-122."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

import manifold_harness as mh
import manifold_ref as sr
import mcmchip as mc
import smmala_cases as sc
from mcmchip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_validation_and_symbols():
    lib = _lib.load()
    cfg = mc.SMMALA(1.0).cfg()
    assert cfg.kind == 7 and lib.mcmc_sampler_validate(ct.byref(cfg)) == 0
    cfg.drift_step = 0.0
    assert lib.mcmc_sampler_validate(ct.byref(cfg)) == _lib.MCMC_E_INVALID_ARG
    assert lib.mcmc_last_error() == b"SMMALA drift step should be > 0"
    cfg = mc.SMMALA(1.0).cfg()
    cfg.tuner, cfg.adapt_step, cfg.max_step, cfg.target_rate = 1, 0, 10, 0.5
    assert lib.mcmc_sampler_validate(ct.byref(cfg)) == _lib.MCMC_E_INVALID_ARG
    header = open(os.path.join(ROOT, "include", "mcmc_hip.h")).read()
    assert re.search(r"MCMC_SMMALA = 7\b", header)
    assert "mcmc_model_eval_tensor" in header and "mcmc_model_eval_tensor" in _lib.EXPORTED_SYMBOLS
    assert hasattr(lib, "mcmc_model_eval_tensor")
    # the ABI structs keep their sizes: the tensor rides has_gradient == 2
    assert ct.sizeof(_lib.ModelDesc) == 4 + 4 + 8 + 8 + 8 + 5 * 8 + 8 + 8 + 8 + 8
    assert ct.sizeof(_lib.SamplerCfg) == 4 + 4 + 8 + 8 + 8 + 8 + 5 * 8 + 4 + 4 + 8 + 8 + 8 + 8 + 8
    assert sc.model("probit_vaso")._desc().has_gradient == 2
    assert sc.model("probit_vaso", False)._desc().has_gradient == 1


def test_python_refusals():
    with pytest.raises(AssertionError, match="SMMALA drift step should be > 0"):
        mc.SMMALA(0.0)
    assert mc.SMMALA(scale=0.3).driftStep == 0.3
    tuned = mc.SMMALA(mc.EmpiricalMCMCTuner(0.6))
    assert tuned.driftStep == 1.0 and tuned.cfg().tuner == 1
    mh.python_refusals("SMMALA", lambda: mc.SMMALA(1.0), dtensor=False)
    sc.model("probit_vaso") * mc.SMMALA(1.0) * mc.SerialMC(steps=10)      # spins without a device


def _closed_form(m, x):
    t = m.target
    eta = t.X @ x
    if t.kind == _lib.MODEL_PROBIT:
        from math import erfc
        lc = np.array([np.log(0.5 * erfc(-e / np.sqrt(2.0))) for e in eta])
        lcm = np.array([np.log(0.5 * erfc(e / np.sqrt(2.0))) for e in eta])
        v = np.exp(-eta ** 2 - lc - lcm - np.log(2 * np.pi))
    else:
        p = 1.0 / (1.0 + np.exp(-eta))
        v = p * (1.0 - p)
    return t.X.T @ (v[:, None] * t.X) + np.eye(m.size) / t.prior_sigma ** 2


@pytest.mark.parametrize("which", ["vaso", "logistic"])
def test_checker_tensor_closed_form(which):
    m = sc.model("probit_vaso") if which == "vaso" else sc.logistic_40_10()
    d = m.size
    x = np.random.default_rng(4).standard_normal((d, 6)) * 0.5
    lp, g, Gp = sr.evalallt(m, x)
    G = sr.unpack(Gp, d)
    for c in range(6):
        ref = _closed_form(m, x[:, c])
        rel = np.abs(G[:, :, c] - ref) / np.abs(ref)
        assert rel.max() <= 1e-12, (c, rel.max())


def _literal(m, h, C, steps, seed):
    """SMMALA.jl:62-122 transcribed with numpy (np.linalg.inv / cholesky, libm), driven by the build's draws"""
    d = m.size

    def evalallt(x):
        lp, g, Gp = sr.evalallt(m, x.reshape(d, 1))
        return lp[0], g[:, 0], _closed_form(m, x)
    samples, grads, accs = np.empty((steps, d, C)), np.empty((steps, d, C)), np.zeros((steps, C), dtype=bool)
    conds = []
    for c in range(C):
        pars = m.init.copy()
        logTarget, grad, G = evalallt(pars)
        invG = np.linalg.inv(G)
        firstTerm = invG @ grad
        for i in range(1, steps + 1):
            z, u = sr.draws(seed, c, i, d)
            parsMean = pars + (h / 2) * firstTerm
            U = np.linalg.cholesky(h * invG).T
            prop = parsMean + U.T @ z
            pLT, pgrad, pG = evalallt(prop)
            conds.append(np.linalg.cond(pG))
            e = parsMean - prop
            pNewOld = -np.sum(np.log(np.diag(U))) - 0.5 * e @ (G / h) @ e
            pinvG = np.linalg.inv(pG)
            pft = pinvG @ pgrad
            pm2 = prop + (h / 2) * pft
            e2 = pm2 - pars
            pOldNew = -np.sum(np.log(np.diag(np.linalg.cholesky(h * pinvG).T))) - 0.5 * e2 @ (pG / h) @ e2
            ratio = pLT + pOldNew - logTarget - pNewOld
            if ratio > 0 or ratio > np.log(u):
                pars, logTarget, grad, G, invG, firstTerm = prop, pLT, pgrad, pG, pinvG, pft
                accs[i - 1, c] = True
            samples[i - 1, :, c], grads[i - 1, :, c] = pars, grad
    return samples, grads, accs, max(conds)


@pytest.mark.parametrize("which,h", [("vaso", 1.0), ("logistic", 0.5)])
def test_checker_against_literal_transcription(which, h):
    """20 steps of 8 chains: identical accept decisions; kept samples and gradients within the project's standing
    1e-10 relative bound (tests/test_literal_reference.py)."""
    m = sc.model("probit_vaso") if which == "vaso" else sc.logistic_40_10()
    r = mc.SerialMC(steps=20)
    oc = sr.SmmalaChains(m, mc.SMMALA(h), 8, seed=3)
    s, g, a = oc.run(r, nthreads=1)
    ls, lg, la, cond = _literal(m, h, 8, 20, 3)
    scale = np.abs(ls).max()
    gscale = np.abs(lg).max()
    print("max deviation", np.abs(s - ls).max() / scale, np.abs(g - lg).max() / gscale, "cond(G)", cond,
          "acceptance", la.mean())
    assert np.array_equal(a.astype(bool), la)
    assert la.any() and not la.all()
    assert np.abs(s - ls).max() <= 1e-10 * scale
    assert np.abs(g - lg).max() <= 1e-10 * gscale


def test_julia_hook_text():
    hook, mod = mh.julia_texts()
    assert re.search(r"hip_sampler\(s::SMMALA\) = hip_cfg\(7, 0\., s\.driftStep", hook)
    assert re.search(r"isa\(s, SMMALA\)", hook) and re.search(r"const SMMALA_K = 7\b", mod)
