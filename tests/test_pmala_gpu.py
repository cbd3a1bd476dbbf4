"""PMALA and the device tensor derivatives (pmala.hip) against the checker (tests/manifold_oracle.c), bit for bit."""
import numpy as np
import pytest

import manifold_harness as mh
import manifold_ref as pr
import mcmchip as mc
import pmala_cases as pc
import smmala_cases as sc
from manifold_harness import R40, _create, _raises, bits
from mcmchip import _lib

pytestmark = pytest.mark.gpu
FAM = mh.Family(pr.PmalaChains, pc, lambda name: mc.PMALA(pc.SHAPES[name][4]),
                manifold=(("grad", "g"), ("G", "G"), ("invG", "invG"), ("first_term", "ft"), ("corr", "c")))


@pytest.mark.parametrize("name", list(pc.SHAPES))
def test_eval_dtensor(gpu, name):
    m = pc.model(name)
    x = pc.points(name)
    d, C = x.shape
    nr = d * (d + 1) // 2
    lp, g, Gp, dG = np.empty(C), np.empty((d, C)), np.empty((nr, C)), np.empty((d, nr, C))
    lib = _lib.load()
    _lib.check(lib.mcmc_model_eval_dtensor(m._handle(0), C, _lib.dptr(x), _lib.dptr(lp), _lib.dptr(g), _lib.dptr(Gp),
                                           _lib.dptr(dG)))
    lp_r, g_r, G_r, dG_r = pr.evalalldt(m, x)
    assert np.array_equal(bits(dG), bits(dG_r))
    assert np.array_equal(bits(lp), bits(lp_r)) and np.array_equal(bits(g), bits(g_r))
    assert np.array_equal(bits(Gp), bits(G_r))
    # lp, grad and G are mcmc_model_eval_tensor's
    lp0, g0, G0 = np.empty(C), np.empty((d, C)), np.empty((nr, C))
    _lib.check(lib.mcmc_model_eval_tensor(m._handle(0), C, _lib.dptr(x), _lib.dptr(lp0), _lib.dptr(g0), _lib.dptr(G0)))
    assert np.array_equal(bits(lp), bits(lp0)) and np.array_equal(bits(g), bits(g0))
    assert np.array_equal(bits(Gp), bits(G0))
    # lp, grad and G may be NULL; the Python wrapper mirrors the triangles
    dG2 = np.empty_like(dG)
    _lib.check(lib.mcmc_model_eval_dtensor(m._handle(0), C, _lib.dptr(x), None, None, None, _lib.dptr(dG2)))
    assert np.array_equal(bits(dG2), bits(dG))
    full = m.evalalldt(x)[3]
    for i in range(d):
        assert np.array_equal(bits(full[:, :, i]), bits(pr.unpack(dG[i], d)))


@pytest.mark.parametrize("name", list(pc.SHAPES))
def test_parity(gpu, name):
    _, _, _, C, h = pc.SHAPES[name]
    ref = FAM.reference(name)
    t = (pc.model(name) * mc.PMALA(h) * R40).batch(C, seed=1)
    ch = mc.run(t)
    FAM.assert_same(ch, t, ref, name)
    assert ref.a.any() and not ref.a.all(), (name, ref.a.mean())          # both accepted and rejected kept steps
    assert t.step_kernel == "pm_step"
    assert np.isnan(t.tuner_state()["step"]).all()


@pytest.mark.parametrize("spl", [0, 1, 7])
def test_steps_per_launch(gpu, spl):
    name = "logistic_n17_d5"
    t = (pc.model(name) * mc.PMALA(1.0) * R40).batch(70, seed=1, steps_per_launch=spl)
    FAM.assert_same(mc.run(t), t, FAM.reference(name), f"spl {spl}")


def test_tuned(gpu):
    """adaptStep 5 inside a burnin of 20: the drift step adapts four times"""
    name = "logistic_n17_d5"
    sp = mc.PMALA(1.0, mc.EmpiricalMCMCTuner(adaptStep=5, targetRate=0.7))
    r = mc.SerialMC(steps=40, burnin=20)
    oc = pr.PmalaChains(pc.model(name), sp, 70, seed=2)
    t = (pc.model(name) * sp * r).batch(70, seed=2)
    FAM.assert_same(mc.run(t), t, FAM.ran(oc, r), "tuned")
    step = t.tuner_state()["step"]
    assert np.array_equal(bits(step), bits(oc.t_step))
    assert len(np.unique(step)) > 1 and not (step == 1.0).any()


def test_fork_reset_set_state(gpu):
    """the fork copies c; set_state: the reset hook keeps the stale invG / firstTerm / c, and the next step uses them;
    reset restarts and recomputes c"""
    mh.fork_reset_set_state(FAM, pc.model("logistic_n17_d5"), mc.PMALA(1.0), stale="corr")


def test_group_equals_one_context(gpu):
    name = "logistic_neg_n33_d16"
    ref = FAM.reference(name)
    t = (pc.model(name) * mc.PMALA(0.5) * R40).batch(100, seed=1, devices=(0, 0))
    mh.assert_outputs(mc.run(t), ref)
    assert np.array_equal(bits(t.manifold_state()["corr"]), bits(ref.state["c"]))


@pytest.mark.parametrize("name", ["probit_n40_d10", "logistic_neg_n33_d16"])
def test_smmala_on_dtensor_model(gpu, name):
    """a has_gradient == 3 model serves SMMALA bit for bit"""
    _, _, _, C, h = pc.SHAPES[name]
    a = mc.run((sc.model(name) * mc.SMMALA(h) * R40).batch(C, seed=1))
    t = (pc.model(name) * mc.SMMALA(h) * R40).batch(C, seed=1)
    b = mc.run(t)
    assert t.step_kernel == "smm_step"
    assert np.array_equal(bits(a._samples), bits(b._samples))
    assert np.array_equal(bits(a._gradients), bits(b._gradients))
    assert np.array_equal(a.diagnostics["accept"], b.diagnostics["accept"])
    assert np.array_equal(bits(a.final_lp), bits(b.final_lp))


def test_refusals(gpu):
    cfg = mc.PMALA(1.0).cfg()
    # d > 16; a model without tensor derivatives, after the gradient and tensor checks
    wide = mh.gradient_refusals("PMALA", cfg, "d <= 16")
    _raises(_lib.MCMC_E_UNSUPPORTED, "d <= 16", lambda: wide.evalalldt(np.zeros(17)))
    name = "logistic_n17_d5"
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, "model has no function of tensor derivatives",
            lambda: sc.model(name).evalalldt(np.zeros(5)))
    # has_gradient == 3 on any other kind
    X, Y = sc.data(20, 4, 2)
    lin = mc.model(mc.LinearRegression(X, Y), vars=np.zeros(4), gradient=True, tensor=True, dtensor=True)
    _raises(_lib.MCMC_E_UNSUPPORTED, "no tensor function", lambda: lin._handle(0))
    # an init whose log-target is -Inf
    big = mc.model(mc.LogisticRegression(np.ones((4, 1)), np.zeros(4)), vars=np.zeros(1), gradient=True, tensor=True,
                   dtensor=True)
    with pytest.raises(_lib.OutOfSupportError):
        _create(big, cfg, 4, np.full((1, 4), 800.0))
    mh.seqmc_refuses((pc.model(name) * mc.PMALA(1.0) * R40).batch(8, seed=1), "PMALA")


def test_posterior_agrees_with_smmala(gpu):
    """4 096 chains of PMALA(0.5) and of SMMALA(0.5) on logistic_40_10, 200 kept steps after 200: per coordinate the
    grand means differ by less than 5 standard errors of their difference, the errors from the between-chain variance
    of the chain means (independent chains: a z-test, false-failure rate below 1e-5 over ten coordinates)."""
    C = 4096
    r = mc.SerialMC(steps=400, burnin=200)
    m = pc.logistic_40_10()
    a = mc.run((m * mc.PMALA(0.5) * r).batch(C, seed=21))
    b = mc.run((m * mc.SMMALA(0.5) * r).batch(C, seed=22))
    z, ma, mb, se = mh.posterior_z(a._samples, b._samples, C)
    print("means", ma, mb, "se", se, "z", z, "acceptance", a.diagnostics["accept"].mean(),
          b.diagnostics["accept"].mean())
    assert (z < 5).all(), (ma, mb, se)
