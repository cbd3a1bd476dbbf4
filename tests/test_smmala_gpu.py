"""SMMALA and the device metric tensor (smmala.hip) against the checker (tests/manifold_oracle.c), bit for bit."""
import numpy as np
import pytest

import manifold_harness as mh
import manifold_ref as sr
import mcmchip as mc
import smmala_cases as sc
from manifold_harness import R40, _create, _raises, bits
from mcmchip import _lib

pytestmark = pytest.mark.gpu
FAM = mh.Family(sr.SmmalaChains, sc, lambda name: mc.SMMALA(sc.SHAPES[name][4]))


@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_eval_tensor(gpu, name):
    m = sc.model(name)
    x = sc.points(name)
    d, C = x.shape
    lp, g, Gp = np.empty(C), np.empty((d, C)), np.empty((d * (d + 1) // 2, C))
    _lib.check(_lib.load().mcmc_model_eval_tensor(m._handle(0), C, _lib.dptr(x), _lib.dptr(lp), _lib.dptr(g),
                                                  _lib.dptr(Gp)))
    lp_r, g_r, G_r = sr.evalallt(m, x)
    assert np.array_equal(bits(lp), bits(lp_r))
    assert np.array_equal(bits(g), bits(g_r))
    assert np.array_equal(bits(Gp), bits(G_r))
    lp0, g0 = m.evalallg(x)
    assert np.array_equal(bits(lp), bits(lp0)) and np.array_equal(bits(g), bits(g0))
    # lp and grad may be NULL; the Python wrapper mirrors the triangle
    G2 = np.empty_like(Gp)
    _lib.check(_lib.load().mcmc_model_eval_tensor(m._handle(0), C, _lib.dptr(x), None, None, _lib.dptr(G2)))
    assert np.array_equal(bits(G2), bits(Gp))
    assert np.array_equal(bits(m.evalallt(x)[2]), bits(sr.unpack(Gp, d)))


@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_parity(gpu, name):
    _, _, _, C, h = sc.SHAPES[name]
    ref = FAM.reference(name)
    t = (sc.model(name) * mc.SMMALA(h) * R40).batch(C, seed=1)
    ch = mc.run(t)
    FAM.assert_same(ch, t, ref, name)
    assert ref.a.any() and not ref.a.all(), (name, ref.a.mean())          # both accepted and rejected kept steps
    assert t.step_kernel == "smm_step"
    assert np.isnan(t.tuner_state()["step"]).all()


@pytest.mark.parametrize("spl", [1, 7])
def test_steps_per_launch(gpu, spl):
    name = "logistic_n17_d5"
    t = (sc.model(name) * mc.SMMALA(1.0) * R40).batch(70, seed=1, steps_per_launch=spl)
    FAM.assert_same(mc.run(t), t, FAM.reference(name), f"spl {spl}")


def test_two_runs_equal_one(gpu):
    name = "probit_n40_d10"
    m = sc.model(name)
    one = (m * mc.SMMALA(1.0) * mc.SerialMC(steps=40)).batch(17, seed=3)
    c1 = mc.run(one)
    two = (m * mc.SMMALA(1.0) * mc.SerialMC(steps=20)).batch(17, seed=3)
    a = mc.run(two)
    b = mc.run(two)
    assert np.array_equal(bits(np.concatenate([a._samples, b._samples])), bits(c1._samples))
    assert np.array_equal(bits(b.final_lp), bits(c1.final_lp))


def _tuned(tuner_burnin):
    name = "logistic_n17_d5"
    sp = mc.SMMALA(1.0, mc.EmpiricalMCMCTuner(adaptStep=5, targetRate=0.7))
    r = mc.SerialMC(steps=40, burnin=20) if tuner_burnin is None else mc.SerialMC(steps=40)
    oc = sr.SmmalaChains(sc.model(name), sp, 70, seed=2)
    t = (sc.model(name) * sp * r).batch(70, seed=2)
    if tuner_burnin is not None:
        oc.tuner_burnin = tuner_burnin
        _lib.check(_lib.load().mcmc_chains_set_tuner_burnin(t.handle(), tuner_burnin))
    FAM.assert_same(mc.run(t), t, FAM.ran(oc, r), "tuned")
    step = t.tuner_state()["step"]
    assert np.array_equal(bits(step), bits(oc.t_step))
    assert len(np.unique(step)) > 1 and not (step == 1.0).any()


def test_tuned_kept_range(gpu):
    _tuned(None)


def test_tuned_set_tuner_burnin(gpu):
    _tuned(20)


def test_fork_reset_set_state(gpu):
    """set_state: the reset hook keeps the stale invG / firstTerm"""
    mh.fork_reset_set_state(FAM, sc.model("logistic_n17_d5"), mc.SMMALA(1.0))


def test_group_equals_one_context(gpu):
    name = "logistic_neg_n33_d16"
    t = (sc.model(name) * mc.SMMALA(0.5) * R40).batch(100, seed=1, devices=(0, 0))
    mh.assert_outputs(mc.run(t), FAM.reference(name))


def test_refusals(gpu):
    cfg = mc.SMMALA(1.0).cfg()
    mh.gradient_refusals("SMMALA", cfg, "d <= 16", dtensor=False)
    X, Y = sc.data(20, 4, 2)
    lin = mc.model(mc.LinearRegression(X, Y), vars=np.zeros(4), gradient=True)
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, "SMMALA sampler requires model with tensor function", lambda: _create(lin, cfg))
    lin_t = mc.model(mc.LinearRegression(X, Y), vars=np.zeros(4), gradient=True, tensor=True)
    _raises(_lib.MCMC_E_UNSUPPORTED, "no tensor function", lambda: lin_t._handle(0))
    iso_t = mc.model(mc.IsoNormalDot(), init=np.ones(3), grad=True, tensor=True)
    _raises(_lib.MCMC_E_UNSUPPORTED, "no tensor function", lambda: iso_t._handle(0))
    name = "logistic_n17_d5"
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, "model has no tensor function",
            lambda: sc.model(name, False).evalallt(np.zeros(5)))
    # an init whose log-target is -Inf: the logistic term saturates (the reference's p rounds to 0)
    big = mc.model(mc.LogisticRegression(np.ones((4, 1)), np.zeros(4)), vars=np.zeros(1), gradient=True, tensor=True)
    with pytest.raises(_lib.OutOfSupportError):
        _create(big, cfg, 4, np.full((1, 4), 800.0))
    mh.seqmc_refuses((sc.model(name) * mc.SMMALA(1.0) * R40).batch(8, seed=1), "SMMALA")


def test_recovers_rwm_posterior_mean(gpu):
    """64 chains x 2 000 steps of vaso SMMALA(1.0) against RWM: means within four Monte-Carlo standard errors, the
    errors from stats.ess of both runs."""
    m = sc.model("probit_vaso")
    r = mc.SerialMC(steps=2000, burnin=200)
    a = mc.run((m * mc.SMMALA(1.0) * r).batch(64, seed=11))
    b = mc.run((m * mc.RWM(0.5) * r).batch(64, seed=12))

    from mcmchip import stats
    xa, xb = a._samples, b._samples                            # [nkept][d][C]
    ma, mb = xa.mean(axis=(0, 2)), xb.mean(axis=(0, 2))
    ea = np.asarray(stats.ess(a)).reshape(64, 3).sum(axis=0)   # [nchains, d] -> per parameter, summed over chains
    eb = np.asarray(stats.ess(b)).reshape(64, 3).sum(axis=0)
    va = xa.transpose(1, 0, 2).reshape(3, -1).var(axis=1)
    vb = xb.transpose(1, 0, 2).reshape(3, -1).var(axis=1)
    se = np.sqrt(va / ea + vb / eb)
    print("means", ma, mb, "se", se, "ess", ea, eb)
    assert (np.abs(ma - mb) < 4 * se).all(), (ma, mb, se)
