"""SMMALA and the device metric tensor (smmala.hip) against the checker (tests/smmala_oracle.c), bit for bit."""
import ctypes as ct
import functools

import numpy as np
import pytest

import mcmchip as mc
import smmala_cases as sc
import smmala_ref as sr
from mcmchip import _lib

pytestmark = pytest.mark.gpu
R40 = mc.SerialMC(steps=40, burnin=10, thinning=3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the checker's R40 run of a shape, computed once and shared: (chains, samples, grads, accept)"""
    _, _, _, C, h = sc.SHAPES[name]
    oc = sr.SmmalaChains(sc.model(name), mc.SMMALA(h), C, seed=1)
    s, g, a = oc.run(R40)
    for v in (s, g, a):
        v.setflags(write=False)
    return oc, s, g, a


def assert_same(ch, task, oc, s, g, a, what=""):
    assert np.array_equal(bits(ch._samples), bits(s)), what + ": samples"
    assert np.array_equal(bits(ch._gradients), bits(g)), what + ": gradients"
    assert np.array_equal(ch.diagnostics["accept"].T, a.astype(bool)), what + ": accept bits"
    assert np.array_equal(bits(ch.final_x), bits(oc.x)), what + ": final_x"
    assert np.array_equal(bits(ch.final_lp), bits(oc.lp)), what + ": final_lp"
    assert task.evals == oc.evals, what + ": evals"


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
    oc, s, g, a = reference(name)
    t = (sc.model(name) * mc.SMMALA(h) * R40).batch(C, seed=1)
    ch = mc.run(t)
    assert_same(ch, t, oc, s, g, a, name)
    assert a.any() and not a.all(), (name, a.mean())          # both accepted and rejected kept steps
    assert t.step_kernel == "smm_step"
    assert np.isnan(t.tuner_state()["step"]).all()


@pytest.mark.parametrize("spl", [1, 7])
def test_steps_per_launch(gpu, spl):
    name = "logistic_n17_d5"
    oc, s, g, a = reference(name)
    t = (sc.model(name) * mc.SMMALA(1.0) * R40).batch(70, seed=1, steps_per_launch=spl)
    assert_same(mc.run(t), t, oc, s, g, a, f"spl {spl}")


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
    s, g, a = oc.run(r)
    assert_same(mc.run(t), t, oc, s, g, a, "tuned")
    step = t.tuner_state()["step"]
    assert np.array_equal(bits(step), bits(oc.t_step))
    assert len(np.unique(step)) > 1 and not (step == 1.0).any()


def test_tuned_kept_range(gpu):
    _tuned(None)


def test_tuned_set_tuner_burnin(gpu):
    _tuned(20)


def test_fork_reset_set_state(gpu):
    name = "logistic_n17_d5"
    m = sc.model(name)
    r = mc.SerialMC(steps=20)
    oc = sr.SmmalaChains(m, mc.SMMALA(1.0), 70, seed=5)
    t = (m * mc.SMMALA(1.0) * r).batch(70, seed=5)
    s, g, a = oc.run(r)
    assert_same(mc.run(t), t, oc, s, g, a, "first run")
    # fork chains [16, 48): continues exactly those chains
    h = ct.c_void_p()
    _lib.check(_lib.load().mcmc_chains_fork(t.handle(), 16, 32, ct.byref(h)))
    try:
        samples = np.empty((20, 5, 32))
        out = _lib.Outputs()
        out.samples = samples.ctypes.data
        rc = _lib.RunnerCfg(0, 1, 20)
        _lib.check(_lib.load().mcmc_run_serialmc(h, ct.byref(rc), ct.byref(out)))
    finally:
        _lib.load().mcmc_chains_destroy(h)
    s2, g2, a2 = oc.run(r)
    assert np.array_equal(bits(samples), bits(s2[:, :, 16:48])), "fork"
    assert_same(mc.run(t), t, oc, s2, g2, a2, "source after fork")
    # set_state: the reset hook keeps the stale invG / firstTerm
    x = np.random.default_rng(9).standard_normal((5, 70)) * 0.3
    lp = mc.reset(t, x)
    assert np.array_equal(bits(lp), bits(oc.set_state(x)))
    s3, g3, a3 = oc.run(r)
    assert_same(mc.run(t), t, oc, s3, g3, a3, "after set_state")
    # reset restarts
    t.reset()
    oc.reset()
    s4, g4, a4 = oc.run(r)
    assert_same(mc.run(t), t, oc, s4, g4, a4, "after reset")
    assert np.array_equal(bits(s4), bits(s))


def test_group_equals_one_context(gpu):
    name = "logistic_neg_n33_d16"
    oc, s, g, a = reference(name)
    t = (sc.model(name) * mc.SMMALA(0.5) * R40).batch(100, seed=1, devices=(0, 0))
    ch = mc.run(t)
    assert np.array_equal(bits(ch._samples), bits(s))
    assert np.array_equal(bits(ch._gradients), bits(g))
    assert np.array_equal(ch.diagnostics["accept"].T, a.astype(bool))


def _raises(code, text, f):
    with pytest.raises(_lib.MCMCError) as e:
        f()
    assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))


def _create(m, sp, C=4):
    h = ct.c_void_p()
    cfg = sp.cfg()
    try:
        _lib.check(_lib.load().mcmc_chains_create(m._handle(0), ct.byref(cfg), C, 0, ct.c_uint64(1), None, ct.byref(h)))
    finally:
        if h.value:
            _lib.load().mcmc_chains_destroy(h)


def test_refusals(gpu):
    X, Y = sc.data(20, 17, 1)
    wide = mc.model(mc.LogisticRegression(X, Y), vars=np.zeros(17), gradient=True, tensor=True)
    _raises(_lib.MCMC_E_UNSUPPORTED, "d <= 16", lambda: _create(wide, mc.SMMALA(1.0)))
    X, Y = sc.data(20, 4, 2)
    lin = mc.model(mc.LinearRegression(X, Y), vars=np.zeros(4), gradient=True)
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, "SMMALA sampler requires model with tensor function",
            lambda: _create(lin, mc.SMMALA(1.0)))
    lin_t = mc.model(mc.LinearRegression(X, Y), vars=np.zeros(4), gradient=True, tensor=True)
    _raises(_lib.MCMC_E_UNSUPPORTED, "no tensor function", lambda: lin_t._handle(0))
    iso_t = mc.model(mc.IsoNormalDot(), init=np.ones(3), grad=True, tensor=True)
    _raises(_lib.MCMC_E_UNSUPPORTED, "no tensor function", lambda: iso_t._handle(0))
    name = "logistic_n17_d5"
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, "SMMALA sampler requires model with tensor function",
            lambda: _create(sc.model(name, False), mc.SMMALA(1.0)))
    nograd = mc.model(sc.model(name).target, vars=np.zeros(5))
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, "SMMALA sampler requires model with gradient function",
            lambda: _create(nograd, mc.SMMALA(1.0)))
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, "model has no tensor function",
            lambda: sc.model(name, False).evalallt(np.zeros(5)))
    # an init whose log-target is -Inf: the logistic term saturates (the reference's p rounds to 0)
    Xb = np.ones((4, 1))
    big = mc.model(mc.LogisticRegression(Xb, np.zeros(4)), vars=np.zeros(1), gradient=True, tensor=True)
    h = ct.c_void_p()
    cfg = mc.SMMALA(1.0).cfg()
    x0 = np.full((1, 4), 800.0)
    with pytest.raises(_lib.OutOfSupportError):
        _lib.check(_lib.load().mcmc_chains_create(big._handle(0), ct.byref(cfg), 4, 0, ct.c_uint64(1), _lib.dptr(x0),
                                                  ct.byref(h)))
    # SeqMC refuses SMMALA targets
    t = (sc.model(name) * mc.SMMALA(1.0) * R40).batch(8, seed=1)
    targets = (ct.c_void_p * 1)(t.handle())
    cfgq = (ct.c_int64 * 2)(2, 0)
    trig = ct.c_double(0.1)
    buf = (ct.c_char * 24)()
    ct.memmove(buf, cfgq, 16)
    ct.memmove(ct.addressof(buf) + 16, ct.addressof(trig), 8)
    parts = np.zeros((5, 8))
    rc = _lib.load().mcmc_run_seqmc(targets, 1, 8, parts.ctypes.data, ct.addressof(buf), ct.c_uint64(1), 0, None, None,
                                    None, None)
    assert rc == _lib.MCMC_E_UNSUPPORTED and b"SMMALA" in _lib.load().mcmc_last_error()


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
