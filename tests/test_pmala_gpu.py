"""PMALA and the device tensor derivatives (pmala.hip) against the checker (tests/pmala_oracle.c), bit for bit."""
import ctypes as ct
import functools

import numpy as np
import pytest

import mcmchip as mc
import pmala_cases as pc
import pmala_ref as pr
import smmala_cases as sc
from mcmchip import _lib

pytestmark = pytest.mark.gpu
R40 = mc.SerialMC(steps=40, burnin=10, thinning=3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the checker's R40 run of a shape, computed once and shared: (samples, grads, accept, final state, evals)"""
    _, _, _, C, h = pc.SHAPES[name]
    oc = pr.PmalaChains(pc.model(name), mc.PMALA(h), C, seed=1)
    s, g, a = oc.run(R40)
    state = {k: getattr(oc, k).copy() for k in ("x", "lp", "g", "G", "invG", "ft", "c")}
    for v in (s, g, a, *state.values()):
        v.setflags(write=False)
    return s, g, a, state, oc.evals


def state_of(oc):
    return {k: getattr(oc, k) for k in ("x", "lp", "g", "G", "invG", "ft", "c")}


def assert_same(ch, task, s, g, a, state, evals, what=""):
    assert np.array_equal(bits(ch._samples), bits(s)), what + ": samples"
    assert np.array_equal(bits(ch._gradients), bits(g)), what + ": gradients"
    assert np.array_equal(ch.diagnostics["accept"].T, a.astype(bool)), what + ": accept bits"
    assert np.array_equal(bits(ch.final_x), bits(state["x"])), what + ": final_x"
    assert np.array_equal(bits(ch.final_lp), bits(state["lp"])), what + ": final_lp"
    ms = task.manifold_state()
    for dev, ref in (("grad", "g"), ("G", "G"), ("invG", "invG"), ("first_term", "ft"), ("corr", "c")):
        assert np.array_equal(bits(ms[dev]), bits(state[ref])), what + ": final " + ref
    assert task.evals == evals, what + ": evals"


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
    s, g, a, state, evals = reference(name)
    t = (pc.model(name) * mc.PMALA(h) * R40).batch(C, seed=1)
    ch = mc.run(t)
    assert_same(ch, t, s, g, a, state, evals, name)
    assert a.any() and not a.all(), (name, a.mean())          # both accepted and rejected kept steps
    assert t.step_kernel == "pm_step"
    assert np.isnan(t.tuner_state()["step"]).all()


@pytest.mark.parametrize("spl", [0, 1, 7])
def test_steps_per_launch(gpu, spl):
    name = "logistic_n17_d5"
    s, g, a, state, evals = reference(name)
    t = (pc.model(name) * mc.PMALA(1.0) * R40).batch(70, seed=1, steps_per_launch=spl)
    assert_same(mc.run(t), t, s, g, a, state, evals, f"spl {spl}")


def test_tuned(gpu):
    """adaptStep 5 inside a burnin of 20: the drift step adapts four times"""
    name = "logistic_n17_d5"
    sp = mc.PMALA(1.0, mc.EmpiricalMCMCTuner(adaptStep=5, targetRate=0.7))
    r = mc.SerialMC(steps=40, burnin=20)
    oc = pr.PmalaChains(pc.model(name), sp, 70, seed=2)
    t = (pc.model(name) * sp * r).batch(70, seed=2)
    s, g, a = oc.run(r)
    assert_same(mc.run(t), t, s, g, a, state_of(oc), oc.evals, "tuned")
    step = t.tuner_state()["step"]
    assert np.array_equal(bits(step), bits(oc.t_step))
    assert len(np.unique(step)) > 1 and not (step == 1.0).any()


def test_fork_reset_set_state(gpu):
    name = "logistic_n17_d5"
    m = pc.model(name)
    r = mc.SerialMC(steps=20)
    oc = pr.PmalaChains(m, mc.PMALA(1.0), 70, seed=5)
    t = (m * mc.PMALA(1.0) * r).batch(70, seed=5)
    s, g, a = oc.run(r)
    assert_same(mc.run(t), t, s, g, a, state_of(oc), oc.evals, "first run")
    # fork chains [16, 48): continues exactly those chains (c is copied)
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
    assert_same(mc.run(t), t, s2, g2, a2, state_of(oc), oc.evals, "source after fork")
    # set_state: the reset hook keeps the stale invG / firstTerm / c, and the next step uses them
    x = np.random.default_rng(9).standard_normal((5, 70)) * 0.3
    stale = oc.c.copy()
    lp = mc.reset(t, x)
    assert np.array_equal(bits(lp), bits(oc.set_state(x)))
    assert np.array_equal(bits(t.manifold_state()["corr"]), bits(stale))
    s3, g3, a3 = oc.run(r)
    assert_same(mc.run(t), t, s3, g3, a3, state_of(oc), oc.evals, "after set_state")
    # reset restarts and recomputes c
    t.reset()
    oc.reset()
    assert np.array_equal(bits(t.manifold_state()["corr"]), bits(oc.c))
    s4, g4, a4 = oc.run(r)
    assert_same(mc.run(t), t, s4, g4, a4, state_of(oc), oc.evals, "after reset")
    assert np.array_equal(bits(s4), bits(s))


def test_group_equals_one_context(gpu):
    name = "logistic_neg_n33_d16"
    s, g, a, state, _ = reference(name)
    t = (pc.model(name) * mc.PMALA(0.5) * R40).batch(100, seed=1, devices=(0, 0))
    ch = mc.run(t)
    assert np.array_equal(bits(ch._samples), bits(s))
    assert np.array_equal(bits(ch._gradients), bits(g))
    assert np.array_equal(ch.diagnostics["accept"].T, a.astype(bool))
    assert np.array_equal(bits(t.manifold_state()["corr"]), bits(state["c"]))


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
    # d > 16
    X, Y = sc.data(20, 17, 1)
    wide = mc.model(mc.LogisticRegression(X, Y), vars=np.zeros(17), gradient=True, tensor=True, dtensor=True)
    _raises(_lib.MCMC_E_UNSUPPORTED, "d <= 16", lambda: _create(wide, mc.PMALA(1.0)))
    _raises(_lib.MCMC_E_UNSUPPORTED, "d <= 16", lambda: wide.evalalldt(np.zeros(17)))
    # a model without tensor derivatives, after the gradient and tensor checks
    name = "logistic_n17_d5"
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, "PMALA sampler requires model with function of tensor derivatives",
            lambda: _create(sc.model(name), mc.PMALA(1.0)))
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, "PMALA sampler requires model with tensor function",
            lambda: _create(sc.model(name, False), mc.PMALA(1.0)))
    nograd = mc.model(sc.model(name).target, vars=np.zeros(5))
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, "PMALA sampler requires model with gradient function",
            lambda: _create(nograd, mc.PMALA(1.0)))
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, "model has no function of tensor derivatives",
            lambda: sc.model(name).evalalldt(np.zeros(5)))
    # has_gradient == 3 on any other kind
    X, Y = sc.data(20, 4, 2)
    lin = mc.model(mc.LinearRegression(X, Y), vars=np.zeros(4), gradient=True, tensor=True, dtensor=True)
    _raises(_lib.MCMC_E_UNSUPPORTED, "no tensor function", lambda: lin._handle(0))
    # an init whose log-target is -Inf
    Xb = np.ones((4, 1))
    big = mc.model(mc.LogisticRegression(Xb, np.zeros(4)), vars=np.zeros(1), gradient=True, tensor=True, dtensor=True)
    h = ct.c_void_p()
    cfg = mc.PMALA(1.0).cfg()
    x0 = np.full((1, 4), 800.0)
    with pytest.raises(_lib.OutOfSupportError):
        _lib.check(_lib.load().mcmc_chains_create(big._handle(0), ct.byref(cfg), 4, 0, ct.c_uint64(1), _lib.dptr(x0),
                                                  ct.byref(h)))
    # SeqMC refuses PMALA targets
    t = (pc.model(name) * mc.PMALA(1.0) * R40).batch(8, seed=1)
    targets = (ct.c_void_p * 1)(t.handle())
    cfgq = (ct.c_int64 * 2)(2, 0)
    trig = ct.c_double(0.1)
    buf = (ct.c_char * 24)()
    ct.memmove(buf, cfgq, 16)
    ct.memmove(ct.addressof(buf) + 16, ct.addressof(trig), 8)
    parts = np.zeros((5, 8))
    rc = _lib.load().mcmc_run_seqmc(targets, 1, 8, parts.ctypes.data, ct.addressof(buf), ct.c_uint64(1), 0, None, None,
                                    None, None)
    assert rc == _lib.MCMC_E_UNSUPPORTED and b"PMALA" in _lib.load().mcmc_last_error()


def test_posterior_agrees_with_smmala(gpu):
    """4 096 chains of PMALA(0.5) and of SMMALA(0.5) on logistic_40_10, 200 kept steps after 200: per coordinate the
    grand means differ by less than 5 standard errors of their difference, the errors from the between-chain variance
    of the chain means (independent chains: a z-test, false-failure rate below 1e-5 over ten coordinates)."""
    C = 4096
    r = mc.SerialMC(steps=400, burnin=200)
    m = pc.logistic_40_10()
    a = mc.run((m * mc.PMALA(0.5) * r).batch(C, seed=21))
    b = mc.run((m * mc.SMMALA(0.5) * r).batch(C, seed=22))
    ca, cb = a._samples.mean(axis=0), b._samples.mean(axis=0)          # chain means [d][C]
    ma, mb = ca.mean(axis=1), cb.mean(axis=1)
    se = np.sqrt(ca.var(axis=1, ddof=1) / C + cb.var(axis=1, ddof=1) / C)
    z = np.abs(ma - mb) / se
    print("means", ma, mb, "se", se, "z", z, "acceptance", a.diagnostics["accept"].mean(),
          b.diagnostics["accept"].mean())
    assert (z < 5).all(), (ma, mb, se)
