"""ERMLMC and RMLMC (lmc.hip) against the checker (tests/lmc_oracle.c), bit for bit."""
import ctypes as ct
import functools

import numpy as np
import pytest

import lmc_ref as lr
import mcmchip as mc
import pmala_cases as pc
import smmala_cases as sc
from mcmchip import _lib

pytestmark = pytest.mark.gpu
R40 = mc.SerialMC(steps=40, burnin=10, thinning=3)
KINDS = ["ermlmc", "rmlmc"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def sampler(kind, h, n=3, tuner=None):
    """ERMLMC(n, h) or RMLMC(n, h, 2)"""
    return mc.ERMLMC(n, float(h), tuner) if kind == "ermlmc" else mc.RMLMC(n, float(h), 2, tuner)


def shape_sampler(kind, name):
    return sampler(kind, sc.SHAPES[name][4])          # h: the shape's SMMALA step


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """the checker's R40 run of a shape, computed once and shared: (samples, grads, accept, final state, evals,
    counters)"""
    C = pc.SHAPES[name][3]
    oc = lr.LmcChains(pc.model(name), shape_sampler(kind, name), C, seed=1)
    s, g, a = oc.run(R40)
    state = {k: getattr(oc, k).copy() for k in ("x", "lp", "g")}
    for v in (s, g, a, *state.values()):
        v.setflags(write=False)
    return s, g, a, state, oc.evals, oc.counters


def state_of(oc):
    return {k: getattr(oc, k) for k in ("x", "lp", "g")}


def assert_same(ch, task, s, g, a, state, evals, what=""):
    assert np.isfinite(s).all() and np.isfinite(g).all(), what + ": the checker's chains carry a NaN"
    assert np.array_equal(bits(ch._samples), bits(s)), what + ": samples"
    assert np.array_equal(bits(ch._gradients), bits(g)), what + ": gradients"
    assert np.array_equal(ch.diagnostics["accept"].T, a.astype(bool)), what + ": accept bits"
    assert np.array_equal(bits(ch.final_x), bits(state["x"])), what + ": final_x"
    assert np.array_equal(bits(ch.final_lp), bits(state["lp"])), what + ": final_lp"
    assert task.evals == evals, what + ": evals"
    assert "lmc_step" in task.step_kernel, task.step_kernel


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(pc.SHAPES))
def test_parity(gpu, name, kind):
    C = pc.SHAPES[name][3]
    s, g, a, state, evals, cn = reference(name, kind)
    t = (pc.model(name) * shape_sampler(kind, name) * R40).batch(C, seed=1)
    ch = mc.run(t)
    assert_same(ch, t, s, g, a, state, evals, name)
    assert f"lmc_step<{kind}>" == t.step_kernel
    assert a.any(), (name, a.mean())
    ts = t.tuner_state()
    assert np.isnan(ts["step"]).all() and (ts["nleaps"] == 0).all()
    assert cn.n_zero == 0 and cn.nrl_min == 1
    if C >= 8:
        assert cn.nrl_max == 3, name                   # chains of one workgroup drew different trajectory lengths


@pytest.mark.parametrize("kind", KINDS)
def test_failed_trajectories_are_rejected(gpu, kind):
    """a leap step so large that the checker counts failed trajectories (a log-target that is not finite, a failed pivot
    of G, invG or G +- c vxC): those steps are rejected under the mask, the others go on, and no chain carries a NaN"""
    name = "logistic_n17_d5"
    sp = sampler(kind, 1.5, n=4)
    oc = lr.LmcChains(pc.model(name), sp, 70, seed=3)
    t = (pc.model(name) * sp * R40).batch(70, seed=3)
    s, g, a = oc.run(R40)
    assert oc.counters.n_failed > 0 and a.any(), (oc.counters.n_failed, a.mean())
    assert_same(mc.run(t), t, s, g, a, state_of(oc), oc.evals, "failed trajectories")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spl", [0, 1, 7])
def test_steps_per_launch(gpu, spl, kind):
    name = "logistic_n17_d5"
    s, g, a, state, evals, _ = reference(name, kind)
    t = (pc.model(name) * shape_sampler(kind, name) * R40).batch(70, seed=1, steps_per_launch=spl)
    assert_same(mc.run(t), t, s, g, a, state, evals, f"spl {spl}")


@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_equal_one(gpu, kind):
    """two runs of 20 against the checker's one of 40"""
    name = "logistic_n17_d5"
    sp = shape_sampler(kind, name)
    oc = lr.LmcChains(pc.model(name), sp, 70, seed=4)
    s, g, a = oc.run(mc.SerialMC(steps=40))
    t = (pc.model(name) * sp * mc.SerialMC(steps=20)).batch(70, seed=4)
    c1 = mc.run(t)
    c2 = mc.run(t)
    assert np.array_equal(bits(np.concatenate([c1._samples, c2._samples])), bits(s))
    assert np.array_equal(bits(np.concatenate([c1._gradients, c2._gradients])), bits(g))
    assert np.array_equal(np.concatenate([c1.diagnostics["accept"].T, c2.diagnostics["accept"].T]), a.astype(bool))
    assert t.evals == oc.evals


@pytest.mark.parametrize("kind", KINDS)
def test_tuned(gpu, kind):
    """adaptStep 5 inside a burnin of 20: leapStep and nLeaps adapt four times"""
    name = "logistic_n17_d5"
    sp = sampler(kind, 0.9, tuner=mc.EmpiricalMCMCTuner(adaptStep=5, targetRate=0.7, maxStep=6, targetPath=2.0))
    r = mc.SerialMC(steps=40, burnin=20)
    oc = lr.LmcChains(pc.model(name), sp, 70, seed=2)
    t = (pc.model(name) * sp * r).batch(70, seed=2)
    s, g, a = oc.run(r)
    assert oc.counters.n_adapt == 4 * 70
    assert_same(mc.run(t), t, s, g, a, state_of(oc), oc.evals, "tuned")
    ts = t.tuner_state()
    assert np.array_equal(bits(ts["step"]), bits(oc.t_step))
    assert np.array_equal(ts["nleaps"], oc.t_leaps)
    assert len(np.unique(ts["step"])) > 1 and not (ts["step"] == 0.9).any()
    assert len(np.unique(ts["nleaps"])) > 1


@pytest.mark.parametrize("kind", KINDS)
def test_fork_reset_set_state(gpu, kind):
    name = "logistic_n17_d5"
    m = pc.model(name)
    sp = shape_sampler(kind, name)
    r = mc.SerialMC(steps=20)
    oc = lr.LmcChains(m, sp, 70, seed=5)
    t = (m * sp * r).batch(70, seed=5)
    s, g, a = oc.run(r)
    assert_same(mc.run(t), t, s, g, a, state_of(oc), oc.evals, "first run")
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
    assert_same(mc.run(t), t, s2, g2, a2, state_of(oc), oc.evals, "source after fork")
    # set_state: pars, logTarget and grad at x; the next step recomputes all geometry from it
    x = np.random.default_rng(9).standard_normal((5, 70)) * 0.3
    lp = mc.reset(t, x)
    assert np.array_equal(bits(lp), bits(oc.set_state(x)))
    s3, g3, a3 = oc.run(r)
    assert_same(mc.run(t), t, s3, g3, a3, state_of(oc), oc.evals, "after set_state")
    t.reset()
    oc.reset()
    s4, g4, a4 = oc.run(r)
    assert_same(mc.run(t), t, s4, g4, a4, state_of(oc), oc.evals, "after reset")
    assert np.array_equal(bits(s4), bits(s))


@pytest.mark.parametrize("kind", KINDS)
def test_group_equals_one_context(gpu, kind):
    """a two-block group on one device"""
    name = "logistic_neg_n33_d16"
    s, g, a, _, _, _ = reference(name, kind)
    t = (pc.model(name) * shape_sampler(kind, name) * R40).batch(100, seed=1, devices=(0, 0))
    ch = mc.run(t)
    assert np.array_equal(bits(ch._samples), bits(s))
    assert np.array_equal(bits(ch._gradients), bits(g))
    assert np.array_equal(ch.diagnostics["accept"].T, a.astype(bool))


def _raises(code, text, f):
    with pytest.raises(_lib.MCMCError) as e:
        f()
    assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))


def _create(m, cfg, C=4):
    h = ct.c_void_p()
    try:
        _lib.check(_lib.load().mcmc_chains_create(m._handle(0), ct.byref(cfg), C, 0, ct.c_uint64(1), None, ct.byref(h)))
    finally:
        if h.value:
            _lib.load().mcmc_chains_destroy(h)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(gpu, kind):
    nm = "ERMLMC" if kind == "ermlmc" else "RMLMC"
    cls = mc.ERMLMC if kind == "ermlmc" else mc.RMLMC
    cfg = cls().cfg()
    # d > 16
    X, Y = sc.data(20, 17, 1)
    wide = mc.model(mc.LogisticRegression(X, Y), vars=np.zeros(17), gradient=True, tensor=True, dtensor=True)
    _raises(_lib.MCMC_E_UNSUPPORTED, nm + " is built for d <= 16", lambda: _create(wide, cfg))
    # a model with has_gradient 2, 1 and 0
    name = "logistic_n17_d5"
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, nm + " sampler requires model with function of tensor derivatives",
            lambda: _create(sc.model(name), cfg))
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, nm + " sampler requires model with tensor function",
            lambda: _create(sc.model(name, False), cfg))
    nograd = mc.model(sc.model(name).target, vars=np.zeros(5))
    _raises(_lib.MCMC_E_NEEDS_GRADIENT, nm + " sampler requires model with gradient function",
            lambda: _create(nograd, cfg))
    # bad n_leaps, leap_step and t0 at the C ABI
    for field, value, text in (("n_leaps", 0, "Number of leapfrog steps should be > 0"),
                               ("leap_step", 0.0, "Leapfrog step size should be > 0")):
        bad = cls().cfg()
        setattr(bad, field, value)
        _raises(_lib.MCMC_E_INVALID_ARG, text, lambda: _create(pc.model(name), bad))
    if kind == "rmlmc":
        for t0, text in ((0.0, "Number of Newton steps should be > 0"), (2.5, "t0 carries nNewton"),
                         (2.0 ** 31, "t0 carries nNewton")):
            bad = cls().cfg()
            bad.t0 = t0
            _raises(_lib.MCMC_E_INVALID_ARG, text, lambda: _create(pc.model(name), bad))
    # storeLeaps and SeqMC
    t = (pc.model(name) * cls() * R40).batch(8, seed=1)
    buf = np.zeros(8 * 5 * 8)
    nl = np.zeros(8, dtype=np.int32)
    rc = _lib.load().mcmc_chains_store_leaps(t.handle(), 1, _lib.dptr(buf), _lib.dptr(buf), _lib.dptr(buf),
                                             _lib.dptr(buf), _lib.dptr(buf), nl.ctypes.data)
    assert rc == _lib.MCMC_E_UNSUPPORTED and nm.encode() in _lib.load().mcmc_last_error()
    targets = (ct.c_void_p * 1)(t.handle())
    cfgq = (ct.c_int64 * 2)(2, 0)
    trig = ct.c_double(0.1)
    sbuf = (ct.c_char * 24)()
    ct.memmove(sbuf, cfgq, 16)
    ct.memmove(ct.addressof(sbuf) + 16, ct.addressof(trig), 8)
    parts = np.zeros((5, 8))
    rc = _lib.load().mcmc_run_seqmc(targets, 1, 8, parts.ctypes.data, ct.addressof(sbuf), ct.c_uint64(1), 0, None, None,
                                    None, None)
    assert rc == _lib.MCMC_E_UNSUPPORTED and nm.encode() in _lib.load().mcmc_last_error()


def test_ermlmc_posterior_agrees_with_smmala(gpu):
    """4 096 chains of ERMLMC(3, 0.5) and of SMMALA(0.5) on logistic_40_10, 100 kept steps after 100: per coordinate the
    grand means differ by less than 5 standard errors of their difference, the errors from the between-chain variance
    of the chain means (independent chains: a z-test).  tests/test_lmc_cpu.py shows the checker's ERMLMC inside the
    same bound at the same leapStep."""
    C = 4096
    r = mc.SerialMC(steps=200, burnin=100)
    m = pc.logistic_40_10()
    a = mc.run((m * mc.ERMLMC(3, 0.5) * r).batch(C, seed=21))
    b = mc.run((m * mc.SMMALA(0.5) * r).batch(C, seed=22))
    ca, cb = a._samples.mean(axis=0), b._samples.mean(axis=0)          # chain means [d][C]
    ma, mb = ca.mean(axis=1), cb.mean(axis=1)
    se = np.sqrt(ca.var(axis=1, ddof=1) / C + cb.var(axis=1, ddof=1) / C)
    z = np.abs(ma - mb) / se
    print("means", ma, mb, "se", se, "z", z, "acceptance", a.diagnostics["accept"].mean(),
          b.diagnostics["accept"].mean())
    assert (z < 5).all(), (ma, mb, se)
