"""ERMLMC and RMLMC (lmc.hip) against the checker (tests/manifold_oracle.c), bit for bit."""
import numpy as np
import pytest

import manifold_harness as mh
import manifold_ref as lr
import mcmchip as mc
import pmala_cases as pc
import smmala_cases as sc
from manifold_harness import R40, _create, _raises, bits
from mcmchip import _lib

pytestmark = pytest.mark.gpu
KINDS = ["ermlmc", "rmlmc"]


def sampler(kind, h, n=3, tuner=None):
    """ERMLMC(n, h) or RMLMC(n, h, 2)"""
    return mc.ERMLMC(n, float(h), tuner) if kind == "ermlmc" else mc.RMLMC(n, float(h), 2, tuner)


def shape_sampler(kind, name):
    return sampler(kind, sc.SHAPES[name][4])          # h: the shape's SMMALA step


FAM = mh.Family(lr.LmcChains, pc, lambda name, kind: shape_sampler(kind, name), kernel="lmc_step")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(pc.SHAPES))
def test_parity(gpu, name, kind):
    C = pc.SHAPES[name][3]
    ref = FAM.reference(name, kind)
    a, cn = ref.a, ref.counters
    t = (pc.model(name) * shape_sampler(kind, name) * R40).batch(C, seed=1)
    ch = mc.run(t)
    FAM.assert_same(ch, t, ref, name)
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
    ref = FAM.ran(oc, R40)
    assert oc.counters.n_failed > 0 and ref.a.any(), (oc.counters.n_failed, ref.a.mean())
    FAM.assert_same(mc.run(t), t, ref, "failed trajectories")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("spl", [0, 1, 7])
def test_steps_per_launch(gpu, spl, kind):
    name = "logistic_n17_d5"
    t = (pc.model(name) * shape_sampler(kind, name) * R40).batch(70, seed=1, steps_per_launch=spl)
    FAM.assert_same(mc.run(t), t, FAM.reference(name, kind), f"spl {spl}")


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
    ref = FAM.ran(oc, r)
    assert oc.counters.n_adapt == 4 * 70
    FAM.assert_same(mc.run(t), t, ref, "tuned")
    ts = t.tuner_state()
    assert np.array_equal(bits(ts["step"]), bits(oc.t_step))
    assert np.array_equal(ts["nleaps"], oc.t_leaps)
    assert len(np.unique(ts["step"])) > 1 and not (ts["step"] == 0.9).any()
    assert len(np.unique(ts["nleaps"])) > 1


@pytest.mark.parametrize("kind", KINDS)
def test_fork_reset_set_state(gpu, kind):
    """set_state: pars, logTarget and grad at x; the next step recomputes all geometry from it"""
    name = "logistic_n17_d5"
    mh.fork_reset_set_state(FAM, pc.model(name), shape_sampler(kind, name))


@pytest.mark.parametrize("kind", KINDS)
def test_group_equals_one_context(gpu, kind):
    """a two-block group on one device"""
    name = "logistic_neg_n33_d16"
    t = (pc.model(name) * shape_sampler(kind, name) * R40).batch(100, seed=1, devices=(0, 0))
    mh.assert_outputs(mc.run(t), FAM.reference(name, kind))


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(gpu, kind):
    nm = "ERMLMC" if kind == "ermlmc" else "RMLMC"
    cls = mc.ERMLMC if kind == "ermlmc" else mc.RMLMC
    cfg = cls().cfg()
    # d > 16; a model with has_gradient 2, 1 and 0
    mh.gradient_refusals(nm, cfg, nm + " is built for d <= 16")
    name = "logistic_n17_d5"
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
    mh.store_leaps_refuses(t, nm)
    mh.seqmc_refuses(t, nm)


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
    z, ma, mb, se = mh.posterior_z(a._samples, b._samples, C)
    print("means", ma, mb, "se", se, "z", z, "acceptance", a.diagnostics["accept"].mean(),
          b.diagnostics["accept"].mean())
    assert (z < 5).all(), (ma, mb, se)
