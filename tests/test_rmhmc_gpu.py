"""RMHMC (rmhmc.hip) against the checker (tests/manifold_oracle.c), bit for bit."""
import numpy as np
import pytest

import manifold_harness as mh
import manifold_ref as rr
import mcmchip as mc
import pmala_cases as pc
from manifold_harness import R40, _create, _raises, bits
from mcmchip import _lib

pytestmark = pytest.mark.gpu
# (nLeaps, leapStep, nNewton): one leapfrog with one pass, and five with four; the step at d = 16 is smaller
SAMPLERS = {"l1n1": (1, 0.8, 1), "l5n4": (5, 0.6, 4)}


def sampler(key, name):
    n, e, k = SAMPLERS[key]
    return mc.RMHMC(n, e / 2 if pc.SHAPES[name][2] == 16 else e, k)


FAM = mh.Family(rr.RmhmcChains, pc, lambda name, key: sampler(key, name))


@pytest.mark.parametrize("key", list(SAMPLERS))
@pytest.mark.parametrize("name", list(pc.SHAPES))
def test_parity(gpu, name, key):
    C = pc.SHAPES[name][3]
    ref = FAM.reference(name, key)
    a, cn = ref.a, ref.counters
    t = (pc.model(name) * sampler(key, name) * R40).batch(C, seed=1)
    ch = mc.run(t)
    FAM.assert_same(ch, t, ref, name)
    assert t.step_kernel == "rm_step"
    assert a.any(), (name, a.mean())
    ts = t.tuner_state()
    assert np.isnan(ts["step"]).all() and (ts["nleaps"] == 0).all()
    if key == "l5n4" and C >= 8:
        # chains of one workgroup drew different trajectory lengths and both signs
        assert cn.nrl_min == 1 and cn.nrl_max == 5 and cn.n_plus > 0 and cn.n_minus > 0, name
        assert cn.n_failed == 0
    if key == "l1n1":
        assert cn.nrl_min == 1 and cn.nrl_max == 1


@pytest.mark.parametrize("spl", [0, 1, 7])
def test_steps_per_launch(gpu, spl):
    name = "logistic_n17_d5"
    t = (pc.model(name) * sampler("l5n4", name) * R40).batch(70, seed=1, steps_per_launch=spl)
    FAM.assert_same(mc.run(t), t, FAM.reference(name, "l5n4"), f"spl {spl}")


def test_chain_offset(gpu):
    """chains 32.. of the 70 as a batch of their own (global ids by chain_offset): a workgroup's trajectory length is
    its own chains' maximum, and a chain's arithmetic does not depend on it"""
    name = "logistic_n17_d5"
    t = (pc.model(name) * sampler("l5n4", name) * R40).batch(38, seed=1, chain_offset=32)
    mh.assert_outputs(mc.run(t), FAM.reference(name, "l5n4"), chains=slice(32, None))


def test_tuned(gpu):
    """adaptStep 5 inside a burnin of 20: leapStep and nLeaps adapt four times"""
    name = "logistic_n17_d5"
    sp = mc.RMHMC(3, 0.9, 2, mc.EmpiricalMCMCTuner(adaptStep=5, targetRate=0.7, maxStep=6, targetPath=2.0))
    r = mc.SerialMC(steps=40, burnin=20)
    oc = rr.RmhmcChains(pc.model(name), sp, 70, seed=2)
    t = (pc.model(name) * sp * r).batch(70, seed=2)
    ref = FAM.ran(oc, r)
    assert oc.counters.n_adapt == 4 * 70
    FAM.assert_same(mc.run(t), t, ref, "tuned")
    ts = t.tuner_state()
    assert np.array_equal(bits(ts["step"]), bits(oc.t_step))
    assert np.array_equal(ts["nleaps"], oc.t_leaps)
    assert len(np.unique(ts["step"])) > 1 and not (ts["step"] == 0.9).any()
    assert len(np.unique(ts["nleaps"])) > 1


def test_fork_reset_set_state(gpu):
    """set_state: pars, logTarget and grad at x; the next step recomputes the rest"""
    name = "logistic_n17_d5"
    mh.fork_reset_set_state(FAM, pc.model(name), sampler("l5n4", name))


def test_group_equals_one_context(gpu):
    name = "logistic_neg_n33_d16"
    t = (pc.model(name) * sampler("l5n4", name) * R40).batch(100, seed=1, devices=(0, 0))
    mh.assert_outputs(mc.run(t), FAM.reference(name, "l5n4"))


def test_failed_trajectories_are_rejected(gpu):
    """a leap step so large that trajectories leave the support or fail a pivot: those steps are rejected, the others
    go on, and no chain carries a NaN"""
    name = "logistic_n17_d5"
    sp = mc.RMHMC(5, 1.2, 2)
    oc = rr.RmhmcChains(pc.model(name), sp, 70, seed=3)
    t = (pc.model(name) * sp * R40).batch(70, seed=3)
    ref = FAM.ran(oc, R40)
    assert oc.counters.n_failed > 0 and ref.a.any(), (oc.counters.n_failed, ref.a.mean())
    FAM.assert_same(mc.run(t), t, ref, "failed trajectories")


def test_refusals(gpu):
    cfg = mc.RMHMC().cfg()
    # d > 16; a model without tensor derivatives, after the gradient and tensor checks
    mh.gradient_refusals("RMHMC", cfg, "RMHMC is built for d <= 16")
    name = "logistic_n17_d5"
    # nNewton travels in t0: an integer in 1 .. 2^31 - 1
    for t0 in (2.5, 2.0 ** 31):
        bad = mc.RMHMC().cfg()
        bad.t0 = t0
        _raises(_lib.MCMC_E_INVALID_ARG, "t0 carries nNewton", lambda: _create(pc.model(name), bad))
    # storeLeaps and SeqMC
    t = (pc.model(name) * mc.RMHMC() * R40).batch(8, seed=1)
    mh.store_leaps_refuses(t, "RMHMC")
    mh.seqmc_refuses(t, "RMHMC")


def test_posterior_agrees_with_smmala(gpu):
    """4 096 chains of RMHMC(3, 0.5, 4) and of SMMALA(0.5) on logistic_40_10, 100 kept steps after 100: per coordinate
    the grand means differ by less than 5 standard errors of their difference, the errors from the between-chain
    variance of the chain means (independent chains: a z-test).  leapStep 0.5 with nNewton 4 is the pair at which
    tests/test_rmhmc_cpu.py shows the checker's RMHMC inside the same bound."""
    C = 4096
    r = mc.SerialMC(steps=200, burnin=100)
    m = pc.logistic_40_10()
    a = mc.run((m * mc.RMHMC(3, 0.5, 4) * r).batch(C, seed=21))
    b = mc.run((m * mc.SMMALA(0.5) * r).batch(C, seed=22))
    z, ma, mb, se = mh.posterior_z(a._samples, b._samples, C)
    print("means", ma, mb, "se", se, "z", z, "acceptance", a.diagnostics["accept"].mean(),
          b.diagnostics["accept"].mean())
    assert (z < 5).all(), (ma, mb, se)
