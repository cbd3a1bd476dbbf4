"""SerialTempMC without a GPU: the library's validation, the checker (tests/stemp_oracle.c) against a literal
transcription of run_serialtempmc (SerialTempMC.jl:31-85), and the census of the case table the GPU tests run."""
import ctypes as ct
import math

import numpy as np
import pytest

import mcmchip as mc
import oracle_ref as orc
import stemp_cases as sc
import stemp_ref
from mcmchip import _lib
from mcmchip.seqmc import target_seed


# ------------------------------------------------------------------ validation
def _validate(steps, burnin, period):
    from mcmchip.serialtemp import _StempCfg
    lib = _lib.load()
    c = _StempCfg(steps, burnin, period)
    return lib.mcmc_serialtempmc_validate(ct.byref(c)), lib.mcmc_last_error().decode()


def test_validate_codes_and_messages():
    """every field at passing and failing values; the reference's assert texts (SerialTempMC.jl:22-23)"""
    assert _validate(1, 0, 5)[0] == 0                                  # the reference's defaults
    assert _validate(100, 99, 1)[0] == 0
    assert _validate(2 ** 32 - 1, 0, 2 ** 40)[0] == 0
    assert _validate(10, -1, 5) == (1, "Burnin rounds (-1) should be >= 0")
    assert _validate(10, 10, 5) == (1, "Steps (10) should be > to burnin (10)")
    assert _validate(0, 0, 5) == (1, "Steps (0) should be > to burnin (0)")
    assert _validate(3, 7, 5) == (1, "Steps (3) should be > to burnin (7)")
    rc, msg = _validate(10, 0, 0)
    assert rc == 1 and "swapPeriod (0)" in msg
    assert _validate(10, 0, -3)[0] == 1
    assert _validate(10, 0, 1)[0] == 0
    assert _validate(2 ** 32, 0, 5) == (1, "steps exceed 2^32")
    assert _validate(2 ** 32 + 5, 2 ** 32, 5)[0] == 1
    assert _lib.load().mcmc_serialtempmc_validate(None) == 1


def test_python_runner_asserts_like_the_reference():
    r = mc.SerialTempMC()
    assert (r.steps, r.burnin, r.swapPeriod) == (1, 0, 5)              # SerialTempMC.jl:29
    r = mc.SerialTempMC(steps=50, burnin=10, swapPeriod=3)
    assert (r.steps, r.burnin, r.swapPeriod) == (50, 10, 3)
    assert mc.SerialTempMC(50, 10, 3).cfg().swap_period == 3
    with pytest.raises(AssertionError, match=r"Burnin rounds \(-1\) should be >= 0"):
        mc.SerialTempMC(steps=5, burnin=-1)
    with pytest.raises(AssertionError, match=r"Steps \(5\) should be > to burnin \(5\)"):
        mc.SerialTempMC(steps=5, burnin=5)
    m = mc.model(mc.NormalDSL(0.0, 1.0), v=np.zeros(2))
    t = m * mc.RWM(0.5) * mc.SerialTempMC(steps=5)
    assert isinstance(t, mc.MCMCTask) and t.runner.swapPeriod == 5
    with pytest.raises(AssertionError, match="Runners do not have the same runner type"):
        mc.run([t, m * mc.RWM(0.5) * mc.SerialMC(steps=5)])
    m3 = mc.model(mc.NormalDSL(0.0, 1.0), v=np.zeros(3))
    with pytest.raises(AssertionError, match="Models do not have the same parameter vector size"):
        mc.run([t, m3 * mc.RWM(0.5) * mc.SerialTempMC(steps=5)])


# ------------------------------------------------------------------ literal transcription
class _Sample:
    def __init__(self, ppars, plogtarget, pars, logtarget):             # samplers.jl:24-25
        self.ppars, self.plogtarget, self.pars, self.logtarget = ppars, plogtarget, pars, logtarget


class _Task:
    """A SamplerTask of one chain: its own position and log-target, moved only when consumed or reset.  The sampler
    step is the oracle's; its draws are those of the library's schedule, in which every target's step counter advances
    on every runner step: `clock` holds the counter a consume at the present runner step reads."""

    def __init__(self, m, s, seed, chain, x0, clock, index):
        self.oc = orc.OracleChains(m, s, nchains=1, seed=seed, chain_offset=chain, init_x=x0.reshape(-1, 1).copy())
        self.m, self.clock, self.index = m, clock, index

    def reset(self, pars):                                              # RWM.jl:49, MALA.jl:75-78
        self.oc.x[:, 0] = pars
        self.oc.lp[0] = orc.eval_batch(self.m, pars.reshape(-1, 1))[0][0]

    def consume(self):
        self.oc.steps_done = self.clock[self.index]
        pars, logtarget = self.oc.x[:, 0].copy(), float(self.oc.lp[0])
        self.oc.run(mc.SerialMC(steps=1), nthreads=1)
        return _Sample(self.oc.x[:, 0].copy(), float(self.oc.lp[0]), pars, logtarget)


def _literal(pairs, seeds, chain, x0, steps, burnin, swapPeriod, logW, seed):
    """run_serialtempmc (SerialTempMC.jl:31-85) line by line, one-based as written"""
    nmods = len(pairs)
    clock = [0] * nmods
    tasks = [_Task(m, s, seeds[k], chain, x0, clock, k) for k, (m, s) in enumerate(pairs)]
    samples = np.full((len(x0), steps - burnin), np.nan)
    mod = np.zeros(steps - burnin, dtype=np.int32)
    swapped = np.zeros(steps - burnin, dtype=bool)
    at = 1
    s = tasks[at - 1].consume()
    ppars, logtarget, pars = s.ppars, s.logtarget, s.pars
    for i in range(1, steps + 1):
        for k in range(nmods):
            clock[k] = (i - 1) + (1 if k == 0 else 0)
        acc = False
        if i % swapPeriod == 0:
            u, u2 = stemp_ref.draws(seed, chain, i)
            at2 = 1 + min(nmods - 2, int(math.floor(u * (nmods - 1))))       # rand(1:(nmods-1))
            at2 = at2 + 1 if at2 >= at else at2
            tasks[at2 - 1].reset(pars)
            s2 = tasks[at2 - 1].consume()
            if u2 < stemp_ref.det_exp(logtarget - s2.logtarget + logW[at2 - 1] - logW[at - 1]):
                at, s = at2, s2
                acc = True
        else:
            s = tasks[at - 1].consume()
        ppars, logtarget, pars = s.ppars, s.logtarget, s.pars
        if i > burnin:
            pos = i - burnin
            samples[:, pos - 1] = ppars
            mod[pos - 1] = at
            swapped[pos - 1] = acc
    return samples, mod, swapped


@pytest.mark.parametrize("K,sname,period,burnin,logW", [
    (2, "rwm", 1, 0, None), (2, "mala", 2, 3, (0.0, 0.5)), (3, "rwm", 2, 0, (0.3, 0.0, -0.6)), (3, "mala", 5, 7, None),
    (3, "rwm", 3, 1, None)])
def test_checker_equals_the_literal_transcription(K, sname, period, burnin, logW):
    """stored rows, the `at` sequence and the swap decisions of every walker"""
    d, C, steps, seed, offset = 2, 5, 40, 77, 3
    pairs = [(mc.model(mc.NormalDSL(0.0, sg), v=np.zeros(d), gradient=True), sc.SAMPLERS[sname]())
             for sg in sc.SIGMAS[:K]]
    seeds = [target_seed(seed, k) for k in range(K)]
    x0 = 1.5 * np.random.default_rng(5).standard_normal((d, C))
    chains = [orc.OracleChains(m, s, nchains=C, seed=seeds[k], chain_offset=offset, init_x=x0.copy())
              for k, (m, s) in enumerate(pairs)]
    w = np.zeros(K) if logW is None else np.array(logW)
    got = stemp_ref.serialtempmc(chains, steps, burnin, period, logW, seed)
    nacc = 0
    for c in range(C):
        s, mod, swapped = _literal(pairs, seeds, offset + c, x0[:, c].copy(), steps, burnin, period, w, seed)
        assert sc.bits_equal(got["samples"][:, :, c], s.T), f"walker {c}: stored rows"
        assert np.array_equal(got["mod"][:, c] + 1, mod), f"walker {c}: at"
        assert np.array_equal(got["swap"][:, c], swapped), f"walker {c}: swap decisions"
        assert got["final_at"][c] + 1 == mod[-1]
        nacc += int(swapped.sum())
    cnt = got["counters"]
    assert 0 < cnt["accepted"] and 0 < cnt["rejected"] and nacc > 0
    assert [c.steps_done for c in chains] == [steps + 1] + [steps] * (K - 1)


def test_pick_is_the_reference_draw():
    """zero-based r = min(K - 2, floor(u (K - 1))) skips the walker's own task"""
    for K in (2, 3, 5):
        for at in range(K):
            seen = set()
            for u in np.linspace(0.0, np.nextafter(1.0, 0.0), 97):
                t = stemp_ref.pick(float(u), K, at)
                assert 0 <= t < K and t != at
                seen.add(t)
            assert seen == set(range(K)) - {at}


# ------------------------------------------------------------------ the case table
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_case_table_census(name):
    """every GPU parity case proposes, accepts and rejects swaps and visits every target, where its logW allows"""
    run = sc.Run(name)
    out, chains = sc.oracle_run(run)
    sc.check_expectation(run.cs, out["counters"], run.C)
    assert out["counters"]["nan"] == 0
    assert np.all(np.isfinite(out["samples"]))
    assert [c.steps_done for c in chains] == [run.cs["steps"] + 1] + [run.cs["steps"]] * (run.K - 1)


def test_forced_vectors():
    """logW = (0, +800): exp(. + 800) is +Inf, the swap to target 1 is always accepted and the swap back, exp(. - 800)
    = 0, never; logW = (0, -800): no swap is ever accepted"""
    up, _ = sc.oracle_run(sc.Run("iso-rwm-k2-c65-up"))
    assert up["counters"]["accepted"] == 65 and np.all(up["final_at"] == 1)
    assert np.all(up["mod"][0] == 0) and np.all(up["mod"][1:] == 1)      # period 2: row 0 is step 1, before any swap
    assert np.all(up["swap"][1]) and not up["swap"][2:].any()
    stay, _ = sc.oracle_run(sc.Run("iso-rwm-k2-c65-stay"))
    assert stay["counters"]["accepted"] == 0 and stay["counters"]["rejected"] == 6 * 65
    assert not stay["swap"].any() and not stay["mod"].any() and not stay["final_at"].any()
