"""SeqMC on the CPU: the oracle's run_seqmc (orc_seqmc) held to references it shares no code with.

(a) the literal run_seqmc of test_literal_reference.py on tuned MALA, HMC, tuned HMC, HMCDA and RAM targets;
(b) resampling indices, the weight reset and the trigger flag against exact rational arithmetic;
(c) weight edges: zero-weight blocks, every weight zero, one particle, out-of-support (-Inf / NaN) weights.
The GPU twin (test_seqmc_gpu.py) runs (b) and (c) on the library and everything else bitwise against this oracle.
"""
import math

import numpy as np
import pytest

import mcmchip as mc
import oracle_ref as orc
import seqmc_cases as sc
import test_literal_reference as lit
from mcmchip.seqmc import target_seed
from test_literal_reference import TASKS, literal_seqmc


# ------------------------------------------------------------------ (a) literal tasks the reference file lacks
def hmcda_task(model, s, burnin, seed, chain, step0=0):
    """HMCDA.jl:72-143 from loop counter step0 + 1 under a runner whose burnin is 0 (SeqMC resets reach the task
    through the :reset hook, HMCDA.jl:82-83, which replaces state0 alone): initializeHMCDAStep leaves leapStep = 1
    (H is NaN, test_literal_reference.hmcda_task), `i < runner.burnin` is false from the first step on, so
    leapStep = dualLeapStep = 1 throughout."""
    assert burnin == 0
    state0 = lit.HMCSample(model.init.copy())
    state0.calc(model)
    leapStep = 1.0
    i = step0 + 1
    while True:
        state0.m = lit.randn(seed, chain, i, len(state0.pars))
        state0.update()
        state = state0.copy()
        nLeaps = max(1, lit.julia02_round(s.len / leapStep))
        for _ in range(int(nLeaps)):
            state = lit.leapfrog(state, leapStep, model)
        p = lit.jmin(1.0, lit.jexp(state0.H - state.H))
        if lit.rand(seed, chain, i) < p:
            yield state.pars, state.grad, True, state.logTarget
            state0 = state.copy()
        else:
            yield state0.pars, state0.grad, False, state0.logTarget
        i += 1


_RAM_S = {}      # (task seed, particle slot) -> S: the jump factor lives in the task, outside the :reset hook


def ram_task(model, s, burnin, seed, chain, step0=0):
    """RAM.jl:41-80.  The :reset hook replaces pars and logTarget only (RAM.jl:47): S keeps adapting across
    resets.  The build runs particle n as chain n of every target, so S belongs to (target, slot n) and the loop
    counter in eta is the outer step."""
    d = len(model.init)
    S = _RAM_S.setdefault((seed, chain), np.diag(model.scale * s.scale))
    pars = model.init.copy()
    logTarget = model.eval(pars)
    i = step0 + 1
    rvec = lit.randn(seed, chain, i, d)
    proposedPars = pars + S @ rvec
    proposedLogTarget = model.eval(proposedPars)
    ratio = proposedLogTarget - logTarget
    eta = min(1.0, d * i ** (-2.0 / 3.0))
    SS = np.outer(rvec, rvec) / rvec.dot(rvec) * eta * (min(1.0, lit.jexp(ratio)) - s.rate)
    _RAM_S[(seed, chain)] = np.linalg.cholesky(S @ (np.eye(d) + SS) @ S.T)
    if ratio > 0 or (ratio > math.log(lit.rand(seed, chain, i))):
        yield proposedPars, None, True, proposedLogTarget
    else:
        yield pars, None, False, logTarget


@pytest.fixture
def more_tasks(monkeypatch):
    monkeypatch.setitem(TASKS, 4, hmcda_task)
    monkeypatch.setitem(TASKS, 5, ram_task)
    _RAM_S.clear()


LITERAL = [(s, d) for s in ("mala_tuned", "hmc", "hmc_tuned", "hmcda") for d in (2, 3)] + [("ram", 3)]


@pytest.mark.parametrize("trigger", [0.0, 1e9])
@pytest.mark.parametrize("sname,d", LITERAL)
def test_oracle_seqmc_matches_literal_on_more_samplers(more_tasks, sname, d, trigger):
    """Tuners do not adapt inside SeqMC (the literal tasks run under burnin 0 and keep their configured steps;
    adaptStep = 1 here would move them at once), HMCDA keeps its unit step, RAM adapts S per particle slot."""
    npart, steps, burnin, seed = 12, 4, 1, 29 + d
    parts = np.random.default_rng(seed).standard_normal((npart, d)) * 1.5
    tg_orc, tg_lit = [], []
    for k, sg in enumerate((3.0, 2.0, 1.2)):
        sp = sc.SAMPLERS[sname]()
        tg_orc.append((mc.model(mc.NormalDSL(0.3, sg), v=np.zeros(d), gradient=True), sp))
        tg_lit.append((lit.NormalDSL(0.3, sg, np.zeros(d)), sp, target_seed(seed, k)))
    seeds = [target_seed(seed, k) for k in range(3)]
    s_o, w_o, f_o = orc.seqmc(tg_orc, parts, steps, burnin, trigger, seed, seeds)
    s_l, w_l, f_l = literal_seqmc(tg_lit, parts, steps, burnin, trigger, seed)
    assert np.array_equal(f_o, f_l) and f_o.all() == (trigger > 0)
    np.testing.assert_allclose(s_o, s_l, rtol=lit.RTOL, atol=1e-12)
    np.testing.assert_allclose(w_o, w_l, rtol=lit.RTOL, atol=1e-300)
    assert len(np.unique(s_o[-1, 0])) > 1                           # the mutations moved the particles


# ------------------------------------------------------------------ (b) exact rational resampling
@pytest.mark.parametrize("npart", sc.EXACT_SIZES)
def test_oracle_resampling_against_exact_rationals(npart):
    sc.check_exact_resampling(sc.oracle_run, sc.exact_particles(npart, sc.EXACT_SEED[npart]), sc.EXACT_SEED[npart])


def test_oracle_draw_equal_to_cp_selects_that_particle():
    sc.check_tie_rule(sc.oracle_run)


# ------------------------------------------------------------------ (c) weight edges
@pytest.mark.parametrize("npart,where", sc.ZERO_BLOCK_CASES)
def test_oracle_zero_weight_blocks_are_never_selected(npart, where):
    P, zero = sc.zero_block_particles(npart, where, 60 + npart)
    rs = sc.check_exact_resampling(sc.oracle_run, P, 60 + npart, zero=zero)
    assert len(set(rs)) > 1


def test_oracle_all_zero_weights_select_the_last_particle():
    sc.check_all_zero_weights(sc.oracle_run)


def test_oracle_single_particle_never_resamples():
    sc.check_single_particle(sc.oracle_run)


def test_oracle_out_of_support_particles_do_not_survive_a_resample():
    sc.check_gamma_always(sc.oracle_run)


def test_oracle_out_of_support_weights_turn_nan_without_resampling():
    sc.check_gamma_never(sc.oracle_run)
