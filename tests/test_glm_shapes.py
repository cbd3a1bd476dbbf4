"""The regression kernels (glm.hip) at observation-tile, padded-row, slice-geometry and chain-count edges, bitwise
against the oracle, which test_glm_exact.py holds within the rounding bound of an exact reference at the same cases.

The kernels stage X through LDS in 16-observation tiles and special-case the tile count (one tile: no prologue
load; two, three: the pipeline's tail conditions) and the padded rows of the last tile (the logistic bound column is
-inf there); the cases of glm_cases.py put 1, 2, 3 and >= 4 tiles with 0, 1 and 15 padded rows on every slice
geometry, widths on both sides of every geometry edge, and chain counts below, at and above one 16-chain tile.

Step sizes are _sampler()'s.  Oracle acceptance over each sampler's whole sweep (measured on the CPU before any GPU
run; the sweeps need both outcomes):
    rwm 0.525, mala 0.549, mala_tuned 0.528, hmc 0.797, hmcda 0.045 (61 of its 290 cases accept at all: ten steps
    from a start far from the mode leave dual averaging little to keep), ram 0.841
"""
import functools

import numpy as np
import pytest

import mcmchip as mc
import glm_cases as gc
import oracle_ref as orc
from test_gpu_parity import assert_parity, _assert_ram_factor

pytestmark = pytest.mark.gpu

SNAMES = ("rwm", "mala", "mala_tuned", "hmc", "hmcda")
RUNNER = dict(steps=10, burnin=3, thinning=2)
SWEEP_C = 19                                                  # one full 16-chain tile and a tail of three


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------ eval
@pytest.mark.parametrize("case", gc.CASES, ids=gc.case_id)
def test_glm_eval_bitwise_at_edge_shapes(gpu, case):
    m = gc.make_model(case.kind, case.n, case.d)
    for regime in gc.REGIMES:
        B = gc.betas(case, regime)[0]
        lp, g = m.evalallg(B)
        lp_r, g_r = orc.eval_batch(m, B)
        assert np.isfinite(lp_r).all()
        assert np.array_equal(_bits(lp), _bits(lp_r)), f"{regime}: log-target"
        assert np.array_equal(_bits(g), _bits(g_r)), f"{regime}: gradient"


# ------------------------------------------------------------------ samplers
def _sampler_cases():
    """(kind, n, d, C): the n sweep at one width per kernel family (the -1 link only where the single-slice MALA
    kernel packs its sign, probit -- the linear instantiation -- at d = 8 and 300), the C sweep at both points."""
    out = []
    for kind, ds in (("logistic", gc.SAMPLER_N_SWEEP_D), ("linear", gc.SAMPLER_N_SWEEP_D), ("logistic_neg", (8, 128)),
                     ("probit", (8, 300))):
        out += [gc.Case(kind, n, d, SWEEP_C) for d in ds for n in gc.N_SWEEP]
    out += [gc.Case(kind, n, d, C) for kind in gc.KINDS for d, n in gc.C_SWEEP_AT for C in gc.C_SWEEP]
    return out


SAMPLER_CASES = _sampler_cases()
D_SWEEP_CASES = [gc.Case(kind, n, d, SWEEP_C) for kind in ("logistic", "linear") for n in gc.D_SWEEP_N
                 for d in gc.D_SWEEP]
RAM_CASES = [gc.Case(kind, n, d, C) for kind in ("logistic", "linear") for d in (10, 64) for n in (1, 16, 17, 33)
             for C in (15, 65)]


def _seed(case):
    return 1000 + 7 * case.n + case.d + 3 * case.C


def _sampler(sname, case):
    """Step sizes in units of h = 1 / sqrt(n d), the scale of these cases' posteriors (the curvature grows with both),
    so that one table serves every shape; multipliers chosen on the oracle alone (module docstring)."""
    h = 1.0 / np.sqrt(case.n * case.d)
    return {"rwm": lambda: mc.RWM(1.5 * h), "mala": lambda: mc.MALA(0.2 * h),
            "mala_tuned": lambda: mc.MALA(0.3 * h, mc.EmpMCTuner(0.6, adaptStep=3)),
            "hmc": lambda: mc.HMC(3, 2.0 * h), "hmcda": lambda: mc.HMCDA(len=1.2 * h, step=0.3 * h),
            "ram": lambda: mc.RAM(0.1 / np.sqrt(case.d), 0.3)}[sname]()


@functools.lru_cache(maxsize=None)
def _oracle_run(case, sname):
    """The oracle's run of one case, computed once and shared (the parity test and the sweep's acceptance test)."""
    m = gc.make_model(case.kind, case.n, case.d)
    oc = orc.OracleChains(m, _sampler(sname, case), nchains=case.C, seed=_seed(case))
    s, g, acc = oc.run(mc.SerialMC(**RUNNER))
    for a in (s, g, acc):
        if a is not None:
            a.setflags(write=False)
    return s, g, acc, oc


def _check(case, sname):
    m = gc.make_model(case.kind, case.n, case.d)
    task = (m * _sampler(sname, case) * mc.SerialMC(**RUNNER)).batch(case.C, seed=_seed(case))
    chain = mc.run(task)
    if sname in ("mala", "mala_tuned") and gc.geometry(case.d)[1] == 1:
        assert task.step_kernel.startswith("glm_mala1ws"), task.step_kernel
    s_ref, g_ref, acc_ref, oc = _oracle_run(case, sname)
    assert_parity(chain, s_ref, g_ref, acc_ref, sname)
    if sname not in ("rwm", "ram"):
        assert np.array_equal(_bits(chain._gradients), _bits(g_ref)), "gradients not bit-identical"
    assert np.array_equal(_bits(chain.final_x), _bits(oc.x)) and np.array_equal(_bits(chain.final_lp), _bits(oc.lp))
    assert task.evals == int(oc.n_evals.sum())
    if sname in ("mala_tuned", "hmcda"):
        assert np.array_equal(_bits(task.tuner_state()["step"]), _bits(oc.t_step))
    return task, oc


@pytest.mark.parametrize("sname", SNAMES)
@pytest.mark.parametrize("case", SAMPLER_CASES, ids=gc.case_id)
def test_glm_samplers_at_tile_and_chain_edges(gpu, case, sname):
    _check(case, sname)


@pytest.mark.parametrize("sname", ["rwm", "hmcda"])
@pytest.mark.parametrize("case", D_SWEEP_CASES, ids=gc.case_id)
def test_glm_samplers_at_geometry_edges(gpu, case, sname):
    _check(case, sname)


@pytest.mark.parametrize("case", RAM_CASES, ids=gc.case_id)
def test_glm_ram_at_tile_and_chain_edges(gpu, case):
    """d = 10: the lane kernel (glm_ram); d = 64: the eval kernel + glm_ram_update (glm_ram_wave.hip)."""
    task, oc = _check(case, "ram")
    assert task.step_kernel.startswith("glm_ram_update<" if case.d == 64 else "glm_ram<"), task.step_kernel
    _assert_ram_factor(task, oc, case.d)


SWEEPS = {**{s: SAMPLER_CASES + (D_SWEEP_CASES if s in ("rwm", "hmcda") else []) for s in SNAMES}, "ram": RAM_CASES}


def sweep_acceptance(sname):
    acc = np.concatenate([_oracle_run(case, sname)[2].ravel() for case in SWEEPS[sname]])
    return acc.mean()


@pytest.mark.parametrize("sname", list(SWEEPS))
def test_sweep_accepts_and_rejects(gpu, sname):
    """Both outcomes occur within each sampler's sweep (the oracle's accept bits, which the parity tests hold the GPU
    to): a sweep of accepts only, or rejects only, would leave half of every step kernel's commit path unrun."""
    assert 0 < sweep_acceptance(sname) < 1
