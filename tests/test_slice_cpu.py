"""The slice sampler without a GPU: the checker (slice_oracle.c) against the literal transcription of slice_sample.jl
(slice_ref.py) on every case of slice_cases.py, the checker's census of paths, the neutrality of splitting a run or the
chains, the launch plan's walk under the sanitizers, and the C ABI's host-side answers."""
import ctypes as ct
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mcmchip as mc
from mcmchip import _lib
import slice_cases as sc
import slice_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_CHAINS = 3        # chains of a case the transcription runs (the first, one inside, the last): chains are independent
REF_MAX_ITERS = 24    # ... and the iterations of a long case (a prefix run is a run: the draws are keyed by iteration)


@pytest.mark.parametrize("case", sc.CASES, ids=[c.id for c in sc.CASES])
def test_checker_equals_the_transcription(case):
    m, init, w, kw = sc.case_args(case)
    if case.out_of_support:
        assert sc.run_checker(m, init, w, **kw).rc == _lib.MCMC_E_INIT_OUT_OF_SUPPORT
        assert not np.isfinite(slice_ref.LogDist(m, 1)(init[:, case.C - 1], budget=False))
        return
    if kw["burnin"] + kw["niter"] > REF_MAX_ITERS:
        kw = dict(kw, burnin=REF_MAX_ITERS - kw["niter"])
        res = sc.run_checker(m, init, w, **kw)
    else:
        res = sc.checker_result(case)
    assert res.rc == 0
    C = case.C
    for c in sorted({0, C // 2, C - 1})[:REF_CHAINS]:
        hist, state, lp, info, evals = slice_ref.slice_sample_chain(
            m, init[:, c], kw["niter"], w, step_out=kw["step_out"], burnin=kw["burnin"], seed=kw["seed"],
            chain=kw["chain_offset"] + c, iter_begin=kw["iter_begin"], max_evals=kw["max_evals"] or sc.DEFAULT_EVALS)
        assert np.array_equal(sc.bits(res.samples[:, :, c]), sc.bits(hist)), (case.id, c)
        assert np.array_equal(sc.bits(res.final_x[:, c]), sc.bits(state))
        assert sc.bits(res.final_lp[c:c + 1])[0] == sc.bits(np.array([lp]))[0]
        assert res.info[c] == info
    # evaluations: the chains' totals add up (one chain alone, then all)
    one = sc.run_checker(m, init[:, :1], w, **kw)
    assert one.evals == slice_ref.slice_sample_chain(
        m, init[:, 0], kw["niter"], w, step_out=kw["step_out"], burnin=kw["burnin"], seed=kw["seed"],
        chain=kw["chain_offset"], iter_begin=kw["iter_begin"], max_evals=kw["max_evals"] or sc.DEFAULT_EVALS)[4]


def test_census_shows_every_path():
    tot = {k: 0 for k in sc.CENSUS}
    for case in sc.ORDINARY:
        res = sc.checker_result(case)
        assert res.rc == 0 and not res.info.any(), case.id
        assert np.isfinite(res.samples).all()
        for k, v in res.census.items():
            tot[k] = max(tot[k], v) if k == "max_evals" else tot[k] + v
        # no ordinary case spends more than a quarter of the default budget on one update
        assert res.census["max_evals"] <= sc.DEFAULT_EVALS // 4, (case.id, res.census)
    for k in ("left0", "left1", "right0", "right1", "shrink_left", "shrink_right", "first_accept", "neg_inf"):
        assert tot[k] > 0, (k, tot)
    assert tot["stopped"] == 0
    # the bounded-support targets end their step-out at the edge on an evaluation of -Inf
    for cid in ("uniform01", "exponential2", "beta23", "ou60"):
        assert sc.checker_result(sc.BY_ID[cid]).census["neg_inf"] > 0, cid
    assert sc.checker_result(sc.BY_ID["iso3-narrow"]).census["left1"] > sc.checker_result(sc.BY_ID["iso3"]).census["left1"]
    ns = sc.checker_result(sc.BY_ID["iso3-no-step-out"]).census
    assert ns["left0"] == ns["left1"] == ns["right0"] == ns["right1"] == 0 and ns["shrink_left"] + ns["shrink_right"] > 0


def test_starved_case_is_a_defined_path():
    case = sc.BY_ID["iso3-starved"]
    m, init, w, kw = sc.case_args(case)
    res = sc.checker_result(case)
    assert res.rc == 0 and (res.info == 1).all() and np.isnan(res.samples).all()
    assert np.array_equal(sc.bits(res.final_x), sc.bits(init))
    assert res.census["stopped"] == case.C and res.census["max_evals"] == 3
    assert res.evals == case.C * (1 + 3)


@pytest.mark.parametrize("cid", ["iso3", "iso17", "beta23", "ou60"])
def test_splitting_a_run_is_neutral(cid):
    """8 iterations as 5 + 3: the second run starts at iter_begin = 5 from the first run's final_x"""
    m, init, w, kw = sc.case_args(sc.BY_ID[cid])
    kw = dict(kw, burnin=0, niter=8)
    whole = sc.run_checker(m, init, w, **kw)
    a = sc.run_checker(m, init, w, **dict(kw, niter=5))
    b = sc.run_checker(m, a.final_x, w, **dict(kw, niter=3, iter_begin=5))
    assert np.array_equal(sc.bits(whole.samples), sc.bits(np.concatenate([a.samples, b.samples])))
    assert np.array_equal(sc.bits(whole.final_x), sc.bits(b.final_x))
    assert np.array_equal(sc.bits(whole.final_lp), sc.bits(b.final_lp))
    assert whole.evals == a.evals + b.evals - init.shape[1]          # the second run evaluates its starts again


@pytest.mark.parametrize("cid", ["iso3-130-offset-init", "iso17-130-offset-init"])
def test_splitting_the_chains_is_neutral(cid):
    """130 chains as two calls of 70 + 60"""
    m, init, w, kw = sc.case_args(sc.BY_ID[cid])
    whole = sc.checker_result(sc.BY_ID[cid])
    a = sc.run_checker(m, init[:, :70], w, **kw)
    b = sc.run_checker(m, init[:, 70:], w, **dict(kw, chain_offset=kw["chain_offset"] + 70))
    assert np.array_equal(sc.bits(whole.samples), sc.bits(np.concatenate([a.samples, b.samples], axis=2)))
    assert np.array_equal(sc.bits(whole.final_x), sc.bits(np.concatenate([a.final_x, b.final_x], axis=1)))
    assert whole.evals == a.evals + b.evals


# ------------------------------------------------------------------ the launch plan
def _expected_name(model, d):
    nb = -(-d // 4)
    return f"lpc_slice<{nb}, {model}>" if d <= 16 else f"lpp_slice<{-(-nb // 2)}, {model}>"


def test_plan_walk_under_the_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "slice_plan_check")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "slice_plan_check.cpp")], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    rows = [ln.split(" ", 8) for ln in r.stdout.splitlines() if ln.startswith("slice ")]
    assert len(rows) == 6 * 40 * 8 and f"{len(rows)} slice plans" in r.stdout
    assert "0 plans built outside the family" in r.stdout
    joint = {"DistObsDSL", "OUDSL"}
    for _, model, d, C, built, grid, threads, cpb, name in rows:
        d, C, built, grid, threads, cpb = int(d), int(C), int(built), int(grid), int(threads), int(cpb)
        assert built == (d <= (4 if model in joint else 32)), (model, d)
        if built:
            assert name == _expected_name(model, d) and threads == 256 and cpb == (256 if d <= 16 else 128)
            assert grid * cpb >= C > (grid - 1) * cpb


def test_plan_call_agrees_with_the_rule():
    lib = _lib.load()
    buf = ct.create_string_buffer(128)
    th, grid = ct.c_int32(0), ct.c_int64(0)
    for kind, model in ((_lib.MODEL_ISO_NORMAL_DOT, "IsoDot"), (_lib.MODEL_NORMAL_DSL, "NormalDSL"),
                        (_lib.MODEL_ABS_NORMAL_DSL, "AbsNormalDSL"), (_lib.MODEL_DIST_DSL, "DistDSL")):
        for d in (1, 3, 4, 5, 16, 17, 24, 25, 32):
            for C in (1, 65, 130, 1 << 18):
                assert lib.mcmc_slice_plan(kind, d, C, buf, 128, ct.byref(th), ct.byref(grid)) == 0
                cpb = 256 if d <= 16 else 128
                assert (buf.value.decode(), th.value, grid.value) == (_expected_name(model, d), 256, -(-C // cpb))
    assert lib.mcmc_slice_plan(_lib.MODEL_OU, 3, 64, None, 0, None, None) == 0
    m = mc.model(mc.IsoNormalDot(), init=np.ones(24))
    assert mc.slice_plan(m, 130) == ("lpp_slice<3, IsoDot>", 256, 2)


# ------------------------------------------------------------------ the C ABI's host-side answers
def _validate(**kw):
    c = _lib.SliceCfg()
    base = dict(niter=10, burnin=0, iter_begin=0, step_out=1, max_evals=0)
    base.update(kw)
    for k, v in base.items():
        setattr(c, k, v)
    lib = _lib.load()
    rc = lib.mcmc_slice_validate(ct.byref(c))
    return rc, lib.mcmc_last_error().decode()


def test_validate_messages():
    assert _validate()[0] == 0
    assert _validate(max_evals=3)[0] == 0 and _validate(max_evals=1 << 20)[0] == 0
    assert _validate(niter=0) == (_lib.MCMC_E_INVALID_ARG, "niter (0) should be > 0")
    assert _validate(burnin=-1) == (_lib.MCMC_E_INVALID_ARG, "burnin (-1) should be >= 0")
    assert _validate(iter_begin=-2) == (_lib.MCMC_E_INVALID_ARG, "iter_begin (-2) should be >= 0")
    for kw in (dict(niter=1 << 32), dict(niter=1 << 31, burnin=1 << 30, iter_begin=1 << 30),
               dict(iter_begin=(1 << 32) - 10)):
        assert _validate(**kw) == (_lib.MCMC_E_INVALID_ARG, "iter_begin + burnin + niter should be < 2^32")
    assert _validate(niter=(1 << 32) - 1)[0] == 0
    for bad in (1, 2, -1, (1 << 20) + 1):
        rc, msg = _validate(max_evals=bad)
        assert rc == _lib.MCMC_E_INVALID_ARG and msg.startswith(f"max_evals ({bad}) should be in 3 .. 2^20")
    assert _lib.load().mcmc_slice_validate(None) == _lib.MCMC_E_INVALID_ARG
    with pytest.raises(_lib.MCMCError, match="niter"):
        mc.slice_sample(mc.model(mc.IsoNormalDot(), init=np.ones(3)), 0)


def test_null_handling_and_refusals():
    lib = _lib.load()
    c = _lib.SliceCfg()
    c.niter, c.step_out = 4, 1
    assert lib.mcmc_run_slice(None, ct.byref(c), 1, 0, 1, None, None, 0, None, None, None, None, None, None,
                              None) == _lib.MCMC_E_INVALID_ARG
    assert lib.mcmc_last_error().decode() == "NULL argument"
    assert lib.mcmc_slice_last_kernel(None, 0) == _lib.MCMC_E_INVALID_ARG
    for kind in (_lib.MODEL_LOGISTIC, _lib.MODEL_LINEAR, _lib.MODEL_PROBIT):
        assert lib.mcmc_slice_plan(kind, 5, 64, None, 0, None, None) == _lib.MCMC_E_UNSUPPORTED
        assert lib.mcmc_last_error().decode().startswith("slice_sample is not built for the regression models")
    assert lib.mcmc_slice_plan(_lib.MODEL_ISO_NORMAL_DOT, 33, 64, None, 0, None, None) == _lib.MCMC_E_UNSUPPORTED
    assert lib.mcmc_last_error().decode() == "slice_sample is built for d <= 32 (d = 33)"
    assert lib.mcmc_slice_plan(_lib.MODEL_OU, 5, 64, None, 0, None, None) == _lib.MCMC_E_UNSUPPORTED
    assert lib.mcmc_slice_plan(10, 3, 64, None, 0, None, None) == _lib.MCMC_E_UNSUPPORTED
    assert lib.mcmc_last_error().decode() == "slice_sample: unknown model kind"
    assert lib.mcmc_slice_plan(_lib.MODEL_ISO_NORMAL_DOT, 0, 64, None, 0, None, None) == _lib.MCMC_E_INVALID_ARG
    assert lib.mcmc_slice_plan(_lib.MODEL_ISO_NORMAL_DOT, 3, 0, None, 0, None, None) == _lib.MCMC_E_INVALID_ARG


def test_struct_and_bindings():
    assert ct.sizeof(_lib.SliceCfg) == 8 + 8 + 8 + 4 + 4 + 8                   # step_out: int32 + pad
    header = open(os.path.join(ROOT, "include", "mcmc_hip.h")).read()
    for sym in ("mcmc_slice_validate", "mcmc_run_slice", "mcmc_slice_plan", "mcmc_slice_last_kernel"):
        assert sym in header and sym in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), sym)
    jl = open(os.path.join(ROOT, "mcmc.jl_amd", "julia", "MCMCHip.jl")).read()
    for needle in ("struct SliceCfg", "niter::Int64", "burnin::Int64", "iter_begin::Int64", "step_out::Int32",
                   "max_evals::Int64", ":mcmc_slice_validate", ":mcmc_run_slice",
                   "function slice_sample(model, initial, niter; widths = nothing, step_out = true, burnin = 0, "
                   "nchains = 1, seed = 1"):
        assert needle in jl, needle
    assert "slice_sample" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
