"""The slice-sampling kernels against the checker (slice_oracle.c), bit for bit, on every case of slice_cases.py; the
device-output path; the reported kernel instance; and the device statistics on the returned device samples."""
import numpy as np
import pytest

import mcmchip as mc
from mcmchip import _lib
import slice_cases as sc

pytestmark = pytest.mark.gpu


def run_gpu(case, on_device=False, **over):
    m, init, w, kw = sc.case_args(case)
    kw = dict(kw, **over)
    return mc.slice_sample(m, kw["niter"], initial=init, widths=w, step_out=kw["step_out"], burnin=kw["burnin"],
                           nchains=init.shape[1], seed=kw["seed"], chain_offset=kw["chain_offset"],
                           iter_begin=kw["iter_begin"], max_evals=kw["max_evals"], on_device=on_device)


def assert_equals_checker(ch, res):
    assert np.array_equal(sc.bits(ch._samples), sc.bits(res.samples))
    assert np.array_equal(sc.bits(ch.final_x), sc.bits(res.final_x))
    assert np.array_equal(sc.bits(ch.final_lp), sc.bits(res.final_lp))
    assert np.array_equal(ch.diagnostics["info"], res.info)
    assert ch.diagnostics["evals"] == res.evals


@pytest.mark.parametrize("case", sc.CASES, ids=[c.id for c in sc.CASES])
def test_kernels_equal_the_checker(gpu, case):
    if case.out_of_support:
        with pytest.raises(mc.OutOfSupportError, match="Initial values out of model support"):
            run_gpu(case)
        return
    ch = run_gpu(case)
    res = sc.checker_result(case)
    assert_equals_checker(ch, res)
    m, init, _, kw = sc.case_args(case)
    assert mc.slice_last_kernel() == mc.slice_plan(m, case.C)[0]                # the reported instance is the plan's
    assert ch.range == range(kw["burnin"] + 1, kw["burnin"] + kw["niter"] + 1)
    assert ch.samples.shape == (case.C, kw["niter"], m.size) and np.isnan(ch.gradients).all()
    if case.starved:
        assert (ch.diagnostics["info"] == 1).all() and np.isnan(ch._samples).all()
        assert np.array_equal(sc.bits(ch.final_x), sc.bits(init))


@pytest.mark.parametrize("cid", ["iso3", "iso17", "iso32", "beta23", "ou60", "iso3-starved"])
def test_device_outputs_equal_host_outputs(gpu, cid):
    case = sc.BY_ID[cid]
    dev = run_gpu(case, on_device=True)
    res = sc.checker_result(case)
    assert np.array_equal(sc.bits(dev._samples.cpu().numpy()), sc.bits(res.samples))
    assert np.array_equal(sc.bits(dev.final_x.cpu().numpy()), sc.bits(res.final_x))
    assert np.array_equal(sc.bits(dev.final_lp.cpu().numpy()), sc.bits(res.final_lp))
    assert np.array_equal(dev.diagnostics["info"].cpu().numpy(), res.info)
    assert dev.diagnostics["evals"] == res.evals


@pytest.mark.parametrize("cid", ["iso3", "iso17", "beta23"])
def test_split_run_on_the_device(gpu, cid):
    """8 iterations as 5 + 3 through the library, against the checker's run of 8"""
    case = sc.BY_ID[cid]
    m, init, w, kw = sc.case_args(case)
    whole = sc.run_checker(m, init, w, **dict(kw, burnin=0, niter=8))
    a = run_gpu(case, burnin=0, niter=5)
    b = mc.slice_sample(m, 3, initial=a.final_x, widths=w, nchains=case.C, seed=kw["seed"],
                        chain_offset=kw["chain_offset"], iter_begin=5)
    assert np.array_equal(sc.bits(np.concatenate([a._samples, b._samples])), sc.bits(whole.samples))
    assert np.array_equal(sc.bits(b.final_x), sc.bits(whole.final_x))
    assert np.array_equal(sc.bits(b.final_lp), sc.bits(whole.final_lp))


def test_split_chains_on_the_device(gpu):
    """130 chains as two calls of 70 + 60"""
    case = sc.BY_ID["iso17-130-offset-init"]
    m, init, w, kw = sc.case_args(case)
    res = sc.checker_result(case)
    parts = [mc.slice_sample(m, kw["niter"], initial=init[:, lo:hi], widths=w, burnin=kw["burnin"], nchains=hi - lo,
                             seed=kw["seed"], chain_offset=kw["chain_offset"] + lo) for lo, hi in ((0, 70), (70, 130))]
    assert np.array_equal(sc.bits(np.concatenate([p._samples for p in parts], axis=2)), sc.bits(res.samples))
    assert sum(p.diagnostics["evals"] for p in parts) == res.evals


def test_defaults_and_univariate_shape(gpu):
    m = mc.model(mc.DistDSL("Normal", 3.0, 1.0), init=np.array([42.0]))        # the header comment's example
    ch = mc.slice_sample(m, 30, 42.0, seed=1)
    assert ch.samples.shape == (30,) and ch._samples.shape == (30, 1, 1)
    res = sc.run_checker(m, np.array([[42.0]]), np.ones(1), niter=30, burnin=0)
    assert np.array_equal(sc.bits(ch.samples), sc.bits(res.samples[:, 0, 0]))
    ch2 = mc.slice_sample(m, 30, seed=1)                                       # initial None: model.init
    assert np.array_equal(sc.bits(ch2._samples), sc.bits(res.samples))
    with pytest.raises(_lib.MCMCError, match="widths\\[0\\] should be finite and > 0"):
        mc.slice_sample(m, 5, widths=[0.0], seed=1)
    reg = mc.model(mc.LinearRegression(np.ones((4, 2)), np.ones(4)), init=np.zeros(2))
    with pytest.raises(_lib.MCMCError, match="not built for the regression models") as e:
        mc.slice_sample(reg, 5, seed=1)
    assert e.value.code == _lib.MCMC_E_UNSUPPORTED
    with pytest.raises(_lib.MCMCError, match="built for d <= 32"):
        mc.slice_sample(mc.model(mc.IsoNormalDot(), init=np.ones(33)), 5, seed=1)


def test_device_statistics_read_the_samples_in_place(gpu):
    """stats.describe_device and stats.ess_device on the returned device samples equal their numpy twins on the host
    copy, under the tolerances test_describe_gpu.py and test_ess_device.py use"""
    m = mc.model(mc.NormalDSL(1.0, 2.0), init=np.full(3, 0.5))
    dev = mc.slice_sample(m, 400, widths=[4.0] * 3, burnin=20, nchains=96, seed=3, on_device=True)
    host = mc.slice_sample(m, 400, widths=[4.0] * 3, burnin=20, nchains=96, seed=3)
    assert np.array_equal(sc.bits(dev._samples.cpu().numpy()), sc.bits(host._samples))
    e_dev = mc.stats.ess_device(dev._samples).cpu().numpy()                    # [d][C]
    assert np.allclose(e_dev.T, mc.stats.ess(host), rtol=1e-9)
    r_dev, r_host = dev.describe(), mc.stats.describe(host)
    assert np.allclose(r_dev.table(), r_host.table(), rtol=1e-9, atol=0)
