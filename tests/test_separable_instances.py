"""Every kernel instance of the separable targets (IsoNormalDot, NormalDSL, AbsNormalDSL, DistDSL) against the
oracle, bit for bit: the step kernels lpc_* / lpp_* / wpc_* / bpc_* over the case table of separable_cases.py (each
case asserts the instance it ran), the eval kernels over the width sweep with out-of-support and special-value
columns, the storeLeaps record kernels at the wide wave and the block widths, and the runner features across the
wave -> block switch at d = 2048 | 2049.  test_separable_cpu.py holds the table's CPU checks: its step sizes make
the oracle both accept and reject in every case, so the accept path is compared here, not only the reject path."""
import numpy as np
import pytest

import mcmchip as mc
import oracle_ref as orc
import separable_cases as sc
from test_gpu_parity import _store_leaps_case

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------ step kernels
@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_step_kernel_instance_parity(gpu, c):
    """samples and gradients bit-identical to the oracle's, accept bits equal, final state and log-target equal, the
    evaluation count equal -- on the instance the table expects for the case's width, model and sampler"""
    m, C, r = sc.model(c), sc.nchains(c), sc.runner(c)
    task = (m * sc.sampler(c) * r).batch(C, seed=sc.seed(c))
    chain = mc.run(task)
    assert task.step_kernel == sc.expected_name(c)
    oc = orc.OracleChains(m, sc.sampler(c), nchains=C, seed=sc.seed(c))
    s_ref, g_ref, acc_ref = oc.run(r)
    acc = chain.diagnostics["accept"].T
    assert np.array_equal(acc, acc_ref.astype(bool)), f"accept bits differ in {np.count_nonzero(acc != acc_ref)}"
    assert 0 < acc_ref.sum() < acc_ref.size                    # both paths compared (test_separable_cpu.py)
    s = chain._samples
    assert s.shape == s_ref.shape
    assert np.array_equal(s.view(np.uint64), s_ref.view(np.uint64)), "samples not bit-identical"
    if sc.kind_of(c.sampler) != "rwm":
        assert np.array_equal(chain._gradients.view(np.uint64), g_ref.view(np.uint64)), "gradients not bit-identical"
    assert np.array_equal(chain.final_x, oc.x, equal_nan=True) and np.array_equal(chain.final_lp, oc.lp, equal_nan=True)
    assert task.evals == int(oc.n_evals.sum())


# ------------------------------------------------------------------ eval kernels
@pytest.mark.parametrize("fl", list(sc.FLAVOURS))
@pytest.mark.parametrize("d", sc.D_SWEEP)
def test_device_eval_matches_oracle(gpu, fl, d, capsys):
    """model.evalallg (lpc_eval / lpp_eval / wpc_eval / bpc_eval) against orc.eval_batch, bitwise, on in-support
    points, on columns with one coordinate out of the support at a chosen lane / slot / wave position (-Inf and an
    all-zero gradient from both), and on columns with one coordinate at the support's edge, -0.0, +-Inf, NaN or the
    smallest subnormal, where the oracle's value is the specification (printed)."""
    f = sc.FLAVOURS[fl]
    x, labels, oos = sc.eval_batch_columns(fl, d)
    m = mc.MCMCLikelihoodModel(f.target(), x[:, 0], gradient=True)
    lp, g = m.evalallg(x)
    lp_r, g_r = orc.eval_batch(m, x)
    for k in oos:
        assert lp_r[k] == -np.inf and not g_r[:, k].any(), labels[k]
        assert lp[k] == -np.inf and not g[:, k].any(), labels[k]
    assert np.all(np.isfinite(lp_r[:4]))
    bad = [labels[k] for k in range(x.shape[1])
           if not (_same_bits(lp[k:k + 1], lp_r[k:k + 1]) and _same_bits(g[:, k], g_r[:, k]))]
    with capsys.disabled():
        spec = {lb: (lp_r[k], g_r[int(lb.split("@")[1]), k]) for k, lb in enumerate(labels) if k >= 4 + len(oos)}
        print(f"\neval {fl} d={d}: " + "; ".join(f"{lb}: lp {v[0]!r} g {v[1]!r}" for lb, v in spec.items()))
    assert not bad, bad


# ------------------------------------------------------------------ storeLeaps record kernels
@pytest.mark.parametrize("sname", ["hmc", "hmcda"])
@pytest.mark.parametrize("fl", ["iso", "gamma"])
@pytest.mark.parametrize("d", [1023, 1025, 2048, 2049, 8193])
def test_store_leaps_wide_bitwise(gpu, sname, fl, d):
    """the trajectory record of every kept step from wpc_hmc_rec<4>, <8> and bpc_hmc_rec<4>, <8>
    (test_gpu_parity.py's comparison, at the widths it does not reach)"""
    c = sc.Case(fl, d, sname, fl != "iso")
    sp = sc.sampler(c, store_leaps=True)
    r = sc.runner(c)
    _store_leaps_case(sc.model(c), sp, C=5, seed=sc.seed(c), order=None, cap=sp.leaps_cap(),
                      steps=min(r.len, 12), burnin=min(r.burnin, 6), thinning=2)


# ------------------------------------------------------------------ the wave -> block switch through the runner
def _edge_task(d, sp, r, C=9, **kw):
    c = sc.Case("normal", d, "mala", True)
    return (sc.model(c) * sp * r).batch(C, seed=61 + d, **kw)


@pytest.mark.parametrize("d", [2048, 2049])
@pytest.mark.parametrize("spl", [1, 7])
def test_steps_per_launch_is_invisible_at_the_switch(gpu, spl, d):
    c = sc.Case("normal", d, "mala", True)
    r = mc.SerialMC(steps=12, burnin=2, thinning=2)
    a = mc.run(_edge_task(d, sc.sampler(c), r))
    b = mc.run(_edge_task(d, sc.sampler(c), r, steps_per_launch=spl))
    assert a.task.step_kernel == sc.expected_step_kernel(d, "NormalDSL", "mala", 9, True)
    assert np.array_equal(a._samples.view(np.uint64), b._samples.view(np.uint64))
    assert np.array_equal(a._gradients.view(np.uint64), b._gradients.view(np.uint64))
    assert np.array_equal(a.diagnostics["accept"], b.diagnostics["accept"])
    assert 0 < a.diagnostics["accept"].sum() < a.diagnostics["accept"].size


@pytest.mark.parametrize("d", [2048, 2049])
def test_continuation_is_invisible_at_the_switch(gpu, d):
    """run(chain) continues the same chains: two runs of 6 steps are one run of 12"""
    c = sc.Case("normal", d, "hmc", True)
    full = mc.run(_edge_task(d, sc.sampler(c), mc.SerialMC(steps=12)))
    c1 = mc.run(_edge_task(d, sc.sampler(c), mc.SerialMC(steps=6)))
    c2 = mc.run(c1)
    assert np.array_equal(np.concatenate([c1._samples, c2._samples]).view(np.uint64), full._samples.view(np.uint64))
    assert np.array_equal(np.concatenate([c1.diagnostics["accept"], c2.diagnostics["accept"]], axis=1),
                          full.diagnostics["accept"])
    assert np.array_equal(c2.final_x, full.final_x) and np.array_equal(c2.final_lp, full.final_lp)
    assert 0 < full.diagnostics["accept"].sum() < full.diagnostics["accept"].size


@pytest.mark.parametrize("d", [2048, 2049])
def test_chain_offset_sharding_is_invisible_at_the_switch(gpu, d):
    c = sc.Case("normal", d, "hmc", True)
    r = mc.SerialMC(steps=8, burnin=2)
    full = mc.run(_edge_task(d, sc.sampler(c), r, C=9))
    lo = mc.run(_edge_task(d, sc.sampler(c), r, C=5, chain_offset=0))
    hi = mc.run(_edge_task(d, sc.sampler(c), r, C=4, chain_offset=5))
    assert np.array_equal(np.concatenate([lo._samples, hi._samples], axis=2).view(np.uint64),
                          full._samples.view(np.uint64))
    assert np.array_equal(np.concatenate([lo.diagnostics["accept"], hi.diagnostics["accept"]]),
                          full.diagnostics["accept"])
    assert 0 < full.diagnostics["accept"].sum() < full.diagnostics["accept"].size
