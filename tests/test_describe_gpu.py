"""mcmc_stats_describe on the device (kernels/describe.hip) against the checker (tests/describe_oracle.c), bit for bit,
NaN positions included: the per-chain table over both sides of every size-class edge, the pooled rows in the documented
reduction order, the exact pooled quantiles of the radix select.  test_describe_cpu.py checks the checker itself."""
import numpy as np
import pytest

import mcmchip as mc
import describe_ref as dr
import ess_cases as ec

pytestmark = pytest.mark.gpu

SERIES_KEYS = [("series", n, d, C) for n, d, C in dr.series_shapes()] + [("poison", 96), ("poison", 618),
                                                                        ("poison", 619), ("stuck",)]
SERIES_KEYS += list(dr.POOL_KEYS)                          # several pool blocks and many histogram blocks merging
_ids = lambda k: "-".join(map(str, k))
_device_results = {}


def _chain(x):
    ch = type("Chain", (), {})()
    ch._samples = x
    return ch


def _device(key):
    """describe_device of the batch through the host-pointer path, in the checker's layout: one launch a batch"""
    if key not in _device_results:
        r = mc.stats.describe_device(_chain(dr.batch(key)), probs=dr.PROBS)
        per = np.ascontiguousarray(r.per_chain.transpose(2, 1, 0))                     # [6][d][C]
        pooled = np.concatenate([np.stack([r.pooled[nm] for nm in r.rows]), r.quantiles])
        _device_results[key] = (per, pooled, r.nbad)
    return _device_results[key]


def _same(got, ref):
    return ec.same_bits_or_nan(got, ref) and np.array_equal(np.isnan(got), np.isnan(ref))


def _diff(got, ref):
    bad = np.argwhere(~((got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))))
    return [(tuple(int(i) for i in ix), float(got[tuple(ix)]), float(ref[tuple(ix)])) for ix in bad[:8]]


@pytest.mark.parametrize("key", SERIES_KEYS, ids=_ids)
def test_tables_match_the_checker(gpu, key):
    """the whole per-chain table, every pooled row, the seven quantiles and nbad"""
    per_ref, pooled_ref, nbad_ref = dr.reference(key)
    per, pooled, nbad = _device(key)
    assert _same(per, per_ref), _diff(per, per_ref)
    assert _same(pooled, pooled_ref), _diff(pooled, pooled_ref)
    assert np.array_equal(nbad, nbad_ref)


@pytest.mark.parametrize("key", SERIES_KEYS, ids=_ids)
def test_ess_column_is_mcmc_stats_ess(gpu, key):
    x = dr.batch(key)
    e = mc.stats.ess_device(_chain(x), "imse")                                         # [C][d]
    per, _, _ = _device(key)
    assert _same(per[4], np.ascontiguousarray(e.T)), _diff(per[4], np.ascontiguousarray(e.T))


def test_stuck_chains_and_constant_parameter(gpu):
    _, pooled, nbad = _device(("stuck",))
    assert nbad.tolist() == [len(dr.STUCK), dr.batch(("stuck",)).shape[2]]
    assert np.isnan(pooled[5, 1]) and np.isfinite(pooled[5, 0])


def test_one_chain_has_no_rhat(gpu):
    _, pooled, _ = _device(("series", 90, 1, 1))
    assert np.isnan(pooled[5]).all() and np.isfinite(pooled[:3]).all()


@pytest.mark.parametrize("key", [("series", 90, 3, 65), ("series", 97, 3, 200), ("series", 619, 1, 64),
                                 ("poison", 96), ("pool", 5, 2, 9000)], ids=_ids)
def test_device_pointers_and_optional_tables(gpu, key):
    """a device tensor in, device tensors out; per_chain alone, pooled alone: each what the full call gives"""
    import torch
    per_ref, pooled_ref, nbad_ref = dr.reference(key)
    xt = torch.from_numpy(dr.batch(key).copy()).cuda()
    r = mc.stats.describe_device(xt, probs=dr.PROBS)
    assert r.per_chain.is_cuda and r.quantiles.is_cuda and r.nbad.is_cuda
    assert _same(r.per_chain.cpu().numpy(), per_ref)
    got = np.concatenate([np.stack([r.pooled[nm].cpu().numpy() for nm in r.rows]), r.quantiles.cpu().numpy()])
    assert _same(got, pooled_ref), _diff(got, pooled_ref)
    assert np.array_equal(r.nbad.cpu().numpy(), nbad_ref)
    assert _same(np.ascontiguousarray(r.column("ess").cpu().numpy().T), per_ref[4])
    assert _same(np.ascontiguousarray(r.table().transpose(2, 1, 0)), per_ref)
    only_per = mc.stats.describe_device(xt, probs=dr.PROBS, pooled=False)
    assert only_per.pooled is None and only_per.quantiles is None and _same(only_per.per_chain.cpu().numpy(), per_ref)
    only_pooled = mc.stats.describe_device(xt, probs=dr.PROBS, per_chain=False)
    got = np.concatenate([np.stack([only_pooled.pooled[nm].cpu().numpy() for nm in only_pooled.rows]),
                          only_pooled.quantiles.cpu().numpy()])
    assert only_pooled.per_chain is None and _same(got, pooled_ref), _diff(got, pooled_ref)
    assert np.array_equal(only_pooled.nbad.cpu().numpy(), nbad_ref)


@pytest.mark.parametrize("n,d,C,maxlag", dr.MAXLAG_CASES)
def test_maxlag_below_the_default(gpu, n, d, C, maxlag):
    """k_desc_reg, k_desc_tile, k_desc_col with the scan capped at pair floor((maxlag - 1) / 2), even and odd maxlag;
    the cap changes the table (some series run to it), and the ess column is still mcmc_stats_ess's"""
    x = dr.batch(("series", n, d, C))
    per_ref, pooled_ref, nbad_ref = dr.describe(x, maxlag=maxlag)
    assert not _same(per_ref[4], dr.reference(("series", n, d, C))[0][4])
    r = mc.stats.describe_device(_chain(x), probs=dr.PROBS, maxlag=maxlag)
    per = np.ascontiguousarray(r.per_chain.transpose(2, 1, 0))
    pooled = np.concatenate([np.stack([r.pooled[nm] for nm in r.rows]), r.quantiles])
    assert _same(per, per_ref), _diff(per, per_ref)
    assert _same(pooled, pooled_ref), _diff(pooled, pooled_ref)
    assert np.array_equal(r.nbad, nbad_ref)
    e = mc.stats.ess_device(_chain(x), "imse", maxlag=maxlag)
    assert _same(per[4], np.ascontiguousarray(e.T))


def test_kept_samples_of_a_short_rwm_run(gpu):
    """real kept samples: runs of repeated values wherever a proposal was rejected"""
    m = mc.model(mc.IsoNormalDot(), init=np.ones(3))
    ch = mc.run((m * mc.RWM(0.8) * mc.SerialMC(steps=300, burnin=30, thinning=3)).batch(130, seed=5))
    x = np.ascontiguousarray(ch._samples)
    assert (np.diff(x, axis=0) == 0).any()
    per_ref, pooled_ref, nbad_ref = dr.describe(x)
    r = ch.describe(probs=dr.PROBS) if hasattr(ch._samples, "data_ptr") else mc.stats.describe_device(ch, probs=dr.PROBS)
    per = np.ascontiguousarray(r.per_chain.transpose(2, 1, 0))
    pooled = np.concatenate([np.stack([r.pooled[nm] for nm in r.rows]), r.quantiles])
    assert _same(per, per_ref), _diff(per, per_ref)
    assert _same(pooled, pooled_ref), _diff(pooled, pooled_ref)
    assert np.array_equal(r.nbad, nbad_ref)


@pytest.mark.parametrize("name", dr.QUANT_CASES)
def test_quantiles_match_the_checker(gpu, name):
    key = ("quant", name)
    per_ref, pooled_ref, nbad_ref = dr.reference(key)
    per, pooled, nbad = _device(key)
    assert _same(pooled[dr.NPOOLED:], pooled_ref[dr.NPOOLED:]), _diff(pooled[dr.NPOOLED:], pooled_ref[dr.NPOOLED:])
    assert _same(pooled, pooled_ref), _diff(pooled, pooled_ref)
    assert _same(per, per_ref) and np.array_equal(nbad, nbad_ref)


def test_quantiles_repeated_probability_and_none(gpu):
    x = dr.batch(("quant", "ties"))
    _, ref, _ = dr.describe(x, probs=(0.5, 0.5, 0.1))
    r = mc.stats.describe_device(_chain(x), probs=(0.5, 0.5, 0.1))
    assert _same(r.quantiles, ref[dr.NPOOLED:]) and ec.same_bits(r.quantiles[0], r.quantiles[1])
    r0 = mc.stats.describe_device(_chain(x), probs=())
    assert r0.quantiles.shape == (0, x.shape[1])
    assert _same(np.stack([r0.pooled[nm] for nm in r0.rows]), ref[:dr.NPOOLED])


def test_nan_samples_neither_fault_nor_loop(gpu):
    """NaN samples sort above +Inf; the value is not promised, the call returns and the other parameter is exact"""
    x = dr.batch(("quant", "signs")).copy()
    x[::3, 0, ::5] = np.nan
    x[1, 0, 7] = -np.nan
    _, ref, _ = dr.describe(x)
    r = mc.stats.describe_device(_chain(x), probs=dr.PROBS)
    assert _same(np.ascontiguousarray(r.quantiles[:, 1:]), np.ascontiguousarray(ref[dr.NPOOLED:, 1:]))
    assert r.quantiles.shape == (len(dr.PROBS), x.shape[1])


def test_refusals_launch_nothing(gpu):
    import torch
    from mcmchip import _lib
    x = torch.zeros((10, 2, 33), dtype=torch.float64).cuda()
    with pytest.raises(mc.MCMCError, match="nprobs = 9") as ei:
        mc.stats.describe_device(x, probs=(0.5,) * 9)
    assert ei.value.code == _lib.MCMC_E_INVALID_ARG
    with pytest.raises(mc.MCMCError, match=r"is not in \[0, 1\]"):
        mc.stats.describe_device(x, probs=(1.5,))
    with pytest.raises(mc.MCMCError, match="maxlag should be < nkept"):
        mc.stats.describe_device(x, maxlag=10)
