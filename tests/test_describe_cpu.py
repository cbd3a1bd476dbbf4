"""describe on the CPU: the checker (tests/describe_oracle.c) against the literal numpy twin (stats.describe) and plain
numpy pooled computations, the quantile rule bit for bit on np.sort, the census of left-out chains, and the C ABI's
refusals (which need no GPU).  test_describe_gpu.py compares the device tables with the checker bit for bit."""
import io
import os
import re

import numpy as np
import pytest

import mcmchip as mc
from mcmchip import _lib
import describe_ref as dr
import ess_cases as ec
import oracle_ref as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-10                                                   # the project's standing bound for twin-vs-oracle

CPU_KEYS = [("series", 90, 3, 65), ("series", 97, 1, 63), ("series", 619, 1, 64), ("series", 2, 3, 200),
            ("series", 3, 1, 1), ("stuck",), ("pool", 5, 2, 9000), ("pool", 8, 1, 12289)]


def _worst(a, b):
    """largest relative deviation over the entries where both are finite; the finite masks must agree"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fa, fb = np.isfinite(a), np.isfinite(b)
    assert np.array_equal(fa, fb), "finite masks differ"
    if not fa.any():
        return 0.0
    den = np.maximum(np.abs(b[fb]), 1e-300)
    return float(np.max(np.abs(a[fa] - b[fb]) / den))


# n = 2 stays out of the twin comparison: there the IMSE variance is (-acv0 + 2 (acv0 + acv1)) / n with
# acv1 = -acv0 / 2, an exact zero in real arithmetic, so its computed value is rounding alone and no relative bound
# applies (the exactness tests below and the GPU tests keep that shape)
# The many-chain batches (n = 5..8) stay out too: for several families the variance of so short a series is again a
# near-exact cancellation.  Their business is the reduction over chains, which the plain-numpy test below checks from
# the checker's own per-chain columns.
TWIN_KEYS = [k for k in CPU_KEYS if k[0] == "stuck" or (k[0] == "series" and k[1] > 2)] + [("series", 96, 1, 65),
                                                                                         ("series", 3, 3, 65)]


@pytest.mark.parametrize("key", TWIN_KEYS, ids=lambda k: "-".join(map(str, k)))
def test_checker_agrees_with_the_numpy_twin(key):
    x = dr.batch(key)
    n, d, C = x.shape
    per, pooled, nbad = dr.reference(key)
    twin = mc.stats.describe(np.transpose(x, (2, 0, 1)), io=None if C > 1 else io.StringIO(), probs=dr.PROBS)
    worst = {}
    for i, nm in enumerate(mc.stats.Describe.columns):
        worst[nm] = _worst(twin.per_chain[:, :, i].T, per[i])
    for i, nm in enumerate(mc.stats.Describe.rows):
        worst["pooled " + nm] = _worst(twin.pooled[nm], pooled[i])
    worst["quantiles"] = _worst(twin.quantiles, pooled[dr.NPOOLED:])
    print("worst relative deviation, checker vs numpy twin:", key, worst)
    assert max(worst.values()) <= REL, worst
    assert np.array_equal(twin.nbad, nbad)


@pytest.mark.parametrize("key", CPU_KEYS, ids=lambda k: "-".join(map(str, k)))
def test_checker_pooled_rows_against_plain_numpy(key):
    x = dr.batch(key)
    n, d, C = x.shape
    per, pooled, nbad = dr.reference(key)
    flat = np.transpose(x, (1, 0, 2)).reshape(d, n * C)
    with np.errstate(all="ignore"):
        means = x.mean(axis=0)                                # [d][C]
        W = np.var(x, axis=0, ddof=1).mean(axis=1)
        rhat = np.sqrt(((n - 1) / n * W + np.var(means, axis=1, ddof=1)) / W) if C > 1 else np.full(d, np.nan)
        rhat = np.where(W == 0, np.nan, rhat)
        # mcerror and ess from the checker's own per-chain columns, summed by numpy (pairwise, another order)
        v, e = per[3] * per[3], per[4]
        good = np.isfinite(v) & np.isfinite(e) & (v > 0)
        mcerr = np.sqrt(np.where(good, v, 0.0).sum(axis=1)) / good.sum(axis=1)
        esum = np.where(good, e, 0.0).sum(axis=1)
    assert np.array_equal(nbad, (~good).sum(axis=1))
    worst = {"min": _worst(pooled[0], flat.min(axis=1) + 0.0), "mean": _worst(pooled[1], means.mean(axis=1)),
             "max": _worst(pooled[2], flat.max(axis=1) + 0.0), "rhat": _worst(pooled[5], rhat),
             "mcerror": _worst(pooled[3], mcerr), "ess": _worst(pooled[4], esum)}
    print("worst relative deviation, checker vs plain numpy:", key, worst)
    assert max(worst.values()) <= REL, worst


@pytest.mark.parametrize("key", CPU_KEYS, ids=lambda k: "-".join(map(str, k)))
def test_checker_ess_fields_are_orc_ess_exactly(key):
    """mean, mcerror, ess, actime from orc_ess's own outputs, bit for bit (min and max from numpy)"""
    x = dr.batch(key)
    n = x.shape[0]
    per, _, _ = dr.reference(key)
    e, v = orc.ess(x, 1, n - 1, 0)
    with np.errstate(all="ignore"):
        assert ec.same_bits_or_nan(per[4], e)
        assert ec.same_bits_or_nan(per[3], np.sqrt(v))
        variid = np.var(x, axis=0, ddof=1) / n                # orc_ess does not return it: actime within the bound
        assert _worst(per[5], v / variid) <= REL
        assert _worst(per[1], x.mean(axis=0)) <= REL
    assert ec.same_bits(per[0], x.min(axis=0) + 0.0) and ec.same_bits(per[2], x.max(axis=0) + 0.0)


@pytest.mark.parametrize("name", dr.QUANT_CASES)
def test_checker_quantiles_are_the_rule_on_sorted_values(name):
    x = dr.batch(("quant", name))
    n, d, C = x.shape
    _, pooled, _ = dr.reference(("quant", name))
    want = np.array([[dr.quantile_rule(x[:, j, :], p) for j in range(d)] for p in dr.PROBS])
    assert ec.same_bits_or_nan(pooled[dr.NPOOLED:], want), (pooled[dr.NPOOLED:], want)
    assert np.array_equal(np.isnan(pooled[dr.NPOOLED:]), np.isnan(want))


def test_checker_quantiles_repeated_probability_and_none():
    x = dr.batch(("quant", "ties"))
    _, p2, _ = dr.describe(x, probs=(0.5, 0.5, 0.1))
    assert ec.same_bits(p2[dr.NPOOLED], p2[dr.NPOOLED + 1])
    _, p0, _ = dr.describe(x, probs=())
    assert p0.shape == (dr.NPOOLED, x.shape[1]) and ec.same_bits_or_nan(p0, p2[:dr.NPOOLED])


def test_census_of_left_out_chains():
    """nbad against an independent numpy census; the hand-built batch marks exactly its stuck chains (and every chain
    of the all-constant parameter) by the reference arithmetic alone"""
    x = dr.batch(("stuck",))
    n, d, C = x.shape
    _, pooled, nbad = dr.reference(("stuck",))
    with np.errstate(all="ignore"):
        v = mc.stats.mcvar_imse(np.transpose(x, (2, 0, 1)))   # [C][d], the reference's estimator in numpy
        e = mc.stats.ess(np.transpose(x, (2, 0, 1)))
    bad = ~(np.isfinite(v) & np.isfinite(e) & (v > 0))
    assert sorted(np.nonzero(bad[:, 0])[0]) == sorted(dr.STUCK)
    assert bad[:, 1].all()
    assert nbad.tolist() == [len(dr.STUCK), C]
    assert np.isnan(pooled[5, 1]) and np.isfinite(pooled[5, 0])             # W = 0 -> rhat NaN
    assert np.isnan(pooled[3, 1]) and pooled[4, 1] == 0.0                   # no chain left: 0/0, empty sum
    for key in (("poison", 96), ("series", 90, 3, 65)):
        x = dr.batch(key)
        with np.errstate(all="ignore"):
            v = mc.stats.mcvar_imse(np.transpose(x, (2, 0, 1)))
            e = mc.stats.ess(np.transpose(x, (2, 0, 1)))
        assert dr.reference(key)[2].tolist() == (~(np.isfinite(v) & np.isfinite(e) & (v > 0))).sum(axis=0).tolist()


def test_rhat_is_nan_for_one_chain():
    _, pooled, _ = dr.reference(("series", 3, 1, 1))
    assert np.isnan(pooled[5]).all() and np.isfinite(pooled[1]).all()


REFUSALS = [
    # nkept, nprobs, probs, per_chain, pooled, message
    (1, 1, (0.5,), True, True, "need nkept >= 2"),
    (10, 9, (0.5,) * 9, True, True, "nprobs = 9"),
    (10, 2, (0.5, 1.5), True, True, "is not in [0, 1]"),
    (10, 1, (-0.1,), False, True, "is not in [0, 1]"),
    (10, 1, (float("nan"),), False, True, "is not in [0, 1]"),
    (10, 1, (0.5,), False, False, "per_chain, pooled or both"),
]


@pytest.mark.parametrize("nkept,nprobs,probs,want_per,want_pooled,msg", REFUSALS)
def test_abi_refuses_bad_arguments_without_a_device(nkept, nprobs, probs, want_per, want_pooled, msg):
    """MCMC_E_INVALID_ARG with a message, before any device is touched: the shape checks come first"""
    lib = _lib.load()
    assert "mcmc_stats_describe" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "mcmc_stats_describe")
    d, C = 2, 5
    x = np.zeros((max(nkept, 1), d, C))
    p = np.array(probs, dtype=np.float64)
    per = np.full((6, d, C), -7.25)
    pooled = np.full((dr.NPOOLED + max(nprobs, 0), d), -7.25)
    nbad = np.full(d, -7, dtype=np.int64)
    rc = lib.mcmc_stats_describe(None, x.ctypes.data, nkept, d, C, 0, 0, per.ctypes.data if want_per else None,
                                 p.ctypes.data, nprobs, pooled.ctypes.data if want_pooled else None, nbad.ctypes.data)
    assert rc == _lib.MCMC_E_INVALID_ARG
    assert msg in lib.mcmc_last_error().decode()
    assert (per == -7.25).all() and (pooled == -7.25).all() and (nbad == -7).all()


def test_header_and_julia_texts_name_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "mcmc_hip.h")).read()
    assert re.search(r"^int mcmc_stats_describe\(mcmc_ctx\* ctx, const double\* samples, int64_t nkept", hdr, re.M)
    assert "MCMC_DESCRIBE_NPOOLED = 6" in hdr and "MCMC_DESCRIBE_MAXPROBS = 8" in hdr
    assert "#define MCMC_ABI_VERSION 1" in hdr
    jdir = os.path.join(ROOT, "mcmc.jl_amd", "julia")
    args = ("Ptr{Float64}, Int64, Int64, Int64, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, "
            "Ptr{Int64})")
    hook = re.sub(r"\s+", " ", open(os.path.join(jdir, "mcmc_jl_hook.jl")).read())
    plain = re.sub(r"\s+", " ", open(os.path.join(jdir, "MCMCHip.jl")).read())
    assert "ccall((:mcmc_stats_describe, hiplib), Cint, (Ptr{Void}, " + args in hook
    assert "ccall((:mcmc_stats_describe, lib), Cint, (Ptr{Cvoid}, " + args in plain
    for needle in ("function hip_describe(x::Array{Float64, 3}", "function describe(io, cs::Array{MCMCChain}",
                   "describe(cs::Array{MCMCChain}) = describe(STDOUT, cs)"):
        assert needle in hook, needle


def test_twin_prints_the_reference_table_for_one_chain():
    x = dr.batch(("series", 3, 1, 1))
    out = io.StringIO()
    r = mc.stats.describe(np.transpose(x, (2, 0, 1)), io=out)
    lines = out.getvalue().splitlines()
    assert [ln.split()[0] for ln in lines[1:7]] == ["Min", "Mean", "Max", "MC", "ESS", "AC"]
    assert lines[1] == f"{'Min':<10} {float(r.per_chain[0, 0, 0])!r}"
    assert lines[7].startswith("NAs") and lines[8].startswith("NA%")
    assert r.table() is r.per_chain and r.column("ess").shape == (1, 1)
    out = io.StringIO()
    r.write_pooled(out, ["beta"])
    lines = out.getvalue().splitlines()
    assert lines[0].startswith("beta (pooled") and [ln.split()[0] for ln in lines[1:7]] == ["Min", "Mean", "Max", "MC",
                                                                                            "ESS", "Rhat"]
    assert len(lines) == 1 + 6 + len(r.probs) + 1
