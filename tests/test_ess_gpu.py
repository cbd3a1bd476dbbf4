"""The device ESS kernels (kernels/stats.hip: k_ess_reg<32|64|96>, k_ess_tile, k_ess_col) against the oracle, bit
for bit, over the case table of ess_cases.py: series that drive Geyer's scan through every round of k_ess_tile, to
the last pair of every kernel and to both sides of every round edge under a maxlag cap, with series that stop in
round 0 next to them in the same lane group, tile and block; batch means; const and NaN series; scaled copies.
test_ess_cpu.py holds the table's CPU checks (where every scan ends, the oracle against the numpy twin)."""
import numpy as np
import pytest

import mcmchip as mc
import ess_cases as ec

pytestmark = pytest.mark.gpu

CASE_VTYPES = [(c, vt) for c in ec.CASES for vt in ec.vtypes(c)]
_ids = lambda cv: f"{cv[0].name}-{cv[1]}"
_device_results = {}


def _device(c, vt, clean=False):
    """ess_device of the case through the host-array path, as the oracle lays it out: (ess [d][C], var [d][C]);
    one launch a (case, vtype), shared by the tests"""
    key = (c, vt, clean)
    if key not in _device_results:
        chain = type("Chain", (), {})()
        chain._samples = ec.samples(c, clean)
        e, v = mc.stats.ess_device(chain, vt, maxlag=c.maxlag, batchlen=c.batchlen, return_var=True)
        _device_results[key] = (np.ascontiguousarray(e.T), np.ascontiguousarray(v.T))
    return _device_results[key]


def _mismatches(c, got, ref):
    bad = np.argwhere(~((got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))))
    return [(int(j), int(ch), ec.family_of(c, j, ch), float(got[j, ch]), float(ref[j, ch])) for j, ch in bad[:8]]


@pytest.mark.parametrize("cv", CASE_VTYPES, ids=_ids)
def test_device_ess_matches_oracle(gpu, cv):
    """ESS and the variance as uint64 views against orc_ess; NaN exactly where the case has a const or nan series"""
    c, vt = cv
    e_ref, v_ref = ec.reference(c, vt)
    e, v = _device(c, vt)
    assert e.shape == e_ref.shape == (c.d, c.C)
    assert np.array_equal(np.isnan(e), ec.poison_mask(c))
    assert np.array_equal(np.isnan(e), np.isnan(e_ref)) and np.array_equal(np.isnan(v), np.isnan(v_ref))
    assert ec.same_bits_or_nan(e, e_ref), _mismatches(c, e, e_ref)
    assert ec.same_bits_or_nan(v, v_ref), _mismatches(c, v, v_ref)


@pytest.mark.parametrize("name", ec.DEVICE_POINTER_CASES)
def test_device_pointer_path_matches_oracle(gpu, name):
    """a device tensor in, a device tensor out, no variance (var = NULL): every kernel"""
    import torch
    c = ec.BY_NAME[name]
    xt = torch.from_numpy(ec.samples(c).copy()).cuda()
    for vt in ec.vtypes(c):
        e_ref, _ = ec.reference(c, vt)
        got = mc.stats.ess_device(xt, vt, maxlag=c.maxlag, batchlen=c.batchlen)
        assert got.is_cuda and tuple(got.shape) == (c.d, c.C)
        got = got.cpu().numpy()
        assert ec.same_bits_or_nan(got, e_ref), (vt, _mismatches(c, got, e_ref))


@pytest.mark.parametrize("n", ec.SCALED_N)
@pytest.mark.parametrize("s", [400, -400])
def test_device_ess_scales_exactly(gpu, n, s):
    """ess_device(2^s x) = ess_device(x) bit for bit and the variance scales by 2^(2s) exactly -- device output
    against device output, the oracle not involved"""
    c = ec.BY_NAME[f"scaled-n{n}-2^{s}"]
    c0 = ec.unscaled(c)
    for vt in ec.vtypes(c):
        e, v = _device(c, vt)
        e0, v0 = _device(c0, vt)
        assert ec.same_bits(e, e0), (vt, _mismatches(c, e, e0))
        assert ec.same_bits(v, np.ldexp(v0, 2 * s)), (vt, _mismatches(c, v, np.ldexp(v0, 2 * s)))


@pytest.mark.parametrize("c", [c for c in ec.CASES if not ec.is_finite_case(c)], ids=ec.case_id)
def test_const_and_nan_series_leave_their_neighbours_alone(gpu, c):
    """the const / nan series of a batch leave their lane-group-, tile- and wave-mates' results bitwise what they
    are with white noise in those places -- device output against device output"""
    bad = ec.poison_mask(c)
    for vt in ec.vtypes(c):
        e, v = _device(c, vt)
        e_clean, v_clean = _device(c, vt, clean=True)
        assert not np.isnan(e_clean).any() and np.array_equal(np.isnan(e), bad)
        assert ec.same_bits(e[~bad], e_clean[~bad]) and ec.same_bits(v[~bad], v_clean[~bad]), vt
        # every lane group's wave (16 series of a tile block) holds a poisoned series and a clean one
        for w in range(0, c.C - 15, 16):
            assert 0 < bad[0, w:w + 16].sum() < 16


REFUSALS = [
    # n, vtype, maxlag, batchlen, message
    (50, 1, 50, 0, "maxlag should be < nkept"),
    (300, 2, 300, 0, "maxlag should be < nkept"),
    (1, 1, 0, 0, "need nkept >= 2"),
    (50, 4, 0, 0, "Unknown ESS type 4"),
    (300, 0, 0, 0, "Unknown ESS type 0"),
    (50, 3, 0, 50, "greather than one"),
    (300, 3, 0, 151, "greather than one"),
]


@pytest.mark.parametrize("n,vtype,maxlag,batchlen,msg", REFUSALS)
def test_refusals_launch_nothing(gpu, n, vtype, maxlag, batchlen, msg):
    """MCMC_E_INVALID_ARG with the message, and the output buffers keep what they held"""
    import torch
    from mcmchip import _lib
    from mcmchip.api import _ctx
    d, C = 2, 33
    x = torch.from_numpy(np.random.default_rng(n).normal(size=(n, d, C))).cuda()
    e = torch.full((d, C), -7.25, dtype=torch.float64, device=x.device)
    v = torch.full((d, C), -7.25, dtype=torch.float64, device=x.device)
    lib = _lib.load()
    rc = lib.mcmc_stats_ess(_ctx(x.device.index or 0), x.data_ptr(), n, d, C, vtype, maxlag, batchlen, 1,
                            e.data_ptr(), v.data_ptr())
    assert rc == _lib.MCMC_E_INVALID_ARG
    assert msg in lib.mcmc_last_error().decode()
    torch.cuda.synchronize()
    assert bool((e == -7.25).all()) and bool((v == -7.25).all())
    if vtype in (1, 2, 3) and n >= 2:                           # the same through ess_device
        with pytest.raises(mc.MCMCError, match=msg) as ei:
            mc.stats.ess_device(x, {1: "imse", 2: "ipse", 3: "bm"}[vtype], maxlag=maxlag, batchlen=batchlen)
        assert ei.value.code == _lib.MCMC_E_INVALID_ARG
