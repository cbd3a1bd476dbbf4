"""CPU checks of the device-ESS case table (ess_cases.py): a census of where Geyer's initial-sequence scan ends for
every series (numpy, plain dot products) -- the proof that the table drives k_ess_tile through every round, k_ess_col
and every k_ess_reg bucket to their last pair, and mixes stop rounds inside a tile -- then the oracle's orc_ess
against the numpy twin (FFT autocovariances), its exact scaling by powers of two, and its NaN positions.  No GPU."""
import types

import numpy as np
import pytest

import mcmchip as mc
import ess_cases as ec

MARGIN = 1e-9            # no pair sum the scan looks at is within this (relative to acv0) of zero

MIXED_LAYOUTS = (ec.MIXED, ec.POISONED, ec.SCALED)


def _case(name):
    return ec.BY_NAME[name]


def _ends(c, fams=None):
    return [e for _, _, f, e, _ in ec.census(c) if fams is None or f in fams]


# ------------------------------------------------------------------ census
def test_table_reaches_every_kernel_edge():
    """every n mod 8 on the tile path, both sides of every kernel and bucket edge, the staging pass and dynamic-LDS
    edges, the smallest and the largest n of every kernel, every shape, and k on both sides of every round edge"""
    full = [c for c in ec.CASES if c.maxlag == c.n - 1 and c.layout == ec.MIXED and c.C == 130]
    by_kernel = {}
    for c in full:
        by_kernel.setdefault(ec.kernel_of(c.n, "imse"), set()).add(c.n)
    assert min(by_kernel["reg32"]) == 2 and max(by_kernel["reg32"]) == 32 and 3 in by_kernel["reg32"]
    assert min(by_kernel["reg64"]) == 33 and max(by_kernel["reg64"]) == 64
    assert min(by_kernel["reg96"]) == 65 and max(by_kernel["reg96"]) == 96 and 95 in by_kernel["reg96"]
    assert min(by_kernel["tile"]) == 97 and max(by_kernel["tile"]) == ec.TILE_MAX_N == 618
    assert {n % 8 for n in by_kernel["tile"]} == set(range(8))
    assert {192, 193, 240, 241, 617} <= by_kernel["tile"]
    assert min(by_kernel["col"]) == 619 and 1000 in by_kernel["col"]
    shapes = {(c.n, c.d, c.C) for c in ec.CASES if c.name.startswith("shape")}
    assert shapes == {(n, d, C) for n in ec.SHAPE_N for d in (1, 3) for C in (1, 31, 33, 65, 130)}
    assert {ec.kernel_of(n, "imse") for n in ec.SHAPE_N} == {"reg64", "tile", "col"}
    for n in (300, 1000):
        ks = {ec.k_of(c.maxlag) for c in ec.CASES if c.name.startswith(f"cap-n{n}-")}
        assert {0, 3, 4, 19, 20, 35, 36, ec.k_of(n - 2), ec.k_of(n - 1)} <= ks
        assert {c.maxlag for c in ec.CASES if c.name.startswith(f"cap-n{n}-")} == \
            {1, 2, 7, 8, 9, 39, 40, 41, 71, 72, 73, n - 2, n - 1}
    bm = {(c.n, c.batchlen) for c in ec.CASES if c.name.startswith("bm-")}
    assert bm == {(4, 2), (33, 16), (618, 20), (618, 309), (1000, 7)}
    assert all(ec.kernel_of(n, "bm") == ("col" if n == 1000 else "tile") for n, _ in bm)
    assert max(c.C for c in ec.CASES) == 130
    assert all(1 <= c.maxlag <= c.n - 1 and (c.batchlen == 0 or c.n // c.batchlen > 1) for c in ec.CASES)


def test_device_pointer_cases_cover_every_kernel():
    kernels = {ec.kernel_of(ec.BY_NAME[n].n, vt) for n in ec.DEVICE_POINTER_CASES for vt in ec.vtypes(ec.BY_NAME[n])}
    assert kernels == {"reg32", "reg64", "reg96", "tile", "col"}


def test_alt_runs_to_k_and_takes_the_imse_clamp():
    """every pair of an `alt` series is positive: only k ends its scan, in every case and at every maxlag; nearly
    all of its pairs take IMSE's clamp, so IMSE and IPSE differ"""
    n_alt = 0
    for c in ec.CASES:
        k = ec.k_of(c.maxlag)
        for e in _ends(c, ("alt",)):
            assert e == k + 1, (c.name, e, k)
            n_alt += 1
    assert n_alt > 500
    for n in (617, 618):
        c = _case(f"tile-n{n}")
        assert ec.family_of(c, 0, 0) == "alt"
        clamps = ec.clamp_count(ec.samples(c)[:, 0, 0], c.maxlag)
        assert clamps >= 0.9 * ec.k_of(c.maxlag), clamps
    c = _case("tile-n618")
    e1, _ = ec.reference(c, "imse")
    e2, _ = ec.reference(c, "ipse")
    m = ec.family_mask(c, ("alt",))
    assert m.sum() >= 16 and np.all(e1[m] != e2[m])


def test_altstop_ends_where_the_table_says():
    for c in ec.CASES:
        if c.maxlag != c.n - 1:
            continue
        seen = 0
        for j in range(c.d):
            for ch in range(c.C):
                if ec.family_of(c, j, ch) == "altstop":
                    p = ec.altstop_pair(c.n, seen)
                    seen += 1
                    e = next(e for jj, cc, _, e, _ in ec.census(c) if (jj, cc) == (j, ch))
                    assert e == (p if p is not None else ec.k_of(c.maxlag) + 1), (c.name, j, ch, e, p)


def test_tile_kernel_runs_every_round():
    """n = 618 (k = 308, 309 pairs): series end their scan in round 0, in round 1 and in every later round up to
    the last (round 20: pairs 308 ..), and one runs all 309 pairs; the same one length down"""
    for name, npairs in (("tile-n618", 309), ("tile-n617", 308), ("bm-n618-bl20", 309), ("poison-n618-bl20", 309)):
        c = _case(name)
        ends = _ends(c)
        last = ec.round_of(npairs)
        want = set(range(last + 1))
        got = {ec.round_of(e) for e in ends}
        if c.layout == ec.MIXED:
            assert got == want, (name, sorted(want - got))
        assert {0, 1, last} <= got and len(got) >= 15
        assert max(ends) == npairs == ec.k_of(c.maxlag) + 1
    assert ec.round_of(309) == 20 and ec.round_of(3) == 0 and ec.round_of(4) == 1 and ec.round_of(19) == 1 and \
        ec.round_of(20) == 2 and ec.round_of(35) == 2 and ec.round_of(36) == 3
    # every tile length has a series that runs to its k, and series in three rounds at least
    for n in ec.TILE_N:
        c = _case(f"tile-n{n}")
        ends = _ends(c)
        assert max(ends) == ec.k_of(n - 1) + 1 and len({ec.round_of(e) for e in ends}) >= 4


def test_column_kernel_runs_to_the_last_pair():
    """n = 1000 (k = 499, 500 pairs): ends in every sixteen-pair stretch and one series through all 500"""
    c = _case("col-n1000")
    ends = _ends(c)
    assert {ec.round_of(e) for e in ends} == set(range(ec.round_of(500) + 1))
    assert max(ends) == 500 == ec.k_of(c.maxlag) + 1
    assert max(_ends(_case("col-n619"))) == 309


def test_register_buckets_run_to_their_last_pair():
    for n in (32, 64, 96):                                     # the bucket's largest n: the scan reaches jj = N/2 - 1
        ends = _ends(_case(f"reg-n{n}"))
        assert max(ends) == n // 2 == ec.k_of(n - 1) + 1
        assert len({e // 2 for e in ends}) >= 5                # the pair loop's uniform exit sees many stop steps
    for n in (2, 3):
        assert set(_ends(_case(f"reg-n{n}"))) == {1}           # k = 0: one pair


def test_mixed_cases_mix_stop_rounds_inside_a_tile():
    """at least three different stop rounds among the first 32 series (one k_ess_tile block, half a wave of
    k_ess_reg / k_ess_col) of every mixed case that has the pairs for it"""
    n_checked = 0
    for c in ec.CASES:
        if c.layout not in MIXED_LAYOUTS or c.C < 31 or ec.k_of(c.maxlag) < 4:
            continue
        rounds = {ec.round_of(e) for j, ch, _, e, _ in ec.census(c) if j == 0 and ch < 32}
        steps = {e // 2 for j, ch, _, e, _ in ec.census(c) if j == 0 and ch < 32}
        if ec.k_of(c.maxlag) >= 36:
            assert len(rounds) >= 3, (c.name, rounds)
        assert len(steps) >= 3, (c.name, steps)
        n_checked += 1
    assert n_checked >= 40


def test_no_pair_sum_is_within_rounding_of_zero():
    """the numpy census and the oracle cannot disagree about where a scan ends: every pair sum a deterministic series'
    scan looks at, the stopping one included, is at least 1e-9 acv0 away from zero"""
    for c in ec.CASES:
        for j, ch, fam, e, margin in ec.census(c):
            if fam in ec.DETERMINISTIC:
                assert margin is not None and margin > MARGIN, (c.name, j, ch, fam, e, margin)


def test_no_two_series_of_a_case_are_equal():
    for c in ec.CASES:
        if c.n < 4 or not ec.is_finite_case(c):                 # n = 2, 3: centred, all series of a family are one
            continue
        x = ec.samples(c).reshape(c.n, -1)
        assert len({x[:, s].tobytes() for s in range(x.shape[1])}) == x.shape[1], c.name


# ------------------------------------------------------------------ the oracle against the numpy twin
def _zero_by_identity(c, vtype):
    """[d][C]: series whose IPSE variance is zero in exact arithmetic.  Summed over every lag 0 .. n - 1 the
    autocovariances of a centred series give -acv0 + 2 sum acv = (sum z)^2 / n = 0; IPSE does exactly that when n
    is even, maxlag = n - 1 and no pair stops the scan (and so does IMSE when, besides, no pair takes its clamp: a
    series of two or four steps).  What either side returns there is rounding residue."""
    m = np.zeros((c.d, c.C), dtype=bool)
    if vtype in ("imse", "ipse") and c.n % 2 == 0 and c.maxlag == c.n - 1:
        for j, ch, _, e, _ in ec.census(c):
            m[j, ch] = e == ec.k_of(c.maxlag) + 1 and \
                (vtype == "ipse" or ec.clamp_count(ec.samples(c)[:, j, ch], c.maxlag) == 0)
    return m


FINITE = [c for c in ec.CASES if ec.is_finite_case(c)]


@pytest.mark.parametrize("c", FINITE, ids=ec.case_id)
def test_oracle_matches_numpy_twin(c):
    """orc_ess against mcmchip.stats (FFT autocovariances) at rtol = 1e-10, ESS and the variance, for imse, ipse and
    the case's batch means.  A series whose IPSE variance is zero by identity (_zero_by_identity) has no relative
    error to speak of: its variance is held to 1e-10 of var_iid (the size of the terms that cancel) instead, and
    its ESS, a quotient by that residue, is not compared."""
    chain = types.SimpleNamespace(samples=np.transpose(ec.samples(c), (2, 0, 1)))
    viid = mc.stats.mcvar_iid(chain).T
    for vt in ec.vtypes(c):
        e, v = ec.reference(c, vt)
        kw = {"batchlen": c.batchlen} if vt == "bm" else {"maxlag": c.maxlag}
        with np.errstate(divide="ignore", invalid="ignore"):
            en = mc.stats.ess(chain, vt, **kw).T
        vn = {"imse": mc.stats.mcvar_imse, "ipse": mc.stats.mcvar_ipse, "bm": mc.stats.mcvar_bm}[vt](chain, **kw).T
        z = _zero_by_identity(c, vt)
        np.testing.assert_allclose(e[~z], en[~z], rtol=1e-10, atol=0, err_msg=f"{c.name} {vt} ess")
        np.testing.assert_allclose(v[~z], vn[~z], rtol=1e-10, atol=0, err_msg=f"{c.name} {vt} var")
        assert np.all(np.abs(v[z] - vn[z]) <= 1e-10 * viid[z]), (c.name, vt)
        assert np.all(np.abs(v[z]) <= 1e-10 * viid[z])


def test_zero_by_identity_is_rare_and_understood():
    """only `alt` series (and `altstop` ones too short for a spike pair) of even full-maxlag cases"""
    n_zero = n_all = 0
    for c in FINITE:
        z = _zero_by_identity(c, "ipse")
        n_zero += int(z.sum())
        n_all += z.size
        assert not (z & ~ec.family_mask(c, ("alt",))).any() or c.n < 6, c.name
        assert not _zero_by_identity(c, "imse").any() or c.n < 6
    assert 0 < n_zero < 0.12 * n_all


# ------------------------------------------------------------------ exact scaling
@pytest.mark.parametrize("n", ec.SCALED_N)
@pytest.mark.parametrize("s", [400, -400])
def test_oracle_scales_exactly(n, s):
    """orc_ess(2^s x) = orc_ess(x) bit for bit, and the variance is the unscaled one times 2^(2s) exactly: every
    operation scales exactly while nothing under- or overflows.  This does not rest on the oracle being right."""
    c = _case(f"scaled-n{n}-2^{s}")
    c0 = ec.unscaled(c)
    assert np.array_equal(ec.samples(c), np.ldexp(ec.samples(c0), s))
    for vt in ec.vtypes(c):
        e, v = ec.reference(c, vt)
        e0, v0 = ec.reference(c0, vt)
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(v0)) and np.any(v0 != 0.0)
        assert ec.same_bits(e, e0), (n, s, vt)
        assert ec.same_bits(v, np.ldexp(v0, 2 * s)), (n, s, vt)


# ------------------------------------------------------------------ const and nan series
POISONED_CASES = [c for c in ec.CASES if not ec.is_finite_case(c)]


@pytest.mark.parametrize("c", POISONED_CASES, ids=ec.case_id)
def test_oracle_nan_positions_and_neighbours(c):
    """ESS is NaN for exactly the const (0 / 0) and nan series; every other series has bit for bit the result it has
    in the same batch with those series replaced by white noise"""
    bad = ec.poison_mask(c)
    assert 20 <= bad.sum() < bad.size / 2
    const = ec.family_mask(c, ("const",))
    for vt in ec.vtypes(c):
        e, v = ec.reference(c, vt)
        ec_, vc = ec.reference(c, vt, True)
        assert np.array_equal(np.isnan(e), bad), (c.name, vt)
        assert np.array_equal(np.isnan(v), bad & ~const) and not v[const].any()   # const: var = +0, ESS = 0 / 0
        assert not np.isnan(ec_).any() and np.all(np.isfinite(vc))
        assert ec.same_bits(e[~bad], ec_[~bad]) and ec.same_bits(v[~bad], vc[~bad])
        assert not np.signbit(v[const]).any()
