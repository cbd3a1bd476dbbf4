"""CPU checks of the separable-target case table (separable_cases.py): the table names every step-kernel instance
the dispatch can produce, the oracle's run of every case both accepts and rejects (and, for the DistDSL flavours,
proposes out of the support), and the oracle itself against a 40-digit sum of the closed forms at the widest wave
and block widths.  No GPU."""
import types

import numpy as np
import pytest

import mcmchip as mc
import oracle_ref as orc
import separable_cases as sc


# ------------------------------------------------------------------ the table against the dispatch rules
def test_cases_name_every_instance():
    """Every instance the dispatch can produce for the four models x four sampler kinds (d = 1 .. 16384, both
    scale kinds, more chains than the look-ahead kernels take) is named by a case, the F instances where they are
    built and only there; no case names anything else."""
    want = sc.all_instances()
    got = {sc.expected_name(c) for c in sc.CASES}
    assert got == want, (sorted(want - got), sorted(got - want))
    # lane: NB 1..4 x {F, not F}; pair: NBL 3, 4 x {F, not F}; wave: NB 1, 2, 4, 8 x {F, not F}; block: W 4, 8
    assert "wpc_hmc<8, true, IsoDot, true>" in want and "wpc_hmc<8, true, NormalDSL, true>" not in want
    assert "lpp_mala<3, true, NormalDSL>" in want and "lpp_mala<3, true, DistDSL>" not in want
    assert "bpc_rwm<4, AbsNormalDSL>" in want and "lpc_rwm<3, false, DistDSL, false>" in want
    n_lane = 4 * (2 * 2 + 2) * (2 + 3)       # NB x (F models: F and not; others: not) x (rwm: 2 scales, 3 others)
    n_pair = 2 * (2 * 2 + 2) * (2 + 3)
    n_wave = 4 * (2 + 3) * 4                  # NB x (IsoDot: F and not; 3 others) x kinds
    n_block = 2 * 4 * 4
    assert len(want) == n_lane + n_pair + n_wave + n_block


def test_sweep_has_both_sides_of_every_class_edge():
    names = lambda d: sc.expected_step_kernel(d, "IsoDot", "mala", 100, False)
    edges = [d for d in range(1, sc.D_MAX) if names(d).replace("true", "false") != names(d + 1).replace("true", "false")]
    for d in edges:                           # 4, 8, 12, 16, 24, 32, 256, 512, 1024, 2048, 8192
        assert d in sc.D_SWEEP and d + 1 in sc.D_SWEEP, d
    for lo, hi in zip([0] + edges, edges + [sc.D_MAX]):
        assert any(lo < d <= hi and d % 4 for d in sc.D_SWEEP), (lo, hi)     # a width off the 4-block grid
    for c in sc.CASES:
        C = sc.nchains(c)
        assert C > sc.LA_MAX_CHAINS or sc.family(c.d) in ("wpc", "bpc")
        assert C % 64 and (sc.family(c.d) != "wpc" or C % 4)                 # tail wave; tail block of 4 waves


# ------------------------------------------------------------------ the oracle's run of every case
def _proposals_out_of_support(c, m, C, r):
    """How many of the oracle's proposals in the run of case c have a -Inf log-target.  HMC kinds: the last
    leapfrog state of the kept steps' trajectory records (orc_run_leaps).  RWM / MALA: the chain stepped one step
    at a time, its proposal rebuilt from the step's normals -- read off a second oracle chain on a flat target that
    accepts every proposal (x = 0, scale 1: its state after the step is the step's normal vector) -- and
    evaluated with eval_batch."""
    sp = sc.sampler(c)
    oc = orc.OracleChains(m, sp, nchains=C, seed=sc.seed(c))
    if sc.kind_of(c.sampler) in ("hmc", "hmcda"):
        cap = sp.leaps_cap()
        _, _, _, lv = oc.run_leaps(r, cap)
        last = np.minimum(lv["nleaps"], cap)
        lp_prop = np.take_along_axis(lv["logTarget"], last[:, None, :], axis=1)[:, 0, :]
        return int(np.sum(lp_prop == -np.inf)), oc
    flat = mc.MCMCLikelihoodModel(mc.DistDSL("Uniform", -1e300, 1e300), np.zeros(c.d))
    zs = orc.OracleChains(flat, mc.RWM(1.0), nchains=C, seed=sc.seed(c))
    one = types.SimpleNamespace(burnin=r.burnin, thinning=1, len=1, r=range(1))    # step i of the case's runner
    sc_eff = m.scale * sp.scale if c.sampler == "rwm" else None
    n_oos = 0
    for t in range(r.len):
        zs.x[:] = 0.0
        zs.steps_done = t
        zs.run(mc.SerialMC(steps=1))
        z = zs.x.copy()
        assert np.all(np.isfinite(z)) and np.all(z != 0.0)
        if c.sampler == "rwm":
            xp = oc.x + z * sc_eff[:, None]
        else:
            h = oc.t_step if sp.tuner is not None else sp.driftStep
            xp = (oc.x + (h / 2.0) * orc.eval_batch(m, oc.x)[1]) + np.sqrt(h) * z
        n_oos += int(np.sum(orc.eval_batch(m, xp)[0] == -np.inf))
        oc.run(one)
    return n_oos, oc


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_oracle_run_accepts_rejects_and_leaves_the_support(c):
    """The step sizes of the table are right for the width: the oracle's run of the case has accepted and rejected
    kept steps and a kept sample off the init (so that a kernel that mis-stored an accepted proposal, or the
    rejected one, cannot pass), and for the DistDSL flavours at least one proposal out of the support."""
    m, C, r = sc.model(c), sc.nchains(c), sc.runner(c)
    assert r.len <= (24 if c.d <= 2048 else 6)
    oc = orc.OracleChains(m, sc.sampler(c), nchains=C, seed=sc.seed(c))
    s, g, acc = oc.run(r)
    assert 0 < acc.sum() < acc.size, f"accept rate {acc.mean()}"
    assert np.any(s != m.init[None, :, None])
    assert np.all(np.isfinite(oc.lp))
    if c.flavour in sc.DIST_FLAVOURS:
        n_oos, oc2 = _proposals_out_of_support(c, m, C, r)
        assert np.array_equal(oc2.x, oc.x) and np.array_equal(oc2.lp, oc.lp)     # the same run, stepped
        assert n_oos > 0


def test_existing_wide_cases_accept_rates(capsys):
    """Measured, not asserted: the oracle's accept rate over the kept steps of the existing wide RWM / MALA cases
    (test_gpu_parity.py test_sampler_parity at d >= 257 and test_block_per_chain_parity).  Measured:
    test_sampler_parity (iso / normal / abs) d = 257: rwm 0 / 0 / 0.009, mala 0.334 / 0.800 / 0.045; d = 1024: rwm
    0 / 0 / 0.027, mala 0.293 / 0.194 / 0.027.  test_block_per_chain_parity (iso / normal) rwm: 0 / 0 at every d
    of 2049, 5000, 8192, 8193, 16384; mala: 0.800 / 0.067 at 2049, then 0.733, 0.800, 0.867, 0.933 / 0 at 5000,
    8192, 8193, 16384.  Where the rate is 0 the case pins only the reject path: the state never moves and the kept
    samples equal the init (every wide RWM case on iso and normal, MALA on normal from d = 5000).  Those cases stay
    as they are; the cases of separable_cases.py are the ones that move."""
    from test_gpu_parity import SAMPLERS, _model
    rows = []
    for d, kinds, C, r, seed in [(d, ("iso", "normal", "abs"), 67, mc.SerialMC(steps=20, burnin=6, thinning=3), 12345 + d)
                                 for d in (257, 1024)] + \
                                [(d, ("iso", "normal"), 5, mc.SerialMC(steps=6, burnin=1, thinning=2), 2024 + d)
                                 for d in (2049, 5000, 8192, 8193, 16384)]:
        for sname in ("rwm", "mala"):
            for mk in kinds:
                m = _model(mk, d)
                s, _, acc = orc.OracleChains(m, SAMPLERS[sname](), nchains=C, seed=seed).run(r)
                rows.append((d, sname, mk, float(acc.mean()), bool(np.any(s != m.init[None, :, None]))))
    with capsys.disabled():
        print()
        for d, sname, mk, rate, moved in rows:
            print(f"existing wide case d={d:5d} {sname:4s} {mk:6s}: oracle accept rate {rate:.3f}"
                  f"{'' if moved else '  (state never moves)'}")
    assert len(rows) == 2 * 2 * 3 + 5 * 2 * 2


# ------------------------------------------------------------------ the oracle against 40 digits
def _mp_terms(fl, x):
    """The closed-form log-density terms of flavour fl at x, 40 digits each"""
    import mpmath as mp
    mp.mp.dps = 40
    f = mp.mpf
    t = sc.FLAVOURS[fl].target()
    if fl == "iso":
        return [-(f(v) * f(v)) for v in x]
    if fl in ("normal", "abs"):
        mu, sg = f(t.mu), f(t.sigma)
        c = -mp.log(2 * mp.pi) / 2 - mp.log(sg)
        return [c - ((abs(f(v)) if fl == "abs" else f(v)) - mu) ** 2 / (2 * sg * sg) for v in x]
    p1, p2 = f(t.mu), f(t.sigma)
    if fl == "gamma":
        c = -mp.loggamma(p1) - p1 * mp.log(p2)
        return [c + (p1 - 1) * mp.log(f(v)) - f(v) / p2 for v in x]
    if fl == "weibull":
        c = mp.log(p1 / p2)
        return [c + (p1 - 1) * mp.log(f(v) / p2) - (f(v) / p2) ** p1 for v in x]
    c = -mp.log(mp.beta(p1, p2))
    return [c + (p1 - 1) * mp.log(f(v)) + (p2 - 1) * mp.log(1 - f(v)) for v in x]


def _closed_form_grad(fl, x):
    """The DSL's x-derivative rules as written (MCMCDerivRules.jl:57, :69, :74, :88): a rearranged form would differ
    from them by the cancellation next to the gradient's zero, which is the rule's own and not an error"""
    t = sc.FLAVOURS[fl].target()
    if fl == "iso":
        return -2.0 * x
    if fl == "normal":
        return (t.mu - x) / t.sigma**2
    if fl == "abs":
        return np.sign(x) * (t.mu - np.abs(x)) / t.sigma**2
    p1, p2 = t.mu, t.sigma
    if fl == "gamma":
        return -(p2 + x - p1 * p2) / (p2 * x)
    if fl == "weibull":
        return ((1.0 - (x / p2) ** p1) * p1 - 1.0) / x
    return (p1 - 1.0) / x - (p2 - 1.0) / (1.0 - x)


K_TERM = 3.0       # allowance for the terms' own error in units of 2^-53 sum |term_i| (measured: the docstring below)
# where the DistDSL gradient rules cross zero (Gamma (p1 - 1) p2, Weibull p2 (1 - 1/p1)^(1/p1), Beta's mode): there the
# rule subtracts two rounded, nearly equal parts and a relative error means nothing, for any implementation
GRAD_ZERO = {"gamma": 1.5 * 0.7, "weibull": 2.0 * (1.0 / 3.0) ** (2.0 / 3.0), "beta": 1.0 / 3.0}


@pytest.mark.parametrize("fl", list(sc.FLAVOURS))
@pytest.mark.parametrize("d", [2048, 16384])
def test_oracle_against_high_precision_at_the_widest(fl, d, capsys):
    """orc.eval_batch in the library's order (wave per chain at 2048, 8 waves at 16384) against the 40-digit sum of
    the closed-form terms, so that the device and the oracle cannot be wrong together at the widths only the new
    GPU cases reach.  Bound: the first-order rounding bound (d + k) 2^-53 sum |term_i| of a d-term sum: d for the
    additions, k for the terms' own error, k = sum |oracle term_i - exact term_i| / (2^-53 sum |term_i|) with the
    oracle's terms evaluated one at a time (a d = 1 model).  (The aggregate form because Beta's and Gamma's
    log-density cross zero inside the batch, where a single term's relative error is unbounded.)
    Measured k: iso 0.36, normal 0.69, abs 0.67, gamma 0.94, weibull 0.60, beta 2.29 (the slowest: two det_log
    products against a constant, cancelling): K_TERM = 3.  Measured |oracle - exact| / (2^-53 sum |term_i|): at most
    1.04 at d = 2048 and 0.96 at d = 16384, against the bounds 2051 and 16387.
    The gradient is elementwise the DSL's rule at 1e-13 relative; points within 5 % of a rule's zero are moved
    10 % up (GRAD_ZERO)."""
    import mpmath as mp
    x = sc._in_support(fl, d, 1)
    if fl in GRAD_ZERO:
        x0 = GRAD_ZERO[fl]
        x = np.where(np.abs(x - x0) < 0.05 * x0, x + 0.1 * x0, x)
    m = mc.MCMCLikelihoodModel(sc.FLAVOURS[fl].target(), x[:, 0], gradient=True)
    lp, g = orc.eval_batch(m, x)
    terms = _mp_terms(fl, x[:, 0])
    exact = mp.fsum(terms)
    sum_abs = mp.fsum(abs(t) for t in terms)
    unit = float(mp.mpf(2) ** -53 * sum_abs)
    dev = abs(float(mp.mpf(float(lp[0])) - exact)) / unit
    m1 = mc.MCMCLikelihoodModel(sc.FLAVOURS[fl].target(), x[:1, 0], gradient=True)
    t1 = orc.eval_batch(m1, x[:, 0][None, :])[0]
    k = float(mp.fsum(abs(mp.mpf(float(a)) - b) for a, b in zip(t1, terms))) / unit
    with capsys.disabled():
        print(f"\noracle vs 40 digits {fl:8s} d={d:5d}: |oracle - exact| = {dev:.2f} x 2^-53 sum|term| "
              f"(bound {d + K_TERM:.0f}), terms' own error k = {k:.3f}")
    assert k <= K_TERM
    assert dev <= d + K_TERM
    np.testing.assert_allclose(g[:, 0], _closed_form_grad(fl, x[:, 0]), rtol=1e-13, atol=0)
