"""The oracle's regression log-target and gradient against an independent high-precision reference, at every case
of glm_cases.py and in three beta regimes (CPU only; test_glm_shapes.py then holds the GPU bitwise to the oracle at
the same points).

The reference is written from the model definitions (include/mcmc_hip.h; the reference project's
examples/{logistic,linear,probit}_regression.jl), not from oracle.c: eta = X beta exactly (fractions.Fraction over
the cases' integer forms), everything after it in mpmath at 50 digits, sums included.

The tolerance is the first-order rounding bound of the operation, per element, from the reference's own
quantities (u = 2^-53, gamma_k = k u / (1 - k u)):

    |d eta_i|  <= gamma_d sum_j |x_ij beta_j|
    |d term_i| <= |f'(eta_i)| |d eta_i| + eps_f(i)
    |d r_i|    <= |r'(eta_i)| |d eta_i| + eps_r(i)
    lp:   sum_i |d term_i| + gamma_{n_pad + d + 4} (sum_i |term_i| + sum_j |prior_j|)
    g_j:  gamma_{n_pad + 2} sum_i |x_ij r_i| + sum_i |x_ij| |d r_i| + 2 u |prior'_j|

with eps_f, eps_r the per-function accuracies that test_oracle.py pins:
  logistic  eps_f = 2 ulp(term) + 2^-57, eps_r = 3 ulp(r) + 2^-57 (test_logistic_term_accuracy);
  linear    eps_f = 4 u |term|; r = (y - eta) * (1 / (s * s)) is four roundings, eps_r = 4 u |r|;
  probit    the log-cdf is within 4e-15 relative (test_erfc_and_normal_logcdf_accuracy) of, for z >= -1, the log-cdf
            of the *rounded* argument RN(z RN(1/sqrt 2)), whose two roundings move log Phi(z) by up to
            2 u |z| phi(z) / Phi(z): eps_f = 4e-15 |f| + [z >= -1] 2 u |z| phi(z) / Phi(z).  The weight is
            exp(A - logcdf), A = -(eta^2 + log 2 pi) / 2: |dA| <= 2 u |A|, the subtraction u |A - logcdf|, exp one
            ulp (2 u): eps_r = |r| (2 u |A| + u |A - f| + eps_f + 2 u).
A factor of 2 over the bound is allowed for second-order terms, nothing more.

Measured worst err / bound over all cases and regimes (lp, gradient):
    logistic      0.063, 0.48
    logistic_neg  0.070, 0.73
    linear        0.064, 0.36
    probit        0.085, 0.43
The cancelling regime's products and partial sums are all exactly representable (few-bit dyadic inputs), so it
measures no rounding: what it checks is that no coordinate of magnitude 2^20 is dropped, doubled or misplaced.
"""
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

import glm_cases as gc
import oracle_ref as orc


U = 2.0**-53


def gamma(k):
    return k * U / (1 - k * U)


# ------------------------------------------------------------------ the reference
def reference(case, num, k):
    """lp [C] and g [d][C] as mpf, and the float64 per-observation quantities the bounds need:
    dict(eta, term, r, dr, z, la) each [n][C], prior [d][C], dprior [d][C]."""
    mp.mp.dps = 50
    kind, n, d, C = case
    _, _, Xi, Yi = gc.data(kind, n, d)
    sp = mp.mpf(gc.PRIOR_SIGMA[kind])
    sn = mp.mpf(gc.NOISE_SIGMA)
    c2pi = mp.log(2 * mp.pi) / 2
    Xo = Xi.astype(object)
    H = Xo @ num                                              # exact integers: eta = H / (64 2^k)
    Xm = [[mp.mpf(int(v)) / 64 for v in col] for col in Xi.T]
    lp, g = [], [[None] * C for _ in range(d)]
    q = {key: np.zeros((n, C)) for key in ("eta", "term", "r", "dr", "z", "la")}
    prior, dprior = np.zeros((d, C)), np.zeros((d, C))
    for c in range(C):
        terms, rs = [], []
        for i in range(n):
            e = Fraction(int(H[i, c]), 64 << k)
            eta = mp.mpf(e.numerator) / e.denominator
            if kind == "linear":
                resid = mp.mpf(int(Yi[i])) / 32 - eta
                term = -(resid / sn) ** 2 / 2 - c2pi - mp.log(sn)      # resid ~ Normal(0, sn)
                r, dr, z, la = resid / sn**2, 1 / sn**2, resid, 0
            elif kind == "probit":
                z = eta if Yi[i] else -eta                              # y logcdf(eta) + (1 - y) logcdf(-eta)
                la = mp.log(mp.ncdf(z))
                term = la
                lam = mp.npdf(z) / mp.ncdf(z)
                r, dr = (lam if Yi[i] else -lam), lam * (lam + z)
            else:                                                       # Y ~ Bernoulli(1 / (1 + exp(-s eta)))
                s = -1 if kind == "logistic_neg" else 1
                w = s if Yi[i] else -s
                p = 1 / (1 + mp.exp(-w * eta))                          # the probability of the observed class
                term, r, dr, z, la = mp.log(p), w * (1 - p), p * (1 - p), eta, 0
            terms.append(term)
            rs.append(r)
            for key, v in (("eta", eta), ("term", term), ("r", r), ("dr", dr), ("z", z), ("la", la)):
                q[key][i, c] = float(v)
        pr = []
        for j in range(d):
            b = mp.mpf(int(num[j, c])) / (1 << k)
            pr.append(-(b / sp) ** 2 / 2 - c2pi - mp.log(sp))           # vars ~ Normal(0, sp)
            dp = -b / sp**2
            g[j][c] = mp.fdot(Xm[j], rs) + dp
            prior[j, c], dprior[j, c] = float(pr[-1]), float(dp)
        lp.append(mp.fsum(terms) + mp.fsum(pr))
    q["prior"], q["dprior"] = prior, dprior
    return lp, g, q


# ------------------------------------------------------------------ the bound
def glm_bounds(kind, X, B, q):
    """First-order rounding bounds (lp [C], g [d][C]) of the module docstring from float64 quantities: X [n][d],
    B [d][C], q the per-observation dict of reference() (term, r, |r'| as dr, z, la; prior, dprior)."""
    n, d = X.shape
    n_pad = (n + 15) // 16 * 16
    aX = np.abs(X)
    deta = gamma(d) * (aX @ np.abs(B))                                  # [n][C]
    term, r = np.abs(q["term"]), np.abs(q["r"])
    if kind == "linear":
        eps_f, eps_r = 4 * U * term, 4 * U * r
    elif kind == "probit":
        z, la = q["z"], q["la"]
        eps_f = 4e-15 * term + np.where(z >= -1, 2 * U * np.abs(z) * r, 0.0)
        A = (z * z + np.log(2 * np.pi)) / 2
        eps_r = r * (2 * U * A + U * np.abs(-A - la) + eps_f + 2 * U)
    else:
        eps_f = 2 * np.spacing(term) + 2.0**-57
        eps_r = 3 * np.spacing(r) + 2.0**-57
    dterm = r * deta + eps_f                                            # f'(eta) = r for all three families
    dr = np.abs(q["dr"]) * deta + eps_r
    lp = dterm.sum(0) + gamma(n_pad + d + 4) * (term.sum(0) + np.abs(q["prior"]).sum(0))
    g = gamma(n_pad + 2) * (aX.T @ r) + aX.T @ dr + 2 * U * np.abs(q["dprior"])
    return lp, g


def float_quantities(kind, X, Y, B, prior_sigma=1.0, noise_sigma=1.0, link_sign=1.0):
    """glm_bounds' per-observation quantities in plain float64, for callers whose reference is itself a float64 one
    (the bound needs them to a few digits only); logistic and linear."""
    eta = X @ B
    if kind == "linear":
        resid = Y[:, None] - eta
        term = -0.5 * (resid / noise_sigma) ** 2 - 0.5 * np.log(2 * np.pi) - np.log(noise_sigma)
        r, dr = resid / noise_sigma**2, np.full_like(eta, 1 / noise_sigma**2)
    else:
        w = np.where(Y[:, None] >= 0.5, link_sign, -link_sign)
        term = -np.logaddexp(0.0, -w * eta)
        p = np.exp(term)
        r, dr = w * (1 - p), p * (1 - p)
    prior = -0.5 * (B / prior_sigma) ** 2 - 0.5 * np.log(2 * np.pi) - np.log(prior_sigma)
    return dict(eta=eta, term=term, r=r, dr=dr, z=eta, la=np.zeros_like(eta), prior=prior, dprior=-B / prior_sigma**2)


def _ratios(case, regime):
    """worst err / bound of the oracle's lp and gradient in one regime, with the regime's own conditions checked"""
    B, num, k = gc.betas(case, regime)
    m = gc.make_model(case.kind, case.n, case.d)
    X = m.target.X
    lp, g = orc.eval_batch(m, B)
    assert np.isfinite(lp).all() and np.isfinite(g).all()              # saturating stays below the -Inf rule
    lp_ref, g_ref, q = reference(case, num, k)
    eta, top = q["eta"], np.abs(q["z"]).max()                          # eta: the exact one, rounded once
    if regime == "saturating":
        sat = gc.SATURATION[case.kind]
        assert (sat / 2 < np.abs(eta).max() <= sat) and (case.kind != "linear" or top <= 50 * gc.NOISE_SIGMA)
    else:
        assert 1.5 < np.abs(eta).max() <= 3.0
    if regime == "cancelling" and case.d >= 4:
        assert ((np.abs(X) @ np.abs(B)) >= 1e3 * np.abs(eta)).all()
    lp_b, g_b = glm_bounds(case.kind, X, B, q)
    lp_err = np.array([float(abs(mp.mpf(float(lp[c])) - lp_ref[c])) for c in range(case.C)])
    g_err = np.array([[float(abs(mp.mpf(float(g[j, c])) - g_ref[j][c])) for c in range(case.C)] for j in range(case.d)])
    assert (lp_b > 0).all() and (g_err[g_b == 0] == 0).all()           # a zero bound: x_ij = 0 = beta_j, no error
    return (lp_err / lp_b).max(), (g_err / np.where(g_b > 0, g_b, 1.0)).max()


@pytest.mark.parametrize("case", gc.CASES, ids=gc.case_id)
def test_oracle_within_rounding_bound_of_exact_reference(case):
    """orc.eval_batch against the exact-eta / 50-digit reference within twice the first-order rounding bound, every
    case of the shared list, moderate, cancelling and saturating betas (measured maxima in the module docstring)."""
    for regime in gc.REGIMES:
        r_lp, r_g = _ratios(case, regime)
        print(f"RATIO {case.kind} {regime} n={case.n} d={case.d} C={case.C} lp {r_lp:.4g} g {r_g:.4g}")
        assert r_lp <= 2.0 and r_g <= 2.0, f"{regime}: err / bound lp {r_lp:.3g}, gradient {r_g:.3g}"


def test_reference_is_not_the_oracle_restated():
    """The reference on a case small enough to write out by hand: n = 1, d = 1, X = [[1]], y = 1, beta = b: the
    logistic log-target is -log(1 + exp(-b)) - b^2/2 - log(2 pi)/2 and its gradient 1/(1 + exp(b)) - b."""
    case = gc.Case("logistic", 1, 1, 1)
    B, num, k = gc.betas(case, "moderate")
    b = mp.mpf(int(num[0, 0])) / (1 << k)
    lp, g, _ = reference(case, num, k)
    mp.mp.dps = 50
    assert abs(lp[0] - (-mp.log(1 + mp.exp(-b)) - b * b / 2 - mp.log(2 * mp.pi) / 2)) < mp.mpf(10) ** -45
    assert abs(g[0][0] - (1 / (1 + mp.exp(b)) - b)) < mp.mpf(10) ** -45
    assert float(b) == B[0, 0]


# ------------------------------------------------------------------ the list itself
def test_case_list_covers_every_class():
    """A condition on the list, not a measurement: every (geometry class (NM, NW), tile-count class 1 / 2 / 3 / >= 4,
    0 / 1 / 15 padded rows, model instantiation) combination is present, so trimming cannot silently drop one; and
    the axes the sweeps promise are all there."""
    geos = {gc.geometry(d) for d in range(1, 1025)}
    assert geos == {(1, 1), (2, 1), (4, 1), (8, 1), (4, 4), (8, 4), (8, 8)}
    have = {(gc.geometry(c.d), gc.tile_class(c.n), gc.padded_rows(c.n), gc.instantiation(c.kind)) for c in gc.CASES}
    want = {(g, t, p, i) for g in geos for t in (1, 2, 3, 4) for p in (0, 1, 15) for i in ("logistic", "linear/probit")}
    assert not want - have, sorted(want - have)
    for kind in gc.KINDS:
        mine = [c for c in gc.CASES if c.kind == kind]
        assert {1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65} <= {c.n for c in mine}
        assert {1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024} <= {c.d for c in mine}
        assert {1, 15, 16, 17, 33, 65} <= {c.C for c in mine}
        assert {c.d for c in mine if c.n == 65} >= {8, 128, 160, 300, 600}
    for d in (16, 32, 64, 128, 256, 512):                                # both sides of every class edge differ
        assert gc.geometry(d) != gc.geometry(d + 1)


def test_case_inputs_are_exact_and_well_formed():
    for kind in gc.KINDS:
        X, Y, Xi, Yi = gc.data(kind, 65, 1024)
        assert np.array_equal(X * 64, Xi) and (X[:, 0] == 1).all() and np.abs(X).max() <= 4
        assert np.array_equal(Xi[:, 7], Xi[:, 5] + Xi[:, 6])
        if kind == "linear":
            assert np.array_equal(Y * 32, Yi) and np.abs(Y).max() <= 2
        else:
            assert set(Y[:2]) == {0.0, 1.0} and set(Y) == {0.0, 1.0}
