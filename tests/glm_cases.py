"""Shared regression cases for test_glm_exact.py (CPU, against an exact / mpmath reference) and test_glm_shapes.py
(GPU, bitwise against the oracle): observation counts at every 16-observation tile edge, widths on both sides of
every slice-geometry edge (glm.hip mcmc_glm_shape), chain counts around one 16-chain tile, four model kinds.

No RNG: every input is an exact dyadic rational built from integer arithmetic, the same on every machine and numpy
version.  X[i][j] = ((37 i + 101 j + 13) mod 257 - 128) / 64, column 0 all ones, and every column j = 3 (mod 4) the
exact sum of the two columns before it, which is what lets the cancelling regime hold on every row (see betas()).
The integer forms (Xi = 64 X, Yi, the betas' numerators) travel with the float arrays so that a reference can form
eta = X beta exactly.
"""
from collections import namedtuple

import numpy as np

import mcmchip as mc

KINDS = ("logistic", "logistic_neg", "linear", "probit")    # logistic_neg: prob = 1/(1+exp(+X*vars)), link_sign -1
# 47 and 63 are not among the tile edges themselves: they give the one-padded-row case at three and four tiles
N_SWEEP = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65)
D_SWEEP = (1, 2, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024)
C_SWEEP = (1, 15, 16, 17, 33, 65)
# one width per kernel family for the n sweep: 8 (single slice, NM = 1), 128 (single slice, NM = 8), 160 (4 x 64),
# 300 (4 x 128, two tiles a workgroup), 600 (8 x 128); 24 and 48 give NM = 2 and 4 their tile x padding classes
N_SWEEP_D = (8, 24, 48, 128, 160, 300, 600)
SAMPLER_N_SWEEP_D = (8, 128, 160, 300, 600)
D_SWEEP_N = (17, 48)
C_SWEEP_AT = ((8, 17), (300, 33))
EVAL_C = 3                                                   # columns per regime outside the C sweep
REGIMES = ("moderate", "cancelling", "saturating")
KBIG = 1 << 20                                               # the cancelling regime's +- magnitude

PRIOR_SIGMA = {"logistic": 1.0, "logistic_neg": 1.5, "linear": 3.0, "probit": 10.0}
NOISE_SIGMA = 0.75                                           # linear
# largest |eta| of the saturating regime: logistic 30 (below the reference's -Inf rule at 36.7), probit 8, linear
# 50 noise sigmas of residual less the largest |y| = 2
SATURATION = {"logistic": 30.0, "logistic_neg": 30.0, "probit": 8.0, "linear": 50 * NOISE_SIGMA - 2.0}

Case = namedtuple("Case", "kind n d C")


def case_id(c):
    return f"{c.kind}-n{c.n}-d{c.d}-C{c.C}"


def _cases():
    out = []
    for kind in KINDS:
        for d in N_SWEEP_D:
            out += [Case(kind, n, d, EVAL_C) for n in N_SWEEP]
        for n in D_SWEEP_N:
            out += [Case(kind, n, d, EVAL_C) for d in D_SWEEP]
        for d, n in C_SWEEP_AT:
            out += [Case(kind, n, d, C) for C in C_SWEEP]
    return list(dict.fromkeys(out))


CASES = _cases()


def geometry(d):
    """(NM, NW) of mcmc_glm_shape, restated: d <= 128 one slice of 16 NM coordinates (NM a power of two), d <= 256
    four slices of 64, above that four or eight slices of 128."""
    if d <= 128:
        nm = 1
        while 16 * nm < d:
            nm *= 2
        return nm, 1
    if d <= 256:
        return 4, 4
    return 8, (4 if d <= 512 else 8)


def tile_class(n):
    return min((n + 15) // 16, 4)                            # 1, 2, 3, or 4 for "four or more"


def padded_rows(n):
    return -n % 16


def instantiation(kind):
    """The kernels' two model instantiations: the logistic one (bound column, det_logi) and the linear / probit one."""
    return "logistic" if kind.startswith("logistic") else "linear/probit"


def data(kind, n, d):
    """(X [n][d], Y [n], Xi = 64 X as int64, Yi): Y is 0/1 (both classes from n = 2 on; Yi = Y) for the logistic and
    probit kinds, ((53 i + 7) mod 129 - 64) / 32 (Yi = 32 Y) for the linear one."""
    i, j = np.arange(n, dtype=np.int64)[:, None], np.arange(d, dtype=np.int64)[None, :]
    Xi = (37 * i + 101 * j + 13) % 257 - 128
    Xi[:, 0] = 64
    for k in range(3, d, 4):
        Xi[:, k] = Xi[:, k - 2] + Xi[:, k - 1]
    i = i[:, 0]
    Yi = (53 * i + 7) % 129 - 64 if kind == "linear" else (i % 3 != 1).astype(np.int64)
    Y = Yi / 32.0 if kind == "linear" else Yi.astype(np.float64)
    return Xi / 64.0, Y, Xi, Yi


def make_model(kind, n, d, init=None):
    X, Y, _, _ = data(kind, n, d)
    init = np.zeros(d) if init is None else init
    if kind == "linear":
        t = mc.LinearRegression(X, Y, prior_sigma=PRIOR_SIGMA[kind], noise_sigma=NOISE_SIGMA)
    elif kind == "probit":
        t = mc.ProbitRegression(X, Y, prior_sigma=PRIOR_SIGMA[kind])
    else:
        t = mc.LogisticRegression(X, Y, prior_sigma=PRIOR_SIGMA[kind], link_sign=-1.0 if kind == "logistic_neg" else 1.0)
    return mc.model(t, vars=init, gradient=True)


def _scaled(Xi, bi, top):
    """The shift k (beta = bi 2^-k) that puts max |eta| in (top / 2, top]; eta = Xi bi / 64 2^-k exactly."""
    H = np.abs(Xi @ bi).max()
    assert 0 < H < 1 << 40
    k = 0
    while H / 64.0 / 2.0**k > top:
        k += 1
    while H / 64.0 / 2.0**k <= top / 2:
        k -= 1
    return k


def betas(case, regime):
    """(B [d][C] float64, num [d][C] Python ints, k): B = num 2^-k exactly.

    moderate: small integers ((29 j + 71 c + 5) mod 61 - 30) scaled by a power of two so that max |eta| lies in
    (1.5, 3].  saturating: another such pattern scaled so that max |eta| lies in (SATURATION / 2, SATURATION].
    cancelling: a moderate pattern plus, on every column triple (j - 2, j - 1, j), j = 3 (mod 4), the amounts
    (+K m, +K m, -K m), K = 2^20, m in {1, 2, 3}: X's column j is the exact sum of the other two, so the triple adds
    exactly nothing to eta while sum_j |x_ij beta_j| grows by K m (|x_i,j-2| + |x_i,j-1| + |x_ij|); for d < 4 there
    is no triple and the regime is a second moderate one."""
    _, _, Xi, _ = data(case.kind, case.n, case.d)
    j, c = np.arange(case.d, dtype=np.int64)[:, None], np.arange(case.C, dtype=np.int64)[None, :]
    a, b, m = {"moderate": (29, 71, 5), "cancelling": (31, 67, 11), "saturating": (23, 73, 17)}[regime]
    bi = (a * j + b * c + m) % 61 - 30
    if case.d >= 3:
        bi[0] = (bi[0] + 30) % 3 - 1                         # the intercept (column of ones) stays small
    k = _scaled(Xi, bi, SATURATION[case.kind] if regime == "saturating" else 3.0)
    num = bi.astype(object) * (1 << max(-k, 0))
    k = max(k, 0)
    if regime == "cancelling":
        for t in range(3, case.d, 4):
            for cc in range(case.C):
                big = KBIG * (1 + (t // 4 + cc) % 3) << k
                num[t - 2, cc] += big
                num[t - 1, cc] += big
                num[t, cc] -= big
    B = np.array([[float(v) for v in row] for row in num]) / 2.0**k
    assert all(int(B[r, q] * 2**k) == num[r, q] for r in range(case.d) for q in range(case.C))   # B is exact
    return B, num, k
