/*
 * smmala_oracle.c -- CPU restatement of the metric tensor of the probit / logistic models -- TEST INFRASTRUCTURE ONLY.
 * A part of tests/manifold_oracle.c, which includes oracle/oracle.c before it.
 *
 * The log-target and the gradient come from orc_eval.  Added here, in the order the kernels document
 * (mcmc.jl_amd/csrc/kernels/smmala.hip): the tensor, the Cholesky factor, the inverse from the
 * factor, the matvecs and quadratic forms.  Matrices are packed lower rows, element (r, c), c <= r, at
 * [r(r+1)/2 + c], chain-strided like the RAM factor.  The sampler's step (reference src/samplers/SMMALA.jl:39-123) is
 * pmala_oracle.c's driver without the correction term.
 */
#define SMM_MAXD 16
#define SMM_NR (SMM_MAXD * (SMM_MAXD + 1) / 2)

static int smm_tri(int r, int c) { return r * (r + 1) / 2 + c; }
static int smm_symi(int r, int c) { return r >= c ? smm_tri(r, c) : smm_tri(c, r); }

/* evalallt: lp and gradient from orc_eval; G[a][b], b <= a: the fma chain over the observations in ascending order,
   from zero, of fma(X[i][a], RN(v_i X[i][b]), .), then 1 / prior_sigma^2 on the diagonal */
static double smm_evalallt(const orc_model* m, const double* x, double* g, double* G) {
    const int d = m->d;
    double tmp[3 * 16 + 16];
    const double lp = orc_eval(m, x, g, tmp, 0);
    for (int k = 0; k < d * (d + 1) / 2; ++k) G[k] = 0.0;
    for (int64_t i = 0; i < m->n; ++i) {
        const double* Xi = m->X + (size_t)i * d;
        double eta = 0.0;                                   /* k-slice e, row q <-> coordinate 4q + e */
        for (int e = 0; e < 4; ++e)
            for (int q = 0; q < 4; ++q) {
                const int k = 4 * q + e;
                eta = fma(k < d ? Xi[k] : 0.0, k < d ? x[k] : 0.0, eta);
            }
        const double y = m->Y[i];
        double v;
        if (m->kind == ORC_MODEL_PROBIT) {                  /* examples/probit_regression.jl:44-49 */
            const double la = orc_normlogcdf(eta), lb = orc_normlogcdf(-eta);
            v = orc_exp(((-(eta * eta) - la) - lb) - ORC_LOG2PI);
        } else {                                            /* expected Fisher information: p (1 - p) */
            double term, r;
            orc_logi(eta, (y >= 0.5) ? m->link_sign : -m->link_sign, &term, &r);
            const double sig = fabs(r);
            v = sig * (1.0 - sig);
        }
        for (int a = 0; a < d; ++a)
            for (int b = 0; b <= a; ++b) G[smm_tri(a, b)] = fma(Xi[a], v * Xi[b], G[smm_tri(a, b)]);
    }
    const double sp = m->prior_sigma;
    const double ip = 1.0 / (sp * sp);
    for (int a = 0; a < d; ++a) G[smm_tri(a, a)] = G[smm_tri(a, a)] + ip;
    return lp;
}

/* in-place Cholesky factor (lower) of the packed SPD matrix W; returns sum_j log L[j][j], NaN on a pivot <= 0 or not
   finite (the column then takes the pivot 1) */
static double smm_chol(double* W, int d) {
    double ld = 0.0;
    int bad = 0;
    for (int j = 0; j < d; ++j) {
        double s = W[smm_tri(j, j)];
        for (int k = 0; k < j; ++k) s = fma(-W[smm_tri(j, k)], W[smm_tri(j, k)], s);
        const int ok = s > 0.0 && s < INFINITY;
        if (!ok) bad = 1;
        const double ljj = sqrt(ok ? s : 1.0);
        ld = ld + orc_log(ljj);
        for (int i = j + 1; i < d; ++i) {
            double t = W[smm_tri(i, j)];
            for (int k = 0; k < j; ++k) t = fma(-W[smm_tri(i, k)], W[smm_tri(j, k)], t);
            W[smm_tri(i, j)] = t / ljj;
        }
        W[smm_tri(j, j)] = ljj;
    }
    return bad ? NAN : ld;
}

/* lower triangle of (L L')^-1, column by column: forward then backward substitution */
static void smm_inverse(const double* L, int d, double* out) {
    double y[SMM_MAXD];
    for (int j = 0; j < d; ++j) {
        for (int i = j; i < d; ++i) {
            double t = i == j ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) t = fma(-L[smm_tri(i, k)], y[k], t);
            y[i] = t / L[smm_tri(i, i)];
        }
        for (int i = d - 1; i >= j; --i) {
            double t = y[i];
            for (int k = i + 1; k < d; ++k) t = fma(-L[smm_tri(k, i)], y[k], t);
            y[i] = t / L[smm_tri(i, i)];
            out[smm_tri(i, j)] = y[i];
        }
    }
}

static void smm_symv(const double* M, const double* v, int d, double* out) {
    for (int r = 0; r < d; ++r) {
        double t = 0.0;
        for (int c = 0; c < d; ++c) t = fma(M[smm_symi(r, c)], v[c], t);
        out[r] = t;
    }
}

/* e' (M / h) e: lane quarter q sums its rows 4q + e in order, the quarters combine as (p0 + p2) + (p1 + p3) */
static double smm_quad(const double* M, const double* ev, int d, double h) {
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < d; ++r) {
        double t = 0.0;
        for (int c = 0; c < d; ++c) t = fma(M[smm_symi(r, c)] / h, ev[c], t);
        p[r >> 2] = fma(ev[r], t, p[r >> 2]);
    }
    return (p[0] + p[2]) + (p[1] + p[3]);
}

/* chain-strided <-> contiguous */
static void smm_get(const double* src, int64_t C, int64_t c, int n, double* dst) {
    for (int k = 0; k < n; ++k) dst[k] = src[(size_t)k * C + c];
}
static void smm_put(double* dst, int64_t C, int64_t c, int n, const double* src) {
    for (int k = 0; k < n; ++k) dst[(size_t)k * C + c] = src[k];
}

/* mcmc_model_eval_tensor: xs [d][C] -> lp [C], grad [d][C], G [d(d+1)/2][C] */
void orc_smm_evalallt(const orc_model* m, int64_t C, const double* xs, double* lp, double* grad, double* G) {
    const int d = m->d, nr = d * (d + 1) / 2;
    for (int64_t c = 0; c < C; ++c) {
        double x[SMM_MAXD], g[SMM_MAXD], Gc[SMM_NR];
        smm_get(xs, C, c, d, x);
        lp[c] = smm_evalallt(m, x, g, Gc);
        if (grad) smm_put(grad, C, c, d, g);
        smm_put(G, C, c, nr, Gc);
    }
}
