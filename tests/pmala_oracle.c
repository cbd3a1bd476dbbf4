/*
 * pmala_oracle.c -- CPU restatement of the derivatives of the metric tensor of the probit / logistic models and of the
 * PMALA sampler (reference src/samplers/PMALA.jl:42-141) -- TEST INFRASTRUCTURE ONLY.
 *
 * Includes tests/smmala_oracle.c unchanged (and through it oracle/oracle.c): the log-target, gradient, tensor, Cholesky
 * factor, inverse, matvec and quadratic form are SMMALA's.  Added here, in the order mcmc.jl_amd/csrc/kernels/pmala.hip
 * documents: the weight's derivative, the d slabs of dG, the fused drift correction
 * c = invG X' (w o qf) and the sampler's step.  dG is d slabs, each packed like G.
 */
#include "smmala_oracle.c"

#define ORC_PMALA 8

typedef struct {
    double* x;        /* [d][C] */
    double* lp;       /* [C] */
    double* g;        /* [d][C] */
    double* G;        /* [d(d+1)/2][C] */
    double* invG;     /* [d(d+1)/2][C] */
    double* ft;       /* [d][C]  firstTerm = invG grad */
    double* c;        /* [d][C]  sum(secondTerm, 2) */
    double* t_step;   /* [C] */
    int32_t* t_acc;
    int32_t* t_prop;
    int64_t* n_evals;
} pm_state;

/* eta of observation row Xi: k-slice e, row q <-> coordinate 4q + e (smm_evalallt's chain) */
static double pm_eta(const double* Xi, const double* x, int d) {
    double eta = 0.0;
    for (int e = 0; e < 4; ++e)
        for (int q = 0; q < 4; ++q) {
            const int k = 4 * q + e;
            eta = fma(k < d ? Xi[k] : 0.0, k < d ? x[k] : 0.0, eta);
        }
    return eta;
}

/* w = dv / d eta.  Probit: examples/probit_regression.jl:52-68 as written; logistic: (v (1 - 2 sig)) (-wt), sig = |r|
   of orc_logi, wt = s (2y - 1) */
static double pm_dw(const orc_model* m, double eta, double y) {
    if (m->kind == ORC_MODEL_PROBIT) {
        const double la = orc_normlogcdf(eta), lb = orc_normlogcdf(-eta);
        const double e2 = eta * eta;
        const double A = (-(e2 + ORC_LOG2PI)) / 2.0;
        const double v01 = orc_exp((((-e2) - 2.0 * la) - lb) - ORC_LOG2PI);
        return v01 * (orc_exp(A - lb) - 2.0 * (orc_exp(A) + eta * orc_exp(la)));
    }
    const double wt = (y >= 0.5) ? m->link_sign : -m->link_sign;
    double term, r;
    orc_logi(eta, wt, &term, &r);
    const double sig = fabs(r);
    const double v = sig * (1.0 - sig);
    return (v * (1.0 - 2.0 * sig)) * (-wt);
}

/* dG[i][a][b], b <= a: the fma chain over the observations in ascending order, from zero, of
   fma(X[o][a], RN(RN(w_o X[o][i]) X[o][b]), .) */
static void pm_dtensor(const orc_model* m, const double* x, double* dG) {
    const int d = m->d, nr = d * (d + 1) / 2;
    for (int k = 0; k < d * nr; ++k) dG[k] = 0.0;
    for (int64_t o = 0; o < m->n; ++o) {
        const double* Xo = m->X + (size_t)o * d;
        const double w = pm_dw(m, pm_eta(Xo, x, d), m->Y[o]);
        for (int i = 0; i < d; ++i) {
            const double wi = w * Xo[i];
            double* S = dG + (size_t)i * nr;
            for (int a = 0; a < d; ++a)
                for (int b = 0; b <= a; ++b) S[smm_tri(a, b)] = fma(Xo[a], wi * Xo[b], S[smm_tri(a, b)]);
        }
    }
}

/* the fused correction c = invG (X' (w o qf)), qf_o = x_o' invG x_o (pmala.hip's header):
   M[j] = fma chain over (e, q') of fma(invG[j][4q' + e], X[o][4q' + e], .); P[j] = RN(M[j] X[o][j]);
   s_q = ((P[q] + P[q+4]) + P[q+8]) + P[q+12]; qf = ((s_0 + s_1) + s_2) + s_3 from +0 (one MFMA with A = 1);
   u[k] = fma chain over the observations of fma(X[o][k], RN(w_o qf_o), .); c = symv(invG, u) */
static void pm_corr(const orc_model* m, const double* x, const double* iG, double* c) {
    const int d = m->d;
    double u[SMM_MAXD];
    for (int k = 0; k < d; ++k) u[k] = 0.0;
    for (int64_t o = 0; o < m->n; ++o) {
        const double* Xo = m->X + (size_t)o * d;
        const double w = pm_dw(m, pm_eta(Xo, x, d), m->Y[o]);
        double P[16];
        for (int j = 0; j < 16; ++j) {
            double M = 0.0;
            for (int e = 0; e < 4; ++e)
                for (int q = 0; q < 4; ++q) {
                    const int k = 4 * q + e;
                    const int ok = j < d && k < d;
                    M = fma(ok ? iG[smm_symi(j, k)] : 0.0, k < d ? Xo[k] : 0.0, M);
                }
            P[j] = M * (j < d ? Xo[j] : 0.0);
        }
        double qf = 0.0;
        for (int q = 0; q < 4; ++q) {
            const double s = ((P[q] + P[q + 4]) + P[q + 8]) + P[q + 12];
            qf = fma(1.0, s, qf);
        }
        const double wq = w * qf;
        for (int k = 0; k < d; ++k) u[k] = fma(Xo[k], wq, u[k]);
    }
    smm_symv(iG, u, d, c);
}

/* mcmc_model_eval_dtensor: xs [d][C] -> lp [C], grad [d][C], G [nr][C] (any may be NULL), dG [d][nr][C] */
void orc_pm_evalalldt(const orc_model* m, int64_t C, const double* xs, double* lp, double* grad, double* G,
                      double* dG) {
    const int d = m->d, nr = d * (d + 1) / 2;
    for (int64_t c = 0; c < C; ++c) {
        double x[SMM_MAXD], g[SMM_MAXD], Gc[SMM_NR], dGc[SMM_MAXD * SMM_NR];
        smm_get(xs, C, c, d, x);
        const double l = smm_evalallt(m, x, g, Gc);
        if (lp) lp[c] = l;
        if (grad) smm_put(grad, C, c, d, g);
        if (G) smm_put(G, C, c, nr, Gc);
        pm_dtensor(m, x, dGc);
        smm_put(dG, C, c, d * nr, dGc);
    }
}

/* the inverse of packed SPD matrices by the kernels' Cholesky route: G [nr][C] -> invG [nr][C] */
void orc_pm_inverse(int d, int64_t C, const double* G, double* invG) {
    const int nr = d * (d + 1) / 2;
    for (int64_t c = 0; c < C; ++c) {
        double W[SMM_NR], iG[SMM_NR];
        smm_get(G, C, c, nr, W);
        (void)smm_chol(W, d);
        smm_inverse(W, d, iG);
        smm_put(invG, C, c, nr, iG);
    }
}

/* the fused correction at xs [d][C] with invG [nr][C] -> cs [d][C] */
void orc_pm_corr(const orc_model* m, int64_t C, const double* xs, const double* invG, double* cs) {
    const int d = m->d, nr = d * (d + 1) / 2;
    for (int64_t c = 0; c < C; ++c) {
        double x[SMM_MAXD], iG[SMM_NR], cv[SMM_MAXD];
        smm_get(xs, C, c, d, x);
        smm_get(invG, C, c, nr, iG);
        pm_corr(m, x, iG, cv);
        smm_put(cs, C, c, d, cv);
    }
}

/* evaluation of chain c at st->x; derive: also invG, firstTerm and the correction.  Returns 1 for a start out of
   support or a failed pivot. */
static int pm_eval_state(const orc_model* m, int64_t C, int64_t c, pm_state* st, int derive) {
    const int d = m->d, nr = d * (d + 1) / 2;
    double x[SMM_MAXD] = {0.0}, g[SMM_MAXD], Gc[SMM_NR], W[SMM_NR], iG[SMM_NR], ft[SMM_MAXD], cv[SMM_MAXD];
    smm_get(st->x, C, c, d, x);
    const double lp = smm_evalallt(m, x, g, Gc);
    st->lp[c] = lp;
    smm_put(st->g, C, c, d, g);
    smm_put(st->G, C, c, nr, Gc);
    int bad = !isfinite(lp);
    if (derive) {
        memcpy(W, Gc, sizeof(double) * nr);
        if (isnan(smm_chol(W, d))) bad = 1;
        smm_inverse(W, d, iG);
        smm_symv(iG, g, d, ft);
        pm_corr(m, x, iG, cv);
        smm_put(st->invG, C, c, nr, iG);
        smm_put(st->ft, C, c, d, ft);
        smm_put(st->c, C, c, d, cv);
    }
    return bad;
}

/* SamplerTask initialisation (PMALA.jl:70-82) */
int64_t orc_pm_init(const orc_model* m, const orc_sampler* s, int64_t C, pm_state* st) {
    int64_t bad = 0;
    for (int64_t c = 0; c < C; ++c) {
        bad += pm_eval_state(m, C, c, st, 1);
        if (s->tuner) {
            st->t_step[c] = s->drift_step;
            st->t_acc[c] = 0;
            st->t_prop[c] = 0;
        }
        if (st->n_evals) st->n_evals[c] = 1;
    }
    return bad;
}

/* the :reset hook as written (PMALA.jl:63-66): pars, logTarget, grad and G at x; invG, firstTerm and secondTerm stay */
void orc_pm_set_state(const orc_model* m, int64_t C, pm_state* st, const double* x) {
    for (int64_t c = 0; c < C; ++c) {
        for (int j = 0; j < m->d; ++j) st->x[(size_t)j * C + c] = x[(size_t)j * C + c];
        (void)pm_eval_state(m, C, c, st, 0);
        if (st->n_evals) st->n_evals[c] += 1;
    }
}

static void pm_chain(const orc_model* m, const orc_sampler* s, uint64_t seed, uint32_t chain, int64_t c, int64_t C,
                     int64_t step0, int64_t burnin, int64_t thinning, int64_t len, int64_t tuner_burnin, pm_state* st,
                     double* samples, double* grads, uint8_t* acc_out) {
    const int d = m->d, nr = d * (d + 1) / 2;
    double x[SMM_MAXD], g[SMM_MAXD], ft[SMM_MAXD], cv[SMM_MAXD], G[SMM_NR], iG[SMM_NR];
    double xp[SMM_MAXD], gp[SMM_MAXD], pft[SMM_MAXD], pc[SMM_MAXD], pG[SMM_NR], piG[SMM_NR], W[SMM_NR];
    double z[SMM_MAXD + 4], ev[SMM_MAXD];
    smm_get(st->x, C, c, d, x);
    smm_get(st->g, C, c, d, g);
    smm_get(st->ft, C, c, d, ft);
    smm_get(st->c, C, c, d, cv);
    smm_get(st->G, C, c, nr, G);
    smm_get(st->invG, C, c, nr, iG);
    double lp = st->lp[c];
    double h = s->tuner ? st->t_step[c] : s->drift_step;
    int32_t n_acc = s->tuner ? st->t_acc[c] : 0, n_prop = s->tuner ? st->t_prop[c] : 0;
    for (int64_t t = 0; t < len; ++t) {
        const int64_t i = step0 + t + 1;
        if (s->tuner) n_prop += 1;
        const double half = h / 2.0;
        for (int k = 0; k < nr; ++k) W[k] = h * iG[k];
        const double ld1 = smm_chol(W, d);                                    /* U' = chol(h invG)' */
        int bad = isnan(ld1);
        orc_normals(seed, chain, (uint32_t)i, d, z);
        for (int r = 0; r < d; ++r) {
            double u = 0.0;
            for (int q = 0; q <= r; ++q) u = fma(W[smm_tri(r, q)], z[q], u);
            const double pm = x[r] + half * (ft[r] - cv[r]);                  /* PMALA.jl:94 */
            xp[r] = pm + u;                                                   /* PMALA.jl:98 */
            ev[r] = pm - xp[r];
        }
        const double qf = (-ld1) - 0.5 * smm_quad(G, ev, d, h);               /* probNewGivenOld */
        const double lpp = smm_evalallt(m, xp, gp, pG);                       /* PMALA.jl:101 */
        const int oos = !isfinite(lpp);
        memcpy(W, pG, sizeof(double) * nr);
        if (isnan(smm_chol(W, d))) bad = 1;
        smm_inverse(W, d, piG);                                               /* PMALA.jl:106 */
        smm_symv(piG, gp, d, pft);                                            /* PMALA.jl:107 */
        pm_corr(m, xp, piG, pc);                                              /* PMALA.jl:108-111 */
        for (int k = 0; k < nr; ++k) W[k] = h * piG[k];
        const double ld2 = smm_chol(W, d);
        if (isnan(ld2)) bad = 1;
        for (int r = 0; r < d; ++r) ev[r] = (xp[r] + half * (pft[r] - pc[r])) - x[r];   /* PMALA.jl:114, 117 */
        const double qb = (-ld2) - 0.5 * smm_quad(pG, ev, d, h);              /* probOldGivenNew */
        const double ratio = ((lpp + qb) - lp) - qf;                          /* PMALA.jl:119 */
        const int acc = !(bad || oos) && orc_mh_short_circuit(seed, chain, (uint32_t)i, ratio);
        if (acc) {
            memcpy(x, xp, sizeof(double) * d);
            memcpy(g, gp, sizeof(double) * d);
            memcpy(ft, pft, sizeof(double) * d);
            memcpy(cv, pc, sizeof(double) * d);
            memcpy(G, pG, sizeof(double) * nr);
            memcpy(iG, piG, sizeof(double) * nr);
            lp = lpp;
            if (s->tuner) n_acc += 1;
        }
        int64_t kk;
        if (orc_kept(i - step0, burnin, thinning, len, &kk)) {
            if (samples)
                for (int q = 0; q < d; ++q) samples[((size_t)kk * d + q) * C + c] = x[q];
            if (grads)
                for (int q = 0; q < d; ++q) grads[((size_t)kk * d + q) * C + c] = g[q];
            if (acc_out) acc_out[(size_t)kk * C + c] = (uint8_t)acc;
        }
        if (s->tuner && i <= tuner_burnin && (i % s->adapt_step) == 0) {      /* PMALA.jl:131-137 */
            h = h * orc_tune_factor(n_acc, n_prop, s->target_rate);
            n_acc = 0;
            n_prop = 0;
        }
    }
    smm_put(st->x, C, c, d, x);
    smm_put(st->g, C, c, d, g);
    smm_put(st->ft, C, c, d, ft);
    smm_put(st->c, C, c, d, cv);
    smm_put(st->G, C, c, nr, G);
    smm_put(st->invG, C, c, nr, iG);
    st->lp[c] = lp;
    if (s->tuner) {
        st->t_step[c] = h;
        st->t_acc[c] = n_acc;
        st->t_prop[c] = n_prop;
    }
    if (st->n_evals) st->n_evals[c] += len;
}

/* run_serialmc of chains [c_begin, c_end) of a batch of C; outputs as orc_smm_run's */
void orc_pm_run(const orc_model* m, const orc_sampler* s, uint64_t seed, int64_t chain0, int64_t C, int64_t c_begin,
                int64_t c_end, int64_t step0, int64_t burnin, int64_t thinning, int64_t len, int64_t tuner_burnin,
                pm_state* st, double* samples, double* grads, uint8_t* acc_out, int nthreads) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads > 0 ? nthreads : 1)
#endif
    for (int64_t c = c_begin; c < c_end; ++c)
        pm_chain(m, s, seed, (uint32_t)(chain0 + c), c, C, step0, burnin, thinning, len, tuner_burnin, st, samples,
                 grads, acc_out);
    (void)nthreads;
}
