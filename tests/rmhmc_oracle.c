/*
 * rmhmc_oracle.c -- CPU restatement of the RMHMC sampler (reference src/samplers/RMHMC.jl:53-183) on the probit /
 * logistic models, and of the frame the trajectory samplers share -- TEST INFRASTRUCTURE ONLY.
 * A part of tests/manifold_oracle.c, after pmala_oracle.c.
 *
 * The log-target, gradient, tensor, Cholesky factor, inverse, matvec, the weight's derivative, the d slabs of dG and
 * the per-observation quadratic form are the earlier parts'.  Added here, in the order
 * mcmc.jl_amd/csrc/kernels/rmhmc.hip documents: the two fused tensor terms X' (w o qf) and
 * X' (w o t^2), the Cholesky solve, the momentum's quadratic form; the state, the HMC-type tuner, the leap count, the
 * counters and the step loop of RMHMC, ERMLMC and RMLMC; and RMHMC's proposal.
 */
#define ORC_TAG_RMHMC 5u

/* log 2 and log pi, the doubles nearest to them (RMHMC.jl:107 writes log(2) + d log(pi), not d log(2 pi)) */
static const double RM_LOG2 = 0x1.62e42fefa39efp-1;
static const double RM_LOGPI = 0x1.250d048e7a1bdp+0;

typedef struct {
    double* x;        /* [d][C] */
    double* lp;       /* [C] */
    double* g;        /* [d][C] */
    double* t_step;   /* [C] */
    int32_t* t_leaps;
    int32_t* t_acc;
    int32_t* t_prop;
    int64_t* n_evals;
} rm_state;

/* the fused terms at x with invG (either output may be NULL):
   u  = X' (w o qf), qf_o = x_o' invG x_o: pm_corr's chains; u[r] = trace(invG dG_r);
   u2 = X' (w o t^2), t = X v by eta's chain (k-slice e, row q <-> coordinate 4q + e): u2[r] = v' dG_r v; the weight is
        RN(w_o RN(t_o t_o)), each u2[k] the fma chain over the observations in ascending order from zero */
static void rm_terms(const orc_model* m, const double* x, const double* iG, const double* v, double* u, double* u2) {
    const int d = m->d;
    for (int k = 0; k < d; ++k) {
        if (u) u[k] = 0.0;
        if (u2) u2[k] = 0.0;
    }
    for (int64_t o = 0; o < m->n; ++o) {
        const double* Xo = m->X + (size_t)o * d;
        const double w = pm_dw(m, pm_eta(Xo, x, d), m->Y[o]);
        if (u) {
            const double wq = w * pm_qform(Xo, iG, d);
            for (int k = 0; k < d; ++k) u[k] = fma(Xo[k], wq, u[k]);
        }
        if (u2) {
            const double t = pm_eta(Xo, v, d);
            const double wt = w * (t * t);
            for (int k = 0; k < d; ++k) u2[k] = fma(Xo[k], wt, u2[k]);
        }
    }
}

/* (L z)[r]: the fma chain over c <= r from zero (cholG' randn, the chain SMMALA and PMALA form) */
static void rm_lmul(const double* L, const double* z, int d, double* out) {
    for (int r = 0; r < d; ++r) {
        double u = 0.0;
        for (int c = 0; c <= r; ++c) u = fma(L[smm_tri(r, c)], z[c], u);
        out[r] = u;
    }
}

/* (L L') \ b: forward y[i] = (b[i] then fma(-L[i][k], y[k], .) over k = 0..i-1) / L[i][i]; backward from i = d-1:
   x[i] = (y[i] then fma(-L[k][i], x[k], .) over k = i+1..d-1) / L[i][i] (smm_inverse's chains with b for the unit
   column) */
static void rm_solve(const double* L, const double* b, int d, double* out) {
    double y[SMM_MAXD];
    for (int i = 0; i < d; ++i) {
        double t = b[i];
        for (int k = 0; k < i; ++k) t = fma(-L[smm_tri(i, k)], y[k], t);
        y[i] = t / L[smm_tri(i, i)];
    }
    for (int i = d - 1; i >= 0; --i) {
        double t = y[i];
        for (int k = i + 1; k < d; ++k) t = fma(-L[smm_tri(k, i)], y[k], t);
        y[i] = t / L[smm_tri(i, i)];
        out[i] = y[i];
    }
}

/* a' b: lane quarter q's fma chain over its rows 4q + e from zero, the quarters as (p0 + p2) + (p1 + p3) */
static double rm_dot(const double* a, const double* b, int d) {
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < d; ++r) p[r >> 2] = fma(a[r], b[r], p[r >> 2]);
    return (p[0] + p[2]) + (p[1] + p[3]);
}

/* RMHMC.jl:107, 162 with ld = sum(log(diag(cholG))) and quad = momentum' invG momentum, left to right as written */
static double rm_hamiltonian(double lp, double ld, double quad, int d) {
    return ((-lp) + 0.5 * ((RM_LOG2 + (double)d * RM_LOGPI) + 2.0 * ld)) + quad / 2.0;
}

/* timeStep and nRandomLeaps of (chain, step): block (chain, step, 0, TAG_RMHMC); the uniform from words 0, 1, the
   normal the cosine branch of Box-Muller on words 2, 3 */
static void rm_draws(uint64_t seed, uint32_t chain, uint32_t step, double* u, double* nz) {
    uint32_t w[4];
    orc_block(seed, chain, step, 0u, ORC_TAG_RMHMC, w);
    *u = orc_uniform52(w[0], w[1]);
    double s, c;
    orc_sincos2pi_u32(w[3], &s, &c);
    *nz = orc_bm_radius_u32(w[2]) * c;
}

static int rm_all_finite(const double* v, int d) {
    for (int k = 0; k < d; ++k)
        if (!isfinite(v[k])) return 0;
    return 1;
}

/* one generalised leapfrog (RMHMC.jl:121-154) from (xp, mom, gcur, iG, tr); returns 1 when the trajectory fails (then
   the step is rejected and nothing it left is read) */
static int rm_leap(const orc_model* m, int n_newton, double eh, double* xp, double* mom, double* gcur, double* iG,
                   double* tr, double* lpp, double* ldp) {
    const int d = m->d, nr = d * (d + 1) / 2;
    double lm[SMM_MAXD], v[SMM_MAXD], v1[SMM_MAXD], v2[SMM_MAXD], u2[SMM_MAXD], lx[SMM_MAXD], cand[SMM_MAXD];
    double gk[SMM_MAXD], G[SMM_NR], W[SMM_NR];
    memcpy(lm, mom, sizeof(double) * d);
    for (int k = 0; k < n_newton; ++k) {                                     /* RMHMC.jl:123-129 */
        smm_symv(iG, lm, d, v);
        rm_terms(m, xp, iG, v, NULL, u2);
        for (int r = 0; r < d; ++r) lm[r] = mom[r] + eh * ((gcur[r] - 0.5 * tr[r]) + 0.5 * u2[r]);
    }
    memcpy(mom, lm, sizeof(double) * d);
    smm_symv(iG, mom, d, v2);                                                /* RMHMC.jl:132 */
    memcpy(lx, xp, sizeof(double) * d);
    for (int k = 0; k < n_newton; ++k) {                                     /* RMHMC.jl:134-138 */
        if (!isfinite(smm_evalallt(m, lx, gk, G))) return 1;
        memcpy(W, G, sizeof(double) * nr);
        if (isnan(smm_chol(W, d))) return 1;
        rm_solve(W, mom, d, v1);
        for (int r = 0; r < d; ++r) cand[r] = xp[r] + eh * (v1[r] + v2[r]);
        if (!rm_all_finite(cand, d)) return 1;
        memcpy(lx, cand, sizeof(double) * d);
    }
    memcpy(xp, lx, sizeof(double) * d);
    *lpp = smm_evalallt(m, xp, gcur, G);                                     /* RMHMC.jl:141, 153, 158 */
    if (!isfinite(*lpp)) return 1;
    memcpy(W, G, sizeof(double) * nr);
    *ldp = smm_chol(W, d);
    if (isnan(*ldp)) return 1;
    smm_inverse(W, d, iG);                                                   /* RMHMC.jl:142 */
    smm_symv(iG, mom, d, v);                                                 /* RMHMC.jl:148 */
    rm_terms(m, xp, iG, v, tr, u2);                                          /* RMHMC.jl:143-151 */
    for (int r = 0; r < d; ++r) mom[r] = mom[r] + eh * ((gcur[r] - 0.5 * tr[r]) + 0.5 * u2[r]);   /* RMHMC.jl:154 */
    return 0;
}

/* SamplerTask initialisation of the trajectory samplers (RMHMC.jl:82-86; ERMLMC's and RMLMC's state is the same) */
int64_t orc_hmc_init(const orc_model* m, const orc_sampler* s, int64_t C, rm_state* st) {
    const int d = m->d;
    int64_t bad = 0;
    for (int64_t c = 0; c < C; ++c) {
        double x[SMM_MAXD] = {0.0}, g[SMM_MAXD], G[SMM_NR];
        smm_get(st->x, C, c, d, x);
        st->lp[c] = smm_evalallt(m, x, g, G);
        smm_put(st->g, C, c, d, g);
        bad += !isfinite(st->lp[c]);
        if (s->tuner) {
            st->t_step[c] = s->leap_step;
            st->t_leaps[c] = (int32_t)s->n_leaps;
            st->t_acc[c] = 0;
            st->t_prop[c] = 0;
        }
        if (st->n_evals) st->n_evals[c] = 0;                /* leapfrogs only, HMC's convention */
    }
    return bad;
}

/* the :reset hook (RMHMC.jl:74-77): pars, logTarget and grad at x; the next step recomputes all geometry from it */
void orc_hmc_set_state(const orc_model* m, int64_t C, rm_state* st, const double* x) {
    const int d = m->d;
    for (int64_t c = 0; c < C; ++c) {
        double xc[SMM_MAXD] = {0.0}, g[SMM_MAXD], G[SMM_NR];
        for (int j = 0; j < d; ++j) st->x[(size_t)j * C + c] = x[(size_t)j * C + c];
        smm_get(st->x, C, c, d, xc);
        st->lp[c] = smm_evalallt(m, xc, g, G);
        smm_put(st->g, C, c, d, g);
        if (st->n_evals) st->n_evals[c] += 1;
    }
}

/* the HMC-type tuner's state of one chain (EmpiricalHMCTune): the sampler's own values where it has no tuner */
typedef struct {
    double eps;
    int64_t nl_fixed;
    int32_t n_acc, n_prop;
} hmc_tune;

static void hmc_tune_load(const orc_sampler* s, const rm_state* st, int64_t c, hmc_tune* tn) {
    tn->eps = s->tuner ? st->t_step[c] : s->leap_step;
    tn->nl_fixed = s->tuner ? (int64_t)st->t_leaps[c] : s->n_leaps;
    tn->n_acc = s->tuner ? st->t_acc[c] : 0;
    tn->n_prop = s->tuner ? st->t_prop[c] : 0;
}

/* RMHMC.jl:174-180, ERMLMC.jl:170-176 */
static void hmc_tune_adapt(const orc_sampler* s, hmc_tune* tn, mf_counters* cn) {
    const int64_t max_leaps = s->max_leaps > 0 ? s->max_leaps : ((int64_t)1 << 20);
    tn->eps = tn->eps * orc_tune_factor(tn->n_acc, tn->n_prop, s->target_rate);
    double nlf = ceil(s->target_path / tn->eps);
    if (nlf > (double)s->max_step) nlf = (double)s->max_step;
    if (nlf > (double)max_leaps) nlf = (double)max_leaps;
    tn->nl_fixed = (int64_t)nlf;
    tn->n_acc = 0;
    tn->n_prop = 0;
    if (cn) {
#ifdef _OPENMP
#pragma omp atomic
#endif
        cn->n_adapt += 1;
    }
}

static void hmc_tune_store(const orc_sampler* s, rm_state* st, int64_t c, const hmc_tune* tn) {
    if (!s->tuner) return;
    st->t_step[c] = tn->eps;
    st->t_leaps[c] = (int32_t)tn->nl_fixed;
    st->t_acc[c] = tn->n_acc;
    st->t_prop[c] = tn->n_prop;
}

/* nRandomLeaps = ceil(u nLeaps) (RMHMC.jl:118) and what the counters keep of it; ts: the step's timeStep, 0 for a
   sampler that draws none */
static int64_t hmc_leap_count(mf_counters* cn, double u, int64_t nl_fixed, double ts) {
    const int64_t nrl = (int64_t)ceil(u * (double)nl_fixed);
    if (cn) {
#ifdef _OPENMP
#pragma omp critical(mf_counters)
#endif
        {
            if (ts > 0.0) cn->n_plus += 1;
            if (ts < 0.0) cn->n_minus += 1;
            if (nrl < cn->nrl_min) cn->nrl_min = nrl;
            if (nrl > cn->nrl_max) cn->nrl_max = nrl;
            if (nrl == 0) cn->n_zero += 1;
        }
    }
    return nrl;
}

/* a sampler's proposal of step i from (x, g, lp) with leapStep eps and nLeaps nl_fixed: the end of its trajectory in
   (xp, gp, *lpp), the leaps it drew in *nrl, whether the trajectory failed in *failed; returns the accept decision */
typedef int (*hmc_propose_fn)(const mf_run* r, uint32_t chain, uint32_t i, double eps, int64_t nl_fixed,
                              const double* x, const double* g, double lp, double* xp, double* gp, double* lpp,
                              int64_t* nrl, int* failed);

/* one chain of a trajectory sampler: everything but the proposal */
static void hmc_chain(const mf_run* r, uint32_t chain, int64_t c, hmc_propose_fn propose) {
    const orc_sampler* s = r->s;
    rm_state* st = (rm_state*)r->st;
    const int64_t C = r->C;
    const int d = r->m->d;
    double x[SMM_MAXD], g[SMM_MAXD], xp[SMM_MAXD], gp[SMM_MAXD];
    smm_get(st->x, C, c, d, x);
    smm_get(st->g, C, c, d, g);
    double lp = st->lp[c];
    hmc_tune tn;
    hmc_tune_load(s, st, c, &tn);
    int64_t n_evals = 0;
    for (int64_t t = 0; t < r->len; ++t) {
        const int64_t i = r->step0 + t + 1;
        if (s->tuner) tn.n_prop += 1;
        double lpp = lp;
        int64_t nrl = 0;
        int failed = 0;
        const int acc = propose(r, chain, (uint32_t)i, tn.eps, tn.nl_fixed, x, g, lp, xp, gp, &lpp, &nrl, &failed);
        n_evals += nrl;
        if (r->cn && failed) {
#ifdef _OPENMP
#pragma omp atomic
#endif
            r->cn->n_failed += 1;
        }
        if (acc) {
            memcpy(x, xp, sizeof(double) * d);
            memcpy(g, gp, sizeof(double) * d);
            lp = lpp;
            if (s->tuner) tn.n_acc += 1;
        }
        mf_store_kept(r, i, c, x, g, acc);
        if (s->tuner && i <= r->tuner_burnin && (i % s->adapt_step) == 0) hmc_tune_adapt(s, &tn, r->cn);
    }
    smm_put(st->x, C, c, d, x);
    smm_put(st->g, C, c, d, g);
    st->lp[c] = lp;
    hmc_tune_store(s, st, c, &tn);
    if (st->n_evals) st->n_evals[c] += n_evals;
}

/* RMHMC's proposal (RMHMC.jl:100-164): the momentum from chol(G), the Hamiltonian, timeStep, the generalised
   leapfrogs and H - H' */
static int rm_propose(const mf_run* r, uint32_t chain, uint32_t i, double eps, int64_t nl_fixed, const double* x,
                      const double* g, double lp, double* xp, double* gp, double* lpp, int64_t* nrl, int* failed) {
    const orc_model* m = r->m;
    const int d = m->d, nr = d * (d + 1) / 2;
    const int n_newton = (int)r->s->t0;
    double mom[SMM_MAXD], v[SMM_MAXD], tr[SMM_MAXD], G[SMM_NR], W[SMM_NR], iG[SMM_NR], g0[SMM_MAXD], z[SMM_MAXD + 4];
    (void)smm_evalallt(m, x, g0, G);                                          /* RMHMC.jl:100 */
    memcpy(W, G, sizeof(double) * nr);
    const double ld0 = smm_chol(W, d);                                        /* RMHMC.jl:102 */
    *failed = isnan(ld0);
    smm_inverse(W, d, iG);                                                    /* RMHMC.jl:101 */
    orc_normals(r->seed, chain, i, d, z);
    rm_lmul(W, z, d, mom);                                                    /* RMHMC.jl:105 */
    smm_symv(iG, mom, d, v);
    const double H = rm_hamiltonian(lp, ld0, rm_dot(mom, v, d), d);           /* RMHMC.jl:107 */
    rm_terms(m, x, iG, NULL, tr, NULL);                                       /* RMHMC.jl:110-114 */
    double u, nz;
    rm_draws(r->seed, chain, i, &u, &nz);
    const double ts = nz > 0.5 ? 1.0 : -1.0;                                  /* RMHMC.jl:117 */
    *nrl = hmc_leap_count(r->cn, u, nl_fixed, ts);                            /* RMHMC.jl:118 */
    const double eh = ts * (eps / 2.0);
    memcpy(xp, x, sizeof(double) * d);
    memcpy(gp, g, sizeof(double) * d);
    double ldp = ld0;
    for (int64_t l = 0; l < *nrl && !*failed; ++l)
        *failed = rm_leap(m, n_newton, eh, xp, mom, gp, iG, tr, lpp, &ldp);
    if (*failed || *nrl <= 0) return 0;
    smm_symv(iG, mom, d, v);
    const double Hp = rm_hamiltonian(*lpp, ldp, rm_dot(mom, v, d), d);        /* RMHMC.jl:161-162 */
    const double ratio = H - Hp;                                              /* RMHMC.jl:164 */
    if (isfinite(ratio)) return orc_mh_short_circuit(r->seed, chain, i, ratio);
    *failed = 1;
    return 0;
}

static void rm_chain(const mf_run* r, uint32_t chain, int64_t c) { hmc_chain(r, chain, c, rm_propose); }

/* the fused terms of one point: x [d], packed invG [nr], v [d] -> u = X' (w o qf), u2 = X' (w o (X v)^2) */
void orc_rm_terms(const orc_model* m, const double* x, const double* iG, const double* v, double* u, double* u2) {
    rm_terms(m, x, iG, v, u, u2);
}

/* (L L') \ b by the kernels' route from packed G [nr]; returns 0 on a failed pivot */
int orc_rm_solve(int d, const double* G, const double* b, double* out) {
    double W[SMM_NR];
    memcpy(W, G, sizeof(double) * (size_t)(d * (d + 1) / 2));
    if (isnan(smm_chol(W, d))) return 0;
    rm_solve(W, b, d, out);
    return 1;
}

/* the trajectory's energy error for the integrator check: from x [d] with momentum mom [d], nl generalised leapfrogs
   of step eps (timeStep = +1); returns H_end - H_start (NaN when the trajectory fails) */
double orc_rm_energy_error(const orc_model* m, const double* x0, const double* mom0, double eps, int64_t nl,
                           int n_newton) {
    const int d = m->d, nr = d * (d + 1) / 2;
    double x[SMM_MAXD], mom[SMM_MAXD], g[SMM_MAXD], G[SMM_NR], W[SMM_NR], iG[SMM_NR], v[SMM_MAXD], tr[SMM_MAXD];
    memcpy(x, x0, sizeof(double) * d);
    memcpy(mom, mom0, sizeof(double) * d);
    double lp = smm_evalallt(m, x, g, G);
    memcpy(W, G, sizeof(double) * nr);
    double ld = smm_chol(W, d);
    if (isnan(ld)) return NAN;
    smm_inverse(W, d, iG);
    smm_symv(iG, mom, d, v);
    const double H0 = rm_hamiltonian(lp, ld, rm_dot(mom, v, d), d);
    rm_terms(m, x, iG, NULL, tr, NULL);
    for (int64_t l = 0; l < nl; ++l)
        if (rm_leap(m, n_newton, eps / 2.0, x, mom, g, iG, tr, &lp, &ld)) return NAN;
    smm_symv(iG, mom, d, v);
    return rm_hamiltonian(lp, ld, rm_dot(mom, v, d), d) - H0;
}
