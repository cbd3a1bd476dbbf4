/*
 * lmc_oracle.c -- CPU restatement of the two Lagrangian Monte Carlo samplers, ERMLMC (reference
 * src/samplers/ERMLMC.jl:84-179) and RMLMC (src/samplers/RMLMC.jl:89-179), on the probit / logistic models -- TEST
 * INFRASTRUCTURE ONLY.  A part of tests/manifold_oracle.c, after rmhmc_oracle.c.
 *
 * The log-target, gradient, tensor, Cholesky factor, inverse, solve, matvec, the weight's derivative, the two fused
 * terms, the state and the step loop (hmc_chain) are the earlier parts'.  Added here, in the order
 * mcmc.jl_amd/csrc/kernels/lmc.hip documents: the weighted Gram matrix
 * K(v) = X' diag(w o X v) X (vxC(v) = 0.5 K(v) on these models), the factor of G + c vxC and both samplers' proposal.
 *
 * Departures from the reference, as lmc.hip's header lists them: a trajectory that meets a log-target that is not
 * finite, a pivot <= 0 or not finite at any G, invG or G +- c vxC, or a position, velocity or ratio that is not finite
 * is rejected; a nRandomLeaps draw of 0 is rejected; set_state re-evaluates at the new position and the next step
 * recomputes all geometry from it.
 */
#define ORC_TAG_LMC 6u

/* K = X' diag(w o t) X, t = X v by eta's chain: K[a][b], b <= a, the fma chain over the observations in ascending
   order from zero of fma(X[i][a], RN(RN(w_i t_i) X[i][b]), .) (the tensor's chain with another weight) */
static void lmc_gram(const orc_model* m, const double* x, const double* v, double* K) {
    const int d = m->d;
    for (int k = 0; k < d * (d + 1) / 2; ++k) K[k] = 0.0;
    for (int64_t i = 0; i < m->n; ++i) {
        const double* Xi = m->X + (size_t)i * d;
        const double w = pm_dw(m, pm_eta(Xi, x, d), m->Y[i]);
        const double wt = w * pm_eta(Xi, v, d);
        for (int a = 0; a < d; ++a)
            for (int b = 0; b <= a; ++b) K[smm_tri(a, b)] = fma(Xi[a], wt * Xi[b], K[smm_tri(a, b)]);
    }
}

/* W = fma(cq, K, G) entry by entry (G + 2 cq vxC), factored in place; returns sum log diag, NaN on a failed pivot */
static double lmc_factor(const double* G, const double* K, double cq, int d, double* W) {
    for (int k = 0; k < d * (d + 1) / 2; ++k) W[k] = fma(cq, K[k], G[k]);
    return smm_chol(W, d);
}

typedef struct {
    double lp, ld;
    double g[SMM_MAXD], G[SMM_NR], iG[SMM_NR], dphi[SMM_MAXD];
} lmc_geo;

/* the geometry at x: evalallt, cholG, invG, traceInvGxdG, dphi = (-grad) + 0.5 trace; returns 1 on a log-target that is
   not finite or a failed pivot */
static int lmc_geom(const orc_model* m, const double* x, lmc_geo* o) {
    const int d = m->d, nr = d * (d + 1) / 2;
    double W[SMM_NR], tr[SMM_MAXD];
    o->lp = smm_evalallt(m, x, o->g, o->G);
    memcpy(W, o->G, sizeof(double) * nr);
    o->ld = smm_chol(W, d);
    smm_inverse(W, d, o->iG);
    rm_terms(m, x, o->iG, NULL, tr, NULL);
    for (int r = 0; r < d; ++r) o->dphi[r] = (-o->g[r]) + 0.5 * tr[r];
    return !isfinite(o->lp) || isnan(o->ld);
}

/* ERMLMC.jl:116-126 (and 141-151): the explicit velocity update at the geometry o; returns 1 on failure */
static int lmc_half(const orc_model* m, const double* x, const lmc_geo* o, double h, double* v, double* delta) {
    const int d = m->d;
    const double hc = 0.5 * h;
    double Gv[SMM_MAXD], rhs[SMM_MAXD] = {0.0}, v1[SMM_MAXD], K[SMM_NR], W[SMM_NR];
    smm_symv(o->G, v, d, Gv);
    for (int r = 0; r < d; ++r) rhs[r] = Gv[r] - hc * o->dphi[r];
    lmc_gram(m, x, v, K);
    const double ldA = lmc_factor(o->G, K, hc * 0.5, d, W);
    rm_solve(W, rhs, d, v1);
    if (isnan(ldA) || !rm_all_finite(v1, d)) return 1;
    *delta = *delta - 2.0 * ldA;
    memcpy(v, v1, sizeof(double) * d);
    lmc_gram(m, x, v, K);
    const double ldB = lmc_factor(o->G, K, -(hc * 0.5), d, W);
    if (isnan(ldB)) return 1;
    *delta = *delta + 2.0 * ldB;
    return 0;
}

/* one ERMLMC leapfrog (ERMLMC.jl:114-152) from (x, v) with the geometry o of x; o becomes the new position's */
static int lmc_leap_e(const orc_model* m, double h, double* x, double* v, lmc_geo* o, double* delta) {
    const int d = m->d;
    double cand[SMM_MAXD];
    if (lmc_half(m, x, o, h, v, delta)) return 1;
    for (int r = 0; r < d; ++r) cand[r] = x[r] + h * v[r];
    if (!rm_all_finite(cand, d)) return 1;
    memcpy(x, cand, sizeof(double) * d);
    if (lmc_geom(m, x, o)) return 1;
    return lmc_half(m, x, o, h, v, delta);
}

/* v - (h/2) (invG (0.5 u2 + dphi)) */
static void lmc_semi_update(const lmc_geo* o, const double* v, const double* u2, double hc, int d, double* out) {
    double sv[SMM_MAXD] = {0.0}, is[SMM_MAXD];
    for (int r = 0; r < d; ++r) sv[r] = 0.5 * u2[r] + o->dphi[r];
    smm_symv(o->iG, sv, d, is);
    for (int r = 0; r < d; ++r) out[r] = v[r] - hc * is[r];
}

/* one RMLMC leapfrog (RMLMC.jl:119-152) */
static int lmc_leap_s(const orc_model* m, int n_newton, double h, double* x, double* v, lmc_geo* o, double* delta) {
    const int d = m->d;
    const double hc = 0.5 * h;
    double lv[SMM_MAXD], lvin[SMM_MAXD], cand[SMM_MAXD], u2[SMM_MAXD], K[SMM_NR], W[SMM_NR];
    memcpy(lv, v, sizeof(double) * d);
    memcpy(lvin, v, sizeof(double) * d);
    for (int k = 0; k < n_newton; ++k) {                                     /* RMLMC.jl:122-127 */
        memcpy(lvin, lv, sizeof(double) * d);
        rm_terms(m, x, o->iG, lv, NULL, u2);
        lmc_semi_update(o, v, u2, hc, d, cand);
        if (!rm_all_finite(cand, d)) return 1;
        memcpy(lv, cand, sizeof(double) * d);
    }
    memcpy(v, lv, sizeof(double) * d);                                       /* RMLMC.jl:128 */
    lmc_gram(m, x, lvin, K);                                                 /* vxC as the loop leaves it */
    const double ldA = lmc_factor(o->G, K, h * 0.5, d, W);                   /* RMLMC.jl:131 */
    if (isnan(ldA)) return 1;
    *delta = *delta - 2.0 * ldA;
    for (int r = 0; r < d; ++r) cand[r] = x[r] + h * v[r];                   /* RMLMC.jl:134 */
    if (!rm_all_finite(cand, d)) return 1;
    memcpy(x, cand, sizeof(double) * d);
    if (lmc_geom(m, x, o)) return 1;                                         /* RMLMC.jl:136-143 */
    lmc_gram(m, x, v, K);
    rm_terms(m, x, o->iG, v, NULL, u2);
    const double ldB = lmc_factor(o->G, K, -(h * 0.5), d, W);                /* RMLMC.jl:149 */
    if (isnan(ldB)) return 1;
    *delta = *delta + 2.0 * ldB;
    lmc_semi_update(o, v, u2, hc, d, cand);                                  /* RMLMC.jl:151 */
    if (!rm_all_finite(cand, d)) return 1;
    memcpy(v, cand, sizeof(double) * d);
    return 0;
}

static double lmc_energy(int semi, double lp, double ld, const double* G, const double* v, int d) {
    double Gv[SMM_MAXD];
    smm_symv(G, v, d, Gv);
    const double quad = rm_dot(v, Gv, d);
    return semi ? ((-lp) + ld) + 0.5 * quad : ((-lp) - ld) + 0.5 * quad;   /* RMLMC.jl:110, ERMLMC.jl:105 */
}

static double lmc_leaps_uniform(uint64_t seed, uint32_t chain, uint32_t step) {
    uint32_t w[4];
    orc_block(seed, chain, step, 0u, ORC_TAG_LMC, w);
    return orc_uniform52(w[0], w[1]);
}

/* either sampler's proposal (ERMLMC.jl:100-160, RMLMC.jl:105-160): the velocity from chol(invG), the energy, the
   leapfrogs with their deltaLogDet and E - E' + deltaLogDet */
static int lmc_propose(const mf_run* r, uint32_t chain, uint32_t i, double eps, int64_t nl_fixed, const double* x,
                       const double* g, double lp, double* xp, double* gp, double* lpp, int64_t* nrl, int* failed) {
    const orc_model* m = r->m;
    const int d = m->d, nr = d * (d + 1) / 2;
    const int semi = r->s->kind == ORC_RMLMC;
    const int n_newton = semi ? (int)r->s->t0 : 0;
    double v[SMM_MAXD], W[SMM_NR], z[SMM_MAXD + 4];
    lmc_geo o;
    (void)g;
    *failed = lmc_geom(m, x, &o);                        /* its log-target and gradient are the state's, bit for bit */
    memcpy(W, o.iG, sizeof(double) * nr);
    if (isnan(smm_chol(W, d))) *failed = 1;                                   /* chol(invG), ERMLMC.jl:103 */
    orc_normals(r->seed, chain, i, d, z);
    rm_lmul(W, z, d, v);
    const double E = lmc_energy(semi, lp, o.ld, o.G, v, d);
    *nrl = hmc_leap_count(r->cn, lmc_leaps_uniform(r->seed, chain, i), nl_fixed, 0.0);
    memcpy(xp, x, sizeof(double) * d);
    double delta = 0.0;
    for (int64_t l = 0; l < *nrl && !*failed; ++l)
        *failed = semi ? lmc_leap_s(m, n_newton, eps, xp, v, &o, &delta) : lmc_leap_e(m, eps, xp, v, &o, &delta);
    if (*failed || *nrl <= 0) return 0;
    const double Ep = lmc_energy(semi, o.lp, o.ld, o.G, v, d);
    const double ratio = (E - Ep) + delta;
    memcpy(gp, o.g, sizeof(double) * d);
    *lpp = o.lp;
    if (isfinite(ratio)) return orc_mh_short_circuit(r->seed, chain, i, ratio);
    *failed = 1;
    return 0;
}

static void lmc_chain(const mf_run* r, uint32_t chain, int64_t c) { hmc_chain(r, chain, c, lmc_propose); }

/* the weighted Gram matrix of one point: x [d], v [d] -> packed K [nr] (vxC(v) = 0.5 K) and u2 = X' (w o (X v)^2)
   (vxC(v) v = 0.5 u2) */
void orc_lmc_gram(const orc_model* m, const double* x, const double* v, double* K, double* u2) {
    double iG[SMM_NR] = {0.0};
    lmc_gram(m, x, v, K);
    rm_terms(m, x, iG, v, NULL, u2);
}

/* G + 2 cq vxC from packed G and K by the kernels' route: sum log diag of the factor (logdet / 2) and, with b, the
   solve; returns 0 on a failed pivot */
int orc_lmc_factor(int d, const double* G, const double* K, double cq, const double* b, double* half_logdet,
                   double* out) {
    double W[SMM_NR];
    *half_logdet = lmc_factor(G, K, cq, d, W);
    if (isnan(*half_logdet)) return 0;
    if (b) rm_solve(W, b, d, out);
    return 1;
}

/* one leapfrog of either sampler from (x, v) [d] each, in place, the geometry computed at x: returns deltaLogDet's
   change, NaN when the trajectory fails */
double orc_lmc_leap(const orc_model* m, int semi, int n_newton, double h, double* x, double* v) {
    lmc_geo o;
    double delta = 0.0;
    if (lmc_geom(m, x, &o)) return NAN;
    if (semi ? lmc_leap_s(m, n_newton, h, x, v, &o, &delta) : lmc_leap_e(m, h, x, v, &o, &delta)) return NAN;
    return delta;
}
