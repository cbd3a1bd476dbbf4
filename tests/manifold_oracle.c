/*
 * manifold_oracle.c -- the CPU checker of the metric-tensor samplers (SMMALA, PMALA, RMHMC, ERMLMC / RMLMC) on the
 * probit / logistic models -- TEST INFRASTRUCTURE ONLY.
 *
 * One translation unit, built into tests/_build/libmanifold_oracle.so: oracle/oracle.c unchanged (the log-target, the
 * gradient, the normals and the accept uniform), the run frame every sampler of the family shares, then the family's
 * parts in the order below.  No part includes another; only this file knows the order.
 *
 *   smmala_oracle.c   the metric tensor, the packed SPD algebra
 *   pmala_oracle.c    the tensor's derivatives, the fused drift correction, and the SMMALA / PMALA driver
 *   rmhmc_oracle.c    the two fused tensor terms, the Cholesky solve, the HMC-type frame, and RMHMC's proposal
 *   lmc_oracle.c      the weighted Gram matrix, the factor of G + c vxC, and the two Lagrangian proposals
 */
#include "../oracle/oracle.c"

#define ORC_SMMALA 7
#define ORC_PMALA 8
#define ORC_RMHMC 9
#define ORC_ERMLMC 10
#define ORC_RMLMC 11

/* what a run's steps covered, summed over the chains run (the trajectory samplers only) */
typedef struct {
    int64_t n_plus, n_minus;     /* steps with timeStep = +1 / -1 (RMHMC) */
    int64_t nrl_min, nrl_max;    /* smallest and largest nRandomLeaps drawn */
    int64_t n_failed;            /* steps rejected for a failed trajectory */
    int64_t n_zero;              /* steps whose nRandomLeaps draw was 0 */
    int64_t n_adapt;             /* tuner adaptations */
} mf_counters;

/* one run_serialmc of a batch of C chains: what every chain of it reads; st is the sampler's state struct */
typedef struct {
    const orc_model* m;
    const orc_sampler* s;
    uint64_t seed;
    int64_t C, step0, burnin, thinning, len;
    int64_t tuner_burnin;        /* the burnin the tuner sees (the sampler's global step counter against it) */
    void* st;
    double* samples;             /* [nkept][d][C], as orc_run's; any of the three may be NULL */
    double* grads;
    uint8_t* acc_out;            /* [nkept][C] */
    mf_counters* cn;             /* may be NULL */
} mf_run;

/* chain c's position, gradient and accept bit after global step i, where the runner keeps that step */
static void mf_store_kept(const mf_run* r, int64_t i, int64_t c, const double* x, const double* g, int acc) {
    const int d = r->m->d;
    const int64_t C = r->C;
    int64_t kk;
    if (!orc_kept(i - r->step0, r->burnin, r->thinning, r->len, &kk)) return;
    if (r->samples)
        for (int q = 0; q < d; ++q) r->samples[((size_t)kk * d + q) * C + c] = x[q];
    if (r->grads)
        for (int q = 0; q < d; ++q) r->grads[((size_t)kk * d + q) * C + c] = g[q];
    if (r->acc_out) r->acc_out[(size_t)kk * C + c] = (uint8_t)acc;
}

/* chains [c_begin, c_end) of the batch, each by `chain` with its global id */
typedef void (*mf_chain_fn)(const mf_run* r, uint32_t chain, int64_t c);

static void mf_fan_out(const mf_run* r, mf_chain_fn chain, int64_t chain0, int64_t c_begin, int64_t c_end,
                       int nthreads) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads > 0 ? nthreads : 1)
#endif
    for (int64_t c = c_begin; c < c_end; ++c) chain(r, (uint32_t)(chain0 + c), c);
    (void)nthreads;
}

#include "smmala_oracle.c"
#include "pmala_oracle.c"
#include "rmhmc_oracle.c"
#include "lmc_oracle.c"

/* run_serialmc of chains [c_begin, c_end) of a batch of C by the sampler s names; outputs as orc_run's.  st is a
   pm_state for SMMALA / PMALA and an rm_state for the others; cn (may be NULL) is added to */
void orc_manifold_run(const orc_model* m, const orc_sampler* s, uint64_t seed, int64_t chain0, int64_t C,
                      int64_t c_begin, int64_t c_end, int64_t step0, int64_t burnin, int64_t thinning, int64_t len,
                      int64_t tuner_burnin, void* st, double* samples, double* grads, uint8_t* acc_out,
                      mf_counters* cn, int nthreads) {
    const mf_run r = {m, s, seed, C, step0, burnin, thinning, len, tuner_burnin, st, samples, grads, acc_out, cn};
    const mf_chain_fn chain = s->kind == ORC_SMMALA ? smm_chain : s->kind == ORC_PMALA ? pm_chain
                            : s->kind == ORC_RMHMC ? rm_chain : lmc_chain;
    mf_fan_out(&r, chain, chain0, c_begin, c_end, nthreads);
}

/* the build's draws of (chain, step) for the literal transcriptions: normals z [d] and the accept uniform (every
   sampler's); RMHMC's leaps' uniform and sign's normal in rm[0..1]; the Lagrangian samplers' leaps' uniform */
void orc_manifold_draws(uint64_t seed, uint32_t chain, uint32_t step, int d, double* z, double* u_acc, double* rm,
                        double* u_leaps_lmc) {
    double zz[SMM_MAXD + 4];
    orc_normals(seed, chain, step, d, zz);
    for (int j = 0; j < d; ++j) z[j] = zz[j];
    *u_acc = orc_accept_uniform(seed, chain, step);
    rm_draws(seed, chain, step, &rm[0], &rm[1]);
    *u_leaps_lmc = lmc_leaps_uniform(seed, chain, step);
}
