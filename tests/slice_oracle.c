/* slice_oracle.c -- the slice-sampling checker (TEST INFRASTRUCTURE ONLY).
 *
 * Includes oracle/oracle.c unchanged and restates mcmc_run_slice (include/mcmc_hip.h; slice_sample.jl:43-103 on the
 * counter-based stream) per chain with three plain while loops, the way the reference writes them -- not the kernel's
 * one loop with a phase.  tests/test_slice_cpu.py holds it against a literal transcription of slice_sample.jl
 * (tests/slice_ref.py).
 *
 * Every logdist is orc_eval of the whole d-vector in the given order.  An update may spend max_evals evaluations: a
 * chain whose update is not finished after that many, or whose proposal equals state[dd] and still is not acceptable,
 * stops (info = the iteration counted from iter_begin, its state the last completed iteration's, NaN rows from then
 * on).
 *
 * census: [0] updates with no step out to the left, [1] with at least one; [2], [3] likewise to the right;
 * [4] shrinks from the left (x_l = xprime), [5] from the right; [6] updates whose first proposal was accepted;
 * [7] evaluations that returned -Inf; [8] the largest evaluation count of one update; [9] updates; [10] chains
 * stopped.  upd_evals (or NULL): [burnin + niter][d][C] int32, the evaluations of every update (0 after a stop). */
#include "../oracle/oracle.c"

#define ORC_TAG_SLICE 9u

/* draw k of the update (iter, dd) of `chain` */
double orc_slice_draw(uint64_t seed, uint32_t chain, uint32_t iter, uint32_t dd, uint32_t k) {
    uint32_t w[4];
    orc_block(seed, chain, iter, (dd << 20) | (k >> 1), ORC_TAG_SLICE, w);
    return (k & 1u) ? orc_uniform52(w[2], w[3]) : orc_uniform52(w[0], w[1]);
}

double orc_slice_log(double x) { return orc_log(x); }

typedef struct {
    const orc_model* m;
    double *x, *tmp;
    int order, dd;
    int64_t ne, max_evals;
    int64_t* census;
} slice_ctx;

/* logdist of the state with coordinate dd at v; 0 when the budget is spent (*out untouched) */
static int slice_eval(slice_ctx* c, double v, double* out) {
    if (c->ne >= c->max_evals) return 0;
    const double keep = c->x[c->dd];
    c->x[c->dd] = v;
    *out = orc_eval(c->m, c->x, NULL, c->tmp, c->order);
    c->x[c->dd] = keep;
    c->ne += 1;
    if (isinf(*out) && *out < 0) c->census[7] += 1;
    return 1;
}

/* returns 0, or MCMC_E_INIT_OUT_OF_SUPPORT (2) when a start's log-density is not finite.
 * init_x [d][C]; samples [niter][d][C]; final_x [d][C]; final_lp, info [C]; evals: every evaluation, the C initial
 * ones included */
int orc_slice(const orc_model* m, int order, int64_t C, int64_t chain0, uint64_t seed, const double* init_x,
              const double* widths, int64_t niter, int64_t burnin, int64_t iter_begin, int step_out,
              int64_t max_evals, double* samples, double* final_x, double* final_lp, int32_t* info, int64_t* evals,
              int64_t* census, int32_t* upd_evals) {
    const int d = m->d;
    double* buf = (double*)malloc(sizeof(double) * (2 * (size_t)d + orc_scratch(m)));
    double *state = buf, *work = state + d, *tmp = work + d;
    int64_t total = 0;
    int rc = 0;
    for (int64_t c = 0; c < C && rc == 0; ++c) {
        const uint32_t chain = (uint32_t)(chain0 + c);
        for (int j = 0; j < d; ++j) state[j] = init_x[(size_t)j * C + c];
        double log_Px = orc_eval(m, state, NULL, tmp, order);                         /* :52 */
        total += 1;
        if (!isfinite(log_Px)) { rc = 2; break; }
        double last_lp = log_Px;
        int32_t stopped = 0;
        for (int64_t it = 1; it <= burnin + niter; ++it) {
            const uint32_t iter = (uint32_t)(iter_begin + it);
            if (!stopped) {
                memcpy(work, state, sizeof(double) * (size_t)d);
                double lp = log_Px;
                int fail = 0;
                for (int dd = 0; dd < d && !fail; ++dd) {
                    slice_ctx e = {m, work, tmp, order, dd, 0, max_evals, census};
                    const double w = widths[dd], xc = work[dd];
                    const double log_uprime = orc_log(orc_slice_draw(seed, chain, iter, (uint32_t)dd, 0u)) + lp;  /* :63 */
                    const double r = orc_slice_draw(seed, chain, iter, (uint32_t)dd, 1u);       /* :68 */
                    const double rw = r * w, qw = (1.0 - r) * w;
                    double x_l = xc - rw;                                                        /* :69 */
                    double x_r = xc + qw;                                                        /* :70 */
                    double v = 0.0;
                    if (step_out) {
                        int64_t nl = 0, nr = 0;
                        while (1) {                                                              /* :72-74 */
                            if (!slice_eval(&e, x_l, &v)) { fail = 1; break; }
                            if (!(v > log_uprime)) break;
                            x_l = x_l - w;
                            nl += 1;
                        }
                        while (!fail) {                                                          /* :75-77 */
                            if (!slice_eval(&e, x_r, &v)) { fail = 1; break; }
                            if (!(v > log_uprime)) break;
                            x_r = x_r + w;
                            nr += 1;
                        }
                        if (!fail) {
                            census[nl ? 1 : 0] += 1;
                            census[nr ? 3 : 2] += 1;
                        }
                    }
                    uint32_t k = 2u;
                    while (!fail) {                                                              /* :81-95 */
                        const double u = orc_slice_draw(seed, chain, iter, (uint32_t)dd, k);
                        const double span = x_r - x_l, prod = u * span;
                        const double xprime = prod + x_l;                                        /* :82 */
                        if (!slice_eval(&e, xprime, &v)) { fail = 1; break; }
                        lp = v;                                                                  /* :83 */
                        if (lp > log_uprime) {
                            if (k == 2u) census[6] += 1;
                            work[dd] = xprime;                                                   /* :96 */
                            break;
                        }
                        if (xprime > xc) { x_r = xprime; census[5] += 1; }
                        else if (xprime < xc) { x_l = xprime; census[4] += 1; }
                        else fail = 1;                                                           /* :92 */
                        k += 1u;
                    }
                    total += e.ne;
                    if (e.ne > census[8]) census[8] = e.ne;
                    census[9] += 1;
                    if (upd_evals) upd_evals[((size_t)(it - 1) * (size_t)d + (size_t)dd) * (size_t)C + (size_t)c] = (int32_t)e.ne;
                }
                if (fail) {
                    stopped = it > 0x7fffffffLL ? 0x7fffffff : (int32_t)it;
                    census[10] += 1;
                } else {
                    memcpy(state, work, sizeof(double) * (size_t)d);
                    log_Px = lp;
                    last_lp = lp;
                }
            }
            if (it > burnin && samples) {
                const size_t row = (size_t)(it - burnin - 1);
                for (int j = 0; j < d; ++j)
                    samples[(row * (size_t)d + (size_t)j) * (size_t)C + (size_t)c] = stopped ? NAN : state[j];
            }
        }
        for (int j = 0; j < d; ++j) final_x[(size_t)j * C + c] = state[j];
        final_lp[c] = last_lp;
        info[c] = stopped;
    }
    *evals = total;
    free(buf);
    return rc;
}
