/* stemp_oracle.c -- the SerialTempMC checker (TEST INFRASTRUCTURE ONLY).
 *
 * Includes oracle/oracle.c unchanged and restates the serial-tempering runner (SerialTempMC.jl:31-85) per walker with
 * the oracle's own one-step function, as orc_seqmc does for SeqMC.  Walker c is chain c of every target's batch.  It
 * carries the fields the runner reads of its last MCMCSample s: cur = s.ppars (stored, SerialTempMC.jl:77),
 * prev = s.pars (what a swap resets the other task to, SerialTempMC.jl:62) and lt = s.logtarget (SerialTempMC.jl:64).
 *
 * The library steps every target on every runner step (each reset to the walker's position first) and the walker
 * takes the sample of its target; so does this loop, so that every target's final state, step counter and
 * evaluation count can be compared too.  tests/test_stemp_cpu.py holds it against a literal transcription of
 * run_serialtempmc that consumes only the task the walker is on.
 *
 * counters: [0] swaps proposed, [1] accepted, [2] rejected, [3] swap ratios that were NaN, [4 + t] runner steps after
 * which the walker was on target t. */
#include "../oracle/oracle.c"

#define ORC_TAG_STEMP 8u

/* the two uniforms of walker `chain` at runner step i */
void orc_stemp_draws(uint64_t seed, uint32_t chain, uint32_t i, double* u) {
    uint32_t w[4];
    orc_block(seed, chain, i, 0u, ORC_TAG_STEMP, w);
    u[0] = orc_uniform52(w[0], w[1]);
    u[1] = orc_uniform52(w[2], w[3]);
}

double orc_stemp_exp(double x) { return orc_exp(x); }

/* zero-based SerialTempMC.jl:59-60 */
int32_t orc_stemp_pick(double u, int32_t K, int32_t at) {
    int32_t r = (int32_t)floor(u * (double)(K - 1));
    if (r > K - 2) r = K - 2;
    return r >= at ? r + 1 : r;
}

static void stemp_step(const orc_model* m, const orc_sampler* s, uint64_t seed, int64_t chain0, int64_t C, int64_t c,
                       int64_t step0, orc_state* st, int order) {
    orc_run(m, s, seed, chain0, C, c, c + 1, step0, 0, 1, 1, st, NULL, NULL, NULL, order, 1);
}

/* samples [steps-burnin][d][C], mods [steps-burnin][C], swaps [steps-burnin][C] bytes, final_at [C] */
void orc_serialtempmc(const orc_model* const* models, const orc_sampler* const* samplers, const uint64_t* seeds,
                      int64_t chain0, orc_state* const* states, int64_t* steps_done, const int* orders, int K,
                      int64_t C, int64_t steps, int64_t burnin, int64_t swap_period, const double* logW,
                      uint64_t seed, double* samples, int32_t* mods, uint8_t* swaps, int32_t* final_at,
                      int64_t* counters) {
    const int d = models[0]->d;
    size_t sc = 0;
    for (int t = 0; t < K; ++t) {
        size_t s1 = orc_scratch(models[t]);
        if (s1 > sc) sc = s1;
    }
    double* buf = (double*)malloc(sizeof(double) * (4 * (size_t)d + sc));
    double *cur = buf, *prev = cur + d, *cand = prev + d, *xv = cand + d, *tmp = xv + d;
    int64_t* sd = (int64_t*)malloc(sizeof(int64_t) * (size_t)K);
    for (int64_t c = 0; c < C; ++c) {
        for (int t = 0; t < K; ++t) sd[t] = steps_done[t];
        int32_t at = 0;
        double lt = states[0]->lp[c], cand_lt = 0.0;
        for (int j = 0; j < d; ++j) prev[j] = states[0]->x[(size_t)j * C + c];
        stemp_step(models[0], samplers[0], seeds[0], chain0, C, c, sd[0], states[0], orders[0]);   /* :51 */
        sd[0] += 1;
        for (int j = 0; j < d; ++j) cur[j] = states[0]->x[(size_t)j * C + c];
        for (int64_t i = 1; i <= steps; ++i) {
            const int is_swap = i % swap_period == 0;
            double u[2];
            orc_stemp_draws(seed, (uint32_t)(chain0 + c), (uint32_t)i, u);
            const int32_t tgt = is_swap ? orc_stemp_pick(u[0], K, at) : at;
            const double* from = is_swap ? prev : cur;
            for (int t = 0; t < K; ++t) {
                orc_state* st = states[t];
                for (int j = 0; j < d; ++j) {                    /* MCMC.reset(tasks[t], from) */
                    st->x[(size_t)j * C + c] = from[j];
                    xv[j] = from[j];
                }
                st->lp[c] = orc_eval(models[t], xv, NULL, tmp, orc_eval_order(orders[t]));
                const double ll0 = st->lp[c];
                stemp_step(models[t], samplers[t], seeds[t], chain0, C, c, sd[t], st, orders[t]);
                sd[t] += 1;
                if (t == tgt) {
                    for (int j = 0; j < d; ++j) cand[j] = st->x[(size_t)j * C + c];
                    cand_lt = ll0;
                }
            }
            int acc = 0;
            if (is_swap) {
                const double r = ((lt - cand_lt) + logW[tgt]) - logW[at];
                acc = u[1] < orc_exp(r);
                counters[0] += 1;
                counters[acc ? 1 : 2] += 1;
                if (isnan(r)) counters[3] += 1;
                if (acc) {                                       /* at, s = at2, s2 (s2.pars is prev) */
                    at = tgt;
                    memcpy(cur, cand, sizeof(double) * (size_t)d);
                    lt = cand_lt;
                }
            } else {                                             /* s = consume(tasks[at].task) */
                memcpy(prev, cur, sizeof(double) * (size_t)d);
                memcpy(cur, cand, sizeof(double) * (size_t)d);
                lt = cand_lt;
            }
            counters[4 + at] += 1;
            if (i > burnin) {
                const size_t row = (size_t)(i - burnin - 1);
                for (int j = 0; j < d; ++j) samples[(row * (size_t)d + (size_t)j) * (size_t)C + (size_t)c] = cur[j];
                mods[row * (size_t)C + (size_t)c] = at;
                swaps[row * (size_t)C + (size_t)c] = (uint8_t)acc;
            }
        }
        final_at[c] = at;
    }
    for (int t = 0; t < K; ++t) steps_done[t] = sd[t];
    free(sd);
    free(buf);
}
