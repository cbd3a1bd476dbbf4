/*
 * nuts_oracle.c -- CPU restatement of the NUTS sampler (reference src/samplers/NUTS.jl) -- TEST INFRASTRUCTURE ONLY.
 *
 * Includes oracle/oracle.c unchanged (orc_eval, orc_normals, orc_block, the deterministic math) and adds
 * orc_nuts_init / orc_nuts_run.  buildTree is written recursively, line for line after NUTS.jl:85-118; the library's
 * kernel walks the same tree iteratively (mcmc.jl_amd/csrc/nuts.hpp), and bitwise agreement between the two is the
 * evidence for that transformation.  The draws the reference takes from a sequential generator are the
 * counter-based blocks DESIGN.md documents: (chain, step i, block j, tag 3) for doubling j's direction and accept
 * uniform, (chain, step i, block (l << 5) | k, tag 4) for the merge of a level-k subtree after l leapfrogs.
 *
 * Per run it also returns coverage counters, so that the tests can show the parity cases exercise every way a step
 * ends: [0] steps ended by the outer U-turn test, [1] by a U-turn inside the last subtree, [2] by s1 false at a leaf
 * (divergence or out of support), [3] by maxdoublings, [4] merges with n1 + n2 == 0, [5] / [6] doublings drawn
 * forwards / backwards.
 */
#include "../oracle/oracle.c"

#define ORC_TAG_NUTS_DOUBLING 3u
#define ORC_TAG_NUTS_MERGE 4u
#define ORC_NUTS_MAXD 32
#define ORC_NUTS_NCOUNT 7

typedef struct {
    double pars[ORC_NUTS_MAXD], grad[ORC_NUTS_MAXD], m[ORC_NUTS_MAXD];
    double logTarget, H;
} nuts_sample;                                   /* HMCSample (HMC.jl:81-87) */

typedef struct {
    const orc_model* model;
    int order;
    uint64_t seed;
    uint32_t chain, step;
    double epsilon, u_slice, H0;
    uint32_t nleap;                              /* leapfrogs of this step so far */
    int64_t n_evals;
    int leaf_fail, inner_uturn;                  /* of the current doubling */
    int64_t zero_merges;
    double tmp[ORC_NUTS_MAXD + 16];
} nuts_ctx;

/* dot(a, b) with fma accumulation in the layout's order: 0 left to right, ORC_ORDER_PAIR the two halves then added */
static double nuts_dot(const double* a, const double* b, int d, int order) {
    if (order == ORC_ORDER_PAIR) {
        const int S = orc_pair_split(d);
        double p = 0.0, q = 0.0;
        for (int j = 0; j < d && j < S; ++j) p = fma(a[j], b[j], p);
        for (int j = S; j < d; ++j) q = fma(a[j], b[j], q);
        return p + q;
    }
    double p = 0.0;
    for (int j = 0; j < d; ++j) p = fma(a[j], b[j], p);
    return p;
}

/* uturn(s1, s2) = dot(s2.pars-s1.pars, s1.m) < 0. || dot(s2.pars-s1.pars, s2.m) < 0.   (NUTS.jl:50) */
static int nuts_uturn(const nuts_ctx* c, const nuts_sample* s1, const nuts_sample* s2) {
    const int d = c->model->d;
    double dx[ORC_NUTS_MAXD];
    for (int j = 0; j < d; ++j) dx[j] = s2->pars[j] - s1->pars[j];
    return nuts_dot(dx, s1->m, d, c->order) < 0.0 || nuts_dot(dx, s2->m, d, c->order) < 0.0;
}

/* leapfrog(s, ve, ll) (HMC.jl:93-102) */
static nuts_sample nuts_leapfrog(nuts_ctx* c, const nuts_sample* s, double ve) {
    const int d = c->model->d;
    nuts_sample n = *s;
    for (int j = 0; j < d; ++j) n.m[j] = n.m[j] + (0.5 * n.grad[j]) * ve;
    for (int j = 0; j < d; ++j) n.pars[j] = n.pars[j] + ve * n.m[j];
    n.logTarget = orc_eval(c->model, n.pars, n.grad, c->tmp, c->order);
    for (int j = 0; j < d; ++j) n.m[j] = n.m[j] + (0.5 * n.grad[j]) * ve;
    n.H = -n.logTarget + 0.5 * orc_dot(n.m, c->model, c->order);
    c->n_evals += 1;
    return n;
}

typedef struct {
    nuts_sample state_minus, state_plus, state1;
    int n1, s1;
    double alpha1;
    int nalpha1;
} nuts_tree;

/* buildTree(state, dir, j, ll)  (NUTS.jl:85-118) */
static void nuts_build_tree(nuts_ctx* c, const nuts_sample* state, int dir, int j, nuts_tree* r) {
    const double deltamax = 100.0;
    if (j == 0) {
        r->state1 = nuts_leapfrog(c, state, (double)dir * c->epsilon);
        c->nleap += 1;
        r->n1 = (c->u_slice <= -r->state1.H) + 0;
        r->s1 = c->u_slice < (deltamax - r->state1.H);
        if (!r->s1) c->leaf_fail = 1;
        r->state_minus = r->state1;
        r->state_plus = r->state1;
        r->alpha1 = fmin(1.0, orc_exp(c->H0 - r->state1.H));
        r->nalpha1 = 1;
        return;
    }
    nuts_build_tree(c, state, dir, j - 1, r);
    if (r->s1) {
        nuts_tree* t2 = (nuts_tree*)malloc(sizeof(nuts_tree));
        if (dir == -1) {
            const nuts_sample from = r->state_minus;
            nuts_build_tree(c, &from, dir, j - 1, t2);
            r->state_minus = t2->state_minus;
        } else {
            const nuts_sample from = r->state_plus;
            nuts_build_tree(c, &from, dir, j - 1, t2);
            r->state_plus = t2->state_plus;
        }
        uint32_t w[4];
        orc_block(c->seed, c->chain, c->step, (c->nleap << 5) | (uint32_t)j, ORC_TAG_NUTS_MERGE, w);
        const double u = orc_uniform52(w[0], w[1]);
        if (u <= (double)t2->n1 / (double)(t2->n1 + r->n1)) r->state1 = t2->state1;
        if (t2->n1 + r->n1 == 0) c->zero_merges += 1;
        r->alpha1 += t2->alpha1;
        r->nalpha1 += t2->nalpha1;
        const int ut = nuts_uturn(c, &r->state_minus, &r->state_plus);
        if (t2->s1 && ut) c->inner_uturn = 1;
        r->s1 = t2->s1 && !ut;
        r->n1 += t2->n1;
        free(t2);
    }
}

/* state0.m = randn(model.size) .* scale; update!(state0) */
static void nuts_momentum(const nuts_ctx* c, nuts_sample* s0, uint32_t step) {
    const orc_model* m = c->model;
    double z[ORC_NUTS_MAXD + 4];
    orc_normals(c->seed, c->chain, step, m->d, z);
    for (int j = 0; j < m->d; ++j) s0->m[j] = z[j] * (m->scale ? m->scale[j] : 1.0);
    s0->H = -s0->logTarget + 0.5 * orc_dot(s0->m, m, c->order);
}

/* SamplerTask initialisation (NUTS.jl:65-82, 127-129) of every chain from st->x: the evaluation, then the initial
   epsilon search with the normals of step 0 (H0 formed from the start's log-target and that momentum); eps, hbar,
   lebar into st->t_step, t_h, t_bar, mu into mu[].  Returns the number of starts out of support. */
int64_t orc_nuts_init(const orc_model* m, uint64_t seed, int64_t chain0, int64_t C, orc_state* st, double* mu,
                      int order) {
    const int d = m->d;
    int64_t bad = 0;
    for (int64_t ch = 0; ch < C; ++ch) {
        nuts_ctx c;
        memset(&c, 0, sizeof c);
        c.model = m; c.order = order; c.seed = seed; c.chain = (uint32_t)(chain0 + ch);
        nuts_sample s0;
        memset(&s0, 0, sizeof s0);
        for (int j = 0; j < d; ++j) s0.pars[j] = st->x[(size_t)j * C + ch];
        s0.logTarget = orc_eval(m, s0.pars, s0.grad, c.tmp, orc_eval_order(order));
        st->lp[ch] = s0.logTarget;
        if (!isfinite(s0.logTarget)) bad++;
        nuts_momentum(&c, &s0, 0u);
        double epsilon = 1.0;
        nuts_sample s1 = nuts_leapfrog(&c, &s0, epsilon);
        double ratio = orc_exp(s0.H - s1.H);
        const int up = ratio > 0.5;                              /* a = 2*(ratio>0.5)-1 */
        /* ratio^a > 2^-a; ends by IEEE arithmetic within about 1 100 passes, the cap of 2 048 never binds */
        for (int it = 0; it < 2048 && (up ? ratio > 0.5 : 1.0 / ratio > 2.0); ++it) {
            epsilon = epsilon * (up ? 2.0 : 0.5);
            s1 = nuts_leapfrog(&c, &s0, epsilon);
            ratio = orc_exp(s0.H - s1.H);
        }
        st->t_step[ch] = epsilon;
        st->t_h[ch] = 0.0;
        st->t_bar[ch] = 0.0;
        mu[ch] = orc_log(10.0 * epsilon);
        if (st->n_evals) st->n_evals[ch] = c.n_evals;
    }
    return bad;
}

/* the :reset hook (NUTS.jl:61-63): position and evaluation only */
void orc_nuts_set_state(const orc_model* m, int64_t C, orc_state* st, const double* x, int order) {
    const int d = m->d;
    double xs[ORC_NUTS_MAXD], g[ORC_NUTS_MAXD], tmp[ORC_NUTS_MAXD + 16];
    for (int64_t ch = 0; ch < C; ++ch) {
        for (int j = 0; j < d; ++j) xs[j] = st->x[(size_t)j * C + ch] = x[(size_t)j * C + ch];
        st->lp[ch] = orc_eval(m, xs, g, tmp, orc_eval_order(order));
        if (st->n_evals) st->n_evals[ch] += 1;
    }
}

static void nuts_chain(const orc_model* m, int maxdoublings, uint64_t seed, uint32_t chain, int64_t ch, int64_t C,
                       int64_t step0, int64_t burnin, int64_t thinning, int64_t len, orc_state* st, double* mu_arr,
                       double* samples, double* grads, uint8_t* acc_out, double* eps_out, int32_t* nd_out, int order,
                       int64_t* counters) {
    const int d = m->d;
    /* adaptation parameters (NUTS.jl:121-125) */
    const double delta = 0.7, gam = 0.05, kappa = 0.75;
    const int64_t nadapt = 1000, t0 = 10;
    nuts_ctx c;
    memset(&c, 0, sizeof c);
    c.model = m; c.order = order; c.seed = seed; c.chain = chain;
    nuts_sample state0;
    memset(&state0, 0, sizeof state0);
    for (int j = 0; j < d; ++j) state0.pars[j] = st->x[(size_t)j * C + ch];
    state0.logTarget = st->lp[ch];
    (void)orc_eval(m, state0.pars, state0.grad, c.tmp, order);    /* the state's gradient (deterministic recompute) */
    double epsilon = st->t_step[ch], hbar = st->t_h[ch], lebar = st->t_bar[ch];
    const double mu = mu_arr[ch];
    nuts_tree* tr = (nuts_tree*)malloc(sizeof(nuts_tree));

    for (int64_t t = 0; t < len; ++t) {
        const int64_t i = step0 + t + 1;
        c.step = (uint32_t)i;
        c.epsilon = epsilon;
        c.nleap = 0;
        nuts_momentum(&c, &state0, (uint32_t)i);                  /* state0.m = randn .* scale; update!(state0) */
        c.H0 = state0.H;
        c.u_slice = orc_log(orc_accept_uniform(seed, chain, (uint32_t)i)) - state0.H;
        nuts_sample state = state0, state_minus = state0, state_plus = state0;
        int j = 0, n = 1, s = 1, s1 = 1, accepted = 0;
        double alpha = 0.0;
        int nalpha = 1;
        while (s && j < maxdoublings) {
            uint32_t w[4];
            orc_block(seed, chain, (uint32_t)i, (uint32_t)j, ORC_TAG_NUTS_DOUBLING, w);
            const int dir = (w[0] & 1u) ? 1 : -1;                 /* dir = randbool() ? 1 : -1 */
            const double u = orc_uniform52(w[2], w[3]);
            counters[dir == 1 ? 5 : 6] += 1;
            c.leaf_fail = 0;
            c.inner_uturn = 0;
            if (dir == -1) {
                const nuts_sample from = state_minus;
                nuts_build_tree(&c, &from, dir, j, tr);
                state_minus = tr->state_minus;
            } else {
                const nuts_sample from = state_plus;
                nuts_build_tree(&c, &from, dir, j, tr);
                state_plus = tr->state_plus;
            }
            s1 = tr->s1;
            if (s1 && u < (double)tr->n1 / (double)n) {          /* accept */
                state = tr->state1;
                accepted = 1;
            }
            n += tr->n1;
            j += 1;
            alpha = tr->alpha1;
            nalpha = tr->nalpha1;
            s = s1 && !nuts_uturn(&c, &state_minus, &state_plus);
        }
        if (s) counters[3] += 1;
        else if (s1) counters[0] += 1;
        else if (c.leaf_fail) counters[2] += 1;
        else counters[1] += 1;
        /* epsilon adjustment (NUTS.jl:166-173) */
        if (i <= nadapt) {
            const double di = (double)i, dit = (double)(i + t0);
            hbar = hbar * (1.0 - 1.0 / dit) + (delta - alpha / (double)nalpha) / dit;
            const double le = mu - sqrt(di) / gam * hbar;
            const double ik = orc_exp(orc_log(di) * (-kappa));   /* i^(-kappa) */
            lebar = ik * le + (1.0 - ik) * lebar;
            epsilon = orc_exp(le);
        } else {
            epsilon = orc_exp(lebar);
        }
        int64_t kk;
        if (orc_kept(i - step0, burnin, thinning, len, &kk)) {
            if (samples)
                for (int q = 0; q < d; ++q) samples[((size_t)kk * d + q) * C + ch] = state.pars[q];
            if (grads)
                for (int q = 0; q < d; ++q) grads[((size_t)kk * d + q) * C + ch] = state.grad[q];
            if (acc_out) acc_out[(size_t)kk * C + ch] = (uint8_t)accepted;
            if (eps_out) eps_out[(size_t)kk * C + ch] = epsilon;
            if (nd_out) nd_out[(size_t)kk * C + ch] = (int32_t)j;
        }
        state0 = state;                                           /* state0 = deepcopy(state) */
    }
    counters[4] += c.zero_merges;
    free(tr);
    for (int j = 0; j < d; ++j) st->x[(size_t)j * C + ch] = state0.pars[j];
    st->lp[ch] = state0.logTarget;
    st->t_step[ch] = epsilon;
    st->t_h[ch] = hbar;
    st->t_bar[ch] = lebar;
    if (st->n_evals) st->n_evals[ch] += c.n_evals;
}

/* run_serialmc of chains [c_begin, c_end) of a batch of C with NUTS(maxdoublings); outputs as orc_run's, plus
   eps_out / nd_out [nkept][C] (diagnostics "epsilon" / "ndoublings") and counters[ORC_NUTS_NCOUNT] (added to) */
void orc_nuts_run(const orc_model* m, int maxdoublings, uint64_t seed, int64_t chain0, int64_t C, int64_t c_begin,
                  int64_t c_end, int64_t step0, int64_t burnin, int64_t thinning, int64_t len, orc_state* st,
                  double* mu, double* samples, double* grads, uint8_t* acc_out, double* eps_out, int32_t* nd_out,
                  int order, int nthreads, int64_t* counters) {
#ifdef _OPENMP
#pragma omp parallel num_threads(nthreads > 0 ? nthreads : 1)
#endif
    {
        int64_t cnt[ORC_NUTS_NCOUNT] = {0};
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 1)
#endif
        for (int64_t ch = c_begin; ch < c_end; ++ch)
            nuts_chain(m, maxdoublings, seed, (uint32_t)(chain0 + ch), ch, C, step0, burnin, thinning, len, st, mu,
                       samples, grads, acc_out, eps_out, nd_out, order, cnt);
#ifdef _OPENMP
#pragma omp critical
#endif
        for (int q = 0; q < ORC_NUTS_NCOUNT; ++q) counters[q] += cnt[q];
    }
    (void)nthreads;
}

/* exp of the checker's deterministic math (tuner_state's step_bar = exp(log epsilon_bar)) */
double orc_nuts_exp(double x) { return orc_exp(x); }
