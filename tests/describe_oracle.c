/* describe_oracle.c -- TEST INFRASTRUCTURE ONLY: a scalar restatement of mcmc_stats_describe (kernels/describe.hip,
 * DESIGN.md §4 "describe" and §5.5).  Built by tests/describe_ref.py on top of the oracle, which it includes unchanged.
 *
 * Per-chain table (summary.jl:35-42) of every (parameter j, chain c) series of samples [n][d][C]: orc_ess_one's
 * arithmetic (sum left to right, ss an fma chain of centred values, the IMSE variance), mcerror = sqrt(varimse),
 * ess = (n variid) / varimse, actime = varimse / variid, min / max by fmin / fmax (a NaN sample is passed over) with
 * -0 returned as +0.
 *
 * Pooled rows: every sum over chains runs in ONE order that depends on C alone.  Chains are cut into blocks of 4096;
 * in block b lane l (0..255) adds its chains b 4096 + 256 k + l, k = 0..15, left to right from +0; each 64-lane wave
 * folds its lanes by an xor butterfly 32, 16, 8, 4, 2, 1; the block's four wave sums are added left to right; the
 * block sums are added left to right from +0.  A chain past C, or one left out of a sum, is a +0 term.
 *
 * Quantiles (Julia's quantile, type 7) of the N = n C values of a parameter, sorted as order-preserving 64-bit keys
 * (-0 taken as +0, NaN above +Inf): h = (double)(N - 1) p, lo = floor(h), f = h - lo,
 * v[lo] + f (v[min(lo + 1, N - 1)] - v[lo]), plain multiply and add. */
#include "../oracle/oracle.c"

#include <stdlib.h>

#define DSC_NPOOLED 6 /* min, mean, max, mcerror, ess, rhat */
#define DSC_BLOCK 4096
#define DSC_LANES 256

static double dsc_reduce(const double* v, int64_t C) {
    double total = 0.0;
    for (int64_t b0 = 0; b0 < C; b0 += DSC_BLOCK) {
        double lane[DSC_LANES];
        for (int l = 0; l < DSC_LANES; ++l) {
            double acc = 0.0;
            for (int k = 0; k < DSC_BLOCK / DSC_LANES; ++k) {
                const int64_t c = b0 + (int64_t)k * DSC_LANES + l;
                acc = acc + (c < C ? v[c] : 0.0);
            }
            lane[l] = acc;
        }
        for (int w = 0; w < DSC_LANES; w += 64)
            for (int m = 32; m >= 1; m >>= 1) {
                double nx[64];
                for (int l = 0; l < 64; ++l) nx[l] = lane[w + l] + lane[w + (l ^ m)];
                for (int l = 0; l < 64; ++l) lane[w + l] = nx[l];
            }
        const double blk = ((lane[0] + lane[64]) + lane[128]) + lane[192];
        total = total + blk;
    }
    return total;
}

static uint64_t dsc_key(double x) {
    uint64_t u;
    if (x != x) return ~(uint64_t)0;
    memcpy(&u, &x, 8);
    if (u == 0x8000000000000000ull) u = 0;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

static double dsc_unkey(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    memcpy(&x, &u, 8);
    return x;
}

static int dsc_cmp(const void* a, const void* b) {
    const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
    return x < y ? -1 : x > y;
}

/* per_chain [6][d][C] or NULL; pooled [DSC_NPOOLED + nprobs][d] or NULL; nbad [d] or NULL.  Returns nonzero for a
 * bad argument. */
int orc_describe(const double* samples, int64_t n, int64_t d, int64_t C, int64_t maxlag, double* per_chain,
                 const double* probs, int32_t nprobs, double* pooled, int64_t* nbad) {
    if (n < 2 || d <= 0 || C <= 0 || nprobs < 0 || nprobs > 8 || (!per_chain && !pooled)) return 1;
    for (int i = 0; i < nprobs; ++i)
        if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) return 1;
    if (maxlag <= 0) maxlag = n - 1;
    const size_t stride = (size_t)d * C, dC = stride;
    const double nd = (double)n;
    double* w = (double*)malloc(9 * (size_t)C * sizeof(double));
    uint64_t* keys = (pooled && nprobs > 0) ? (uint64_t*)malloc((size_t)n * C * sizeof(uint64_t)) : NULL;
    double *mn = w, *mean = w + C, *mx = w + 2 * C, *s2 = w + 3 * C, *vi = w + 4 * C, *es = w + 5 * C, *e2 = w + 6 * C,
           *gv = w + 7 * C, *ge = w + 8 * C;
    for (int64_t j = 0; j < d; ++j) {
        int64_t bad = 0;
        for (int64_t c = 0; c < C; ++c) {
            const double* x = samples + (size_t)j * C + c;
            double sum = 0.0, lo = x[0], hi = x[0];
            for (int64_t t = 0; t < n; ++t) {
                const double v = x[(size_t)t * stride];
                sum = sum + v;
                lo = fmin(lo, v);
                hi = fmax(hi, v);
            }
            const double m = sum / nd;
            double ss = 0.0;
            for (int64_t t = 0; t < n; ++t) {
                const double z = x[(size_t)t * stride] - m;
                ss = fma(z, z, ss);
            }
            double varimse;
            const double ess = orc_ess_one(x, stride, n, 1, maxlag, 0, &varimse);
            const double variid = (ss / (nd - 1.0)) / nd;
            mn[c] = lo + 0.0;
            mx[c] = hi + 0.0;
            mean[c] = m;
            s2[c] = ss / (nd - 1.0);
            vi[c] = varimse;
            es[c] = ess;
            const int good = isfinite(varimse) && isfinite(ess) && varimse > 0.0;
            bad += !good;
            gv[c] = good ? varimse : 0.0;
            ge[c] = good ? ess : 0.0;
            if (per_chain) {
                const size_t o = (size_t)j * C + c;
                per_chain[0 * dC + o] = mn[c];
                per_chain[1 * dC + o] = m;
                per_chain[2 * dC + o] = mx[c];
                per_chain[3 * dC + o] = sqrt(varimse);
                per_chain[4 * dC + o] = ess;
                per_chain[5 * dC + o] = varimse / variid;
            }
        }
        if (nbad) nbad[j] = bad;
        if (!pooled) continue;
        double pmin = mn[0], pmax = mx[0];
        for (int64_t c = 0; c < C; ++c) {
            pmin = fmin(pmin, mn[c]);
            pmax = fmax(pmax, mx[c]);
        }
        const double Cd = (double)C, gm = dsc_reduce(mean, C) / Cd;
        for (int64_t c = 0; c < C; ++c) {
            const double e = mean[c] - gm;
            e2[c] = e * e;
        }
        const double W = dsc_reduce(s2, C) / Cd;
        const double Bn = dsc_reduce(e2, C) / (Cd - 1.0);
        const double good = (double)(C - bad);
        pooled[0 * d + j] = pmin;
        pooled[1 * d + j] = gm;
        pooled[2 * d + j] = pmax;
        pooled[3 * d + j] = sqrt(dsc_reduce(gv, C)) / good;
        pooled[4 * d + j] = dsc_reduce(ge, C);
        pooled[5 * d + j] = (C == 1 || W == 0.0) ? NAN : sqrt((((nd - 1.0) / nd) * W + Bn) / W);
        if (nprobs > 0) {
            const int64_t N = n * C;
            for (int64_t t = 0; t < n; ++t)
                for (int64_t c = 0; c < C; ++c) keys[t * C + c] = dsc_key(samples[(size_t)t * stride + (size_t)j * C + c]);
            qsort(keys, (size_t)N, sizeof(uint64_t), dsc_cmp);
            for (int i = 0; i < nprobs; ++i) {
                const double h = (double)(N - 1) * probs[i];
                const double fl = floor(h);
                const double f = h - fl;
                const int64_t lo = (int64_t)fl, hi = lo + 1 < N - 1 ? lo + 1 : N - 1;
                const double vlo = dsc_unkey(keys[lo]), vhi = dsc_unkey(keys[hi]);
                const double diff = vhi - vlo;
                const double prod = f * diff;
                pooled[(DSC_NPOOLED + i) * d + j] = vlo + prod;
            }
        }
    }
    free(w);
    free(keys);
    return 0;
}

/* the six fields of one series as orc_ess_one alone gives them (the exactness check of the per-chain table) */
void orc_describe_ess_fields(const double* samples, int64_t n, int64_t d, int64_t C, int64_t maxlag, double* ess,
                             double* var) {
    orc_ess(samples, n, d, C, 1, maxlag, 0, ess, var);
}
