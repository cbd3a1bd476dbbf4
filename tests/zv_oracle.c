/* zv_oracle.c -- TEST INFRASTRUCTURE ONLY.  Scalar restatement of the arithmetic kernels/zv.hip documents
 * (DESIGN.md §5.5): the zero-variance estimators of src/stats/zv.jl:8-68, one chain at a time.
 *
 *   z = -g/2; the k control variates w of a kept step (order 1: z; order 2: z_j, (2 z_j) x_j - 1, and
 *   x_i z_j + x_j z_i for i < j), no fused multiply-adds in them;
 *   means: sums of the columns of [w | x] left to right over t, divided by n; a column whose n values all equal its
 *   first has that value as its mean, so it centres to exact zeros;
 *   Gram: G[i][m] and S[i][j] are fma chains over t = 0 .. 4 ceil(n/4) - 1 of the centred values, starting from
 *   +0, the steps t >= n contributing fma(0, 0, s);
 *   Cholesky: L[i][m] = (G[i][m] - sum_{q<m} L[i][q] L[m][q]) / L[m][m], the sum as s = fma(-L[i][q], L[m][q], s)
 *   from s = G[i][m], q ascending; the pivot s of column m must be > 0 and finite, else info = m + 1;
 *   moves: the number of kept steps t >= 1 whose row of [w | x] differs (!=) from step t - 1 in any column; with
 *   moves < k the centred rows have rank <= moves < k, so info = moves + 1 (the pivot that is zero in exact
 *   arithmetic at the latest) without factorising: a chain that never moved gets info = 1;
 *   forward: y[m][j] likewise from S[m][j] with fma(-y[q][j], L[m][q], s), divided by L[m][m];
 *   backward, m = k-1 .. 0: b[m][j] = (y[m][j] - sum_{q>m} L[q][m] b[q][j]) / L[m][m], s = fma(-L[q][m], b[q][j], s),
 *   q descending from k - 1; a = -b;
 *   apply: zv[t][j] = x[t][j] + s, s the fma chain fma(w[t][i], a[i][j], s) from +0 over i = 0 .. 4 ceil(k/4) - 1,
 *   i >= k contributing fma(0, 0, s).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int64_t zv_k(int order, int64_t d) { return order == 2 ? d * (d + 3) / 2 : d; }

/* the control variates of one kept step: x, z [d] -> w [k] */
static void zv_w(int order, int64_t d, const double* x, const double* z, double* w) {
    for (int64_t j = 0; j < d; ++j) w[j] = z[j];
    if (order != 2) return;
    for (int64_t j = 0; j < d; ++j) {
        const double t = (2.0 * z[j]) * x[j];
        w[d + j] = t - 1.0;
    }
    int64_t l = 2 * d;
    for (int64_t i = 0; i + 1 < d; ++i)
        for (int64_t j = i + 1; j < d; ++j) {
            const double p = x[i] * z[j], q = x[j] * z[i];
            w[l++] = p + q;
        }
}

static double zv_nan(void) {
    const uint64_t bits = 0x7ff8000000000000ull;
    double v;
    memcpy(&v, &bits, 8);
    return v;
}

/* samples, grads, zv [n][d][C]; coef [k][d][C] or NULL; info [C] or NULL.  Returns 0, or -1 on a bad argument. */
int orc_zv(int order, const double* samples, const double* grads, int64_t n, int64_t d, int64_t C, double* zv,
           double* coef, int32_t* info) {
    if ((order != 1 && order != 2) || d < 1 || C < 1) return -1;
    const int64_t k = zv_k(order, d), K = k + d;
    if (n <= k) return -1;
    double* x = malloc(sizeof(double) * (size_t)(n * d));
    double* W = malloc(sizeof(double) * (size_t)(n * K));      /* [n][k + d]: w, then x */
    double* mean = malloc(sizeof(double) * (size_t)K);
    double* M = malloc(sizeof(double) * (size_t)(K * k));      /* rows < k: G then L; rows k + j: S^T, y, b */
    double* z = malloc(sizeof(double) * (size_t)d);
    const int64_t n4 = 4 * ((n + 3) / 4), k4 = 4 * ((k + 3) / 4);
    for (int64_t c = 0; c < C; ++c) {
        for (int64_t t = 0; t < n; ++t) {
            for (int64_t j = 0; j < d; ++j) {
                x[t * d + j] = samples[(t * d + j) * C + c];
                z[j] = -0.5 * grads[(t * d + j) * C + c];
            }
            zv_w(order, d, x + t * d, z, W + t * K);
            for (int64_t j = 0; j < d; ++j) W[t * K + k + j] = x[t * d + j];
        }
        for (int64_t i = 0; i < K; ++i) {
            double s = 0.0;
            int same = 1;
            for (int64_t t = 0; t < n; ++t) {
                s = s + W[t * K + i];
                same = same && W[t * K + i] == W[i];
            }
            mean[i] = same ? W[i] : s / (double)n;             /* a constant column centres to exact zeros */
        }
        for (int64_t i = 0; i < K; ++i)
            for (int64_t m = 0; m < k && m <= i; ++m) {
                double s = 0.0;
                for (int64_t t = 0; t < n4; ++t) {
                    const double a = t < n ? W[t * K + i] - mean[i] : 0.0;
                    const double b = t < n ? W[t * K + m] - mean[m] : 0.0;
                    s = fma(a, b, s);
                }
                M[i * k + m] = s;
            }
        /* kept steps that differ from the one before: the centred rows span at most `moves` dimensions */
        int64_t moves = 0;
        for (int64_t t = 1; t < n; ++t) {
            int ch = 0;
            for (int64_t i = 0; i < K; ++i) ch = ch || W[t * K + i] != W[(t - 1) * K + i];
            moves += ch;
        }
        int32_t bad = moves < k ? (int32_t)(moves + 1) : 0;
        for (int64_t m = 0; m < k && !bad; ++m) {
            double s = M[m * k + m];
            for (int64_t q = 0; q < m; ++q) s = fma(-M[m * k + q], M[m * k + q], s);
            if (!(s > 0.0) || !(s < INFINITY)) {
                bad = (int32_t)(m + 1);
                break;
            }
            const double r = sqrt(s);
            M[m * k + m] = r;
            for (int64_t i = m + 1; i < K; ++i) {
                s = M[i * k + m];
                for (int64_t q = 0; q < m; ++q) s = fma(-M[i * k + q], M[m * k + q], s);
                M[i * k + m] = s / r;
            }
        }
        if (!bad)
            for (int64_t m = k - 1; m >= 0; --m)
                for (int64_t j = 0; j < d; ++j) {
                    double s = M[(k + j) * k + m];
                    for (int64_t q = k - 1; q > m; --q) s = fma(-M[q * k + m], M[(k + j) * k + q], s);
                    M[(k + j) * k + m] = s / M[m * k + m];
                }
        if (info) info[c] = bad;
        if (coef)
            for (int64_t i = 0; i < k; ++i)
                for (int64_t j = 0; j < d; ++j) coef[(i * d + j) * C + c] = bad ? zv_nan() : -M[(k + j) * k + i];
        for (int64_t t = 0; t < n; ++t)
            for (int64_t j = 0; j < d; ++j) {
                double s = 0.0;
                for (int64_t i = 0; i < k4; ++i) {
                    const double w = i < k ? W[t * K + i] : 0.0;
                    const double a = i < k ? -M[(k + j) * k + i] : 0.0;
                    s = fma(w, a, s);
                }
                zv[(t * d + j) * C + c] = bad ? zv_nan() : x[t * d + j] + s;
            }
    }
    free(x);
    free(W);
    free(mean);
    free(M);
    free(z);
    return 0;
}
