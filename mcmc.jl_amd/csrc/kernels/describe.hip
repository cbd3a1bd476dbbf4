// describe.hip -- describe(chain) on the device (src/stats/summary.jl:24-55): per-chain and pooled posterior summaries
// of a batched MCMCChain's kept samples [nkept][d][C].
//
// (a) k_desc_reg<32|64|96>, k_desc_tile, k_desc_col: the per-series pass.  They are stats.hip's three ESS kernels (the
//     same size classes, staging, lag sums and scan, on ess_device.hpp's pieces; IMSE) with the extremes of the series
//     riding the sum that already has every value in a register, and the six columns min, mean, max, mcerror, ess,
//     actime stored instead of one: one read of the samples.  The same pass leaves ss and varimse per series for (b).
// (b) k_desc_pool / k_desc_pool_final: the pooled rows from those per-series values, never from the samples, every
//     floating-point sum over chains in one order fixed by C alone (below).
// (c) k_desc_hist / k_desc_scan / k_desc_quant: exact pooled quantiles by a most-significant-digit-first radix select on
//     order-preserving 64-bit keys, eight passes of eight bits, integer counts only.
#include "ess_device.hpp"

#include <math.h>

namespace mcmc {

// one series' results.  mn .. act are the table's columns [d][C] (all NULL when the table is not asked for); wmn, wmean,
// wmx, wss, wvar what the pooled rows read (all NULL when they are not; wmn, wmean, wmx alias the table's columns when
// both are).
struct DescOut {
    double *mn, *mean, *mx, *mcerr, *ess, *act;
    double *wmn, *wmean, *wmx, *wss, *wvar;
    // what is known once the series has been summed (k_desc_reg stores it before its lag loop: the three values
    // would otherwise sit in registers the loop needs)
    __device__ __forceinline__ void store_head(size_t o, double m, double lo, double hi) const {
        lo = lo + 0.0;                                         // -0 -> +0
        hi = hi + 0.0;
        if (mn) {
            mn[o] = lo;
            mean[o] = m;
            mx[o] = hi;
        }
        if (wss && wmn != mn) {
            wmn[o] = lo;
            wmean[o] = m;
            wmx[o] = hi;
        }
    }
    __device__ __forceinline__ void store_tail(size_t o, double nd, double ss, double var_v) const {
        if (mn) {
            const double var_iid = (ss / (nd - 1.0)) / nd;     // summary.jl:35-42
            mcerr[o] = sqrt(var_v);
            ess[o] = (nd * var_iid) / var_v;                   // ess.jl:9, bit for bit mcmc_stats_ess's
            act[o] = var_v / var_iid;                          // ess.jl:17
        }
        if (wss) {
            wss[o] = ss;
            wvar[o] = var_v;
        }
    }
    __device__ __forceinline__ void store(size_t o, double nd, double m, double lo, double hi, double ss,
                                          double var_v) const {
        store_head(o, m, lo, hi);
        store_tail(o, nd, ss, var_v);
    }
};

constexpr int32_t kDescVtype = 1;      // describe's variance is IMSE (summary.jl:38); EssArgs' vtype, batchlen, ess and
                                       // var are not read by the k_desc_* kernels

// the extremes of a series, a NaN sample passed over (v_min_f64 / v_max_f64)
__device__ __forceinline__ void desc_minmax(double v, double& mn, double& mx) {
    mn = __builtin_fmin(mn, v);
    mx = __builtin_fmax(mx, v);
}

__global__ __launch_bounds__(kEssThreads) void k_desc_tile(EssArgs a, DescOut out) {
    extern __shared__ __attribute__((aligned(16))) double tile[];   // [32][S]: x, then z = x - mean, zero pad
    const int tid = (int)threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * kEssTile;
    const int64_t j = blockIdx.y;
    const int n = (int)a.n;
    const int S = ess_stride(n);
    const size_t stride = (size_t)a.d * (size_t)a.C;
    const double* base = a.s + (size_t)j * (size_t)a.C;
    // stage: rows of 32 chains (256 B) from HBM, 4 rows per pass of the block, transposed into the series-major
    // tile; then the zero pad
    {
        const int cc = tid & 31;
        const bool live = c0 + cc < a.C;
        const double* col = base + (size_t)(live ? c0 + cc : 0);
        double* dst = tile + cc * S;
        // every row of a 96-row pass requested before the first is written to LDS (24 loads in flight per thread:
        // the staging is latency-bound otherwise, a block's whole tile being one HBM round trip)
        for (int t0 = tid >> 5; t0 < n; t0 += 96) {
            double v[24];
#pragma unroll
            for (int u = 0; u < 24; ++u) {
                const int t = t0 + 4 * u;
                v[u] = (live && t < n) ? col[(size_t)t * stride] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 24; ++u)
                if (t0 + 4 * u < n) dst[t0 + 4 * u] = v[u];
        }
        for (int t2 = n + (tid >> 5); t2 < S; t2 += 4) dst[t2] = 0.0;
    }
    __syncthreads();
    const int sr = tid >> 2, q = tid & 3;                      // series and lane within its group
    double* zc = tile + sr * S;
    const double nd = (double)n;
    double ss = 0.0, var_v = 0.0, mean = 0.0, mn = 0.0, mx = 0.0;
    if (q == 0) {
        // mean (mean.jl:6), left to right; 16 steps of LDS reads in flight per block of the dependent adds
        double sum = 0.0;
        int t = 0;
        mn = mx = zc[0];
        for (; t + 16 <= n; t += 16) {
            ess_f64x2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const ess_f64x2*>(zc + t + 2 * u);
#pragma unroll
            for (int u = 0; u < 8; ++u) sum = (sum + v[u].x) + v[u].y;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                desc_minmax(v[u].x, mn, mx);
                desc_minmax(v[u].y, mn, mx);
            }
        }
        for (; t < n; ++t) {
            sum = sum + zc[t];
            desc_minmax(zc[t], mn, mx);
        }
        mean = sum / nd;
        // centre in place; ss = sum of z^2 with the lag sums' fma chain
        for (t = 0; t + 16 <= n; t += 16) {
            ess_f64x2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const ess_f64x2*>(zc + t + 2 * u);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                v[u].x = v[u].x - mean;
                v[u].y = v[u].y - mean;
                ss = __builtin_fma(v[u].x, v[u].x, ss);
                ss = __builtin_fma(v[u].y, v[u].y, ss);
                *reinterpret_cast<ess_f64x2*>(zc + t + 2 * u) = v[u];
            }
        }
        for (; t < n; ++t) {
            const double z = zc[t] - mean;
            zc[t] = z;
            ss = __builtin_fma(z, z, ss);
        }
    }
    __syncthreads();
    const int gl = (tid & 63) & ~3;                            // the group's first lane in the wave
    ss = __shfl(ss, gl, 64);
    const double acv0 = ss / nd;
    {
        const int64_t k = (a.maxlag - 1) >= 0 ? (a.maxlag - 1) / 2 : -1;
        double gsum = 0.0, prev = 0.0;
        bool done = k < 0;
        // round 0: one pair per lane (pairs 0-3; nearly independent draws stop there), then 4 pairs per lane
        ess_round<2>(zc, n, nd, 0, q, gl, k, kDescVtype, done, prev, gsum);
        for (int64_t p0 = 4; !__all(done); p0 += 16) ess_round<8>(zc, n, nd, p0, q, gl, k, kDescVtype, done, prev, gsum);
        var_v = (-acv0 + 2.0 * gsum) / nd;
    }
    const int64_t c = c0 + sr;
    if (q == 0 && c < a.C) out.store((size_t)j * (size_t)a.C + (size_t)c, nd, mean, mn, mx, ss, var_v);
}

// Series of up to N = 32, 64 or 96 kept samples (the metric keeps 90): one lane per series, the whole series in
// registers, as stats.hip's k_ess_reg (its comment explains the zero pad and the quotient); the extremes are taken
// from the registers before they are centred, over the positions t < n only
template <int N>
__global__ __launch_bounds__(256, 2) void k_desc_reg(EssArgs a, DescOut out) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t j = blockIdx.y;
    const bool live = c < a.C;
    const int n = (int)a.n;
    const size_t stride = (size_t)a.d * (size_t)a.C;
    const double* col = a.s + (size_t)j * (size_t)a.C + (size_t)(live ? c : 0);
    double z[N];
#pragma unroll
    for (int t = 0; t < N; ++t) {
        if (t < N - 32) {
            z[t] = col[(size_t)t * stride];
        } else {                                               // the last 32 positions: rows past n read row n-1
            const double v = col[(size_t)(t < n ? t : n - 1) * stride];
            z[t] = t < n ? v : 0.0;
        }
    }
    const double nd = (double)n;
    // s / n for the autocovariances: q0 = RN(s rn), then one correction with the exact residual (fma).  With rn the
    // correctly rounded 1/n and q0 faithful, q0 + (s - n q0) rn rounds to the correctly rounded s / n (Markstein's
    // theorem; no underflow here): the IEEE quotient orc_ess computes, for 3 operations instead of the ~11 of a
    // division (tests/test_oracle.py checks the identity on half a billion quotients, near-exact ones included).
    // Bitwise parity with orc_ess is claimed for normal-range sums: where z^2 is subnormal (|x| below about 2^-500)
    // the residual fma underflows and the result can differ from the IEEE quotient at a tie.
    const double rn = 1.0 / nd;
    auto qdiv = [&](double x) {
        const double q0 = x * rn;
        return __builtin_fma(__builtin_fma(-q0, nd, x), rn, q0);
    };
    double sum = 0.0;
#pragma unroll
    for (int t = 0; t < N; ++t) sum = sum + z[t];              // mean.jl:6, left to right; the zero pad adds +0
    const double mean = sum / nd;
    double mn = z[0], mx = z[0];
#pragma unroll
    for (int t = 1; t < N; ++t)
        if (t < N - 32 || t < n) desc_minmax(z[t], mn, mx);
    const size_t o = (size_t)j * (size_t)a.C + (size_t)c;
    if (live) out.store_head(o, mean, mn, mx);
#pragma unroll
    for (int t = 0; t < N; ++t) z[t] = (t < N - 32 || t < n) ? z[t] - mean : 0.0;
    // the lag-0 sum is ss (the same fma chain): it runs as the first of step 0's four chains
    double ss = 0.0, acv0 = 0.0;
    const int64_t k = (a.maxlag - 1) >= 0 ? (a.maxlag - 1) / 2 : -1;
    double gsum = 0.0, prev = 0.0;
    bool done = k < 0 || !live;
#pragma unroll
    for (int jp = 0; jp < N / 2; jp += 2) {                    // pairs jp, jp + 1: lags 2 jp .. 2 jp + 3
        if (jp > 0 && __ballot(!done) == 0) break;
        double sl[4] = {0.0, 0.0, 0.0, 0.0};
        auto lag_terms = [&](int t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int L = 2 * jp + i;
                if (t + L < N) sl[i] = __builtin_fma(z[t], z[t + L], sl[i]);
            }
        };
        // t in blocks of 4; once z[t + 2 jp] can be the zero pad (t + 2 jp >= N - 32), a block starting at or past
        // n - 2 jp (a uniform test) ends the sums: every term left is fma(z, 0, s) = s
#pragma unroll
        for (int tb = 0; tb < N; tb += 4) {
            if (tb + 2 * jp >= N - 32 && tb + 2 * jp >= n) break;
#pragma unroll
            for (int t = tb; t < tb + 4; ++t) lag_terms(t);
        }
        if (jp == 0) {
            ss = sl[0];
            acv0 = qdiv(ss);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int jj = jp + h;
            if (jj >= N / 2) break;
            const double g = (jj == 0 ? acv0 : qdiv(sl[2 * h])) + qdiv(sl[2 * h + 1]);   // acv[2j] + acv[2j+1]
            if (!done) done = jj > k || !geyer_take(g, jj, kDescVtype, prev, gsum);
        }
    }
    if (live) {
        const double var_v = (-acv0 + 2.0 * gsum) / nd;
        out.store_tail(o, nd, ss, var_v);
    }
}

// long series (n > kEssTileMaxN): one thread per series, the column re-read from global memory per lag
__global__ __launch_bounds__(kEssBlock) void k_desc_col(EssArgs a, DescOut out) {
    const int64_t c = (int64_t)blockIdx.x * kEssBlock + threadIdx.x;
    const int64_t j = blockIdx.y;
    const bool live = c < a.C;
    const int64_t n = a.n;
    const size_t stride = (size_t)a.d * (size_t)a.C;
    const double* col = a.s + (size_t)j * (size_t)a.C + (size_t)(live ? c : 0);
    auto x = [&](int64_t t) { return col[(size_t)t * stride]; };
    double sum = 0.0, mn = 0.0, mx = 0.0;
    mn = mx = x(0);
    for (int64_t t = 0; t < n; ++t) {
        const double v = x(t);
        sum = sum + v;
        desc_minmax(v, mn, mx);
    }
    const double nd = (double)n;
    const double mean = sum / nd;
    double ss = 0.0;
    for (int64_t t = 0; t < n; ++t) {
        const double z = x(t) - mean;
        ss = __builtin_fma(z, z, ss);
    }
    const int64_t k = (a.maxlag - 1) >= 0 ? (a.maxlag - 1) / 2 : -1;
    double gsum = 0.0, prev = 0.0;
    for (int64_t jj = 0; jj <= k; ++jj) {
        const int64_t L0 = 2 * jj, L1 = L0 + 1;
        double s0 = 0.0, s1 = 0.0;
        for (int64_t t = 0; t + L1 < n; ++t) {
            const double zt = x(t) - mean;
            s0 = __builtin_fma(zt, x(t + L0) - mean, s0);
            s1 = __builtin_fma(zt, x(t + L1) - mean, s1);
        }
        s0 = __builtin_fma(x(n - 1 - L0) - mean, x(n - 1) - mean, s0);
        if (!geyer_take(s0 / nd + s1 / nd, jj, kDescVtype, prev, gsum)) break;
    }
    const double var_v = (-(ss / nd) + 2.0 * gsum) / nd;
    if (live) out.store((size_t)j * (size_t)a.C + (size_t)c, nd, mean, mn, mx, ss, var_v);
}

// ------------------------------------------------------------------ (b) pooled rows
// The order of every sum over chains (tests/describe_oracle.c dsc_reduce): chains in blocks of 4096; in
// block b lane l of 256 adds its chains 4096 b + 256 k + l, k = 0..15, left to right from +0; each wave's xor butterfly
// 32..1; the four wave sums left to right; k_desc_pool_final adds the block sums left to right from +0.  A chain past
// C or one left out of a sum is a +0 term.  The extremes and the census are exact in any order.
constexpr int kPoolBlock = 4096;
constexpr int kPoolLanes = 256;
constexpr int kPoolParts = 7;          // pass 0: mean, s2, varimse, ess, min, max, bad; pass 1: (mean - grand mean)^2

struct PoolArgs {
    const double *mn, *mean, *mx, *ss, *var;   // [d][C], from the per-series pass
    int64_t n, d, C, nb;
    double* part;                              // [kPoolParts][d][nb]
    double* pooled;                            // [6 + nprobs][d]
    double* scal;                              // [d]: W between the passes
    long long* nbad;                           // [d] or NULL
};

__device__ __forceinline__ double pool_wave_sum(double x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = x + __shfl_xor(x, m, 64);
    return x;
}

// the block's value of one quantity from its lanes' partial sums, on thread 0
__device__ __forceinline__ double pool_block_sum(double x, double* wsum) {
    x = pool_wave_sum(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

template <int PASS>
__global__ __launch_bounds__(kPoolLanes) void k_desc_pool(PoolArgs a) {
    __shared__ double wsum[kPoolLanes / 64];
    const int l = (int)threadIdx.x;
    const int64_t b = blockIdx.x, j = blockIdx.y;
    const size_t row = (size_t)j * (size_t)a.C;
    const size_t po = (size_t)j * (size_t)a.nb + (size_t)b, ps = (size_t)a.d * (size_t)a.nb;
    const double nd = (double)a.n;
    if (PASS == 0) {
        double sm = 0.0, s2 = 0.0, sv = 0.0, se = 0.0, bad = 0.0, lo = 0.0, hi = 0.0;
        bool any = false;
        for (int k = 0; k < kPoolBlock / kPoolLanes; ++k) {
            const int64_t c = b * kPoolBlock + (int64_t)k * kPoolLanes + l;
            if (c >= a.C) break;                               // the +0 terms of the chains past C
            const double ss = a.ss[row + c], var_v = a.var[row + c];
            const double var_iid = (ss / (nd - 1.0)) / nd;
            const double ess = (nd * var_iid) / var_v;
            const bool good = isfinite(var_v) && isfinite(ess) && var_v > 0.0;
            sm = sm + a.mean[row + c];
            s2 = s2 + ss / (nd - 1.0);
            sv = sv + (good ? var_v : 0.0);
            se = se + (good ? ess : 0.0);
            bad = bad + (good ? 0.0 : 1.0);
            const double cmn = a.mn[row + c], cmx = a.mx[row + c];
            lo = any ? __builtin_fmin(lo, cmn) : cmn;
            hi = any ? __builtin_fmax(hi, cmx) : cmx;
            any = true;
        }
        // lanes without a chain: the block's first chain (every block has one) stands in for their extremes
        const double lo0 = a.mn[row + b * kPoolBlock], hi0 = a.mx[row + b * kPoolBlock];
        if (!any) {
            lo = lo0;
            hi = hi0;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            lo = __builtin_fmin(lo, __shfl_xor(lo, m, 64));
            hi = __builtin_fmax(hi, __shfl_xor(hi, m, 64));
        }
        __shared__ double wlo[kPoolLanes / 64], whi[kPoolLanes / 64];
        if ((l & 63) == 0) {
            wlo[l >> 6] = lo;
            whi[l >> 6] = hi;
        }
        const double bm = pool_block_sum(sm, wsum), b2 = pool_block_sum(s2, wsum), bv = pool_block_sum(sv, wsum),
                     be = pool_block_sum(se, wsum), bb = pool_block_sum(bad, wsum);
        if (l == 0) {
            a.part[0 * ps + po] = bm;
            a.part[1 * ps + po] = b2;
            a.part[2 * ps + po] = bv;
            a.part[3 * ps + po] = be;
            a.part[4 * ps + po] = __builtin_fmin(__builtin_fmin(wlo[0], wlo[1]), __builtin_fmin(wlo[2], wlo[3]));
            a.part[5 * ps + po] = __builtin_fmax(__builtin_fmax(whi[0], whi[1]), __builtin_fmax(whi[2], whi[3]));
            a.part[6 * ps + po] = bb;
        }
    } else {
        const double gm = a.pooled[1 * a.d + j];
        double s = 0.0;
        for (int k = 0; k < kPoolBlock / kPoolLanes; ++k) {
            const int64_t c = b * kPoolBlock + (int64_t)k * kPoolLanes + l;
            if (c >= a.C) break;
            const double e = a.mean[row + c] - gm;
            s = s + e * e;
        }
        const double bs = pool_block_sum(s, wsum);
        if (l == 0) a.part[0 * ps + po] = bs;
    }
}

template <int PASS>
__global__ __launch_bounds__(64) void k_desc_pool_final(PoolArgs a) {
    const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= a.d) return;
    const size_t ps = (size_t)a.d * (size_t)a.nb;
    const double* p = a.part + (size_t)j * (size_t)a.nb;
    const double nd = (double)a.n, Cd = (double)a.C;
    if (PASS == 0) {
        double sm = 0.0, s2 = 0.0, sv = 0.0, se = 0.0, bad = 0.0, lo = p[4 * ps], hi = p[5 * ps];
        for (int64_t b = 0; b < a.nb; ++b) {
            sm = sm + p[0 * ps + b];
            s2 = s2 + p[1 * ps + b];
            sv = sv + p[2 * ps + b];
            se = se + p[3 * ps + b];
            lo = __builtin_fmin(lo, p[4 * ps + b]);
            hi = __builtin_fmax(hi, p[5 * ps + b]);
            bad = bad + p[6 * ps + b];                         // whole numbers: exact
        }
        a.pooled[0 * a.d + j] = lo;
        a.pooled[1 * a.d + j] = sm / Cd;
        a.pooled[2 * a.d + j] = hi;
        a.pooled[3 * a.d + j] = sqrt(sv) / (Cd - bad);
        a.pooled[4 * a.d + j] = se;
        a.scal[j] = s2 / Cd;
        if (a.nbad) a.nbad[j] = (long long)bad;
    } else {
        double s = 0.0;
        for (int64_t b = 0; b < a.nb; ++b) s = s + p[b];
        const double W = a.scal[j], Bn = s / (Cd - 1.0);
        a.pooled[5 * a.d + j] =
            (a.C == 1 || W == 0.0) ? __builtin_nan("") : sqrt((((nd - 1.0) / nd) * W + Bn) / W);
    }
}

// ------------------------------------------------------------------ (c) exact pooled quantiles: radix select
constexpr int kQT = 16;                // target ranks a parameter: lo and lo + 1 of up to 8 probabilities
constexpr int kQBins = 256;            // 8 passes of 8 bits, most significant digit first
constexpr int kQPasses = 8;
constexpr int kQThreads = 256;
constexpr int kQChains = 256;          // chains a block of k_desc_hist owns: one a thread
constexpr int kQRows = 4;              // kept steps a thread loads at a time
constexpr int64_t kQSteps = 1 << 20;   // kept steps a block covers: its 32-bit LDS counts hold 2^28 elements
constexpr int kQParams = 32;           // parameters a round of launches

typedef unsigned long long u64;

struct QState {                        // one parameter's select state between the passes
    u64 prefix[kQT];                   // the digits found so far, in place (the low bits 0)
    u64 rank[kQT];                     // the target's rank among the elements that share its prefix
    u64 gprefix[kQT];                  // the distinct prefixes: one histogram each
    int32_t group[kQT];                // target -> its prefix's histogram
    int32_t ngroups, pad;
};

struct QTargets {
    u64 rank[kQT];
    int32_t nt, nprobs;
    int32_t lo[8], hi[8];              // probability i -> its targets
    double f[8];
};

// order-preserving key: -0 taken as +0, NaN above +Inf; sign bit flipped for non-negatives, every bit for negatives
__device__ __forceinline__ u64 desc_key(double x) {
    if (x != x) return ~0ull;
    u64 u = (u64)__double_as_longlong(x);
    if (u == 0x8000000000000000ull) u = 0;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double desc_unkey(u64 k) {
    const u64 u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

__global__ __launch_bounds__(64) void k_desc_qinit(QState* qs, u64* hist, QTargets tg) {
    QState& q = qs[blockIdx.x];
    const int t = (int)threadIdx.x;
    if (t < kQT) {
        q.prefix[t] = 0;
        q.rank[t] = t < tg.nt ? tg.rank[t] : 0;
        q.gprefix[t] = 0;
        q.group[t] = 0;
    }
    if (t == 0) q.ngroups = 1;
    u64* h = hist + (size_t)blockIdx.x * kQT * kQBins;
    for (int i = t; i < kQT * kQBins; i += 64) h[i] = 0;
}

// digit `pass` of every element of parameter j0 + blockIdx.y that matches a target prefix, counted per prefix: LDS
// integer atomics, then one 64-bit integer atomic per non-empty bin to HBM
__global__ __launch_bounds__(kQThreads) void k_desc_hist(const double* s, int64_t n, int64_t d, int64_t C, int64_t j0,
                                                         int pass, const QState* qs, u64* hist) {
    __shared__ unsigned int h[kQT * kQBins];
    __shared__ u64 gp[kQT];
    const int tid = (int)threadIdx.x;
    const int jj = (int)blockIdx.y;
    const QState& q = qs[jj];
    const int ng = q.ngroups;
    for (int i = tid; i < ng * kQBins; i += kQThreads) h[i] = 0;
    if (tid < kQT) gp[tid] = q.gprefix[tid];
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const u64 mask = pass == 0 ? 0ull : ~0ull << (shift + 8);
    const int64_t c = (int64_t)blockIdx.x * kQChains + tid;
    const bool live = c < C;
    const int64_t t0 = (int64_t)blockIdx.z * kQSteps, t1 = t0 + kQSteps < n ? t0 + kQSteps : n;
    const size_t stride = (size_t)d * (size_t)C;
    const double* col = s + (size_t)(j0 + jj) * (size_t)C + (size_t)(live ? c : 0);
    for (int64_t t = t0; live && t < t1; t += kQRows) {        // kQRows rows of loads in flight
        double v[kQRows];
#pragma unroll
        for (int u = 0; u < kQRows; ++u) v[u] = col[(size_t)(t + u < t1 ? t + u : t1 - 1) * stride];
#pragma unroll
        for (int u = 0; u < kQRows; ++u) {
            if (t + u >= t1) continue;
            const u64 key = desc_key(v[u]);
            const u64 pre = key & mask;
            const unsigned dg = (unsigned)(key >> shift) & (kQBins - 1);
            for (int g = 0; g < ng; ++g)
                if (pre == gp[g]) {
                    atomicAdd(&h[g * kQBins + dg], 1u);
                    break;
                }
        }
    }
    __syncthreads();
    u64* out = hist + (size_t)jj * kQT * kQBins;
    for (int i = tid; i < ng * kQBins; i += kQThreads)
        if (h[i]) atomicAdd(&out[i], (u64)h[i]);
}

// between the passes: every target's next digit and its rank inside that bin, the distinct prefixes, and the
// histograms cleared for the next pass
__global__ __launch_bounds__(64) void k_desc_scan(int pass, int nt, QState* qs, u64* hist) {
    QState& q = qs[blockIdx.x];
    u64* hj = hist + (size_t)blockIdx.x * kQT * kQBins;
    const int t = (int)threadIdx.x;
    if (t < nt) {
        const u64* H = hj + (size_t)q.group[t] * kQBins;
        const u64 r = q.rank[t];
        u64 cum = 0;
        int b = 0;
        for (; b < kQBins - 1; ++b) {
            const u64 hb = H[b];
            if (r < cum + hb) break;
            cum += hb;
        }
        q.prefix[t] |= (u64)b << (56 - 8 * pass);
        q.rank[t] = r - cum;
    }
    __syncthreads();
    if (t == 0) {
        int ng = 0;
        for (int i = 0; i < nt; ++i) {
            int g = 0;
            while (g < ng && q.gprefix[g] != q.prefix[i]) ++g;
            if (g == ng) q.gprefix[ng++] = q.prefix[i];
            q.group[i] = g;
        }
        q.ngroups = ng;
    }
    for (int i = t; i < kQT * kQBins; i += 64) hj[i] = 0;
}

// Julia's quantile (type 7) from the two order statistics of each probability: plain multiply and add
__global__ __launch_bounds__(64) void k_desc_quant(const QState* qs, QTargets tg, int64_t j0, int64_t nj, int64_t d,
                                                   double* qrows) {
    const int64_t jj = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (jj >= nj) return;
    for (int i = 0; i < tg.nprobs; ++i) {
        const double vlo = desc_unkey(qs[jj].prefix[tg.lo[i]]), vhi = desc_unkey(qs[jj].prefix[tg.hi[i]]);
        const double diff = vhi - vlo;
        const double prod = tg.f[i] * diff;
        qrows[(size_t)i * (size_t)d + (size_t)(j0 + jj)] = vlo + prod;
    }
}

static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace mcmc

size_t mcmc_describe_ws_bytes(int64_t d, int64_t C, int has_per_chain, int has_pooled, int32_t nprobs) {
    using namespace mcmc;
    if (!has_pooled) return 0;
    const size_t dC = (size_t)d * (size_t)C, nb = (size_t)((C + kPoolBlock - 1) / kPoolBlock);
    size_t b = up256((has_per_chain ? 2 : 5) * dC * 8) + up256(kPoolParts * (size_t)d * nb * 8) + up256((size_t)d * 8);
    if (nprobs > 0) b += up256(kQParams * sizeof(QState)) + up256((size_t)kQParams * kQT * kQBins * 8);
    return b;
}

hipError_t mcmc_launch_describe(const double* samples, int64_t n, int64_t d, int64_t C, int64_t maxlag,
                                double* per_chain, const double* probs, int32_t nprobs, double* pooled, int64_t* nbad,
                                void* ws, hipStream_t st) {
    using namespace mcmc;
    const size_t dC = (size_t)d * (size_t)C, nb = (size_t)((C + kPoolBlock - 1) / kPoolBlock);
    char* w = (char*)ws;
    DescOut o{};
    if (per_chain) {
        o.mn = per_chain;
        o.mean = per_chain + dC;
        o.mx = per_chain + 2 * dC;
        o.mcerr = per_chain + 3 * dC;
        o.ess = per_chain + 4 * dC;
        o.act = per_chain + 5 * dC;
    }
    double *part = nullptr, *scal = nullptr;
    if (pooled) {
        double* sw = (double*)w;
        w += up256((per_chain ? 2 : 5) * dC * 8);
        o.wss = sw;
        o.wvar = sw + dC;
        o.wmn = per_chain ? o.mn : sw + 2 * dC;
        o.wmean = per_chain ? o.mean : sw + 3 * dC;
        o.wmx = per_chain ? o.mx : sw + 4 * dC;
        part = (double*)w;
        w += up256(kPoolParts * (size_t)d * nb * 8);
        scal = (double*)w;
        w += up256((size_t)d * 8);
    }
    // (a) the per-series pass: mcmc_launch_ess's size classes
    EssArgs a{samples, n, d, C, maxlag, 0, 1, nullptr, nullptr};
    if (n <= 96) {
        const dim3 grid((unsigned)((C + 255) / 256), (unsigned)d);
        if (n <= 32) k_desc_reg<32><<<grid, 256, 0, st>>>(a, o);
        else if (n <= 64) k_desc_reg<64><<<grid, 256, 0, st>>>(a, o);
        else k_desc_reg<96><<<grid, 256, 0, st>>>(a, o);
    } else if (n <= kEssTileMaxN) {
        const size_t lds = (size_t)kEssTile * ess_stride((int)n) * sizeof(double);
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)k_desc_tile, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds);
            if (e != hipSuccess) return e;
        }
        const dim3 grid((unsigned)((C + kEssTile - 1) / kEssTile), (unsigned)d);
        k_desc_tile<<<grid, kEssThreads, lds, st>>>(a, o);
    } else {
        const dim3 grid((unsigned)((C + kEssBlock - 1) / kEssBlock), (unsigned)d);
        k_desc_col<<<grid, kEssBlock, 0, st>>>(a, o);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !pooled) return e;
    // (b) the pooled rows
    PoolArgs p{o.wmn, o.wmean, o.wmx, o.wss, o.wvar, n, d, C, (int64_t)nb, part, pooled, scal, (long long*)nbad};
    const dim3 pgrid((unsigned)nb, (unsigned)d);
    const unsigned fgrid = (unsigned)((d + 63) / 64);
    k_desc_pool<0><<<pgrid, kPoolLanes, 0, st>>>(p);
    k_desc_pool_final<0><<<fgrid, 64, 0, st>>>(p);
    k_desc_pool<1><<<pgrid, kPoolLanes, 0, st>>>(p);
    k_desc_pool_final<1><<<fgrid, 64, 0, st>>>(p);
    e = hipGetLastError();
    if (e != hipSuccess || nprobs <= 0) return e;
    // (c) the quantiles: the distinct target ranks, then per round of kQParams parameters eight histogram passes
    QTargets tg{};
    const u64 N = (u64)n * (u64)C;
    tg.nprobs = nprobs;
    auto target = [&](u64 r) {
        for (int i = 0; i < tg.nt; ++i)
            if (tg.rank[i] == r) return i;
        tg.rank[tg.nt] = r;
        return tg.nt++;
    };
    for (int i = 0; i < nprobs; ++i) {
        const double h = (double)(N - 1) * probs[i];
        const double fl = floor(h);
        const u64 lo = (u64)fl;
        tg.f[i] = h - fl;
        tg.lo[i] = target(lo);
        tg.hi[i] = target(lo + 1 < N - 1 ? lo + 1 : N - 1);
    }
    QState* qs = (QState*)w;
    w += up256(kQParams * sizeof(QState));
    u64* hist = (u64*)w;
    double* qrows = pooled + 6 * (size_t)d;
    for (int64_t j0 = 0; j0 < d; j0 += kQParams) {
        const int64_t nj = d - j0 < kQParams ? d - j0 : kQParams;
        k_desc_qinit<<<(unsigned)nj, 64, 0, st>>>(qs, hist, tg);
        const dim3 hgrid((unsigned)((C + kQChains - 1) / kQChains), (unsigned)nj, (unsigned)((n + kQSteps - 1) / kQSteps));
        for (int pass = 0; pass < kQPasses; ++pass) {
            k_desc_hist<<<hgrid, kQThreads, 0, st>>>(samples, n, d, C, j0, pass, qs, hist);
            k_desc_scan<<<(unsigned)nj, 64, 0, st>>>(pass, tg.nt, qs, hist);
        }
        k_desc_quant<<<(unsigned)((nj + 63) / 64), 64, 0, st>>>(qs, tg, j0, nj, d, qrows);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}
