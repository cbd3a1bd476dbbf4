// ess_device.hpp -- the pieces the per-series kernels over a batched MCMCChain's kept samples share
// (src/stats/ess.jl:6-10, var.jl:7-8,20-27,45-117): the size classes and the LDS tile geometry, the kernel arguments,
// batch means, Geyer's scan step, the lag sums and the lane-group round.  stats.hip's k_ess_* (the ESS and the variance)
// and describe.hip's k_desc_* (the six columns of describe's table in the same single read) are built on them.
// The kernels' layout and their arithmetic order are described at the top of stats.hip.
#pragma once
#include "../common.hpp"
#include "../host/kernels_api.hpp"

namespace mcmc {

constexpr int kEssBlock = 64;          // k_ess_col: one thread per series
constexpr int kEssTile = 32;           // k_ess_tile: series per block
constexpr int kEssThreads = 128;       // k_ess_tile: 4 lanes per series
// k_ess_tile's LDS tile is series-major, [32][S] doubles: a series is contiguous in t, so two consecutive steps
// come in one ds_read_b128.  S >= n + 16 (a zero pad: the lag loops run in whole 8-step blocks and read up to 15
// past the series' end) and S = 2 mod 8: the 16 lanes of a ds_read_b128 lane group (4 series x 4 lanes whose
// windows sit 8 steps apart) then cover the 64 banks once.
__host__ __device__ constexpr int ess_stride(int n) { return n + 16 + (((2 - (n + 16)) % 8) + 8) % 8; }
constexpr int kEssTileMaxN = 618;      // 32 x ess_stride(618) x 8 B = 162 304 B: fits the 160 KB of LDS
static_assert(32 * ess_stride(kEssTileMaxN) * 8 <= 160 * 1024 && 32 * ess_stride(kEssTileMaxN + 1) * 8 > 160 * 1024,
              "kEssTileMaxN is the largest series the LDS tile holds");

typedef double ess_f64x2 __attribute__((ext_vector_type(2)));

struct EssArgs {
    const double* s;
    int64_t n, d, C;
    int64_t maxlag;
    int64_t batchlen;
    int32_t vtype;        // 1 imse, 2 ipse, 3 bm
    double* ess;          // [d][C]
    double* var;          // [d][C] or NULL: the vtype variance of the mean
};

// batch means (var.jl:20-27): batchlen * var(batch means) / (nbatches * batchlen); x(t) = the raw series
template <class X>
__device__ __forceinline__ double ess_bm(const X& x, int64_t n, int64_t bl) {
    const int64_t nb = n / bl;
    double bsum = 0.0;
    for (int64_t b = 0; b < nb; ++b) {
        double s = 0.0;
        for (int64_t t = b * bl; t < (b + 1) * bl; ++t) s = s + x(t);
        bsum = bsum + s / (double)bl;
    }
    const double bmean = bsum / (double)nb;
    double bss = 0.0;
    for (int64_t b = 0; b < nb; ++b) {
        double s = 0.0;
        for (int64_t t = b * bl; t < (b + 1) * bl; ++t) s = s + x(t);
        const double e = s / (double)bl - bmean;
        bss = bss + e * e;
    }
    return ((double)bl * (bss / (double)(nb - 1))) / (double)(nb * bl);
}

// Geyer's initial sequence step for pair j with pair sum g (var.jl:45-75 imse, :95-117 ipse); returns
// false at the first non-positive pair (m = j) -- the sequence ends there
__device__ __forceinline__ bool geyer_take(double g, int64_t j, int32_t vtype, double& prev, double& gsum) {
    if (g <= 0.0) return false;
    if (vtype == 1 && j > 0 && g > prev) g = prev;             // monotone: g[j] = min(g[j], g[j-1])
    prev = g;
    gsum = gsum + g;
    return true;
}

// acc[i] = sum over t < tn (tn a multiple of LPL) of z_t z_{t+L0+i}, in t order: lag L0+i's autocovariance sum
// once the zero pad has absorbed the terms past the series' end (fma(z, 0, s) = s; s is never -0).  The LPL
// values z_{t+L0} .. z_{t+L0+LPL-1} ride in a register window rotated by renaming; every two steps take one
// ds_read_b128 of (z_t, z_{t+1}) (shared by the lane group) and one of the window's next two entries.
template <int LPL>
__device__ __forceinline__ void ess_lag_sums(const double* zc, int L0, int tn, double (&acc)[LPL]) {
    double w[LPL];
#pragma unroll
    for (int i = 0; i < LPL; i += 2) {
        const ess_f64x2 v = *reinterpret_cast<const ess_f64x2*>(zc + L0 + i);
        w[i] = v.x;
        w[i + 1] = v.y;
    }
#pragma unroll
    for (int i = 0; i < LPL; ++i) acc[i] = 0.0;
    for (int t = 0; t < tn; t += LPL) {
#pragma unroll
        for (int u = 0; u < LPL; u += 2) {
            const ess_f64x2 zz = *reinterpret_cast<const ess_f64x2*>(zc + t + u);            // z_{t+u}, z_{t+u+1}
            const ess_f64x2 nw = *reinterpret_cast<const ess_f64x2*>(zc + t + u + L0 + LPL); // next window pair
#pragma unroll
            for (int i = 0; i < LPL; ++i) acc[i] = __builtin_fma(zz.x, w[(i + u) % LPL], acc[i]);
            w[u] = nw.x;                                                                     // z_{t+u+L0+LPL}
#pragma unroll
            for (int i = 0; i < LPL; ++i) acc[i] = __builtin_fma(zz.y, w[(i + u + 1) % LPL], acc[i]);
            w[u + 1] = nw.y;
        }
    }
}

// one Geyer round: lane q of the group computes pairs p0 + q LPL/2 ... (lags 2 p0 + q LPL ...), the group's
// 4 LPL/2 pair sums are shared and scanned in pair order by every lane of the group
template <int LPL>
__device__ __forceinline__ void ess_round(const double* zc, int n, double nd, int64_t p0, int q, int gl, int64_t k,
                                          int32_t vtype, bool& done, double& prev, double& gsum) {
    constexpr int PP = LPL / 2;                                // pairs per lane
    double g[PP];
#pragma unroll
    for (int i = 0; i < PP; ++i) g[i] = 0.0;
    const int64_t L0 = 2 * (p0 + (int64_t)q * PP);
    if (!done && p0 + (int64_t)q * PP <= k && L0 < n) {
        double acc[LPL];
        const int tn = (int)((n - L0 + LPL - 1) / LPL) * LPL;
        ess_lag_sums<LPL>(zc, (int)L0, tn, acc);
#pragma unroll
        for (int i = 0; i < PP; ++i) g[i] = acc[2 * i] / nd + acc[2 * i + 1] / nd;   // acv[2j] + acv[2j+1]
    }
#pragma unroll
    for (int qq = 0; qq < 4; ++qq)
#pragma unroll
        for (int i = 0; i < PP; ++i) {
            const double gi = __shfl(g[i], gl + qq, 64);
            const int64_t jp = p0 + qq * PP + i;
            if (!done) done = jp > k || !geyer_take(gi, jp, vtype, prev, gsum);
        }
}

}  // namespace mcmc
