// zv.hip -- zero-variance control-variate estimators on the device (src/stats/zv.jl:8-68; Mira, Solgi & Imparato
// 2013): linear (k = d control variates z = -grad/2) and quadratic (k = d(d+3)/2: z_j, 2 z_j x_j - 1, and
// x_i z_j + x_j z_i for i < j in zv.jl's loop order).  Per chain: a = -cov(w)^-1 cov(w, x), zv = x + w a.
//
// One kernel, k_zv<F, NTK, NTD>, runs the three passes for a tile of 16 adjacent chains; F generates the control
// variates, so linear and quadratic share all of it.  In the C-ABI layout [nkept][d][C] a (t, j) row of 16 chains
// is one 128-byte segment: the 1024 threads stage blocks of 16 kept steps of x and z = -g/2 into LDS as
// R[tt][row][chain] (row < d: x, row >= d: z; 17 doubles per row), and wave w of the workgroup then owns chain w.
//
//   pass 1  lane `col` of the wave sums column col of [w | x] left to right over t; mean = sum / n (a column that
//           never changed: its value).  The wave also counts the kept steps that differ from the one before.
//   pass 2  the wave accumulates the lower tiles of [Wc | Xc]^T Wc (centred while the operands are formed) with
//           v_mfma_f64_16x16x4_f64: the operand of 16-column tile ti is, in lane l, column 16 ti + (l & 15) at step
//           4 kb + (l >> 4), both as A and as B.  That instruction is a sequential fma chain over its k, so every
//           Gram entry is one fma chain over t in order, the last four steps padded with zeros.
//   solve   the accumulators go to a per-chain (k + d) x k block in LDS (rows < k: G, rows k + j: the right-hand
//           sides, transposed), eight chains at a time; the wave runs a right-looking Cholesky over all k + d rows
//           (which is also the forward substitution), then the back substitution, column by column from the last.
//   pass 3  zv - x = W a on the same MFMA (rows: 16 kept steps, k: the control variates in blocks of 4, a held in
//           registers as the B operands), added to x in LDS in place and stored coalesced over chains.
//
// Arithmetic order (restated bit for bit by tests/zv_oracle.c): DESIGN.md §5.5.  IEEE division and sqrt; no
// reciprocals.  A chain with fewer than k moves (rank-deficient by counting: info = moves + 1, so 1 for a chain that
// never moved) or whose pivot m is not positive and finite (info = m + 1) gets NaN; a wave touches no other chain's
// block, so its neighbours are unaffected.
#include "../common.hpp"
#include "../host/kernels_api.hpp"

namespace mcmc {

constexpr int kZvTile = 16;            // chains per workgroup, one wave each
constexpr int kZvThreads = 64 * kZvTile;
constexpr int kZvTt = 16;              // kept steps per staged block (pass 3's MFMA rows)
constexpr int kZvRow = 17;             // doubles per staged (step, row) segment of 16 chains: odd, conflict-free
constexpr int kZvLoads = 2;            // staged rows per thread in flight
constexpr int kZvSolveBatch = 8;       // chains whose (k + d) x k blocks share the LDS during the solve
constexpr int kZvMaxDLinear = 32, kZvMaxDQuadratic = 8;

typedef double zv_f64x4 __attribute__((ext_vector_type(4)));

// staged block: doubles per kept step, = 1 mod 32 (lanes that differ in step or in row then meet on at most one bank)
__host__ __device__ constexpr int zv_tstride(int d) { return 2 * d * kZvRow + (((1 - 2 * d * kZvRow) % 32) + 32) % 32; }
__host__ __device__ constexpr int zv_mstride(int k) { return k | 1; }
__host__ __device__ constexpr int zv_lds_doubles(int d, int k) {
    const int stage = kZvTt * zv_tstride(d), solve = kZvSolveBatch * (k + d) * zv_mstride(k);
    return stage > solve ? stage : solve;
}

// a column of [w | x], packed: kind | a << 8 | b << 16
enum { ZV_NONE = 0, ZV_ROW = 1, ZV_SQ = 2, ZV_PAIR = 3 };
__device__ __forceinline__ int zv_col(int kind, int a, int b) { return kind | (a << 8) | (b << 16); }

struct ZvLinear {
    static constexpr bool kQuad = false;
    static __host__ __device__ constexpr int k(int d) { return d; }
    static __device__ __forceinline__ int col(int i, int d) { return zv_col(ZV_ROW, d + i, 0); }          // z_i
};
struct ZvQuadratic {
    static constexpr bool kQuad = true;
    static __host__ __device__ constexpr int k(int d) { return d * (d + 3) / 2; }
    static __device__ __forceinline__ int col(int i, int d) {
        if (i < d) return zv_col(ZV_ROW, d + i, 0);                                                       // z_i
        if (i < 2 * d) return zv_col(ZV_SQ, i - d, 0);                                                    // 2 z_j x_j - 1
        int p = i - 2 * d, a = 0;                                                                         // zv.jl:48-53
        while (p >= d - 1 - a) { p -= d - 1 - a; ++a; }
        return zv_col(ZV_PAIR, a, a + 1 + p);
    }
};
static_assert(ZvLinear::k(kZvMaxDLinear) + kZvMaxDLinear <= 64 && ZvQuadratic::k(kZvMaxDQuadratic) + kZvMaxDQuadratic <= 64,
              "a lane per column of [w | x]");
static_assert(zv_lds_doubles(kZvMaxDLinear, ZvLinear::k(kZvMaxDLinear)) * 8 <= 160 * 1024 &&
              zv_lds_doubles(kZvMaxDQuadratic, ZvQuadratic::k(kZvMaxDQuadratic)) * 8 <= 160 * 1024, "fits the 160 KB of LDS");

// the value of packed column c at the staged step `row` points to (the wave's chain: row[r * kZvRow] is row r)
template <class F>
__device__ __forceinline__ double zv_eval(int c, const double* row, int d) {
    const int kind = c & 255, a = (c >> 8) & 255;
    if (!F::kQuad || kind == ZV_ROW) return row[a * kZvRow];
    if (kind == ZV_SQ) return (2.0 * row[(d + a) * kZvRow]) * row[a * kZvRow] - 1.0;
    const int b = c >> 16;
    return row[a * kZvRow] * row[(d + b) * kZvRow] + row[b * kZvRow] * row[(d + a) * kZvRow];
}

struct ZvArgs {
    const double* x;
    const double* g;
    int64_t n, C;
    int d, k;
    double* zv;
    double* coef;
    int32_t* info;
};

// LDS operations of one wave complete in order; the fence keeps the compiler from moving them across each other
__device__ __forceinline__ void zv_wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// Right-looking Cholesky of the wave's block M (rows 0..k-1: the lower triangle of G; rows k..k+d-1: the right-hand
// sides), then the back substitution.  On return row k + j holds b[.][j] with G b = S; the result is the failing
// pivot's 1-based index, or 0.
__device__ __forceinline__ int zv_solve(double* M, int k, int d, int ms, int lane) {
    const int R = k + d;
    for (int m = 0; m < k; ++m) {
        const double p = M[m * ms + m];
        if (!(p > 0.0) || !(p < __builtin_inf())) return m + 1;
        const double r = __builtin_sqrt(p);
        zv_wave_fence();
        for (int i = m + lane; i < R; i += 64) M[i * ms + m] = (i == m) ? r : M[i * ms + m] / r;
        zv_wave_fence();
        for (int i = m + 1 + (lane >> 3); i < R; i += 8) {
            const double lim = M[i * ms + m];
            const int je = i < k ? i : k - 1;
            for (int j = m + 1 + (lane & 7); j <= je; j += 8)
                M[i * ms + j] = __builtin_fma(-lim, M[j * ms + m], M[i * ms + j]);
        }
        zv_wave_fence();
    }
    for (int q = k - 1; q >= 0; --q) {
        const double r = M[q * ms + q];
        if (lane < d) M[(k + lane) * ms + q] = M[(k + lane) * ms + q] / r;
        zv_wave_fence();
        for (int e = lane; e < d * q; e += 64) {
            const int j = e / q, m = e - j * q;
            M[(k + j) * ms + m] = __builtin_fma(-M[q * ms + m], M[(k + j) * ms + q], M[(k + j) * ms + m]);
        }
        zv_wave_fence();
    }
    return 0;
}

template <class F, int NTK, int NTD>
__global__ __launch_bounds__(kZvThreads) void k_zv(ZvArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int NT = NTK + NTD;
    const int tid = (int)threadIdx.x, lane = tid & 63, wc = tid >> 6;
    const int d = a.d, k = a.k;
    const int64_t n = a.n;
    const int S = zv_tstride(d);
    const int64_t c0 = (int64_t)blockIdx.x * kZvTile;
    const double* Rc = lds + wc;                                // the wave's chain within the staged rows
    // staging: 16 consecutive threads take the 16 chains of one (step, coordinate) row, 64 rows per sweep
    const int cc = tid & 15, rs = tid >> 4;
    const bool clive = c0 + cc < a.C;
    const size_t cg = (size_t)(clive ? c0 + cc : 0);
    const int nrows = kZvTt * d;
    auto stage = [&](int64_t t0) {
        for (int r0 = rs; r0 < nrows; r0 += 64 * kZvLoads) {
            double xv[kZvLoads], gv[kZvLoads];
#pragma unroll
            for (int u = 0; u < kZvLoads; ++u) {
                const int r = r0 + 64 * u, tt = r / d;
                const bool ok = clive && r < nrows && t0 + tt < n;
                const size_t o = ok ? ((size_t)t0 * d + (size_t)r) * (size_t)a.C + cg : 0;
                xv[u] = ok ? a.x[o] : 0.0;
                gv[u] = ok ? a.g[o] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kZvLoads; ++u) {
                const int r = r0 + 64 * u, tt = r / d, j = r - tt * d;
                if (r < nrows) {
                    lds[tt * S + j * kZvRow + cc] = xv[u];
                    lds[tt * S + (d + j) * kZvRow + cc] = -0.5 * gv[u];                  // z = -grad / 2, exact
                }
            }
        }
    };

    // ---- pass 1: means of the columns of [w | x], lane = column
    const int mycol = lane < k ? F::col(lane, d) : lane < k + d ? zv_col(ZV_ROW, lane - k, 0) : ZV_NONE;
    double sum = 0.0, prev = 0.0, first = 0.0;
    bool col_moved = false;
    int moves = 0;                                             // kept steps that differ from the one before (wave-uniform)
    for (int64_t t0 = 0; t0 < n; t0 += kZvTt) {
        stage(t0);
        __syncthreads();
        const int m = (int)(n - t0 < kZvTt ? n - t0 : kZvTt);
        for (int tt = 0; tt < m; ++tt) {
            const double v = mycol != ZV_NONE ? zv_eval<F>(mycol, Rc + tt * S, d) : 0.0;
            sum = sum + v;
            const bool first_step = t0 == 0 && tt == 0;
            const bool ch = !first_step && v != prev;          // this column differs from the step before
            if (first_step) first = v;
            col_moved = col_moved || ch;
            moves += __ballot(ch) != 0;                        // ... and so does the chain's row of [w | x]
            prev = v;
        }
        __syncthreads();
    }
    // a column that never changed has its value as its mean and centres to exact zeros
    const double mean = col_moved ? sum / (double)n : first;

    // ---- pass 2: centred Gram tiles.  Padded column p = 16 ti + (lane & 15): w for ti < NTK, x after
    int pc[NT];
    double pm[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        const int p = 16 * ti + (lane & 15);
        int src;
        if (ti < NTK) {
            pc[ti] = p < k ? F::col(p, d) : ZV_NONE;
            src = p;
        } else {
            const int j = p - 16 * NTK;
            pc[ti] = j < d ? zv_col(ZV_ROW, j, 0) : ZV_NONE;
            src = k + j;
        }
        pm[ti] = __shfl(mean, pc[ti] != ZV_NONE ? src : 0, 64);
    }
    zv_f64x4 acc[NT][NTK];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj < NTK; ++tj) acc[ti][tj] = zv_f64x4{0.0, 0.0, 0.0, 0.0};
    for (int64_t t0 = 0; t0 < n; t0 += kZvTt) {
        stage(t0);
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < kZvTt / 4; ++kb) {
            if (t0 + 4 * kb >= n) continue;
            const int tt = 4 * kb + (lane >> 4);
            const bool live = t0 + tt < n;
            double v[NT];
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
                v[ti] = (live && pc[ti] != ZV_NONE) ? zv_eval<F>(pc[ti], Rc + tt * S, d) - pm[ti] : 0.0;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj < NTK; ++tj)
                    if (tj <= ti) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[ti], v[tj], acc[ti][tj], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- solve, eight chains at a time; a comes back as pass 3's B operands: areg[ib][tj] = a[4 ib + (lane >> 4)]
    //      [16 tj + (lane & 15)]
    const int ms = zv_mstride(k);
    double* M = lds + (size_t)(wc % kZvSolveBatch) * (size_t)((k + d) * ms);
    // fewer than k moves: the centred rows have rank <= moves < k, pivot moves + 1 is zero in exact arithmetic at the
    // latest; such a chain (one that never moved: info = 1) is marked without factorising its rounding residue
    int bad = moves < k ? moves + 1 : 0;
    double areg[4 * NTK][NTD];
    for (int b = 0; b < kZvTile / kZvSolveBatch; ++b) {
        if (wc / kZvSolveBatch == b) {
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj < NTK; ++tj) {
                    if (tj > ti) continue;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * ti + (lane >> 4) + 4 * r, j = 16 * tj + (lane & 15);
                        const int row = ti < NTK ? (i < k ? i : -1) : (i - 16 * NTK < d ? k + i - 16 * NTK : -1);
                        if (row >= 0 && j < k) M[row * ms + j] = acc[ti][tj][r];
                    }
                }
            zv_wave_fence();
            if (!bad) bad = zv_solve(M, k, d, ms, lane);
            zv_wave_fence();
            const int64_t c = c0 + wc;
            if (a.coef && c < a.C)
                for (int e = lane; e < k * d; e += 64) {
                    const int i = e / d, j = e - i * d;
                    a.coef[(size_t)e * (size_t)a.C + (size_t)c] = bad ? __builtin_nan("") : -M[(k + j) * ms + i];
                }
            if (a.info && c < a.C && lane == 0) a.info[c] = bad;
#pragma unroll
            for (int ib = 0; ib < 4 * NTK; ++ib)
#pragma unroll
                for (int tj = 0; tj < NTD; ++tj) {
                    const int i = 4 * ib + (lane >> 4), j = 16 * tj + (lane & 15);
                    areg[ib][tj] = (!bad && i < k && j < d) ? -M[(k + j) * ms + i] : 0.0;
                }
        }
        __syncthreads();
    }

    // ---- pass 3: zv = x + W a; lane's A operand: control variate 4 ib + (lane >> 4) at step lane & 15, not centred
    int wcol[4 * NTK];
#pragma unroll
    for (int ib = 0; ib < 4 * NTK; ++ib) {
        const int i = 4 * ib + (lane >> 4);
        wcol[ib] = i < k ? F::col(i, d) : ZV_NONE;
    }
    for (int64_t t0 = 0; t0 < n; t0 += kZvTt) {
        stage(t0);
        __syncthreads();
        zv_f64x4 o[NTD];
#pragma unroll
        for (int tj = 0; tj < NTD; ++tj) o[tj] = zv_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ib = 0; ib < 4 * NTK; ++ib) {
            if (4 * ib < k) {
                const double w = wcol[ib] != ZV_NONE ? zv_eval<F>(wcol[ib], Rc + (lane & 15) * S, d) : 0.0;
#pragma unroll
                for (int tj = 0; tj < NTD; ++tj)
                    o[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(w, areg[ib][tj], o[tj], 0, 0, 0);
            }
        }
        zv_wave_fence();
#pragma unroll
        for (int tj = 0; tj < NTD; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tt = (lane >> 4) + 4 * r, j = 16 * tj + (lane & 15);
                if (j < d) {
                    double* px = lds + tt * S + j * kZvRow + wc;
                    *px = bad ? __builtin_nan("") : *px + o[tj][r];
                }
            }
        __syncthreads();
        for (int r = rs; r < nrows; r += 64) {
            const int tt = r / d, j = r - tt * d;
            if (clive && t0 + tt < n)
                a.zv[((size_t)t0 * d + (size_t)r) * (size_t)a.C + cg] = lds[tt * S + j * kZvRow + cc];
        }
        __syncthreads();
    }
}

template <class F, int NTK, int NTD>
static hipError_t zv_launch(const ZvArgs& a, hipStream_t st) {
    const size_t lds = (size_t)zv_lds_doubles(a.d, a.k) * sizeof(double);
    hipError_t e = hipFuncSetAttribute((const void*)k_zv<F, NTK, NTD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return e;
    k_zv<F, NTK, NTD><<<dim3((unsigned)((a.C + kZvTile - 1) / kZvTile)), kZvThreads, lds, st>>>(a);
    return hipGetLastError();
}

}  // namespace mcmc

int mcmc_zv_max_d(int order) { return order == 1 ? mcmc::kZvMaxDLinear : order == 2 ? mcmc::kZvMaxDQuadratic : 0; }
int64_t mcmc_zv_k(int order, int64_t d) { return order == 2 ? d * (d + 3) / 2 : d; }

hipError_t mcmc_launch_zv(int order, const double* x, const double* g, int64_t n, int d, int64_t C, double* zv,
                          double* coef, int32_t* info, hipStream_t st) {
    using namespace mcmc;
    if (d < 1 || d > mcmc_zv_max_d(order)) return hipErrorInvalidValue;
    ZvArgs a{x, g, n, C, d, (int)mcmc_zv_k(order, d), zv, coef, info};
    if (order == 1) return d <= 16 ? zv_launch<ZvLinear, 1, 1>(a, st) : zv_launch<ZvLinear, 2, 2>(a, st);
    if (a.k <= 16) return zv_launch<ZvQuadratic, 1, 1>(a, st);
    if (a.k <= 32) return zv_launch<ZvQuadratic, 2, 1>(a, st);
    return zv_launch<ZvQuadratic, 3, 1>(a, st);
}
