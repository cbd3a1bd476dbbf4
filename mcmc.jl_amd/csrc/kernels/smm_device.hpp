// smm_device.hpp -- the device pieces the manifold samplers share (smmala.hip, pmala.hip): the LDS carve-up of a
// workgroup of four 16-chain tiles, the pass over the observation tiles that forms the log-target, the gradient and the
// metric tensor on fp64 MFMA (smm_tiles, smm_evalallt), and the small SPD algebra in the chain's four lanes (Cholesky
// factor, inverse, matvec, quadratic form) with its load / store helpers.  The arithmetic of every piece is stated in
// smmala.hip's header and DESIGN.md §4; tests/smmala_oracle.c restates every sum in the same order.
#pragma once
#include "glm_device.hpp"

namespace mcmc {

constexpr int kSmMaxD = 16;
constexpr int kSmXS = glm_tile_doubles(16);                // one staged tile
constexpr int kSmW = (kSmMaxD * (kSmMaxD + 1) / 2) * 16;   // a tile's packed matrices [136][16 chains]
constexpr int kSmY = 16 * 64;                              // a lane's private vector [16][64 lanes]; also the tile's
                                                           // shared vectors V0, V1 [16 coords][16 chains]
constexpr int kSmWork = kSmW + kSmY;
// LDS (doubles): X tiles [2][XS] | the logistic term's table | weights v [4 waves][4 r][64 lanes] | work [4 waves]
constexpr int kSmLdsDoubles = 2 * kSmXS + SP_NROWS * 10 + 4 * 256 + 4 * kSmWork;
static_assert((2 * kSmXS + SP_NROWS * 10) % 2 == 0, "the weights are read as 16-byte pairs");

struct SmLds {
    double* X;
    double* sp;
    double* vb;      // this wave's weights
    double* W;       // this wave's matrix workspace
    double* Y;       // this wave's vector workspace
};

__device__ __forceinline__ SmLds smm_lds(double* smem, int wave) {
    SmLds S;
    S.X = smem;
    S.sp = smem + 2 * kSmXS;
    S.vb = S.sp + SP_NROWS * 10 + wave * 256;
    S.W = S.sp + SP_NROWS * 10 + 4 * 256 + wave * kSmWork;
    S.Y = S.W + kSmW;
    return S;
}

// LDS handed between the lanes of one wave: the wave's LDS operations execute in order, so only the compiler has to
// keep them in order
__device__ __forceinline__ void smm_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// HBM handed between the lanes of one wave (the proposal's G and inverse, the state on accept)
__device__ __forceinline__ void smm_mem_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int smm_tri(int r, int c) { return ((r * (r + 1)) >> 1) + c; }
__device__ __forceinline__ int smm_symi(int r, int c) { return r >= c ? smm_tri(r, c) : smm_tri(c, r); }

// The probit model's term and gradient weight (glm_probit_obs, the same operations) and the example's tensor weight
// exp(-eta^2 - logcdf(eta) - logcdf(-eta) - log 2 pi) (examples/probit_regression.jl:44-49)
__device__ __forceinline__ void smm_probit_obs(double eta, double y, double& term, double& w, double& v) {
    const double la = det_normlogcdf(eta), lb = det_normlogcdf(-eta);
    term = y * la + (1.0 - y) * lb;
    const double A = (-(eta * eta + kLog2Pi)) / 2.0;
    w = y * det_exp(A - la) - (1.0 - y) * det_exp(A - lb);
    v = det_exp(((-(eta * eta) - la) - lb) - kLog2Pi);
}

// One pass over the observation tiles: the likelihood partial of the lane, the gradient accumulator G (own
// coordinates) and the tile's sixteen tensor accumulators T.  Every wave of the workgroup calls it (barriers inside).
template <bool LOGI>
__device__ __forceinline__ double smm_tiles(const GlmArgs& a, const GlmPos& p, const SmLds& S, const double (&x)[4],
                                            f64x4& G, f64x4 (&T)[16]) {
    typedef double f64x2_t __attribute__((ext_vector_type(2)));
    const ModelArgs& M = a.m;
    constexpr int SR = glm_row_stride(16);
    constexpr int YO = glm_y_offset(16);
    constexpr int BO = glm_b_offset(16);
    constexpr int kHalf = kSmXS / 2;
    const int64_t ntiles = a.g.n_pad / 16;
    const int64_t nfull = M.n / 16;
    const int ti = threadIdx.x < kHalf ? (int)threadIdx.x : 0;
    const bool tl = threadIdx.x < kHalf;
    __syncthreads();                                          // the previous evaluation's last tile has been read
    {
        const f64x2_t v = reinterpret_cast<const f64x2_t*>(M.X)[ti];
        if (tl) reinterpret_cast<f64x2_t*>(S.X)[ti] = v;
    }
    const double (*sptab)[10] = reinterpret_cast<const double (*)[10]>(S.sp);
    if (LOGI) {
        for (int i = threadIdx.x; i < SP_NROWS * 10; i += 256) S.sp[i] = (&kSoftplusTab[0][0])[i];
    }
    G = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 16; ++c) T[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    __syncthreads();
    double lik_part = 0.0;
    double ubnd = -__builtin_inf();
    for (int64_t t = 0; t < ntiles; ++t) {
        const int b = (int)(t & 1);
        const double* LX = S.X + b * kSmXS;
        const bool more = t + 1 < ntiles;
        f64x2_t nxt = f64x2_t{0.0, 0.0};
        if (more) nxt = reinterpret_cast<const f64x2_t*>(M.X + (size_t)(t + 1) * kSmXS)[ti];
        // eta: k-slice e, row q <-> coordinate 4q + e
        f64x4 eta = f64x4{0.0, 0.0, 0.0, 0.0};
        {
            const double* xrow = LX + p.cl * SR + 4 * p.q;
#pragma unroll
            for (int slot = 0; slot < 4; ++slot)
                eta = __builtin_amdgcn_mfma_f64_16x16x4f64(xrow[slot], x[slot], eta, 0, 0, 0);
        }
        double term[4], rv[4], vv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double y = LX[YO + p.q + 4 * r];
            if (LOGI) {
                // the expected Fisher information weight p (1 - p) from the sigmoid |rv| of det_logi (either link sign)
                LogiState E;
                det_logi_s1(eta[r], y, E, sptab);
                ubnd = __builtin_fmax(ubnd, E.u + LX[BO + p.q + 4 * r]);
                det_logi_s2(E);
                det_logi_fin(E, y, term[r], rv[r]);
                const double sig = __builtin_fabs(rv[r]);
                vv[r] = sig * (1.0 - sig);
            } else {
                smm_probit_obs(eta[r], y, term[r], rv[r], vv[r]);
            }
        }
        if (t < nfull) {
#pragma unroll
            for (int r = 0; r < 4; ++r) lik_part = lik_part + term[r];
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool in = t * 16 + p.q + 4 * r < M.n;
                lik_part = in ? lik_part + term[r] : lik_part;
                rv[r] = in ? rv[r] : 0.0;
                vv[r] = in ? vv[r] : 0.0;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) S.vb[64 * r + p.lane] = vv[r];
        // the gradient: tile row i = cl <-> coordinate 4 (cl & 3) + (cl >> 2), k-slice kk <-> observations 4kk + q
        {
            const double* gcol = LX + p.q * SR + 4 * (p.cl & 3) + (p.cl >> 2);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                G = __builtin_amdgcn_mfma_f64_16x16x4f64(gcol[4 * kk * SR], rv[kk], G, 0, 0, 0);
        }
        smm_wave_sync();
        // the tensor: per k-slice, chain c: A = X[obs 4kk + q][cl], B = v_c[obs 4kk + q] X[obs 4kk + q][cl]
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const double xa = LX[(4 * kk + p.q) * SR + p.cl];
            const f64x2_t* vrow = reinterpret_cast<const f64x2_t*>(S.vb + 64 * kk + 16 * p.q);
#pragma unroll
            for (int c2 = 0; c2 < 8; ++c2) {
                const f64x2_t v2 = vrow[c2];
                T[2 * c2] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, v2.x * xa, T[2 * c2], 0, 0, 0);
                T[2 * c2 + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, v2.y * xa, T[2 * c2 + 1], 0, 0, 0);
            }
        }
        smm_wave_sync();
        if (more && tl) reinterpret_cast<f64x2_t*>(S.X + (b ^ 1) * kSmXS)[ti] = nxt;
        __syncthreads();
    }
    return LOGI && ubnd >= 0.0 ? -__builtin_inf() : lik_part;
}

// evalallt at the lane's coordinates x: returns the log-target, the gradient in g (own coordinates) and the tile's
// tensors in the workspace S.W (lower triangles, the prior precision on the diagonal)
__device__ __forceinline__ double smm_evalallt(const GlmArgs& a, const GlmPos& p, const SmLds& S, const double (&x)[4],
                                               f64x4 (&g)[1], bool& oos) {
    f64x4 T[16];
    const double lik = a.m.kind == MK_LOGISTIC ? smm_tiles<true>(a, p, S, x, g[0], T)
                                               : smm_tiles<false>(a, p, S, x, g[0], T);
    const GlmLds none{};
    const double lp = glm_finish<1, 1, true>(a, p, none, XArr<4>{x}, g, lik, oos);
    const int d = a.s.d;
    const double sp = a.m.prior_sigma;
    const double ip = 1.0 / (sp * sp);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ar = p.q + 4 * r;
            if (ar < d && p.cl <= ar) S.W[16 * smm_tri(ar, p.cl) + c] = ar == p.cl ? T[c][r] + ip : T[c][r];
        }
    }
    smm_wave_sync();
    return lp;
}

// Cholesky factor of the chain's packed SPD matrix in W (Wc = W + cl), in place: column j's pivot is formed by all
// four lanes, s = A[j][j] then fma(-L[j][k], L[j][k], s) over k < j; row i > j by its owner,
// (A[i][j] then fma(-L[i][k], L[j][k], .) over k < j) / L[j][j].  Returns sum_j log L[j][j] (added in j order), or NaN
// when a pivot is <= 0 or not finite (that column then takes the pivot 1).
__device__ __forceinline__ double smm_chol(double* Wc, int d, int q) {
    double ld = 0.0;
    bool bad = false;
    for (int j = 0; j < d; ++j) {
        double s = Wc[16 * smm_tri(j, j)];
        for (int k = 0; k < j; ++k) {
            const double l = Wc[16 * smm_tri(j, k)];
            s = __builtin_fma(-l, l, s);
        }
        const bool ok = s > 0.0 && s < __builtin_inf();
        bad = bad || !ok;
        const double ljj = __builtin_sqrt(ok ? s : 1.0);
        ld = ld + det_log(ljj);
        smm_wave_sync();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = 4 * q + e;
            if (i > j && i < d) {
                double t = Wc[16 * smm_tri(i, j)];
                for (int k = 0; k < j; ++k) t = __builtin_fma(-Wc[16 * smm_tri(i, k)], Wc[16 * smm_tri(j, k)], t);
                Wc[16 * smm_tri(i, j)] = t / ljj;
            }
        }
        if (q == (j >> 2)) Wc[16 * smm_tri(j, j)] = ljj;
        smm_wave_sync();
    }
    return bad ? __builtin_nan("") : ld;
}

// The lower triangle of (L L')^-1 from the factor L in W: lane q forms columns j = 4q + e.  Forward: y[j] = 1 / L[j][j],
// y[i] = (0 then fma(-L[i][k], y[k], .) over k = j..i-1) / L[i][i]; backward from i = d-1 down to j:
// x[i] = (y[i] then fma(-L[k][i], x[k], .) over k = i+1..d-1) / L[i][i].  Element (i, j) -> out[tri(i, j) ld].
__device__ __forceinline__ void smm_inverse(const double* Wc, double* Yl, int d, int q, double* out, size_t ld,
                                            bool live) {
#pragma unroll 1
    for (int e = 0; e < 4; ++e) {
        const int j = 4 * q + e;
        if (j >= d) continue;
        for (int i = j; i < d; ++i) {
            double t = i == j ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) t = __builtin_fma(-Wc[16 * smm_tri(i, k)], Yl[64 * k], t);
            Yl[64 * i] = t / Wc[16 * smm_tri(i, i)];
        }
        for (int i = d - 1; i >= j; --i) {
            double t = Yl[64 * i];
            for (int k = i + 1; k < d; ++k) t = __builtin_fma(-Wc[16 * smm_tri(k, i)], Yl[64 * k], t);
            const double xi = t / Wc[16 * smm_tri(i, i)];
            Yl[64 * i] = xi;
            if (live) out[(size_t)smm_tri(i, j) * ld] = xi;
        }
    }
}

// the chain's packed matrix: HBM (chain pointer src, stride ld) -> W scaled by f, and W -> HBM; entries idx = q, q + 4, ...
__device__ __forceinline__ void smm_load_w(double* Wc, const double* src, size_t ld, int nr, int q, double f) {
    for (int idx = q; idx < nr; idx += 4) Wc[16 * idx] = f * src[(size_t)idx * ld];
}
__device__ __forceinline__ void smm_store_w(const double* Wc, double* dst, size_t ld, int nr, int q, bool live) {
    if (!live) return;
    for (int idx = q; idx < nr; idx += 4) dst[(size_t)idx * ld] = Wc[16 * idx];
}
// own coordinates of a vector -> the tile's shared vector V [16 coords][16 chains]
__device__ __forceinline__ void smm_put_vec(double* V, const GlmPos& p, const double (&v)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) V[16 * (4 * p.q + e) + p.cl] = v[e];
}
// rows 4q + e of (symmetric packed M in W) v: an fma chain over c = 0..d-1 from zero
__device__ __forceinline__ void smm_symv(const double* Wc, const double* Vc, int d, int q, double (&out)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = 4 * q + e;
        double t = 0.0;
        if (r < d)
            for (int c = 0; c < d; ++c) t = __builtin_fma(Wc[16 * smm_symi(r, c)], Vc[16 * c], t);
        out[e] = t;
    }
}
// the lane's partial of e' (M / h) e, M symmetric packed in HBM (chain pointer, stride ld): rows 4q + e in order,
// t = fma chain over c of (M[r][c] / h) e[c], then fma(e[r], t, partial)
__device__ __forceinline__ double smm_quad(const double* Mc, size_t ld, const double* Vc, int d, int q, double h,
                                           const double (&ev)[4]) {
    double part = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = 4 * q + e;
        if (r < d) {
            double t = 0.0;
            for (int c = 0; c < d; ++c) t = __builtin_fma(Mc[(size_t)smm_symi(r, c) * ld] / h, Vc[16 * c], t);
            part = __builtin_fma(ev[e], t, part);
        }
    }
    return part;
}

static hipError_t smm_lds_attr(const void* f) {
    return hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kSmLdsDoubles * sizeof(double)));
}

}  // namespace mcmc
