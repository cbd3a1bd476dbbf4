// smm_device.hpp -- the device pieces the manifold samplers share (smmala.hip, pmala.hip, rmhmc.hip, lmc.hip): the LDS carve-up of a
// workgroup of four 16-chain tiles, the pass over the observation tiles that forms the log-target, the gradient and the
// metric tensor on fp64 MFMA (smm_tiles, smm_evalallt), and the small SPD algebra in the chain's four lanes (Cholesky
// factor, inverse, solve, matvec, quadratic form) with its load / store helpers, and the second pass over the tiles with
// the weight's derivative (smm_dw_tiles, smm_pass: PMALA's drift correction pm_corr, RMHMC's two tensor terms, the
// Lagrangian samplers' weighted Gram matrix).  On top of them the two frames the step kernels share: the MALA step body
// (smm_mala_step: smm_step, pm_step) and the trajectory samplers' tuner registers, leapfrog count and mask (RmTuner,
// rm_leaps, rm_take: rm_step, lmc_step), both closed by smm_commit, and the launch of a kernel of the family
// (smm_launch).  The arithmetic of every piece is stated in smmala.hip's and pmala.hip's headers and DESIGN.md §4;
// tests/smmala_oracle.c and its successors restate every sum in the same order.
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

// X' diag(weights) X of one staged tile added to the tile's sixteen accumulators T (chain c: rows q + 4r, column cl):
// the weights of (observation q + 4r, chain cl) in vb[64 r + lane]; per k-slice, chain c: A = X[obs 4kk + q][cl],
// B = v_c[obs 4kk + q] X[obs 4kk + q][cl]
__device__ __forceinline__ void smm_gram_mfma(const double* LX, const SmLds& S, const GlmPos& p, f64x4 (&T)[16]) {
    typedef double f64x2_t __attribute__((ext_vector_type(2)));
    constexpr int SR = glm_row_stride(16);
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
        smm_gram_mfma(LX, S, p, T);
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
// rows 4q + e of L z, L the lower factor in W, z in the tile's shared vector V (Vc = V + cl): an fma chain over c <= r
// from zero; zero past d
__device__ __forceinline__ void smm_lower_mul(const double* Wc, const double* Vc, int d, int q, double (&out)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = 4 * q + e;
        double t = 0.0;
        if (r < d)
            for (int c = 0; c <= r; ++c) t = __builtin_fma(Wc[16 * smm_tri(r, c)], Vc[16 * c], t);
        out[e] = t;
    }
}
// (L L')^-1 from the factor L in W -> HBM (chain pointer out, stride ld) and from there into W: the lanes that form
// its columns hand it to the chain's other lanes through HBM.  The caller syncs the wave before it reads W.
__device__ __forceinline__ void smm_invert(double* Wc, double* Yl, int d, int nr, int q, double* out, size_t ld,
                                           bool live) {
    smm_inverse(Wc, Yl, d, q, out, ld, live);
    smm_mem_sync();
    smm_load_w(Wc, out, ld, nr, q, 1.0);
}
// the chain's SPD matrix in W factored (smm_chol's return) and inverted (smm_invert)
__device__ __forceinline__ double smm_factor_invert(double* Wc, double* Yl, int d, int nr, int q, double* out,
                                                    size_t ld, bool live) {
    const double ldet = smm_chol(Wc, d, q);
    smm_invert(Wc, Yl, d, nr, q, out, ld, live);
    return ldet;
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

// ------------------------------------------------------------------ the tensor's derivatives (pmala.hip, rmhmc.hip)
__device__ __forceinline__ double pm_probit_dw(double eta) {
    const double la = det_normlogcdf(eta), lb = det_normlogcdf(-eta);
    const double e2 = eta * eta;
    const double A = (-(e2 + kLog2Pi)) / 2.0;
    const double v01 = det_exp((((-e2) - 2.0 * la) - lb) - kLog2Pi);
    return v01 * (det_exp(A - lb) - 2.0 * (det_exp(A) + eta * det_exp(la)));
}

// w = dv / d eta (pmala.hip's header).  y: the tile's response column (probit: unused; logistic: wt = s (2y - 1))
template <bool LOGI>
__device__ __forceinline__ double pm_dw(double eta, double y, const double (*sptab)[10]) {
    if (LOGI) {
        double term, rv;
        det_logi(eta, y, term, rv, sptab);
        const double sig = __builtin_fabs(rv);
        const double v = sig * (1.0 - sig);
        return (v * (1.0 - 2.0 * sig)) * (-y);
    }
    return pm_probit_dw(eta);
}

// first tile and the logistic term's table into LDS; every wave of the workgroup (two barriers)
template <bool LOGI>
__device__ __forceinline__ void pm_stage_first(const GlmArgs& a, const SmLds& S) {
    constexpr int kHalf = kSmXS / 2;
    const int ti = threadIdx.x < kHalf ? (int)threadIdx.x : 0;
    __syncthreads();                                          // the previous pass's last tile has been read
    {
        const f64x2 v = reinterpret_cast<const f64x2*>(a.m.X)[ti];
        if (threadIdx.x < kHalf) reinterpret_cast<f64x2*>(S.X)[ti] = v;
    }
    if (LOGI) {
        for (int i = threadIdx.x; i < SP_NROWS * 10; i += 256) S.sp[i] = (&kSoftplusTab[0][0])[i];
    }
    __syncthreads();
}

// The second pass over the staged X tiles at the lane's coordinates x, with the weight's derivative w:
//   QF: U  = X' (w o qf), qf_o = x_o' invG x_o, the chains' invG in the workspace S.W (pmala.hip's header: the sum over
//       the slabs of dG_i invG[:, i], and trace(invG dG_r) in row r);
//   T2: U2 = X' (w o t^2), t = X v by eta's MFMA chain with the lane's coordinates of v as the B operand (k-slice e, row
//       q <-> coordinate 4q + e; v zero past d), the weight RN(w_o RN(t_o t_o)) (zero on padded observations), then the
//       gradient's MFMA: an fma chain over the observations in ascending order from zero; row r is v' dG_r v.
// Both read the same eta and w.  Returns at the lane's own coordinates.  Every wave of the workgroup calls it (barriers
// inside; their number depends on the tile count alone).
//   GR: T += X' diag(w o t) X of the tile's sixteen chains, the tensor pass's accumulators and MFMA path
//       (smm_gram_mfma) with the weight RN(w_o t_o) (zero on padded observations): lmc.hip's K(v), 2 vxC(v).  Not
//       with QF: both use the wave's weight rows.
template <bool LOGI, bool QF, bool T2, bool GR>
__device__ __forceinline__ void smm_dw_tiles(const GlmArgs& a, const GlmPos& p, const SmLds& S, const double (&x)[4],
                                             const double (&v)[4], f64x4& U, f64x4& U2, f64x4 (&T)[16]) {
    static_assert(!(QF && GR), "QF and GR share the wave's weight rows");
    const ModelArgs& M = a.m;
    constexpr int SR = glm_row_stride(16);
    constexpr int YO = glm_y_offset(16);
    constexpr int kHalf = kSmXS / 2;
    const int64_t ntiles = a.g.n_pad / 16;
    const int d = a.s.d;
    const int ti = threadIdx.x < kHalf ? (int)threadIdx.x : 0;
    const bool tl = threadIdx.x < kHalf;
    const double (*sptab)[10] = reinterpret_cast<const double (*)[10]>(S.sp);
    // the A operands of M = invG_c X': invG_c[cl][4q + e], for the whole pass
    double IA[16][4];
    if (QF) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = 4 * p.q + e;
            const bool ok = p.cl < d && k < d;
            const f64x2* row = reinterpret_cast<const f64x2*>(S.W + 16 * (ok ? smm_symi(p.cl, k) : 0));
#pragma unroll
            for (int c2 = 0; c2 < 8; ++c2) {
                const f64x2 v2 = row[c2];
                IA[2 * c2][e] = ok ? v2.x : 0.0;
                IA[2 * c2 + 1][e] = ok ? v2.y : 0.0;
            }
        }
    }
    pm_stage_first<LOGI>(a, S);
    U = f64x4{0.0, 0.0, 0.0, 0.0};
    U2 = f64x4{0.0, 0.0, 0.0, 0.0};
    if (GR) {
#pragma unroll
        for (int c = 0; c < 16; ++c) T[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    for (int64_t t = 0; t < ntiles; ++t) {
        const int b = (int)(t & 1);
        const double* LX = S.X + b * kSmXS;
        const bool more = t + 1 < ntiles;
        f64x2 nxt = f64x2{0.0, 0.0};
        if (more) nxt = reinterpret_cast<const f64x2*>(M.X + (size_t)(t + 1) * kSmXS)[ti];
        const double* xrow = LX + p.cl * SR + 4 * p.q;
        f64x4 eta = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int slot = 0; slot < 4; ++slot)
            eta = __builtin_amdgcn_mfma_f64_16x16x4f64(xrow[slot], x[slot], eta, 0, 0, 0);
        double w[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = p.q + 4 * r;
            const double wr = pm_dw<LOGI>(eta[r], LX[YO + o], sptab);
            w[r] = t * 16 + o < M.n ? wr : 0.0;
        }
        const double* gcol = LX + p.q * SR + 4 * (p.cl & 3) + (p.cl >> 2);
        f64x4 tt = f64x4{0.0, 0.0, 0.0, 0.0};
        if (T2 || GR) {
#pragma unroll
            for (int slot = 0; slot < 4; ++slot)
                tt = __builtin_amdgcn_mfma_f64_16x16x4f64(xrow[slot], v[slot], tt, 0, 0, 0);
        }
        if (GR) {
#pragma unroll
            for (int r = 0; r < 4; ++r) S.vb[64 * r + p.lane] = w[r] * tt[r];
            smm_wave_sync();
            smm_gram_mfma(LX, S, p, T);
        }
        if (T2) {
            double wt[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) wt[r] = w[r] * (tt[r] * tt[r]);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                U2 = __builtin_amdgcn_mfma_f64_16x16x4f64(gcol[4 * kk * SR], wt[kk], U2, 0, 0, 0);
        }
        if (QF) {
            // qf of (observation cl, chain c) -> vb[16 cl + c]
            double xo[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) xo[r] = LX[p.cl * SR + p.q + 4 * r];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                f64x4 Mq = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int e = 0; e < 4; ++e) Mq = __builtin_amdgcn_mfma_f64_16x16x4f64(IA[c][e], xrow[e], Mq, 0, 0, 0);
                const double sq = ((Mq[0] * xo[0] + Mq[1] * xo[1]) + Mq[2] * xo[2]) + Mq[3] * xo[3];
                const f64x4 Q = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, sq, f64x4{0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
                if ((c & 3) == p.q) S.vb[16 * p.cl + c] = Q[0];
            }
            smm_wave_sync();
            double wq[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) wq[r] = w[r] * S.vb[16 * (p.q + 4 * r) + p.cl];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                U = __builtin_amdgcn_mfma_f64_16x16x4f64(gcol[4 * kk * SR], wq[kk], U, 0, 0, 0);
        }
        smm_wave_sync();
        if (more && tl) reinterpret_cast<f64x2*>(S.X + (b ^ 1) * kSmXS)[ti] = nxt;
        __syncthreads();
    }
}

// the tile's sixteen accumulators -> the workspace S.W (lower triangles), as smm_evalallt lays the tensor out
__device__ __forceinline__ void smm_put_tiles(const GlmPos& p, const SmLds& S, int d, const f64x4 (&T)[16]) {
#pragma unroll
    for (int c = 0; c < 16; ++c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ar = p.q + 4 * r;
            if (ar < d && p.cl <= ar) S.W[16 * smm_tri(ar, p.cl) + c] = T[c][r];
        }
    }
    smm_wave_sync();
}

// The second pass (smm_dw_tiles) at x for the model's link, at the lane's own coordinates: QF the trace term
// u = X' (w o qf) from invG in W; T2 u2 = X' (w o t^2), t = X v; GR the raw weighted Gram matrices K(v) of the tile's
// chains -> W (lower triangles).  Every wave of the workgroup calls it.
template <bool QF, bool T2, bool GR>
__device__ __forceinline__ void smm_pass(const GlmArgs& a, const GlmPos& p, const SmLds& S, const double (&x)[4],
                                         const double (&v)[4], double (&u)[4], double (&u2)[4]) {
    f64x4 U, U2;
    f64x4 T[16];
    if (a.m.kind == MK_LOGISTIC) smm_dw_tiles<true, QF, T2, GR>(a, p, S, x, v, U, U2, T);
    else smm_dw_tiles<false, QF, T2, GR>(a, p, S, x, v, U, U2, T);
    if (GR) smm_put_tiles(p, S, a.s.d, T);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        u[e] = U[e];
        u2[e] = U2[e];
    }
}

// (L L') \ b from the factor L in W: b in the tile's shared vector B [16 coords][16 chains] (Bc = B + cl); every lane
// of the chain runs the whole substitution in its private LDS vector Yl (smm_inverse's chains with b for the unit
// column: forward y[i] = (b[i] then fma(-L[i][k], y[k], .) over k = 0..i-1) / L[i][i]; backward from i = d-1:
// x[i] = (y[i] then fma(-L[k][i], x[k], .) over k = i+1..d-1) / L[i][i]) and keeps its own coordinates.  B must not
// overlap the lanes' private vectors.
__device__ __forceinline__ void smm_solve(const double* Wc, const double* Bc, double* Yl, int d, int q,
                                          double (&out)[4]) {
    for (int i = 0; i < d; ++i) {
        double t = Bc[16 * i];
        for (int k = 0; k < i; ++k) t = __builtin_fma(-Wc[16 * smm_tri(i, k)], Yl[64 * k], t);
        Yl[64 * i] = t / Wc[16 * smm_tri(i, i)];
    }
    for (int i = d - 1; i >= 0; --i) {
        double t = Yl[64 * i];
        for (int k = i + 1; k < d; ++k) t = __builtin_fma(-Wc[16 * smm_tri(k, i)], Yl[64 * k], t);
        Yl[64 * i] = t / Wc[16 * smm_tri(i, i)];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = 4 * q + e < d ? Yl[64 * (4 * q + e)] : 0.0;
}

// out = M in, M the chain's symmetric packed matrix in W, through the tile's shared vector V
__device__ __forceinline__ void rm_symv(const GlmPos& p, const double* Wc, double* V, int d, const double (&in)[4],
                                        double (&out)[4]) {
    smm_put_vec(V, p, in);
    smm_wave_sync();
    smm_symv(Wc, V + p.cl, d, p.q, out);
    smm_wave_sync();
}

// c = invG (X' (w o qf)) at x, invG in S.W; V: one of the tile's shared vectors.  Every wave of the workgroup calls it.
__device__ __forceinline__ void pm_corr(const GlmArgs& a, const GlmPos& p, const SmLds& S, const double (&x)[4],
                                        double* V, double (&cv)[4]) {
    double u[4], u2[4];
    smm_pass<true, false, false>(a, p, S, x, x, u, u2);
    rm_symv(p, S.W + p.cl, V, a.s.d, u, cv);
}

// any of the lane's four values not finite, over the chain's four lanes
__device__ __forceinline__ bool smm_not_finite(const double (&u)[4]) {
    int nf = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) nf |= !(u[e] - u[e] == 0.0);
    nf |= __shfl_xor(nf, 16, 64);
    nf |= __shfl_xor(nf, 32, 64);
    return nf != 0;
}

// A step's end: the accepted proposal (x, g) becomes the state; step i's kept sample (on reject the state, read back
// into x and g) and its accept bit
__device__ __forceinline__ void smm_commit(const GlmArgs& a, const GlmPos& p, int64_t i, bool acc, double (&x)[4],
                                           f64x4 (&g)[1]) {
    const StepArgs& s = a.s;
    if (acc) {
        glm_store<1>(a, p, a.st.x, s.ld, x);
        glm_store4<1>(a, p, a.st.g, s.ld, g);
    }
    int64_t kk;
    if (kept_index(i - s.run_step0, s.burnin, s.thinning, s.len, &kk)) {
        if (!acc) {
            glm_load<1>(a, p, a.st.x, x);
            glm_load4<1>(a, p, a.st.g, g);
        }
        glm_store_kept<1>(a, p, kk, s.samples, x);
        glm_store_kept4<1>(a, p, kk, s.grads, g);
        glm_store_bit(a, p, kk, acc);
    }
}

// ------------------------------------------------------------------ the MALA pair (smmala.hip, pmala.hip)
// SMMALA.jl:72-122 and, with CORR (the drift correction c), PMALA.jl:85-140: one step per loop pass; the state (pars,
// logTarget, grad, G, invG, firstTerm and PMALA's c) lives in HBM.  smem: the workgroup's dynamic LDS.
template <bool CORR>
__device__ __forceinline__ void smm_mala_step(const GlmArgs& a, double* smem) {
    const StepArgs& s = a.s;
    const SamplerArgs& sa = a.sa;
    const GlmPos p = glm_pos(a);
    const SmLds S = smm_lds(smem, p.wave);
    const GlmLds none{};
    const Stream rs{s.key0, s.key1};
    const uint32_t chain = s.chain0 + (uint32_t)p.c;
    const int64_t cc = p.live ? p.c : 0;
    const int d = s.d, nr = d * (d + 1) / 2;
    const size_t ld = (size_t)s.ld;
    double* const Wc = S.W + p.cl;
    double* const V0 = S.Y;
    double* const V1 = S.Y + 256;
    double* const Gc = a.st.sm_G + cc;
    double* const iGc = a.st.sm_invG + cc;
    double* const pGc = a.st.sm_pG + cc;
    double* const piGc = a.st.sm_pinvG + cc;
    double lp = a.st.lp[cc];
    double h = sa.tuner ? a.st.t_step[cc] : sa.drift_step;
    int32_t n_acc = sa.tuner ? a.st.t_acc[cc] : 0;
    int32_t n_prop = sa.tuner ? a.st.t_prop[cc] : 0;
    for (int t = 0; t < s.nsteps; ++t) {
        const int64_t i = s.step_begin + t;
        if (sa.tuner) n_prop += 1;
        const double half = h / 2.0;
        double xp[4], ev[4];
        // U = chol(h invG): its transpose, the lower factor, in W
        smm_load_w(Wc, iGc, ld, nr, p.q, h);
        smm_wave_sync();
        const double ld1 = smm_chol(Wc, d, p.q);
        bool bad = !(ld1 == ld1);
        {
            double z[4], x[4], ft[4], cv[4], u[4];
            glm_normals<1>(p, rs, chain, (uint32_t)i, d, z);
            glm_load<1>(a, p, a.st.x, x);
            glm_load<1>(a, p, a.st.sm_ft, ft);
            if (CORR) glm_load<1>(a, p, a.st.pm_c, cv);
            smm_put_vec(V0, p, z);
            smm_wave_sync();
            smm_lower_mul(Wc, V0 + p.cl, d, p.q, u);                    // U' z
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = 4 * p.q + e < d;
                const double pm = x[e] + half * (CORR ? ft[e] - cv[e] : ft[e]);   // SMMALA.jl:85, PMALA.jl:94
                xp[e] = in ? pm + u[e] : 0.0;                           // SMMALA.jl:88, PMALA.jl:98
                ev[e] = in ? pm - xp[e] : 0.0;
            }
        }
        smm_put_vec(V1, p, ev);
        smm_wave_sync();
        // probNewGivenOld = -sum(log(diag(U))) - 0.5 e' (G / h) e     SMMALA.jl:93-94, PMALA.jl:103-104
        const double quad1 = glm_sum(a, p, none, smm_quad(Gc, ld, V1 + p.cl, d, p.q, h, ev));
        const double qf = (-ld1) - 0.5 * quad1;
        smm_wave_sync();
        bool oos;
        f64x4 gp[1];
        const double lpp = smm_evalallt(a, p, S, xp, gp, oos);         // SMMALA.jl:90, PMALA.jl:101
        smm_store_w(Wc, pGc, ld, nr, p.q, p.live);
        // proposedG = L L', proposedInvG   SMMALA.jl:97, PMALA.jl:106
        const double ldg = smm_factor_invert(Wc, S.Y + p.lane, d, nr, p.q, piGc, ld, p.live);
        bad = bad || !(ldg == ldg);
        double pft[4], pc[4];
        {
            const double gv[4] = {gp[0][0], gp[0][1], gp[0][2], gp[0][3]};
            rm_symv(p, Wc, V0, d, gv, pft);                            // proposedFirstTerm   SMMALA.jl:98, PMALA.jl:107
        }
        if (CORR) pm_corr(a, p, S, xp, V0, pc);                        // sum(proposedSecondTerm, 2)   PMALA.jl:108-111
        for (int idx = p.q; idx < nr; idx += 4) Wc[16 * idx] = h * Wc[16 * idx];
        smm_wave_sync();
        const double ld2 = smm_chol(Wc, d, p.q);                       // chol(h proposedInvG)
        bad = bad || !(ld2 == ld2);
        {
            double x[4];
            glm_load<1>(a, p, a.st.x, x);
#pragma unroll
            for (int e = 0; e < 4; ++e)   // SMMALA.jl:99-101, PMALA.jl:114, 117
                ev[e] = 4 * p.q + e < d ? (xp[e] + half * (CORR ? pft[e] - pc[e] : pft[e])) - x[e] : 0.0;
        }
        smm_put_vec(V1, p, ev);
        smm_wave_sync();
        const double quad2 = glm_sum(a, p, none, smm_quad(pGc, ld, V1 + p.cl, d, p.q, h, ev));
        const double qb = (-ld2) - 0.5 * quad2;                        // probOldGivenNew
        const double ratio = ((lpp + qb) - lp) - qf;                   // SMMALA.jl:104, PMALA.jl:119
        // a proposal out of support or with a failed pivot is rejected (the reference throws out of chol)
        const bool acc = !(bad || oos) && glm_mh_short_circuit(rs, chain, (uint32_t)i, ratio);
        if (acc) {
            glm_store<1>(a, p, a.st.sm_ft, s.ld, pft);
            if (CORR) glm_store<1>(a, p, a.st.pm_c, s.ld, pc);
            if (p.live)
                for (int idx = p.q; idx < nr; idx += 4) {
                    Gc[(size_t)idx * ld] = pGc[(size_t)idx * ld];
                    iGc[(size_t)idx * ld] = piGc[(size_t)idx * ld];
                }
            lp = lpp;
            if (sa.tuner) n_acc += 1;
        }
        smm_commit(a, p, i, acc, xp, gp);
        // SMMALA.jl:113-119, PMALA.jl:131-137 (EmpiricalMALATune)
        if (sa.tuner && i <= s.tuner_burnin && (i % sa.adapt_step) == 0) {
            h = h * glm_tune_factor(n_acc, n_prop, sa.target_rate);
            n_acc = 0;
            n_prop = 0;
        }
        smm_mem_sync();                                                // the state the next step's lanes read
    }
    if (p.live && p.q == 0) {
        a.st.lp[p.c] = lp;
        if (sa.tuner) {
            a.st.t_step[p.c] = h;
            a.st.t_acc[p.c] = n_acc;
            a.st.t_prop[p.c] = n_prop;
        }
    }
}

// ------------------------------------------------------------------ the trajectory samplers (rmhmc.hip, lmc.hip)
// smm_device.hpp's carve-up, then the leapfrog count's maximum
constexpr int kRmLdsDoubles = kSmLdsDoubles + 2;

// workgroup-wide max of the live chains' leapfrog counts (0 when none is live): every wave must reach it
__device__ __forceinline__ int rm_max(int* iscr, int v, bool live) {
    __syncthreads();
    if (threadIdx.x == 0) iscr[0] = 0;
    __syncthreads();
    if (live) atomicMax(&iscr[0], v);
    __syncthreads();
    const int r = iscr[0];
    __syncthreads();
    return r;
}

// nRandomLeaps = ceil(uniform52(w0, w1) nLeaps) of the step's block w, and in nl_wg the workgroup's longest trajectory
// (rm_max: every wave must reach it)
__device__ __forceinline__ int rm_leaps(int* iscr, const u32x4& w, int64_t nl_fixed, bool live, int& nl_wg) {
    const int nrl = (int)__builtin_ceil(uniform52(w.x, w.y) * (double)nl_fixed);
    nl_wg = rm_max(iscr, nrl, live);
    return nrl;
}

// A masked update of a trajectory: a chain that has finished (!on) or has failed (dead) keeps still, and a bad value
// kills the trajectory.  Returns whether the chain takes the update.  Never around a pass over X.
__device__ __forceinline__ bool rm_take(bool on, bool& dead, bool bad) {
    if (!on || dead) return false;
    dead = bad;
    return !bad;
}

// the lane's partial of a' b over its coordinates
__device__ __forceinline__ double rm_dot_part(const GlmPos& p, int d, const double (&u)[4], const double (&v)[4]) {
    double part = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (4 * p.q + e < d) part = __builtin_fma(u[e], v[e], part);
    return part;
}

// The chain's EmpiricalHMCTune registers: leapStep, nLeaps and the window's counts (without a tuner the sampler's
// constants, and the counts stay 0)
struct RmTuner {
    double eps;
    int64_t nl_fixed;
    int32_t n_acc, n_prop;
};
__device__ __forceinline__ RmTuner rm_tuner_load(const GlmArgs& a, int64_t cc) {
    const SamplerArgs& sa = a.sa;
    const bool tuned = sa.tuner != 0;
    RmTuner T;
    T.eps = tuned ? a.st.t_step[cc] : sa.leap_step;
    T.nl_fixed = tuned ? (int64_t)a.st.t_leaps[cc] : sa.n_leaps;
    T.n_acc = tuned ? a.st.t_acc[cc] : 0;
    T.n_prop = tuned ? a.st.t_prop[cc] : 0;
    return T;
}
// the window's end at step i: leapStep by the window's rate, nLeaps = ceil(targetPath / leapStep) under its two caps
__device__ __forceinline__ void rm_tuner_adapt(const GlmArgs& a, int64_t i, RmTuner& T) {
    const SamplerArgs& sa = a.sa;
    if (sa.tuner && i <= a.s.tuner_burnin && (i % sa.adapt_step) == 0) {
        T.eps = T.eps * glm_tune_factor(T.n_acc, T.n_prop, sa.target_rate);
        double nlf = __builtin_ceil(sa.target_path / T.eps);
        if (nlf > (double)sa.max_step) nlf = (double)sa.max_step;
        if (nlf > (double)sa.max_leaps) nlf = (double)sa.max_leaps;
        T.nl_fixed = (int64_t)nlf;
        T.n_acc = 0;
        T.n_prop = 0;
    }
}
// the launch's end: the chain's log-target and tuner registers -> the state (the chain's lane q = 0)
__device__ __forceinline__ void rm_write_back(const GlmArgs& a, const GlmPos& p, double lp, const RmTuner& T) {
    if (p.live && p.q == 0) {
        a.st.lp[p.c] = lp;
        if (a.sa.tuner) {
            a.st.t_step[p.c] = T.eps;
            a.st.t_leaps[p.c] = (int32_t)T.nl_fixed;
            a.st.t_acc[p.c] = T.n_acc;
            a.st.t_prop[p.c] = T.n_prop;
        }
    }
}

// One launch of a kernel of the family: glm_grid workgroups of 256 threads with lds_doubles of dynamic LDS.  note: the
// step kernel's name for mcmc_note_step_kernel, or NULL.  rest: the kernel's arguments after GlmArgs.
template <typename... P, typename... A>
static hipError_t smm_launch(void (*kern)(GlmArgs, P...), const char* note, int lds_doubles, const KernelArgs& k,
                             hipStream_t st, A... rest) {
    const GlmShape gs = mcmc_glm_shape(k.s.d, k.m.n);
    const GlmArgs a = glm_args(k, gs);
    const size_t lds = (size_t)lds_doubles * sizeof(double);
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (note) mcmc_note_step_kernel("%s", note);
    kern<<<dim3(glm_grid(k.s.C, gs)), 256, lds, st>>>(a, rest...);
    return hipGetLastError();
}

}  // namespace mcmc
