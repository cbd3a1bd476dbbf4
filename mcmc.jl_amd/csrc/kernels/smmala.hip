// smmala.hip -- the metric tensor of the probit / logistic regression models on fp64 MFMA (`evalallt`,
// likmodel.jl) and the simplified manifold MALA sampler on top of it (src/samplers/SMMALA.jl:39-123), d <= 16.
//
// Geometry: the regression family's single-slice one (glm_device.hpp, GlmShape with NM = 1): a wave owns a tile of 16
// chains, lane (q, cl) chain cl and coordinates 4q + e; four tiles a workgroup share the staged X tiles
// (glm_layout.hpp image).  The log-target and the gradient are glm_eval1's, operation for operation (eta chains over
// (e, q); the gradient chains over observations; a lane's likelihood terms in (t, r) order), so they are
// mcmc_model_eval's bit for bit.
//
// The tensor G(x) = X' diag(v(x)) X + I / prior_sigma^2 rides the same pass over the observation tiles: per chain c of
// the tile and per 4 observations one v_mfma_f64_16x16x4_f64 with A = X' (lane (q, cl): X[obs 4kk + q][coord cl], the
// same for every chain) and B = diag(v_c) X (lane (q, cl): v_c[obs 4kk + q] * X[obs 4kk + q][coord cl], the product
// rounded first).  The weights v of the tile cross from the lanes that formed them (lane (q, c): obs q + 4r of chain c)
// to the B operands through LDS.  The sixteen accumulators of a tile stay in registers (64 doubles a lane); lane (q, cl)
// register r of chain c is G_c[q + 4r][cl].  Element (a, b), b <= a, is therefore the fma chain over the observations
// i in ascending order, from zero, of fma(X[i][a], RN(v_i X[i][b]), .), the prior precision added to the diagonal last;
// the upper triangle is its mirror.
//
// The small algebra runs in the chain's four lanes on the tile's LDS workspace W [136 packed rows][16 chains]: the
// Cholesky factor in place (pivots formed by all four lanes, a column's rows by their owners 4q + e), the inverse
// column by column (lane q owns columns 4q + e: forward then backward substitution in a private LDS vector), the
// matvecs and quadratic forms by rows.  tests/smmala_oracle.c restates every sum in the same order.
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

// evalallt alone (mcmc_model_eval_tensor, the chains' first evaluation, mcmc_chains_set_state): lp, gradient [d][ld] and
// G packed [d(d+1)/2][ld]; with invG_out the inverse and firstTerm = invG grad too.  check: a start out of support or a
// failed pivot sets the error word.
__global__ __launch_bounds__(256) void smm_eval_kernel(GlmArgs a, const double* xin, double* lp_out, double* g_out,
                                                       double* G_out, double* invG_out, double* ft_out, int32_t check) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const GlmPos p = glm_pos(a);
    const SmLds S = smm_lds(smem, p.wave);
    const int d = a.s.d, nr = d * (d + 1) / 2;
    const size_t ld = (size_t)a.s.ld;
    const int64_t cc = p.live ? p.c : 0;
    double* const Wc = S.W + p.cl;
    double x[4];
    f64x4 g[1];
    glm_load<1>(a, p, xin, x);
    bool oos;
    const double lp = smm_evalallt(a, p, S, x, g, oos);
    if (p.live && p.q == 0 && lp_out) lp_out[p.c] = lp;
    if (g_out) glm_store4<1>(a, p, g_out, a.s.ld, g);
    bool fail = !(lp - lp == 0.0);
    if (G_out) smm_store_w(Wc, G_out + cc, ld, nr, p.q, p.live);
    if (invG_out) {
        const double ldet = smm_chol(Wc, d, p.q);
        fail = fail || !(ldet == ldet);
        smm_inverse(Wc, S.Y + p.lane, d, p.q, invG_out + cc, ld, p.live);
        smm_mem_sync();
        smm_load_w(Wc, invG_out + cc, ld, nr, p.q, 1.0);
        double gv[4] = {g[0][0], g[0][1], g[0][2], g[0][3]};
        smm_put_vec(S.Y, p, gv);
        smm_wave_sync();
        double ft[4];
        smm_symv(Wc, S.Y + p.cl, d, p.q, ft);
        glm_store<1>(a, p, ft_out, a.s.ld, ft);
    }
    if (check && p.live && fail) atomicOr(a.s.err, 1);
}

// SMMALA.jl:72-122, one step per loop pass; the state (pars, logTarget, grad, G, invG, firstTerm) lives in HBM
__global__ __launch_bounds__(256) void smm_step(GlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
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
            double z[4], x[4], ft[4];
            glm_normals<1>(p, rs, chain, (uint32_t)i, d, z);
            glm_load<1>(a, p, a.st.x, x);
            glm_load<1>(a, p, a.st.sm_ft, ft);
            smm_put_vec(V0, p, z);
            smm_wave_sync();
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * p.q + e;
                double u = 0.0;                                         // (U' z)[r]: fma chain over c <= r
                if (r < d)
                    for (int c = 0; c <= r; ++c) u = __builtin_fma(Wc[16 * smm_tri(r, c)], V0[16 * c + p.cl], u);
                const double pm = x[e] + half * ft[e];                  // SMMALA.jl:85
                xp[e] = r < d ? pm + u : 0.0;                           // SMMALA.jl:88
                ev[e] = r < d ? pm - xp[e] : 0.0;
            }
        }
        smm_put_vec(V1, p, ev);
        smm_wave_sync();
        // probNewGivenOld = -sum(log(diag(U))) - 0.5 e' (G / h) e     SMMALA.jl:93-94
        const double quad1 = glm_sum(a, p, none, smm_quad(Gc, ld, V1 + p.cl, d, p.q, h, ev));
        const double qf = (-ld1) - 0.5 * quad1;
        smm_wave_sync();
        bool oos;
        f64x4 gp[1];
        const double lpp = smm_evalallt(a, p, S, xp, gp, oos);         // SMMALA.jl:90
        smm_store_w(Wc, pGc, ld, nr, p.q, p.live);
        const double ldg = smm_chol(Wc, d, p.q);                       // proposedG = L L'
        bad = bad || !(ldg == ldg);
        smm_inverse(Wc, S.Y + p.lane, d, p.q, piGc, ld, p.live);      // proposedInvG   SMMALA.jl:97
        smm_mem_sync();
        smm_load_w(Wc, piGc, ld, nr, p.q, 1.0);
        double pft[4];
        {
            double gv[4] = {gp[0][0], gp[0][1], gp[0][2], gp[0][3]};
            smm_put_vec(V0, p, gv);
            smm_wave_sync();
            smm_symv(Wc, V0 + p.cl, d, p.q, pft);                      // proposedFirstTerm   SMMALA.jl:98
            smm_wave_sync();
        }
        for (int idx = p.q; idx < nr; idx += 4) Wc[16 * idx] = h * Wc[16 * idx];
        smm_wave_sync();
        const double ld2 = smm_chol(Wc, d, p.q);                       // chol(h proposedInvG)
        bad = bad || !(ld2 == ld2);
        {
            double x[4];
            glm_load<1>(a, p, a.st.x, x);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                ev[e] = 4 * p.q + e < d ? (xp[e] + half * pft[e]) - x[e] : 0.0;   // SMMALA.jl:99-101
        }
        smm_put_vec(V1, p, ev);
        smm_wave_sync();
        const double quad2 = glm_sum(a, p, none, smm_quad(pGc, ld, V1 + p.cl, d, p.q, h, ev));
        const double qb = (-ld2) - 0.5 * quad2;                        // probOldGivenNew
        const double ratio = ((lpp + qb) - lp) - qf;                   // SMMALA.jl:104
        // a proposal out of support or with a failed pivot is rejected (the reference throws out of chol)
        const bool acc = !(bad || oos) && glm_mh_short_circuit(rs, chain, (uint32_t)i, ratio);
        if (acc) {
            glm_store<1>(a, p, a.st.x, s.ld, xp);
            glm_store4<1>(a, p, a.st.g, s.ld, gp);
            glm_store<1>(a, p, a.st.sm_ft, s.ld, pft);
            if (p.live)
                for (int idx = p.q; idx < nr; idx += 4) {
                    Gc[(size_t)idx * ld] = pGc[(size_t)idx * ld];
                    iGc[(size_t)idx * ld] = piGc[(size_t)idx * ld];
                }
            lp = lpp;
            if (sa.tuner) n_acc += 1;
        }
        int64_t kk;
        if (kept_index(i - s.run_step0, s.burnin, s.thinning, s.len, &kk)) {
            if (!acc) {
                glm_load<1>(a, p, a.st.x, xp);
                glm_load4<1>(a, p, a.st.g, gp);
            }
            glm_store_kept<1>(a, p, kk, s.samples, xp);
            glm_store_kept4<1>(a, p, kk, s.grads, gp);
            glm_store_bit(a, p, kk, acc);
        }
        if (sa.tuner && i <= s.tuner_burnin && (i % sa.adapt_step) == 0) {   // SMMALA.jl:113-119 (EmpiricalMALATune)
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

static hipError_t smm_lds_attr(const void* f) {
    return hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kSmLdsDoubles * sizeof(double)));
}

}  // namespace mcmc

int mcmc_smmala_max_d() { return mcmc::kSmMaxD; }

hipError_t mcmc_launch_smmala_eval(const mcmc::KernelArgs& k, const double* xin, double* lp, double* g, double* G,
                                   double* invG, double* ft, int check, hipStream_t st) {
    using namespace mcmc;
    if (k.s.d > kSmMaxD) return hipErrorInvalidValue;
    const GlmShape gs = mcmc_glm_shape(k.s.d, k.m.n);
    const GlmArgs a = glm_args(k, gs);
    hipError_t e = smm_lds_attr((const void*)smm_eval_kernel);
    if (e != hipSuccess) return e;
    smm_eval_kernel<<<dim3(glm_grid(k.s.C, gs)), 256, kSmLdsDoubles * sizeof(double), st>>>(a, xin, lp, g, G, invG, ft,
                                                                                          check);
    return hipGetLastError();
}

hipError_t mcmc_launch_smmala_step(const mcmc::KernelArgs& k, hipStream_t st) {
    using namespace mcmc;
    if (k.s.d > kSmMaxD || k.sa.kind != SK_SMMALA) return hipErrorInvalidValue;
    const GlmShape gs = mcmc_glm_shape(k.s.d, k.m.n);
    const GlmArgs a = glm_args(k, gs);
    hipError_t e = smm_lds_attr((const void*)smm_step);
    if (e != hipSuccess) return e;
    mcmc_note_step_kernel("smm_step");
    smm_step<<<dim3(glm_grid(k.s.C, gs)), 256, kSmLdsDoubles * sizeof(double), st>>>(a);
    return hipGetLastError();
}
