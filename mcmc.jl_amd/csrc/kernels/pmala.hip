// pmala.hip -- the derivatives of the metric tensor of the probit / logistic regression models (`evalalldt`,
// likmodel.jl:27) and the position-dependent MALA sampler on top of them (src/samplers/PMALA.jl:42-141), d <= 16.
//
// Geometry, log-target, gradient, tensor and the small algebra are smmala.hip's (smm_device.hpp): a wave owns a tile
// of 16 chains, lane (q, cl) chain cl and coordinates 4q + e, four tiles a workgroup share the staged X tiles.
//
// The weight's derivative w = dv / d eta of observation o (pm_dw):
//   probit (examples/probit_regression.jl:52-68, as written, on det_exp / det_normlogcdf): la = logcdf(eta),
//     lb = logcdf(-eta), A = (-(eta^2 + log 2 pi)) / 2, v01 = exp((((-eta^2) - 2 la) - lb) - log 2 pi),
//     w = v01 (exp(A - lb) - 2 (exp(A) + eta exp(la)));
//   logistic: sig = |rv| of det_logi (p or 1 - p), v = sig (1 - sig), w = (v (1 - 2 sig)) (-wt), wt = s (2y - 1) the
//     tile's response column: p (1 - p) (1 - 2p) for the example's link s = +1, its negative for s = -1.
//
// The full dG (pm_dtensor_kernel; an inspection path): d slabs formed one at a time by smm_tiles' tensor contraction
// with the weights RN(w_o X[o][i]).  Element (a, b), b <= a, of slab i is the fma chain over the observations o in
// ascending order, from zero, of fma(X[o][a], RN(RN(w_o X[o][i]) X[o][b]), .); the upper triangle is its mirror; the
// prior precision is constant and adds nothing.  eta is smm_tiles' chain.
//
// The sampler's drift correction c = sum_i invG dG_i invG[:, i] (PMALA.jl:77-80, 94) never forms the slabs:
// sum_i dG_i invG[:, i] = X' (w o qf), qf_o = x_o' invG x_o.  pm_corr (smm_device.hpp, beside the step body that calls
// it) is a second pass over the staged X tiles (smm_dw_tiles; the weight pm_dw and the staging live there too) with the
// chain's invG in the tile's workspace W; per tile of 16 observations and per chain c of the wave's tile:
//   eta           smm_tiles' MFMA chain;
//   M = invG_c X' one v_mfma_f64_16x16x4_f64 per k-slice e: A lane (q, cl) = invG_c[cl][4q + e] (held in registers for
//                 the whole pass, zero past d), B lane (q, cl) = X[obs cl][4q + e]; lane (q, cl) register r is
//                 M[j][obs cl], j = q + 4r: the fma chain over (e, q') of fma(invG_c[j][4q' + e], X[o][4q' + e], .);
//   qf            P[j] = RN(M[j][o] X[o][j]); the lane's s_q = ((P[q] + P[q+4]) + P[q+8]) + P[q+12]; the four
//                 quarters by one MFMA with A = 1: qf_o = ((s_0 + s_1) + s_2) + s_3 (from +0); it crosses to the lanes
//                 that hold w through LDS (the weights' buffer vb, [16 obs][16 chains]);
//   u = X' (w o qf)  the gradient's MFMA with the B operand RN(w_o qf_o) (zero on padded observations): an fma chain
//                 over the observations in ascending order from zero;
// and c = invG u by smm_symv (rows' fma chains over the columns 0..d-1).  tests/pmala_oracle.c restates all of it.
#include "smm_device.hpp"

namespace mcmc {

// slab i of dG for the tile's sixteen chains into T (lane (q, cl) register r of chain c: dG_i[q + 4r][cl])
template <bool LOGI>
__device__ __forceinline__ void pm_slab(const GlmArgs& a, const GlmPos& p, const SmLds& S, const double (&x)[4], int i,
                                        f64x4 (&T)[16]) {
    const ModelArgs& M = a.m;
    constexpr int SR = glm_row_stride(16);
    constexpr int YO = glm_y_offset(16);
    constexpr int kHalf = kSmXS / 2;
    const int64_t ntiles = a.g.n_pad / 16;
    const int ti = threadIdx.x < kHalf ? (int)threadIdx.x : 0;
    const bool tl = threadIdx.x < kHalf;
    const double (*sptab)[10] = reinterpret_cast<const double (*)[10]>(S.sp);
    pm_stage_first<LOGI>(a, S);
#pragma unroll
    for (int c = 0; c < 16; ++c) T[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int64_t t = 0; t < ntiles; ++t) {
        const int b = (int)(t & 1);
        const double* LX = S.X + b * kSmXS;
        const bool more = t + 1 < ntiles;
        f64x2 nxt = f64x2{0.0, 0.0};
        if (more) nxt = reinterpret_cast<const f64x2*>(M.X + (size_t)(t + 1) * kSmXS)[ti];
        f64x4 eta = f64x4{0.0, 0.0, 0.0, 0.0};
        {
            const double* xrow = LX + p.cl * SR + 4 * p.q;
#pragma unroll
            for (int slot = 0; slot < 4; ++slot)
                eta = __builtin_amdgcn_mfma_f64_16x16x4f64(xrow[slot], x[slot], eta, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = p.q + 4 * r;
            const double w = pm_dw<LOGI>(eta[r], LX[YO + o], sptab);
            const bool in = t * 16 + o < M.n;
            S.vb[64 * r + p.lane] = in ? w * LX[o * SR + i] : 0.0;
        }
        smm_wave_sync();
        smm_gram_mfma(LX, S, p, T);
        smm_wave_sync();
        if (more && tl) reinterpret_cast<f64x2*>(S.X + (b ^ 1) * kSmXS)[ti] = nxt;
        __syncthreads();
    }
}

// evalalldt (mcmc_model_eval_dtensor): lp, gradient [d][ld], G packed [d(d+1)/2][ld] (smm_evalallt's, any may be
// NULL) and dG [d slabs][d(d+1)/2][ld]
__global__ __launch_bounds__(256) void pm_dtensor_kernel(GlmArgs a, const double* xin, double* lp_out, double* g_out,
                                                         double* G_out, double* dG_out) {
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
    if (G_out) smm_store_w(Wc, G_out + cc, ld, nr, p.q, p.live);
    smm_wave_sync();
    for (int i = 0; i < d; ++i) {
        f64x4 T[16];
        if (a.m.kind == MK_LOGISTIC) pm_slab<true>(a, p, S, x, i, T);
        else pm_slab<false>(a, p, S, x, i, T);
        smm_put_tiles(p, S, d, T);
        smm_store_w(Wc, dG_out + (size_t)i * (size_t)nr * ld + cc, ld, nr, p.q, p.live);
        smm_wave_sync();
    }
}

// the correction c of the chains' current position from the state's invG (the chains' first evaluation)
__global__ __launch_bounds__(256) void pm_corr_kernel(GlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const GlmPos p = glm_pos(a);
    const SmLds S = smm_lds(smem, p.wave);
    const int d = a.s.d, nr = d * (d + 1) / 2;
    const int64_t cc = p.live ? p.c : 0;
    double x[4], cv[4];
    glm_load<1>(a, p, a.st.x, x);
    smm_load_w(S.W + p.cl, a.st.sm_invG + cc, (size_t)a.s.ld, nr, p.q, 1.0);
    smm_wave_sync();
    pm_corr(a, p, S, x, S.Y, cv);
    glm_store<1>(a, p, a.st.pm_c, a.s.ld, cv);
}

// PMALA.jl:85-140: smm_device.hpp's MALA step body with the drift correction
__global__ __launch_bounds__(256) void pm_step(GlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    smm_mala_step<true>(a, smem);
}

}  // namespace mcmc

hipError_t mcmc_launch_pmala_dtensor(const mcmc::KernelArgs& k, const double* xin, double* lp, double* g, double* G,
                                     double* dG, hipStream_t st) {
    using namespace mcmc;
    if (k.s.d > kSmMaxD || dG == nullptr) return hipErrorInvalidValue;
    return smm_launch(pm_dtensor_kernel, nullptr, kSmLdsDoubles, k, st, xin, lp, g, G, dG);
}

hipError_t mcmc_launch_pmala_corr(const mcmc::KernelArgs& k, hipStream_t st) {
    using namespace mcmc;
    if (k.s.d > kSmMaxD || k.st.pm_c == nullptr || k.st.sm_invG == nullptr) return hipErrorInvalidValue;
    return smm_launch(pm_corr_kernel, nullptr, kSmLdsDoubles, k, st);
}

hipError_t mcmc_launch_pmala_step(const mcmc::KernelArgs& k, hipStream_t st) {
    using namespace mcmc;
    if (k.s.d > kSmMaxD || k.sa.kind != SK_PMALA || k.st.pm_c == nullptr) return hipErrorInvalidValue;
    return smm_launch(pm_step, "pm_step", kSmLdsDoubles, k, st);
}
