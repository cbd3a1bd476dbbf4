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
// sum_i dG_i invG[:, i] = X' (w o qf), qf_o = x_o' invG x_o.  pm_corr is a second pass over the staged X tiles
// (smm_device.hpp's smm_dw_tiles, which rmhmc.hip shares; the weight pm_dw and the staging live there too) with the
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
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const double xa = LX[(4 * kk + p.q) * SR + p.cl];
            const f64x2* vrow = reinterpret_cast<const f64x2*>(S.vb + 64 * kk + 16 * p.q);
#pragma unroll
            for (int c2 = 0; c2 < 8; ++c2) {
                const f64x2 v2 = vrow[c2];
                T[2 * c2] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, v2.x * xa, T[2 * c2], 0, 0, 0);
                T[2 * c2 + 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, v2.y * xa, T[2 * c2 + 1], 0, 0, 0);
            }
        }
        smm_wave_sync();
        if (more && tl) reinterpret_cast<f64x2*>(S.X + (b ^ 1) * kSmXS)[ti] = nxt;
        __syncthreads();
    }
}

// c = invG (X' (w o qf)) at x, invG in S.W; V: one of the tile's shared vectors
__device__ __forceinline__ void pm_corr(const GlmArgs& a, const GlmPos& p, const SmLds& S, const double (&x)[4],
                                        double* V, double (&cv)[4]) {
    f64x4 U, U2;
    if (a.m.kind == MK_LOGISTIC) smm_dw_tiles<true, true, false>(a, p, S, x, x, U, U2);
    else smm_dw_tiles<false, true, false>(a, p, S, x, x, U, U2);
    const double u[4] = {U[0], U[1], U[2], U[3]};
    smm_put_vec(V, p, u);
    smm_wave_sync();
    smm_symv(S.W + p.cl, V + p.cl, a.s.d, p.q, cv);
    smm_wave_sync();
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
#pragma unroll
        for (int c = 0; c < 16; ++c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ar = p.q + 4 * r;
                if (ar < d && p.cl <= ar) S.W[16 * smm_tri(ar, p.cl) + c] = T[c][r];
            }
        }
        smm_wave_sync();
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

// PMALA.jl:85-140, one step per loop pass; the state (pars, logTarget, grad, G, invG, firstTerm, c) lives in HBM
__global__ __launch_bounds__(256) void pm_step(GlmArgs a) {
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
            double z[4], x[4], ft[4], cv[4];
            glm_normals<1>(p, rs, chain, (uint32_t)i, d, z);
            glm_load<1>(a, p, a.st.x, x);
            glm_load<1>(a, p, a.st.sm_ft, ft);
            glm_load<1>(a, p, a.st.pm_c, cv);
            smm_put_vec(V0, p, z);
            smm_wave_sync();
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * p.q + e;
                double u = 0.0;                                         // (U' z)[r]: fma chain over c <= r
                if (r < d)
                    for (int c = 0; c <= r; ++c) u = __builtin_fma(Wc[16 * smm_tri(r, c)], V0[16 * c + p.cl], u);
                const double pm = x[e] + half * (ft[e] - cv[e]);        // PMALA.jl:94
                xp[e] = r < d ? pm + u : 0.0;                           // PMALA.jl:98
                ev[e] = r < d ? pm - xp[e] : 0.0;
            }
        }
        smm_put_vec(V1, p, ev);
        smm_wave_sync();
        // probNewGivenOld = -sum(log(diag(U))) - 0.5 e' (G / h) e     PMALA.jl:103-104
        const double quad1 = glm_sum(a, p, none, smm_quad(Gc, ld, V1 + p.cl, d, p.q, h, ev));
        const double qf = (-ld1) - 0.5 * quad1;
        smm_wave_sync();
        bool oos;
        f64x4 gp[1];
        const double lpp = smm_evalallt(a, p, S, xp, gp, oos);         // PMALA.jl:101
        smm_store_w(Wc, pGc, ld, nr, p.q, p.live);
        const double ldg = smm_chol(Wc, d, p.q);                       // proposedG = L L'
        bad = bad || !(ldg == ldg);
        smm_inverse(Wc, S.Y + p.lane, d, p.q, piGc, ld, p.live);      // proposedInvG   PMALA.jl:106
        smm_mem_sync();
        smm_load_w(Wc, piGc, ld, nr, p.q, 1.0);
        double pft[4], pc[4];
        {
            double gv[4] = {gp[0][0], gp[0][1], gp[0][2], gp[0][3]};
            smm_put_vec(V0, p, gv);
            smm_wave_sync();
            smm_symv(Wc, V0 + p.cl, d, p.q, pft);                      // proposedFirstTerm   PMALA.jl:107
            smm_wave_sync();
        }
        pm_corr(a, p, S, xp, V0, pc);                                  // sum(proposedSecondTerm, 2)   PMALA.jl:108-111
        for (int idx = p.q; idx < nr; idx += 4) Wc[16 * idx] = h * Wc[16 * idx];
        smm_wave_sync();
        const double ld2 = smm_chol(Wc, d, p.q);                       // chol(h proposedInvG)
        bad = bad || !(ld2 == ld2);
        {
            double x[4];
            glm_load<1>(a, p, a.st.x, x);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                ev[e] = 4 * p.q + e < d ? (xp[e] + half * (pft[e] - pc[e])) - x[e] : 0.0;   // PMALA.jl:114, 117
        }
        smm_put_vec(V1, p, ev);
        smm_wave_sync();
        const double quad2 = glm_sum(a, p, none, smm_quad(pGc, ld, V1 + p.cl, d, p.q, h, ev));
        const double qb = (-ld2) - 0.5 * quad2;                        // probOldGivenNew
        const double ratio = ((lpp + qb) - lp) - qf;                   // PMALA.jl:119
        // a proposal out of support or with a failed pivot is rejected (the reference throws out of chol)
        const bool acc = !(bad || oos) && glm_mh_short_circuit(rs, chain, (uint32_t)i, ratio);
        if (acc) {
            glm_store<1>(a, p, a.st.x, s.ld, xp);
            glm_store4<1>(a, p, a.st.g, s.ld, gp);
            glm_store<1>(a, p, a.st.sm_ft, s.ld, pft);
            glm_store<1>(a, p, a.st.pm_c, s.ld, pc);
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
        if (sa.tuner && i <= s.tuner_burnin && (i % sa.adapt_step) == 0) {   // PMALA.jl:131-137 (EmpiricalMALATune)
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

}  // namespace mcmc

hipError_t mcmc_launch_pmala_dtensor(const mcmc::KernelArgs& k, const double* xin, double* lp, double* g, double* G,
                                     double* dG, hipStream_t st) {
    using namespace mcmc;
    if (k.s.d > kSmMaxD || dG == nullptr) return hipErrorInvalidValue;
    const GlmShape gs = mcmc_glm_shape(k.s.d, k.m.n);
    const GlmArgs a = glm_args(k, gs);
    hipError_t e = smm_lds_attr((const void*)pm_dtensor_kernel);
    if (e != hipSuccess) return e;
    pm_dtensor_kernel<<<dim3(glm_grid(k.s.C, gs)), 256, kSmLdsDoubles * sizeof(double), st>>>(a, xin, lp, g, G, dG);
    return hipGetLastError();
}

hipError_t mcmc_launch_pmala_corr(const mcmc::KernelArgs& k, hipStream_t st) {
    using namespace mcmc;
    if (k.s.d > kSmMaxD || k.st.pm_c == nullptr || k.st.sm_invG == nullptr) return hipErrorInvalidValue;
    const GlmShape gs = mcmc_glm_shape(k.s.d, k.m.n);
    const GlmArgs a = glm_args(k, gs);
    hipError_t e = smm_lds_attr((const void*)pm_corr_kernel);
    if (e != hipSuccess) return e;
    pm_corr_kernel<<<dim3(glm_grid(k.s.C, gs)), 256, kSmLdsDoubles * sizeof(double), st>>>(a);
    return hipGetLastError();
}

hipError_t mcmc_launch_pmala_step(const mcmc::KernelArgs& k, hipStream_t st) {
    using namespace mcmc;
    if (k.s.d > kSmMaxD || k.sa.kind != SK_PMALA || k.st.pm_c == nullptr) return hipErrorInvalidValue;
    const GlmShape gs = mcmc_glm_shape(k.s.d, k.m.n);
    const GlmArgs a = glm_args(k, gs);
    hipError_t e = smm_lds_attr((const void*)pm_step);
    if (e != hipSuccess) return e;
    mcmc_note_step_kernel("pm_step");
    pm_step<<<dim3(glm_grid(k.s.C, gs)), 256, kSmLdsDoubles * sizeof(double), st>>>(a);
    return hipGetLastError();
}
