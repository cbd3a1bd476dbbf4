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
//
// The pass over the tiles, evalallt and the small algebra live in smm_device.hpp, which pmala.hip shares.
#include "smm_device.hpp"

namespace mcmc {

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
