// lmc.hip -- the two Lagrangian Monte Carlo samplers on the probit / logistic regression models, d <= 16, on a model
// with tensor derivatives: ERMLMC (src/samplers/ERMLMC.jl:84-179, lmc_step<false>) and the semi-explicit RMLMC
// (src/samplers/RMLMC.jl:89-179, lmc_step<true>), statement by statement.
//
// Geometry, log-target, gradient, tensor and the small algebra are smmala.hip's (smm_device.hpp); the barrier
// discipline is rmhmc.hip's.
//
// Neither sampler forms C = 0.5 (permutedims(dG, [3 2 1]) + permutedims(dG, [1 3 2]) - dG).  On these models
// dG[a, b, r] = sum_o w_o X_oa X_ob X_or is symmetric in all three indices, so C = 0.5 dG and
//   vxC(v)   = 0.5 K(v),  K(v) = X' diag(w o t) X,  t = X v      the weighted Gram pass (smm_dw_tiles_impl<.., GR>);
//   vxC(v) v = 0.5 X' (w o t^2)                                   RMHMC's T2 term;
//   G + c vxC(v) = fma(0.5 c, K, G) entry by entry: symmetric, factored by smm_chol, logdet = 2 sum log diag.
//
// One step (i the sampler's counter, c the chain), lmc_geom the geometry at a position:
//   lmc_geom          evalallt -> G (kept in st.sm_pG), cholG (ld = sum log diag), invG (kept in st.sm_pinvG),
//                     traceInvGxdG = X' (w o qf) (PMALA's U), dphi = (-grad) + 0.5 trace;
//   velocity          chol(invG)' randn: the inverse factored again by smm_chol, row r of the lower factor times the
//                     step's NORMAL blocks, the fma chain over c <= r;
//   E                 ((-lp) - ld) + 0.5 v'(G v) for ERMLMC, ((-lp) + ld) + 0.5 v'(G v) for RMLMC, as written;
//   nRandomLeaps      ceil(uniform52(w0, w1) nLeaps), block (c, i, 0, TAG_LMC);
//   ERMLMC leapfrog   half, pars + h v, lmc_geom, half; half: rhs = G v - (h/2) dphi, A+ = G + (h/2) vxC(v),
//                     delta - 2 ld(A+), v = A+ \ rhs, A- = G - (h/2) vxC(v), delta + 2 ld(A-): 4 Gram passes, one
//                     tensor pass and one trace pass;
//   RMLMC leapfrog    nNewton passes lv = v - (h/2) (invG (0.5 X'(w o t(lv)^2) + dphi)); delta - 2 ld(G + h vxC(lvin)),
//                     lvin the last pass's input; pars + h v; lmc_geom; K(v) and X'(w o t^2) from one pass;
//                     delta + 2 ld(G - h vxC(v)); v - (h/2) (invG (0.5 X'(w o t^2) + dphi)): nNewton + 4 passes;
//   accept            glm_mh_short_circuit on (E - proposedE) + delta.
//
// Barriers.  Every pass over X has workgroup barriers inside, so every wave makes the same passes: 2 at the step's
// start, then the leapfrog's for the workgroup's longest trajectory (rm_max).  Nothing between the passes depends on a
// chain's values: a chain that has finished its trajectory, or whose trajectory has failed, keeps still under a mask.
//
// Failed trajectories.  A log-target that is not finite at any evaluation, a pivot <= 0 or not finite at any G, invG or
// G +- c vxC (the reference's logdet throws on a negative determinant and goes through LU on an indefinite matrix with
// a positive one: both reject here), a position or velocity that is not finite, a ratio that is not finite, or a
// nRandomLeaps draw of 0 rejects the step.  No chain carries a NaN forward.  tests/lmc_oracle.c restates all of it.
#include "smm_device.hpp"

namespace mcmc {

// any of the lane's four values not finite, over the chain's four lanes
__device__ __forceinline__ bool lmc_not_finite(const double (&u)[4]) {
    int nf = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) nf |= !(u[e] - u[e] == 0.0);
    nf |= __shfl_xor(nf, 16, 64);
    nf |= __shfl_xor(nf, 32, 64);
    return nf != 0;
}

// the second pass with the weight's derivative at x: QF the trace term from invG in W; GR the raw weighted Gram
// matrices K(v) of the tile's chains -> W (lower triangles); T2 X' (w o t^2)
template <bool QF, bool T2, bool GR>
__device__ __forceinline__ void lmc_pass(const GlmArgs& a, const GlmPos& p, const SmLds& S, const double (&x)[4],
                                         const double (&v)[4], double (&u)[4], double (&u2)[4]) {
    f64x4 U, U2;
    f64x4 T[16];
    if (a.m.kind == MK_LOGISTIC) smm_dw_tiles_impl<true, QF, T2, GR>(a, p, S, x, v, U, U2, T);
    else smm_dw_tiles_impl<false, QF, T2, GR>(a, p, S, x, v, U, U2, T);
    if (GR) smm_put_tiles(p, S, a.s.d, T);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        u[e] = U[e];
        u2[e] = U2[e];
    }
}

// W = G + (2 cq) vxC from the raw Gram matrix in W and G in the workspace: fma(cq, K, G) entry by entry, then its
// Cholesky factor in place; returns sum log diag, or NaN on a failed pivot
__device__ __forceinline__ double lmc_factor(double* Wc, const double* Gc, size_t ld, int d, int nr, int q, double cq) {
    for (int idx = q; idx < nr; idx += 4) Wc[16 * idx] = __builtin_fma(cq, Wc[16 * idx], Gc[(size_t)idx * ld]);
    smm_wave_sync();
    return smm_chol(Wc, d, q);
}

struct LmcGeom {
    double lp, ld;      // log-target, sum log diag cholG
    f64x4 g;            // gradient
    double tr[4];       // traceInvGxdG
    bool bad;           // out of support or a failed pivot
};

// The geometry at x.  Leaves G in st.sm_pG, invG in st.sm_pinvG and in W.  vel (uniform over the workgroup): also the
// step's velocity chol(invG)' randn (ERMLMC.jl:103), a failed pivot of that factor in bad.
__device__ __forceinline__ void lmc_geom(const GlmArgs& a, const GlmPos& p, const SmLds& S, const double (&x)[4],
                                         double* Gc, double* iGc, bool vel, const Stream& rs, uint32_t chain,
                                         uint32_t step, LmcGeom& o, double (&v)[4]) {
    const int d = a.s.d, nr = d * (d + 1) / 2;
    const size_t ld = (size_t)a.s.ld;
    double* const Wc = S.W + p.cl;
    bool oos;
    f64x4 g1[1];
    o.lp = smm_evalallt(a, p, S, x, g1, oos);
    o.g = g1[0];
    smm_store_w(Wc, Gc, ld, nr, p.q, p.live);
    smm_wave_sync();
    o.ld = smm_chol(Wc, d, p.q);
    o.bad = oos || !(o.ld == o.ld);
    smm_inverse(Wc, S.Y + p.lane, d, p.q, iGc, ld, p.live);
    smm_mem_sync();
    smm_load_w(Wc, iGc, ld, nr, p.q, 1.0);
    smm_wave_sync();
    if (vel) {
        const double ldi = smm_chol(Wc, d, p.q);
        o.bad = o.bad || !(ldi == ldi);
        double z[4];
        glm_normals<1>(p, rs, chain, step, d, z);
        smm_put_vec(S.Y, p, z);
        smm_wave_sync();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 4 * p.q + e;
            double u = 0.0;
            if (r < d)
                for (int c = 0; c <= r; ++c) u = __builtin_fma(Wc[16 * smm_tri(r, c)], S.Y[16 * c + p.cl], u);
            v[e] = u;
        }
        smm_wave_sync();
        smm_load_w(Wc, iGc, ld, nr, p.q, 1.0);
        smm_wave_sync();
    }
    double u2[4];
    lmc_pass<true, false, false>(a, p, S, x, x, o.tr, u2);
}

template <bool SEMI>
__global__ __launch_bounds__(256) void lmc_step(GlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const StepArgs& s = a.s;
    const SamplerArgs& sa = a.sa;
    const GlmPos p = glm_pos(a);
    const SmLds S = smm_lds(smem, p.wave);
    int* const iscr = reinterpret_cast<int*>(smem + kSmLdsDoubles);
    const GlmLds none{};
    const Stream rs{s.key0, s.key1};
    const uint32_t chain = s.chain0 + (uint32_t)p.c;
    const int64_t cc = p.live ? p.c : 0;
    const int d = s.d, nr = d * (d + 1) / 2;
    const size_t ld = (size_t)s.ld;
    const int nn = sa.n_newton;
    const bool tuned = sa.tuner != 0;
    const int64_t max_leaps = sa.max_leaps;
    double* const Wc = S.W + p.cl;
    double* const V0 = S.Y;
    double* const pGc = a.st.sm_pG + cc;
    double* const piGc = a.st.sm_pinvG + cc;
    double lp = a.st.lp[cc];
    double eps = tuned ? a.st.t_step[cc] : sa.leap_step;
    int64_t nl_fixed = tuned ? (int64_t)a.st.t_leaps[cc] : sa.n_leaps;
    int32_t n_acc = tuned ? a.st.t_acc[cc] : 0;
    int32_t n_prop = tuned ? a.st.t_prop[cc] : 0;
    int64_t n_evals = 0;
    for (int t = 0; t < s.nsteps; ++t) {
        const int64_t i = s.step_begin + t;
        if (tuned) n_prop += 1;
        const double hc = 0.5 * eps;                                    // (0.5*leapStep)
        double xp[4], v[4], dphi[4], w4[4], u2[4];
        f64x4 gp;
        double ldp, lpp = lp;
        bool dead;
        glm_load<1>(a, p, a.st.x, xp);
        {
            LmcGeom o;
            lmc_geom(a, p, S, xp, pGc, piGc, true, rs, chain, (uint32_t)i, o, v);   // ERMLMC.jl:73-79, 103
            dead = o.bad;
            ldp = o.ld;
            f64x4 gs[1];
            glm_load4<1>(a, p, a.st.g, gs);                             // the state's gradient, bit for bit
            gp = gs[0];
#pragma unroll
            for (int e = 0; e < 4; ++e) dphi[e] = (-gp[e]) + 0.5 * o.tr[e];
        }
        smm_load_w(Wc, pGc, ld, nr, p.q, 1.0);
        smm_wave_sync();
        rm_symv(p, Wc, V0, d, v, w4);
        const double quad0 = glm_sum(a, p, none, rm_dot_part(p, d, v, w4));
        const double E = SEMI ? ((-lp) + ldp) + 0.5 * quad0 : ((-lp) - ldp) + 0.5 * quad0;   // RMLMC.jl:110, ERMLMC.jl:105
        int nrl;
        {
            const u32x4 w = rs.block(chain, (uint32_t)i, 0u, TAG_LMC);
            nrl = (int)__builtin_ceil(uniform52(w.x, w.y) * (double)nl_fixed);   // ERMLMC.jl:112
        }
        n_evals += nrl;
        const int nl_wg = rm_max(iscr, nrl, p.live);                    // the workgroup's longest trajectory
        double delta = 0.0;
        for (int l = 0; l < nl_wg; ++l) {
            const bool on = l < nrl;                                    // chains that finished keep still
            if (!SEMI) {
#pragma unroll 1
                for (int hs = 0; hs < 2; ++hs) {                        // ERMLMC.jl:116-126, 141-151
                    double rhs[4];
                    smm_load_w(Wc, pGc, ld, nr, p.q, 1.0);
                    smm_wave_sync();
                    rm_symv(p, Wc, V0, d, v, w4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) rhs[e] = w4[e] - hc * dphi[e];
#pragma unroll 1
                    for (int sg = 0; sg < 2; ++sg) {
                        lmc_pass<false, false, true>(a, p, S, xp, v, w4, u2);
                        const double ldA = lmc_factor(Wc, pGc, ld, d, nr, p.q, sg == 0 ? hc * 0.5 : -(hc * 0.5));
                        if (sg == 0) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) S.vb[16 * (4 * p.q + e) + p.cl] = rhs[e];
                            smm_wave_sync();
                            double v1[4];
                            smm_solve(Wc, S.vb + p.cl, S.Y + p.lane, d, p.q, v1);
                            smm_wave_sync();
                            const bool bad = !(ldA == ldA) || lmc_not_finite(v1);
                            if (on && !dead) {
                                if (bad) {
                                    dead = true;
                                } else {
                                    delta = delta - 2.0 * ldA;
#pragma unroll
                                    for (int e = 0; e < 4; ++e) v[e] = v1[e];
                                }
                            }
                        } else if (on && !dead) {
                            if (!(ldA == ldA)) dead = true;
                            else delta = delta + 2.0 * ldA;
                        }
                    }
                    if (hs == 0) {
                        double cand[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) cand[e] = xp[e] + eps * v[e];   // ERMLMC.jl:129
                        const bool nfx = lmc_not_finite(cand);
                        if (on && !dead) {
                            if (nfx) {
                                dead = true;
                            } else {
#pragma unroll
                                for (int e = 0; e < 4; ++e) xp[e] = cand[e];
                            }
                        }
                        LmcGeom o;
                        lmc_geom(a, p, S, xp, pGc, piGc, false, rs, chain, (uint32_t)i, o, w4);   // ERMLMC.jl:131-138
                        if (on && !dead) {
                            if (o.bad) {
                                dead = true;
                            } else {
                                lpp = o.lp;
                                ldp = o.ld;
                                gp = o.g;
#pragma unroll
                                for (int e = 0; e < 4; ++e) dphi[e] = (-gp[e]) + 0.5 * o.tr[e];
                            }
                        }
                    }
                }
            } else {
                double lv[4], lvin[4], is[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) lv[e] = lvin[e] = v[e];
                smm_load_w(Wc, piGc, ld, nr, p.q, 1.0);
                smm_wave_sync();
                for (int k = 0; k < nn; ++k) {                          // RMLMC.jl:122-127
#pragma unroll
                    for (int e = 0; e < 4; ++e) lvin[e] = lv[e];
                    lmc_pass<false, true, false>(a, p, S, xp, lv, w4, u2);
                    double sv[4], cand[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) sv[e] = 0.5 * u2[e] + dphi[e];
                    rm_symv(p, Wc, V0, d, sv, is);
#pragma unroll
                    for (int e = 0; e < 4; ++e) cand[e] = v[e] - hc * is[e];
                    const bool nfv = lmc_not_finite(cand);
                    if (on && !dead) {
                        if (nfv) {
                            dead = true;
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) lv[e] = cand[e];
                        }
                    }
                }
                if (on && !dead) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = lv[e];           // RMLMC.jl:128
                }
#pragma unroll 1
                for (int sg = 0; sg < 2; ++sg) {
                    // sg 0: vxC of the last pass's input iterate (RMLMC.jl:131); sg 1: of the velocity (RMLMC.jl:146-149)
                    double gv[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) gv[e] = sg == 0 ? lvin[e] : v[e];
                    lmc_pass<false, true, true>(a, p, S, xp, gv, w4, u2);
                    const double ldA = lmc_factor(Wc, pGc, ld, d, nr, p.q, sg == 0 ? eps * 0.5 : -(eps * 0.5));
                    if (on && !dead) {
                        if (!(ldA == ldA)) dead = true;
                        else delta = sg == 0 ? delta - 2.0 * ldA : delta + 2.0 * ldA;
                    }
                    if (sg == 0) {
                        double cand[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) cand[e] = xp[e] + eps * v[e];   // RMLMC.jl:134
                        const bool nfx = lmc_not_finite(cand);
                        if (on && !dead) {
                            if (nfx) {
                                dead = true;
                            } else {
#pragma unroll
                                for (int e = 0; e < 4; ++e) xp[e] = cand[e];
                            }
                        }
                        LmcGeom o;
                        lmc_geom(a, p, S, xp, pGc, piGc, false, rs, chain, (uint32_t)i, o, w4);   // RMLMC.jl:136-142
                        if (on && !dead) {
                            if (o.bad) {
                                dead = true;
                            } else {
                                lpp = o.lp;
                                ldp = o.ld;
                                gp = o.g;
#pragma unroll
                                for (int e = 0; e < 4; ++e) dphi[e] = (-gp[e]) + 0.5 * o.tr[e];
                            }
                        }
                    }
                }
                smm_load_w(Wc, piGc, ld, nr, p.q, 1.0);
                smm_wave_sync();
                double sv[4], cand[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) sv[e] = 0.5 * u2[e] + dphi[e];
                rm_symv(p, Wc, V0, d, sv, is);
#pragma unroll
                for (int e = 0; e < 4; ++e) cand[e] = v[e] - hc * is[e];   // RMLMC.jl:151
                const bool nfv = lmc_not_finite(cand);
                if (on && !dead) {
                    if (nfv) {
                        dead = true;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = cand[e];
                    }
                }
            }
        }
        smm_load_w(Wc, pGc, ld, nr, p.q, 1.0);
        smm_wave_sync();
        rm_symv(p, Wc, V0, d, v, w4);
        const double quadp = glm_sum(a, p, none, rm_dot_part(p, d, v, w4));
        const double Ep = SEMI ? ((-lpp) + ldp) + 0.5 * quadp : ((-lpp) - ldp) + 0.5 * quadp;   // RMLMC.jl:155, ERMLMC.jl:155
        const double ratio = (E - Ep) + delta;                          // ERMLMC.jl:158
        const bool acc = !dead && nrl > 0 && (ratio - ratio == 0.0) && glm_mh_short_circuit(rs, chain, (uint32_t)i, ratio);
        f64x4 go[1] = {gp};
        if (acc) {
            glm_store<1>(a, p, a.st.x, s.ld, xp);
            glm_store4<1>(a, p, a.st.g, s.ld, go);
            lp = lpp;
            if (tuned) n_acc += 1;
        }
        int64_t kk;
        if (kept_index(i - s.run_step0, s.burnin, s.thinning, s.len, &kk)) {
            if (!acc) {
                glm_load<1>(a, p, a.st.x, xp);
                glm_load4<1>(a, p, a.st.g, go);
            }
            glm_store_kept<1>(a, p, kk, s.samples, xp);
            glm_store_kept4<1>(a, p, kk, s.grads, go);
            glm_store_bit(a, p, kk, acc);
        }
        if (tuned && i <= s.tuner_burnin && (i % sa.adapt_step) == 0) {   // ERMLMC.jl:170-176 (EmpiricalHMCTune)
            eps = eps * glm_tune_factor(n_acc, n_prop, sa.target_rate);
            double nlf = __builtin_ceil(sa.target_path / eps);
            if (nlf > (double)sa.max_step) nlf = (double)sa.max_step;
            if (nlf > (double)max_leaps) nlf = (double)max_leaps;
            nl_fixed = (int64_t)nlf;
            n_acc = 0;
            n_prop = 0;
        }
        smm_mem_sync();                                                // the state the next step's lanes read
    }
    if (p.live && p.q == 0) {
        a.st.lp[p.c] = lp;
        if (tuned) {
            a.st.t_step[p.c] = eps;
            a.st.t_leaps[p.c] = (int32_t)nl_fixed;
            a.st.t_acc[p.c] = n_acc;
            a.st.t_prop[p.c] = n_prop;
        }
    }
    glm_count_evals(a, p, n_evals);
}

}  // namespace mcmc

hipError_t mcmc_launch_lmc_step(const mcmc::KernelArgs& k, hipStream_t st) {
    using namespace mcmc;
    const bool semi = k.sa.kind == SK_RMLMC;
    if (k.s.d > kSmMaxD || (k.sa.kind != SK_ERMLMC && !semi) || (semi && k.sa.n_newton < 1) ||
        k.st.sm_pG == nullptr || k.st.sm_pinvG == nullptr || (k.m.kind != MK_LOGISTIC && k.m.kind != MK_PROBIT))
        return hipErrorInvalidValue;
    const GlmShape gs = mcmc_glm_shape(k.s.d, k.m.n);
    const GlmArgs a = glm_args(k, gs);
    const void* f = semi ? (const void*)lmc_step<true> : (const void*)lmc_step<false>;
    hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kRmLdsDoubles * sizeof(double)));
    if (e != hipSuccess) return e;
    mcmc_note_step_kernel(semi ? "lmc_step<rmlmc>" : "lmc_step<ermlmc>");
    if (semi) lmc_step<true><<<dim3(glm_grid(k.s.C, gs)), 256, kRmLdsDoubles * sizeof(double), st>>>(a);
    else lmc_step<false><<<dim3(glm_grid(k.s.C, gs)), 256, kRmLdsDoubles * sizeof(double), st>>>(a);
    return hipGetLastError();
}
