// lmc.hip -- the two Lagrangian Monte Carlo samplers on the probit / logistic regression models, d <= 16, on a model
// with tensor derivatives: ERMLMC (src/samplers/ERMLMC.jl:84-179, lmc_step<false>) and the semi-explicit RMLMC
// (src/samplers/RMLMC.jl:89-179, lmc_step<true>), statement by statement.
//
// Geometry, log-target, gradient, tensor and the small algebra are smmala.hip's (smm_device.hpp); the barrier
// discipline and the step's frame (tuner registers, leapfrog count, mask, commit) are rmhmc.hip's.
//
// Neither sampler forms C = 0.5 (permutedims(dG, [3 2 1]) + permutedims(dG, [1 3 2]) - dG).  On these models
// dG[a, b, r] = sum_o w_o X_oa X_ob X_or is symmetric in all three indices, so C = 0.5 dG and
//   vxC(v)   = 0.5 K(v),  K(v) = X' diag(w o t) X,  t = X v      the weighted Gram pass (smm_pass<.., GR>);
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

// The geometry at x (ERMLMC.jl:73-79).  Leaves G in st.sm_pG, invG in st.sm_pinvG and in W.  Every wave of the
// workgroup calls it (two passes over X).
__device__ __forceinline__ void lmc_geom(const GlmArgs& a, const GlmPos& p, const SmLds& S, const double (&x)[4],
                                         double* Gc, double* iGc, LmcGeom& o) {
    const int d = a.s.d, nr = d * (d + 1) / 2;
    const size_t ld = (size_t)a.s.ld;
    double* const Wc = S.W + p.cl;
    bool oos;
    f64x4 g1[1];
    o.lp = smm_evalallt(a, p, S, x, g1, oos);
    o.g = g1[0];
    smm_store_w(Wc, Gc, ld, nr, p.q, p.live);
    smm_wave_sync();
    o.ld = smm_factor_invert(Wc, S.Y + p.lane, d, nr, p.q, iGc, ld, p.live);
    o.bad = oos || !(o.ld == o.ld);
    smm_wave_sync();
    double u2[4];
    smm_pass<true, false, false>(a, p, S, x, x, o.tr, u2);
}

// The step's velocity chol(invG)' randn (ERMLMC.jl:103) from invG in W, which it leaves factored; returns whether a
// pivot of that factor failed
__device__ __forceinline__ bool lmc_velocity(const GlmPos& p, const SmLds& S, int d, const Stream& rs, uint32_t chain,
                                             uint32_t step, double (&v)[4]) {
    double* const Wc = S.W + p.cl;
    const double ldi = smm_chol(Wc, d, p.q);
    double z[4];
    glm_normals<1>(p, rs, chain, step, d, z);
    smm_put_vec(S.Y, p, z);
    smm_wave_sync();
    smm_lower_mul(Wc, S.Y + p.cl, d, p.q, v);
    smm_wave_sync();
    return !(ldi == ldi);
}

// the trajectory's registers of one chain
struct LmcTraj {
    double x[4], v[4], dphi[4];   // position, velocity, dphi = (-grad) + 0.5 traceInvGxdG at the position
    f64x4 g;                      // gradient at the position
    double lp, ld;                // log-target and sum log diag cholG at the position
    double delta;                 // the log-determinants' sum
    bool dead;                    // the trajectory has failed
};

// pars + eps v (ERMLMC.jl:129, RMLMC.jl:134), then the geometry there (ERMLMC.jl:131-138, RMLMC.jl:136-142), each
// taken under the mask.  Every wave of the workgroup calls it (lmc_geom's passes).
__device__ __forceinline__ void lmc_move(const GlmArgs& a, const GlmPos& p, const SmLds& S, double* Gc, double* iGc,
                                         double eps, bool on, LmcTraj& T) {
    double cand[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) cand[e] = T.x[e] + eps * T.v[e];
    if (rm_take(on, T.dead, smm_not_finite(cand))) {
#pragma unroll
        for (int e = 0; e < 4; ++e) T.x[e] = cand[e];
    }
    LmcGeom o;
    lmc_geom(a, p, S, T.x, Gc, iGc, o);
    if (rm_take(on, T.dead, o.bad)) {
        T.lp = o.lp;
        T.ld = o.ld;
        T.g = o.g;
#pragma unroll
        for (int e = 0; e < 4; ++e) T.dphi[e] = (-T.g[e]) + 0.5 * o.tr[e];
    }
}

// RMLMC's velocity update v - hc (invG (0.5 u2 + dphi)) (RMLMC.jl:124-126, 151), invG in W, u2 = X' (w o t^2): taken
// into out under the mask
__device__ __forceinline__ void lmc_kick(const GlmPos& p, const double* Wc, double* V, int d, double hc,
                                         const double (&u2)[4], bool on, LmcTraj& T, double (&out)[4]) {
    double sv[4], is[4], cand[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) sv[e] = 0.5 * u2[e] + T.dphi[e];
    rm_symv(p, Wc, V, d, sv, is);
#pragma unroll
    for (int e = 0; e < 4; ++e) cand[e] = T.v[e] - hc * is[e];
    if (rm_take(on, T.dead, smm_not_finite(cand))) {
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = cand[e];
    }
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
    double* const Wc = S.W + p.cl;
    double* const V0 = S.Y;
    double* const pGc = a.st.sm_pG + cc;
    double* const piGc = a.st.sm_pinvG + cc;
    double lp = a.st.lp[cc];
    RmTuner tn = rm_tuner_load(a, cc);
    int64_t n_evals = 0;
    for (int t = 0; t < s.nsteps; ++t) {
        const int64_t i = s.step_begin + t;
        if (tuned) tn.n_prop += 1;
        const double eps = tn.eps;
        const double hc = 0.5 * eps;                                    // (0.5*leapStep)
        double w4[4], u2[4];
        LmcTraj T;
        T.lp = lp;
        T.delta = 0.0;
        glm_load<1>(a, p, a.st.x, T.x);
        {
            LmcGeom o;
            lmc_geom(a, p, S, T.x, pGc, piGc, o);                       // ERMLMC.jl:73-79
            const bool badv = lmc_velocity(p, S, d, rs, chain, (uint32_t)i, T.v);   // ERMLMC.jl:103
            T.dead = o.bad || badv;
            T.ld = o.ld;
            f64x4 gs[1];
            glm_load4<1>(a, p, a.st.g, gs);                             // the state's gradient, bit for bit
            T.g = gs[0];
#pragma unroll
            for (int e = 0; e < 4; ++e) T.dphi[e] = (-T.g[e]) + 0.5 * o.tr[e];
        }
        smm_load_w(Wc, pGc, ld, nr, p.q, 1.0);
        smm_wave_sync();
        rm_symv(p, Wc, V0, d, T.v, w4);
        const double quad0 = glm_sum(a, p, none, rm_dot_part(p, d, T.v, w4));
        const double E = SEMI ? ((-lp) + T.ld) + 0.5 * quad0 : ((-lp) - T.ld) + 0.5 * quad0;   // RMLMC.jl:110, ERMLMC.jl:105
        int nl_wg;                                                      // the workgroup's longest trajectory
        const int nrl = rm_leaps(iscr, rs.block(chain, (uint32_t)i, 0u, TAG_LMC), tn.nl_fixed, p.live, nl_wg);   // ERMLMC.jl:112
        n_evals += nrl;
        for (int l = 0; l < nl_wg; ++l) {
            const bool on = l < nrl;                                    // chains that finished keep still
            if (!SEMI) {
#pragma unroll 1
                for (int hs = 0; hs < 2; ++hs) {                        // ERMLMC.jl:116-126, 141-151
                    double rhs[4];
                    smm_load_w(Wc, pGc, ld, nr, p.q, 1.0);
                    smm_wave_sync();
                    rm_symv(p, Wc, V0, d, T.v, w4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) rhs[e] = w4[e] - hc * T.dphi[e];
#pragma unroll 1
                    for (int sg = 0; sg < 2; ++sg) {
                        smm_pass<false, false, true>(a, p, S, T.x, T.v, w4, u2);
                        const double ldA = lmc_factor(Wc, pGc, ld, d, nr, p.q, sg == 0 ? hc * 0.5 : -(hc * 0.5));
                        if (sg == 0) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) S.vb[16 * (4 * p.q + e) + p.cl] = rhs[e];
                            smm_wave_sync();
                            double v1[4];
                            smm_solve(Wc, S.vb + p.cl, S.Y + p.lane, d, p.q, v1);
                            smm_wave_sync();
                            if (rm_take(on, T.dead, !(ldA == ldA) || smm_not_finite(v1))) {
                                T.delta = T.delta - 2.0 * ldA;
#pragma unroll
                                for (int e = 0; e < 4; ++e) T.v[e] = v1[e];
                            }
                        } else if (rm_take(on, T.dead, !(ldA == ldA))) {
                            T.delta = T.delta + 2.0 * ldA;
                        }
                    }
                    if (hs == 0) lmc_move(a, p, S, pGc, piGc, eps, on, T);
                }
            } else {
                double lv[4], lvin[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) lv[e] = lvin[e] = T.v[e];
                smm_load_w(Wc, piGc, ld, nr, p.q, 1.0);
                smm_wave_sync();
                for (int k = 0; k < nn; ++k) {                          // RMLMC.jl:122-127
#pragma unroll
                    for (int e = 0; e < 4; ++e) lvin[e] = lv[e];
                    smm_pass<false, true, false>(a, p, S, T.x, lv, w4, u2);
                    lmc_kick(p, Wc, V0, d, hc, u2, on, T, lv);
                }
                if (on && !T.dead) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) T.v[e] = lv[e];         // RMLMC.jl:128
                }
#pragma unroll 1
                for (int sg = 0; sg < 2; ++sg) {
                    // sg 0: vxC of the last pass's input iterate (RMLMC.jl:131); sg 1: of the velocity (RMLMC.jl:146-149)
                    double gv[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) gv[e] = sg == 0 ? lvin[e] : T.v[e];
                    smm_pass<false, true, true>(a, p, S, T.x, gv, w4, u2);
                    const double ldA = lmc_factor(Wc, pGc, ld, d, nr, p.q, sg == 0 ? eps * 0.5 : -(eps * 0.5));
                    if (rm_take(on, T.dead, !(ldA == ldA))) T.delta = sg == 0 ? T.delta - 2.0 * ldA : T.delta + 2.0 * ldA;
                    if (sg == 0) lmc_move(a, p, S, pGc, piGc, eps, on, T);
                }
                smm_load_w(Wc, piGc, ld, nr, p.q, 1.0);
                smm_wave_sync();
                lmc_kick(p, Wc, V0, d, hc, u2, on, T, T.v);             // RMLMC.jl:151
            }
        }
        smm_load_w(Wc, pGc, ld, nr, p.q, 1.0);
        smm_wave_sync();
        rm_symv(p, Wc, V0, d, T.v, w4);
        const double quadp = glm_sum(a, p, none, rm_dot_part(p, d, T.v, w4));
        const double Ep = SEMI ? ((-T.lp) + T.ld) + 0.5 * quadp : ((-T.lp) - T.ld) + 0.5 * quadp;   // RMLMC.jl:155, ERMLMC.jl:155
        const double ratio = (E - Ep) + T.delta;                        // ERMLMC.jl:158
        const bool acc = !T.dead && nrl > 0 && (ratio - ratio == 0.0) && glm_mh_short_circuit(rs, chain, (uint32_t)i, ratio);
        if (acc) {
            lp = T.lp;
            if (tuned) tn.n_acc += 1;
        }
        f64x4 go[1] = {T.g};
        smm_commit(a, p, i, acc, T.x, go);
        rm_tuner_adapt(a, i, tn);                                       // ERMLMC.jl:170-176 (EmpiricalHMCTune)
        smm_mem_sync();                                                // the state the next step's lanes read
    }
    rm_write_back(a, p, lp, tn);
    glm_count_evals(a, p, n_evals);
}

}  // namespace mcmc

hipError_t mcmc_launch_lmc_step(const mcmc::KernelArgs& k, hipStream_t st) {
    using namespace mcmc;
    const bool semi = k.sa.kind == SK_RMLMC;
    if (k.s.d > kSmMaxD || (k.sa.kind != SK_ERMLMC && !semi) || (semi && k.sa.n_newton < 1) ||
        k.st.sm_pG == nullptr || k.st.sm_pinvG == nullptr || (k.m.kind != MK_LOGISTIC && k.m.kind != MK_PROBIT))
        return hipErrorInvalidValue;
    return semi ? smm_launch(lmc_step<true>, "lmc_step<rmlmc>", kRmLdsDoubles, k, st)
                : smm_launch(lmc_step<false>, "lmc_step<ermlmc>", kRmLdsDoubles, k, st);
}
