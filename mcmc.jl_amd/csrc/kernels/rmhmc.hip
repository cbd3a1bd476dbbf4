// rmhmc.hip -- Riemannian manifold HMC on the probit / logistic regression models (src/samplers/RMHMC.jl:53-183,
// statement by statement), d <= 16, on a model with tensor derivatives.
//
// Geometry, log-target, gradient, tensor and the small algebra are smmala.hip's (smm_device.hpp): a wave owns a tile
// of 16 chains, lane (q, cl) chain cl and coordinates 4q + e, four tiles a workgroup share the staged X tiles.
//
// The two tensor-derivative terms never form the slabs of dG (dG_r = X' diag(w o X[:, r]) X, the prior adds nothing):
//   trace(invG dG_r)                 = (X' (w o qf))[r],  qf_o = x_o' invG x_o       (PMALA's U, bit for bit);
//   0.5 p' invG dG_r invG p          = 0.5 (X' (w o t^2))[r],  t = X v,  v = invG p;
// both come from smm_pass (smm_dw_tiles), one pass over the staged X tiles producing either or both from the same eta
// and w.  The step's frame -- tuner registers, leapfrog count, mask, commit -- is smm_device.hpp's, lmc.hip's too.
//
// One step (i the sampler's counter, c the chain):
//   G = evalt(pars), cholG, invG      smm_evalallt at the state's position (lp and grad come out the state's, bit for
//                                     bit), smm_chol, smm_inverse;
//   momentum = cholG' randn           the lower factor times the step's NORMAL blocks: row r the fma chain over c <= r;
//   H                                 ((-lp) + 0.5 ((log 2 + d log pi) + 2 sum log diag cholG)) + (p' (invG p)) / 2, the
//                                     constant as the reference writes it; p' v: the lane's fma chain over its
//                                     coordinates from zero, the quarters as (q0 + q2) + (q1 + q3);
//   timeStep, nRandomLeaps            block (c, i, 0, TAG_RMHMC): nRandomLeaps = ceil(uniform52(w0, w1) nLeaps);
//                                     timeStep = +1 iff bm_radius_u32(w2) cos(2 pi w3 2^-32) > 0.5 (a normal against
//                                     0.5, as written: +1 with probability 0.31), else -1;
//   nRandomLeaps generalised leapfrogs, each nNewton momentum passes (symv, a t^2 pass, the update
//   p + eh ((grad - 0.5 trace) + 0.5 X'(w o t^2)), eh = timeStep (leapStep / 2)), nNewton position passes (evalallt at
//   the iterate, smm_chol, smm_solve, pars + eh (G \ p + invG0 p)), then evalallt, chol, inverse, one pass for both
//   terms and the closing momentum update;
//   proposedH from the last leapfrog's G and invG; accept by glm_mh_short_circuit on H - proposedH.
//
// Barriers.  Every pass over X has workgroup barriers inside, so every wave makes the same passes: 2 at the step's start,
// then per leapfrog 2 nNewton + 2, for the workgroup's longest trajectory (rm_max over its live chains' nRandomLeaps).
// Nothing between the passes depends on a chain's values: a chain that has finished its own trajectory, or whose
// trajectory has failed, keeps still under a mask (its position, momentum and terms are not updated; its evaluations
// repeat at the position it holds, so its invG in the workspace stays that position's).
//
// Failed trajectories.  A log-target that is not finite at any evaluation of the trajectory, a Cholesky pivot <= 0 or
// not finite at any G, a position iterate that is not finite, or a ratio that is not finite rejects the step (the
// reference would throw out of chol); so does a nRandomLeaps draw of 0, which leaves proposedGrad undefined in the
// reference.  No chain carries a NaN forward: x, lp and grad are the state, and only an accepted finite proposal
// replaces them.  tests/rmhmc_oracle.c restates all of it.
#include "smm_device.hpp"

namespace mcmc {

// log 2 and log pi, the nearest doubles (RMHMC.jl:107)
constexpr double kRmLog2 = 0x1.62e42fefa39efp-1;
constexpr double kRmLogPi = 0x1.250d048e7a1bdp+0;

__device__ __forceinline__ double rm_hamiltonian(double lp, double ld, double quad, int d) {
    return ((-lp) + 0.5 * ((kRmLog2 + (double)d * kRmLogPi) + 2.0 * ld)) + quad / 2.0;
}

// RMHMC.jl:89-183, one step per loop pass; the state (pars, logTarget, grad) lives in HBM, sm_pinvG is the inverse's
// way from the lanes that form its columns to the workspace
__global__ __launch_bounds__(256) void rm_step(GlmArgs a) {
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
    double* const piGc = a.st.sm_pinvG + cc;
    double lp = a.st.lp[cc];
    RmTuner tn = rm_tuner_load(a, cc);
    int64_t n_evals = 0;
    for (int t = 0; t < s.nsteps; ++t) {
        const int64_t i = s.step_begin + t;
        if (tuned) tn.n_prop += 1;
        double xp[4], mom[4], tr[4], v[4], u2[4];
        f64x4 gp;
        double ld0;
        bool dead;
        {
            bool oos0;
            f64x4 g0[1];
            glm_load<1>(a, p, a.st.x, xp);
            (void)smm_evalallt(a, p, S, xp, g0, oos0);                  // G = evalt(pars)   RMHMC.jl:100
            ld0 = smm_chol(Wc, d, p.q);                                 // cholG             RMHMC.jl:102
            dead = !(ld0 == ld0);
            double z[4];
            glm_normals<1>(p, rs, chain, (uint32_t)i, d, z);
            smm_put_vec(V0, p, z);
            smm_wave_sync();
            smm_lower_mul(Wc, V0 + p.cl, d, p.q, mom);                  // cholG' z          RMHMC.jl:105
            smm_wave_sync();
            smm_invert(Wc, S.Y + p.lane, d, nr, p.q, piGc, ld, p.live);   // invG            RMHMC.jl:101
            smm_wave_sync();
            f64x4 gs[1];
            glm_load4<1>(a, p, a.st.g, gs);
            gp = gs[0];
        }
        rm_symv(p, Wc, V0, d, mom, v);
        const double H = rm_hamiltonian(lp, ld0, glm_sum(a, p, none, rm_dot_part(p, d, mom, v)), d);   // RMHMC.jl:107
        smm_pass<true, false, false>(a, p, S, xp, xp, tr, u2);          // trace(invG dG_r)   RMHMC.jl:110-114
        const u32x4 w = rs.block(chain, (uint32_t)i, 0u, TAG_RMHMC);
        double eh;
        {
            double sn, cs;
            det_sincos2pi_u32(w.w, sn, cs);
            const double nz = bm_radius_u32(w.z, rad_tab_global()) * cs;
            const double ts = nz > 0.5 ? 1.0 : -1.0;                    // RMHMC.jl:117
            eh = ts * (tn.eps / 2.0);
        }
        int nl_wg;                                                      // the workgroup's longest trajectory
        const int nrl = rm_leaps(iscr, w, tn.nl_fixed, p.live, nl_wg);  // RMHMC.jl:118
        n_evals += nrl;
        double lpp = lp, ldp = ld0;
        for (int l = 0; l < nl_wg; ++l) {
            const bool on = l < nrl;                                    // chains that finished keep still
            double lm[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) lm[e] = mom[e];
            for (int k = 0; k < nn; ++k) {                              // RMHMC.jl:123-129
                rm_symv(p, Wc, V0, d, lm, v);
                double un[4];
                smm_pass<false, true, false>(a, p, S, xp, v, un, u2);
                if (on && !dead) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) lm[e] = mom[e] + eh * ((gp[e] - 0.5 * tr[e]) + 0.5 * u2[e]);
                }
            }
            if (on && !dead) {
#pragma unroll
                for (int e = 0; e < 4; ++e) mom[e] = lm[e];             // RMHMC.jl:131
            }
            double v2[4], lx[4];
            rm_symv(p, Wc, V0, d, mom, v2);                             // RMHMC.jl:132
#pragma unroll
            for (int e = 0; e < 4; ++e) lx[e] = xp[e];
            for (int k = 0; k < nn; ++k) {                              // RMHMC.jl:134-138
                bool oosk;
                f64x4 gk[1];
                (void)smm_evalallt(a, p, S, lx, gk, oosk);
                const double ldk = smm_chol(Wc, d, p.q);
#pragma unroll
                for (int e = 0; e < 4; ++e) S.vb[16 * (4 * p.q + e) + p.cl] = mom[e];
                smm_wave_sync();
                double v1[4];
                smm_solve(Wc, S.vb + p.cl, S.Y + p.lane, d, p.q, v1);   // G \ momentum
                smm_wave_sync();
                double cand[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) cand[e] = xp[e] + eh * (v1[e] + v2[e]);
                const bool badk = oosk || !(ldk == ldk) || smm_not_finite(cand);
                if (rm_take(on, dead, badk)) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) lx[e] = cand[e];
                }
            }
            if (on && !dead) {
#pragma unroll
                for (int e = 0; e < 4; ++e) xp[e] = lx[e];              // RMHMC.jl:140
            }
            {
                bool oosc;
                f64x4 gc[1];
                const double lpc = smm_evalallt(a, p, S, xp, gc, oosc);   // RMHMC.jl:141, 153, 158
                const double ldc = smm_factor_invert(Wc, S.Y + p.lane, d, nr, p.q, piGc, ld, p.live);   // RMHMC.jl:142
                smm_wave_sync();
                if (rm_take(on, dead, oosc || !(ldc == ldc))) {
                    lpp = lpc;
                    ldp = ldc;
                    gp = gc[0];
                }
            }
            rm_symv(p, Wc, V0, d, mom, v);                              // RMHMC.jl:148
            double trn[4];
            smm_pass<true, true, false>(a, p, S, xp, v, trn, u2);       // RMHMC.jl:143-151
            if (on && !dead) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    tr[e] = trn[e];
                    mom[e] = mom[e] + eh * ((gp[e] - 0.5 * tr[e]) + 0.5 * u2[e]);   // RMHMC.jl:154
                }
            }
        }
        rm_symv(p, Wc, V0, d, mom, v);
        const double Hp = rm_hamiltonian(lpp, ldp, glm_sum(a, p, none, rm_dot_part(p, d, mom, v)), d);   // RMHMC.jl:161-162
        const double ratio = H - Hp;                                    // RMHMC.jl:164
        const bool acc = !dead && nrl > 0 && (ratio - ratio == 0.0) && glm_mh_short_circuit(rs, chain, (uint32_t)i, ratio);
        if (acc) {
            lp = lpp;
            if (tuned) tn.n_acc += 1;
        }
        f64x4 go[1] = {gp};
        smm_commit(a, p, i, acc, xp, go);
        rm_tuner_adapt(a, i, tn);                                       // RMHMC.jl:174-180 (EmpiricalHMCTune)
        smm_mem_sync();                                                // the state the next step's lanes read
    }
    rm_write_back(a, p, lp, tn);
    glm_count_evals(a, p, n_evals);
}

}  // namespace mcmc

hipError_t mcmc_launch_rmhmc_step(const mcmc::KernelArgs& k, hipStream_t st) {
    using namespace mcmc;
    if (k.s.d > kSmMaxD || k.sa.kind != SK_RMHMC || k.sa.n_newton < 1 || k.st.sm_pinvG == nullptr ||
        (k.m.kind != MK_LOGISTIC && k.m.kind != MK_PROBIT))
        return hipErrorInvalidValue;
    return smm_launch(rm_step, "rm_step", kRmLdsDoubles, k, st);
}
