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
// The pass over the tiles, evalallt, the small algebra and the step body (smm_mala_step, pmala.hip's too) live in
// smm_device.hpp.
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
        const double ldet = smm_factor_invert(Wc, S.Y + p.lane, d, nr, p.q, invG_out + cc, ld, p.live);
        fail = fail || !(ldet == ldet);
        double gv[4] = {g[0][0], g[0][1], g[0][2], g[0][3]};
        smm_put_vec(S.Y, p, gv);
        smm_wave_sync();
        double ft[4];
        smm_symv(Wc, S.Y + p.cl, d, p.q, ft);
        glm_store<1>(a, p, ft_out, a.s.ld, ft);
    }
    if (check && p.live && fail) atomicOr(a.s.err, 1);
}

// SMMALA.jl:72-122: smm_device.hpp's MALA step body without the drift correction
__global__ __launch_bounds__(256) void smm_step(GlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    smm_mala_step<false>(a, smem);
}

}  // namespace mcmc

int mcmc_smmala_max_d() { return mcmc::kSmMaxD; }

hipError_t mcmc_launch_smmala_eval(const mcmc::KernelArgs& k, const double* xin, double* lp, double* g, double* G,
                                   double* invG, double* ft, int check, hipStream_t st) {
    using namespace mcmc;
    if (k.s.d > kSmMaxD) return hipErrorInvalidValue;
    return smm_launch(smm_eval_kernel, nullptr, kSmLdsDoubles, k, st, xin, lp, g, G, invG, ft, check);
}

hipError_t mcmc_launch_smmala_step(const mcmc::KernelArgs& k, hipStream_t st) {
    using namespace mcmc;
    if (k.s.d > kSmMaxD || k.sa.kind != SK_SMMALA) return hipErrorInvalidValue;
    return smm_launch(smm_step, "smm_step", kSmLdsDoubles, k, st);
}
