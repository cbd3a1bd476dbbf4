// glm.hip -- regression models on fp64 MFMA: logistic (examples/logistic_regression.jl:16-22)
// and linear (examples/linear_regression.jl:14-20) log-targets with their gradients, fused into
// the RWM / MALA / HMC / HMCDA step loops.
//
// Mapping.  A wave owns a tile of 16 chains; the dense contractions are
//     eta[obs][chain] = X[obs][:] . beta[:][chain]        (v_mfma_f64_16x16x4_f64, K = coordinates)
//     G[coord][chain] = X[:][coord] . r[:][chain]          (same instruction, K = observations)
// per 16-observation tile of X staged in LDS and shared by the workgroup's waves.  Lane l holds
// chain cl = l & 15 and quarter q = l >> 4; for d-slice s (d > 64 is split over NW = d_pad/64
// waves) it owns coordinates k = s*DS + 16m + 4q + e (m < DS/16, e < 4), which are exactly the four
// normals of Philox blocks k/4 -- so proposals, momenta, gradients and every per-coordinate term
// stay lane-local.  The MFMA row <-> coordinate maps are permuted to make that so:
//     eta k-slice kk (= 4m + e), row q      <-> coordinate 16m + 4q + e
//     G tile T, row i (= 4r + q')           <-> coordinate 16T + 4q' + r
// and the eta accumulator (obs q + 4r on lane (q, cl)) is, register for register, the B operand
// of the G product (k-slice r): no data movement between the two MFMA chains.
//
// Arithmetic (restated by oracle/oracle.c orc_glm_eval): v_mfma_f64_16x16x4_f64 is a
// sequential fma chain over its k (probed bitwise on gfx950, scripts/probe_mfma.py), so eta is an
// fma chain over coordinates in (m, e, q) order per slice, slices added left to right; G is an fma
// chain over observations; per-coordinate sums are lane partials in (m, e) order combined as
// (q0 + q2) + (q1 + q3), then slices left to right.
//
// This unit: the evaluation kernel, the step kernels other than the wave-specialised single-slice MALA
// (glm_mala1ws.hip), the storeLeaps record kernel, the geometry (mcmc_glm_shape), the image packer and the launchers.
// The evaluation and everything the kernels share is glm_device.hpp.
#include <type_traits>

#include "../ram.hpp"
#include "glm_device.hpp"

namespace mcmc {

// ------------------------------------------------------------------ kernels
template <int NM, int NW>
__global__ __launch_bounds__(glm_block<NW>()) void glm_eval_kernel(GlmArgs a, const double* xin, double* lp_out,
                                                             double* g_out, int32_t check) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const GlmPos p = glm_pos(a);
    const GlmLds L = glm_lds(a, smem);
    double x[(4 * NM)];
    f64x4 g[NM];
    glm_load_all<NM>(a, p, xin, x);
    bool oos;
    const double lp = glm_eval<NM, NW, true>(a, p, L, x, g, oos);
    if (p.live && p.q == 0 && p.slice == 0) lp_out[p.c] = lp;
    if (g_out) glm_store4<NM>(a, p, g_out, a.s.ld, g);
    if (check && p.live && !(lp - lp == 0.0)) atomicOr(a.s.err, 1);
}

template <int NM, int NW>
__global__ __launch_bounds__(glm_block<NW>()) void glm_rwm(GlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const StepArgs& s = a.s;
    const GlmPos p = glm_pos(a);
    const GlmLds L = glm_lds(a, smem);
    const Stream rs{s.key0, s.key1};
    const uint32_t chain = s.chain0 + (uint32_t)p.c;
    f64x4 dummy[NM];
    const double* scl = s.scale + p.base + 4 * p.q;
    double lp = a.st.lp[p.live ? p.c : 0];
    for (int t = 0; t < s.nsteps; ++t) {
        const int64_t i = s.step_begin + t;
        double xp[(4 * NM)];
        {
            double x[(4 * NM)];
            glm_load<NM>(a, p, a.st.x, x);
            glm_normals<NM>(p, rs, chain, (uint32_t)i, a.s.d, xp);
#pragma unroll
            for (int slot = 0; slot < (4 * NM); ++slot)                         // RWM.jl:59
                xp[slot] = x[slot] + xp[slot] * (glm_valid(a, p, slot) ? scl[16 * (slot >> 2) + (slot & 3)] : 0.0);
        }
        bool oos;
        const double lpp = glm_eval<NM, NW, false>(a, p, L, xp, dummy, oos);
        const bool acc = glm_mh_short_circuit(rs, chain, (uint32_t)i, lpp - lp);
        if (acc) {
            glm_store<NM>(a, p, a.st.x, s.ld, xp);
            lp = lpp;
        }
        int64_t kk;
        if (kept_index(i - s.run_step0, s.burnin, s.thinning, s.len, &kk)) {
            if (!acc) glm_load<NM>(a, p, a.st.x, xp);
            glm_store_kept<NM>(a, p, kk, s.samples, xp);
            glm_store_bit(a, p, kk, acc);
        }
    }
    if (p.live && p.q == 0 && p.slice == 0) a.st.lp[p.c] = lp;
    glm_count_evals(a, p, s.nsteps);
}

// RAM (RAM.jl:55-78) for d <= 32 (one d-slice, NW = 1), the factor padded to DF = 16 NM (ram.hpp).
// Row r of S belongs to the lane that owns coordinate r (own_coord): it forms u[r] = (S z)[r] from the
// full normal vector (every lane of the chain draws all DF/4 blocks), keeps it across the evaluation,
// and after the accept updates its rows of every column k; the pivot u[k] comes from its owner by a
// cross-lane read.  Rows r <= k of a column compute throw-away values whose stores go to the trash row
// of the tile (index ram_rows(DF)), so the loop carries no branches.
template <int NM, int NW>
__global__ __launch_bounds__(glm_block<NW>()) void glm_ram(GlmArgs a) {
    static_assert(NW == 1, "RAM on regression targets is built for d <= 32");
    constexpr int DF = 16 * NM;
    constexpr int NS = 4 * NM;                                          // own coordinates per lane
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const StepArgs& s = a.s;
    const GlmPos p = glm_pos(a);
    const GlmLds L = glm_lds(a, smem);
    const Stream rs{s.key0, s.key1};
    const uint32_t chain = s.chain0 + (uint32_t)p.c;
    f64x4 dummy[NM];
    // the wave's 16 chains lie in one 64-chain tile of the factor store (ram.hpp layout; padding chains past
    // the last one), addressed through buffer resources: lane offset lo, own row r's base rowb[slot]
    const uint32_t rtile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * a.g.tpw + p.tile) >> 2));
    double* const T0 = a.st.ram_L + (uint64_t)rtile * (uint64_t)ram_tile_doubles(DF);
    const uint64_t ld = (uint64_t)a.st.ram_ld;
    const uint32_t lo = (uint32_t)(p.c & 63) * 8;
    uint32_t rowb[NS];
#pragma unroll
    for (int slot = 0; slot < NS; ++slot) {
        const int r = own_coord(p, slot);
        rowb[slot] = lo + (uint32_t)(r * (r + 1) / 2) * 512;
    }
    const int d = s.d;
    double lp = a.st.lp[p.live ? p.c : 0];
    for (int t = 0; t < s.nsteps; ++t) {
        const int64_t i = s.step_begin + t;
        double xp[NS], u[NS], nz = 0.0;
        {
            double z[DF];
#pragma unroll
            for (int b = 0; b < DF / 4; ++b) {                                  // rvec = randn(d)
                const u32x4 w = rs.block(chain, (uint32_t)i, (uint32_t)b, TAG_NORMAL);
                normals4(w, z[4 * b], z[4 * b + 1], z[4 * b + 2], z[4 * b + 3]);
            }
#pragma unroll
            for (int k = 0; k < DF; ++k) {
                if (k >= d) z[k] = 0.0;                                         // padding: identity block
                nz = __builtin_fma(z[k], z[k], nz);                             // dot(rvec, rvec)
            }
            double x[NS];
            glm_load<NM>(a, p, a.st.x, x);
            const ram_rsrc_t Rs = ram_tile_rsrc<DF>(ram_half<DF>(T0, i - 1, ld));
#pragma unroll
            for (int slot = 0; slot < NS; ++slot) {
                // own row r: the fma chain over c <= r, then exact no-ops fma(0, z, acc)
                const int r = own_coord(p, slot);
                double acc = 0.0;
#pragma unroll
                for (int c = 0; c < DF; ++c) {
                    const double v = ram_tload(Rs, rowb[slot], c);            // row r(r+1)/2 + c (in the tile)
                    acc = __builtin_fma(c <= r ? v : 0.0, z[c], acc);
                }
                u[slot] = acc;
                xp[slot] = x[slot] + acc;                                     // RAM.jl:60
                __builtin_amdgcn_sched_barrier(0);                            // one row's loads at a time
            }
        }
        bool oos;
        const double lpp = glm_eval<NM, NW, false>(a, p, L, xp, dummy, oos);
        const double ratio = lpp - lp;
        const bool acc = glm_mh_short_circuit(rs, chain, (uint32_t)i, ratio);
        if (acc) {
            glm_store<NM>(a, p, a.st.x, s.ld, xp);
            lp = lpp;
        }
        int64_t kk;
        if (kept_index(i - s.run_step0, s.burnin, s.thinning, s.len, &kk)) {
            if (!acc) glm_load<NM>(a, p, a.st.x, xp);
            glm_store_kept<NM>(a, p, kk, s.samples, xp);
            glm_store_bit(a, p, kk, acc);
        }
        // S <- chol(S S' + beta u u')' (ram.hpp ram_update, distributed over the chain's four lanes)
        const double beta = ram_alpha(i, d, ratio, a.sa.rate) / nz;
        const bool up = beta >= 0.0;
        const double sb = __builtin_sqrt(__builtin_fabs(beta));
#pragma unroll
        for (int slot = 0; slot < NS; ++slot) u[slot] = sb * u[slot];
        const ram_rsrc_t Rs = ram_tile_rsrc<DF>(ram_half<DF>(T0, i - 1, ld));
        const ram_rsrc_t Rd = ram_tile_rsrc<DF>(ram_half<DF>(T0, i, ld));
#pragma unroll
        for (int k = 0; k < DF; ++k) {
            const int kslot = 4 * (k >> 4) + (k & 3);                           // owner: q = (k & 15) >> 2
            const double xk = __shfl(u[kslot], p.cl + 16 * ((k & 15) >> 2), 64);
            const double lkk = ram_tload(Rs, lo, k * (k + 1) / 2 + k);
            const double t2 = xk * xk;
            const double l2 = lkk * lkk;
            const double r = __builtin_sqrt(up ? l2 + t2 : l2 - t2);
            const double cc = r / lkk;
            const double sn = xk / lkk;
            const double sns = up ? sn : -sn;                                   // as ram.hpp ram_update
            const double ic = 1.0 / cc;
            ram_tstore(Rd, lo, k * (k + 1) / 2 + k, r);
#pragma unroll
            for (int slot = 0; slot < NS; ++slot) {
                const int q = own_coord(p, slot);
                if (16 * (slot >> 2) + 12 + (slot & 3) <= k) continue;          // no row of this slot is below k
                const bool below = q > k;
                const double l0 = ram_tload(Rs, rowb[slot], k);                // in bounds for q <= k too
                const double l = (l0 + sns * u[slot]) * ic;
                // rows q <= k store to the tile's trash row (index ram_rows(DF))
                ram_tstore(Rd, below ? rowb[slot] : lo + (uint32_t)(ram_rows(DF) - k) * 512, k, l);
                const double un = cc * u[slot] - sn * l;
                u[slot] = below ? un : u[slot];
            }
            __builtin_amdgcn_sched_barrier(0);                                  // one column's loads at a time
        }
    }
    if (p.live && p.q == 0 && p.slice == 0) a.st.lp[p.c] = lp;
    glm_count_evals(a, p, s.nsteps);
}

template <int NM, int NW>
__global__ __launch_bounds__(glm_block<NW>()) void glm_mala(GlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const StepArgs& s = a.s;
    const SamplerArgs& sa = a.sa;
    const GlmPos p = glm_pos(a);
    const GlmLds L = glm_lds(a, smem);
    const Stream rs{s.key0, s.key1};
    const uint32_t chain = s.chain0 + (uint32_t)p.c;
    const int64_t cc = p.live ? p.c : 0;
    double lp = a.st.lp[cc];
    double h = sa.tuner ? a.st.t_step[cc] : sa.drift_step;
    int32_t n_acc = sa.tuner ? a.st.t_acc[cc] : 0;
    int32_t n_prop = sa.tuner ? a.st.t_prop[cc] : 0;
    for (int t = 0; t < s.nsteps; ++t) {
        const int64_t i = s.step_begin + t;
        if (sa.tuner) n_prop += 1;
        const double half = h / 2.0;
        const double sq = __builtin_sqrt(h);
        const double twoh = 2.0 * h;
        const double Lc = det_log(kTwoPi * h) / 2.0;
        double xp[(4 * NM)];
        f64x4 gp[NM];
        double qf = 0.0;
        {
            double x[(4 * NM)];                                        // state, reloaded after eval
            glm_normals<NM>(p, rs, chain, (uint32_t)i, a.s.d, xp);
            glm_load<NM>(a, p, a.st.x, x);
            glm_load4<NM>(a, p, a.st.g, gp);                           // current gradient (state)
#pragma unroll
            for (int slot = 0; slot < (4 * NM); ++slot) {
                const double pm = x[slot] + half * gp[slot >> 2][slot & 3];   // MALA.jl:98
                xp[slot] = pm + sq * xp[slot];                                 // MALA.jl:100
                const double e = pm - xp[slot];
                if (glm_valid(a, p, slot)) qf = qf + ((-(e * e)) / twoh - Lc);   // MALA.jl:103
            }
        }
        qf = glm_sum(a, p, L, qf);
        bool oos;
        const double lpp = glm_eval<NM, NW, true>(a, p, L, xp, gp, oos);    // MALA.jl:101
        double qb = 0.0;
        {
            double x[(4 * NM)];
            glm_load<NM>(a, p, a.st.x, x);
#pragma unroll
            for (int slot = 0; slot < (4 * NM); ++slot) {
                const double e = (xp[slot] + half * gp[slot >> 2][slot & 3]) - x[slot];   // MALA.jl:104-105
                if (glm_valid(a, p, slot)) qb = qb + ((-(e * e)) / twoh - Lc);
            }
        }
        qb = glm_sum(a, p, L, qb);
        const double ratio = ((lpp + qb) - lp) - qf;                   // MALA.jl:107
        const bool acc = glm_mh_short_circuit(rs, chain, (uint32_t)i, ratio);
        if (acc) {
            glm_store<NM>(a, p, a.st.x, s.ld, xp);
            glm_store4<NM>(a, p, a.st.g, s.ld, gp);
            lp = lpp;
            if (sa.tuner) n_acc += 1;
        }
        int64_t kk;
        if (kept_index(i - s.run_step0, s.burnin, s.thinning, s.len, &kk)) {
            if (!acc) {
                glm_load<NM>(a, p, a.st.x, xp);
                glm_load4<NM>(a, p, a.st.g, gp);
            }
            glm_store_kept<NM>(a, p, kk, s.samples, xp);
            glm_store_kept4<NM>(a, p, kk, s.grads, gp);
            glm_store_bit(a, p, kk, acc);
        }
        if (sa.tuner && i <= s.tuner_burnin && (i % sa.adapt_step) == 0) {   // MALA.jl:116-118
            h = h * glm_tune_factor(n_acc, n_prop, sa.target_rate);
            n_acc = 0;
            n_prop = 0;
        }
    }
    if (p.live && p.q == 0 && p.slice == 0) {
        a.st.lp[p.c] = lp;
        if (sa.tuner) {
            a.st.t_step[p.c] = h;
            a.st.t_acc[p.c] = n_acc;
            a.st.t_prop[p.c] = n_prop;
        }
    }
    glm_count_evals(a, p, s.nsteps);
}

// storeLeaps: leap l's state into the record, [l][d][C] and [l][C] (HMC.jl:145-150)
template <int NM>
__device__ __forceinline__ void glm_rec_put(const GlmArgs& a, const GlmPos& p, int64_t l, const double (&x)[4 * NM],
                                            const f64x4 (&g)[NM], const double (&m)[4 * NM], double lpv, double Hv) {
    if (l > a.rec.cap) return;
    glm_store_kept<NM>(a, p, l, a.rec.pars, x);
    glm_store_kept4<NM>(a, p, l, a.rec.grads, g);
    glm_store_kept<NM>(a, p, l, a.rec.mom, m);
    if (p.live && p.q == 0 && p.slice == 0) {
        a.rec.lp[(size_t)l * (size_t)a.s.C + (size_t)p.c] = lpv;
        a.rec.H[(size_t)l * (size_t)a.s.C + (size_t)p.c] = Hv;
    }
}

// REC: record the trajectory of the launch's single step (storeLeaps) and leave the chains where they are
template <int NM, int NW, bool DA, bool REC = false>
__global__ __launch_bounds__(glm_block<NW>()) void glm_hmc(GlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const StepArgs& s = a.s;
    const SamplerArgs& sa = a.sa;
    const GlmPos p = glm_pos(a);
    const GlmLds L = glm_lds(a, smem);
    const Stream rs{s.key0, s.key1};
    const uint32_t chain = s.chain0 + (uint32_t)p.c;
    const int64_t cc = p.live ? p.c : 0;
    const bool tuned = !DA && sa.tuner;
    const int64_t max_leaps = sa.max_leaps;
    double lp = a.st.lp[cc];
    double eps = (DA || tuned) ? a.st.t_step[cc] : sa.leap_step;
    int64_t nl_fixed = tuned ? (int64_t)a.st.t_leaps[cc] : sa.n_leaps;
    double eps_bar = DA ? a.st.t_bar[cc] : 0.0;
    double h_bar = DA ? a.st.t_h[cc] : 0.0;
    int32_t n_acc = tuned ? a.st.t_acc[cc] : 0;
    int32_t n_prop = tuned ? a.st.t_prop[cc] : 0;
    const double mu = DA ? det_log(10.0) : 0.0;
    int64_t n_evals = 0;
    for (int t = 0; t < s.nsteps; ++t) {
        const int64_t i = s.step_begin + t;
        if (tuned) n_prop += 1;
        double x[(4 * NM)], m[(4 * NM)];
        f64x4 g[NM];
        glm_normals<NM>(p, rs, chain, (uint32_t)i, a.s.d, m);          // state0.m = randn(model.size)
        double mm = 0.0;
#pragma unroll
        for (int slot = 0; slot < (4 * NM); ++slot)
            if (glm_valid(a, p, slot)) mm = __builtin_fma(m[slot], m[slot], mm);
        const double H0 = -lp + 0.5 * glm_sum(a, p, L, mm);         // update!(state0)
        glm_load<NM>(a, p, a.st.x, x);
        glm_load4<NM>(a, p, a.st.g, g);
        if (REC) glm_rec_put<NM>(a, p, 0, x, g, m, lp, H0);             // leapStates[1] = deepcopy(state0)
        int64_t nl;
        if (DA) {
            const double r = round_away(sa.len / eps);              // HMCDA.jl:104
            nl = r < 1.0 ? 1 : (r > (double)max_leaps ? max_leaps : (int64_t)r);
        } else {
            nl = nl_fixed;
        }
        n_evals += nl;
        // the workgroup runs its longest trajectory; a d-sliced chain tile whose chains have all finished theirs
        // stops computing (glm_eval on = false: it takes its share of the staging and the barriers, and keeps its
        // last evaluation, made at the same x), so the other tile's waves have the SIMDs to themselves
        int64_t nl_tile = nl;
        constexpr bool kTileSkip = NW > 1 && NW < 8;                 // two chain tiles a workgroup
        const int64_t nl_wg = (DA || tuned) ? (kTileSkip ? glm_max_tile(L, nl, p.live, p.tile, nl_tile) : glm_max(L, nl, p.live))
                                            : nl;
        if (!(kTileSkip && (DA || tuned))) nl_tile = nl_wg;
        double lpl = lp;
        for (int64_t l = 0; l < nl_wg; ++l) {
            const bool active = l < nl;                              // chains that finished keep still
            if (active) {
#pragma unroll
                for (int slot = 0; slot < (4 * NM); ++slot) {
                    m[slot] = m[slot] + (0.5 * g[slot >> 2][slot & 3]) * eps;   // n.m += 0.5*n.grad*ve
                    x[slot] = x[slot] + eps * m[slot];                          // n.pars += ve * n.m
                }
            }
            bool oos;
            // d-slices: the momentum waits in HBM while the evaluation runs (its 4 NM doubles a lane would otherwise
            // be spilled inside the tile loop at the 256-register budget); plain stores and loads, bitwise the same
            constexpr bool kPark = NW > 1 && !REC;
            if (kPark && p.live) {
                double* mp = glm_lane_ptr(p, a.st.mom, s.ld, p.c);
#pragma unroll
                for (int slot = 0; slot < (4 * NM); ++slot) mp[(size_t)(16 * (slot >> 2) + (slot & 3)) * (size_t)s.ld] = m[slot];
            }
            const bool tile_on = l < nl_tile;                                // wave-uniform
            const double lpe = glm_eval<NM, NW, true>(a, p, L, x, g, oos, tile_on);   // calc!(n, ll); same x -> same (lp, g)
            if (tile_on) lpl = lpe;
            if (kPark) {
                const double* mp = glm_lane_ptr(p, a.st.mom, s.ld, p.live ? p.c : 0);
#pragma unroll
                for (int slot = 0; slot < (4 * NM); ++slot) m[slot] = mp[(size_t)(16 * (slot >> 2) + (slot & 3)) * (size_t)s.ld];
            }
            if (active) {
#pragma unroll
                for (int slot = 0; slot < (4 * NM); ++slot) m[slot] = m[slot] + (0.5 * g[slot >> 2][slot & 3]) * eps;
            }
            if (REC) {
                double m2 = 0.0;
#pragma unroll
                for (int slot = 0; slot < (4 * NM); ++slot)
                    if (glm_valid(a, p, slot)) m2 = __builtin_fma(m[slot], m[slot], m2);
                const double Hl = -lpl + 0.5 * glm_sum(a, p, L, m2);      // update!(n): every wave reaches it
                if (active) glm_rec_put<NM>(a, p, l + 1, x, g, m, lpl, Hl);
            }
        }
        if (REC) {                                                       // uniform: every wave returns here
            if (p.live && p.q == 0 && p.slice == 0) a.rec.nl[p.c] = (int32_t)nl;
            return;
        }
        mm = 0.0;
#pragma unroll
        for (int slot = 0; slot < (4 * NM); ++slot)
            if (glm_valid(a, p, slot)) mm = __builtin_fma(m[slot], m[slot], mm);
        const double H = -lpl + 0.5 * glm_sum(a, p, L, mm);
        const u32x4 w = rs.block(chain, (uint32_t)i, 0u, TAG_ACCEPT);
        const double u = uniform52(w.x, w.y);
        double pa = 0.0;
        bool acc;
        if (DA) {
            pa = __builtin_fmin(1.0, det_exp(H0 - H));              // HMCDA.jl:120
            acc = u < pa;
        } else {
            acc = u < det_exp(H0 - H);                              // HMC.jl:154
        }
        if (acc) {
            glm_store<NM>(a, p, a.st.x, s.ld, x);
            glm_store4<NM>(a, p, a.st.g, s.ld, g);
            lp = lpl;
            if (tuned) n_acc += 1;
        }
        int64_t kk;
        if (kept_index(i - s.run_step0, s.burnin, s.thinning, s.len, &kk)) {
            if (!acc) {
                glm_load<NM>(a, p, a.st.x, x);
                glm_load4<NM>(a, p, a.st.g, g);
            }
            glm_store_kept<NM>(a, p, kk, s.samples, x);
            glm_store_kept4<NM>(a, p, kk, s.grads, g);
            glm_store_bit(a, p, kk, acc);
        }
        if (DA) {
            const double di = (double)i;
            if (di < (double)s.tuner_burnin) {                      // HMCDA.jl:133-138
                double eta = 1.0 / (di + sa.t0);
                h_bar = (1.0 - eta) * h_bar + eta * (sa.rate - pa);
                eps = det_exp(mu - (__builtin_sqrt(di) * h_bar) / sa.shrinkage);
                eta = det_exp(det_log(di) * (-sa.step));
                eps_bar = det_exp((1.0 - eta) * det_log(eps_bar) + eta * det_log(eps));
            } else {
                eps = eps_bar;
            }
        } else if (tuned && i <= s.tuner_burnin && (i % sa.adapt_step) == 0) {
            eps = eps * glm_tune_factor(n_acc, n_prop, sa.target_rate);
            double nlf = __builtin_ceil(sa.target_path / eps);
            if (nlf > (double)sa.max_step) nlf = (double)sa.max_step;
            if (nlf > (double)max_leaps) nlf = (double)max_leaps;
            nl_fixed = (int64_t)nlf;
            n_acc = 0;
            n_prop = 0;
        }
    }
    if (p.live && p.q == 0 && p.slice == 0) {
        a.st.lp[p.c] = lp;
        if (DA || tuned) a.st.t_step[p.c] = eps;
        if (DA) {
            a.st.t_bar[p.c] = eps_bar;
            a.st.t_h[p.c] = h_bar;
        } else if (tuned) {
            a.st.t_leaps[p.c] = (int32_t)nl_fixed;
            a.st.t_acc[p.c] = n_acc;
            a.st.t_prop[p.c] = n_prop;
        }
    }
    glm_count_evals(a, p, n_evals);
}

}  // namespace mcmc

// ------------------------------------------------------------------ host side
mcmc::GlmShape mcmc_glm_shape(int d, int64_t n) {
    // d <= 128: one wave per 16-chain tile, DS = d_pad = 16 NM (NM a power of two, pipelined glm_eval1), 4 tiles
    // per workgroup;
    // 128 < d <= 256: NW = 4 slices of DS = 64 coordinates (NM = 4), two 16-chain tiles per 8-wave workgroup;
    // 256 < d <= 512: NW = 4 slices of DS = 128 (NM = 8), two tiles per workgroup, so each staged X tile feeds 32
    // chains (round 4: config 5 0.557 -> 0.582 of the fp64 MFMA spec against 64-wide slices on one box; at d = 256
    // 128-wide slices measured 0.30 against 0.53, two waves a tile);
    // 512 < d <= 1024: NW = 8 slices of DS = 128 coordinates (NM = 8), one tile per workgroup; d_pad = 1024 keeps
    // one LDS tile buffer (glm_xbufs).
    // The slice geometry fixes each chain's summation order, so it is a function of d alone, restated by the oracle
    // (orc_glm_geometry); no run-time switch changes it.
    mcmc::GlmShape g{};
    if (d <= 128) {
        int nm = 1;
        while (16 * nm < d) nm *= 2;
        g.nw = 1;
        g.nm = nm;
    } else if (d <= 256) {
        int nw = 4;
        while (64 * nw < d) nw *= 2;
        g.nw = nw;
        g.nm = 4;
    } else {
        int nw = 2;
        while (128 * nw < d) nw *= 2;
        g.nw = nw;
        g.nm = 8;
    }
    g.ds = 16 * g.nm;
    g.d_pad = g.ds * g.nw;
    g.tpw = g.nw == 1 ? 4 : 8 / g.nw;
    g.lds_stride = mcmc::glm_row_stride(g.d_pad);
    g.ts = mcmc::glm_tile_doubles(g.d_pad);
    g.n_pad = (n + 15) / 16 * 16;
    return g;
}

int mcmc_glm_max_d() { return 1024; }

// steps one launch of the regression step kernel may fuse (0: any): the single-slice MALA kernel is a
// one-step kernel (glm_mala1ws)
int mcmc_glm_steps_per_launch(int d, int64_t n, int sampler_kind) {
    const mcmc::GlmShape g = mcmc_glm_shape(d, n);
    return (g.nw == 1 && sampler_kind == mcmc::SK_MALA) ? 1 : 0;
}

int mcmc_glm_d_pad(int d) { return mcmc_glm_shape(d, 1).d_pad; }

int mcmc_glm_tiles_per_wg(int d) { return mcmc_glm_shape(d, 1).tpw; }

size_t mcmc_glm_image_doubles(int d, int64_t n) {
    const mcmc::GlmShape g = mcmc_glm_shape(d, n);
    return (size_t)(g.n_pad / 16) * (size_t)g.ts;
}

// the staged-tile image of X [n][d] (row-major) and Y [n] (glm_layout.hpp): tile t = rows 16t..16t+15 at
// positions glm_pos(k) of stride S, then Y; zeros elsewhere (padded rows, coordinates k >= d, gaps)
void mcmc_glm_pack_image(int d, int64_t n, const double* X, const double* Y, const double* B, double* img) {
    const mcmc::GlmShape g = mcmc_glm_shape(d, n);
    const size_t total = mcmc_glm_image_doubles(d, n);
    for (size_t i = 0; i < total; ++i) img[i] = 0.0;
    const int S = g.lds_stride, YO = mcmc::glm_y_offset(g.d_pad), BO = mcmc::glm_b_offset(g.d_pad);
    for (int64_t i = 0; i < n; ++i) {
        double* tile = img + (size_t)(i / 16) * (size_t)g.ts;
        const int r = (int)(i % 16);
        for (int k = 0; k < d; ++k) tile[r * S + k] = X[(size_t)i * d + k];
        tile[YO + r] = Y[i];
        tile[BO + r] = B ? B[i] : 0.0;
    }
    if (B)
        for (int64_t i = n; i < g.n_pad; ++i) img[(size_t)(i / 16) * (size_t)g.ts + BO + (int)(i % 16)] = -HUGE_VAL;
}

// The (NM, NW) slice geometries mcmc_glm_shape produces: f(NM, NW), both as std::integral_constant, for g's pair
template <class F>
static hipError_t glm_for_shape(const mcmc::GlmShape& g, F f) {
    using c1 = std::integral_constant<int, 1>;
    using c2 = std::integral_constant<int, 2>;
    using c4 = std::integral_constant<int, 4>;
    using c8 = std::integral_constant<int, 8>;
    switch (g.nm * 10 + g.nw) {
        case 11: return f(c1{}, c1{});
        case 21: return f(c2{}, c1{});
        case 41: return f(c4{}, c1{});
        case 81: return f(c8{}, c1{});
        case 44: return f(c4{}, c4{});
        case 48: return f(c4{}, c8{});
        case 82: return f(c8{}, c2{});
        case 84: return f(c8{}, c4{});
        case 88: return f(c8{}, c8{});
        default: return hipErrorInvalidValue;
    }
}

template <int NM, int NW>
static hipError_t glm_step_nm(const mcmc::GlmArgs& a, size_t lds, dim3 grid, hipStream_t st) {
    using namespace mcmc;
    constexpr int B = glm_block<NW>();
    switch (a.sa.kind) {
        case SK_RWM: mcmc_note_step_kernel("glm_rwm<%d, %d>", NM, NW); break;
        case SK_MALA:
            if (NW == 1 && NM == 8 && a.m.prior_sigma == 1.0)
                mcmc_note_step_kernel("glm_mala1ws<%d, true>", NM);          // the unit-prior instance
            else if (NW == 1) mcmc_note_step_kernel("glm_mala1ws<%d>", NM);
            else mcmc_note_step_kernel("glm_mala<%d, %d>", NM, NW);
            break;
        case SK_HMC: mcmc_note_step_kernel("glm_hmc<%d, %d, false>", NM, NW); break;
        case SK_HMCDA: mcmc_note_step_kernel("glm_hmc<%d, %d, true>", NM, NW); break;
        case SK_RAM: mcmc_note_step_kernel("glm_ram<%d, %d>", NM, NW); break;
        default: break;
    }
    switch (a.sa.kind) {
        case SK_RWM: glm_rwm<NM, NW><<<grid, B, lds, st>>>(a); break;
        case SK_MALA:
            if constexpr (NW == 1) return mcmc_launch_glm_mala1ws(a, grid, st);          // glm_mala1ws.hip
            else glm_mala<NM, NW><<<grid, B, lds, st>>>(a);
            break;
        case SK_HMC: glm_hmc<NM, NW, false><<<grid, B, lds, st>>>(a); break;
        case SK_HMCDA: glm_hmc<NM, NW, true><<<grid, B, lds, st>>>(a); break;
        case SK_RAM:
            if constexpr (NW == 1 && NM <= 2) {
                glm_ram<NM, NW><<<grid, B, lds, st>>>(a);
                break;
            }
            return hipErrorInvalidValue;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t mcmc_launch_glm_step(const mcmc::KernelArgs& k, hipStream_t st) {
    using namespace mcmc;
    const GlmShape g = mcmc_glm_shape(k.s.d, k.m.n);
    const GlmArgs a = glm_args(k, g);
    const size_t lds = glm_lds_bytes(g);
    const dim3 grid(glm_grid(k.s.C, g));
    return glm_for_shape(g, [&](auto nm, auto nw) {
        return glm_step_nm<decltype(nm)::value, decltype(nw)::value>(a, lds, grid, st);
    });
}

template <int NM, int NW>
static hipError_t glm_rec_nm(const mcmc::GlmArgs& a, size_t lds, dim3 grid, hipStream_t st) {
    using namespace mcmc;
    constexpr int B = glm_block<NW>();
    if (a.sa.kind == SK_HMCDA) glm_hmc<NM, NW, true, true><<<grid, B, lds, st>>>(a);
    else glm_hmc<NM, NW, false, true><<<grid, B, lds, st>>>(a);
    return hipGetLastError();
}

hipError_t mcmc_launch_glm_record(const mcmc::KernelArgs& k, const mcmc::LeapRec& r, hipStream_t st) {
    using namespace mcmc;
    if (k.sa.kind != SK_HMC && k.sa.kind != SK_HMCDA) return hipErrorInvalidValue;
    const GlmShape g = mcmc_glm_shape(k.s.d, k.m.n);
    GlmArgs a = glm_args(k, g);
    a.rec = r;
    const size_t lds = glm_lds_bytes(g);
    const dim3 grid(glm_grid(k.s.C, g));
    return glm_for_shape(g, [&](auto nm, auto nw) {
        return glm_rec_nm<decltype(nm)::value, decltype(nw)::value>(a, lds, grid, st);
    });
}

hipError_t mcmc_launch_glm_eval(const mcmc::KernelArgs& k, const double* xin, double* lp, double* g, int check,
                                hipStream_t st) {
    using namespace mcmc;
    const GlmShape gs = mcmc_glm_shape(k.s.d, k.m.n);
    const GlmArgs a = glm_args(k, gs);
    const dim3 grid(glm_grid(k.s.C, gs));
    const size_t lds = glm_lds_bytes(gs);
    return glm_for_shape(gs, [&](auto nm, auto nw) {
        constexpr int NM = decltype(nm)::value, NW = decltype(nw)::value;
        glm_eval_kernel<NM, NW><<<grid, glm_block<NW>(), lds, st>>>(a, xin, lp, g, check);
        return hipGetLastError();
    });
}
