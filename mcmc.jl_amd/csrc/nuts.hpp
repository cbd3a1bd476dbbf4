// nuts.hpp -- the No-U-Turn sampler (NUTS.jl:53-183) for the lane-per-chain and two-lanes-per-chain mappings.
//
// The reference's buildTree (NUTS.jl:85-118) is recursive.  Here a doubling of depth j is a walk over its 2^j leaves
// in the order the recursion visits them (each leaf is one leapfrog from the previous one, in the doubling's
// direction), with an explicit stack of the open levels:
//   * after leaf t (0-based) the finished subtree R (level 0: the leaf) climbs: at level k it is the second half when
//     bit k-1 of t is set -- it merges with the parked first half (NUTS.jl:106-113) and climbs on; otherwise it is a
//     first half -- parked when its s holds (the walk goes on to leaf t + 1), passed up unchanged when not
//     (NUTS.jl:100: the level returns at once), so a failed subtree still merges wherever it is a second half;
//   * the U-turn test of a level-k merge (NUTS.jl:112) is between the first leaf of that level-k subtree and the leaf
//     just made: a leaf is saved once, at level ctz(t) (j for t = 0), which is where every enclosing subtree that
//     starts at it finds it (subtree start t0 = t with the low k bits cleared, slot ctz(t0)).
// Registers hold the leaf (x, m), the tree's other edge, the step's sample and R's candidate; the level stack -- per
// level the first leaf's (x, m), the parked half's candidate x and (lp, n, alpha sum, n_alpha) -- lives in a
// per-chain HBM workspace [level][slot][d][ld] (ChainState::nuts_wv / nuts_ws), dead between steps.  The gradient at
// an edge is recomputed when a doubling starts from it (bitwise the value the leapfrog that made it computed).
//
// Draws the reference takes from its sequential generator, as counter-based blocks of (chain, step i):
//   normals          (block b, TAG_NORMAL)  as every sampler; step 0 is the initial epsilon search's momentum
//   slice uniform    (0, TAG_ACCEPT) words 0, 1
//   doubling j       (j, TAG_NUTS_DOUBLING): direction +1 if word 0 is odd, else -1; accept uniform words 2, 3
//   merge            ((l << 5) | k, TAG_NUTS_MERGE) words 0, 1: k the level of the merged subtree, l the leapfrogs of
//                    this step taken so far (<= 1023)
// PairChain: every decision is taken on reduced sums and on uniforms both lanes draw alike, so the two lanes of a
// chain stay on one path; each lane keeps its own copy of the level scalars (a lane reads only what it wrote).
#pragma once
#include "samplers.hpp"

namespace mcmc {

constexpr int kNutsMaxDoublings = 10;      // levels of the workspace; 1 + 2 + ... + 2^9 = 1023 leapfrogs a step
constexpr int kNutsWsVec = 3;              // vector slots per level: first leaf x, first leaf m, parked candidate x
constexpr int kNutsWsScal = 4;             // scalar slots per level: parked candidate lp, n, alpha sum, n_alpha
constexpr int kNutsInitCap = 2048;         // passes of the initial epsilon search (never binds, see nuts_init_body)

// one leapfrog of step ve from (x, m) (HMC.jl:93-102); returns H, lp the log-target at the new point
template <class P, class M>
__device__ __forceinline__ double nuts_leapfrog(const P& p, const M& model, double ve, double (&x)[P::NC],
                                                double (&m)[P::NC], double& lp) {
    {
        const GradAt<M, P::NC> g0(model, x);                    // the state's gradient (in support)
#pragma unroll
        for (int k = 0; k < P::NC; ++k) {
            m[k] = m[k] + (0.5 * g0(k, x[k])) * ve;             // n.m += 0.5*n.grad*ve
            x[k] = x[k] + ve * m[k];                            // n.pars += ve * n.m
        }
    }
    bool oos;
    lp = eval_lp(p, model, x, oos);                             // calc!(n, ll)
    const GradAt<M, P::NC> g1(model, x, !oos);
#pragma unroll
    for (int k = 0; k < P::NC; ++k) {
        const double g = oos ? 0.0 : g1(k, x[k]);
        m[k] = m[k] + (0.5 * g) * ve;                           // n.m += 0.5*n.grad*ve
    }
    return -lp + half_dot(p, m);                                // update!(n)
}

// uturn(minus, plus) (NUTS.jl:50) of the edges A = (xa, ma), B = (xb, mb), B the one further along direction dir
template <class P>
__device__ __forceinline__ bool nuts_uturn(const P& p, const double (&xa)[P::NC], const double (&ma)[P::NC],
                                           const double (&xb)[P::NC], const double (&mb)[P::NC], bool fwd) {
    double da = 0.0, db = 0.0;
#pragma unroll
    for (int k = 0; k < P::NC; ++k)
        if (p.valid(k)) {
            const double dx = fwd ? xb[k] - xa[k] : xa[k] - xb[k];      // plus.pars - minus.pars
            da = __builtin_fma(dx, ma[k], da);
            db = __builtin_fma(dx, mb[k], db);
        }
    da = p.reduce(da);
    db = p.reduce(db);
    return da < 0.0 || db < 0.0;
}

// the chain's workspace: vector slot (level, q) as a state-layout array [d][ld]; scalar slot (level, q) of this lane
template <class P>
struct NutsWs {
    double* wv;
    double* ws;
    int64_t ld;
    int d;
    size_t sidx, lds;
    __device__ NutsWs(const P& p, const KernelArgs& a) : wv(a.st.nuts_wv), ws(a.st.nuts_ws), ld(a.s.ld), d(a.s.d) {
        lds = (size_t)(P::kPairs ? 2 : 1) * (size_t)ld;
        size_t h = 0;
        if constexpr (P::kPairs) h = (size_t)p.h;
        sidx = (size_t)(p.live ? p.c : 0) + h * (size_t)ld;
    }
    __device__ __forceinline__ double* vec(int level, int q) const {
        return wv + (size_t)(level * kNutsWsVec + q) * (size_t)d * (size_t)ld;
    }
    __device__ __forceinline__ double& scal(int level, int q) const {
        return ws[(size_t)(level * kNutsWsScal + q) * lds + sidx];
    }
};

// ------------------------------------------------------------------ initial epsilon (NUTS.jl:71-82, 127-129)
// After the chains' initial evaluation: m = randn .* scale (the normals of step 0), epsilon doubled or halved from 1
// until the one-leapfrog acceptance ratio crosses 0.5; mu = log(10 epsilon), hbar = 0, log epsilon_bar = 0.
template <class P, class M>
__device__ __forceinline__ void nuts_init_body(const KernelArgs& a) {
    const StepArgs& s = a.s;
    const P p(s);
    const M model(a.m);
    const Stream rs{s.key0, s.key1};
    const uint32_t chain = s.chain0 + (uint32_t)p.c;
    constexpr int NC = P::NC;
    double x0[NC], m0[NC];
    p.load(a.st.x, s.ld, x0);
    const double lp0 = p.load_scalar(a.st.lp);
    int64_t n_evals = 0;
    if (p.live) {
        gen_normals(p, rs, chain, 0u, m0);
#pragma unroll
        for (int k = 0; k < NC; ++k) m0[k] = p.valid(k) ? m0[k] * s.scale[p.coord(k)] : 0.0;
        const double H0 = -lp0 + half_dot(p, m0);
        double eps = 1.0;
        auto ratio_at = [&](double e) {
            double x[NC], m[NC], lp1;
#pragma unroll
            for (int k = 0; k < NC; ++k) { x[k] = x0[k]; m[k] = m0[k]; }
            const double H1 = nuts_leapfrog(p, model, e, x, m, lp1);
            n_evals += 1;
            return det_exp(H0 - H1);
        };
        double ratio = ratio_at(eps);
        const bool up = ratio > 0.5;                            // a = 2*(ratio>0.5)-1
        // ratio^a > 2^-a.  The loop ends by IEEE arithmetic within about 1 100 passes (epsilon overflows and the ratio
        // turns NaN or 0, or epsilon underflows to 0 and the ratio is 1); the cap never binds.
        for (int it = 0; it < kNutsInitCap && (up ? ratio > 0.5 : 1.0 / ratio > 2.0); ++it) {
            eps = eps * (up ? 2.0 : 0.5);                       // epsilon *= 2^a
            ratio = ratio_at(eps);
        }
        p.store_t(a.st.t_step, eps);
        p.store_t(a.st.t_mu, det_log(10.0 * eps));
        p.store_t(a.st.t_h, 0.0);
        p.store_t(a.st.t_bar, 0.0);
    }
    p.count_evals(s, n_evals);
}

// ------------------------------------------------------------------ the step loop (NUTS.jl:134-181)
template <class P, class M>
__device__ __forceinline__ void nuts_body(const KernelArgs& a) {
    const StepArgs& s = a.s;
    const P p(s);
    const M model(a.m);
    const Stream rs{s.key0, s.key1};
    const uint32_t chain = s.chain0 + (uint32_t)p.c;
    constexpr int NC = P::NC;
    const int maxd = (int)a.sa.n_leaps;                         // maxdoublings
    const NutsWs<P> ws(p, a);
    // adaptation constants (NUTS.jl:121-125)
    const double delta = 0.7, gam = 0.05, kappa = 0.75;
    const int64_t nadapt = 1000, t0 = 10;

    double xs[NC], sc[NC];
    p.load(a.st.x, s.ld, xs);
    double lps = p.load_scalar(a.st.lp);
    double eps = p.load_scalar(a.st.t_step);
    double hbar = p.load_scalar(a.st.t_h);
    double lebar = p.load_scalar(a.st.t_bar);
    const double mu = p.load_scalar(a.st.t_mu);
#pragma unroll
    for (int k = 0; k < NC; ++k) sc[k] = p.valid(k) ? s.scale[p.coord(k)] : 0.0;

    int64_t n_evals = 0;
    Keeper keep(s);
    if (p.live) {
        for (int t = 0; t < s.nsteps; ++t) {
            const int64_t i = s.step_begin + t;
            const uint32_t si = (uint32_t)i;
            double x[NC], m[NC], xo[NC], mo[NC], xc[NC];        // leaf, other edge, subtree candidate
            gen_normals(p, rs, chain, si, m);
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                m[k] = m[k] * sc[k];                            // state0.m = randn(model.size) .* scale
                x[k] = xs[k];
                xo[k] = xs[k];
                mo[k] = m[k];
            }
            const double H0 = -lps + half_dot(p, m);            // update!(state0)
            const u32x4 wa = rs.block(chain, si, 0u, TAG_ACCEPT);
            const double u_slice = det_log(uniform52(wa.x, wa.y)) - H0;
            bool leaf_fwd = true;                               // the leaf registers hold the plus edge
            bool ok = true, accepted = false;
            int j = 0, n = 1;
            uint32_t nleap = 0;
            double alpha = 0.0;
            int nalpha = 1;
            double lpc = lps;
            while (ok && j < maxd) {
                const u32x4 wd = rs.block(chain, si, (uint32_t)j, TAG_NUTS_DOUBLING);
                const bool fwd = (wd.x & 1u) != 0u;             // dir = randbool() ? 1 : -1
                const double ud = uniform52(wd.z, wd.w);
                if (fwd != leaf_fwd) {                          // walk from the other edge
#pragma unroll
                    for (int k = 0; k < NC; ++k) {
                        const double tx = x[k], tm = m[k];
                        x[k] = xo[k]; m[k] = mo[k];
                        xo[k] = tx; mo[k] = tm;
                    }
                    leaf_fwd = fwd;
                }
                const double ve = fwd ? eps : -eps;             // dir*epsilon
                // ---- buildTree(edge, dir, j) (NUTS.jl:85-118), iteratively
                int nR = 0, naR = 1;
                bool sR = true;
                double aR = 0.0;
                const int nleaf = 1 << j;
                for (int tl = 0; tl < nleaf; ++tl) {
                    double lp1;
                    const double H1 = nuts_leapfrog(p, model, ve, x, m, lp1);
                    nleap += 1;
                    nR = (u_slice <= -H1) ? 1 : 0;              // NUTS.jl:94
                    sR = u_slice < (100.0 - H1);                // NUTS.jl:95, deltamax = 100
                    aR = __builtin_fmin(1.0, det_exp(H0 - H1));
                    naR = 1;
                    lpc = lp1;
#pragma unroll
                    for (int k = 0; k < NC; ++k) xc[k] = x[k];
                    if ((tl & 1) == 0 && j >= 1) {              // the first leaf of the subtrees that start here
                        const int lvl = tl == 0 ? j : __builtin_ctz((unsigned)tl);
                        p.store(ws.vec(lvl, 0), s.ld, x);
                        p.store(ws.vec(lvl, 1), s.ld, m);
                    }
                    int k = 1;
                    for (; k <= j; ++k) {
                        if ((tl >> (k - 1)) & 1) {              // second half of level k: merge (NUTS.jl:106-113)
                            const double lpL = ws.scal(k, 0);
                            const int nL = (int)ws.scal(k, 1);
                            const double aL = ws.scal(k, 2);
                            const int naL = (int)ws.scal(k, 3);
                            const u32x4 wm = rs.block(chain, si, (nleap << 5) | (uint32_t)k, TAG_NUTS_MERGE);
                            const double um = uniform52(wm.x, wm.y);
                            const bool take2 = um <= (double)nR / (double)(nR + nL);   // 0/0: NaN, false
                            if (!take2) {
                                p.load(ws.vec(k, 2), s.ld, xc);
                                lpc = lpL;
                            }
                            aR = aL + aR;                       // alpha1 += alpha2
                            naR = naL + naR;
                            const int t0l = tl & ~((1 << k) - 1);
                            const int lvl = t0l == 0 ? j : __builtin_ctz((unsigned)t0l);
                            double xf[NC], mf[NC];
                            p.load(ws.vec(lvl, 0), s.ld, xf);
                            p.load(ws.vec(lvl, 1), s.ld, mf);
                            const bool ut = nuts_uturn(p, xf, mf, x, m, fwd);
                            sR = sR && !ut;                     // s1 = s2 && !uturn(state_minus, state_plus)
                            nR = nL + nR;
                        } else if (sR) {                        // first half of level k: park it, next leaf
                            p.store(ws.vec(k, 2), s.ld, xc);
                            ws.scal(k, 0) = lpc;
                            ws.scal(k, 1) = (double)nR;
                            ws.scal(k, 2) = aR;
                            ws.scal(k, 3) = (double)naR;
                            break;
                        }                                       // a failed first half returns at once (NUTS.jl:100)
                    }
                    if (k > j) break;                           // the depth-j subtree is complete
                }
                // ---- NUTS.jl:157-162
                if (sR && ud < (double)nR / (double)n) {
#pragma unroll
                    for (int k = 0; k < NC; ++k) xs[k] = xc[k];
                    lps = lpc;
                    accepted = true;
                }
                n += nR;
                j += 1;
                alpha = aR;
                nalpha = naR;
                ok = sR && !nuts_uturn(p, xo, mo, x, m, fwd);
            }
            n_evals += (int64_t)nleap;
            // ---- epsilon adjustment (NUTS.jl:166-173)
            if (i <= nadapt) {
                const double di = (double)i, dit = (double)(i + t0);
                hbar = hbar * (1.0 - 1.0 / dit) + (delta - alpha / (double)nalpha) / dit;
                const double le = mu - __builtin_sqrt(di) / gam * hbar;
                const double ik = det_exp(det_log(di) * (-kappa));             // i^(-kappa)
                lebar = ik * le + (1.0 - ik) * lebar;
                eps = det_exp(le);
            } else {
                eps = det_exp(lebar);
            }
            int64_t kk;
            if (keep.take(i, &kk)) {
                p.store_kept(s, kk, xs, s.samples);
                if (s.grads != nullptr) {
                    const bool oos = M::kLLAcc && !(lps - lps == 0.0);
                    double g[NC];
                    const GradAt<M, NC> gk(model, xs, !oos);
#pragma unroll
                    for (int k = 0; k < NC; ++k) g[k] = oos ? 0.0 : gk(k, xs[k]);
                    p.store_kept(s, kk, g, s.grads);
                }
                p.store_bit(s, kk, accepted);
                if (s.nuts_eps != nullptr) p.store_t(s.nuts_eps + (size_t)kk * (size_t)s.C, eps);
                if (s.nuts_nd != nullptr) p.store_t(s.nuts_nd + (size_t)kk * (size_t)s.C, (int32_t)j);
            }
        }
        p.store(a.st.x, s.ld, xs);
        p.store_t(a.st.lp, lps);
        p.store_t(a.st.t_step, eps);
        p.store_t(a.st.t_h, hbar);
        p.store_t(a.st.t_bar, lebar);
    }
    p.count_evals(s, n_evals);
}

}  // namespace mcmc
