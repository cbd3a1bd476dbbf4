// slice_impl.hpp -- the reference's slice sampler (src/samplers/slice_sample.jl:43-103: Neal's univariate-at-a-time
// slice sampler with stepping out and shrinkage) for the lane-per-chain (d <= 16) and two-lanes-per-chain
// (16 < d <= 32) mappings.  Included by one translation unit per model (slice_<model>.hip); slice.hip looks the
// model's unit up.  256-thread blocks, no normals (so no Box-Muller tables), no LDS and no barrier.
//
// One launch runs whole iterations.  x[NC], log_Px and info live in registers for the launch; the coordinate being
// updated is substituted in place in x (its value before the update, state[dd], is kept beside it), so x_l, x_r and
// xprime are scalars, not the reference's three vector copies.
//
// Draw k of the update (iter, dd) is uniform52 of words (w0, w1) (k even) or (w2, w3) (k odd) of the Philox block
// (global chain id, iter, (dd << 20) | (k >> 1), TAG_SLICE): k = 0 is the slice level's uniform, k = 1 the interval
// position r, k >= 2 shrink proposal k - 2.
//
// Divergence: the reference's three consecutive while loops (step out left, step out right, shrink) would make a wave
// pay the maximum over its lanes three times per coordinate.  The update is one loop with one evaluation site and a
// per-lane phase; the wave runs the maximum over its lanes of the *total* evaluations of the update.  The draws are
// keyed by counters, so the order in which lanes reach their draws changes nothing.
//
// Departures from the reference, which would loop without end or assert:
//  * every coordinate update may spend max_evals evaluations (stepping out and shrinking together).  A chain whose
//    update is not finished after that many, or whose proposal equals state[dd] and still is not acceptable (the
//    reference's "BUG" assert, slice_sample.jl:92), stops: info = the iteration (counted from the call's iter_begin,
//    1-based; saturated at INT32_MAX), its state stays the last completed iteration's, its history rows from that
//    iteration on are NaN, and it idles under the mask from then on;
//  * a start whose log-density is not finite is refused by the host (MCMC_E_INIT_OUT_OF_SUPPORT).
#pragma once
#include "../samplers.hpp"
#include "layout_api.hpp"

namespace mcmc {

constexpr uint32_t TAG_SLICE = 9u;

enum SlicePhase : int { PH_LEFT = 0, PH_RIGHT = 1, PH_SHRINK = 2, PH_DONE = 3 };

// x[k] for a wave-uniform k
template <int NC>
__device__ __forceinline__ double slice_get(const double (&x)[NC], int k) {
    // (each element passes through an empty asm: the bare chain of selects is folded into one load at a variable
    // index, which sends x to scratch or LDS)
    double v = x[0];
#pragma unroll
    for (int j = 1; j < NC; ++j) {
        double xj = x[j];
        asm("" : "+v"(xj));
        if (k == j) v = xj;
    }
    return v;
}
// x[k] = v in the lanes that own the coordinate, for a wave-uniform k: a scalar branch to one move, not NC selects
template <int NC>
__device__ __forceinline__ void slice_set(double (&x)[NC], int k, double v, bool owner) {
    // (the empty asm keeps each test a branch: without it the chain is if-converted into two v_cndmask per coordinate
    // per evaluation, twice the work of IsoDot's fma; a switch has its stores sunk into one with a variable index,
    // which sends x to scratch)
#pragma unroll
    for (int j = 0; j < NC; ++j)
        if (k == j) {
            asm volatile("");
            x[j] = owner ? v : x[j];
        }
}

template <class P, class M>
__device__ __forceinline__ void slice_body(const SliceKernelArgs& a) {
    const SliceArgs& s = a.s;
    constexpr int NC = P::NC;
    StepArgs sa{};                                              // what the mapping reads of a step launch
    sa.C = s.C;
    sa.ld = s.ld;
    sa.d = s.d;
    sa.n_evals = s.n_evals;
    const P p(sa);
    const M model(a.m);
    const Stream rs{s.key0, s.key1};
    const uint32_t chain = s.chain0 + (uint32_t)p.c;
    double x[NC];
    p.load(s.x, s.ld, x);
    double lp = p.load_scalar(s.lp);
    int32_t info = p.load_t(s.info);
    if (!p.live) info = 1;                                      // lanes past the batch idle; nothing of theirs is stored
    int64_t nev = 0;
    const int32_t max_evals = s.max_evals;

    for (int t = 0; t < s.niters; ++t) {
        const int64_t iter = s.iter_first + t;
        bool ok = info == 0;
        for (int dd = 0; dd < s.d; ++dd) {
            // the lanes that hold coordinate dd, and where
            const int oh = P::kPairs && dd >= NC ? 1 : 0;
            const int kl = dd - oh * NC;
            bool owner = true;
            double xc = slice_get(x, kl);                       // state[dd]
            if constexpr (P::kPairs) {
                double v0, v1;
                p.halves(xc, v0, v1);
                xc = oh ? v1 : v0;
                owner = p.h == oh;
            }
            const u32x4 w0 = rs.block(chain, (uint32_t)iter, (uint32_t)dd << 20, TAG_SLICE);
            const double lup = det_log(uniform52(w0.x, w0.y)) + lp;     // log_uprime (slice_sample.jl:63)
            const double r = uniform52(w0.z, w0.w);
            const double wd = s.widths[dd];
            double xl = xc - r * wd;                            // :69
            double xr = xc + (1.0 - r) * wd;                    // :70
            int phase = !ok ? PH_DONE : s.step_out ? PH_LEFT : PH_SHRINK;
            uint32_t k = 2u, cz = 0u, cw = 0u;
            int32_t ne = 0;
            double xp = xc;
            while (phase != PH_DONE) {
                double xe;
                if (phase == PH_SHRINK) {
                    uint32_t ua, ub;
                    if ((k & 1u) == 0u) {
                        const u32x4 w = rs.block(chain, (uint32_t)iter, ((uint32_t)dd << 20) | (k >> 1), TAG_SLICE);
                        ua = w.x; ub = w.y; cz = w.z; cw = w.w;
                    } else {
                        ua = cz; ub = cw;
                    }
                    k += 1u;
                    xp = uniform52(ua, ub) * (xr - xl) + xl;    // :82
                    xe = xp;
                } else {
                    xe = phase == PH_LEFT ? xl : xr;
                }
                slice_set(x, kl, xe, owner);
                bool oos;
                const double lpe = eval_lp(p, model, x, oos);   // the one evaluation site
                ne += 1;
                const bool above = lpe > lup;
                if (phase == PH_LEFT) {                         // :72-74
                    if (above) xl = xl - wd;
                    else phase = PH_RIGHT;
                } else if (phase == PH_RIGHT) {                 // :75-77
                    if (above) xr = xr + wd;
                    else phase = PH_SHRINK;
                } else {                                        // :83-94
                    lp = lpe;
                    if (above) phase = PH_DONE;
                    else if (xp > xc) xr = xp;
                    else if (xp < xc) xl = xp;
                    else { ok = false; phase = PH_DONE; }
                }
                if (phase != PH_DONE && ne >= max_evals) { ok = false; phase = PH_DONE; }
            }
            nev += ne;
        }
        if (ok) {
            p.store(s.x, s.ld, x);
            p.store_t(s.lp, lp);
        } else if (info == 0) {
            const int64_t at = iter - s.iter_begin;
            info = at > 0x7fffffffLL ? 0x7fffffff : (int32_t)at;
        }
        if (s.samples != nullptr && iter > s.keep_after) {
            double row[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) row[j] = ok ? x[j] : __builtin_nan("");
            p.store_kept(sa, iter - s.keep_after - 1, row, s.samples);
        }
    }
    p.store_t(s.info, info);
    p.count_evals(sa, nev);                                     // once per wave, at the end of the launch
}

template <int NB, class M>
__global__ __launch_bounds__(kPlanBlock) void lpc_slice(SliceKernelArgs a) {
    slice_body<LaneChain<NB, false, false, kPlanBlock, kTabGlobal>, M>(a);
}
template <int NBL, class M>
__global__ __launch_bounds__(kPlanBlock) void lpp_slice(SliceKernelArgs a) {
    slice_body<PairChain<NBL, false, kPlanBlock, kTabGlobal>, M>(a);
}

// MAXNB, the model's row: the widest instance built (the joint models run lane per chain at their catalogue sizes)
template <class M, int32_t MK>
static hipError_t slice_launch(const SliceKernelArgs& a, const LaunchPlan& p, hipStream_t st) {
    constexpr int MAXNB = unit_model<M, MK>().nuts_max_nb;
    const KernelInstance& k = p.k;
    if (k.body != B_SLICE) return hipErrorInvalidValue;
    const hipError_t e =
        k.map == MAP_LPC
            ? for_int<1, 2, 3, 4>(k.n, [&](auto nb) {
                  constexpr int NB = decltype(nb)::value;
                  if constexpr (NB > MAXNB) return hipErrorInvalidValue;
                  else return launch_inst(p, inst(MAP_LPC, B_SLICE, NB, kPlanBlock), lpc_slice<NB, M>, st, a);
              })
            : for_int<3, 4>(k.n, [&](auto nbl) {
                  constexpr int NBL = decltype(nbl)::value;
                  if constexpr (2 * NBL - 1 > MAXNB) return hipErrorInvalidValue;   // NBL serves NB = 2 NBL - 1, 2 NBL
                  else return launch_inst(p, inst(MAP_LPP, B_SLICE, NBL, kPlanBlock), lpp_slice<NBL, M>, st, a);
              });
    return note_launched(e, p, M::kName);
}

}  // namespace mcmc

// one translation unit per model: SLICE_UNIT(iso, IsoDot, MK_ISO) defines the launcher mcmc::slice_iso (layout_api.hpp)
#define SLICE_UNIT(name, Model, MK)                                                                          \
    hipError_t mcmc::slice_##name(const SliceKernelArgs& a, const LaunchPlan& p, hipStream_t st) {           \
        return slice_launch<Model, MK>(a, p, st);                                                            \
    }
