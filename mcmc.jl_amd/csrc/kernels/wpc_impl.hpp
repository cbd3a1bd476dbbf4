// wpc_impl.hpp -- wave-per-chain kernels (32 < d <= 2048): one wave = one chain (4 chains per 256-thread
// block), and block-per-chain kernels (2048 < d <= 16384): W = 4 or 8 waves = one chain; see samplers.hpp for
// the step code and its reference lines.  Included by one translation unit per model (wpc_<model>.hip); wpc.hip
// looks the model's unit up.  Which instance a launch runs is launch_plan.hpp's.
#pragma once
#include "../samplers.hpp"
#include "layout_api.hpp"

namespace mcmc {

constexpr int kChainsPerBlock = kBlock / 64;

// F: d == 256 NB (WaveChain FULL).  The Box-Muller tables: from LDS for NB >= 4 (two waves per SIMD anyway by their
// registers, so two 56 KB blocks per CU cost nothing; config 4 is NB = 4), from global memory for NB <= 2 (three or
// four waves per SIMD, which 56 KB blocks would cut to two)
template <int NB>
constexpr int wpc_tab() { return NB >= 4 ? kTabLds : kTabGlobal; }
template <int NB, bool F, class M>
__global__ __launch_bounds__(kBlock) void wpc_rwm(KernelArgs a) { rwm_body<WaveChain<NB, F, 1, wpc_tab<NB>()>, M>(a); }
template <int NB, bool F, class M>
__global__ __launch_bounds__(kBlock) void wpc_mala(KernelArgs a) { mala_body<WaveChain<NB, F, 1, wpc_tab<NB>()>, M>(a); }
template <int NB, bool F, class M, bool DA>
__global__ __launch_bounds__(kBlock) void wpc_hmc(KernelArgs a) {
    hmc_body<WaveChain<NB, F, 1, wpc_tab<NB>()>, M, DA>(a);
}
template <int NB, class M>
__global__ __launch_bounds__(kBlock) void wpc_eval(KernelArgs a, const double* xin, double* lp, double* g,
                                                   int32_t check) {
    eval_body<WaveChain<NB>, M>(a, xin, lp, g, check);
}

// block per chain, d > 2048: W waves hold the chain's coordinates (WaveChain<8, false, W>), one chain per block
template <int W, class M>
__global__ __launch_bounds__(64 * W) void bpc_rwm(KernelArgs a) { rwm_body<WaveChain<8, false, W, kTabLds>, M>(a); }
template <int W, class M>
__global__ __launch_bounds__(64 * W) void bpc_mala(KernelArgs a) { mala_body<WaveChain<8, false, W, kTabLds>, M>(a); }
template <int W, class M, bool DA>
__global__ __launch_bounds__(64 * W) void bpc_hmc(KernelArgs a) { hmc_body<WaveChain<8, false, W, kTabLds>, M, DA>(a); }
template <int W, class M>
__global__ __launch_bounds__(64 * W) void bpc_eval(KernelArgs a, const double* xin, double* lp, double* g,
                                                   int32_t check) {
    eval_body<WaveChain<8, false, W>, M>(a, xin, lp, g, check);
}
template <int W, class M, bool DA>
__global__ __launch_bounds__(64 * W) void bpc_hmc_rec(KernelArgs a, LeapRec r) {
    hmc_record_body<WaveChain<8, false, W>, M, DA>(a, r);
}
// storeLeaps records (samplers.hpp hmc_record_body), generic mapping only: a diagnostic
template <int NB, class M, bool DA>
__global__ __launch_bounds__(kBlock) void wpc_hmc_rec(KernelArgs a, LeapRec r) { hmc_record_body<WaveChain<NB>, M, DA>(a, r); }

// ------------------------------------------------------------------ launchers
// Each launches the instance the plan names (layout_api.hpp for_int / for_bool / launch_inst; launch_plan.hpp
// inst(map, body, n, threads, F, US, DA) restates it beside the kernel): W in {4, 8}, NB in {1, 2, 4, 8}; F is out of
// reach at compile time on a model without FULL instances.
template <class M, int32_t MK>
static hipError_t wpc_step(const KernelArgs& a, const LaunchPlan& p, hipStream_t st) {
    constexpr bool FULL = unit_model<M, MK>().full_wave;
    const KernelInstance& k = p.k;
    const hipError_t e = for_bools(k.F, k.US, k.DA, [&](auto f, auto us, auto da) {
        constexpr bool F = decltype(f)::value, US = decltype(us)::value, DA = decltype(da)::value;
        if constexpr (US || (F && !FULL)) return hipErrorInvalidValue;           // no wave kernel has a US instance
        else if (k.map == MAP_BPC)
            return for_int<4, 8>(k.n, [&](auto w) {
                constexpr int W = decltype(w)::value, T = 64 * W;
                switch (k.body) {
                    case B_RWM: return launch_inst(p, inst(MAP_BPC, B_RWM, W, T, F, US, DA), bpc_rwm<W, M>, st, a);
                    case B_MALA: return launch_inst(p, inst(MAP_BPC, B_MALA, W, T, F, US, DA), bpc_mala<W, M>, st, a);
                    case B_HMC: return launch_inst(p, inst(MAP_BPC, B_HMC, W, T, F, US, DA), bpc_hmc<W, M, DA>, st, a);
                    default: return hipErrorInvalidValue;
                }
            });
        else
            return for_int<1, 2, 4, 8>(k.n, [&](auto nb) {
                constexpr int NB = decltype(nb)::value, T = kBlock;
                switch (k.body) {
                    case B_RWM: return launch_inst(p, inst(MAP_WPC, B_RWM, NB, T, F, US, DA), wpc_rwm<NB, F, M>, st, a);
                    case B_MALA:
                        return launch_inst(p, inst(MAP_WPC, B_MALA, NB, T, F, US, DA), wpc_mala<NB, F, M>, st, a);
                    case B_HMC:
                        return launch_inst(p, inst(MAP_WPC, B_HMC, NB, T, F, US, DA), wpc_hmc<NB, F, M, DA>, st, a);
                    default: return hipErrorInvalidValue;
                }
            });
    });
    return note_launched(e, p, M::kName);
}

template <class M>
static hipError_t wpc_eval_m(const KernelArgs& a, const LaunchPlan& p, const double* xin, double* lp, double* g,
                             int check, hipStream_t st) {
    if (p.k.map == MAP_BPC)
        return for_int<4, 8>(p.k.n, [&](auto w) {
            constexpr int W = decltype(w)::value;
            return launch_inst(p, inst(MAP_BPC, B_EVAL, W, 64 * W), bpc_eval<W, M>, st, a, xin, lp, g, check);
        });
    return for_int<1, 2, 4, 8>(p.k.n, [&](auto nb) {
        constexpr int NB = decltype(nb)::value;
        return launch_inst(p, inst(MAP_WPC, B_EVAL, NB, kBlock), wpc_eval<NB, M>, st, a, xin, lp, g, check);
    });
}

template <class M>
static hipError_t wpc_record_m(const KernelArgs& a, const LaunchPlan& p, const LeapRec& r, hipStream_t st) {
    return for_bool(p.k.DA, [&](auto da) {
        constexpr bool DA = decltype(da)::value;
        if (p.k.map == MAP_BPC)
            return for_int<4, 8>(p.k.n, [&](auto w) {
                constexpr int W = decltype(w)::value;
                return launch_inst(p, inst(MAP_BPC, B_HMC_REC, W, 64 * W, false, false, DA),
                                   bpc_hmc_rec<W, M, DA>, st, a, r);
            });
        return for_int<1, 2, 4, 8>(p.k.n, [&](auto nb) {
            constexpr int NB = decltype(nb)::value;
            return launch_inst(p, inst(MAP_WPC, B_HMC_REC, NB, kBlock, false, false, DA),
                               wpc_hmc_rec<NB, M, DA>, st, a, r);
        });
    });
}

}  // namespace mcmc

// one translation unit per model: WPC_UNIT(iso, IsoDot, MK_ISO) defines the unit mcmc::wpc_iso (layout_api.hpp)
#define WPC_UNIT(name, Model, MK)                                                                        \
    mcmc::KernelUnit mcmc::wpc_##name() {                                                                \
        return {wpc_step<Model, MK>, wpc_eval_m<Model>, wpc_record_m<Model>};                            \
    }

