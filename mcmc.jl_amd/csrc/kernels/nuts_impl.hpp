// nuts_impl.hpp -- NUTS kernels (nuts.hpp) for the lane-per-chain (d <= 16) and two-lanes-per-chain (16 < d <= 32)
// mappings.  Included by one translation unit per model (nuts_<model>.hip); nuts.hip looks the model's unit up.
// 256-thread blocks, the Box-Muller tables read from global memory (one draw of normals per step, against up to 1 023
// leapfrogs), no LDS and no barrier: the chains of a wave walk trees of different depth.
#pragma once
#include "../nuts.hpp"
#include "layout_api.hpp"

namespace mcmc {

template <int NB, class M>
__global__ __launch_bounds__(kBlock) void lpc_nuts(KernelArgs a) {
    nuts_body<LaneChain<NB, false, false, kBlock, kTabGlobal>, M>(a);
}
template <int NB, class M>
__global__ __launch_bounds__(kBlock) void lpc_nuts_init(KernelArgs a) {
    nuts_init_body<LaneChain<NB, false, false, kBlock, kTabGlobal>, M>(a);
}
template <int NBL, class M>
__global__ __launch_bounds__(kBlock) void lpp_nuts(KernelArgs a) {
    nuts_body<PairChain<NBL, false, kBlock, kTabGlobal>, M>(a);
}
template <int NBL, class M>
__global__ __launch_bounds__(kBlock) void lpp_nuts_init(KernelArgs a) {
    nuts_init_body<PairChain<NBL, false, kBlock, kTabGlobal>, M>(a);
}

// The step loop or the initial epsilon search, as the plan's body says.  MAXNB, the model's row: the widest instance
// built (joint models run lane per chain, d <= 16); wider ones are out of reach at compile time.
template <class M, int32_t MK>
static hipError_t nuts_launch(const KernelArgs& a, const LaunchPlan& p, hipStream_t st) {
    constexpr int MAXNB = unit_model<M, MK>().nuts_max_nb;
    const KernelInstance& k = p.k;
    if (k.body != B_NUTS && k.body != B_NUTS_INIT) return hipErrorInvalidValue;
    const bool init = k.body == B_NUTS_INIT;
    const hipError_t e =
        k.map == MAP_LPC
            ? for_int<1, 2, 3, 4>(k.n, [&](auto nb) {
                  constexpr int NB = decltype(nb)::value;
                  if constexpr (NB > MAXNB) return hipErrorInvalidValue;
                  else
                      return launch_inst(p, inst(MAP_LPC, k.body, NB, kBlock),
                                         init ? lpc_nuts_init<NB, M> : lpc_nuts<NB, M>, st, a);
              })
            : for_int<3, 4>(k.n, [&](auto nbl) {
                  constexpr int NBL = decltype(nbl)::value;
                  if constexpr (2 * NBL - 1 > MAXNB) return hipErrorInvalidValue;   // NBL serves NB = 2 NBL - 1, 2 NBL
                  else
                      return launch_inst(p, inst(MAP_LPP, k.body, NBL, kBlock),
                                         init ? lpp_nuts_init<NBL, M> : lpp_nuts<NBL, M>, st, a);
              });
    return init ? e : note_launched(e, p, M::kName);              // the epsilon search is no step kernel
}

}  // namespace mcmc

// one translation unit per model: NUTS_UNIT(iso, IsoDot, MK_ISO) defines the unit mcmc::nuts_iso (layout_api.hpp)
#define NUTS_UNIT(name, Model, MK) \
    mcmc::KernelUnit mcmc::nuts_##name() { return {nuts_launch<Model, MK>, nullptr, nullptr}; }
