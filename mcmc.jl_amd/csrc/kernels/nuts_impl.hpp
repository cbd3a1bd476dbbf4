// nuts_impl.hpp -- NUTS kernels (nuts.hpp) for the lane-per-chain (d <= 16) and two-lanes-per-chain (16 < d <= 32)
// mappings.  Included by one translation unit per model (nuts_<model>.hip); nuts.hip dispatches on the model kind.
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

// MAXNB: the widest instance built for the model (joint models run lane per chain, d <= 16; the catalogue's two
// are d = 1 and d = 3)
template <class M, int MAXNB>
static hipError_t nuts_launch(const KernelArgs& a, bool init, hipStream_t st) {
    const int nb = (a.s.d + 3) / 4;
    if (nb < 1 || nb > MAXNB) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.s.C + kBlock - 1) / kBlock));
    const dim3 grid2((unsigned)((a.s.C + kBlock / 2 - 1) / (kBlock / 2)));       // PairChain: 128 chains a block
#define NUTS_LPC(NB)                                                                  \
    case NB:                                                                          \
        if constexpr (NB <= MAXNB) {                                                  \
            if (init) lpc_nuts_init<NB, M><<<grid, kBlock, 0, st>>>(a);               \
            else {                                                                    \
                mcmc_note_step_kernel("lpc_nuts<%d, %s>", NB, M::kName);              \
                lpc_nuts<NB, M><<<grid, kBlock, 0, st>>>(a);                          \
            }                                                                         \
        }                                                                             \
        break;
#define NUTS_LPP(NB, NBL)                                                             \
    case NB:                                                                          \
        if constexpr (NB <= MAXNB) {                                                  \
            if (init) lpp_nuts_init<NBL, M><<<grid2, kBlock, 0, st>>>(a);             \
            else {                                                                    \
                mcmc_note_step_kernel("lpp_nuts<%d, %s>", NBL, M::kName);             \
                lpp_nuts<NBL, M><<<grid2, kBlock, 0, st>>>(a);                        \
            }                                                                         \
        }                                                                             \
        break;
    switch (nb) {
        NUTS_LPC(1) NUTS_LPC(2) NUTS_LPC(3) NUTS_LPC(4) NUTS_LPP(5, 3) NUTS_LPP(6, 3) NUTS_LPP(7, 4) NUTS_LPP(8, 4)
        default: return hipErrorInvalidValue;
    }
#undef NUTS_LPC
#undef NUTS_LPP
    return hipGetLastError();
}

}  // namespace mcmc

// one translation unit per model: NUTS_UNIT(iso, IsoDot, 8) defines mcmc_nuts_iso
#define NUTS_UNIT(name, Model, MAXNB)                                                       \
    hipError_t mcmc_nuts_##name(const mcmc::KernelArgs& a, int init, hipStream_t st) {      \
        return mcmc::nuts_launch<mcmc::Model, MAXNB>(a, init != 0, st);                     \
    }
