// wpc_ram.hip -- wave-per-chain RAM kernels (src/samplers/RAM.jl:41-79) for 32 < d <= 1024, every separable
// model kind: ram_wave.hpp ram_wave_body over the wave layout of the jump factor (two chains per wave up to d = 256,
// one beyond).
#include "wpc_impl.hpp"
#include "../ram_wave.hpp"

namespace mcmc {

template <int G, class M>
__global__ __launch_bounds__(kBlock) void wpc_ram(KernelArgs a) { ram_wave_body<WaveChain<G, false>, M>(a); }

// 32 < d <= 256: two chains per wave (HalfWaveChain), so a column's pivot (three readlanes, a square root and three
// divisions) serves two chains' rows; G slot groups of 128 coordinates.
// Three waves per SIMD (168 VGPRs): at d = 256 the G = 2 kernel spills ~35 VGPRs (outside the column loop's
// critical path) and still runs 7 % faster than at two waves, 206 VGPRs (r4l: 9.06 against 8.44e6 chain-steps/s;
// d = 128 fits 168 without spills either way).
template <int G, class M>
__global__ __launch_bounds__(kBlock, 3) void wpc_ram2(KernelArgs a) { ram_wave_body<HalfWaveChain<G>, M>(a); }

template <class M>
static hipError_t wpc_ram_step(const KernelArgs& a, const LaunchPlan& p, hipStream_t st) {
    const hipError_t e = p.k.body == B_RAM2 ? for_int<1, 2>(p.k.n, [&](auto g) {
        constexpr int G = decltype(g)::value;
        return launch_inst(p, inst(MAP_WPC, B_RAM2, G, kBlock), wpc_ram2<G, M>, st, a);
    }) : for_int<2, 4>(p.k.n, [&](auto g) {
        constexpr int G = decltype(g)::value;
        return launch_inst(p, inst(MAP_WPC, B_RAM, G, kBlock), wpc_ram<G, M>, st, a);
    });
    return note_launched(e, p, M::kName);
}

KernelUnit wpc_ram_iso() { return {wpc_ram_step<IsoDot>, nullptr, nullptr}; }
KernelUnit wpc_ram_normal() { return {wpc_ram_step<NormalDSL>, nullptr, nullptr}; }
KernelUnit wpc_ram_absnormal() { return {wpc_ram_step<AbsNormalDSL>, nullptr, nullptr}; }
KernelUnit wpc_ram_dist() { return {wpc_ram_step<DistDSL>, nullptr, nullptr}; }

}  // namespace mcmc
