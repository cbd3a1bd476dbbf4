// glm_stamps.hpp -- dev-only profiling instruments of the regression kernels: shader-clock phase stamps of the tile
// loops.  Two builds, each of ONE translation unit with its flag (the other objects as shipped):
//   -DGLM_STAMP    on glm.hip          the d-sliced tile loop of glm_eval (glm_device.hpp), scripts/glm_stamps.py
//   -DGLM_WS_STAMP on glm_mala1ws.hip  glm_mala1ws's tile loop and phases, scripts/ws_stamps.py
// Without the flags the macros below are empty statements and nothing else here is compiled.  The stamp sites stay
// in the kernels; the stamps are kept in LDS past the kernel's own (global stores inside the loop would count on
// vmcnt and stretch the DMA waits they measure) and copied out after the loop.
#pragma once
#include <hip/hip_runtime.h>

#ifdef GLM_STAMP
// Low 32 bits of the shader clock at the d-sliced tile loop's phases, every wave of workgroups 0..3, tiles 8..23 of the
// last evaluation (the points: loop top, eta partial stored, barrier 1, weights stored, barrier 2, G issued, tile t+1
// landed, barrier 3), in 4 KB of LDS (stamp_lds, glm_eval).
namespace mcmc {
constexpr int kGlmStampLdsBytes = 8 * 16 * 8 * 4;
static __device__ unsigned g_glm_stamps[4][8][16][8];
}  // namespace mcmc
#define GLM_STAMPT(pt)                                                                                  \
    do {                                                                                               \
        if (t >= 8 && t < 24) {                                                                        \
            const unsigned ts_ = (unsigned)__builtin_amdgcn_s_memtime();                              \
            if ((threadIdx.x & 63) == 0) stamp_lds[((threadIdx.x >> 6) * 16 + (t - 8)) * 8 + (pt)] = ts_; \
        }                                                                                              \
    } while (0)
extern "C" int mcmc_debug_glm_stamps(long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(mcmc::g_glm_stamps), sizeof(mcmc::g_glm_stamps)) == hipSuccess ? 0 : 4;
}
#else
#define GLM_STAMPT(pt) do { } while (0)
#endif

#ifdef GLM_WS_STAMP
// Low 32 bits of the shader clock in glm_mala1ws, every wave of workgroups 0..3.  Tiles 8..23 of the tile loop
// (WS_STAMP, in LDS wst): M waves at the loop top, eta_{t+1} stored, G_{t-1} issued, past the barrier; V waves at the
// loop top, tile t+2 issued, the terms of tile t done, r_t stored, past the barrier.
namespace mcmc {
static __device__ unsigned g_ws_stamps[4][8][16][8];
static __device__ unsigned g_ws_wg[4][8][8];           // per wave: start, proposal, bx/tile 2, eta_0, loop end, final barrier, end
static __device__ unsigned g_ws_wg2[4][8][8];          // inside the proposal phase (V: normals done, qf summed, table; M: tiles 0, 1)
}  // namespace mcmc
#define WS_WG2(pt)                                                                                     \
    do {                                                                                               \
        const unsigned ts_ = (unsigned)__builtin_amdgcn_s_memtime();                                  \
        if (blockIdx.x < 4 && (threadIdx.x & 63) == 0) g_ws_wg2[blockIdx.x][threadIdx.x >> 6][pt] = ts_; \
    } while (0)
#define WS_WG(pt)                                                                                      \
    do {                                                                                               \
        const unsigned ts_ = (unsigned)__builtin_amdgcn_s_memtime();                                  \
        if (blockIdx.x < 4 && (threadIdx.x & 63) == 0) g_ws_wg[blockIdx.x][threadIdx.x >> 6][pt] = ts_; \
    } while (0)
#define WS_STAMP(pt)                                                                                   \
    do {                                                                                               \
        if (t >= 8 && t < 24) {                                                                        \
            const unsigned ts_ = (unsigned)__builtin_amdgcn_s_memtime();                              \
            if (p.lane == 0) wst[(wv * 16 + (int)(t - 8)) * 8 + (pt)] = ts_;                          \
        }                                                                                              \
    } while (0)
extern "C" int mcmc_debug_ws_stamps(unsigned* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(mcmc::g_ws_stamps), sizeof(mcmc::g_ws_stamps)) == hipSuccess ? 0 : 4;
}
extern "C" int mcmc_debug_ws_wg(unsigned* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(mcmc::g_ws_wg), sizeof(mcmc::g_ws_wg)) == hipSuccess ? 0 : 4;
}
extern "C" int mcmc_debug_ws_wg2(unsigned* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(mcmc::g_ws_wg2), sizeof(mcmc::g_ws_wg2)) == hipSuccess ? 0 : 4;
}
#else
#define WS_STAMP(pt) do { } while (0)
#define WS_WG(pt) do { } while (0)
#define WS_WG2(pt) do { } while (0)
#endif
