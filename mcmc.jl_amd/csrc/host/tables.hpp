// tables.hpp -- the host runtime's two tables: what it asks about a sampler kind, and which ChainState buffers a
// chain batch owns.  A new sampler adds one row to each.  Plain C++: no HIP runtime is needed, so
// tests/state_table_check.cpp walks both on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../common.hpp"

namespace mcmc {

// ------------------------------------------------------------------ sampler table
// the per-chain adaptive state a sampler keeps: driftStep (MALA.jl), leapStep and nLeaps (EmpiricalHMCTune, HMC.jl),
// the dual-averaged step (HMCDA.jl, NUTS.jl)
enum TunerState { TUNE_NONE, TUNE_DRIFT, TUNE_LEAP, TUNE_DUAL };

struct SamplerInfo {
    int32_t kind;
    const char* name;
    int needs;                  // the model's has_gradient level: 0 none, 1 gradient, 2 tensor, 3 tensor derivatives
    bool newton_in_t0;          // t0 carries nNewton, a double holding an integer
    const char* d_reason;       // non-NULL: built for d <= mcmc_smmala_max_d(), and why
    // One log-target evaluation per chain-step, so a launch of n steps adds C n evaluations: counted on the host.
    // The step kernels count only where the count is data-dependent (trajectories): one device-scope atomic per wave
    // on a single address serialises at the memory side (32 768 of them per 2^20-chain launch of the pair kernel,
    // ~10 ns apart) and held a short launch's tail for hundreds of microseconds.
    bool evals_on_host;
    bool emits_grads;           // the chain's gradients can be stored (RWM, RAM: no gradients)
    TunerState tuner_state;     // DRIFT and LEAP only with the tuner on
    bool manifold;              // the state carries the metric tensor, its inverse and firstTerm (SMMALA, PMALA)
    bool rm_family;             // the trajectory samplers on the metric tensor: the state is x, lp and g
    bool lmc;                   // ... of which ERMLMC and RMLMC
    bool records_leaps;         // storeLeaps is built (HMC.jl:145-150, HMCDA.jl:110-117)
    const char* leaps_refusal;  // non-NULL: why storeLeaps is not built for a sampler one could expect it of
    const char* seqmc_refusal;  // non-NULL: why SeqMC does not run targets of this sampler
};

inline const char kTile[] = " (the metric tensor of a 16-chain tile is held in registers); d = ";
inline const char kSmmTile[] = " (SMMALA's geometry: the metric tensor of a 16-chain tile is held in registers); d = ";

inline const SamplerInfo kSamplers[] = {
    {SK_RWM, "RWM", 0, false, nullptr, true, false, TUNE_NONE, false, false, false, false, nullptr, nullptr},
    {SK_RAM, "RAM", 0, false, nullptr, true, false, TUNE_NONE, false, false, false, false, nullptr, nullptr},
    {SK_MALA, "MALA", 1, false, nullptr, true, true, TUNE_DRIFT, false, false, false, false, nullptr, nullptr},
    {SK_HMC, "HMC", 1, false, nullptr, false, true, TUNE_LEAP, false, false, false, true, nullptr, nullptr},
    {SK_HMCDA, "HMCDA", 1, false, nullptr, false, true, TUNE_DUAL, false, false, false, true, nullptr, nullptr},
    {SK_NUTS, "NUTS", 1, false, nullptr, false, true, TUNE_DUAL, false, false, false, false, nullptr,
     "SeqMC does not run NUTS targets: NUTS adapts epsilon by its own step counter (NUTS.jl:166), which a population "
     "runner's resets do not carry"},
    {SK_SMMALA, "SMMALA", 2, false, kTile, true, true, TUNE_DRIFT, true, false, false, false, nullptr,   // SMMALA.jl:51
     "SeqMC does not run SMMALA targets: the sampler's reset hook keeps invG and firstTerm of the chain's previous "
     "position (SMMALA.jl:54-57)"},
    {SK_PMALA, "PMALA", 3, false, kSmmTile, true, true, TUNE_DRIFT, true, false, false, false, nullptr,  // PMALA.jl:54-55
     "SeqMC does not run PMALA targets: the sampler's reset hook keeps invG, firstTerm and secondTerm of the chain's "
     "previous position (PMALA.jl:63-66)"},
    {SK_RMHMC, "RMHMC", 3, true, kSmmTile, false, true, TUNE_LEAP, false, true, false, false,          // RMHMC.jl:65-66
     "storeLeaps is not built for RMHMC: the reference's RMHMC keeps no leapfrog record (RMHMC.jl:120-155)",
     "SeqMC does not run RMHMC targets: the population runner's device path is built for the samplers without a "
     "metric tensor"},
    {SK_ERMLMC, "ERMLMC", 3, false, kSmmTile, false, true, TUNE_LEAP, false, true, true, false,        // ERMLMC.jl:60-61
     "storeLeaps is not built for ERMLMC: the reference's sampler keeps no leapfrog record (ERMLMC.jl:114-152)",
     "SeqMC does not run ERMLMC targets: the sampler's reset hook keeps invG, cholG, traceInvGxdG, dphi and C of the "
     "chain's previous position (ERMLMC.jl:64-67), which mcmc_chains_set_state does not"},
    {SK_RMLMC, "RMLMC", 3, true, kSmmTile, false, true, TUNE_LEAP, false, true, true, false,           // RMLMC.jl:65-66
     "storeLeaps is not built for RMLMC: the reference's sampler keeps no leapfrog record (ERMLMC.jl:114-152)",
     "SeqMC does not run RMLMC targets: the sampler's reset hook keeps invG, cholG, traceInvGxdG, dphi and C of the "
     "chain's previous position (ERMLMC.jl:64-67), which mcmc_chains_set_state does not"},
};

// the row of a kind; NULL for a kind the library does not know (mcmc_sampler_validate refuses it)
inline const SamplerInfo* sampler_row(int32_t kind) {
    for (const SamplerInfo& si : kSamplers)
        if (si.kind == kind) return &si;
    return nullptr;
}

// ------------------------------------------------------------------ chain-state table
enum Layout { LAYOUT_LPC = 0, LAYOUT_WPC = 1, LAYOUT_GLM = 2 };

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
// rows of a packed lower-triangular d x d matrix
inline size_t packed_rows(int d) { return (size_t)d * (size_t)(d + 1) / 2; }

// what a chain batch's buffer sizes depend on
struct StateDims {
    const SamplerInfo* si;
    int32_t tuner;              // EmpMCTuner on/off
    Layout layout;
    int d;
    int64_t C, ld;              // chains; leading dimension of the state arrays
    int d_pad;                  // regression layout: the kernels' padded coordinate count (mcmc_glm_d_pad)
    int64_t levels;             // NUTS: maxdoublings
    int64_t ram_hs;             // RAM: doubles in one half of the factor
};

enum StateShape {
    SHAPE_STATE,                // state rows: [d][ld], wave-per-chain [C][ld]
    SHAPE_PACKED,               // packed lower rows [d(d+1)/2][ld]
    SHAPE_F64,                  // one double per chain, padded to 64 chains
    SHAPE_I32,                  // one int32 per chain, likewise
    SHAPE_RAM,                  // RAM's factor, two halves (ram.hpp); forked by its own re-tiling code
    SHAPE_NUTS_WV,              // NUTS level stack, vectors [maxdoublings][3][d][ld] (nuts.hpp)
    SHAPE_NUTS_WS,              // NUTS level stack, scalars [maxdoublings][4][ld] ([2 ld] with two lanes per chain)
    SHAPE_MOM                   // regression HMC / HMCDA on d-slices: parked momentum [d_pad][ld] (glm_hmc)
};

// One ChainState pointer: its member, shape, whether it holds state between steps (mcmc_chains_fork copies exactly
// those), and which batches own it.  mcmc_chains_create, free_state and mcmc_chains_fork walk this table.
struct StateBuf {
    const char* name;
    double* ChainState::*f64;   // the member: f64 or i32 is set
    int32_t* ChainState::*i32;
    StateShape shape;
    bool live;
    bool (*exists)(const StateDims&);
};

inline bool tuned(const StateDims& s) {
    return s.tuner && (s.si->tuner_state == TUNE_DRIFT || s.si->tuner_state == TUNE_LEAP);
}
inline bool dual(const StateDims& s) { return s.si->tuner_state == TUNE_DUAL; }
inline bool is_nuts(const StateDims& s) { return s.si->kind == SK_NUTS; }

// in the order mcmc_chains_fork copies them; the buffers dead between steps last
inline const StateBuf kStateTable[] = {
    {"x", &ChainState::x, nullptr, SHAPE_STATE, true, [](const StateDims&) { return true; }},
    // gradient at the state (regression targets are not separable)
    {"g", &ChainState::g, nullptr, SHAPE_STATE, true, [](const StateDims& s) { return s.layout == LAYOUT_GLM; }},
    {"sm_ft", &ChainState::sm_ft, nullptr, SHAPE_STATE, true, [](const StateDims& s) { return s.si->manifold; }},
    {"pm_c", &ChainState::pm_c, nullptr, SHAPE_STATE, true, [](const StateDims& s) { return s.si->kind == SK_PMALA; }},
    {"sm_G", &ChainState::sm_G, nullptr, SHAPE_PACKED, true, [](const StateDims& s) { return s.si->manifold; }},
    {"sm_invG", &ChainState::sm_invG, nullptr, SHAPE_PACKED, true, [](const StateDims& s) { return s.si->manifold; }},
    {"lp", &ChainState::lp, nullptr, SHAPE_F64, true, [](const StateDims&) { return true; }},
    {"t_step", &ChainState::t_step, nullptr, SHAPE_F64, true, [](const StateDims& s) { return tuned(s) || dual(s); }},
    {"t_bar", &ChainState::t_bar, nullptr, SHAPE_F64, true, dual},
    {"t_h", &ChainState::t_h, nullptr, SHAPE_F64, true, dual},
    {"t_mu", &ChainState::t_mu, nullptr, SHAPE_F64, true, is_nuts},
    {"t_leaps", nullptr, &ChainState::t_leaps, SHAPE_I32, true,
     [](const StateDims& s) { return tuned(s) && s.si->tuner_state == TUNE_LEAP; }},
    {"t_acc", nullptr, &ChainState::t_acc, SHAPE_I32, true, tuned},
    {"t_prop", nullptr, &ChainState::t_prop, SHAPE_I32, true, tuned},
    {"ram_L", &ChainState::ram_L, nullptr, SHAPE_RAM, true, [](const StateDims& s) { return s.si->kind == SK_RAM; }},
    // the proposal's tensor and inverse (SMMALA, PMALA); the trajectory's current inverse (rmhmc.hip) and tensor
    // (lmc.hip)
    {"sm_pG", &ChainState::sm_pG, nullptr, SHAPE_PACKED, false,
     [](const StateDims& s) { return s.si->manifold || s.si->lmc; }},
    {"sm_pinvG", &ChainState::sm_pinvG, nullptr, SHAPE_PACKED, false,
     [](const StateDims& s) { return s.si->manifold || s.si->rm_family; }},
    {"nuts_wv", &ChainState::nuts_wv, nullptr, SHAPE_NUTS_WV, false, is_nuts},
    {"nuts_ws", &ChainState::nuts_ws, nullptr, SHAPE_NUTS_WS, false, is_nuts},
    {"mom", &ChainState::mom, nullptr, SHAPE_MOM, false,
     [](const StateDims& s) {
         return s.layout == LAYOUT_GLM && s.d > 128 && (s.si->kind == SK_HMC || s.si->kind == SK_HMCDA);
     }},
};

inline size_t state_elem_bytes(const StateBuf& b) { return b.i32 ? sizeof(int32_t) : sizeof(double); }

// elements of a buffer the batch owns
inline size_t state_count(const StateBuf& b, const StateDims& s) {
    const size_t ld = (size_t)s.ld, d = (size_t)s.d;
    switch (b.shape) {
        case SHAPE_STATE: return s.layout != LAYOUT_WPC ? d * ld : (size_t)s.C * ld;
        case SHAPE_PACKED: return packed_rows(s.d) * ld;
        case SHAPE_F64:
        case SHAPE_I32: return (size_t)round_up(s.C, 64);
        case SHAPE_RAM: return 2 * (size_t)s.ram_hs;
        case SHAPE_NUTS_WV: return (size_t)s.levels * 3 * d * ld;
        case SHAPE_NUTS_WS: return (size_t)s.levels * 4 * (size_t)(s.d > 16 ? 2 : 1) * ld;
        case SHAPE_MOM: return (size_t)s.d_pad * ld;
    }
    return 0;
}

inline void* state_get(const ChainState& st, const StateBuf& b) {
    return b.i32 ? (void*)(st.*b.i32) : (void*)(st.*b.f64);
}
inline void state_set(ChainState& st, const StateBuf& b, void* p) {
    if (b.i32) st.*b.i32 = (int32_t*)p;
    else st.*b.f64 = (double*)p;
}

}  // namespace mcmc
