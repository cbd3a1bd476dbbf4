// launch_plan.hpp -- which kernel instance of the separable and joint targets a launch runs, with what grid and block,
// and the name it reports: the instance rule, stated once.  Plain C++: no HIP runtime is needed, so
// tests/launch_plan_check.cpp walks it on the CPU.  lpc_impl.hpp, wpc_impl.hpp, nuts_impl.hpp, slice_impl.hpp and wpc_ram.hip launch
// what the plan names; the kernels' __launch_bounds__ read the block sizes below.  A host compiler that includes it
// defines __host__ and __device__ to nothing first (common.hpp marks its argument blocks with them), as for tables.hpp.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../common.hpp"

namespace mcmc {

// ------------------------------------------------------------------ class limits and block sizes
constexpr int kLaneMaxD = 16;         // lpc: one lane per chain, NB = ceil(d/4) Philox blocks a lane
constexpr int kPairMaxD = 32;         // lpp: two lanes per chain, NBL = ceil(NB/2); the state layout [d][ld] ends here
constexpr int kWaveMaxD = 2048;       // wpc: one wave per chain, NB slots of 256 coordinates
constexpr int kBlockMaxD = 16384;     // bpc: W waves per chain; the state layout [C][ld] ends here
constexpr int kRamHalfMaxD = 256;     // wpc_ram2: two chains per wave, G slot groups of 128 coordinates
constexpr int kRamMaxD = 1024;        // wpc_ram
constexpr int kNutsMaxD = kPairMaxD;
constexpr int kSliceMaxD = kPairMaxD;
constexpr int kLaMaxChains = 64;      // RWM on C <= 64 chains of d <= 32: lpc_rwm_la, one block
constexpr int kSpecMaxD = 4;          // ... and on one chain of d <= 4: lpc_rwm_spec<d>
constexpr int kPlanBlock = 256;       // samplers.hpp kBlock: every kernel without a size of its own
constexpr int kPairThreads = 512;     // lpp_rwm, lpp_hmc

// waves per chain for d > 2048 (8 slots of 256 W coordinates); 0: not built
constexpr int bpc_waves_for(int d) { return d <= kWaveMaxD ? 1 : d <= 8192 ? 4 : d <= kBlockMaxD ? 8 : 0; }
// Philox blocks per lane of the wave kernels: d <= 256 NB; 0: not built
constexpr int wpc_nb_for(int d) { return d <= 256 ? 1 : d <= 512 ? 2 : d <= 1024 ? 4 : d <= kWaveMaxD ? 8 : 0; }

// lpc_rwm: 512-thread blocks of 56 KB LDS, two a CU, so 2^20 chains are exactly four rounds of the resident blocks
constexpr int kLpcRwmThreads = 512;
// lpc_mala / lpc_hmc: two 56 KB-LDS blocks a CU, sized so that they fill the occupancy the registers allow
// (d <= 4: 125 VGPRs, four waves per SIMD; d <= 8: ~155, three; d <= 16: ~200-240, two)
constexpr int lpc_grad_threads(int nb) { return nb == 1 ? 512 : (nb == 2 ? 768 : 256); }
// lpp_mala, measured at d = 32: 768 threads 0.0957 ms a step, 512 0.0966; the masked instances fit two waves
constexpr int lpp_mala_threads(bool full) { return full ? 768 : kPairThreads; }

// ------------------------------------------------------------------ one row per model of the family
struct PlanModel {
    int32_t kind;
    const char* name;            // the model class's kName (models.hpp)
    bool full_lane, full_wave;   // FULL instances (every lane coordinate is a real one): the models the benchmarks run
    bool wave;                   // wave- and block-per-chain kernels are built (d > 32)
    bool ram;                    // RAM kernels are built
    int nuts_max_nb;             // NUTS: the widest NB built (joint models: the catalogue's two are d = 1 and d = 3)
};
inline constexpr PlanModel kPlanModels[] = {
    {MK_ISO, "IsoDot", true, true, true, true, 8},
    {MK_NORMAL, "NormalDSL", true, false, true, true, 8},
    {MK_ABS_NORMAL, "AbsNormalDSL", false, false, true, true, 8},
    {MK_DIST, "DistDSL", false, false, true, true, 8},
    {MK_DIST_OBS, "DistObsDSL", false, false, false, false, 1},
    {MK_OU, "OUDSL", false, false, false, true, 1},
};
// the row of a kind; NULL for a kind outside the family
constexpr const PlanModel* plan_model(int32_t kind) {
    for (const PlanModel& m : kPlanModels)
        if (m.kind == kind) return &m;
    return nullptr;
}
constexpr bool plan_same_name(const char* a, const char* b) {
    for (; *a && *a == *b; ++a, ++b) {}
    return *a == *b;
}

// ------------------------------------------------------------------ the plan
// A kernel family is a mapping and a body: <map>_<body>, e.g. lpp_rwm, wpc_ram2, lpc_nuts_init
enum Mapping : int32_t { MAP_LPC, MAP_LPP, MAP_WPC, MAP_BPC };
enum Body : int32_t {
    B_RWM, B_RWM_LA, B_RWM_SPEC, B_MALA, B_HMC, B_RAM, B_RAM2, B_NUTS, B_NUTS_INIT, B_EVAL, B_HMC_REC, B_SLICE
};
// OP_SLICE: the slice sampler (slice_impl.hpp), a function on a model and no sampler kind: `sampler` is not read
enum PlanOp : int32_t { OP_STEP, OP_EVAL, OP_RECORD, OP_NUTS_INIT, OP_SLICE };

struct KernelInstance {
    Mapping map;
    Body body;
    int n;               // NB (lpc, wpc), NBL (lpp), W (bpc), G (wpc_ram, wpc_ram2) or D (lpc_rwm_spec)
    bool F, US, DA;      // FULL; uniform RWM scale; HMCDA
    int threads;         // per block
};
constexpr KernelInstance inst(Mapping map, Body body, int n, int threads, bool F = false, bool US = false,
                                  bool DA = false) {
    return KernelInstance{map, body, n, F, US, DA, threads};
}
inline bool operator==(const KernelInstance& a, const KernelInstance& b) {
    return a.map == b.map && a.body == b.body && a.n == b.n && a.F == b.F && a.US == b.US && a.DA == b.DA &&
           a.threads == b.threads;
}
struct LaunchPlan {
    bool built;          // false: the library refuses the combination
    KernelInstance k;
    int chains_per_block;
    int64_t grid;
};

inline LaunchPlan launch_plan(int32_t model, int32_t sampler, int d, int64_t C, bool scale_uniform, PlanOp op) {
    LaunchPlan p{};
    KernelInstance& k = p.k;
    const PlanModel* row = plan_model(model);
    if (!row) return p;
    const PlanModel& pm = *row;
    const int nb = (d + 3) / 4;
    const bool lane = d <= kLaneMaxD, pair = d <= kPairMaxD;         // pair: lane-per-chain state, one lane or two
    if (d < 1 || (!pair && !pm.wave)) return p;
    k.threads = kPlanBlock;
    if (op == OP_NUTS_INIT || (op == OP_STEP && sampler == SK_NUTS)) {
        if (nb > pm.nuts_max_nb) return p;                           // at most 8: d <= kNutsMaxD
        const Body body = op == OP_STEP ? B_NUTS : B_NUTS_INIT;
        k = lane ? inst(MAP_LPC, body, nb, kPlanBlock) : inst(MAP_LPP, body, (nb + 1) / 2, kPlanBlock);
    } else if (op == OP_SLICE) {
        // d <= kSliceMaxD; the joint models at their catalogue sizes, like NUTS (nuts_max_nb)
        if (!pair || nb > pm.nuts_max_nb) return p;
        k = lane ? inst(MAP_LPC, B_SLICE, nb, kPlanBlock) : inst(MAP_LPP, B_SLICE, (nb + 1) / 2, kPlanBlock);
    } else if (op == OP_STEP && sampler == SK_RAM) {
        if (!pm.ram || d > kRamMaxD) return p;
        if (pair) k = inst(MAP_LPC, B_RAM, nb, kPlanBlock);
        else if (d <= kRamHalfMaxD) k = inst(MAP_WPC, B_RAM2, d <= kRamHalfMaxD / 2 ? 1 : 2, kPlanBlock);
        else k = inst(MAP_WPC, B_RAM, wpc_nb_for(d), kPlanBlock);
    } else {
        if (d > kBlockMaxD || (op == OP_STEP && (sampler < SK_RWM || sampler > SK_HMCDA))) return p;
        k.map = lane ? MAP_LPC : pair ? MAP_LPP : d <= kWaveMaxD ? MAP_WPC : MAP_BPC;
        k.n = lane ? nb : pair ? (nb + 1) / 2 : d <= kWaveMaxD ? wpc_nb_for(d) : bpc_waves_for(d);
        k.DA = op != OP_EVAL && sampler == SK_HMCDA;
        k.body = op == OP_EVAL ? B_EVAL : op == OP_RECORD ? B_HMC_REC
                 : sampler == SK_RWM ? B_RWM : sampler == SK_MALA ? B_MALA : B_HMC;
        if (op == OP_STEP) {
            // FULL: d fills every coordinate slot of the instance (4 NB, 8 NBL, 256 NB), on the models that have it
            const int slots = (lane ? 4 : pair ? 8 : 256) * k.n;
            k.F = k.map != MAP_BPC && d == slots && (pair ? pm.full_lane : pm.full_wave);
            if (pair && sampler == SK_RWM) {
                k.US = scale_uniform;                                // US: RWM of the lane and pair mappings only
                if (C <= kLaMaxChains) {                             // the look-ahead and speculation kernels
                    const bool spec = C == 1 && d <= kSpecMaxD;
                    k = inst(MAP_LPC, spec ? B_RWM_SPEC : B_RWM_LA, spec ? d : nb, kPlanBlock, false, k.US);
                } else {
                    k.threads = lane ? kLpcRwmThreads : kPairThreads;
                }
            } else if (pair) {
                k.threads = lane ? lpc_grad_threads(nb) : k.body == B_MALA ? lpp_mala_threads(k.F) : kPairThreads;
            }
        }
        if (k.map == MAP_BPC) k.threads = 64 * k.n;
    }
    p.chains_per_block = k.body == B_RWM_LA ? kLaMaxChains : k.body == B_RWM_SPEC ? 1
                         : k.map == MAP_LPC ? k.threads : k.map == MAP_LPP ? k.threads / 2
                         : k.map == MAP_BPC ? 1 : kPlanBlock / 64 * (k.body == B_RAM2 ? 2 : 1);
    p.grid = (C + p.chains_per_block - 1) / p.chains_per_block;
    p.built = true;
    return p;
}

// the instance as mcmc_chains_step_kernel reports it: "family<template arguments>"; returns snprintf's count
inline int plan_kernel_name(char* buf, size_t size, const KernelInstance& k, const char* model) {
    static const char* const maps[] = {"lpc", "lpp", "wpc", "bpc"};
    static const char* const bodies[] = {"rwm", "rwm_la", "rwm_spec", "mala", "hmc", "ram", "ram2", "nuts", "nuts_init",
                                         "eval", "hmc_rec", "slice"};
    const bool has_f = (k.body == B_RWM || k.body == B_MALA || k.body == B_HMC) && k.map != MAP_BPC;
    const bool has_us = k.body == B_RWM_LA || k.body == B_RWM_SPEC || (k.body == B_RWM && k.map <= MAP_LPP);
    const bool has_da = k.body == B_HMC || k.body == B_HMC_REC;
    auto b = [](bool v) { return v ? "true" : "false"; };
    return snprintf(buf, size, "%s_%s<%d%s%s, %s%s%s>", maps[k.map], bodies[k.body], k.n, has_f ? ", " : "",
                    has_f ? b(k.F) : "", model, has_us || has_da ? ", " : "", has_us ? b(k.US) : has_da ? b(k.DA) : "");
}

}  // namespace mcmc
