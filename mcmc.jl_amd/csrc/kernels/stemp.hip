// stemp.hip -- the walker bookkeeping of the SerialTempMC runner (src/runners/SerialTempMC.jl:31-85) on the device:
// C independent serial-tempering walkers, walker c = chain c of every target's chain batch.  The sampler step itself
// is the ordinary step kernel of each target; these four kernels pick the walker's target of a step, take its
// MCMCSample out of that target's batch, decide the swap and store.  One thread per walker, every array [..][C]:
// consecutive lanes touch consecutive doubles.
//
// A walker carries what run_serialtempmc reads of its last MCMCSample s (samplers.jl:10-18):
//   cur  = s.ppars      the position the walker's task holds; what is stored (SerialTempMC.jl:77)
//   prev = s.pars       the position before that step; what a swap resets the other task to (SerialTempMC.jl:62)
//   lt   = s.logtarget  the log-target at prev (SerialTempMC.jl:64)
// and the index `at` of its task.  The draws of runner step i are one Philox block (global chain id, i, 0,
// TAG_STEMP) under the run's seed: u = uniform52(w0, w1) picks the other task, u2 = uniform52(w2, w3) decides.
#include "../common.hpp"
#include "../detmath.hpp"
#include "../host/kernels_api.hpp"

namespace mcmc {

enum : uint32_t { TAG_STEMP = 8u };
constexpr int kStempT = 256;                       // whole waves: k_stemp_store ballots a word per wave

// tgt[c]: the task whose sample walker c takes this step.  Swap step (i % swapPeriod == 0): at2 = rand(1:(K-1)),
// at2 >= at ? at2 + 1 : at2 (SerialTempMC.jl:59-60), zero-based r = min(K - 2, floor(u (K - 1))).  Else: at.
__global__ void k_stemp_pick(int64_t C, int32_t K, uint32_t chain0, uint32_t key0, uint32_t key1, uint32_t step,
                             int32_t is_swap, const int32_t* at, int32_t* tgt) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int32_t a = at[c];
    int32_t t = a;
    if (is_swap) {
        const u32x4 w = philox4x32_10(chain0 + (uint32_t)c, step, 0u, TAG_STEMP, key0, key1);
        const double u = uniform52(w.x, w.y);
        int32_t r = (int32_t)__builtin_floor(u * (double)(K - 1));
        if (r > K - 2) r = K - 2;
        t = r >= a ? r + 1 : r;
    }
    tgt[c] = t;
}

// where tgt[c] == t: the sample of target t's chain c -- its new position x (columns, row stride ldx) and the
// log-target ll0 of the position it stepped from -- into the walker's candidate
__global__ void k_stemp_take(int64_t C, int d, int32_t t, const int32_t* tgt, const double* x, int64_t ldx,
                             const double* ll0, double* cand, double* cand_lt) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C || tgt[c] != t) return;
    for (int j = 0; j < d; ++j) cand[(size_t)j * C + c] = x[(size_t)j * ldx + c];
    cand_lt[c] = ll0[c];
}

// Swap step: accept iff u2 < exp(logtarget - s2.logtarget + logW[at2] - logW[at]) (SerialTempMC.jl:64), summed left
// to right; a NaN compares false.  Accepted: at = at2, s = s2 (cur, lt; s2.pars is prev already: at2 was reset to it).
// Rejected: the walker keeps its sample.  Other steps: s = consume(tasks[at]) -- the candidate, which stepped from cur.
__global__ void k_stemp_swap(int64_t C, int d, uint32_t chain0, uint32_t key0, uint32_t key1, uint32_t step,
                             int32_t is_swap, const double* logW, int32_t* at, const int32_t* tgt, double* cur,
                             double* prev, double* lt, const double* cand, const double* cand_lt, int32_t* swapped) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    int32_t acc = 0;
    if (is_swap) {
        const int32_t a = at[c], a2 = tgt[c];
        const u32x4 w = philox4x32_10(chain0 + (uint32_t)c, step, 0u, TAG_STEMP, key0, key1);
        const double u2 = uniform52(w.z, w.w);
        const double r = ((lt[c] - cand_lt[c]) + logW[a2]) - logW[a];
        acc = u2 < det_exp(r) ? 1 : 0;
        if (acc) at[c] = a2;
    } else {
        for (int j = 0; j < d; ++j) prev[(size_t)j * C + c] = cur[(size_t)j * C + c];
    }
    if (acc || !is_swap) {
        for (int j = 0; j < d; ++j) cur[(size_t)j * C + c] = cand[(size_t)j * C + c];
        lt[c] = cand_lt[c];
    }
    swapped[c] = acc;
}

// a runner step past burnin (SerialTempMC.jl:75-79): ppars, the task index, and the swap-accepted bit of walker c in
// bit c % 64 of word c / 64 (one wave ballot per word, as the step kernels' accept bits)
__global__ __launch_bounds__(kStempT) void k_stemp_store(int64_t C, int d, const double* cur, const int32_t* at,
                                                         const int32_t* swapped, double* samples, int32_t* models,
                                                         uint64_t* bits) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = c < C;
    if (live && samples)
        for (int j = 0; j < d; ++j) samples[(size_t)j * C + c] = cur[(size_t)j * C + c];
    if (live && models) models[c] = at[c];
    if (bits) {                                    // every lane of the wave reaches the ballot
        const uint64_t word = __ballot(live && swapped[c] != 0);
        if ((threadIdx.x & 63) == 0 && live) bits[c >> 6] = word;
    }
}

static unsigned stemp_blocks(int64_t n) { return (unsigned)((n + kStempT - 1) / kStempT); }

}  // namespace mcmc

hipError_t mcmc_stemp_pick(int64_t C, int32_t K, uint32_t chain0, uint64_t seed, uint32_t step, int32_t is_swap,
                           const int32_t* at, int32_t* tgt, hipStream_t st) {
    mcmc::k_stemp_pick<<<mcmc::stemp_blocks(C), mcmc::kStempT, 0, st>>>(C, K, chain0, (uint32_t)seed,
                                                                       (uint32_t)(seed >> 32), step, is_swap, at, tgt);
    return hipGetLastError();
}
hipError_t mcmc_stemp_take(int64_t C, int d, int32_t t, const int32_t* tgt, const double* x, int64_t ldx,
                           const double* ll0, double* cand, double* cand_lt, hipStream_t st) {
    mcmc::k_stemp_take<<<mcmc::stemp_blocks(C), mcmc::kStempT, 0, st>>>(C, d, t, tgt, x, ldx, ll0, cand, cand_lt);
    return hipGetLastError();
}
hipError_t mcmc_stemp_swap(int64_t C, int d, uint32_t chain0, uint64_t seed, uint32_t step, int32_t is_swap,
                           const double* logW, int32_t* at, const int32_t* tgt, double* cur, double* prev, double* lt,
                           const double* cand, const double* cand_lt, int32_t* swapped, hipStream_t st) {
    mcmc::k_stemp_swap<<<mcmc::stemp_blocks(C), mcmc::kStempT, 0, st>>>(C, d, chain0, (uint32_t)seed,
                                                                       (uint32_t)(seed >> 32), step, is_swap, logW, at,
                                                                       tgt, cur, prev, lt, cand, cand_lt, swapped);
    return hipGetLastError();
}
hipError_t mcmc_stemp_store(int64_t C, int d, const double* cur, const int32_t* at, const int32_t* swapped,
                            double* samples, int32_t* models, uint64_t* bits, hipStream_t st) {
    mcmc::k_stemp_store<<<mcmc::stemp_blocks(C), mcmc::kStempT, 0, st>>>(C, d, cur, at, swapped, samples, models, bits);
    return hipGetLastError();
}
