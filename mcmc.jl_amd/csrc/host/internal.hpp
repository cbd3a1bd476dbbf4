// internal.hpp -- what the host runtime's translation units share (not part of the C ABI): the objects behind the
// opaque handles, error reporting, device-memory helpers and the layout helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../../include/mcmc_hip.h"
#include "../common.hpp"
#include "kernels_api.hpp"
#include "tables.hpp"

// ------------------------------------------------------------------ errors
// set the calling thread's mcmc_last_error() message; returns code
int mcmc_set_error(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            return mcmc_set_error(e_ == hipErrorOutOfMemory ? MCMC_E_OOM : MCMC_E_HIP,         \
                                  std::string(#expr) + ": " + hipGetErrorString(e_));          \
        }                                                                                      \
    } while (0)

// ------------------------------------------------------------------ objects
struct mcmc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int32_t* d_err = nullptr;
    // a second stream for launch sequences that split a batch in two halves whose kernels bind on different resources
    // (RAM on regression targets: the MFMA eval of one half beside the HBM-bound factor update of the other)
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};

struct mcmc_model {
    mcmc_ctx* ctx = nullptr;
    mcmc::ModelArgs args{};
    int has_gradient = 0;
    std::vector<double> init, scale;
    double* d_init = nullptr;
    double* d_scale = nullptr;
    double* d_X = nullptr;
    double* d_Y = nullptr;
    int chains_alive = 0;            // chains created on this model and not yet destroyed
    bool released = false;           // mcmc_model_destroy called: free when the last chains go
};

struct DevBuf { void* p = nullptr; size_t bytes = 0; };   // a library-owned device buffer that only grows (ensure)

struct mcmc_chains {
    mcmc_model* model = nullptr;
    mcmc_sampler_cfg cfg{};          // the sampler configuration it was created with (mcmc_chains_fork)
    mcmc::SamplerArgs sa{};
    const mcmc::SamplerInfo* si = nullptr;   // the sampler table's row of sa.kind
    int64_t C = 0, ld = 0, offset = 0;
    uint64_t seed = 0;
    mcmc::Layout layout = mcmc::LAYOUT_LPC;
    mcmc::ChainState st{};
    double* d_scale_eff = nullptr;   // model.scale .* sampler.scale (RWM.jl:52)
    std::vector<double> h_scale_eff; // its host copy
    int ram_dpad = 0;                // RAM: padded factor width
    bool ram_wave = false;           // RAM: the factor in the wave-per-chain layout (separable d > 32, regression d > 32)
    bool glm_ram_wave = false;       // RAM on a regression target with d > 32: the split step (glm_ram_wave.hip)
    double *ram_u = nullptr, *ram_nz = nullptr, *xprop = nullptr, *lpp = nullptr;   // ... its buffers
    double scale1 = 0.0;             // its common value when all coordinates agree
    int32_t scale_uniform = 0;
    double* d_init_x = nullptr;      // optional per-chain start, [d][C]
    unsigned long long* d_evals = nullptr;   // log-target evaluations since create/reset (all chains)
    int64_t h_evals = 0;             // ... of the samplers with one evaluation per chain-step, counted here
    int64_t steps_done = 0;
    int64_t spl = 0;                 // steps per launch (0: whole run)
    int store_grads = 1;
    int64_t tuner_burnin = -1;       // the tuners' burnin (mcmc_chains_set_tuner_burnin); -1: the run's runner burnin
    DevBuf out_samples, out_grads, out_bits, out_tmp, stage_samples, stage_grads;
    DevBuf order_buf;                // regression HMC / HMCDA: chain slot -> chain (StepArgs.order)
    std::vector<int32_t> h_order;
    bool last_order = false;         // the last run launched with order_buf (mcmc_debug_chains_order)
    // storeLeaps (HMC.jl:145-150): host buffers the next run fills (h_lpars == NULL: off), device staging
    int64_t leap_cap = 0;
    double *h_lpars = nullptr, *h_lgrads = nullptr, *h_lmom = nullptr, *h_llp = nullptr, *h_lH = nullptr;
    int32_t* h_lnl = nullptr;
    DevBuf leap_buf;
    // NUTS diagnostics (mcmc_chains_nuts_diagnostics): buffers the next run fills (nuts_eps == NULL: off)
    double* nuts_eps = nullptr;
    int32_t* nuts_nd = nullptr;
    bool nuts_on_device = false;
    DevBuf nuts_buf;
    std::string step_kernel;         // the step kernel instance the last run launched
};

// ------------------------------------------------------------------ device memory
// Transfers are ordered on the context's (non-blocking) stream, after every kernel queued there,
// and waited for before the host buffer is released.
inline hipError_t copy_wait(mcmc_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
    return e == hipSuccess ? hipStreamSynchronize(ctx->stream) : e;
}
inline hipError_t h2d(mcmc_ctx* ctx, void* dst, const void* src, size_t bytes) {
    return copy_wait(ctx, dst, src, bytes, hipMemcpyHostToDevice);
}
inline hipError_t d2h(mcmc_ctx* ctx, void* dst, const void* src, size_t bytes) {
    return copy_wait(ctx, dst, src, bytes, hipMemcpyDeviceToHost);
}
inline hipError_t dzero(mcmc_ctx* ctx, void* dst, size_t bytes) {
    return hipMemsetAsync(dst, 0, bytes, ctx->stream);
}

inline int set_device(mcmc_ctx* ctx) {
    HIP_TRY(hipSetDevice(ctx->device));
    return MCMC_OK;
}

inline int dmalloc_bytes(void** p, size_t bytes) {
    *p = nullptr;
    if (bytes == 0) return MCMC_OK;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        *p = nullptr;
        return mcmc_set_error(MCMC_E_OOM, std::string("hipMalloc(") + std::to_string(bytes) + " B): " +
                                              hipGetErrorString(e));
    }
    return MCMC_OK;
}
template <class T>
inline int dmalloc(T** p, size_t count) {
    return dmalloc_bytes((void**)p, count * sizeof(T));
}

inline void dfree(void* p) { if (p) (void)hipFree(p); }

// grow a library-owned output buffer to at least `bytes` (chains.cpp)
int ensure(DevBuf& b, size_t bytes);

// The device temporaries of one call: freed together on scope exit, after the stream has drained.
class DevScope {
    hipStream_t st_;
    std::vector<void*> owned_;

public:
    explicit DevScope(hipStream_t st) : st_(st) {}
    DevScope(const DevScope&) = delete;
    DevScope& operator=(const DevScope&) = delete;
    ~DevScope() {
        (void)hipStreamSynchronize(st_);
        for (void* p : owned_) dfree(p);
    }
    template <class T>
    int alloc(T** p, size_t count) {
        const int rc = dmalloc(p, count);
        if (*p) owned_.push_back(*p);
        return rc;
    }
};

// the sampler table's row of a kind mcmc_sampler_validate has accepted (tables.hpp)
inline const mcmc::SamplerInfo& sampler_info(int32_t kind) { return *mcmc::sampler_row(kind); }

// ------------------------------------------------------------------ layouts (model.cpp)
// the lane / wave-per-chain kernel families (the joint OU target runs there too, at its fixed d = 3)
bool model_is_separable(const mcmc_model* m);
bool model_is_glm(const mcmc_model* m);
// State layout of a chain batch: lane-per-chain [d][ld] for d <= 32, wave-per-chain [C][ld] above.
mcmc::Layout layout_for(const mcmc_model* m);
inline int64_t ld_for(mcmc::Layout L, int64_t C, int d) {
    return L == mcmc::LAYOUT_WPC ? mcmc::round_up(d, 4) : mcmc::round_up(C, 64);
}
mcmc::KernelArgs base_args(const mcmc_model* m, int64_t C, int64_t ld);
hipError_t launch_eval(mcmc::Layout L, const mcmc::KernelArgs& a, const double* xin, double* lp, double* g, int check,
                       hipStream_t st);
// [d][C] (stride ldc) <-> state layout
hipError_t cols_to_state(mcmc::Layout L, double* state, int64_t ld, const double* cols, int64_t ldc, int d, int64_t C,
                         hipStream_t st);
hipError_t state_to_cols(mcmc::Layout L, double* cols, int64_t ldc, const double* state, int64_t ld, int d, int64_t C,
                         hipStream_t st);
void model_free(mcmc_model* m);

// ------------------------------------------------------------------ launches (run.cpp)
// the runner range a step launch sees (run-local), and the tuners' burnin
struct RunRange {
    int64_t burnin, thinning, len, tuner_burnin;
};
// the launch arguments of a batch: its chains, their random streams and state, the evaluation counter, and the range
mcmc::KernelArgs step_args(const mcmc_chains* c, const RunRange& r);
// the step kernels of one launch: the only place that maps a sampler kind to its step launcher
hipError_t launch_chain_step(const mcmc_chains* c, const mcmc::KernelArgs& a, hipStream_t st);
// one sampler step of every chain of c from its current state, nothing kept, the tuners' burnin 0: the `consume` of
// the population runners (seqmc_stats.cpp; SeqMC.jl:69, SerialTempMC.jl:63,68)
int step_once(mcmc_chains* c, hipStream_t st);
// forget the step kernel noted on this thread (kernels_api.hpp mcmc_note_step_kernel; context.cpp)
void mcmc_clear_step_kernel();
// mcmc_run_serialmc with host outputs of a larger batch: rows ldc chains apart (run.cpp)
int mcmc_run_serialmc_ld(mcmc_chains* c, const mcmc_runner_cfg* r, mcmc_outputs* out, int64_t ldc, double* copy_s);
