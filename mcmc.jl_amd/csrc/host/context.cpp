// context.cpp -- error reporting and device contexts of the host runtime behind the C ABI (include/mcmc_hip.h).
//
// The runtime owns device contexts (here), model uploads (model.cpp), per-chain state (chains.cpp), the SerialMC loop
// (run.cpp) and SeqMC, statistics and probes (seqmc_stats.cpp).  Everything numeric runs in the HIP kernels; the host
// validates arguments (sampler.cpp: the reference's @asserts), plans launches and moves buffers.
#include <cstdarg>
#include <cstdio>

#include "internal.hpp"

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;

extern "C" const char* mcmc_last_error(void) { return g_err.c_str(); }
int mcmc_set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// the step kernel instance the last launch function on this thread dispatched (kernels_api.hpp)
static thread_local char g_step_kernel[160];
static thread_local bool g_noted;                      // false: cleared (g_step_kernel keeps the text it was formatted to)
static thread_local mcmc::KernelInstance g_inst;       // the instance g_step_kernel was formatted from, while
static thread_local const char* g_inst_model;          // g_inst_model is not NULL
void mcmc_note_step_kernel(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_step_kernel, sizeof g_step_kernel, fmt, ap);
    va_end(ap);
    g_inst_model = nullptr;
    g_noted = true;
}
// a run of one-step launches notes the same instance every time: it is formatted once
void mcmc_note_step_instance(const mcmc::KernelInstance& k, const char* model) {
    if (g_inst_model != model || !(g_inst == k)) {
        mcmc::plan_kernel_name(g_step_kernel, sizeof g_step_kernel, k, model);
        g_inst = k;
        g_inst_model = model;
    }
    g_noted = true;
}
const char* mcmc_last_step_kernel() { return g_noted ? g_step_kernel : ""; }
void mcmc_clear_step_kernel() { g_noted = false; }

extern "C" int mcmc_abi_version(void) { return MCMC_ABI_VERSION; }
extern "C" int mcmc_device_count(int* count) {
    if (!count) return mcmc_set_error(MCMC_E_INVALID_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count = n;
    return MCMC_OK;
}

// ------------------------------------------------------------------ context
extern "C" int mcmc_ctx_create(int device, mcmc_ctx** out) {
    if (!out) return mcmc_set_error(MCMC_E_INVALID_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return mcmc_set_error(MCMC_E_HIP, "no HIP device available");
    if (device < 0 || device >= n) return mcmc_set_error(MCMC_E_INVALID_ARG, "device ordinal out of range");
    auto* c = new mcmc_ctx();
    c->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_err, sizeof(int32_t));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
    if (e != hipSuccess) {
        delete c;
        return mcmc_set_error(MCMC_E_HIP, std::string("context creation: ") + hipGetErrorString(e));
    }
    *out = c;
    return MCMC_OK;
}

extern "C" int mcmc_ctx_destroy(mcmc_ctx* ctx) {
    if (!ctx) return MCMC_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    dfree(ctx->d_err);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return MCMC_OK;
}

extern "C" int mcmc_ctx_synchronize(mcmc_ctx* ctx) {
    if (!ctx) return mcmc_set_error(MCMC_E_INVALID_ARG, "ctx is NULL");
    if (int r = set_device(ctx)) return r;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MCMC_OK;
}
