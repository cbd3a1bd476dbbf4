// slice.cpp -- slice_sample (slice_sample.jl:43-103) for a batch of independent chains: a function on a model's
// log-density, not an MCMCSampler, so it has no row in the sampler table and no mcmc_chains.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "internal.hpp"

using namespace mcmc;

// A long run is split into launches of whole iterations, at most this many each: a launch then stays far below any
// watchdog whatever niter is, and a chain's registers reach memory often enough for the split to cost nothing that can
// be measured.  Every draw is keyed by (chain, iteration, coordinate, draw), so the split changes no result.
static constexpr int64_t kSliceItersPerLaunch = 256;
static constexpr int64_t kSliceDefaultEvals = 4096, kSliceMaxEvals = 1 << 20;

static thread_local std::string g_slice_kernel;

extern "C" int mcmc_slice_validate(const mcmc_slice_cfg* cfg) {
    if (!cfg) return mcmc_set_error(MCMC_E_INVALID_ARG, "slice cfg is NULL");
    char buf[160];
    if (!(cfg->niter > 0)) {
        snprintf(buf, sizeof buf, "niter (%lld) should be > 0", (long long)cfg->niter);
        return mcmc_set_error(MCMC_E_INVALID_ARG, buf);
    }
    if (!(cfg->burnin >= 0)) {
        snprintf(buf, sizeof buf, "burnin (%lld) should be >= 0", (long long)cfg->burnin);
        return mcmc_set_error(MCMC_E_INVALID_ARG, buf);
    }
    if (!(cfg->iter_begin >= 0)) {
        snprintf(buf, sizeof buf, "iter_begin (%lld) should be >= 0", (long long)cfg->iter_begin);
        return mcmc_set_error(MCMC_E_INVALID_ARG, buf);
    }
    const int64_t lim = 0x100000000LL;
    if (cfg->niter >= lim || cfg->burnin >= lim || cfg->iter_begin >= lim ||
        cfg->iter_begin + cfg->burnin + cfg->niter >= lim)
        return mcmc_set_error(MCMC_E_INVALID_ARG, "iter_begin + burnin + niter should be < 2^32");
    if (cfg->max_evals != 0 && (cfg->max_evals < 3 || cfg->max_evals > kSliceMaxEvals)) {
        snprintf(buf, sizeof buf, "max_evals (%lld) should be in 3 .. 2^20, or 0 for the default %lld",
                 (long long)cfg->max_evals, (long long)kSliceDefaultEvals);
        return mcmc_set_error(MCMC_E_INVALID_ARG, buf);
    }
    return MCMC_OK;
}

// the plan of (kind, d, C), or the refusal's text
static int slice_plan_of(int32_t kind, int64_t d, int64_t C, LaunchPlan& p) {
    if (kind == MK_LOGISTIC || kind == MK_LINEAR || kind == MK_PROBIT)
        return mcmc_set_error(MCMC_E_UNSUPPORTED,
                              "slice_sample is not built for the regression models: a coordinate sweep would "
                              "re-evaluate X * beta in full for every coordinate");
    if (!plan_model(kind)) return mcmc_set_error(MCMC_E_UNSUPPORTED, "slice_sample: unknown model kind");
    if (d > kSliceMaxD) {
        char buf[96];
        snprintf(buf, sizeof buf, "slice_sample is built for d <= %d (d = %lld)", kSliceMaxD, (long long)d);
        return mcmc_set_error(MCMC_E_UNSUPPORTED, buf);
    }
    p = launch_plan(kind, 0, (int)d, C, false, OP_SLICE);
    if (!p.built) return mcmc_set_error(MCMC_E_UNSUPPORTED, "slice_sample: this model is not built at this d");
    return MCMC_OK;
}

extern "C" int mcmc_slice_plan(int32_t model_kind, int64_t d, int64_t nchains, char* name, int64_t cap,
                               int32_t* threads, int64_t* grid) {
    if (d < 1) return mcmc_set_error(MCMC_E_INVALID_ARG, "model size d should be > 0");
    if (nchains < 1) return mcmc_set_error(MCMC_E_INVALID_ARG, "nchains should be > 0");
    LaunchPlan p;
    if (int r = slice_plan_of(model_kind, d, nchains, p)) return r;
    if (name && cap > 0) plan_kernel_name(name, (size_t)cap, p.k, plan_model(model_kind)->name);
    if (threads) *threads = p.k.threads;
    if (grid) *grid = p.grid;
    return MCMC_OK;
}

extern "C" int mcmc_slice_last_kernel(char* buf, int64_t cap) {
    if (!buf || cap <= 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL buffer");
    snprintf(buf, (size_t)cap, "%s", g_slice_kernel.c_str());
    return MCMC_OK;
}

extern "C" int mcmc_run_slice(mcmc_model* m, const mcmc_slice_cfg* cfg, int64_t nchains, int64_t chain_offset,
                              uint64_t seed, const double* init_x, const double* widths, int32_t on_device,
                              double* samples, double* final_x, double* final_lp, int32_t* info, int64_t* evals,
                              double* runtime_s, double* kernel_ms) {
    if (!m || !cfg) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    if (int r = mcmc_slice_validate(cfg)) return r;
    if (nchains < 1) return mcmc_set_error(MCMC_E_INVALID_ARG, "nchains should be > 0");
    if (chain_offset < 0 || chain_offset + nchains > 0x100000000LL)
        return mcmc_set_error(MCMC_E_INVALID_ARG, "chain ids exceed 2^32");
    const int d = m->args.d;
    LaunchPlan plan;
    if (int r = slice_plan_of(m->args.kind, d, nchains, plan)) return r;
    // a sample row's byte offsets are 32-bit in the pair mapping (samplers.hpp PairChain::store_kept)
    if ((int64_t)d * nchains * 8 >= 0x100000000LL)
        return mcmc_set_error(MCMC_E_INVALID_ARG, "d * nchains * 8 should be < 2^32: split the chains over calls");
    std::vector<double> w((size_t)d, 1.0);                  // widths = ones(length(initial)) (slice_sample.jl:44)
    if (widths)
        for (int j = 0; j < d; ++j) {
            if (!(std::isfinite(widths[j]) && widths[j] > 0.0)) {
                char buf[96];
                snprintf(buf, sizeof buf, "widths[%d] should be finite and > 0", j);
                return mcmc_set_error(MCMC_E_INVALID_ARG, buf);
            }
            w[(size_t)j] = widths[j];
        }
    mcmc_ctx* ctx = m->ctx;
    if (int r = set_device(ctx)) return r;
    hipStream_t st = ctx->stream;
    const int64_t C = nchains, ld = ld_for(LAYOUT_LPC, C, d);
    const size_t N = (size_t)C, nd = (size_t)d * N;
    const size_t nrows = (size_t)cfg->niter;
    double *dx = nullptr, *dlp = nullptr, *dw = nullptr, *dcols = nullptr, *dsamp = on_device ? samples : nullptr;
    int32_t* dinfo = nullptr;
    unsigned long long* dev = nullptr;
    DevScope tmp(st);
    const auto t0 = std::chrono::steady_clock::now();
    float ms = 0;
    unsigned long long nev = 0;
    auto run = [&]() -> int {
        int rc = MCMC_OK;
        if ((rc = tmp.alloc(&dx, (size_t)d * ld)) || (rc = tmp.alloc(&dlp, (size_t)ld)) ||
            (rc = tmp.alloc(&dinfo, (size_t)ld)) || (rc = tmp.alloc(&dw, (size_t)d)) || (rc = tmp.alloc(&dev, 1)) ||
            (rc = tmp.alloc(&dcols, nd)))
            return rc;
        if (!on_device && samples && (rc = tmp.alloc(&dsamp, nrows * nd))) return rc;
        hipError_t e = hipMemsetAsync(ctx->d_err, 0, sizeof(int32_t), st);
        if (e == hipSuccess) e = dzero(ctx, dev, sizeof *dev);
        if (e == hipSuccess) e = dzero(ctx, dinfo, (size_t)ld * 4);
        if (e == hipSuccess) e = dzero(ctx, dx, (size_t)d * ld * 8);
        if (e == hipSuccess) e = dzero(ctx, dlp, (size_t)ld * 8);
        if (e == hipSuccess) e = h2d(ctx, dw, w.data(), (size_t)d * 8);
        if (e == hipSuccess) {
            if (init_x && on_device) e = mcmc_copy_cols(dx, ld, init_x, C, d, C, st);
            else if (init_x) {
                e = h2d(ctx, dcols, init_x, nd * 8);
                if (e == hipSuccess) e = mcmc_copy_cols(dx, ld, dcols, C, d, C, st);
            } else e = mcmc_broadcast_cols(dx, ld, m->d_init, d, C, st);
        }
        // log_Px = logdist(state) (slice_sample.jl:52); a start out of support sets the error word
        if (e == hipSuccess) e = launch_eval(LAYOUT_LPC, base_args(m, C, ld), dx, dlp, nullptr, 1, st);
        int32_t err = 0;
        if (e == hipSuccess) e = d2h(ctx, &err, ctx->d_err, sizeof err);
        if (e != hipSuccess) return mcmc_set_error(MCMC_E_HIP, std::string("slice_sample: ") + hipGetErrorString(e));
        if (err)
            return mcmc_set_error(MCMC_E_INIT_OUT_OF_SUPPORT, "Initial values out of model support, try other values");
        SliceKernelArgs a{};
        a.m = m->args;
        SliceArgs& s = a.s;
        s.C = C;
        s.ld = ld;
        s.d = d;
        s.chain0 = (uint32_t)chain_offset;
        s.key0 = (uint32_t)seed;
        s.key1 = (uint32_t)(seed >> 32);
        s.iter_begin = cfg->iter_begin;
        s.keep_after = cfg->iter_begin + cfg->burnin;
        s.step_out = cfg->step_out != 0;
        s.max_evals = (int32_t)(cfg->max_evals ? cfg->max_evals : kSliceDefaultEvals);
        s.widths = dw;
        s.x = dx;
        s.lp = dlp;
        s.info = dinfo;
        s.samples = dsamp;
        s.n_evals = dev;
        const int64_t total = cfg->burnin + cfg->niter;
        mcmc_clear_step_kernel();
        e = hipEventRecord(ctx->ev0, st);
        for (int64_t done = 0; e == hipSuccess && done < total; done += kSliceItersPerLaunch) {
            s.iter_first = cfg->iter_begin + 1 + done;
            s.niters = (int32_t)std::min(kSliceItersPerLaunch, total - done);
            e = mcmc_launch_slice(a, st);
        }
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
        g_slice_kernel = mcmc_last_step_kernel();
        if (e == hipSuccess) e = d2h(ctx, &nev, dev, sizeof nev);
        if (e == hipSuccess && samples && !on_device) e = d2h(ctx, samples, dsamp, nrows * nd * 8);
        if (e == hipSuccess && final_x) {
            if (on_device) e = mcmc_copy_cols(final_x, C, dx, ld, d, C, st);
            else {
                e = mcmc_copy_cols(dcols, C, dx, ld, d, C, st);
                if (e == hipSuccess) e = d2h(ctx, final_x, dcols, nd * 8);
            }
        }
        const hipMemcpyKind back = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (e == hipSuccess && final_lp) e = hipMemcpyAsync(final_lp, dlp, N * 8, back, st);
        if (e == hipSuccess && info) e = hipMemcpyAsync(info, dinfo, N * 4, back, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return mcmc_set_error(MCMC_E_HIP, std::string("slice_sample: ") + hipGetErrorString(e));
        return MCMC_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(st);
    if (runtime_s) *runtime_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (kernel_ms) *kernel_ms = ms;
    if (evals) *evals = rc == MCMC_OK ? (int64_t)nev + C : 0;
    return rc;
}
