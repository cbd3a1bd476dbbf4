// serialtemp.cpp -- the serial-tempering runner (SerialTempMC.jl:16-85): nwalkers independent walkers as one batch.
#include <chrono>
#include <cstdio>
#include <cstring>

#include "internal.hpp"

using namespace mcmc;

extern "C" int mcmc_serialtempmc_validate(const mcmc_serialtempmc_cfg* cfg) {
    if (!cfg) return mcmc_set_error(MCMC_E_INVALID_ARG, "serialtempmc cfg is NULL");
    char buf[160];
    if (!(cfg->burnin >= 0)) {
        snprintf(buf, sizeof buf, "Burnin rounds (%lld) should be >= 0", (long long)cfg->burnin);   // SerialTempMC.jl:22
        return mcmc_set_error(MCMC_E_INVALID_ARG, buf);
    }
    if (!(cfg->steps > cfg->burnin)) {
        snprintf(buf, sizeof buf, "Steps (%lld) should be > to burnin (%lld)", (long long)cfg->steps,
                 (long long)cfg->burnin);                                                            // SerialTempMC.jl:23
        return mcmc_set_error(MCMC_E_INVALID_ARG, buf);
    }
    if (cfg->swap_period < 1) {                            // the reference would throw out of i % swapPeriod
        snprintf(buf, sizeof buf, "swapPeriod (%lld) should be >= 1", (long long)cfg->swap_period);
        return mcmc_set_error(MCMC_E_INVALID_ARG, buf);
    }
    if (cfg->steps > 0xffffffffLL) return mcmc_set_error(MCMC_E_INVALID_ARG, "steps exceed 2^32");
    return MCMC_OK;
}

// a sampler SeqMC refuses is refused for the same reason (both runners reset a target before every step): the
// table's text with this runner's name in front
static std::string stemp_refusal(const SamplerInfo* si) {
    const char* why = std::strchr(si->seqmc_refusal, ':');
    return std::string("SerialTempMC does not run ") + si->name + " targets" + (why ? why : "");
}

extern "C" int mcmc_run_serialtempmc(mcmc_chains* const* targets, int32_t ntargets, int64_t nwalkers,
                                     const mcmc_serialtempmc_cfg* cfg, const double* logW, uint64_t seed,
                                     int32_t on_device, double* samples, int32_t* models, uint64_t* swap_bits,
                                     int32_t* final_at, double* runtime_s) {
    if (!targets || !cfg) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    if (int r = mcmc_serialtempmc_validate(cfg)) return r;
    if (ntargets < 2) return mcmc_set_error(MCMC_E_INVALID_ARG, "serial tempering needs at least two targets");
    if (nwalkers < 1) return mcmc_set_error(MCMC_E_INVALID_ARG, "need at least one walker");
    for (int t = 0; t < ntargets; ++t)
        if (!targets[t]) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL target");
    mcmc_ctx* ctx = targets[0]->model->ctx;
    const int d = targets[0]->model->args.d;
    for (int t = 0; t < ntargets; ++t) {
        const mcmc_chains* c = targets[t];
        if (c->model->args.d != d)
            return mcmc_set_error(MCMC_E_INVALID_ARG, "Models do not have the same parameter vector size");  // SerialTempMC.jl:39
        if (c->model->ctx != ctx) return mcmc_set_error(MCMC_E_INVALID_ARG, "targets live on different contexts");
        if (c->C != nwalkers) return mcmc_set_error(MCMC_E_INVALID_ARG, "every target needs nchains == nwalkers");
        if (c->offset != targets[0]->offset)
            return mcmc_set_error(MCMC_E_INVALID_ARG, "every target needs the same chain offset");
        if (c->si->seqmc_refusal) return mcmc_set_error(MCMC_E_UNSUPPORTED, stemp_refusal(c->si));
        if (c->steps_done + cfg->steps + 1 > 0xffffffffLL)
            return mcmc_set_error(MCMC_E_INVALID_ARG, "step counter exceeds 2^32");
    }
    if (int r = set_device(ctx)) return r;
    hipStream_t st = ctx->stream;
    const int64_t C = nwalkers;
    const size_t N = (size_t)C, nd = (size_t)d * N, nw = (N + 63) / 64;
    const size_t nstore = (size_t)(cfg->steps - cfg->burnin);
    const uint32_t chain0 = (uint32_t)targets[0]->offset;
    double *cur = nullptr, *prev = nullptr, *cand = nullptr, *xcols = nullptr, *lt = nullptr, *cand_lt = nullptr,
           *ll0 = nullptr, *dlogW = nullptr, *dsamp = on_device ? samples : nullptr;
    int32_t *at = nullptr, *tgt = nullptr, *swapped = nullptr, *dmod = on_device ? models : nullptr;
    uint64_t* dbits = on_device ? swap_bits : nullptr;
    bool wave = false;
    for (int t = 0; t < ntargets; ++t) wave = wave || targets[t]->layout == LAYOUT_WPC;
    std::vector<double> hW((size_t)ntargets, 0.0);         // logW = zeros(nmods) (SerialTempMC.jl:49)
    if (logW) hW.assign(logW, logW + ntargets);
    DevScope tmp(st);
    auto t0 = std::chrono::steady_clock::now();
    auto run = [&]() -> int {
        int rc = MCMC_OK;
        if ((rc = tmp.alloc(&cur, nd)) || (rc = tmp.alloc(&prev, nd)) || (rc = tmp.alloc(&cand, nd)) ||
            (rc = tmp.alloc(&xcols, wave ? nd : 0)) || (rc = tmp.alloc(&lt, N)) || (rc = tmp.alloc(&cand_lt, N)) ||
            (rc = tmp.alloc(&ll0, N)) || (rc = tmp.alloc(&dlogW, (size_t)ntargets)) || (rc = tmp.alloc(&at, N)) ||
            (rc = tmp.alloc(&tgt, N)) || (rc = tmp.alloc(&swapped, N)))
            return rc;
        if (!on_device && ((samples && (rc = tmp.alloc(&dsamp, nstore * nd))) ||
                           (models && (rc = tmp.alloc(&dmod, nstore * N))) ||
                           (swap_bits && (rc = tmp.alloc(&dbits, nstore * nw)))))
            return rc;
        hipError_t e = h2d(ctx, dlogW, hW.data(), (size_t)ntargets * 8);
        if (e == hipSuccess) e = dzero(ctx, at, N * 4);                         // at = 1: the first task
        // s = consume(tasks[at].task) (SerialTempMC.jl:51): one step of target 0 from where its chains stand
        {
            mcmc_chains* c = targets[0];
            if (e == hipSuccess) e = state_to_cols(c->layout, prev, C, c->st.x, c->ld, d, C, st);
            if (e == hipSuccess) e = hipMemcpyAsync(lt, c->st.lp, N * 8, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess && (rc = step_once(c, st))) return rc;
            if (e == hipSuccess) e = state_to_cols(c->layout, cur, C, c->st.x, c->ld, d, C, st);
        }
        for (int64_t i = 1; e == hipSuccess && i <= cfg->steps; ++i) {
            const int32_t is_swap = i % cfg->swap_period == 0;
            e = mcmc_stemp_pick(C, ntargets, chain0, seed, (uint32_t)i, is_swap, at, tgt, st);
            // a swap resets the other task to s.pars (SerialTempMC.jl:62); the walker's own task stands at s.ppars
            const double* from = is_swap ? prev : cur;
            for (int t = 0; e == hipSuccess && t < ntargets; ++t) {
                mcmc_chains* c = targets[t];
                KernelArgs a = base_args(c->model, c->C, c->ld);
                e = cols_to_state(c->layout, c->st.x, c->ld, from, C, d, C, st);
                if (e == hipSuccess) e = launch_eval(c->layout, a, c->st.x, c->st.lp, c->st.g, 0, st);
                if (e == hipSuccess) e = hipMemcpyAsync(ll0, c->st.lp, N * 8, hipMemcpyDeviceToDevice, st);
                if (e != hipSuccess) break;
                if ((rc = step_once(c, st))) return rc;
                const double* x = c->st.x;                  // lane and regression layouts: columns as they are
                int64_t ldx = c->ld;
                if (c->layout == LAYOUT_WPC) {
                    e = state_to_cols(c->layout, xcols, C, c->st.x, c->ld, d, C, st);
                    x = xcols;
                    ldx = C;
                }
                if (e == hipSuccess) e = mcmc_stemp_take(C, d, t, tgt, x, ldx, ll0, cand, cand_lt, st);
            }
            if (e == hipSuccess)
                e = mcmc_stemp_swap(C, d, chain0, seed, (uint32_t)i, is_swap, dlogW, at, tgt, cur, prev, lt, cand,
                                    cand_lt, swapped, st);
            if (e == hipSuccess && i > cfg->burnin && (dsamp || dmod || dbits)) {
                const size_t row = (size_t)(i - cfg->burnin - 1);
                e = mcmc_stemp_store(C, d, cur, at, swapped, dsamp ? dsamp + row * nd : nullptr,
                                     dmod ? dmod + row * N : nullptr, dbits ? dbits + row * nw : nullptr, st);
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess && !on_device) {
            if (samples) e = d2h(ctx, samples, dsamp, nstore * nd * 8);
            if (e == hipSuccess && models) e = d2h(ctx, models, dmod, nstore * N * 4);
            if (e == hipSuccess && swap_bits) e = d2h(ctx, swap_bits, dbits, nstore * nw * 8);
        }
        if (e == hipSuccess && final_at) {
            e = on_device ? hipMemcpyAsync(final_at, at, N * 4, hipMemcpyDeviceToDevice, st) : d2h(ctx, final_at, at, N * 4);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
        if (e != hipSuccess) return mcmc_set_error(MCMC_E_HIP, std::string("serialtempmc: ") + hipGetErrorString(e));
        return MCMC_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(st);
    if (runtime_s) *runtime_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}
