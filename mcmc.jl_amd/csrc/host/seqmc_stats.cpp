// seqmc_stats.cpp -- the population runner (SeqMC.jl:21-122), the statistics calls and the debug probes.
#include <chrono>
#include <cstdio>

#include "internal.hpp"

using namespace mcmc;

extern "C" int mcmc_seqmc_validate(const mcmc_seqmc_cfg* cfg) {
    if (!cfg) return mcmc_set_error(MCMC_E_INVALID_ARG, "seqmc cfg is NULL");
    char buf[160];
    if (!(cfg->burnin >= 0)) {
        snprintf(buf, sizeof buf, "Burnin rounds (%lld) should be >= 0", (long long)cfg->burnin);        // SeqMC.jl:30
        return mcmc_set_error(MCMC_E_INVALID_ARG, buf);
    }
    if (!(cfg->steps > cfg->burnin)) {
        snprintf(buf, sizeof buf, "Steps (%lld) should be > to burnin (%lld)", (long long)cfg->steps,
                 (long long)cfg->burnin);                                                                 // SeqMC.jl:31
        return mcmc_set_error(MCMC_E_INVALID_ARG, buf);
    }
    return MCMC_OK;
}

// One sampler step of every chain of `c` from its current state, nothing kept (the SamplerTask's
// `consume` inside run_seqmc, SeqMC.jl:69).
int step_once(mcmc_chains* c, hipStream_t st) {
    KernelArgs a = step_args(c, {0, 1, 1, 0});             // a run of one step, nothing kept; the tuners' burnin 0
    a.s.step_begin = c->steps_done + 1;
    a.s.nsteps = 1;
    HIP_TRY(launch_chain_step(c, a, st));
    if (c->si->evals_on_host) c->h_evals += c->C;
    c->steps_done += 1;
    return MCMC_OK;
}

extern "C" int mcmc_run_seqmc(mcmc_chains* const* targets, int32_t ntargets, int64_t npart, const double* particles,
                              const mcmc_seqmc_cfg* cfg, uint64_t seed, int32_t on_device, double* samples,
                              double* weights, int32_t* resampled, double* runtime_s) {
    if (!targets || ntargets < 1 || !particles || !cfg) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    if (int r = mcmc_seqmc_validate(cfg)) return r;
    if (npart < 1) return mcmc_set_error(MCMC_E_INVALID_ARG, "need at least one particle");
    for (int t = 0; t < ntargets; ++t)
        if (!targets[t]) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL target");
    mcmc_ctx* ctx = targets[0]->model->ctx;
    const int d = targets[0]->model->args.d;
    for (int t = 0; t < ntargets; ++t) {
        if (targets[t]->model->args.d != d)
            return mcmc_set_error(MCMC_E_INVALID_ARG, "Models do not have the same parameter vector size");  // SeqMC.jl:49
        if (targets[t]->model->ctx != ctx) return mcmc_set_error(MCMC_E_INVALID_ARG, "targets live on different contexts");
        if (targets[t]->C != npart) return mcmc_set_error(MCMC_E_INVALID_ARG, "every target needs nchains == npart");
        if (const char* why = targets[t]->si->seqmc_refusal) return mcmc_set_error(MCMC_E_UNSUPPORTED, why);
    }
    if (cfg->steps > 0xffffffffLL) return mcmc_set_error(MCMC_E_INVALID_ARG, "steps exceed 2^32");
    if (int r = set_device(ctx)) return r;
    hipStream_t st = ctx->stream;
    const size_t nd = (size_t)d * (size_t)npart, N = (size_t)npart;
    const int64_t nstore = cfg->steps - cfg->burnin;
    double *parsA = nullptr, *parsB = nullptr, *logW = nullptr, *lt = nullptr, *lt2 = nullptr, *ll0 = nullptr,
           *cp = nullptr, *dsamp = on_device ? samples : nullptr, *dw = on_device ? weights : nullptr;
    int32_t* flags = nullptr;
    DevScope tmp(st);
    auto t0 = std::chrono::steady_clock::now();
    auto run = [&]() -> int {
        int rc = MCMC_OK;
        if ((rc = tmp.alloc(&parsA, nd)) || (rc = tmp.alloc(&parsB, nd)) || (rc = tmp.alloc(&logW, N)) ||
            (rc = tmp.alloc(&lt, N)) || (rc = tmp.alloc(&lt2, N)) || (rc = tmp.alloc(&ll0, N)) ||
            (rc = tmp.alloc(&cp, N)) || (rc = tmp.alloc(&flags, (size_t)cfg->steps * ntargets)))
            return rc;
        if (!on_device && ((samples && (rc = tmp.alloc(&dsamp, (size_t)nstore * nd))) ||
                           (weights && (rc = tmp.alloc(&dw, (size_t)nstore * N)))))
            return rc;
        hipError_t e = on_device ? hipMemcpyAsync(parsA, particles, nd * 8, hipMemcpyDeviceToDevice, st)
                                 : h2d(ctx, parsA, particles, nd * 8);
        if (e == hipSuccess) e = dzero(ctx, logW, N * 8);                       // logW = zeros(npart)
        if (e == hipSuccess) e = dzero(ctx, lt, N * 8);                         // logtarget = zeros(npart)
        for (int64_t i = 1; e == hipSuccess && i <= cfg->steps; ++i) {
            for (int t = 0; e == hipSuccess && t < ntargets; ++t) {
                mcmc_chains* c = targets[t];
                KernelArgs a = base_args(c->model, c->C, c->ld);
                // MCMC.reset(t, pars[n]): state <- particle, logtarget <- eval (RWM.jl:49, MALA.jl:75-78)
                e = cols_to_state(c->layout, c->st.x, c->ld, parsA, npart, d, npart, st);
                if (e == hipSuccess) e = launch_eval(c->layout, a, c->st.x, c->st.lp, c->st.g, 0, st);
                if (e == hipSuccess) e = hipMemcpyAsync(ll0, c->st.lp, N * 8, hipMemcpyDeviceToDevice, st);
                if (e != hipSuccess) break;
                if ((rc = step_once(c, st))) break;                             // sample = consume(t.task)
                e = state_to_cols(c->layout, parsA, npart, c->st.x, c->ld, d, npart, st);   // pars[n] = ppars
                if (e == hipSuccess) e = mcmc_seqmc_weights(npart, logW, ll0, lt, c->st.lp, st);
                int32_t* flag = flags + (size_t)(i - 1) * ntargets + t;
                if (e == hipSuccess) e = mcmc_seqmc_scan(npart, logW, cfg->trigger, cp, flag, st);
                if (e == hipSuccess)
                    e = mcmc_seqmc_resample(npart, d, cp, flag, seed, (uint32_t)i, (uint32_t)t, parsA, parsB, lt, lt2,
                                            logW, st);
                std::swap(parsA, parsB);
                std::swap(lt, lt2);
            }
            if (rc) return rc;
            if (e == hipSuccess) e = dzero(ctx, lt, N * 8);                     // logtarget = zeros(npart)
            if (e == hipSuccess && i > cfg->burnin && (dsamp || dw)) {
                const size_t row = (size_t)(i - cfg->burnin - 1);
                double* ps = dsamp ? dsamp + row * nd : parsB;                  // parsB: scratch when not wanted
                double* pw = dw ? dw + row * N : ll0;
                e = mcmc_seqmc_store(npart, d, parsA, logW, ps, pw, st);
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess && !on_device) {
            if (samples) e = d2h(ctx, samples, dsamp, (size_t)nstore * nd * 8);
            if (e == hipSuccess && weights) e = d2h(ctx, weights, dw, (size_t)nstore * N * 8);
        }
        if (e == hipSuccess && resampled) {
            e = on_device ? hipMemcpyAsync(resampled, flags, (size_t)cfg->steps * ntargets * 4, hipMemcpyDeviceToDevice, st)
                          : d2h(ctx, resampled, flags, (size_t)cfg->steps * ntargets * 4);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
        if (e != hipSuccess) return mcmc_set_error(MCMC_E_HIP, std::string("seqmc: ") + hipGetErrorString(e));
        return MCMC_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(st);
    if (runtime_s) *runtime_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

extern "C" int mcmc_stats_ess(mcmc_ctx* ctx, const double* samples, int64_t nkept, int64_t d, int64_t nchains,
                              int32_t vtype, int64_t maxlag, int64_t batchlen, int32_t on_device, double* ess,
                              double* var) {
    if (!ctx || !samples || !ess) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    if (vtype != MCMC_VAR_IMSE && vtype != MCMC_VAR_IPSE && vtype != MCMC_VAR_BM)       // ess.jl:7
        return mcmc_set_error(MCMC_E_INVALID_ARG, "Unknown ESS type " + std::to_string(vtype));
    if (nkept < 2 || d <= 0 || nchains <= 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "need nkept >= 2, d > 0, nchains > 0");
    if (d > 65535) return mcmc_set_error(MCMC_E_UNSUPPORTED, "d > 65535");
    if (maxlag <= 0) maxlag = nkept - 1;
    if (maxlag > nkept - 1) return mcmc_set_error(MCMC_E_INVALID_ARG, "maxlag should be < nkept");
    if (vtype == MCMC_VAR_BM && !(batchlen > 0 && nkept / batchlen > 1))                   // var.jl:22
        return mcmc_set_error(MCMC_E_INVALID_ARG, "Choose batch size such that the number of batches is greather than one");
    if (int r = set_device(ctx)) return r;
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)nkept * (size_t)d * (size_t)nchains, no = (size_t)d * (size_t)nchains;
    const double* ds = samples;
    double *dsb = nullptr, *de = ess, *dv = var;
    DevScope tmp(st);
    if (!on_device) {
        if (int rc = tmp.alloc(&dsb, ns)) return rc;
        if (int rc = tmp.alloc(&de, no)) return rc;
        if (int rc = tmp.alloc(&dv, var ? no : 0)) return rc;
        if (h2d(ctx, dsb, samples, ns * 8) != hipSuccess) return mcmc_set_error(MCMC_E_HIP, "samples upload failed");
        ds = dsb;
    }
    hipError_t e = mcmc_launch_ess(ds, nkept, d, nchains, vtype, maxlag, batchlen, de, dv, st);
    if (e == hipSuccess && !on_device) e = d2h(ctx, ess, de, no * 8);
    if (e == hipSuccess && !on_device && var) e = d2h(ctx, var, dv, no * 8);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return mcmc_set_error(MCMC_E_HIP, std::string("ess: ") + hipGetErrorString(e));
    return MCMC_OK;
}

extern "C" int mcmc_stats_describe(mcmc_ctx* ctx, const double* samples, int64_t nkept, int64_t d, int64_t nchains,
                                   int64_t maxlag, int32_t on_device, double* per_chain, const double* probs,
                                   int32_t nprobs, double* pooled, int64_t* nbad) {
    // the shape checks come first and need no device (tests/test_describe_cpu.py runs them without one)
    if (!per_chain && !pooled) return mcmc_set_error(MCMC_E_INVALID_ARG, "describe: ask for per_chain, pooled or both");
    if (nkept < 2 || d <= 0 || nchains <= 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "need nkept >= 2, d > 0, nchains > 0");
    if (d > 65535) return mcmc_set_error(MCMC_E_UNSUPPORTED, "d > 65535");
    if (maxlag <= 0) maxlag = nkept - 1;
    if (maxlag > nkept - 1) return mcmc_set_error(MCMC_E_INVALID_ARG, "maxlag should be < nkept");
    if (!pooled) nprobs = 0;
    if (nprobs < 0 || nprobs > MCMC_DESCRIBE_MAXPROBS)
        return mcmc_set_error(MCMC_E_INVALID_ARG, "describe: nprobs = " + std::to_string(nprobs) + " is not in 0.." +
                                            std::to_string(MCMC_DESCRIBE_MAXPROBS));
    if (nprobs > 0 && !probs) return mcmc_set_error(MCMC_E_INVALID_ARG, "describe: nprobs > 0 and probs is NULL");
    double hp[MCMC_DESCRIBE_MAXPROBS] = {0};
    auto probs_ok = [&]() {
        for (int i = 0; i < nprobs; ++i)
            if (!(hp[i] >= 0.0 && hp[i] <= 1.0))
                return mcmc_set_error(MCMC_E_INVALID_ARG, "describe: probability " + std::to_string(hp[i]) + " is not in [0, 1]");
        return (int)MCMC_OK;
    };
    if (!on_device) {
        for (int i = 0; i < nprobs; ++i) hp[i] = probs[i];
        if (int r = probs_ok()) return r;
    }
    if (!ctx || !samples) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    if (int r = set_device(ctx)) return r;
    hipStream_t st = ctx->stream;
    if (on_device && nprobs > 0) {
        if (d2h(ctx, hp, probs, (size_t)nprobs * 8) != hipSuccess) return mcmc_set_error(MCMC_E_HIP, "probs download failed");
        if (int r = probs_ok()) return r;
    }
    const size_t dC = (size_t)d * (size_t)nchains, ns = (size_t)nkept * dC;
    const size_t npool = (size_t)(MCMC_DESCRIBE_NPOOLED + nprobs) * (size_t)d;
    const double* ds = samples;
    double *dsb = nullptr, *dpc = per_chain, *dpo = pooled;
    int64_t* dnb = nbad;
    char* ws = nullptr;
    DevScope tmp(st);
    if (!on_device) {
        if (int rc = tmp.alloc(&dsb, ns)) return rc;
        if (int rc = tmp.alloc(&dpc, per_chain ? 6 * dC : 0)) return rc;
        if (int rc = tmp.alloc(&dpo, pooled ? npool : 0)) return rc;
        if (int rc = tmp.alloc(&dnb, pooled && nbad ? (size_t)d : 0)) return rc;
        if (h2d(ctx, dsb, samples, ns * 8) != hipSuccess) return mcmc_set_error(MCMC_E_HIP, "samples upload failed");
        ds = dsb;
    }
    if (int rc = tmp.alloc(&ws, mcmc_describe_ws_bytes(d, nchains, per_chain != nullptr, pooled != nullptr, nprobs)))
        return rc;
    hipError_t e = mcmc_launch_describe(ds, nkept, d, nchains, maxlag, dpc, hp, nprobs, dpo, pooled ? dnb : nullptr, ws,
                                        st);
    if (e == hipSuccess && !on_device && per_chain) e = d2h(ctx, per_chain, dpc, 6 * dC * 8);
    if (e == hipSuccess && !on_device && pooled) e = d2h(ctx, pooled, dpo, npool * 8);
    if (e == hipSuccess && !on_device && pooled && nbad) e = d2h(ctx, nbad, dnb, (size_t)d * 8);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return mcmc_set_error(MCMC_E_HIP, std::string("describe: ") + hipGetErrorString(e));
    return MCMC_OK;
}

extern "C" int mcmc_stats_zv(mcmc_ctx* ctx, int32_t order, const double* samples, const double* grads, int64_t nkept,
                             int64_t d, int64_t nchains, int32_t on_device, double* zv, double* coef, int32_t* info) {
    if (!ctx || !samples || !grads || !zv) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    if (order != MCMC_ZV_LINEAR && order != MCMC_ZV_QUADRATIC)
        return mcmc_set_error(MCMC_E_INVALID_ARG, "Unknown ZV order " + std::to_string(order));
    if (d <= 0 || nchains <= 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "need d > 0, nchains > 0");
    if (d > mcmc_zv_max_d(order))
        return mcmc_set_error(MCMC_E_UNSUPPORTED, std::string(order == MCMC_ZV_LINEAR ? "linear" : "quadratic") +
                                            " ZV is built for d <= " + std::to_string(mcmc_zv_max_d(order)) +
                                            " (d = " + std::to_string(d) + ")");
    const int64_t k = mcmc_zv_k(order, d);
    if (nkept <= k)                                        // the centred Gram matrix has rank <= nkept - 1
        return mcmc_set_error(MCMC_E_INVALID_ARG, "ZV needs nkept > k = " + std::to_string(k) + " control variates (nkept = " +
                                            std::to_string(nkept) + ")");
    if (int r = set_device(ctx)) return r;
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)nkept * (size_t)d * (size_t)nchains, nc = (size_t)k * (size_t)d * (size_t)nchains;
    const double *dx = samples, *dg = grads;
    double *dxb = nullptr, *dgb = nullptr, *dzb = nullptr, *dcb = nullptr, *dz = zv, *dc = coef;
    int32_t *dib = nullptr, *di = info;
    DevScope tmp(st);
    if (!on_device) {
        if (int rc = tmp.alloc(&dxb, ns)) return rc;
        if (int rc = tmp.alloc(&dgb, ns)) return rc;
        if (int rc = tmp.alloc(&dzb, ns)) return rc;
        if (int rc = tmp.alloc(&dcb, coef ? nc : 0)) return rc;
        if (int rc = tmp.alloc(&dib, info ? (size_t)nchains : 0)) return rc;
        if (h2d(ctx, dxb, samples, ns * 8) != hipSuccess || h2d(ctx, dgb, grads, ns * 8) != hipSuccess)
            return mcmc_set_error(MCMC_E_HIP, "samples / gradients upload failed");
        dx = dxb, dg = dgb, dz = dzb, dc = dcb, di = dib;
    }
    hipError_t e = mcmc_launch_zv(order, dx, dg, nkept, (int)d, nchains, dz, dc, di, st);
    if (e == hipSuccess && !on_device) e = d2h(ctx, zv, dz, ns * 8);
    if (e == hipSuccess && !on_device && coef) e = d2h(ctx, coef, dc, nc * 8);
    if (e == hipSuccess && !on_device && info) e = d2h(ctx, info, di, (size_t)nchains * 4);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return mcmc_set_error(MCMC_E_HIP, std::string("zv: ") + hipGetErrorString(e));
    return MCMC_OK;
}

static int probe_result(hipError_t e, const char* what) {
    if (e != hipSuccess) return mcmc_set_error(MCMC_E_HIP, std::string(what) + " probe: " + hipGetErrorString(e));
    return MCMC_OK;
}

extern "C" int mcmc_debug_detmath(mcmc_ctx* ctx, int op, int64_t n, const double* x, const double* y, double* out) {
    if (!ctx || !x || !out || n <= 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "bad argument");
    if (int r = set_device(ctx)) return r;
    const size_t nout = (op == 6) ? 4 * (size_t)n : (size_t)n;
    double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    DevScope tmp(ctx->stream);
    if (int rc = tmp.alloc(&dx, (size_t)n)) return rc;
    if (int rc = tmp.alloc(&dy, (size_t)n)) return rc;
    if (int rc = tmp.alloc(&dout, nout)) return rc;
    hipError_t e = h2d(ctx, dx, x, (size_t)n * 8);
    if (e == hipSuccess && y) e = h2d(ctx, dy, y, (size_t)n * 8);
    if (e == hipSuccess) e = mcmc_detmath(op, n, dx, dy, dout, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = d2h(ctx, out, dout, nout * 8);
    return probe_result(e, "detmath");
}

extern "C" int mcmc_debug_philox(mcmc_ctx* ctx, int64_t n, const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
    if (!ctx || !ctr || !key || !out || n <= 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "bad argument");
    if (int r = set_device(ctx)) return r;
    uint32_t *dc = nullptr, *dk = nullptr, *dout = nullptr;
    DevScope tmp(ctx->stream);
    if (int rc = tmp.alloc(&dc, 4 * (size_t)n)) return rc;
    if (int rc = tmp.alloc(&dk, 2 * (size_t)n)) return rc;
    if (int rc = tmp.alloc(&dout, 4 * (size_t)n)) return rc;
    hipError_t e = h2d(ctx, dc, ctr, 16 * (size_t)n);
    if (e == hipSuccess) e = h2d(ctx, dk, key, 8 * (size_t)n);
    if (e == hipSuccess) e = mcmc_philox(n, dc, dk, dout, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = d2h(ctx, out, dout, 16 * (size_t)n);
    return probe_result(e, "philox");
}

extern "C" int mcmc_debug_mfma_f64(mcmc_ctx* ctx, int nk, const double* A, const double* B, const double* C,
                                   double* D) {
    if (!ctx || !A || !B || !C || !D || nk <= 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "bad argument");
    if (int r = set_device(ctx)) return r;
    double *dA = nullptr, *dB = nullptr, *dC = nullptr, *dD = nullptr;
    DevScope tmp(ctx->stream);
    if (int rc = tmp.alloc(&dA, 64 * (size_t)nk)) return rc;
    if (int rc = tmp.alloc(&dB, 64 * (size_t)nk)) return rc;
    if (int rc = tmp.alloc(&dC, 256)) return rc;
    if (int rc = tmp.alloc(&dD, 256)) return rc;
    hipError_t e = h2d(ctx, dA, A, 512 * (size_t)nk);
    if (e == hipSuccess) e = h2d(ctx, dB, B, 512 * (size_t)nk);
    if (e == hipSuccess) e = h2d(ctx, dC, C, 2048);
    if (e == hipSuccess) e = mcmc_mfma_probe(dA, dB, dC, dD, nk, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = d2h(ctx, D, dD, 2048);
    return probe_result(e, "mfma");
}

