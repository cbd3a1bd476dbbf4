// chains.cpp -- chain batches: their state buffers (walked from the chain-state table, tables.hpp), create / fork /
// reset / set_state, and the getters and setters.
#include <algorithm>
#include <cstdio>

#include "internal.hpp"

using namespace mcmc;

int ensure(DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return MCMC_OK;
    dfree(b.p);
    b.p = nullptr;
    b.bytes = 0;
    if (bytes == 0) return MCMC_OK;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        return mcmc_set_error(MCMC_E_OOM, std::string("hipMalloc(") + std::to_string(bytes) + " B) for outputs: " +
                                              hipGetErrorString(e));
    }
    b.bytes = bytes;
    return MCMC_OK;
}

// RAM jump factor (ram.hpp): packed lower-triangular rows padded to the kernel's width + a trash row, two halves.
// First element of column k in the wave layout's column-major packing (ram.hpp ram_wave_colstart)
static int64_t wave_colstart(int64_t k, int64_t d) { return k * d - k * (k - 1) / 2; }

// what the chain-state table's sizes and predicates read of a batch
static StateDims state_dims(const mcmc_chains* c) {
    const int d = c->model->args.d;
    return {c->si, c->sa.tuner, c->layout, d, c->C, c->ld, c->layout == LAYOUT_GLM ? mcmc_glm_d_pad(d) : 0,
            c->sa.n_leaps, c->st.ram_hs};
}

static void free_state(mcmc_chains* c) {
    for (const StateBuf& b : kStateTable) dfree(state_get(c->st, b));
    c->st = ChainState{};
}

// Put every chain at its start and reset the sampler's state (SamplerTask initialisation).
static int init_state(mcmc_chains* c) {
    mcmc_model* m = c->model;
    mcmc_ctx* ctx = m->ctx;
    const int d = m->args.d;
    const SamplerArgs& sa = c->sa;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemsetAsync(ctx->d_err, 0, sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(c->d_evals, 0, sizeof(unsigned long long), st));
    c->h_evals = 0;
    if (c->d_init_x) {
        HIP_TRY(cols_to_state(c->layout, c->st.x, c->ld, c->d_init_x, c->C, d, c->C, st));
    } else if (c->layout == LAYOUT_WPC) {       // chain-major [C][ld]
        HIP_TRY(mcmc_broadcast_rows(c->st.x, c->ld, m->d_init, d, c->C, st));
    } else {                                    // coordinate-major [d][ld] (LPC, GLM)
        HIP_TRY(mcmc_broadcast_cols(c->st.x, c->ld, m->d_init, d, c->C, st));
    }
    KernelArgs a = base_args(m, c->C, c->ld);
    if (c->si->manifold) {
        // evalallt at the start, invG and firstTerm = invG grad (SMMALA.jl:62-67); a failed pivot sets the error word
        HIP_TRY(mcmc_launch_smmala_eval(a, c->st.x, c->st.lp, c->st.g, c->st.sm_G, c->st.sm_invG, c->st.sm_ft, 1, st));
        if (sa.kind == SK_PMALA) {                 // sum(secondTerm, 2) of the start (PMALA.jl:77-80)
            KernelArgs ac = a;
            ac.st = c->st;
            HIP_TRY(mcmc_launch_pmala_corr(ac, st));
        }
        c->h_evals = c->C;
    } else {
        HIP_TRY(launch_eval(c->layout, a, c->st.x, c->st.lp, c->st.g, 1, st));
    }
    if (c->si->tuner_state == TUNE_DRIFT && sa.tuner) HIP_TRY(mcmc_fill_f64(c->st.t_step, c->C, sa.drift_step, st));
    if (c->si->tuner_state == TUNE_LEAP && sa.tuner) {   // EmpiricalHMCTune(nLeaps, leapStep, 0, 0)
        HIP_TRY(mcmc_fill_f64(c->st.t_step, c->C, sa.leap_step, st));
        HIP_TRY(mcmc_fill_i32(c->st.t_leaps, c->C, (int32_t)sa.n_leaps, st));
    }
    if (sa.kind == SK_HMCDA) {
        // initializeHMCDAStep returns 1 for every chain: state0.H is still NaN when it runs
        // (HMC.jl:88 ctor, HMCDA.jl:86-92), so p = NaN, a = -1 and the while loop never runs.
        HIP_TRY(mcmc_fill_f64(c->st.t_step, c->C, 1.0, st));
        HIP_TRY(mcmc_fill_f64(c->st.t_bar, c->C, 1.0, st));     // dualLeapStep = 1.
        HIP_TRY(mcmc_fill_f64(c->st.t_h, c->C, 0.0, st));       // dualH = 0.
    }
    if (sa.kind == SK_NUTS) {
        // the initial epsilon search and mu, hbar, lebar (NUTS.jl:71-82, 127-129), from the evaluated start; its
        // leapfrogs are counted (d_evals was zeroed above)
        HIP_TRY(mcmc_launch_nuts(step_args(c, {0, 1, 0, 0}), 1, st));
    }
    if (sa.kind == SK_RAM) {
        // S = diag(model.scale .* sampler.scale) (RAM.jl:51,55) in half 0: packed rows in 64-chain tiles
        // (ram.hpp), diagonal (r, r) at row r(r+1)/2 + r of every tile; the padding block d..dpad-1 is the identity
        const int64_t rl = c->st.ram_ld;
        HIP_TRY(hipMemsetAsync(c->st.ram_L, 0, 2 * (size_t)c->st.ram_hs * 8, st));
        if (c->ram_wave) {                                 // diagonal (k, k) at colstart(k) of every chain block
            for (int k = 0; k < d; ++k)
                HIP_TRY(mcmc_fill_f64_strided(c->st.ram_L + wave_colstart(k, d), c->st.ram_hs / rl, 1, rl,
                                              c->h_scale_eff[k], st));
        } else {
            const int64_t tile = (int64_t)(packed_rows(c->ram_dpad) + 1) * 64;
            for (int r = 0; r < c->ram_dpad; ++r)
                HIP_TRY(mcmc_fill_f64_strided(c->st.ram_L + (size_t)(r * (r + 1) / 2 + r) * 64, rl / 64, 64, tile,
                                              r < d ? c->h_scale_eff[r] : 1.0, st));
        }
    }
    if (sa.tuner) {
        HIP_TRY(mcmc_fill_i32(c->st.t_acc, c->C, 0, st));
        HIP_TRY(mcmc_fill_i32(c->st.t_prop, c->C, 0, st));
    }
    int32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, ctx->d_err, sizeof err, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (err) return mcmc_set_error(MCMC_E_INIT_OUT_OF_SUPPORT, "Initial values out of model support, try other values");
    c->steps_done = 0;
    return MCMC_OK;
}

extern "C" int mcmc_chains_create(mcmc_model* m, const mcmc_sampler_cfg* s, int64_t nchains, int64_t chain_offset,
                                  uint64_t seed, const double* init_x, mcmc_chains** out) {
    if (!m || !s || !out) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (int r = mcmc_sampler_validate(s)) return r;
    if (nchains <= 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "nchains should be > 0");
    if (chain_offset < 0 || chain_offset + nchains > (int64_t)0x100000000LL)
        return mcmc_set_error(MCMC_E_INVALID_ARG, "global chain ids must fit in 32 bits");
    if (s->kind == MCMC_RAM && m->args.d > mcmc_wpc_ram_max_d())
        return mcmc_set_error(MCMC_E_UNSUPPORTED, "RAM is built for d <= " + std::to_string(mcmc_wpc_ram_max_d()) +
                                        " (the d x d jump factor of every chain is kept in HBM)");
    const SamplerInfo& si = sampler_info(s->kind);
    const std::string needs = std::string(si.name) + " sampler requires model with ";
    if (si.needs >= 1 && !m->has_gradient) return mcmc_set_error(MCMC_E_NEEDS_GRADIENT, needs + "gradient function");
    if (si.needs >= 2 && m->has_gradient < 2) return mcmc_set_error(MCMC_E_NEEDS_GRADIENT, needs + "tensor function");
    if (si.needs >= 3 && m->has_gradient < 3)
        return mcmc_set_error(MCMC_E_NEEDS_GRADIENT, needs + "function of tensor derivatives");
    mcmc_ctx* ctx = m->ctx;
    if (int r = set_device(ctx)) return r;
    const int d = m->args.d;
    if (model_is_separable(m) && d > mcmc_wpc_max_d())
        return mcmc_set_error(MCMC_E_UNSUPPORTED, "separable targets support d <= 16384");
    if (si.d_reason && d > mcmc_smmala_max_d())
        return mcmc_set_error(MCMC_E_UNSUPPORTED, std::string(si.name) + " is built for d <= " +
                                            std::to_string(mcmc_smmala_max_d()) + si.d_reason + std::to_string(d));
    if (s->kind == MCMC_NUTS) {
        if (model_is_glm(m))
            return mcmc_set_error(MCMC_E_UNSUPPORTED, "NUTS is not built for the regression models (built: the separable and joint "
                                            "targets with d <= " + std::to_string(mcmc_nuts_max_d()) + ")");
        if (d > mcmc_nuts_max_d())
            return mcmc_set_error(MCMC_E_UNSUPPORTED, "NUTS is built for d <= " + std::to_string(mcmc_nuts_max_d()) +
                                                " (lane-per-chain and two-lanes-per-chain targets); d = " +
                                                std::to_string(d));
    }
    auto* c = new mcmc_chains();
    c->model = m;
    m->chains_alive += 1;
    c->C = nchains;
    c->layout = layout_for(m);
    c->ld = ld_for(c->layout, nchains, d);
    c->offset = chain_offset;
    c->seed = seed;
    c->cfg = *s;
    c->si = &si;
    SamplerArgs& sa = c->sa;                     // in SamplerArgs' member order (common.hpp)
    sa = SamplerArgs{s->kind, s->tuner, s->scale, s->drift_step, s->n_leaps, s->leap_step, s->rate, s->len,
                     s->shrinkage, s->t0, s->step, s->adapt_step, s->max_step, s->target_path, s->target_rate,
                     s->max_leaps > 0 ? s->max_leaps : (int64_t)1 << 20, si.newton_in_t0 ? (int32_t)s->t0 : 0};
    auto bail = [&](int code) {
        mcmc_chains_destroy(c);
        return code;
    };
    // scale = model.scale .* sampler.scale (RWM.jl:52); other samplers do not use it.
    std::vector<double> se(m->scale);
    if (sa.kind == SK_RWM || sa.kind == SK_RAM)                       // RAM.jl:51
        for (auto& v : se) v = v * sa.scale;
    c->h_scale_eff = se;
    if (sa.kind == SK_RAM) {
        // padded width: the lane-per-chain kernel's NC = 4 ceil(d/4), the regression kernel's DF = d_pad
        c->ram_wave = c->layout == LAYOUT_WPC || (c->layout == LAYOUT_GLM && d > 32);
        c->glm_ram_wave = c->layout == LAYOUT_GLM && d > 32;
        if (c->ram_wave) {
            // wave-per-chain: [half][chain][column-major packed factor] (ram.hpp wave layout), one block per chain of
            // every launched wave (8 chains per workgroup when two chains share a wave)
            c->ram_dpad = d;
            c->st.ram_ld = round_up((int64_t)packed_rows(d), 8);
            c->st.ram_hs = round_up(nchains, 8) * c->st.ram_ld;
        } else {
            c->ram_dpad = c->layout == LAYOUT_GLM ? mcmc_glm_d_pad(d) : (int)round_up(d, 4);
            c->st.ram_ld = round_up(nchains, 256);
            c->st.ram_hs = (int64_t)(packed_rows(c->ram_dpad) + 1) * c->st.ram_ld;
        }
    }
    const StateDims dims = state_dims(c);
    for (const StateBuf& b : kStateTable) {
        if (!b.exists(dims)) continue;
        void* p = nullptr;
        if (int r = dmalloc_bytes(&p, state_count(b, dims) * state_elem_bytes(b))) return bail(r);
        state_set(c->st, b, p);
    }
    if (c->glm_ram_wave) {                       // the buffers between the split step's kernels
        if (int r = dmalloc(&c->ram_u, (size_t)nchains * (size_t)mcmc_glm_ram_wave_ustride(d))) return bail(r);
        if (int r = dmalloc(&c->ram_nz, (size_t)nchains)) return bail(r);
        if (int r = dmalloc(&c->xprop, (size_t)d * c->ld)) return bail(r);
        if (int r = dmalloc(&c->lpp, (size_t)round_up(nchains, 64))) return bail(r);
    }
    c->scale1 = se.empty() ? 0.0 : se[0];
    c->scale_uniform = 1;
    for (double v : se)
        if (!(v == c->scale1)) c->scale_uniform = 0;   // bitwise-equal products only (NaN never)
    if (int r = dmalloc(&c->d_scale_eff, (size_t)round_up(d, 256))) return bail(r);
    if (int r = dmalloc(&c->d_evals, 1)) return bail(r);
    if (dzero(ctx, c->d_scale_eff, (size_t)round_up(d, 256) * 8) != hipSuccess ||
        h2d(ctx, c->d_scale_eff, se.data(), (size_t)d * 8) != hipSuccess)
        return bail(mcmc_set_error(MCMC_E_HIP, "scale upload failed"));
    if (init_x) {
        if (int r = dmalloc(&c->d_init_x, (size_t)d * nchains)) return bail(r);
        if (h2d(ctx, c->d_init_x, init_x, (size_t)d * nchains * 8) != hipSuccess)
            return bail(mcmc_set_error(MCMC_E_HIP, "init_x upload failed"));
    }
    if (int r = init_state(c)) return bail(r);
    *out = c;
    return MCMC_OK;
}

extern "C" int mcmc_chains_destroy(mcmc_chains* c) {
    if (!c) return MCMC_OK;
    (void)hipSetDevice(c->model->ctx->device);
    (void)hipStreamSynchronize(c->model->ctx->stream);
    free_state(c);
    for (void* p : {(void*)c->d_scale_eff, (void*)c->d_init_x, (void*)c->d_evals, (void*)c->ram_u, (void*)c->ram_nz,
                    (void*)c->xprop, (void*)c->lpp})
        dfree(p);
    for (const DevBuf* b : {&c->out_samples, &c->out_grads, &c->out_bits, &c->out_tmp, &c->stage_samples,
                            &c->stage_grads, &c->order_buf, &c->nuts_buf, &c->leap_buf})
        dfree(b->p);
    mcmc_model* m = c->model;
    delete c;
    if (--m->chains_alive == 0 && m->released) model_free(m);
    return MCMC_OK;
}

extern "C" int mcmc_chains_reset(mcmc_chains* c) {
    if (!c) return mcmc_set_error(MCMC_E_INVALID_ARG, "chains is NULL");
    if (int r = set_device(c->model->ctx)) return r;
    return init_state(c);
}

// MCMC.reset(t, x) (MCMC.jl:39): the task-local :reset hook of every sampler (RWM.jl:49, MALA.jl:75-80,
// HMC.jl:114-116, HMCDA.jl:82-83, RAM.jl:47) sets pars = x and re-evaluates the log-target (and gradient) there; the
// step counter, the tuners' state and RAM's factor are left as they are.  x: host [d][C]; lp (may be NULL): host [C],
// the log-targets at x.  A point out of support is accepted (the reference's hook does not assert): its log-target
// is -Inf and the next proposal's ratio decides.
extern "C" int mcmc_chains_set_state(mcmc_chains* c, const double* x, double* lp) {
    if (!c || !x) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    mcmc_model* m = c->model;
    mcmc_ctx* ctx = m->ctx;
    if (int r = set_device(ctx)) return r;
    const int d = m->args.d;
    const int64_t C = c->C;
    hipStream_t st = ctx->stream;
    DevScope tmp(st);
    double* dcols = nullptr;
    if (int r = tmp.alloc(&dcols, (size_t)d * C)) return r;
    hipError_t e = hipMemcpyAsync(dcols, x, (size_t)d * C * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = cols_to_state(c->layout, c->st.x, c->ld, dcols, C, d, C, st);
    KernelArgs a = base_args(m, C, c->ld);
    // SMMALA's :reset hook (SMMALA.jl:54-57) re-evaluates evalallt only: invG and firstTerm stay as they were; PMALA's
    // (PMALA.jl:63-66) likewise, secondTerm (the correction c) too
    if (e == hipSuccess && c->si->manifold)
        e = mcmc_launch_smmala_eval(a, c->st.x, c->st.lp, c->st.g, c->st.sm_G, nullptr, nullptr, 0, st);
    else if (e == hipSuccess) e = launch_eval(c->layout, a, c->st.x, c->st.lp, c->st.g, 0, st);
    if (e == hipSuccess && lp) e = hipMemcpyAsync(lp, c->st.lp, (size_t)C * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return mcmc_set_error(MCMC_E_HIP, std::string("set_state: ") + hipGetErrorString(e));
    c->h_evals += C;                                    // model.eval(pars) once per chain
    return MCMC_OK;
}

// fork's copy of RAM's factor: the one written last sits in half (steps_done & 1) of both batches (the step counter
// is copied)
static hipError_t fork_ram_factor(const mcmc_chains* src, mcmc_chains* c, int64_t first, int64_t count,
                                  hipStream_t st) {
    const size_t half = (size_t)(src->steps_done & 1);
    const double* sh = src->st.ram_L + half * (size_t)src->st.ram_hs;
    double* dh = c->st.ram_L + half * (size_t)c->st.ram_hs;
    if (c->ram_wave)                                       // [chain][ram_ld]
        return hipMemcpyAsync(dh, sh + (size_t)first * src->st.ram_ld, (size_t)count * c->st.ram_ld * 8,
                              hipMemcpyDeviceToDevice, st);
    // [64-chain tile][row][64]: re-tile on the host
    const size_t tile = (packed_rows(src->ram_dpad) + 1) * 64;
    std::vector<double> hs(((size_t)src->C + 63) / 64 * tile), hd(((size_t)count + 63) / 64 * tile, 0.0);
    hipError_t e = hipMemcpyAsync(hs.data(), sh, hs.size() * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hd.data(), dh, hd.size() * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    for (int64_t k = 0; k < count; ++k) {
        const size_t a = (size_t)(first + k), b = (size_t)k;
        for (size_t r = 0; r + 1 < tile / 64; ++r)
            hd[(b >> 6) * tile + r * 64 + (b & 63)] = hs[(a >> 6) * tile + r * 64 + (a & 63)];
    }
    e = hipMemcpyAsync(dh, hd.data(), hd.size() * 8, hipMemcpyHostToDevice, st);
    // hd leaves scope with the copy queued from pageable memory: wait for it here
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
}

// chains [first, first + count) of src as an independent batch: the same model, sampler and seed, global chain ids
// src's + first, and a copy of their whole state -- position, log-target, gradient, the tuners' per-chain state, RAM's
// factor and the step counter -- so running the new batch continues exactly those chains (their random streams are
// keyed by (seed, global chain, global step)), whatever src does afterwards.  Evaluation counts restart at 0.  Used
// for run(t::Array{MCMCTask}) on GPU tasks: one batched launch, then every returned MCMCChain's task continues its own
// chain (runners.jl:14).
extern "C" int mcmc_chains_fork(mcmc_chains* src, int64_t first, int64_t count, mcmc_chains** out) {
    if (!src || !out) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (first < 0 || count <= 0 || first + count > src->C)
        return mcmc_set_error(MCMC_E_INVALID_ARG, "fork: chains [" + std::to_string(first) + ", " + std::to_string(first + count) +
                                            ") are not inside the batch of " + std::to_string(src->C));
    mcmc_model* m = src->model;
    mcmc_ctx* ctx = m->ctx;
    if (int r = set_device(ctx)) return r;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipStreamSynchronize(st));
    const int d = m->args.d;
    std::vector<double> init;
    if (src->d_init_x) {                                   // the forked chains' own starts (resume restarts there)
        init.resize((size_t)d * count);
        HIP_TRY(hipMemcpy2DAsync(init.data(), (size_t)count * 8, src->d_init_x + first, (size_t)src->C * 8,
                                 (size_t)count * 8, (size_t)d, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    mcmc_chains* c = nullptr;
    if (int r = mcmc_chains_create(m, &src->cfg, count, src->offset + first, src->seed,
                                   init.empty() ? nullptr : init.data(), &c))
        return r;
    auto bail = [&](hipError_t e) {
        mcmc_chains_destroy(c);
        return mcmc_set_error(MCMC_E_HIP, std::string("fork: ") + hipGetErrorString(e));
    };
    // exactly the buffers live between steps (tables.hpp): chains [first, first + count) of each
    const StateDims dims = state_dims(c);
    const size_t dpitch = (size_t)c->ld * 8, spitch = (size_t)src->ld * 8;
    hipError_t e = hipSuccess;
    for (const StateBuf& b : kStateTable) {
        if (e != hipSuccess) break;
        if (!b.live || !b.exists(dims)) continue;
        char* dst = (char*)state_get(c->st, b);
        const char* from = (const char*)state_get(src->st, b);
        const size_t esz = state_elem_bytes(b);
        switch (b.shape) {
            case SHAPE_STATE:                              // per-chain rows, or per-coordinate rows
                e = c->layout == LAYOUT_WPC
                        ? hipMemcpyAsync(dst, from + (size_t)first * spitch, (size_t)count * dpitch,
                                         hipMemcpyDeviceToDevice, st)
                        : hipMemcpy2DAsync(dst, dpitch, from + (size_t)first * 8, spitch, (size_t)count * 8, (size_t)d,
                                           hipMemcpyDeviceToDevice, st);
                break;
            case SHAPE_PACKED:
                e = hipMemcpy2DAsync(dst, dpitch, from + (size_t)first * 8, spitch, (size_t)count * 8, packed_rows(d),
                                     hipMemcpyDeviceToDevice, st);
                break;
            case SHAPE_F64:
            case SHAPE_I32:
                e = hipMemcpyAsync(dst, from + (size_t)first * esz, (size_t)count * esz, hipMemcpyDeviceToDevice, st);
                break;
            case SHAPE_RAM: e = fork_ram_factor(src, c, first, count, st); break;
            default: break;                                // the remaining shapes are dead between steps
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return bail(e);
    HIP_TRY(hipMemsetAsync(c->d_evals, 0, sizeof(unsigned long long), st));   // NUTS: create's epsilon search counted
    HIP_TRY(hipStreamSynchronize(st));
    c->h_evals = 0;
    c->steps_done = src->steps_done;
    c->spl = src->spl;
    c->store_grads = src->store_grads;
    c->tuner_burnin = src->tuner_burnin;
    *out = c;
    return MCMC_OK;
}

extern "C" int mcmc_debug_chains_order(mcmc_chains* c, int32_t* used, int32_t* order) {
    if (!c || !used) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    *used = c->last_order ? 1 : 0;
    if (c->last_order && order) std::copy(c->h_order.begin(), c->h_order.end(), order);
    return MCMC_OK;
}

extern "C" int mcmc_chains_evals(mcmc_chains* c, int64_t* evals) {
    if (!c || !evals) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    mcmc_ctx* ctx = c->model->ctx;
    if (int r = set_device(ctx)) return r;
    unsigned long long v = 0;
    HIP_TRY(d2h(ctx, &v, c->d_evals, sizeof v));
    *evals = (int64_t)v + c->h_evals;
    return MCMC_OK;
}

// SMMALA / PMALA: the state beside pars and logTarget, host buffers (any may be NULL): grad, ft, c [d][C]; G, invG
// packed [d(d+1)/2][C]
extern "C" int mcmc_chains_manifold_state(mcmc_chains* c, double* grad, double* G, double* invG, double* ft,
                                          double* corr) {
    if (!c) return mcmc_set_error(MCMC_E_INVALID_ARG, "chains is NULL");
    if (!c->si->manifold) return mcmc_set_error(MCMC_E_INVALID_ARG, "chains do not run the SMMALA or PMALA sampler");
    if (corr && c->sa.kind != SK_PMALA) return mcmc_set_error(MCMC_E_INVALID_ARG, "SMMALA keeps no drift correction");
    mcmc_ctx* ctx = c->model->ctx;
    if (int r = set_device(ctx)) return r;
    const size_t d = (size_t)c->model->args.d, nr = d * (d + 1) / 2, C = (size_t)c->C;
    auto rows = [&](double* dst, const double* src, size_t n) -> hipError_t {
        if (!dst) return hipSuccess;
        return hipMemcpy2DAsync(dst, C * 8, src, (size_t)c->ld * 8, C * 8, n, hipMemcpyDeviceToHost, ctx->stream);
    };
    hipError_t e = rows(grad, c->st.g, d);
    if (e == hipSuccess) e = rows(G, c->st.sm_G, nr);
    if (e == hipSuccess) e = rows(invG, c->st.sm_invG, nr);
    if (e == hipSuccess) e = rows(ft, c->st.sm_ft, d);
    if (e == hipSuccess) e = rows(corr, c->st.pm_c, d);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return mcmc_set_error(MCMC_E_HIP, std::string("manifold state: ") + hipGetErrorString(e));
    return MCMC_OK;
}

extern "C" int mcmc_chains_ram_factor(mcmc_chains* c, double* S) {
    if (!c || !S) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    if (c->sa.kind != SK_RAM) return mcmc_set_error(MCMC_E_INVALID_ARG, "chains do not run the RAM sampler");
    mcmc_ctx* ctx = c->model->ctx;
    if (int r = set_device(ctx)) return r;
    const size_t rows = packed_rows(c->model->args.d);          // the leading rows of the padded packing
    const size_t rl = (size_t)c->st.ram_ld;
    const double* cur = c->st.ram_L + (size_t)(c->steps_done & 1) * (size_t)c->st.ram_hs;   // written last
    if (c->ram_wave) {                                         // [chain][column-major packed] -> [row][chain]
        const int64_t d = c->model->args.d;
        std::vector<double> h((size_t)c->C * rl);
        HIP_TRY(hipMemcpyAsync(h.data(), cur, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (int64_t r = 0; r < d; ++r)
            for (int64_t q = 0; q <= r; ++q)
                for (size_t ch = 0; ch < (size_t)c->C; ++ch)
                    S[(size_t)(r * (r + 1) / 2 + q) * (size_t)c->C + ch] = h[ch * rl + (size_t)(wave_colstart(q, d) + r - q)];
        return MCMC_OK;
    }
    const size_t tile = (packed_rows(c->ram_dpad) + 1) * 64;    // one 64-chain tile of a half (ram.hpp)
    const size_t ntiles = ((size_t)c->C + 63) / 64;
    std::vector<double> h(ntiles * tile);
    HIP_TRY(hipMemcpyAsync(h.data(), cur, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t r = 0; r < rows; ++r)                          // [tile][row][64] -> [row][chain]
        for (size_t ch = 0; ch < (size_t)c->C; ++ch) S[r * (size_t)c->C + ch] = h[(ch >> 6) * tile + r * 64 + (ch & 63)];
    return MCMC_OK;
}

// per-chain adaptive state: the step size (MALA driftStep, HMC leapStep, HMCDA leapStep), HMCDA's dual-averaged
// step (dualLeapStep, HMCDA.jl:139) and the tuned HMC nLeaps; a buffer the sampler does not keep is filled with
// NaN (step, step_bar) or 0 (nleaps)
extern "C" int mcmc_chains_tuner_state(mcmc_chains* c, double* step, double* step_bar, int32_t* nleaps) {
    if (!c) return mcmc_set_error(MCMC_E_INVALID_ARG, "chains is NULL");
    mcmc_ctx* ctx = c->model->ctx;
    if (int r = set_device(ctx)) return r;
    const size_t C = (size_t)c->C;
    if (step) {
        if (c->st.t_step) HIP_TRY(d2h(ctx, step, c->st.t_step, C * 8));
        else std::fill(step, step + C, __builtin_nan(""));
    }
    if (step_bar) {
        if (c->sa.kind == SK_NUTS) {                            // exp(log epsilon_bar), the device's exp
            DevScope scope(ctx->stream);
            double* tmp = nullptr;
            if (int r = scope.alloc(&tmp, C)) return r;
            hipError_t e = mcmc_detmath(1, (int64_t)C, c->st.t_bar, c->st.t_bar, tmp, ctx->stream);
            if (e == hipSuccess) e = d2h(ctx, step_bar, tmp, C * 8);
            HIP_TRY(e);
        } else if (c->st.t_bar) HIP_TRY(d2h(ctx, step_bar, c->st.t_bar, C * 8));
        else std::fill(step_bar, step_bar + C, __builtin_nan(""));
    }
    if (nleaps) {
        if (c->st.t_leaps) HIP_TRY(d2h(ctx, nleaps, c->st.t_leaps, C * 4));
        else std::fill(nleaps, nleaps + C, 0);
    }
    return MCMC_OK;
}

extern "C" int mcmc_chains_steps_done(mcmc_chains* c, int64_t* steps) {
    if (!c || !steps) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    *steps = c->steps_done;
    return MCMC_OK;
}

extern "C" int mcmc_chains_step_kernel(mcmc_chains* c, char* buf, int64_t cap) {
    if (!c || !buf || cap < 1) return mcmc_set_error(MCMC_E_INVALID_ARG, "bad argument");
    std::snprintf(buf, (size_t)cap, "%s", c->step_kernel.c_str());
    return MCMC_OK;
}

extern "C" int mcmc_chains_set_steps_per_launch(mcmc_chains* c, int64_t spl) {
    if (!c || spl < 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "bad argument");
    c->spl = spl;
    return MCMC_OK;
}

extern "C" int mcmc_chains_set_tuner_burnin(mcmc_chains* c, int64_t burnin) {
    if (!c) return mcmc_set_error(MCMC_E_INVALID_ARG, "chains is NULL");
    if (burnin < -1) return mcmc_set_error(MCMC_E_INVALID_ARG, "tuner burnin must be >= 0, or -1 (the runner's burnin)");
    c->tuner_burnin = burnin;
    return MCMC_OK;
}

extern "C" int mcmc_chains_set_store_gradients(mcmc_chains* c, int32_t store) {
    if (!c) return mcmc_set_error(MCMC_E_INVALID_ARG, "chains is NULL");
    c->store_grads = store ? 1 : 0;
    return MCMC_OK;
}

// Pre-size the library-owned output buffers of a run keeping nkept steps (the wave-per-chain staging
// rows, and the device copies used when the caller's buffers are on the host), so that the run itself
// allocates nothing.  Buffers only grow; they are freed with the chains.
extern "C" int mcmc_chains_reserve_outputs(mcmc_chains* c, int64_t nkept, int32_t on_device) {
    if (!c || nkept < 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "bad argument");
    if (int rc = set_device(c->model->ctx)) return rc;
    const size_t d = (size_t)c->model->args.d, C = (size_t)c->C, nk = (size_t)nkept;
    const bool grads = c->si->emits_grads && c->store_grads;
    if (c->layout == LAYOUT_WPC) {
        const size_t nstage = nk * C * (size_t)c->ld;
        if (int rc = ensure(c->stage_samples, nstage * 8)) return rc;
        if (grads)
            if (int rc = ensure(c->stage_grads, nstage * 8)) return rc;
    }
    if (!on_device) {
        if (int rc = ensure(c->out_samples, nk * d * C * 8)) return rc;
        if (grads)
            if (int rc = ensure(c->out_grads, nk * d * C * 8)) return rc;
        if (int rc = ensure(c->out_bits, nk * ((C + 63) / 64) * 8)) return rc;
    }
    return MCMC_OK;
}

extern "C" int mcmc_chains_store_leaps(mcmc_chains* c, int64_t cap, double* pars, double* grads, double* mom,
                                       double* lp, double* H, int32_t* nleaps) {
    if (!c) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL chains");
    if (pars == nullptr) {
        c->h_lpars = nullptr;
        c->leap_cap = 0;
        return MCMC_OK;
    }
    if (c->si->leaps_refusal) return mcmc_set_error(MCMC_E_UNSUPPORTED, c->si->leaps_refusal);
    if (!c->si->records_leaps)
        return mcmc_set_error(MCMC_E_INVALID_ARG, "storeLeaps needs an HMC or HMCDA sampler");
    if (cap < 0 || !grads || !mom || !lp || !H || !nleaps) return mcmc_set_error(MCMC_E_INVALID_ARG, "bad storeLeaps buffers");
    c->leap_cap = cap;
    c->h_lpars = pars;
    c->h_lgrads = grads;
    c->h_lmom = mom;
    c->h_llp = lp;
    c->h_lH = H;
    c->h_lnl = nleaps;
    return MCMC_OK;
}

extern "C" int mcmc_chains_nuts_diagnostics(mcmc_chains* c, double* epsilon, int32_t* ndoublings, int32_t on_device) {
    if (!c) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL chains");
    if (epsilon == nullptr) {
        c->nuts_eps = nullptr;
        c->nuts_nd = nullptr;
        return MCMC_OK;
    }
    if (c->sa.kind != SK_NUTS) return mcmc_set_error(MCMC_E_INVALID_ARG, "the NUTS diagnostics need a NUTS sampler");
    if (!ndoublings) return mcmc_set_error(MCMC_E_INVALID_ARG, "bad NUTS diagnostics buffers");
    c->nuts_eps = epsilon;
    c->nuts_nd = ndoublings;
    c->nuts_on_device = on_device != 0;
    return MCMC_OK;
}
