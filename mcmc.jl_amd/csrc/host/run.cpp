// run.cpp -- the SerialMC step loop: launch arguments, the step launchers, the storeLeaps record and the outputs.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "internal.hpp"

using namespace mcmc;

static int64_t nkept_of(const mcmc_runner_cfg& r) {
    if (r.len <= r.burnin) return 0;
    return (r.len - r.burnin - 1) / r.thinning + 1;
}

static hipError_t launch_record(Layout L, const KernelArgs& a, const LeapRec& r, hipStream_t st) {
    if (L == LAYOUT_GLM) return mcmc_launch_glm_record(a, r, st);
    return L == LAYOUT_LPC ? mcmc_launch_lpc_record(a, r, st) : mcmc_launch_wpc_record(a, r, st);
}

// The storeLeaps record of a run inside leap_buf (HMC.jl:145-150): for each of nk kept steps pars / grads / mom
// [rows][d][C] and lp / H [rows][C] (doubles, rows = cap + 1), then nl [C] (int32).  The six sub-arrays' offsets in
// doubles; nl's is also the count of doubles before it
struct LeapLayout {
    size_t nk, C, lsz, lsc;                    // lsz, lsc: doubles per kept step of a vector / a scalar sub-array
    size_t pars, grads, mom, lp, H, nl;
    LeapLayout(size_t rows, size_t d, size_t C_, size_t nk_)
        : nk(nk_), C(C_), lsz(rows * d * C_), lsc(rows * C_), pars(0), grads(nk * lsz), mom(2 * nk * lsz),
          lp(3 * nk * lsz), H(lp + nk * lsc), nl(H + nk * lsc) {}
    size_t nl_bytes() const { return nk * C * 4; }
};

// RAM on a regression target with d > 32 is a sequence of kernels per step
hipError_t launch_chain_step(const mcmc_chains* c, const KernelArgs& a, hipStream_t st) {
    if (c->glm_ram_wave) {
        const mcmc_ctx* ctx = c->model->ctx;
        return mcmc_launch_glm_ram_wave(a, c->ram_u, c->ram_nz, c->xprop, c->lpp, st,
                                        st == ctx->stream ? ctx->stream2 : nullptr, ctx->ev_fork, ctx->ev_join);
    }
    switch (c->sa.kind) {
        case SK_NUTS: return mcmc_launch_nuts(a, 0, st);
        case SK_SMMALA: return mcmc_launch_smmala_step(a, st);
        case SK_PMALA: return mcmc_launch_pmala_step(a, st);
        case SK_RMHMC: return mcmc_launch_rmhmc_step(a, st);
        case SK_ERMLMC:
        case SK_RMLMC: return mcmc_launch_lmc_step(a, st);
        default: break;                                    // RWM, MALA, HMC, HMCDA, RAM: the layout's fused step kernel
    }
    if (c->layout == LAYOUT_GLM) return mcmc_launch_glm_step(a, st);
    return c->layout == LAYOUT_LPC ? mcmc_launch_lpc_step(a, st) : mcmc_launch_wpc_step(a, st);
}

KernelArgs step_args(const mcmc_chains* c, const RunRange& r) {
    KernelArgs a = base_args(c->model, c->C, c->ld);
    a.sa = c->sa;
    a.st = c->st;
    StepArgs& s = a.s;
    s.chain0 = (uint32_t)c->offset;
    s.key0 = (uint32_t)c->seed;
    s.key1 = (uint32_t)(c->seed >> 32);
    s.scale = c->d_scale_eff;
    s.scale1 = c->scale1;
    s.scale_uniform = c->scale_uniform;
    s.run_step0 = c->steps_done;
    s.burnin = r.burnin;
    s.thinning = r.thinning;
    s.len = r.len;
    s.tuner_burnin = r.tuner_burnin;
    s.nw = (c->C + 63) / 64;
    s.n_evals = c->si->evals_on_host ? nullptr : c->d_evals;
    return a;
}

// Regression HMC / HMCDA: the chains' order for the next run, longest trajectory first.  A 16-chain MFMA tile runs
// its leapfrog loop to the longest trajectory among its chains (glm_hmc's glm_max), and an HMCDA chain's length
// round(len / leapStep) follows its own adapted leapStep (config 5: 240 to 384 leapfrogs a step), so tiles of
// arbitrary chains idle on ~10% of their leapfrogs; sorted, a tile's chains take (nearly) the same number, and the
// longest tiles are dispatched first.  Bitwise neutral: a tile's MFMA columns are independent chains, and every
// chain-indexed access goes through the permutation (glm.hip glm_pos).  The key is the state the run starts from:
// the current leapStep (HMCDA; smaller is longer, NaN last) or the tuned nLeaps (HMC).
static int glm_trajectory_order(mcmc_chains* c, hipStream_t st) {
    mcmc_ctx* ctx = c->model->ctx;
    const int64_t C = c->C;
    if (int rc = ensure(c->order_buf, (size_t)C * sizeof(int32_t))) return rc;
    std::vector<double> key((size_t)C);
    if (c->sa.kind == SK_HMCDA) {
        HIP_TRY(d2h(ctx, key.data(), c->st.t_step, (size_t)C * sizeof(double)));
    } else {
        std::vector<int32_t> nl((size_t)C);
        HIP_TRY(d2h(ctx, nl.data(), c->st.t_leaps, (size_t)C * sizeof(int32_t)));
        for (int64_t i = 0; i < C; ++i) key[(size_t)i] = -(double)nl[(size_t)i];
    }
    c->h_order.resize((size_t)C);
    for (int64_t i = 0; i < C; ++i) c->h_order[(size_t)i] = (int32_t)i;
    std::stable_sort(c->h_order.begin(), c->h_order.end(), [&](int32_t a, int32_t b) {
        const double ka = key[(size_t)a], kb = key[(size_t)b];
        const bool na = std::isnan(ka), nb = std::isnan(kb);
        return na != nb ? nb : (!na && ka < kb);
    });
    // two tiles a workgroup (d-sliced, 128 < d <= 512): the longest tile shares its workgroup with the shortest, the
    // second longest with the second shortest, ...: the workgroup runs its longer tile's trajectory, and once the
    // shorter tile's chains have all finished it stops computing (glm_hmc's tile skip), so the long tiles -- the
    // dispatch's end -- run their tails with the SIMDs to themselves.  Whole 32-chain workgroups only.
    if (mcmc_glm_tiles_per_wg(c->model->args.d) == 2 && C % 32 == 0) {
        const int64_t nt = C / 16;
        std::vector<int32_t> paired((size_t)C);
        for (int64_t w = 0; w < nt / 2; ++w)
            for (int h = 0; h < 2; ++h) {
                const int64_t src = h == 0 ? w : nt - 1 - w;             // sorted tile
                for (int k = 0; k < 16; ++k)
                    paired[(size_t)((2 * w + h) * 16 + k)] = c->h_order[(size_t)(src * 16 + k)];
            }
        c->h_order.swap(paired);
    }
    HIP_TRY(hipMemcpyAsync(c->order_buf.p, c->h_order.data(), (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MCMC_OK;
}
// steps fused per launch for a run of len steps: the user's setting (0: the whole run), capped by the
// kernels that fuse a bounded number of steps (the single-slice regression MALA kernel: one)
static int64_t launch_steps(const mcmc_chains* c, int64_t len) {
    int64_t spl = c->spl > 0 ? c->spl : len;
    if (c->layout == LAYOUT_GLM) {
        const int64_t kmax = mcmc_glm_steps_per_launch(c->model->args.d, c->model->args.n, c->sa.kind);
        if (kmax > 0 && spl > kmax) spl = kmax;
    }
    return spl < 1 ? 1 : spl;
}

extern "C" int mcmc_chains_launches(mcmc_chains* c, int64_t len, int64_t* launches) {
    if (!c || !launches || len < 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "bad argument");
    const int64_t spl = launch_steps(c, len);
    *launches = len == 0 ? 0 : (len + spl - 1) / spl;
    return MCMC_OK;
}

// device -> host copy of `rows` rows of `width` bytes from a packed device array into a host array whose
// rows are `dpitch` bytes apart (dpitch == width: one contiguous copy)
static hipError_t d2h_rows(mcmc_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t width, size_t rows) {
    hipError_t e = dpitch == width
                       ? hipMemcpyAsync(dst, src, width * rows, hipMemcpyDeviceToHost, ctx->stream)
                       : hipMemcpy2DAsync(dst, dpitch, src, width, width, rows, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e;
}
extern "C" int mcmc_run_serialmc(mcmc_chains* c, const mcmc_runner_cfg* r, mcmc_outputs* out) {
    return mcmc_run_serialmc_ld(c, r, out, c ? c->C : 0, nullptr);
}

// run_serialmc with host outputs laid out for a larger chain batch this one is a block of (mcmc_group.cpp):
// samples/gradients/final_x rows are ldc chains apart, accept-bit rows ceil(ldc/64) words apart; the caller
// has offset every pointer to this block's first chain (a multiple of 64 when ldc != C).  copy_s: the
// device -> host time of the outputs.
int mcmc_run_serialmc_ld(mcmc_chains* c, const mcmc_runner_cfg* r, mcmc_outputs* out, int64_t ldc, double* copy_s) {
    if (!c || !r) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    if (ldc < c->C) return mcmc_set_error(MCMC_E_INVALID_ARG, "output leading dimension below the chain count");
    if (out && out->on_device && ldc != c->C)
        return mcmc_set_error(MCMC_E_INVALID_ARG, "strided outputs are host buffers");
    if (int rc = mcmc_runner_validate(r)) return rc;
    mcmc_model* m = c->model;
    mcmc_ctx* ctx = m->ctx;
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const int d = m->args.d;
    const int64_t C = c->C;
    const Layout L = c->layout;
    const int64_t nkept = nkept_of(*r);
    const int64_t nw = (C + 63) / 64;
    if (c->steps_done + r->len > 0xffffffffLL) return mcmc_set_error(MCMC_E_INVALID_ARG, "step counter exceeds 2^32");
    const bool on_dev = out && out->on_device;
    const bool want_samples = out && out->samples;
    const bool want_grads = out && out->gradients && c->si->emits_grads && c->store_grads;
    const bool want_bits = out && out->accept_bits;

    // output buffers in the C ABI layout ([nkept][d][C]) on the device: the caller's, or library-owned ones
    int rc = MCMC_OK;
    auto device_out = [&](bool want, void* callers, DevBuf& own, size_t bytes) -> void* {
        if (!want || rc) return nullptr;
        if (callers) return callers;
        rc = ensure(own, bytes);
        return own.p;
    };
    const size_t nsamp = (size_t)nkept * (size_t)d * (size_t)C;
    double* d_samples = (double*)device_out(want_samples, on_dev ? out->samples : nullptr, c->out_samples, nsamp * 8);
    double* d_grads = (double*)device_out(want_grads, on_dev ? out->gradients : nullptr, c->out_grads, nsamp * 8);
    uint64_t* d_bits = (uint64_t*)device_out(want_bits, on_dev ? out->accept_bits : nullptr, c->out_bits,
                                             (size_t)nkept * nw * 8);
    // wave-per-chain kernels write kept rows chain-major ([nkept][C][ld]); transposed after the loop
    const bool staged = L == LAYOUT_WPC;
    const size_t nstage = (size_t)nkept * (size_t)C * (size_t)c->ld;
    double* k_samples = staged ? (double*)device_out(want_samples, nullptr, c->stage_samples, nstage * 8) : d_samples;
    double* k_grads = staged ? (double*)device_out(want_grads, nullptr, c->stage_grads, nstage * 8) : d_grads;
    if (rc) return rc;

    // the tuners' burnin: MALA.jl:116, HMC.jl:167, HMCDA.jl:133
    KernelArgs a = step_args(c, {r->burnin, r->thinning, r->len, c->tuner_burnin >= 0 ? c->tuner_burnin : r->burnin});
    StepArgs& s = a.s;
    s.samples = k_samples;
    s.grads = k_grads;
    s.acc_bits = d_bits;
    c->last_order = false;
    // regression tiles run their leapfrog loop to their longest chain.  (The lane / pair layouts were measured
    // with the same order and it did not pay: DESIGN.md §5.3.)
    if (L == LAYOUT_GLM && C > 16 && (c->sa.kind == SK_HMCDA || (c->sa.kind == SK_HMC && c->sa.tuner))) {
        if (int rc = glm_trajectory_order(c, st)) return rc;
        s.order = (const int32_t*)c->order_buf.p;
        c->last_order = true;
    }

    // NUTS diagnostics of the kept steps: straight into the caller's device buffers, or staged
    const bool ndiag = c->sa.kind == SK_NUTS && c->nuts_eps != nullptr;
    if (ndiag) {
        const size_t nd = (size_t)nkept * (size_t)C;
        if (c->nuts_on_device) {
            s.nuts_eps = c->nuts_eps;
            s.nuts_nd = c->nuts_nd;
        } else {
            if (int rc = ensure(c->nuts_buf, nd * 12)) return rc;
            s.nuts_eps = (double*)c->nuts_buf.p;
            s.nuts_nd = (int32_t*)(s.nuts_eps + nd);
        }
    }
    // storeLeaps: one step per launch; before each kept step, a record launch of its trajectory
    const bool rec = c->h_lpars != nullptr;
    const int64_t spl = rec ? 1 : launch_steps(c, r->len);
    const LeapLayout ll(rec ? (size_t)(c->leap_cap + 1) : 0, (size_t)d, (size_t)C, (size_t)nkept);
    double* dl = nullptr;
    if (rec) {
        if (int rc = ensure(c->leap_buf, ll.nl * 8 + ll.nl_bytes())) return rc;
        dl = (double*)c->leap_buf.p;
        HIP_TRY(mcmc_fill_f64(dl, (int64_t)ll.nl, __builtin_nan(""), st));
        HIP_TRY(hipMemsetAsync(dl + ll.nl, 0, ll.nl_bytes(), st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipEventRecord(ctx->ev0, st));
    if (want_bits && L != LAYOUT_LPC) HIP_TRY(hipMemsetAsync(d_bits, 0, (size_t)nkept * nw * 8, st));
    for (int64_t done = 0; done < r->len; done += spl) {
        const int64_t n = std::min(spl, r->len - done);
        s.step_begin = c->steps_done + done + 1;
        s.nsteps = (int32_t)n;
        int64_t kk;
        if (rec && kept_index(done + 1, r->burnin, r->thinning, r->len, &kk)) {
            const size_t k = (size_t)kk;
            const LeapRec lr{c->leap_cap,          dl + ll.pars + k * ll.lsz, dl + ll.grads + k * ll.lsz,
                             dl + ll.mom + k * ll.lsz, dl + ll.lp + k * ll.lsc,   dl + ll.H + k * ll.lsc,
                             (int32_t*)(dl + ll.nl) + k * (size_t)C};
            HIP_TRY(launch_record(L, a, lr, st));
        }
        mcmc_clear_step_kernel();
        HIP_TRY(launch_chain_step(c, a, st));
        c->step_kernel = mcmc_last_step_kernel();
        if (c->si->evals_on_host) c->h_evals += C * n;
    }
    HIP_TRY(hipEventRecord(ctx->ev1, st));
    if (L == LAYOUT_WPC) {
        if (want_samples) HIP_TRY(mcmc_transpose(d_samples, C, k_samples, c->ld, nkept, C, d, st));
        if (want_grads) HIP_TRY(mcmc_transpose(d_grads, C, k_grads, c->ld, nkept, C, d, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    auto t1 = std::chrono::steady_clock::now();
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    c->steps_done += r->len;
    if (rec) {
        HIP_TRY(d2h(ctx, c->h_lpars, dl + ll.pars, ll.nk * ll.lsz * 8));
        HIP_TRY(d2h(ctx, c->h_lgrads, dl + ll.grads, ll.nk * ll.lsz * 8));
        HIP_TRY(d2h(ctx, c->h_lmom, dl + ll.mom, ll.nk * ll.lsz * 8));
        HIP_TRY(d2h(ctx, c->h_llp, dl + ll.lp, ll.nk * ll.lsc * 8));
        HIP_TRY(d2h(ctx, c->h_lH, dl + ll.H, ll.nk * ll.lsc * 8));
        HIP_TRY(d2h(ctx, c->h_lnl, dl + ll.nl, ll.nl_bytes()));
        c->h_lpars = nullptr;                          // one run consumes the registration
    }
    if (ndiag) {
        if (!c->nuts_on_device) {
            const size_t nd = (size_t)nkept * (size_t)C;
            HIP_TRY(d2h(ctx, c->nuts_eps, s.nuts_eps, nd * 8));
            HIP_TRY(d2h(ctx, c->nuts_nd, s.nuts_nd, nd * 4));
        }
        c->nuts_eps = nullptr;                         // one run consumes the registration
        c->nuts_nd = nullptr;
    }

    if (out) {
        out->nkept = nkept;
        out->runtime_s = std::chrono::duration<double>(t1 - t0).count();
        out->kernel_ms = ms;
        const size_t rowb = (size_t)C * 8, drow = (size_t)ldc * 8;
        const size_t nwl = (size_t)(ldc + 63) / 64;
        auto c0 = std::chrono::steady_clock::now();
        if (!on_dev) {
            if (want_samples) HIP_TRY(d2h_rows(ctx, out->samples, drow, d_samples, rowb, (size_t)nkept * d));
            if (want_grads) HIP_TRY(d2h_rows(ctx, out->gradients, drow, d_grads, rowb, (size_t)nkept * d));
            if (want_bits) HIP_TRY(d2h_rows(ctx, out->accept_bits, nwl * 8, d_bits, (size_t)nw * 8, (size_t)nkept));
        }
        if (out->final_x) {
            if (on_dev) {
                HIP_TRY(state_to_cols(L, out->final_x, C, c->st.x, c->ld, d, C, st));
            } else {
                if (int rc = ensure(c->out_tmp, (size_t)d * C * 8)) return rc;
                HIP_TRY(state_to_cols(L, (double*)c->out_tmp.p, C, c->st.x, c->ld, d, C, st));
                HIP_TRY(d2h_rows(ctx, out->final_x, drow, c->out_tmp.p, rowb, (size_t)d));
            }
        }
        if (out->final_lp)
            HIP_TRY(hipMemcpyAsync(out->final_lp, c->st.lp, (size_t)C * 8,
                                   on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (copy_s) *copy_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - c0).count();
    }
    return MCMC_OK;
}
