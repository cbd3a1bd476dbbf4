// model.cpp -- model uploads, the state-layout helpers every unit shares, and the evaluation calls.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "../glm_layout.hpp"
#include "internal.hpp"

using namespace mcmc;

extern "C" int mcmc_model_create(mcmc_ctx* ctx, const mcmc_model_desc* desc, mcmc_model** out) {
    if (!ctx || !desc || !out) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (int r = set_device(ctx)) return r;
    const int64_t d = desc->d;
    if (d <= 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "model size d should be > 0");
    if (!desc->init) return mcmc_set_error(MCMC_E_INVALID_ARG, "model init is NULL");
    auto* m = new mcmc_model();
    m->ctx = ctx;
    m->init.assign(desc->init, desc->init + d);
    m->scale.assign((size_t)d, 1.0);
    if (desc->scale) m->scale.assign(desc->scale, desc->scale + d);
    m->has_gradient = desc->has_gradient;
    // has_gradient == 2: gradient and metric tensor (hastensor(m), mcmcmodels.jl:20); built for the probit model
    // (examples/probit_regression.jl:44-49) and the logistic model (expected Fisher information + prior precision)
    // has_gradient == 3: the tensor's derivatives too (hasdtensor(m), mcmcmodels.jl:21): the probit example's
    // deriv_tensor (examples/probit_regression.jl:52-68) and d[p (1 - p)] / d eta for the logistic model
    if (desc->has_gradient >= 2 && desc->kind != MCMC_MODEL_PROBIT && desc->kind != MCMC_MODEL_LOGISTIC) {
        delete m;
        return mcmc_set_error(MCMC_E_UNSUPPORTED, "this model kind has no tensor function (built: PROBIT, LOGISTIC)");
    }
    ModelArgs& a = m->args;
    a.kind = desc->kind;
    a.d = (int32_t)d;
    a.mu = desc->mu;
    a.sigma = desc->sigma;
    a.prior_sigma = desc->prior_sigma;
    a.noise_sigma = desc->noise_sigma;
    a.link_sign = desc->link_sign;
    a.n = 0;
    a.n_pad = 0;
    auto bail = [&](int code) {
        mcmc_model_destroy(m);
        return code;
    };
    auto upload_series = [&]() -> int {             // Y [n] as it is (the DIST_OBS data, the OU series)
        if (int r = dmalloc(&m->d_Y, (size_t)desc->n)) return r;
        if (h2d(ctx, m->d_Y, desc->Y, (size_t)desc->n * 8) != hipSuccess)
            return mcmc_set_error(MCMC_E_HIP, "model data upload failed");
        a.n = desc->n;
        a.Y = m->d_Y;
        return MCMC_OK;
    };
    switch (desc->kind) {
        case MCMC_MODEL_ISO_NORMAL_DOT:
            break;
        case MCMC_MODEL_NORMAL_DSL:
        case MCMC_MODEL_ABS_NORMAL_DSL:
            if (!(desc->sigma > 0)) return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "Normal sigma should be > 0"));
            break;
        case MCMC_MODEL_DIST_OBS:
            if (d != 1) return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "y = x * v needs a scalar parameter x (d = 1)"));
            if (desc->n <= 0 || !desc->Y) return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "y = x * v needs the data v (n > 0, Y)"));
            [[fallthrough]];
        case MCMC_MODEL_DIST_DSL: {
            const double p1 = desc->mu, p2 = desc->sigma;
            const double kPi = 3.14159265358979323846;
            double c = 0.0;
            bool ok = true;
            switch (desc->dist) {
                case MCMC_DIST_NORMAL: ok = p2 > 0; c = -std::log(p2); break;
                case MCMC_DIST_UNIFORM: ok = p1 < p2; c = -std::log(p2 - p1); break;
                case MCMC_DIST_WEIBULL: ok = p1 > 0 && p2 > 0; c = std::log(p1 / p2); break;
                case MCMC_DIST_BETA: ok = p1 > 0 && p2 > 0; c = std::lgamma(p1 + p2) - std::lgamma(p1) - std::lgamma(p2); break;
                case MCMC_DIST_TDIST:
                    ok = p1 > 0;
                    c = std::lgamma((p1 + 1.0) / 2.0) - std::lgamma(p1 / 2.0) - 0.5 * std::log(p1 * kPi);
                    break;
                case MCMC_DIST_EXPONENTIAL: ok = p1 > 0; c = -std::log(p1); break;
                case MCMC_DIST_GAMMA: ok = p1 > 0 && p2 > 0; c = -std::lgamma(p1) - p1 * std::log(p2); break;
                case MCMC_DIST_CAUCHY: ok = p2 > 0; c = -std::log(kPi * p2); break;
                case MCMC_DIST_LOGNORMAL: ok = p2 > 0; c = -std::log(p2) - 0.5 * std::log(2.0 * kPi); break;
                case MCMC_DIST_LAPLACE: ok = p2 > 0; c = -std::log(2.0 * p2); break;
                default: return bail(mcmc_set_error(MCMC_E_UNSUPPORTED, "unknown distribution"));
            }
            if (!ok) return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "invalid distribution parameters"));
            a.dist = desc->dist;
            a.dconst = c;
            if (desc->kind == MCMC_MODEL_DIST_OBS)                      // the data v, read by every chain
                if (int r = upload_series()) return bail(r);
            break;
        }
        case MCMC_MODEL_OU: {
            // examples/ornstein.jl:19-30; the prior part of the LLAcc sum, ((0 + logpdf(Uniform(0, 100), tau)) +
            // logpdf(Uniform(0, 2), sigma)) + logpdf(Uniform(0, 20), mu) inside the support, -log(b - a) each
            if (d != 3) return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "the Ornstein-Uhlenbeck model has 3 parameters (tau, sigma, mu)"));
            if (desc->n < 2 || !desc->Y) return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "the Ornstein-Uhlenbeck model needs a series of n >= 2 values (Y)"));
            a.dconst = ((0.0 + -std::log(100.0)) + -std::log(2.0)) + -std::log(20.0);
            if (int r = upload_series()) return bail(r);
            break;
        }
        case MCMC_MODEL_LOGISTIC:
        case MCMC_MODEL_PROBIT:
        case MCMC_MODEL_LINEAR: {
            if (d > mcmc_glm_max_d()) return bail(mcmc_set_error(MCMC_E_UNSUPPORTED, "regression models support d <= 1024"));
            if (desc->n <= 0 || !desc->X || !desc->Y) return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "regression needs n > 0, X, Y"));
            if (!(desc->prior_sigma > 0)) return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "prior sigma should be > 0"));
            if (desc->kind == MCMC_MODEL_LINEAR && !(desc->noise_sigma > 0))
                return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "noise sigma should be > 0"));
            if (desc->kind == MCMC_MODEL_LOGISTIC && !(desc->link_sign == 1.0 || desc->link_sign == -1.0))
                return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "link_sign must be +1 or -1"));
            if (desc->kind == MCMC_MODEL_LOGISTIC || desc->kind == MCMC_MODEL_PROBIT)
                for (int64_t i = 0; i < desc->n; ++i)
                    if (!(desc->Y[i] == 0.0 || desc->Y[i] == 1.0))
                        return bail(mcmc_set_error(MCMC_E_INVALID_ARG, desc->kind == MCMC_MODEL_LOGISTIC
                                                                 ? "logistic responses must be 0 or 1 (Bernoulli)"
                                                                 : "probit responses must be 0 or 1"));
            // the kernels' staged-tile image of X and Y (glm_layout.hpp: 16-row tiles in the LDS layout, Y inside
            // each tile, zero padding), plus Y [n_pad] on its own
            const int64_t n_pad = (desc->n + 15) / 16 * 16;
            std::vector<double> Xp(mcmc_glm_image_doubles((int)d, desc->n)), Yp((size_t)n_pad, 0.0);
            for (int64_t i = 0; i < desc->n * (int64_t)d; ++i)
                if (!std::isfinite(desc->X[i])) return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "X must be finite"));
            for (int64_t i = 0; i < desc->n; ++i)
                if (!std::isfinite(desc->Y[i])) return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "Y must be finite"));
            // The logistic / probit terms clamp |eta| into their tables (det_logi, the normal log-cdf twins), so a
            // NaN eta would not reach LLAcc's non-finite rule as it does in the reference (a NaN term makes the sum
            // NaN and the point out of support, modelparser.jl:64-72).  eta is NaN only when X vars overflows with
            // mixed signs: every partial sum of row i is bounded by |vars|_inf |X_i|_1, and a vars whose prior term
            // is finite has |vars|_inf < sqrt(DBL_MAX) prior_sigma.  Data for which that product can reach 2^1022
            // (rows with L1 norm ~1e154 / prior_sigma) are refused here instead of clamped in the kernels.
            if (desc->kind == MCMC_MODEL_LOGISTIC || desc->kind == MCMC_MODEL_PROBIT) {
                double l1max = 0.0;
                for (int64_t i = 0; i < desc->n; ++i) {
                    double l1 = 0.0;
                    for (int k = 0; k < d; ++k) l1 += std::fabs(desc->X[i * (int64_t)d + k]);
                    l1max = std::max(l1max, l1);
                }
                if (!(l1max * (std::sqrt(DBL_MAX) * desc->prior_sigma) < 0x1p1022))
                    return bail(mcmc_set_error(MCMC_E_UNSUPPORTED, "covariates too large: X * vars can overflow to NaN at a "
                                                         "parameter vector of finite prior density"));
            }
            // the logistic model's tile columns hold w = s (2y - 1) (s the link sign) instead of y and the bounds
            // -T(y) where the reference's p rounds to 1 or 0 (detmath.hpp det_logi, logi_bound)
            std::vector<double> Yw, Bw;
            if (desc->kind == MCMC_MODEL_LOGISTIC) {
                Yw.resize((size_t)desc->n);
                Bw.resize((size_t)desc->n);
                for (int64_t i = 0; i < desc->n; ++i) {
                    Yw[(size_t)i] = desc->Y[i] == 1.0 ? desc->link_sign : -desc->link_sign;
                    Bw[(size_t)i] = mcmc::logi_bound(desc->Y[i]);
                }
            }
            mcmc_glm_pack_image((int)d, desc->n, desc->X, Yw.empty() ? desc->Y : Yw.data(),
                                Bw.empty() ? nullptr : Bw.data(), Xp.data());
            for (int64_t i = 0; i < desc->n; ++i) Yp[(size_t)i] = desc->Y[i];
            if (int r = dmalloc(&m->d_X, Xp.size())) return bail(r);
            if (int r = dmalloc(&m->d_Y, Yp.size())) return bail(r);
            if (h2d(ctx, m->d_X, Xp.data(), Xp.size() * 8) != hipSuccess ||
                h2d(ctx, m->d_Y, Yp.data(), Yp.size() * 8) != hipSuccess)
                return bail(mcmc_set_error(MCMC_E_HIP, "model data upload failed"));
            a.n = desc->n;
            a.n_pad = n_pad;
            a.X = m->d_X;
            a.Y = m->d_Y;
            break;
        }
        default:
            return bail(mcmc_set_error(MCMC_E_UNSUPPORTED, "unknown model kind"));
    }
    if (d > 0x7fffffff) return bail(mcmc_set_error(MCMC_E_INVALID_ARG, "d too large"));
    if (int r = dmalloc(&m->d_init, (size_t)d)) return bail(r);
    if (int r = dmalloc(&m->d_scale, (size_t)d)) return bail(r);
    a.init = m->d_init;
    hipError_t e = h2d(ctx, m->d_init, m->init.data(), (size_t)d * 8);
    if (e == hipSuccess) e = h2d(ctx, m->d_scale, m->scale.data(), (size_t)d * 8);
    if (e != hipSuccess) return bail(mcmc_set_error(MCMC_E_HIP, std::string("model upload: ") + hipGetErrorString(e)));
    // likmodel.jl:54  @assert isfinite(f(i)) "Initial values out of model support, try other values"
    double lp = 0;
    if (int r = mcmc_model_eval(m, 1, m->init.data(), &lp, nullptr)) return bail(r);
    if (!std::isfinite(lp))
        return bail(mcmc_set_error(MCMC_E_INIT_OUT_OF_SUPPORT, "Initial values out of model support, try other values"));
    *out = m;
    return MCMC_OK;
}

void model_free(mcmc_model* m) {
    (void)hipSetDevice(m->ctx->device);
    dfree(m->d_init);
    dfree(m->d_scale);
    dfree(m->d_X);
    dfree(m->d_Y);
    delete m;
}

// A model outlives its chains: destroying it while chains still use it (garbage-collected hosts
// finalize in any order) only marks it; the last mcmc_chains_destroy frees it.
extern "C" int mcmc_model_destroy(mcmc_model* m) {
    if (!m) return MCMC_OK;
    m->released = true;
    if (m->chains_alive == 0) model_free(m);
    return MCMC_OK;
}

// the lane / wave-per-chain kernel families (the joint OU target runs there too, at its fixed d = 3)
bool model_is_separable(const mcmc_model* m) {
    return m->args.kind == MK_ISO || m->args.kind == MK_NORMAL || m->args.kind == MK_ABS_NORMAL ||
           m->args.kind == MK_DIST || m->args.kind == MK_DIST_OBS || m->args.kind == MK_OU;
}
bool model_is_glm(const mcmc_model* m) {
    return m->args.kind == MK_LOGISTIC || m->args.kind == MK_LINEAR || m->args.kind == MK_PROBIT;
}
// State layout of a chain batch: lane-per-chain [d][ld] for d <= 32, wave-per-chain [C][ld] above.
Layout layout_for(const mcmc_model* m) {
    if (model_is_glm(m)) return LAYOUT_GLM;
    return m->args.d <= mcmc_lpc_max_d() ? LAYOUT_LPC : LAYOUT_WPC;
}
KernelArgs base_args(const mcmc_model* m, int64_t C, int64_t ld) {
    KernelArgs a{};
    a.m = m->args;
    a.s.C = C;
    a.s.ld = ld;
    a.s.d = m->args.d;
    a.s.err = m->ctx->d_err;
    a.s.thinning = 1;
    return a;
}

hipError_t launch_eval(Layout L, const KernelArgs& a, const double* xin, double* lp, double* g, int check,
                       hipStream_t st) {
    if (L == LAYOUT_GLM) return mcmc_launch_glm_eval(a, xin, lp, g, check, st);
    return L == LAYOUT_LPC ? mcmc_launch_lpc_eval(a, xin, lp, g, check, st)
                           : mcmc_launch_wpc_eval(a, xin, lp, g, check, st);
}
// [d][C] (stride ldc) <-> state layout
hipError_t cols_to_state(Layout L, double* state, int64_t ld, const double* cols, int64_t ldc, int d, int64_t C,
                         hipStream_t st) {
    if (L != LAYOUT_WPC) return mcmc_copy_cols(state, ld, cols, ldc, d, C, st);
    // [d][C] -> [C][ld]: transpose of a d x C matrix
    hipError_t e = hipMemsetAsync(state, 0, (size_t)C * ld * 8, st);
    if (e != hipSuccess) return e;
    return mcmc_transpose(state, ld, cols, ldc, 1, d, C, st);
}
hipError_t state_to_cols(Layout L, double* cols, int64_t ldc, const double* state, int64_t ld, int d, int64_t C,
                         hipStream_t st) {
    if (L != LAYOUT_WPC) return mcmc_copy_cols(cols, ldc, state, ld, d, C, st);
    return mcmc_transpose(cols, ldc, state, ld, 1, C, d, st);
}

// ------------------------------------------------------------------ evaluation calls
// One device output of an evaluation launch: `count` doubles (0: not allocated), which come back to `host` (may be
// NULL) as one vector of n (rows == 0), as `rows` rows of the leading dimension (rows > 0), or, a state-layout array,
// through state_to_cols (via_cols: the wave layout transposes)
struct EvalOut {
    double* host;
    size_t count, rows;
    bool via_cols;
    double* dev;
};

// What the mcmc_model_eval* calls share: x [d][n] uploaded into the state layout, one launch, the outputs downloaded.
template <class Launch>
static int eval_call(mcmc_model* m, Layout L, int64_t n, int64_t ld, const double* x, EvalOut* outs, int nouts,
                     const char* what, Launch launch) {
    hipStream_t st = m->ctx->stream;
    const int d = m->args.d;
    const size_t ncols = (size_t)d * n;
    DevScope tmp(st);
    double *dcols = nullptr, *dx = nullptr;
    if (int rc = tmp.alloc(&dcols, ncols)) return rc;
    if (int rc = tmp.alloc(&dx, L != LAYOUT_WPC ? (size_t)d * ld : (size_t)n * ld)) return rc;
    for (int i = 0; i < nouts; ++i)
        if (int rc = tmp.alloc(&outs[i].dev, outs[i].count)) return rc;
    hipError_t e = hipMemcpyAsync(dcols, x, ncols * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = cols_to_state(L, dx, ld, dcols, n, d, n, st);
    if (e == hipSuccess) e = launch(base_args(m, n, ld), dx);
    for (int i = 0; e == hipSuccess && i < nouts; ++i) {
        const EvalOut& o = outs[i];
        if (!o.host) continue;
        if (o.via_cols) {
            e = state_to_cols(L, dcols, n, o.dev, ld, d, n, st);
            if (e == hipSuccess) e = hipMemcpyAsync(o.host, dcols, ncols * 8, hipMemcpyDeviceToHost, st);
        } else if (o.rows == 0) {
            e = hipMemcpyAsync(o.host, o.dev, (size_t)n * 8, hipMemcpyDeviceToHost, st);
        } else {
            e = hipMemcpy2DAsync(o.host, (size_t)n * 8, o.dev, (size_t)ld * 8, (size_t)n * 8, o.rows,
                                 hipMemcpyDeviceToHost, st);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return mcmc_set_error(MCMC_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return MCMC_OK;
}

extern "C" int mcmc_model_eval(mcmc_model* m, int64_t nchains, const double* x, double* lp, double* grad) {
    if (!m || !x || !lp) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    if (nchains <= 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "nchains should be > 0");
    if (int r = set_device(m->ctx)) return r;
    const int d = m->args.d;
    if (model_is_separable(m) && d > mcmc_wpc_max_d()) return mcmc_set_error(MCMC_E_UNSUPPORTED, "d > 16384 is not built");
    const Layout L = layout_for(m);
    const int64_t ld = ld_for(L, nchains, d);
    const size_t nst = L != LAYOUT_WPC ? (size_t)d * ld : (size_t)nchains * ld;
    EvalOut o[] = {{lp, (size_t)nchains, 0, false, nullptr}, {grad, grad ? nst : 0, 0, true, nullptr}};
    hipStream_t st = m->ctx->stream;
    return eval_call(m, L, nchains, ld, x, o, 2, "model eval", [&](const KernelArgs& a, const double* dx) {
        return launch_eval(L, a, dx, o[0].dev, o[1].dev, 0, st);
    });
}

// the tensor calls' sizes: built for the regression layout at d <= mcmc_smmala_max_d()
static int tensor_dims(mcmc_model* m, int64_t nchains, int need, const char* missing, const char* what) {
    if (nchains <= 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "nchains should be > 0");
    if (m->has_gradient < need) return mcmc_set_error(MCMC_E_NEEDS_GRADIENT, missing);
    if (int r = set_device(m->ctx)) return r;
    if (m->args.d > mcmc_smmala_max_d())
        return mcmc_set_error(MCMC_E_UNSUPPORTED, std::string(what) + std::to_string(mcmc_smmala_max_d()));
    return MCMC_OK;
}

// model.evalallt (likmodel.jl): log-target, gradient and metric tensor of nchains parameter vectors; G packed by rows,
// element (r, c), c <= r, of chain k at G[(r(r+1)/2 + c) * nchains + k]
extern "C" int mcmc_model_eval_tensor(mcmc_model* m, int64_t nchains, const double* x, double* lp, double* grad,
                                      double* G) {
    if (!m || !x || !G) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    if (int r = tensor_dims(m, nchains, 2, "model has no tensor function", "the tensor is built for d <= ")) return r;
    const size_t d = (size_t)m->args.d, nr = packed_rows(m->args.d), ld = (size_t)round_up(nchains, 64);
    EvalOut o[] = {{lp, ld, 0, false, nullptr}, {grad, d * ld, d, false, nullptr}, {G, nr * ld, nr, false, nullptr}};
    hipStream_t st = m->ctx->stream;
    return eval_call(m, LAYOUT_GLM, nchains, (int64_t)ld, x, o, 3, "model eval tensor",
                     [&](const KernelArgs& a, const double* dx) {
                         return mcmc_launch_smmala_eval(a, dx, o[0].dev, o[1].dev, o[2].dev, nullptr, nullptr, 0, st);
                     });
}

// model.evalalldt (likmodel.jl:27): evalallt's outputs (lp, grad and G may be NULL) and the tensor's derivatives, d
// slabs packed like G: element (r, c), c <= r, of slab i of chain k at dG[((i nr + r(r+1)/2 + c) * nchains + k],
// nr = d(d+1)/2
extern "C" int mcmc_model_eval_dtensor(mcmc_model* m, int64_t nchains, const double* x, double* lp, double* grad,
                                       double* G, double* dG) {
    if (!m || !x || !dG) return mcmc_set_error(MCMC_E_INVALID_ARG, "NULL argument");
    if (int r = tensor_dims(m, nchains, 3, "model has no function of tensor derivatives",
                            "the tensor derivatives are built for d <= "))
        return r;
    const size_t d = (size_t)m->args.d, nr = packed_rows(m->args.d), ld = (size_t)round_up(nchains, 64);
    EvalOut o[] = {{lp, ld, 0, false, nullptr},
                   {grad, d * ld, d, false, nullptr},
                   {G, nr * ld, nr, false, nullptr},
                   {dG, d * nr * ld, d * nr, false, nullptr}};
    hipStream_t st = m->ctx->stream;
    return eval_call(m, LAYOUT_GLM, nchains, (int64_t)ld, x, o, 4, "model eval dtensor",
                     [&](const KernelArgs& a, const double* dx) {
                         return mcmc_launch_pmala_dtensor(a, dx, o[0].dev, o[1].dev, o[2].dev, o[3].dev, st);
                     });
}

