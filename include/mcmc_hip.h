/*
 * mcmc_hip.h -- C ABI of the MI355X (gfx950) many-chain MCMC inner loop.
 *
 * Drop-in boundary for MCMC.jl's model x sampler x runner hot path
 * (reference: /root/reference, Julia 0.2).  Plain C types only: int32/int64,
 * double*, uint64_t*; no torch, no C++ in the signatures.  A Julia host binds
 * these with `ccall` (INTEGRATION.md shows the binding); the in-tree host is
 * Python/ctypes (mcmc.jl_amd/mcmchip).
 *
 *   reference interface                              replaced by
 *   -----------------------------------------------  -------------------------------------------
 *   model(f; init, grad, scale)      mcmcmodels.jl:27-33,   mcmc_model_create (catalogue kind, init,
 *     MCMCLikelihoodModel ctor        likmodel.jl:100-143    scale, data X/Y)
 *   RWM / MALA / HMC / HMCDA / NUTS  RWM.jl:24-36,          mcmc_sampler_cfg (validated like the
 *                                    MALA.jl:50-62,         reference @asserts: mcmc_sampler_validate)
 *                                    HMC.jl:53-74,
 *                                    HMCDA.jl:24-43
 *   EmpMCTuner                       samplers.jl:32-50      mcmc_sampler_cfg.tuner_*
 *   SerialMC(steps,burnin,thinning)  SerialMC.jl:12-35      mcmc_runner_cfg
 *   m * s * r -> MCMCTask (spinTask) MCMC.jl:87-98,         mcmc_chains_create (a batch of C
 *                                    samplers.jl:53          independent MCMCTasks: one per chain)
 *   run(t::MCMCTask) / run_serialmc  runners.jl:7-11,45,    mcmc_run_serialmc
 *                                    SerialMC.jl:37-85
 *   run(c::MCMCChain) (continue)     runners.jl:14          mcmc_run_serialmc again on the same chains
 *   resume(c; steps)                 SerialMC.jl:93-97      a new batch (mcmc_chains_create) on fresh global
 *                                                           chain ids + mcmc_run_serialmc
 *   MCMCChain fields                 MCMC.jl:58-80          mcmc_outputs (samples, gradients,
 *                                                           accept bits, runtime)
 *   acceptance(chain)                summary.jl:6-15        computed by the host from accept bits
 *
 * Errors: every call returns an int status (MCMC_OK = 0) and sets a
 * thread-local message readable with mcmc_last_error(); the reference's
 * @assert texts are reproduced verbatim where one exists.
 *
 * Threading: one host thread drives a context; calls on one context are not
 * re-entrant; distinct contexts are independent and may be driven from
 * different host threads at once (also on one GPU).  mcmc_group_* drives
 * several GPUs from one host thread (library worker threads per device).  Ownership: the caller owns
 * every output buffer; the library owns device state inside ctx/model/chains
 * and never keeps a caller pointer after a call returns.
 */
#ifndef MCMC_HIP_H
#define MCMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCMC_ABI_VERSION 1

/* status codes */
enum {
    MCMC_OK = 0,
    MCMC_E_INVALID_ARG = 1,          /* a reference @assert failed, or a NULL/size error            */
    MCMC_E_INIT_OUT_OF_SUPPORT = 2,  /* "Initial values out of model support, try other values"    */
    MCMC_E_NEEDS_GRADIENT = 3,       /* "<S> sampler requires model with gradient function"         */
    MCMC_E_HIP = 4,                  /* a HIP runtime call failed                                   */
    MCMC_E_OOM = 5,                  /* device allocation failed                                    */
    MCMC_E_UNSUPPORTED = 6           /* model x sampler x size combination not built                */
};

/* model catalogue (Julia closures cannot cross a C ABI) */
enum {
    MCMC_MODEL_ISO_NORMAL_DOT = 1,   /* model(v -> -dot(v,v), grad = v -> -2v)   README.md:60,63      */
    MCMC_MODEL_NORMAL_DSL = 2,       /* model(:(v ~ Normal(mu, sigma)), gradient=true)  README.md:67-72 */
    MCMC_MODEL_LOGISTIC = 3,         /* examples/logistic_regression.jl:16-22 (DSL, gradient=true)   */
    MCMC_MODEL_LINEAR = 4,           /* examples/linear_regression.jl:14-20  (DSL, gradient=true)    */
    MCMC_MODEL_ABS_NORMAL_DSL = 5,   /* model(:(y = abs(x); y ~ Normal(mu, sigma)))  README.md:246-251 */
    MCMC_MODEL_DIST_DSL = 6,         /* model(:(v ~ Dist(p1, p2))): dist = MCMC_DIST_*, p1 = mu, p2 = sigma */
    MCMC_MODEL_PROBIT = 7,           /* examples/probit_regression.jl:18-40: log-prior MvNormal(0, prior_sigma^2 I)
                                        + dot(logcdf(N, X pars), Y) + dot(logcdf(N, -X pars), 1 - Y), Y 0.0 / 1.0 */
    MCMC_MODEL_DIST_OBS = 8,         /* model(:(y = x * v; y ~ Dist(p1, p2))), benchmarks/benchunits/bare_distribs.jl:13:
                                        scalar x (d = 1), data v = Y [n]; dist / mu / sigma as MCMC_MODEL_DIST_DSL */
    MCMC_MODEL_OU = 9                /* examples/ornstein.jl:19-30: pars (tau, sigma, mu) (d = 3), the series x = Y [n],
                                        n >= 2: tau ~ Uniform(0,100), sigma ~ Uniform(0,2), mu ~ Uniform(0,20),
                                        resid = x[2:end] - x[1:end-1] exp(-1/tau) - mu (1 - exp(-1/tau)) ~ Normal(0, sigma) */
};

/* distributions of MCMC_MODEL_DIST_DSL: the DSL's continuous logpdf rules, MCMCDerivRules.jl:56-104
   (Distributions.jl parametrisations) */
enum {
    MCMC_DIST_NORMAL = 1,       /* Normal(mu, sigma)          */
    MCMC_DIST_UNIFORM = 2,      /* Uniform(a, b)              */
    MCMC_DIST_WEIBULL = 3,      /* Weibull(shape, scale)      */
    MCMC_DIST_BETA = 4,         /* Beta(alpha, beta)          */
    MCMC_DIST_TDIST = 5,        /* TDist(df)     (p2 unused)  */
    MCMC_DIST_EXPONENTIAL = 6,  /* Exponential(scale)         */
    MCMC_DIST_GAMMA = 7,        /* Gamma(shape, scale)        */
    MCMC_DIST_CAUCHY = 8,       /* Cauchy(location, scale)    */
    MCMC_DIST_LOGNORMAL = 9,    /* LogNormal(meanlog, sdlog)  */
    MCMC_DIST_LAPLACE = 10      /* Laplace(location, scale)   */
};

/* samplers */
enum { MCMC_RWM = 1, MCMC_MALA = 2, MCMC_HMC = 3, MCMC_HMCDA = 4, MCMC_RAM = 5, MCMC_NUTS = 6, MCMC_SMMALA = 7,
       MCMC_PMALA = 8, MCMC_RMHMC = 9, MCMC_ERMLMC = 10, MCMC_RMLMC = 11 };

typedef struct mcmc_ctx mcmc_ctx;
typedef struct mcmc_model mcmc_model;
typedef struct mcmc_chains mcmc_chains;

typedef struct {
    int32_t kind;            /* MCMC_MODEL_*                                                     */
    int32_t has_gradient;    /* 0: eval only (hasgradient(model) == false, mcmcmodels.jl:19); 1: gradient;
                                2: gradient and metric tensor (hastensor(model), mcmcmodels.jl:20): PROBIT uses
                                examples/probit_regression.jl:44-49, G = X' diag(v) X + I/prior_sigma^2 with
                                v = exp(-eta^2 - logcdf(eta) - logcdf(-eta) - log 2 pi); LOGISTIC the expected Fisher
                                information plus the prior precision, v = p (1 - p) for either link_sign (the metric of
                                Girolami & Calderhead 2011 for this model; the reference's logistic example passes no
                                tensor);
                                3: gradient, tensor and the tensor's derivatives (hasdtensor(model), mcmcmodels.jl:21):
                                slab i of dG is X' diag(w o X[:, i]) X, w = dv / d eta: PROBIT the example's
                                deriv_tensor as written (probit_regression.jl:52-68), LOGISTIC p (1 - p) (1 - 2p) for
                                link_sign = +1 and its negative for -1.  A model with 3 serves everything a model
                                with 2 does.  With 2 or 3 any other kind answers MCMC_E_UNSUPPORTED        */
    int64_t d;               /* parameter vector size (model.size)                               */
    const double* init;      /* [d]  model.init                                                  */
    const double* scale;     /* [d]  model.scale (NULL -> ones)                                   */
    double mu, sigma;        /* NORMAL_DSL, ABS_NORMAL_DSL: Normal(mu, sigma)                     */
    double prior_sigma;      /* LOGISTIC/LINEAR: vars ~ Normal(0, prior_sigma)                    */
    double noise_sigma;      /* LINEAR: resid ~ Normal(0, noise_sigma)                             */
    double link_sign;        /* LOGISTIC: +1 -> prob = 1/(1+exp(-X*vars)) (example),
                                          -1 -> prob = 1/(1+exp(+X*vars)) (test/test_syntax.jl:13) */
    int64_t n;               /* observations                                                      */
    const double* X;         /* [n][d] row-major covariates                                        */
    const double* Y;         /* [n] responses (LOGISTIC: 0.0 / 1.0)                                */
    int32_t dist;            /* DIST_DSL: MCMC_DIST_* (parameters in mu, sigma)                     */
} mcmc_model_desc;

typedef struct {
    int32_t kind;            /* MCMC_RWM | MCMC_MALA | MCMC_HMC | MCMC_HMCDA | MCMC_RAM | MCMC_NUTS | MCMC_SMMALA |
                                MCMC_PMALA | MCMC_RMHMC | MCMC_ERMLMC | MCMC_RMLMC                */
    double scale;            /* RWM, RAM: scale (RWM.jl:25, RAM.jl:23)                             */
    double drift_step;       /* MALA: driftStep (MALA.jl:51); SMMALA: driftStep (SMMALA.jl:24);
                                PMALA: driftStep (PMALA.jl:26)                                    */
    int64_t n_leaps;         /* HMC: nLeaps (HMC.jl:54); NUTS: maxdoublings (NUTS.jl:31);
                                RMHMC: nLeaps (RMHMC.jl:29), at most 2^20; ERMLMC, RMLMC: nLeaps
                                (ERMLMC.jl:26, RMLMC.jl:27), at most 2^20                          */
    double leap_step;        /* HMC: leapStep (HMC.jl:55); RMHMC: leapStep (RMHMC.jl:30); ERMLMC, RMLMC:
                                leapStep (ERMLMC.jl:27, RMLMC.jl:28)                               */
    double rate, len, shrinkage, t0, step;   /* HMCDA (HMCDA.jl:25-29); rate: RAM target rate (RAM.jl:24);
                                t0: RMHMC's nNewton (RMHMC.jl:31), a double holding an integer in 1 .. 2^31 - 1
                                t0: RMLMC's nNewton (RMLMC.jl:29) likewise; ERMLMC does not read it
                                (the struct's size is fixed; any other value answers MCMC_E_INVALID_ARG)  */
    int32_t tuner;           /* 0: nothing; 1: EmpiricalMCMCTuner (MALA, HMC, SMMALA, PMALA, RMHMC, ERMLMC, RMLMC) */
    int64_t adapt_step, max_step;            /* EmpMCTuner (samplers.jl:33-37)                      */
    double target_path, target_rate;
    int64_t max_leaps;       /* HMCDA/HMC-tuner safety cap on leapfrogs per step (0 -> 1<<20)      */
} mcmc_sampler_cfg;

typedef struct {
    int64_t burnin;          /* SerialMC.burnin                                                    */
    int64_t thinning;        /* SerialMC.thinning                                                  */
    int64_t len;             /* SerialMC.len: steps consumed per run                              */
} mcmc_runner_cfg;

/* Output buffers.  Any pointer may be NULL (not wanted).  Layouts:
 *   samples, gradients : [nkept][d][nchains]   (MCMCChain.samples / .gradients, per chain c:
 *                                              samples[j][:, c] is row j of its DataFrame)
 *   accept_bits        : [nkept][ceil(nchains/64)]  bit (c % 64) of word c/64 = diagnostics["accept"][j]
 *   final_x            : [d][nchains]          state after the run
 *   final_lp           : [nchains]
 * nkept = length((burnin+1):thinning:len).  on_device != 0 means every pointer is a
 * device pointer on the context's GPU (e.g. torch tensors): nothing crosses PCIe. */
typedef struct {
    double* samples;
    double* gradients;
    uint64_t* accept_bits;
    double* final_x;
    double* final_lp;
    int32_t on_device;
    double runtime_s;        /* out: wall time of the step loop (MCMCChain.runTime, SerialMC.jl:38,84) */
    double kernel_ms;        /* out: device time of the step kernels (HIP events)                     */
    int64_t nkept;           /* out */
} mcmc_outputs;

/* ---- library ---- */
const char* mcmc_last_error(void);
int mcmc_abi_version(void);
int mcmc_device_count(int* count);

/* ---- context: one GPU, one stream ---- */
int mcmc_ctx_create(int device, mcmc_ctx** out);
int mcmc_ctx_destroy(mcmc_ctx* ctx);
int mcmc_ctx_synchronize(mcmc_ctx* ctx);

/* ---- model: uploads init/scale/X/Y once (model data is replicated per GPU) ---- */
int mcmc_model_create(mcmc_ctx* ctx, const mcmc_model_desc* desc, mcmc_model** out);
int mcmc_model_destroy(mcmc_model* model);
/* evaluate log-target (and gradient) of `nchains` parameter vectors x[d][nchains] on the device
 * (model.eval / model.evalallg, likmodel.jl:21,25); host pointers. grad may be NULL. */
int mcmc_model_eval(mcmc_model* model, int64_t nchains, const double* x, double* lp, double* grad);
/* model.evalallt (likmodel.jl): log-target, gradient and the metric tensor G of x[d][nchains]; host pointers, lp and
 * grad may be NULL.  G is symmetric and packed like the RAM factor: element (r, c), c <= r, of chain k at
 * G[(r(r+1)/2 + c) * nchains + k] (d(d+1)/2 * nchains doubles).  lp and grad are mcmc_model_eval's bit for bit.  A model
 * created with has_gradient < 2 answers MCMC_E_NEEDS_GRADIENT, "model has no tensor function"; built for d <= 16. */
int mcmc_model_eval_tensor(mcmc_model* model, int64_t nchains, const double* x, double* lp, double* grad, double* G);
/* model.evalalldt (likmodel.jl:27): evalallt's outputs (lp, grad and G may be NULL; mcmc_model_eval_tensor's bit for
 * bit) and the derivatives of G: d slabs, each packed like G, element (r, c), c <= r, of slab i of chain k at
 * dG[((i * d(d+1)/2) + r(r+1)/2 + c) * nchains + k] (d * d(d+1)/2 * nchains doubles).  A model created with
 * has_gradient < 3 answers MCMC_E_NEEDS_GRADIENT, "model has no function of tensor derivatives"; d > 16
 * MCMC_E_UNSUPPORTED.  An inspection path: the PMALA step loop never forms the slabs. */
int mcmc_model_eval_dtensor(mcmc_model* model, int64_t nchains, const double* x, double* lp, double* grad, double* G,
                            double* dG);

/* ---- sampler config validation (the reference constructors' @asserts) ---- */
int mcmc_sampler_validate(const mcmc_sampler_cfg* cfg);
int mcmc_runner_validate(const mcmc_runner_cfg* cfg);

/* ---- chains: C independent MCMCTasks of one (model, sampler) on one GPU ----
 * chain_offset = global id of local chain 0 (multi-GPU sharding): the random
 * stream is keyed by (seed, global chain, global step), so results do not
 * depend on the number of GPUs.  init_x: optional per-chain start [d][nchains]
 * (NULL -> every chain starts at model.init, RWM.jl:53).  Sizes built: d <= 16384 for the separable
 * models, d <= 1024 for the regression models; RAM d <= 1024 (separable and regression), else
 * MCMC_E_UNSUPPORTED.  NUTS (NUTS.jl:53-183): built for the separable targets with d <= 32 and the joint targets
 * (DIST_OBS, OU; d <= 16), maxdoublings 1..10 (n_leaps; the reference default is 5).  Wider targets, the regression
 * models and maxdoublings 11..19 (valid in the reference) answer MCMC_E_UNSUPPORTED; mcmc_run_seqmc refuses NUTS
 * targets (NUTS adapts by its own step counter).  The initial epsilon search (NUTS.jl:71-82) runs here and again at
 * mcmc_chains_reset; mcmc_chains_set_state keeps epsilon and the dual-averaging state (the :reset hook,
 * NUTS.jl:61-63).  The accept bit of a kept NUTS step is 1 if any doubling's candidate was taken.
 * SMMALA (SMMALA.jl:39-123): built for PROBIT and LOGISTIC models with a tensor (has_gradient == 2) and d <= 16; a wider d
 * answers MCMC_E_UNSUPPORTED, a model without a tensor MCMC_E_NEEDS_GRADIENT ("SMMALA sampler requires model with tensor
 * function", after the gradient check), a start whose log-target is not finite or whose G has a Cholesky pivot <= 0 or
 * not finite MCMC_E_INIT_OUT_OF_SUPPORT.  Outputs, tuner (EmpiricalMALATune) and tuner_state are MALA's; evals count one
 * per step plus the initial one.  A proposal out of support, or whose G or h invG fails a pivot, is rejected (the
 * reference would throw out of chol).  mcmc_chains_set_state keeps invG and firstTerm of the previous position (the
 * :reset hook as written, SMMALA.jl:54-57); mcmc_run_seqmc refuses SMMALA targets.
 * PMALA (PMALA.jl:42-141): SMMALA's models, sizes, outputs, tuner and departures, on a model with tensor derivatives
 * (has_gradient == 3; otherwise MCMC_E_NEEDS_GRADIENT, "PMALA sampler requires model with function of tensor
 * derivatives", after the gradient and tensor checks).  The drift is (h/2)(firstTerm - c), c = sum_i invG dG_i invG[:, i],
 * formed without the slabs as invG X' (w o q), q_o = x_o' invG x_o.  c is state beside SMMALA's: recomputed by
 * mcmc_chains_reset, copied by mcmc_chains_fork, left as it is by mcmc_chains_set_state (the :reset hook as written,
 * PMALA.jl:63-66); mcmc_run_seqmc refuses PMALA targets.
 * RMHMC (RMHMC.jl:53-183): PMALA's models and sizes (has_gradient == 3, d <= 16; otherwise MCMC_E_NEEDS_GRADIENT with
 * "RMHMC sampler requires model with gradient function" / "... tensor function" / "... function of tensor
 * derivatives", or MCMC_E_UNSUPPORTED for d > 16).  n_leaps = nLeaps, leap_step = leapStep, t0 = nNewton; the tuner is
 * HMC's EmpiricalHMCTune (tuner_state: step = leapStep, nleaps = nLeaps).  The state is x, lp and the gradient; G, invG
 * and the two tensor terms are recomputed by every step, so mcmc_chains_set_state has no quirk to keep.  Each step
 * draws timeStep = +1 iff a standard normal exceeds 0.5 (as written, probability 0.31) and nRandomLeaps =
 * ceil(rand() nLeaps) generalised leapfrogs; evals count the leapfrogs (HMC's convention).  A trajectory with a
 * log-target that is not finite, a Cholesky pivot <= 0 or not finite at any G, or a position or ratio that is not
 * finite is rejected (the reference would throw out of chol), and so is a step whose nRandomLeaps draw is 0 (the
 * reference leaves proposedGrad undefined there).  mcmc_run_seqmc and mcmc_chains_store_leaps answer
 * MCMC_E_UNSUPPORTED for RMHMC chains.
 * ERMLMC (ERMLMC.jl:84-179, MCMC_ERMLMC = 10) and RMLMC (RMLMC.jl:89-179, MCMC_RMLMC = 11): RMHMC's models and sizes
 * (has_gradient == 3, d <= 16; otherwise MCMC_E_NEEDS_GRADIENT with "ERMLMC / RMLMC sampler requires model with
 * gradient function" / "... tensor function" / "... function of tensor derivatives", or MCMC_E_UNSUPPORTED for
 * d > 16).  n_leaps = nLeaps, leap_step = leapStep, RMLMC: t0 = nNewton; the tuner is HMC's EmpiricalHMCTune.  The
 * state is x, lp and the gradient; every step recomputes G, cholG, invG, traceInvGxdG and dphi at the state's position
 * and draws velocity = chol(invG)' randn and nRandomLeaps = ceil(rand() nLeaps) (there is no timeStep).  The tensor
 * C = 0.5 (permutedims(dG, [3 2 1]) + permutedims(dG, [1 3 2]) - dG) is never formed: on these models dG is symmetric
 * in its three indices, so vxC(v) = 0.5 X' diag(w o X v) X, one weighted Gram pass over X.  The energies are the
 * reference's as written: ERMLMC's carries -sum(log(diag(cholG))), RMLMC's +sum(log(diag(cholG))).  The evaluation
 * count is the sum of nRandomLeaps.  Departures: a step whose trajectory meets a log-target that is not finite, a
 * Cholesky pivot <= 0 or not finite at any G, invG or G +- c vxC (the reference's logdet throws on a negative
 * determinant and goes through LU on an indefinite matrix with a positive one), or a position, velocity or ratio that
 * is not finite is rejected, and so is a step whose nRandomLeaps draw is 0 (the reference would read an undefined
 * proposedLogTarget).  mcmc_chains_set_state re-evaluates at the new position and the next step recomputes all geometry
 * from it; the reference's reset hooks (ERMLMC.jl:64-67, RMLMC.jl:69-72) leave invG, cholG, traceInvGxdG, dphi and C at
 * the previous position, which is why mcmc_run_seqmc answers MCMC_E_UNSUPPORTED for these targets;
 * mcmc_chains_store_leaps does too. */
int mcmc_chains_create(mcmc_model* model, const mcmc_sampler_cfg* sampler, int64_t nchains,
                       int64_t chain_offset, uint64_t seed, const double* init_x, mcmc_chains** out);
int mcmc_chains_destroy(mcmc_chains* chains);
/* restart from model.init (resume(), SerialMC.jl:93-97): step counter back to 0. */
int mcmc_chains_reset(mcmc_chains* chains);
/* MCMC.reset(t, x) (src/MCMC.jl:39; the samplers' task-local :reset hooks, RWM.jl:49, MALA.jl:75-80, HMC.jl:114-116,
 * HMCDA.jl:82-83, RAM.jl:47): every chain's position := x (host [d][nchains]) and its log-target (and gradient)
 * re-evaluated there; lp (may be NULL) receives the log-targets [nchains].  The step counter, tuner state and RAM
 * factor are kept.  Used by SeqMC-style drivers (SeqMC.jl:68-69) that move particles between tasks. */
int mcmc_chains_set_state(mcmc_chains* chains, const double* x, double* lp);
/* chains [first, first + count) of src as a new, independent batch (same model, sampler and seed; global chain ids
 * src's + first) holding a copy of their whole state and step counter, so that running it continues exactly those
 * chains whatever src does next.  No reference counterpart beyond run(c::MCMCChain) = run(c.task) (runners.jl:14):
 * after one batched run of an Array{MCMCTask}, each returned chain's task continues its own chain. */
int mcmc_chains_fork(mcmc_chains* src, int64_t first, int64_t count, mcmc_chains** out);
/* steps consumed so far (the sampler's own loop counter i). */
int mcmc_chains_steps_done(mcmc_chains* chains, int64_t* steps);
/* per-chain adaptive state after the last run, [nchains] each (any may be NULL): step = the current step size
 * (MALA / SMMALA / PMALA driftStep under EmpiricalMALATune, HMC / RMHMC / ERMLMC / RMLMC leapStep under EmpiricalHMCTune, HMCDA leapStep, HMCDA.jl:136,140);
 * step_bar = HMCDA's dual-averaged dualLeapStep (HMCDA.jl:138); nleaps = the tuned HMC / RMHMC / ERMLMC / RMLMC nLeaps (HMC.jl:42).
 * NUTS: step = epsilon, step_bar = exp(log epsilon_bar) (NUTS.jl:169-172).
 * A quantity the sampler does not adapt reads NaN (steps) or 0 (nleaps). */
int mcmc_chains_tuner_state(mcmc_chains* chains, double* step, double* step_bar, int32_t* nleaps);
/* log-target evaluations (with gradient for MALA/HMC/HMCDA) summed over all chains since
 * create/reset: steps x C for RWM/MALA, the leapfrog count for HMC/HMCDA (HMC.jl:93-102) and RMHMC, ERMLMC, RMLMC (the sum of nRandomLeaps),
 * whose trajectory length varies per chain under HMCDA / EmpMCTuner; NUTS: the leapfrogs of every tree and of
 * the initial epsilon search. */
int mcmc_chains_evals(mcmc_chains* chains, int64_t* evals);
/* RAM: the current jump factor S of every chain (RAM.jl:55, :78), lower triangle packed by rows:
 * element (r, c), c <= r, of chain k at S[(r(r+1)/2 + c) * nchains + k]; host buffer of
 * d(d+1)/2 * nchains doubles.  MCMC_E_INVALID_ARG for other samplers. */
int mcmc_chains_ram_factor(mcmc_chains* chains, double* S);
/* SMMALA / PMALA: the sampler's state beside the position and its log-target, host buffers, any may be NULL: grad,
 * first_term and corr (PMALA's c; MCMC_E_INVALID_ARG for SMMALA) [d][nchains]; G and invG packed like
 * mcmc_model_eval_tensor's G.  MCMC_E_INVALID_ARG for other samplers. */
int mcmc_chains_manifold_state(mcmc_chains* chains, double* grad, double* G, double* invG, double* first_term,
                               double* corr);
/* steps fused per kernel launch (0 = whole run in one launch, the default). */
int mcmc_chains_set_steps_per_launch(mcmc_chains* chains, int64_t steps_per_launch);
/* The burnin the samplers' adaptation sees, apart from the kept range of mcmc_run_serialmc.  The reference's
 * tuners read the task's own runner: EmpiricalMALATune / EmpiricalHMCTune adapt while i <= runner.burnin
 * (MALA.jl:116, HMC.jl:167) and HMCDA dual-averages while i < runner.burnin (HMCDA.jl:133-141), i the sampler's
 * step counter.  A host that keeps every step of a run and applies the kept range itself (a Julia Task producing
 * one MCMCSample per consume, in chunks: julia/mcmc_jl_hook.jl) sets the task runner's burnin here.  -1 (the
 * default): each run's own runner->burnin.  Copied by mcmc_chains_fork. */
int mcmc_chains_set_tuner_burnin(mcmc_chains* chains, int64_t burnin);
/* store gradients of kept samples for gradient samplers (default 1, SerialMC.jl:51-53) */
int mcmc_chains_set_store_gradients(mcmc_chains* chains, int32_t store);
/* pre-size the library's own output buffers for runs keeping up to nkept steps (staging of the
 * wave-per-chain layout; device copies when on_device == 0), so that mcmc_run_serialmc allocates
 * nothing (no reference counterpart: the Julia runner grows its DataFrame per run, SerialMC.jl:39-42). */
int mcmc_chains_reserve_outputs(mcmc_chains* chains, int64_t nkept, int32_t on_device);
/* kernel launches a run of len steps takes (steps per launch as set, capped by kernels that fuse a
 * bounded number of steps); for timing per launch. */
int mcmc_chains_launches(mcmc_chains* chains, int64_t len, int64_t* launches);
/* the step kernel instance the last mcmc_run_serialmc launched, e.g. "lpc_rwm<8, true, IsoDot, true>"
 * (the template instance rocprofv3 names, without the namespace), NUL-terminated into buf[cap];
 * "" before the first run.  No reference counterpart: lets tests and benchmarks check which
 * specialisation ran. */
int mcmc_chains_step_kernel(mcmc_chains* chains, char* buf, int64_t cap);

/* storeLeaps (HMC.jl:145-150, HMCDA.jl:110-117; HMC and HMCDA only).  The next mcmc_run_serialmc records, for
 * every kept step, the states of its trajectory -- leap 0 = state0 after update!, leap l = the state after
 * the l-th leapfrog, l <= min(nLeaps, cap) -- into host buffers: pars, grads, mom [nkept][cap+1][d][C];
 * lp, H [nkept][cap+1][C] (NaN past nLeaps); nleaps [nkept][C] (the full nLeaps, also when above cap).
 * That run takes one step per launch.  pars == NULL switches it off; one run consumes the registration. */
int mcmc_chains_store_leaps(mcmc_chains* chains, int64_t cap, double* pars, double* grads, double* mom, double* lp,
                            double* H, int32_t* nleaps);

/* NUTS diagnostics (NUTS.jl:177; NUTS only, MCMC_E_INVALID_ARG otherwise).  The next mcmc_run_serialmc records, for
 * every kept step, diagnostics["epsilon"] (the value after the step's adaptation) and diagnostics["ndoublings"] into
 * epsilon, ndoublings [nkept][nchains] (on_device != 0: device pointers on the context's GPU).  epsilon == NULL
 * switches it off; one run consumes the registration.  Group runs sample with NUTS but do not gather these two. */
int mcmc_chains_nuts_diagnostics(mcmc_chains* chains, double* epsilon, int32_t* ndoublings, int32_t on_device);

/* run_serialmc: consume runner->len steps, keep (burnin+1):thinning:len. */
int mcmc_run_serialmc(mcmc_chains* chains, const mcmc_runner_cfg* runner, mcmc_outputs* out);

/* ---- one node's GPUs driven by one host thread (SURVEY.md §8(b),(e)) ----
 * Replaces the reference's only parallel path, prun -> pmap of independent tasks over worker processes
 * (src/runners/runners.jl:35-42, examples/parallel_serialmc.jl:1-8): one batch of nchains chains is split
 * into contiguous blocks of whole 64-chain groups, block g on devices[g] (mcmc_group_plan).  Every block
 * keys its random streams by global chain id (chain_offset + its first chain), so the results are
 * bit-identical to one context running all chains, for any device list.  A run launches every block's step
 * loop concurrently (one library worker thread per block, each with its own context and stream; no
 * collective inside the step loop), then gathers each block's outputs device -> host straight into the
 * caller's [nkept][d][nchains] buffers (a strided copy per GPU over that GPU's own host link: the end
 * gather of MCMCChain assembly, timed apart).  A device may be listed more than once (several blocks on one
 * GPU).  Outputs of a group run are host buffers (on_device must be 0). */
typedef struct mcmc_group mcmc_group;
typedef struct mcmc_group_chains mcmc_group_chains;
int mcmc_group_create(const int32_t* devices, int32_t ndevices, mcmc_group** out);
int mcmc_group_destroy(mcmc_group* group);     /* after every mcmc_group_chains of it is destroyed */
int mcmc_group_size(mcmc_group* group, int32_t* ndevices);
/* the block of every device: block g = chains [first[g], first[g] + count[g]); blocks of ceil(nchains /
 * nblocks) rounded up to a multiple of 64 chains, so trailing blocks may be short or empty (count 0).
 * Host-only arithmetic (no device needed). */
int mcmc_group_plan(int64_t nchains, int32_t nblocks, int64_t* first, int64_t* count);
/* model (replicated: uploaded once per device), sampler and chains on every device; init_x: optional
 * [d][nchains] host array (NULL -> model.init) */
int mcmc_group_chains_create(mcmc_group* group, const mcmc_model_desc* model, const mcmc_sampler_cfg* sampler,
                             int64_t nchains, int64_t chain_offset, uint64_t seed, const double* init_x,
                             mcmc_group_chains** out);
int mcmc_group_chains_destroy(mcmc_group_chains* gc);
int mcmc_group_chains_reset(mcmc_group_chains* gc);                       /* resume(): every block */
int mcmc_group_chains_steps_done(mcmc_group_chains* gc, int64_t* steps);
int mcmc_group_chains_set_steps_per_launch(mcmc_group_chains* gc, int64_t steps_per_launch);
/* block g's chains (NULL when the block is empty) and its first chain / chain count; the block's
 * mcmc_chains may be queried (evals, step kernel, RAM factor) but not run or destroyed on its own */
int mcmc_group_chains_block(mcmc_group_chains* gc, int32_t g, mcmc_chains** chains, int64_t* first,
                            int64_t* count);
/* run_serialmc on every block concurrently; out holds host buffers for all nchains chains (mcmc_outputs
 * layout); out->runtime_s / kernel_ms: the slowest block's step loop; gather_s (may be NULL): the slowest
 * block's device -> host gather of its outputs.  Output buffers that are not already page-locked are
 * registered (hipHostRegister, portable) for the duration of the call, so the gather is direct DMA; callers
 * that run repeatedly into the same buffers can pin them once themselves.  If any block fails, the error
 * names the block and device, and these chains refuse further runs (and steps_done) until
 * mcmc_group_chains_reset: the blocks may then be at different steps. */
int mcmc_group_run_serialmc(mcmc_group_chains* gc, const mcmc_runner_cfg* runner, mcmc_outputs* out,
                            double* gather_s);
/* the last mcmc_group_run_serialmc's page-locking of the caller's output buffers (hipHostRegister before,
 * hipHostUnregister after; 0 when they were pinned already), in seconds.  It is not part of gather_s, which
 * times the copies alone: a caller that runs once into fresh pageable buffers pays both. */
int mcmc_group_last_pin_s(const mcmc_group_chains* gc, double* pin_s);
/* test hook: the next mcmc_group_run_serialmc fails block `block` before it starts (the others run) */
int mcmc_debug_group_inject_failure(mcmc_group_chains* gc, int32_t block);

/* ---- SeqMC population runner (src/runners/SeqMC.jl:21-122) ----
 * targets[t] (t < ntargets) are chain batches of one context, equal d, each with nchains == npart:
 * particle n is chain n of every target.  Per outer step i = 1..steps and target t: every particle is
 * reset into target t (state = particle, lp = eval: MCMC.reset, MCMC.jl:39) and advanced one step of
 * its sampler; logW += lp_t(reset) - logtarget; logtarget = lp after the step; when var(exp(logW)) <
 * trigger the particles are resampled multinomially from cumsum(W)/sum(W) (one Philox uniform of
 * (particle, i, t, tag 2) under `seed`) and logW = 0.  After each outer step logtarget = 0, and for
 * i > burnin the particles and exp(logW) are stored.
 *   particles : [d][npart] start values (SeqMC.jl:43 `particles`)
 *   samples   : [steps-burnin][d][npart]   (row i-burnin-1: the particles after outer step i)
 *   weights   : [steps-burnin][npart]      (diagnostics["weigths"])
 *   resampled : [steps][ntargets] int32 flags, or NULL
 * on_device != 0: particles/samples/weights/resampled are device pointers on the context's GPU. */
typedef struct {
    int64_t steps;           /* SeqMC.steps   (SeqMC.jl:24)                                          */
    int64_t burnin;          /* SeqMC.burnin                                                          */
    double trigger;          /* SeqMC.trigger: resample when var(W) < trigger                        */
} mcmc_seqmc_cfg;
int mcmc_seqmc_validate(const mcmc_seqmc_cfg* cfg);
int mcmc_run_seqmc(mcmc_chains* const* targets, int32_t ntargets, int64_t npart, const double* particles,
                   const mcmc_seqmc_cfg* cfg, uint64_t seed, int32_t on_device, double* samples, double* weights,
                   int32_t* resampled, double* runtime_s);

/* ---- SerialTempMC serial-tempering runner (src/runners/SerialTempMC.jl:16-85) ----
 * targets[t] (2 <= ntargets) are chain batches of one context with equal d, chain offset and nchains == nwalkers:
 * walker c is chain c of every target, an independent run_serialtempmc keyed by its global chain id.  A walker holds
 * the fields run_serialtempmc reads of its last MCMCSample s (samplers.jl:10-18): s.ppars, the position its task
 * stands at, which is what is stored (SerialTempMC.jl:77); s.pars and s.logtarget, the position and log-target
 * before that step, which is what a swap resets the other task to and compares (SerialTempMC.jl:62-64).
 * It starts on targets[0] with one step from that batch's current state (SerialTempMC.jl:51).  Step i = 1..steps:
 *   i % swap_period == 0: at2 = r >= at ? r + 1 : r with r = min(K - 2, floor(u (K - 1))); target at2 is reset to
 *     s.pars (position, then lp and gradient by the eval kernel) and takes one step, s2; the swap is accepted iff
 *     u2 < exp(((s.logtarget - s2.logtarget) + logW[at2]) - logW[at]), each operation rounded once, a NaN rejecting.
 *     Accepted: at = at2, s = s2.  Rejected: the walker keeps at and s; its task is not consumed.
 *   otherwise: s = one step of target `at` from s.ppars.
 * For i > burnin, s.ppars, at (zero-based) and the swap-accepted bit are stored.  u = uniform52(w0, w1) and
 * u2 = uniform52(w2, w3) of the Philox block (global chain id, i, 0, tag 8) under `seed`; each target's sampler draws
 * come from its own batch's key and step counter.  On the device every target resets to the walkers' positions and
 * steps all its chains on every step, and walker c takes the sample of its target: the step counter of every target
 * advances by steps (targets[0]: steps + 1), its evaluation count as under mcmc_run_seqmc, the tuners see burnin 0
 * (tuned MALA / HMC and HMCDA do not adapt), and RAM's factor of (target, walker) adapts on every step.  A sampler
 * mcmc_run_seqmc refuses is refused here for the same reason (MCMC_E_UNSUPPORTED).
 *   logW      : host [ntargets] log-weights of the targets, or NULL for zeros (SerialTempMC.jl:49; the reference's
 *               adaptation is a TODO, SerialTempMC.jl:71)
 *   samples   : [steps-burnin][d][nwalkers], or NULL
 *   models    : [steps-burnin][nwalkers] int32 (the reference's commented res.misc[:mod]), or NULL
 *   swap_bits : [steps-burnin][ceil(nwalkers/64)] uint64, walker c in bit c % 64 of word c / 64, or NULL
 *   final_at  : [nwalkers] int32, the walkers' targets after the last step, or NULL
 * on_device != 0: samples/models/swap_bits/final_at are device pointers on the context's GPU. */
typedef struct {
    int64_t steps;           /* SerialTempMC.steps (SerialTempMC.jl:17)                               */
    int64_t burnin;          /* SerialTempMC.burnin                                                   */
    int64_t swap_period;     /* SerialTempMC.swapPeriod: a swap is proposed when i % swap_period == 0 */
} mcmc_serialtempmc_cfg;
int mcmc_serialtempmc_validate(const mcmc_serialtempmc_cfg* cfg);
int mcmc_run_serialtempmc(mcmc_chains* const* targets, int32_t ntargets, int64_t nwalkers,
                          const mcmc_serialtempmc_cfg* cfg, const double* logW, uint64_t seed, int32_t on_device,
                          double* samples, int32_t* models, uint64_t* swap_bits, int32_t* final_at,
                          double* runtime_s);

/* ---- slice sampling (src/samplers/slice_sample.jl:43-103) ----
 * Neal's univariate-at-a-time slice sampler with stepping out and shrinkage, as the reference writes it, for nchains
 * independent chains of one catalogue model: a function on the model's log-density, not an MCMCSampler -- no
 * mcmc_sampler_cfg, no mcmc_chains.  Every logdist(...) of the reference is one full evaluation of the d-vector,
 * bitwise what mcmc_model_eval returns for it.  Per iteration iter = iter_begin + 1 .. iter_begin + burnin + niter and
 * coordinate dd = 0 .. d - 1 in order:
 *   log_uprime = log(u0) + log_Px;  x_l = state[dd] - r w[dd];  x_r = state[dd] + (1 - r) w[dd]  (the product rounded,
 *   then the sum);  step_out: while logdist(x_l) > log_uprime: x_l -= w[dd], likewise x_r += w[dd];  shrink:
 *   xprime = u_k (x_r - x_l) + x_l (three roundings), log_Px = logdist(xprime), accepted iff log_Px > log_uprime (a NaN
 *   is not), else x_r = xprime if xprime > state[dd], x_l = xprime if xprime < state[dd].
 * After the sweep of iteration iter > iter_begin + burnin the state is row iter - iter_begin - burnin - 1 of samples.
 * Draw k of the update (iter, dd) is the 52-bit uniform of words (w0, w1) (k even) or (w2, w3) (k odd) of the Philox
 * block (global chain id, iter, (dd << 20) | (k >> 1), tag 9) under `seed`: k = 0 is u0, k = 1 is r, k >= 2 is shrink
 * proposal k - 2.  So a run of a + b iterations is bitwise a run of a followed by one of b with iter_begin = a from the
 * first run's final_x, and results do not depend on how chains are split over calls (chain_offset).
 * Where the reference would loop without end or assert:
 *   - a start whose log-density is not finite answers MCMC_E_INIT_OUT_OF_SUPPORT;
 *   - one coordinate update may spend max_evals evaluations, stepping out and shrinking together.  A chain whose update
 *     is not finished after that many, or whose xprime == state[dd] and still is not acceptable (slice_sample.jl:92),
 *     stops: info[c] = the iteration, counted from iter_begin, 1-based (saturating at 2^31 - 1); final_x and final_lp
 *     keep its last completed iteration's state; its rows of samples from that iteration on are NaN.  The other chains
 *     are unaffected and the call answers MCMC_OK.  info[c] = 0 otherwise.  max_evals is a guard against unbounded
 *     loops on a shared GPU, not a tuning knob: 3 .. 2^20, 0 -> 4096.
 * Built for the separable and joint targets with d <= 32 (ISO_NORMAL_DOT, NORMAL_DSL, ABS_NORMAL_DSL, DIST_DSL,
 * DIST_OBS, OU); the regression models and wider d answer MCMC_E_UNSUPPORTED.  A long run is split by the library into
 * launches of at most 256 whole iterations; the split changes no result.
 *   init_x   : [d][nchains] per-chain starts, or NULL -> model.init for every chain
 *   widths   : host [d], finite and > 0 (else MCMC_E_INVALID_ARG), or NULL -> ones
 *   samples  : [niter][d][nchains] (the mcmc_outputs layout: mcmc_stats_ess, mcmc_stats_describe and mcmc_stats_zv's
 *              sample argument read it in place), or NULL
 *   final_x  : [d][nchains], final_lp : [nchains], info : int32 [nchains]; any may be NULL
 *   evals    : host, every logdist call of the run over all chains, the nchains initial ones included, or NULL
 *   runtime_s, kernel_ms : host, wall time of the run and device time of its kernels, or NULL
 * on_device != 0: init_x, samples, final_x, final_lp and info are device pointers on the model's GPU. */
typedef struct {
    int64_t niter;           /* iterations recorded (> 0)                                                */
    int64_t burnin;          /* iterations run first without recording (>= 0)                            */
    int64_t iter_begin;      /* iterations this chain has run before (>= 0): keys the draws             */
    int32_t step_out;        /* 0: the widths are known to be large enough (slice_sample.jl:23-24)       */
    int64_t max_evals;       /* evaluations one coordinate update may spend: 3 .. 2^20, 0 -> 4096        */
} mcmc_slice_cfg;
int mcmc_slice_validate(const mcmc_slice_cfg* cfg);
int mcmc_run_slice(mcmc_model* model, const mcmc_slice_cfg* cfg, int64_t nchains, int64_t chain_offset, uint64_t seed,
                   const double* init_x, const double* widths, int32_t on_device, double* samples, double* final_x,
                   double* final_lp, int32_t* info, int64_t* evals, double* runtime_s, double* kernel_ms);
/* The kernel instance mcmc_run_slice launches for (model kind, d, nchains), as rocprofv3 names it without the namespace
 * ("lpc_slice<NB, Model>", "lpp_slice<NBL, Model>"), its block size and its grid; needs no GPU.  A combination that is
 * not built answers MCMC_E_UNSUPPORTED.  name (cap bytes), threads and grid may be NULL. */
int mcmc_slice_plan(int32_t model_kind, int64_t d, int64_t nchains, char* name, int64_t cap, int32_t* threads,
                    int64_t* grid);
/* the instance the calling thread's last mcmc_run_slice launched ("" before the first) */
int mcmc_slice_last_kernel(char* buf, int64_t cap);

/* ---- output analysis (src/stats/ess.jl:6-10, var.jl:7-117) ----
 * Effective sample size n * var_iid / var_vtype of every (parameter j, chain c) series of
 * samples [nkept][d][nchains] (the mcmc_outputs layout).  vtype: MCMC_VAR_IMSE (Geyer initial
 * monotone sequence), MCMC_VAR_IPSE (initial positive sequence), MCMC_VAR_BM (batch means of
 * `batchlen`).  maxlag <= 0 -> nkept - 1.  Outputs ess[j][c] and optionally var[j][c] (the vtype
 * variance of the mean).  on_device != 0: every pointer is device memory on ctx's GPU. */
enum { MCMC_VAR_IMSE = 1, MCMC_VAR_IPSE = 2, MCMC_VAR_BM = 3 };
int mcmc_stats_ess(mcmc_ctx* ctx, const double* samples, int64_t nkept, int64_t d, int64_t nchains, int32_t vtype,
                   int64_t maxlag, int64_t batchlen, int32_t on_device, double* ess, double* var);

/* describe(chain) (src/stats/summary.jl:24-55) of samples [nkept][d][nchains], in one read of the samples, plus the
 * pooled row a many-chain run is read by.  Both tables are optional; at least one must be asked for.
 *   per_chain [6][d][nchains] or NULL: min, mean, max, mcerror, ess, actime of every (parameter j, chain c) series,
 *     summary.jl:35-42 as written: mean = sum / n, variid = (ss / (n - 1)) / n, varimse the MCMC_VAR_IMSE variance
 *     (maxlag <= 0 -> nkept - 1), mcerror = sqrt(varimse), ess = (n variid) / varimse (bit for bit mcmc_stats_ess's),
 *     actime = varimse / variid; min and max with -0 returned as +0, a NaN sample passed over.
 *   pooled [MCMC_DESCRIBE_NPOOLED + nprobs][d] or NULL: rows min, mean, max, mcerror, ess, rhat (MCMC_DESCRIBE_*), then
 *     the nprobs exact quantiles (Julia's quantile, type 7) of the nkept * nchains values of each parameter.  mean: the
 *     mean over chains of the chain means; mcerror = sqrt(sum_c varimse_c) / C' and ess = sum_c ess_c over the C' chains
 *     whose varimse and ess are finite and varimse > 0; rhat (Gelman-Rubin) = sqrt(((n - 1)/n W + B/n) / W) with
 *     W = mean_c ss_c / (n - 1), B/n = var_c(mean_c) (divisor C - 1), NaN when nchains = 1 or W = 0.  Sums over chains
 *     run in one order fixed by nchains alone.
 *   nbad [d] or NULL (filled with the pooled table): the chains left out of mcerror and ess (a chain that never moved,
 *     or whose first Geyer pair is <= 0); they still count in mean, min, max, rhat and the quantiles.
 * probs: nprobs <= MCMC_DESCRIBE_MAXPROBS probabilities in [0, 1].  nkept < 2, nprobs out of range, a probability
 * outside [0, 1] or both tables NULL answer MCMC_E_INVALID_ARG.  on_device != 0: every pointer is device memory on
 * ctx's GPU. */
enum { MCMC_DESCRIBE_MIN = 0, MCMC_DESCRIBE_MEAN = 1, MCMC_DESCRIBE_MAX = 2, MCMC_DESCRIBE_MCERROR = 3,
       MCMC_DESCRIBE_ESS = 4, MCMC_DESCRIBE_RHAT = 5, MCMC_DESCRIBE_ACTIME = 5 /* per_chain's last column */,
       MCMC_DESCRIBE_NPOOLED = 6, MCMC_DESCRIBE_MAXPROBS = 8 };
int mcmc_stats_describe(mcmc_ctx* ctx, const double* samples, int64_t nkept, int64_t d, int64_t nchains, int64_t maxlag,
                        int32_t on_device, double* per_chain, const double* probs, int32_t nprobs, double* pooled,
                        int64_t* nbad);

/* Zero-variance control-variate estimators (src/stats/zv.jl:8-68) of every chain of samples / grads
 * [nkept][d][nchains].  With z = -grads/2 and w_t the k control variates of kept step t -- MCMC_ZV_LINEAR: k = d,
 * w = z; MCMC_ZV_QUADRATIC: k = d(d+3)/2, the z_j, then 2 z_j x_j - 1, then x_i z_j + x_j z_i for i < j in zv.jl's
 * loop order -- a = -cov(w)^-1 cov(w, x) per chain and zv[t][j] = x[t][j] + sum_i w[t][i] a[i][j].  Built for
 * d <= 32 (linear) and d <= 8 (quadratic); wider answers MCMC_E_UNSUPPORTED.  nkept <= k answers
 * MCMC_E_INVALID_ARG.  A chain whose Gram matrix is not positive definite gets info[c] = the 1-based index of the
 * failing pivot and NaN in its zv and coef columns; info[c] = 0 otherwise.  Two things mark it: fewer than k kept
 * steps that differ from the step before (the matrix then has rank <= moves < k whatever rounding leaves behind:
 * info[c] = moves + 1, so a chain that never moved always gets 1), or a Cholesky pivot <= 0 or not finite.  coef [k][d][nchains] and info [nchains] may be NULL.  on_device != 0: every pointer is
 * device memory on ctx's GPU. */
enum { MCMC_ZV_LINEAR = 1, MCMC_ZV_QUADRATIC = 2 };
int mcmc_stats_zv(mcmc_ctx* ctx, int32_t order, const double* samples, const double* grads, int64_t nkept, int64_t d,
                  int64_t nchains, int32_t on_device, double* zv, double* coef, int32_t* info);

/* ---- diagnostics used by the parity tests: evaluate the build's deterministic
 *      math on the device.  op: 0 log, 1 exp, 2 sin2pi, 3 cos2pi,
 *      4 sqrt, 5 div(x, y), 6 normals (x = block counters), 7 Julia-0.2 round,
 *      8 accept uniform, 9 Box-Muller radius log, 10/11 Box-Muller angle sin/cos,
 *      12 guard-free sqrt of the Box-Muller radius, 13/14 det_exp_tab / det_log_tab, 15 the screened accept test,
 *      16 the Box-Muller radius^2 -2 log u (bm_rad2_u32, bitwise -2 x op 9), 17 the Box-Muller radius
 *      sqrt(-2 log u) (bm_radius_u32, the segment polynomials), 22 / 23 the logistic Bernoulli term / its
 *      eta-derivative weight of (eta = x, w = y) (det_logi). ---- */
int mcmc_debug_detmath(mcmc_ctx* ctx, int op, int64_t n, const double* x, const double* y, double* out);
int mcmc_debug_philox(mcmc_ctx* ctx, int64_t n, const uint32_t* ctr /*[n][4]*/, const uint32_t* key /*[n][2]*/,
                      uint32_t* out /*[n][4]*/);
/* nk chained v_mfma_f64_16x16x4_f64: D = A[16][4nk] * B[4nk][16] + C[16][16] (row-major, host pointers);
   pins the fp64 MFMA accumulation order the regression kernels rely on. */
int mcmc_debug_mfma_f64(mcmc_ctx* ctx, int nk, const double* A, const double* B, const double* C, double* D);
/* The chain order the last run of `chains` launched with (regression HMC / HMCDA run their chains
   sorted by trajectory length, slot -> local chain): *used = 1 and order[0..C) filled, or *used = 0 (identity). */
int mcmc_debug_chains_order(mcmc_chains* chains, int32_t* used, int32_t* order);

#ifdef __cplusplus
}
#endif
#endif
