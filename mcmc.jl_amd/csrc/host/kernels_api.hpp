// kernels_api.hpp -- launch entry points exported by the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common.hpp"
#include "../kernels/launch_plan.hpp"

namespace mcmc {
struct KernelArgs {
    StepArgs s;
    SamplerArgs sa;
    ModelArgs m;
    ChainState st;
};
// the slice-sampling kernels' block (slice.hip)
struct SliceKernelArgs {
    ModelArgs m;
    SliceArgs s;
};
}  // namespace mcmc

// The step kernel a launch function dispatched, as "family<template arguments>" (the instance name rocprofv3
// shows, without the namespace): the launch functions record it, mcmc_chains_step_kernel reports it (tests and
// bench.py check which instance ran).  Host-side, thread-local; printf-style, or an instance of the launch plan
// (kernels/launch_plan.hpp plan_kernel_name formats it) with the model class's kName, a string that outlives the call.
void mcmc_note_step_kernel(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void mcmc_note_step_instance(const mcmc::KernelInstance& k, const char* model);
const char* mcmc_last_step_kernel();

// lane-per-chain kernels (d <= 32), state [d][ld]
hipError_t mcmc_launch_lpc_step(const mcmc::KernelArgs& a, hipStream_t st);
hipError_t mcmc_launch_lpc_eval(const mcmc::KernelArgs& a, const double* xin, double* lp, double* g, int check,
                                hipStream_t st);
int mcmc_lpc_max_d();
// NUTS (nuts.hip), lane-per-chain state, d <= mcmc_nuts_max_d(): the step loop (init == 0), or the initial epsilon
// search after the chains' first evaluation (init != 0); the level stack lives in ChainState::nuts_wv / nuts_ws,
// sized for SamplerArgs::n_leaps (maxdoublings <= mcmc_nuts_max_doublings()) levels
hipError_t mcmc_launch_nuts(const mcmc::KernelArgs& a, int init, hipStream_t st);
int mcmc_nuts_max_d();
int mcmc_nuts_max_doublings();
// slice sampling (slice.hip), lane-per-chain state [d][ld], d <= mcmc_slice_max_d(): a.s.niters whole iterations of
// every chain; the launched instance is noted like a step kernel's
hipError_t mcmc_launch_slice(const mcmc::SliceKernelArgs& a, hipStream_t st);
int mcmc_slice_max_d();
// wave- and block-per-chain kernels (32 < d <= mcmc_wpc_max_d() = 16384; RAM: d <= mcmc_wpc_ram_max_d() = 1024),
// state [C][ld] (ld = row stride, multiple of 4)
hipError_t mcmc_launch_wpc_step(const mcmc::KernelArgs& a, hipStream_t st);
hipError_t mcmc_launch_wpc_eval(const mcmc::KernelArgs& a, const double* xin, double* lp, double* g, int check,
                                hipStream_t st);
int mcmc_wpc_max_d();
int mcmc_wpc_ram_max_d();
// regression models on fp64 MFMA, state [d][ld] (+ gradient [d][ld])
hipError_t mcmc_launch_glm_step(const mcmc::KernelArgs& a, hipStream_t st);
// storeLeaps: record the trajectory of the next step (HMC / HMCDA) without moving the chains
hipError_t mcmc_launch_lpc_record(const mcmc::KernelArgs& a, const mcmc::LeapRec& r, hipStream_t st);
hipError_t mcmc_launch_wpc_record(const mcmc::KernelArgs& a, const mcmc::LeapRec& r, hipStream_t st);
hipError_t mcmc_launch_glm_record(const mcmc::KernelArgs& a, const mcmc::LeapRec& r, hipStream_t st);
hipError_t mcmc_launch_glm_eval(const mcmc::KernelArgs& a, const double* xin, double* lp, double* g, int check,
                                hipStream_t st);
int mcmc_glm_max_d();
// SMMALA on the probit / logistic models, d <= mcmc_smmala_max_d() (smmala.hip), state [d][ld] and packed matrices
// [d(d+1)/2][ld].  The evaluation alone: lp, gradient g, tensor G, and with invG != NULL its inverse and
// ft = invG g; check != 0: a non-finite lp or a failed Cholesky pivot sets the error word
hipError_t mcmc_launch_smmala_eval(const mcmc::KernelArgs& a, const double* xin, double* lp, double* g, double* G,
                                   double* invG, double* ft, int check, hipStream_t st);
hipError_t mcmc_launch_smmala_step(const mcmc::KernelArgs& a, hipStream_t st);
int mcmc_smmala_max_d();
// PMALA on the same models and sizes (pmala.hip).  dtensor: evalalldt, lp / g / G (any may be NULL) as
// mcmc_launch_smmala_eval's and dG [d][d(d+1)/2][ld].  corr: the drift correction st.pm_c of the state's position from
// st.sm_invG (after mcmc_launch_smmala_eval has formed it)
hipError_t mcmc_launch_pmala_dtensor(const mcmc::KernelArgs& a, const double* xin, double* lp, double* g, double* G,
                                     double* dG, hipStream_t st);
hipError_t mcmc_launch_pmala_corr(const mcmc::KernelArgs& a, hipStream_t st);
hipError_t mcmc_launch_pmala_step(const mcmc::KernelArgs& a, hipStream_t st);
// RMHMC on the same models and sizes (rmhmc.hip): the state is x, lp and g; st.sm_pinvG is its workspace
hipError_t mcmc_launch_rmhmc_step(const mcmc::KernelArgs& a, hipStream_t st);
// ERMLMC and RMLMC on the same models and sizes (lmc.hip): the state is x, lp and g; st.sm_pG and st.sm_pinvG are the
// trajectory's workspace
hipError_t mcmc_launch_lmc_step(const mcmc::KernelArgs& a, hipStream_t st);
// RAM on regression targets, 32 < d <= 1024 (glm_ram_wave.hip): per step the eval kernel and the accept / factor-update
// kernel; u [C][ustride], nz [C], xprop [d][ld], lpp [C] are the device buffers between them.  st2 (may be null):
// a second stream on which half of a large batch runs, forked from and joined back to st by the two events
hipError_t mcmc_launch_glm_ram_wave(const mcmc::KernelArgs& a, double* u, double* nz, double* xprop, double* lpp,
                                    hipStream_t st, hipStream_t st2, hipEvent_t ev_fork, hipEvent_t ev_join);
int64_t mcmc_glm_ram_wave_ustride(int d);
// SeqMC population bookkeeping (seqmc.hip)
hipError_t mcmc_seqmc_weights(int64_t N, double* logW, const double* ll0, double* logtarget, const double* plogtarget,
                              hipStream_t st);
hipError_t mcmc_seqmc_scan(int64_t N, const double* logW, double trigger, double* cp, int32_t* flag, hipStream_t st);
hipError_t mcmc_seqmc_resample(int64_t N, int d, const double* cp, const int32_t* flag, uint64_t seed, uint32_t step,
                               uint32_t target, const double* pars, double* pars_out, const double* logtarget,
                               double* logtarget_out, double* logW, hipStream_t st);
hipError_t mcmc_seqmc_store(int64_t N, int d, const double* pars, const double* logW, double* samples, double* weights,
                            hipStream_t st);
// SerialTempMC walker bookkeeping (stemp.hip): every array is [..][C] over the walkers; chain0 the first walker's
// global chain id, step the runner step, seed the run's Philox key.  x: a target's positions as columns, row stride ldx
hipError_t mcmc_stemp_pick(int64_t C, int32_t K, uint32_t chain0, uint64_t seed, uint32_t step, int32_t is_swap,
                           const int32_t* at, int32_t* tgt, hipStream_t st);
hipError_t mcmc_stemp_take(int64_t C, int d, int32_t t, const int32_t* tgt, const double* x, int64_t ldx,
                           const double* ll0, double* cand, double* cand_lt, hipStream_t st);
hipError_t mcmc_stemp_swap(int64_t C, int d, uint32_t chain0, uint64_t seed, uint32_t step, int32_t is_swap,
                           const double* logW, int32_t* at, const int32_t* tgt, double* cur, double* prev, double* lt,
                           const double* cand, const double* cand_lt, int32_t* swapped, hipStream_t st);
hipError_t mcmc_stemp_store(int64_t C, int d, const double* cur, const int32_t* at, const int32_t* swapped,
                            double* samples, int32_t* models, uint64_t* bits, hipStream_t st);
// effective sample size of every (parameter, chain) series of samples [n][d][C] (stats.hip)
hipError_t mcmc_launch_ess(const double* samples, int64_t n, int64_t d, int64_t C, int32_t vtype, int64_t maxlag,
                           int64_t batchlen, double* ess, double* var, hipStream_t st);
// describe's tables (describe.hip) of samples [n][d][C], every pointer but probs device memory: per_chain [6][d][C]
// or NULL; pooled [6 + nprobs][d] or NULL (then probs, nprobs and nbad are not looked at); nbad [d] or NULL; ws a
// workspace of mcmc_describe_ws_bytes.  IMSE with maxlag as mcmc_launch_ess takes it
size_t mcmc_describe_ws_bytes(int64_t d, int64_t C, int has_per_chain, int has_pooled, int32_t nprobs);
hipError_t mcmc_launch_describe(const double* samples, int64_t n, int64_t d, int64_t C, int64_t maxlag,
                                double* per_chain, const double* probs, int32_t nprobs, double* pooled, int64_t* nbad,
                                void* ws, hipStream_t st);
// zero-variance estimators (zv.hip): order 1 linear, 2 quadratic; samples x and gradients g [n][d][C] -> zv [n][d][C],
// coef [k][d][C] (or NULL), info [C] (or NULL).  d <= mcmc_zv_max_d(order); k = mcmc_zv_k(order, d)
hipError_t mcmc_launch_zv(int order, const double* x, const double* g, int64_t n, int d, int64_t C, double* zv,
                          double* coef, int32_t* info, hipStream_t st);
int mcmc_zv_max_d(int order);
int64_t mcmc_zv_k(int order, int64_t d);
// padded coordinate count of the regression kernels; their 16-chain tiles per workgroup
int mcmc_glm_d_pad(int d);
int mcmc_glm_tiles_per_wg(int d);
// the regression kernels' staged-tile image of X and Y (glm_layout.hpp): its size in doubles, and the packing
size_t mcmc_glm_image_doubles(int d, int64_t n);
void mcmc_glm_pack_image(int d, int64_t n, const double* X, const double* Y, const double* B, double* img);
// steps one launch of the regression step kernel may fuse (0: any)
int mcmc_glm_steps_per_launch(int d, int64_t n, int sampler_kind);

hipError_t mcmc_fill_f64(double* p, int64_t n, double v, hipStream_t st);
hipError_t mcmc_fill_f64_strided(double* p, int64_t nb, int64_t w, int64_t stride, double v, hipStream_t st);
hipError_t mcmc_fill_i32(int32_t* p, int64_t n, int32_t v, hipStream_t st);
hipError_t mcmc_broadcast_cols(double* dst, int64_t ldd, const double* v, int d, int64_t C, hipStream_t st);
hipError_t mcmc_broadcast_rows(double* dst, int64_t ldr, const double* v, int d, int64_t C, hipStream_t st);
hipError_t mcmc_copy_cols(double* dst, int64_t ldd, const double* src, int64_t lds, int d, int64_t C, hipStream_t st);
// dst[b][s][r] (row stride ldd) <- src[b][r][s] (row stride lds), r < R, s < S; batch strides R*lds / S*ldd
hipError_t mcmc_transpose(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t batch, int64_t R,
                          int64_t S, hipStream_t st);
hipError_t mcmc_detmath(int op, int64_t n, const double* x, const double* y, double* out, hipStream_t st);
hipError_t mcmc_philox(int64_t n, const uint32_t* ctr, const uint32_t* key, uint32_t* out, hipStream_t st);
hipError_t mcmc_mfma_probe(const double* A, const double* B, const double* C, double* D, int nk, hipStream_t st);
