// glm_device.hpp -- the device side of the regression family on fp64 MFMA that more than one translation unit
// needs (glm.hip, glm_mala1ws.hip, smmala.hip): the logistic (examples/logistic_regression.jl:16-22), linear
// (examples/linear_regression.jl:14-20) and probit log-targets with their gradients (glm_eval, glm_eval1), the
// workgroup geometry and LDS carve-up, the state access functions and the samplers' shared pieces; host side, the
// launch arguments, grid and LDS size.
//
// Mapping.  A wave owns a tile of 16 chains; the dense contractions are
//     eta[obs][chain] = X[obs][:] . beta[:][chain]        (v_mfma_f64_16x16x4_f64, K = coordinates)
//     G[coord][chain] = X[:][coord] . r[:][chain]          (same instruction, K = observations)
// per 16-observation tile of X staged in LDS and shared by the workgroup's waves.  Lane l holds
// chain cl = l & 15 and quarter q = l >> 4; for d-slice s (d > 64 is split over NW = d_pad/64
// waves) it owns coordinates k = s*DS + 16m + 4q + e (m < DS/16, e < 4), which are exactly the four
// normals of Philox blocks k/4 -- so proposals, momenta, gradients and every per-coordinate term
// stay lane-local.  The MFMA row <-> coordinate maps are permuted to make that so:
//     eta k-slice kk (= 4m + e), row q      <-> coordinate 16m + 4q + e
//     G tile T, row i (= 4r + q')           <-> coordinate 16T + 4q' + r
// and the eta accumulator (obs q + 4r on lane (q, cl)) is, register for register, the B operand
// of the G product (k-slice r): no data movement between the two MFMA chains.
//
// Arithmetic (restated by oracle/oracle.c orc_glm_eval): v_mfma_f64_16x16x4_f64 is a
// sequential fma chain over its k (probed bitwise on gfx950, scripts/probe_mfma.py), so eta is an
// fma chain over coordinates in (m, e, q) order per slice, slices added left to right; G is an fma
// chain over observations; per-coordinate sums are lane partials in (m, e) order combined as
// (q0 + q2) + (q1 + q3), then slices left to right.
#pragma once
#include "../common.hpp"
#include "../detmath.hpp"
#include "../models.hpp"
#include "../glm_layout.hpp"
#include "../host/kernels_api.hpp"
#include "glm_stamps.hpp"

namespace mcmc {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// workgroup: one slice (NW = 1): 4 waves = 4 tiles of 16 chains; d-sliced (NW = 2, 4, 8): 8 waves = 8 / NW tiles
template <int NW>
constexpr int glm_block() { return NW == 1 ? 256 : 512; }
constexpr int kGlmMaxWaves = 8;
// NM (template parameter) = DS/16 in {1, 2, 4, 8}: the lane owns NS = 4*NM coordinates.

struct GlmShape {
    int nw;          // waves per 16-chain tile (d-slices)
    int tpw;         // tiles per workgroup = max(4, nw) / nw
    int ds;          // coordinates per wave
    int nm;          // ds / 16
    int d_pad;
    int lds_stride;  // X tile row stride (doubles), glm_row_stride(d_pad)
    int ts;          // doubles per staged tile (rows, then Y), glm_tile_doubles(d_pad)
    int64_t n_pad;
};

struct GlmArgs {
    StepArgs s;
    SamplerArgs sa;
    ModelArgs m;
    ChainState st;
    GlmShape g;
    LeapRec rec;      // storeLeaps record (glm_hmc<..., REC = true>); zero otherwise
};

}  // namespace mcmc

// the geometry of a (d, n) regression model (glm.hip)
mcmc::GlmShape mcmc_glm_shape(int d, int64_t n);
// one step of single-slice MALA (a.g.nw == 1): the wave-specialised kernel (glm_mala1ws.hip)
hipError_t mcmc_launch_glm_mala1ws(const mcmc::GlmArgs& a, dim3 grid, hipStream_t st);

namespace mcmc {

// lane position inside the workgroup
struct GlmPos {
    int lane, q, cl, wave, slice, tile;
    int64_t c;
    bool live;
    int base;
};

__device__ __forceinline__ GlmPos glm_pos(const GlmArgs& a) {
    GlmPos p;
    p.lane = threadIdx.x & 63;
    p.q = p.lane >> 4;
    p.cl = p.lane & 15;
    p.wave = threadIdx.x >> 6;
    p.slice = p.wave % a.g.nw;
    p.tile = p.wave / a.g.nw;
    const int64_t slot = ((int64_t)blockIdx.x * a.g.tpw + p.tile) * 16 + p.cl;
    p.live = slot < a.s.C;
    // every chain-indexed access below goes through p.c; a tile's MFMA columns are independent chains, so the
    // permutation changes which chains share a tile (and its leapfrog loop), never a chain's arithmetic
    p.c = (a.s.order != nullptr && p.live) ? (int64_t)a.s.order[slot] : slot;
    p.base = p.slice * a.g.ds;
    return p;
}

__device__ __forceinline__ int own_coord(const GlmPos& p, int slot) {
    return p.base + 16 * (slot >> 2) + 4 * p.q + (slot & 3);
}

// tile buffers in LDS (each glm_tile_doubles: 16 X rows in the glm_layout.hpp image, then Y): the d-sliced
// evaluation double-buffers, the single-slice one (glm_eval1) keeps three (tile t for G, t+1 for eta, t+2 being
// written); at d_pad = 1024 one tile is 129 KB, so the d-sliced evaluation keeps one (glm_eval: staged after the
// tile's last reader, behind a barrier)
__host__ __device__ constexpr int glm_xbufs(int nw, int d_pad) { return nw == 1 ? 3 : (d_pad > 512 ? 1 : 2); }

// LDS carve-up (doubles): tiles [xbufs][ts] | eta partials [8 waves][64][4] (single-slice kernels: the logistic
// term's table, kSoftplusTab, instead) | chain scalars [8 waves][16] | residual weights [4 tiles][4][64] | int scratch
struct GlmLds {
    double* X;
    double* part;
    double* scal;
    double* rbuf;     // [4 tiles][4 r][64 lanes]: residual weights of a tile, exchanged between slice waves
    int* iscr;
};

__host__ __device__ constexpr int glm_part_doubles(int nw) {
    return nw == 1 && SP_NROWS * 10 > kGlmMaxWaves * 64 * 4 ? SP_NROWS * 10 : kGlmMaxWaves * 64 * 4;
}

__device__ __forceinline__ GlmLds glm_lds(const GlmArgs& a, double* smem) {
    GlmLds L;
    L.X = smem;
    L.part = L.X + glm_xbufs(a.g.nw, a.g.d_pad) * a.g.ts;                 // tile buffers
    L.scal = L.part + glm_part_doubles(a.g.nw);
    L.rbuf = L.scal + kGlmMaxWaves * 16;
    L.iscr = (int*)(L.rbuf + 4 * 4 * 64);
    return L;
}

// The single-slice term 4 * 4 NM * 64 was the one-wave MALA kernel's proposal area; no kernel reads it any more.  It
// stays in the size so that every kernel's LDS footprint (and with it the workgroups a CU holds) is what was measured.
inline size_t glm_lds_bytes(const GlmShape& g) {
    return (size_t)(glm_xbufs(g.nw, g.d_pad) * g.ts + glm_part_doubles(g.nw) + kGlmMaxWaves * 16 +
                    4 * 4 * 64 + 2 + (g.nw == 1 ? 4 * 4 * g.nm * 64 : 0)) * 8
#ifdef GLM_STAMP
           + 16 + (g.nw > 1 ? kGlmStampLdsBytes : 0)
#endif
        ;
}

// sum of a per-chain quantity held as 4 quarter partials per wave and NW slice partials:
// (q0 + q2) + (q1 + q3), then slices left to right.  Contains a barrier when nw > 1:
// every wave of the workgroup must reach it.
__device__ __forceinline__ double glm_sum(const GlmArgs& a, const GlmPos& p, const GlmLds& L, double v) {
    v = v + __shfl_xor(v, 32, 64);
    v = v + __shfl_xor(v, 16, 64);
    if (a.g.nw == 1) return v;
    __syncthreads();
    if (p.q == 0) L.scal[p.wave * 16 + p.cl] = v;
    __syncthreads();
    double t = L.scal[(p.tile * a.g.nw) * 16 + p.cl];
    for (int s = 1; s < a.g.nw; ++s) t = t + L.scal[(p.tile * a.g.nw + s) * 16 + p.cl];
    return t;
}

// workgroup-wide max of a per-chain integer (leapfrog counts): every wave must reach it.
__device__ __forceinline__ int64_t glm_max(const GlmLds& L, int64_t v, bool live) {
    __syncthreads();
    if (threadIdx.x == 0) L.iscr[0] = 1;
    __syncthreads();
    if (live) atomicMax(&L.iscr[0], (int)v);
    __syncthreads();
    const int r = L.iscr[0];
    __syncthreads();
    return r;
}

// the workgroup-wide max of a per-chain integer and the max over this wave's chain tile (d-sliced geometry: at most
// two tiles a workgroup); every wave must reach it
__device__ __forceinline__ int64_t glm_max_tile(const GlmLds& L, int64_t v, bool live, int tile, int64_t& tmax) {
    __syncthreads();
    if (threadIdx.x == 0) {
        L.iscr[0] = 1;
        L.iscr[1] = 1;
        L.iscr[2] = 1;
    }
    __syncthreads();
    if (live) {
        atomicMax(&L.iscr[0], (int)v);
        atomicMax(&L.iscr[1 + tile], (int)v);
    }
    __syncthreads();
    const int r = L.iscr[0];
    tmax = L.iscr[1 + tile];
    __syncthreads();
    return r;
}

// The lane's coordinates of the evaluation point, held in registers
template <int NS>
struct XArr {
    const double (&v)[NS];
    __device__ __forceinline__ double operator()(int s) const { return v[s]; }
};

// The end of an evaluation: likelihood partials combined (quarters, then slices left to right), the
// prior vars ~ Normal(0, sp) over own coordinates, the LLAcc rule, and the prior's gradient added to G.
template <int NM, int NW, bool GRAD, class XA>
__device__ __forceinline__ double glm_finish(const GlmArgs& a, const GlmPos& p, const GlmLds& L,
                                          const XA& x, f64x4 (&G)[NM], double lik_part, bool& oos, bool on = true) {
    const ModelArgs& M = a.m;
    const int d = M.d;
    const double lik = glm_sum(a, p, L, lik_part);
    // prior vars ~ Normal(0, sp) over own coordinates
    const double sp = M.prior_sigma, s2p = sp * sp, logsp = det_log(sp);
    double pp = 0.0;
#pragma unroll
    for (int slot = 0; slot < (4 * NM); ++slot) {
        const int k = own_coord(p, slot);
        if (true && k < d) {
            const double z = (x(slot) - 0.0) / sp;
            pp = pp + (-0.5 * (z * z + kLog2Pi) - logsp);
        }
    }
    const double prior = glm_sum(a, p, L, pp);
    double acc = 0.0 + prior;                                           // LLAcc(0.) + ...
    bool bad = !(acc - acc == 0.0);
    acc = acc + lik;
    bad = bad || !(acc - acc == 0.0);
    oos = bad;
    if (bad) acc = -__builtin_inf();
    if (GRAD && on) {
#pragma unroll
        for (int slot = 0; slot < (4 * NM); ++slot)
            G[slot >> 2][slot & 3] = bad ? 0.0 : (0.0 - x(slot)) / s2p + G[slot >> 2][slot & 3];
    }
    return acc;
}

// The probit model's elementwise part for one observation (examples/probit_regression.jl:26-40; oracle orc_glm_eval):
// term = y logcdf(N, eta) + (1 - y) logcdf(N, -eta), and its eta-derivative, the example's grad_log_posterior weight
// y exp(A - logcdf(N, eta)) - (1 - y) exp(A - logcdf(N, -eta)), A = -(eta^2 + log(2 pi))/2
__device__ __forceinline__ void glm_probit_obs(double eta, double y, double& term, double& w) {
    const double la = det_normlogcdf(eta), lb = det_normlogcdf(-eta);
    term = y * la + (1.0 - y) * lb;
    const double A = (-(eta * eta + kLog2Pi)) / 2.0;
    w = y * det_exp(A - la) - (1.0 - y) * det_exp(A - lb);
}

// Single-slice evaluation (NW = 1: the wave holds all d_pad coordinates of its 16 chains), software
// pipelined over the 16-observation tiles with three LDS tile buffers:
//     iteration t:  eta_{t+1} = X_{t+1} beta   (MFMA chain, buffer (t+1) % 3)
//                   elementwise on eta_t        (VALU, independent of the chain above: the two interleave)
//                   G += X_t^T r_t              (MFMA, buffer t % 3)
//                   tile t+2 -> buffer (t+2) % 3 (its last readers finished before the previous barrier)
//                   one barrier
// The arithmetic is glm_eval's, operation for operation (eta chains over (m, e, q); G chains over
// observations; a lane's likelihood terms in (t, r) order), so the oracle's orc_glm_eval restates both.
template <int NM, bool GRAD, bool LOGI, class XA>
__device__ __forceinline__ double glm_eval1_tiles(const GlmArgs& a, const GlmPos& p, const GlmLds& L,
                                                const XA& x, f64x4 (&G)[NM]) {
    const ModelArgs& M = a.m;
    const GlmShape& g = a.g;
    constexpr int S = glm_row_stride(16 * NM);
    const bool probit = !LOGI && M.kind == MK_PROBIT;          // probit runs in the linear instantiation (uniform)
    const double sn = M.noise_sigma, s2n = sn * sn;
    const double logsn = LOGI ? 0.0 : det_log(sn);
    const double isn = 1.0 / sn, is2n = 1.0 / s2n;
    double lik_part = 0.0;
    const int64_t ntiles = g.n_pad / 16;
    constexpr int kBlk = glm_block<1>();
    constexpr int DP = 16 * NM;
    constexpr int XS = glm_tile_doubles(DP);                  // one staged tile: X rows, then Y
    constexpr int YO = glm_y_offset(DP);
    constexpr int BO = glm_b_offset(DP);
    constexpr int kHalf = XS / 2;                             // f64x2 per tile
    constexpr int kPer = (kHalf + kBlk - 1) / kBlk;
    static_assert(glm_row_stride(DP) > 0, "");
    f64x2 buf[kPer];
    // the tile image moves linearly (glm_layout.hpp): HBM tile tt -> LDS buffer b
    auto load_tile = [&](int64_t tt) {
        const f64x2* src = reinterpret_cast<const f64x2*>(M.X + (size_t)tt * XS);
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int i = threadIdx.x + kBlk * j;
            buf[j] = src[i < kHalf ? i : 0];
        }
    };
    auto store_tile = [&](int b) {
        f64x2* dst = reinterpret_cast<f64x2*>(L.X + b * XS);
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int i = threadIdx.x + kBlk * j;
            if (i < kHalf) dst[i] = buf[j];
        }
    };
    const int eta_lane = p.cl * S + 4 * p.q;              // + glm_eta_off(slot): coordinate 16m + 4q + e
    // eta of the tile in buffer b: k-slice kk = 4m + e, row q <-> coordinate 16m + 4q + e
    auto eta_of = [&](int b) {
        f64x4 e = f64x4{0.0, 0.0, 0.0, 0.0};
        const double* xrow = L.X + b * XS + eta_lane;
#pragma unroll
        for (int slot = 0; slot < (4 * NM); ++slot)
            e = __builtin_amdgcn_mfma_f64_16x16x4f64(xrow[glm_eta_off(slot)], x(slot), e, 0, 0, 0);
        return e;
    };
    load_tile(0);
    store_tile(0);
    if (ntiles > 1) {
        load_tile(1);
        store_tile(1);
    }
    // logistic: the term's segment-polynomial table (det_logi) staged in the eta-partials area, which the
    // single-slice kernels do not otherwise use
    const double (*sptab)[10] = reinterpret_cast<const double (*)[10]>(L.part);
    if (LOGI) {
        for (int i = threadIdx.x; i < SP_NROWS * 10; i += kBlk) L.part[i] = (&kSoftplusTab[0][0])[i];
    }
    if (GRAD) {
#pragma unroll
        for (int T = 0; T < NM; ++T) G[T] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    __syncthreads();
    f64x4 eta = eta_of(0);
    double ubnd = -__builtin_inf();                           // logistic: max of u + b over the lane's observations
    const int64_t nfull = M.n / 16;                           // tiles without padded observations
    int b = 0;                                                // buffer of tile t
    for (int64_t t = 0; t < ntiles; ++t) {
        const bool more = t + 2 < ntiles;
        if (more) load_tile(t + 2);
        const int b1 = b == 2 ? 0 : b + 1, b2 = b1 == 2 ? 0 : b1 + 1;
        // eta_{t+1} (buffer b1; garbage past the last tile, unused) interleaved with the elementwise work on
        // eta_t in the source: the rows' work runs in NSUB sub-stages, and sub-stage j is preceded by the eta MFMAs
        // [j KM / NSUB, (j+1) KM / NSUB), KM = 4 NM (an in-order wave can only overlap a dependent MFMA chain with
        // VALU placed between its MFMAs).  The final interleaving is the compiler's: a scheduling fence after every
        // sub-stage, which pinned the source order, ran config 3 3.7 % slower and is gone.
        // The eta operands are read from LDS kLA MFMAs ahead.
        constexpr int KM = 4 * NM;
        constexpr int kLA = 4;
        f64x4 eta_next = f64x4{0.0, 0.0, 0.0, 0.0};
        const double* xrow1 = L.X + b1 * XS + eta_lane;
        const double* LY = L.X + b * XS + YO;
        const double* LB = L.X + b * XS + BO;
        double av[KM];
#pragma unroll
        for (int m = 0; m < (kLA < KM ? kLA : KM); ++m) av[m] = xrow1[glm_eta_off(m)];
        double y[4], bnd[4], term[4], rv[4];                    // y: the response, for the logistic model w (det_logi)
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = LY[p.q + 4 * r];
        if (LOGI) {
#pragma unroll
            for (int r = 0; r < 4; ++r) bnd[r] = LB[p.q + 4 * r];
        }
        // sub-stage j: the eta MFMAs [j KM / NSUB, (j+1) KM / NSUB), then all four rows of the lane, four independent
        // dependency chains (GR: linear, probit); logistic: one row's whole det_logi a sub-stage (its state stays in
        // registers only that long)
        constexpr bool GR = !LOGI;
        constexpr int NSUB = GR ? 1 : 4;
#pragma unroll
        for (int j = 0; j < NSUB; ++j) {
#pragma unroll
            for (int m = j * KM / NSUB; m < (j + 1) * KM / NSUB; ++m) {
                if (m + kLA < KM) av[m + kLA] = xrow1[glm_eta_off(m + kLA)];
                eta_next = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], x(m), eta_next, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (!GR && r != (j & 3)) continue;
                if (LOGI) {
                    // prob = 1/(1+exp(-X*vars)); Y ~ Bernoulli(prob); its eta-derivative (MCMCDerivRules.jl:111)
                    LogiState E;
                    det_logi_s1(eta[r], y[r], E, sptab);
                    ubnd = __builtin_fmax(ubnd, E.u + bnd[r]);                    // the reference's -Inf
                    det_logi_s2(E);
                    det_logi_fin(E, y[r], term[r], rv[r]);
                } else if (probit) {
                    glm_probit_obs(eta[r], y[r], term[r], rv[r]);
                } else {
                    const double resid = y[r] - eta[r];                             // resid = Y - X*vars
                    const double z = resid * isn;
                    term[r] = -0.5 * (z * z + kLog2Pi) - logsn;                     // resid ~ Normal(0, sn)
                    rv[r] = resid * is2n;
                }
            }
        }
        if (t < nfull) {                                                        // uniform: no padded observation
#pragma unroll
            for (int r = 0; r < 4; ++r) lik_part = lik_part + term[r];          // the lane's terms in (t, r) order
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool in = t * 16 + p.q + 4 * r < M.n;
                lik_part = in ? lik_part + term[r] : lik_part;
                rv[r] = in ? rv[r] : 0.0;
            }
        }
        if (GRAD) {
            // G tile T, k-slice kk: A[i][k] = X[obs 4kk+q][coord 16T+4(i&3)+(i>>2)], i = cl; kk outer so that
            // consecutive MFMAs feed independent accumulators; operands one kk ahead, a fence after each k-slice
            const double* gcol = L.X + b * XS + p.q * S + 4 * (p.cl & 3) + (p.cl >> 2);
            double ga[NM];
#pragma unroll
            for (int T = 0; T < NM; ++T) ga[T] = gcol[glm_g_off(T)];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                double gn[NM];
                if (kk < 3) {
#pragma unroll
                    for (int T = 0; T < NM; ++T) gn[T] = gcol[4 * (kk + 1) * S + glm_g_off(T)];
                }
#pragma unroll
                for (int T = 0; T < NM; ++T) G[T] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[T], rv[kk], G[T], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (kk < 3) {
#pragma unroll
                    for (int T = 0; T < NM; ++T) ga[T] = gn[T];
                }
            }
        }
        if (more) store_tile(b2);                             // held tile t-1: read before the last barrier
        __syncthreads();
        eta = eta_next;
        b = b1;
    }
    return LOGI && ubnd >= 0.0 ? -__builtin_inf() : lik_part;
}

template <int NM, bool GRAD, class XA>
__device__ __forceinline__ double glm_eval1(const GlmArgs& a, const GlmPos& p, const GlmLds& L,
                                         const XA& x, f64x4 (&G)[NM], bool& oos) {
    const double lik_part = a.m.kind == MK_LOGISTIC ? glm_eval1_tiles<NM, GRAD, true>(a, p, L, x, G)
                                                    : glm_eval1_tiles<NM, GRAD, false>(a, p, L, x, G);
    return glm_finish<NM, 1, GRAD>(a, p, L, x, G, lik_part, oos);
}

// LDS-DMA of staged tile tt into an LDS buffer: the image is contiguous (glm_layout.hpp), so each wave moves whole
// 1-KiB pieces (global_load_lds_dwordx4: LDS M0 + 16 lane bytes), pieces w, w + 8, ... of the tile.  The copy is
// counted on vmcnt only: the reader waits vmcnt(0) (glm_dma_wait) and passes a barrier after it (glm_eval).
// Written as inline asm: the compiler's waitcnt pass treats a __builtin_amdgcn_global_load_lds as an LDS store
// that may alias every later ds_write, and put an s_waitcnt vmcnt(0) before the eta-partial store right after the
// eta MFMAs -- draining the next tile's copy a few hundred cycles after it was issued (r04 ISA).  The asm is
// opaque to that pass.  The LDS address goes in through the "{m0}" operand constraint: the compiler writes M0
// itself and knows what it holds afterwards (M0 is a reserved register, so a clobber would not be honoured).
// Loads the pass does track stay correctly waited for: vmcnt decrements in issue order, so an extra load in flight
// only makes its counted waits longer.
template <int TS>
constexpr int glm_dma_pieces_per_wave() { return (TS / 128 + 7) / 8; }
// piece j (0 <= j < glm_dma_pieces_per_wave) of this wave's share of tile image img -> LDS buffer buf
template <int TS>
__device__ __forceinline__ void glm_dma_piece(const double* img, double* buf, int j) {
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    constexpr int kPieces = TS / 128;
    const int c = w + 8 * j;
    if (c < kPieces) {
        const double* src = img + c * 128 + 2 * lane;
        const uint32_t lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(uintptr_t)buf + (uint32_t)c * 1024u));
        asm volatile("global_load_lds_dwordx4 %0, off" :: "v"(src), "{m0}"(lds) : "memory");
    }
}
template <int TS>
__device__ __forceinline__ void glm_dma_tile(const double* img, double* buf) {
#pragma unroll
    for (int j = 0; j < glm_dma_pieces_per_wave<TS>(); ++j) glm_dma_piece<TS>(img, buf, j);
}
// tile image img -> LDS buffer buf by the NWV waves of one role (w: the wave's index among them, wave-uniform),
// pieces w, w + NWV, ... (glm_mala1ws: the V waves stage the X ring)
template <int TS, int NWV>
__device__ __forceinline__ void glm_dma_tile_w(const double* img, double* buf, int w) {
    constexpr int kPieces = TS / 128;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < (kPieces + NWV - 1) / NWV; ++j) {
        const int c = w + NWV * j;
        if (c < kPieces) {
            const double* src = img + c * 128 + 2 * lane;
            const uint32_t lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(uintptr_t)buf + (uint32_t)c * 1024u));
            asm volatile("global_load_lds_dwordx4 %0, off" :: "v"(src), "{m0}"(lds) : "memory");
        }
    }
}
// a workgroup barrier for LDS data written by ds_write (lgkmcnt) that leaves LDS-DMAs in flight: __syncthreads()
// would also wait vmcnt(0), draining the next tile's copy (cdna_hip_programming.md §5, pipelining across barriers)
__device__ __forceinline__ void glm_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
__device__ __forceinline__ void glm_dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// log-target and (GRAD) gradient of the regression model at the lane's coordinates x.
// Every wave of the workgroup calls it the same number of times (barriers inside).
// gout doubles as the MFMA accumulator of G = X^T r (G[T] covers slots 4T..4T+3).
//
// d-sliced form (NW = 2, 4, 8 slices of DS = 16 NM = 128 coordinates; 8 / NW tiles of 16 chains per workgroup):
// per 16-observation tile t, in LDS buffer t & 1 (one buffer at d_pad = 1024),
//     LDS-DMA of tile t+1 into the other buffer (issued first, waited for at the end of the iteration)
//     eta partial over the wave's slice (NM k-groups of MFMAs, operands read kLA ahead)  -> part[wave]
//     barrier; the slice wave owning row r of its tile adds the NW partials left to right, the likelihood term and
//     residual weight of that row -> rbuf[tile][r]
//     barrier; every wave reads its tile's 4 rows' weights; G += X_t^T r (NM independent accumulators)
//     vmcnt(0) + barrier: tile t+1 has landed and tile t's buffer, part and rbuf are free again.
// Two tiles of chains share each staged tile (reuse 32 chains per X byte from L2 / MALL).
// on = false (wave-uniform; a chain tile whose every chain has finished its trajectory, glm_hmc): the wave takes its
// share of the staging and every barrier, and skips its MFMAs and elementwise work; G is left as it is, and the
// returned value and oos are undefined: neither is the log-target's (no likelihood term was summed), so the caller
// keeps its own and must not read them.
template <int NM, int NW, bool GRAD>
__device__ __forceinline__ double glm_eval(const GlmArgs& a, const GlmPos& p, const GlmLds& L,
                                        const double (&x)[(4 * NM)], f64x4 (&G)[NM], bool& oos, bool on = true) {
    if constexpr (NW == 1) return glm_eval1<NM, GRAD>(a, p, L, XArr<4 * NM>{x}, G, oos);
    const ModelArgs& M = a.m;
    const GlmShape& g = a.g;
    constexpr int DP = 16 * NM * NW;
    constexpr int S = glm_row_stride(DP);
    constexpr int XS = glm_tile_doubles(DP);
    constexpr int YO = glm_y_offset(DP);
    constexpr int BO = glm_b_offset(DP);
    constexpr bool kOneBuf = DP > 512;                        // glm_xbufs: one LDS tile buffer
    const bool logistic = M.kind == MK_LOGISTIC;
    const double sn = M.noise_sigma, s2n = sn * sn;
    const double logsn = logistic ? 0.0 : det_log(sn);
    const double isn = 1.0 / sn, is2n = 1.0 / s2n;
    if (GRAD && on) {
#pragma unroll
        for (int T = 0; T < NM; ++T) G[T] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    double lik_part = 0.0;
    double ubnd = -__builtin_inf();                           // logistic: max of u + b over the lane's observations
    const int64_t ntiles = g.n_pad / 16;
    const int eta_lane = p.cl * S + 4 * p.q + p.base;                       // + glm_eta_off(slot)
    const int g_lane = p.q * S + 4 * (p.cl & 3) + (p.cl >> 2) + p.base;   // + 4 kk S + glm_g_off(T)
#ifdef GLM_STAMP
    unsigned* const stamp_lds = reinterpret_cast<unsigned*>(L.iscr + 4);
#endif
    glm_dma_tile<XS>(M.X, L.X);
    glm_dma_wait();
    __syncthreads();
    for (int64_t t = 0; t < ntiles; ++t) {
        GLM_STAMPT(0);
        const int b = kOneBuf ? 0 : (int)(t & 1);
        const double* LX = L.X + b * XS;
        const bool more = t + 1 < ntiles;
        const double* const nimg = M.X + (size_t)(t + 1) * XS;
        double* const nbuf = L.X + (b ^ 1) * XS;
        // the wave's share of tile t+1's DMA: one piece after every kDmaSpread-th eta MFMA; all here without them.
        // Issued all at the loop top, the pieces delayed the second tile's eta (config 5, spread 2: 0.584 -> 0.605 of
        // the fp64 spec; 1 and 4 measured 2 % slower, profiles/r06_ab_glm.md)
        constexpr int kDmaSpread = 2;
        if (!on && more && !kOneBuf) glm_dma_tile<XS>(nimg, nbuf);
        // eta partial over this wave's coordinates: k-slice kk = 4m + e, row q <-> coord base+16m+4q+e.  Every operand
        // read is issued before the first MFMA (a scheduling fence keeps them there: left alone, the scheduler sank
        // each read next to its MFMA and the chain waited out every LDS round trip); the waitcnt pass then waits
        // for each MFMA's own read only.
        constexpr int RPW = NW >= 4 ? 1 : 4 / NW;
        const int r0 = p.slice * RPW;
        const double* LY = LX + YO;
        double yv[RPW], bv[RPW];
#pragma unroll
        for (int rr_ = 0; rr_ < RPW; ++rr_) yv[rr_] = LY[p.q + 4 * ((r0 + rr_) & 3)];
        if (logistic) {
#pragma unroll
            for (int rr_ = 0; rr_ < RPW; ++rr_) bv[rr_] = LX[BO + p.q + 4 * ((r0 + rr_) & 3)];
        }
        f64x4 eta = f64x4{0.0, 0.0, 0.0, 0.0};
        if (on) {
            constexpr int KM = 4 * NM;
            // eta A-operand reads this far ahead of their MFMA in the 128-wide slices (the 64-wide ones read all 16
            // before the first MFMA): 4 measured the same, 16 2.6 % slower on config 5 (profiles/r06_ab_glm.md)
            constexpr int kEtaLA = 8;
            constexpr int kLA = NM <= 4 ? KM : kEtaLA;
            const double* xrow = LX + eta_lane;
            double av[KM];
#pragma unroll
            for (int m = 0; m < kLA; ++m) av[m] = xrow[glm_eta_off(m)];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < KM; ++m) {
                if (m + kLA < KM) av[m + kLA] = xrow[glm_eta_off(m + kLA)];
                eta = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], x[m], eta, 0, 0, 0);
                constexpr int SP = kDmaSpread;
                if (!kOneBuf && m % SP == SP - 1 && m / SP < glm_dma_pieces_per_wave<XS>()) {   // after every SP-th
                    if (more) glm_dma_piece<XS>(nimg, nbuf, m / SP);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (!kOneBuf && more) {
#pragma unroll
                for (int j = KM / kDmaSpread; j < glm_dma_pieces_per_wave<XS>(); ++j) glm_dma_piece<XS>(nimg, nbuf, j);
            }
        }
        // Elementwise part, split over the slice waves: wave slice s owns observation rows r in
        // [s*RPW, (s+1)*RPW) of its tile (obs 16t + q + 4r for lane (q, cl)); with NW = 8 slices 4..7 own
        // none.  Its eta is the slices' partials added left to right.  Partials are [wave][r][lane] (lane-contiguous
        // 8-byte stores and loads: no bank conflicts), all NW of a row read before the first add.
        {
            double* mine = L.part + p.wave * 256 + p.lane;
#pragma unroll
            for (int r = 0; r < 4; ++r) mine[64 * r] = eta[r];
        }
        GLM_STAMPT(1);
        glm_lds_barrier();
        GLM_STAMPT(2);
        double rv[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int rr_ = 0; rr_ < RPW; ++rr_) {
            const int r = r0 + rr_;
            if (r >= 4 || !on) break;
            double pe[NW];
#pragma unroll
            for (int sl = 0; sl < NW; ++sl) pe[sl] = L.part[(p.tile * NW + sl) * 256 + r * 64 + p.lane];
            double e = pe[0];
#pragma unroll
            for (int sl = 1; sl < NW; ++sl) e = e + pe[sl];
            const int64_t obs = t * 16 + p.q + 4 * r;
            const double y = yv[rr_];
            double term, w;
            if (logistic) {
                // prob = 1/(1+exp(-X*vars)); Y ~ Bernoulli(prob); MCMCDerivRules.jl:111 (y: the image's w, det_logi)
                LogiState E;
                det_logi_s1(e, y, E);
                ubnd = __builtin_fmax(ubnd, E.u + bv[rr_]);                  // the reference's -Inf (logi_bound)
                det_logi_s2(E);
                det_logi_fin(E, y, term, w);
            } else if (M.kind == MK_PROBIT) {
                glm_probit_obs(e, y, term, w);
            } else {
                const double resid = y - e;                             // resid = Y - X*vars
                const double z = resid * isn;
                term = -0.5 * (z * z + kLog2Pi) - logsn;                // resid ~ Normal(0, sn)
                w = resid * is2n;
            }
            const bool in = obs < M.n;
            if (in) lik_part = lik_part + term;
            rv[rr_] = in ? w : 0.0;
        }
        // G tile T, k-slice kk': A[i][k] = X[obs 4kk'+q][coord base+16T+4(i&3)+(i>>2)], i = cl; kk outer so that
        // consecutive MFMAs feed independent accumulators.  NM <= 4: all 4 NM operands are read before the weights
        // barrier (they do not depend on it); NM = 8: one k-slice ahead.
        constexpr int kGA = NM <= 4 ? 4 : 1;                      // k-slices of operands read up front
        const double* gcol = LX + g_lane;
        double ga[4][NM];
        if (GRAD && on) {
#pragma unroll
            for (int kk = 0; kk < kGA; ++kk)
#pragma unroll
                for (int T = 0; T < NM; ++T) ga[kk][T] = gcol[4 * kk * S + glm_g_off(T)];
        }
        {
            // publish the owned rows' weights, then every slice wave reads all four for its G product
            double* rb = L.rbuf + p.tile * 256;
#pragma unroll
            for (int rr_ = 0; rr_ < RPW; ++rr_)
                if (r0 + rr_ < 4) rb[(r0 + rr_) * 64 + p.lane] = rv[rr_];
            GLM_STAMPT(3);
            glm_lds_barrier();
            GLM_STAMPT(4);
#pragma unroll
            for (int r = 0; r < 4; ++r) rv[r] = rb[r * 64 + p.lane];
        }
        if (GRAD && on) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                if (kGA == 1 && kk < 3) {
#pragma unroll
                    for (int T = 0; T < NM; ++T) ga[kk + 1][T] = gcol[4 * (kk + 1) * S + glm_g_off(T)];
                }
#pragma unroll
                for (int T = 0; T < NM; ++T)
                    G[T] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[kk][T], rv[kk], G[T], 0, 0, 0);
            }
        }
        if (kOneBuf) {                                        // the one buffer: after its last reader of tile t
            __syncthreads();
            if (more) glm_dma_tile<XS>(M.X + (size_t)(t + 1) * XS, L.X);
        }
        GLM_STAMPT(5);
        glm_dma_wait();                                       // tile t+1 landed (this wave's pieces) ...
        GLM_STAMPT(6);
        __syncthreads();                                      // ... and every wave's; buffers, part, rbuf free
        GLM_STAMPT(7);
    }
#ifdef GLM_STAMP
    if (blockIdx.x < 4 && (threadIdx.x & 63) == 0)
        for (int j = 0; j < 16 * 8; ++j) (&g_glm_stamps[blockIdx.x][threadIdx.x >> 6][0][0])[j] = stamp_lds[(threadIdx.x >> 6) * 128 + j];
#endif
    return glm_finish<NM, NW, GRAD>(a, p, L, XArr<4 * NM>{x}, G, logistic && ubnd >= 0.0 ? -__builtin_inf() : lik_part,
                                    oos, on);
}

// ------------------------------------------------------------------ state access (layout [d][ld])
// Lane pointer at coordinate base + 4q; slot (m, e) adds the wave-uniform offset (16m + e) * ld,
// so the 32 slot addresses cost SGPRs, not VGPRs.
// The pointer passes through an empty volatile asm at every use: the per-slot addresses derived from it are then
// formed where they are used instead of being hoisted out of the step / leapfrog loops, where 4 NM 64-bit addresses per
// state array stayed live across the tile loop and spilled (glm_hmc<8, 4> needed > 1.3 KB of scratch a lane).
template <class T>
__device__ __forceinline__ T* glm_lane_ptr(const GlmPos& p, T* base, int64_t ld, int64_t c) {
    T* r = base + (size_t)(p.base + 4 * p.q) * (size_t)ld + (size_t)c;
    asm volatile("" : "+v"(r));
    return r;
}
__device__ __forceinline__ bool glm_valid(const GlmArgs& a, const GlmPos& p, int slot) {
    return own_coord(p, slot) < a.s.d;
}
// an unconditional load's offset from the lane pointer (row base + 4q of the chain) to slot `slot`'s row, or, for a
// slot past d, to the chain's row 0: the state holds d rows, and the lane's own row base + 4q is past them too when
// d is not a multiple of the slice geometry (d = 300: rows 300..511; the loaded value is zeroed either way)
__device__ __forceinline__ ptrdiff_t glm_slot_off(const GlmArgs& a, const GlmPos& p, int slot, size_t ld) {
    return glm_valid(a, p, slot) ? (ptrdiff_t)(16 * (slot >> 2) + (slot & 3)) * (ptrdiff_t)ld
                                 : -(ptrdiff_t)(p.base + 4 * p.q) * (ptrdiff_t)ld;
}
template <int NM>
__device__ __forceinline__ void glm_load(const GlmArgs& a, const GlmPos& p, const double* src,
                                         double (&v)[(4 * NM)]) {
    const double* lp = glm_lane_ptr(p, src, a.s.ld, p.live ? p.c : 0);
    const size_t ld = (size_t)a.s.ld;
#pragma unroll
    for (int slot = 0; slot < (4 * NM); ++slot)
        v[slot] = glm_valid(a, p, slot) ? lp[(size_t)(16 * (slot >> 2) + (slot & 3)) * ld] : 0.0;
}
// glm_load with unconditional loads (an invalid slot reads the chain's row 0 and is zeroed): no masked load and wait
// per slot, every load in flight together -- for kernels that load the state once and have the registers for it
// (the evaluation kernel); in the step kernels the compiler then keeps the loads live across the step and spills
template <int NM>
__device__ __forceinline__ void glm_load_all(const GlmArgs& a, const GlmPos& p, const double* src,
                                             double (&v)[(4 * NM)]) {
    const double* lp = glm_lane_ptr(p, src, a.s.ld, p.live ? p.c : 0);
    const size_t ld = (size_t)a.s.ld;
#pragma unroll
    for (int slot = 0; slot < (4 * NM); ++slot) {
        const bool ok = glm_valid(a, p, slot);
        const double t = lp[glm_slot_off(a, p, slot, ld)];
        v[slot] = ok ? t : 0.0;
    }
}
template <int NM>
__device__ __forceinline__ void glm_store(const GlmArgs& a, const GlmPos& p, double* dst, int64_t ldd,
                                          const double (&v)[(4 * NM)]) {
    if (!p.live) return;
    double* lp = glm_lane_ptr(p, dst, ldd, p.c);
    const size_t ld = (size_t)ldd;
#pragma unroll
    for (int slot = 0; slot < (4 * NM); ++slot)
        if (glm_valid(a, p, slot)) lp[(size_t)(16 * (slot >> 2) + (slot & 3)) * ld] = v[slot];
}
template <int NM>
__device__ __forceinline__ void glm_store_kept(const GlmArgs& a, const GlmPos& p, int64_t kk, double* base,
                                               const double (&v)[(4 * NM)]) {
    if (base == nullptr) return;
    glm_store<NM>(a, p, base + (size_t)kk * (size_t)a.s.d * (size_t)a.s.C, a.s.C, v);
}
template <int NM>
__device__ __forceinline__ void glm_load4(const GlmArgs& a, const GlmPos& p, const double* src,
                                          f64x4 (&v)[NM]) {
    const double* lp = glm_lane_ptr(p, src, a.s.ld, p.live ? p.c : 0);
    const size_t ld = (size_t)a.s.ld;
#pragma unroll
    for (int slot = 0; slot < (4 * NM); ++slot)
        v[slot >> 2][slot & 3] = glm_valid(a, p, slot) ? lp[(size_t)(16 * (slot >> 2) + (slot & 3)) * ld] : 0.0;
}
template <int NM>
__device__ __forceinline__ void glm_store4(const GlmArgs& a, const GlmPos& p, double* dst, int64_t ldd,
                                           const f64x4 (&v)[NM]) {
    if (!p.live) return;
    double* lp = glm_lane_ptr(p, dst, ldd, p.c);
    const size_t ld = (size_t)ldd;
#pragma unroll
    for (int slot = 0; slot < (4 * NM); ++slot)
        if (glm_valid(a, p, slot)) lp[(size_t)(16 * (slot >> 2) + (slot & 3)) * ld] = v[slot >> 2][slot & 3];
}
template <int NM>
__device__ __forceinline__ void glm_store_kept4(const GlmArgs& a, const GlmPos& p, int64_t kk, double* base,
                                                const f64x4 (&v)[NM]) {
    if (base == nullptr) return;
    glm_store4<NM>(a, p, base + (size_t)kk * (size_t)a.s.d * (size_t)a.s.C, a.s.C, v);
}
// add the tile's evaluation counts to the launch-wide counter (one atomic per wave)
__device__ __forceinline__ void glm_count_evals(const GlmArgs& a, const GlmPos& p, int64_t n) {
    if (a.s.n_evals == nullptr) return;
    unsigned long long v = (p.live && p.q == 0 && p.slice == 0) ? (unsigned long long)n : 0ull;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (p.lane == 0) atomicAdd(a.s.n_evals, v);
}
// the tile's accept bits of a kept step (called by every lane of the wave): its 16 chains are consecutive from
// c0 = 16 (block tpw + tile), i.e. bits c0 & 63 .. +15 of one word, set by one atomic per wave (a per-chain
// atomicOr put up to 64 device-scope atomics on every word)
__device__ __forceinline__ void glm_store_bit(const GlmArgs& a, const GlmPos& p, int64_t kk, bool acc) {
    if (a.s.order != nullptr) {                                  // permuted tile: chains anywhere, a bit each
        if (p.live && acc && p.q == 0 && p.slice == 0 && a.s.acc_bits != nullptr)
            atomicOr((unsigned long long*)&a.s.acc_bits[(size_t)kk * (size_t)a.s.nw + (size_t)(p.c >> 6)],
                     1ull << (p.c & 63));
        return;
    }
    const uint64_t m = __ballot(p.live && acc && p.q == 0 && p.slice == 0) & 0xffffull;   // lane cl < 16: bit cl
    if (p.lane == 0 && m != 0 && a.s.acc_bits != nullptr)                                   // lane 0: c == c0
        atomicOr((unsigned long long*)&a.s.acc_bits[(size_t)kk * (size_t)a.s.nw + (size_t)(p.c >> 6)],
                 (unsigned long long)(m << (p.c & 63)));
}

// normals of the lane's coordinates; padded coordinates (k >= d) get 0 so they stay at 0
template <int NM>
__device__ __forceinline__ void glm_normals(const GlmPos& p, const Stream& rs, uint32_t chain, uint32_t step,
                                            int d, double (&z)[(4 * NM)]) {
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        if (true) {
            const uint32_t blk = (uint32_t)((p.base >> 2) + 4 * m + p.q);   // coords 4*blk .. 4*blk+3
            const u32x4 w = rs.block(chain, step, blk, TAG_NORMAL);
            normals4(w, z[4 * m], z[4 * m + 1], z[4 * m + 2], z[4 * m + 3]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((int)(4 * blk) + e >= d) z[4 * m + e] = 0.0;
        } else {
            z[4 * m] = z[4 * m + 1] = z[4 * m + 2] = z[4 * m + 3] = 0.0;
        }
    }
}

__device__ __forceinline__ bool glm_mh_short_circuit(const Stream& rs, uint32_t chain, uint32_t step, double ratio) {
    bool acc = ratio > 0.0;                                           // RWM.jl:63, MALA.jl:108
    if (!acc) {
        const u32x4 w = rs.block(chain, step, 0u, TAG_ACCEPT);
        acc = gt_det_log(ratio, uniform52(w.x, w.y));
    }
    return acc;
}

__device__ __forceinline__ double glm_tune_factor(int32_t acc, int32_t prop, double target) {
    const double rate = (double)acc / (double)prop;                   // MALA.jl:36-39, HMC.jl:165-169
    return 1.0 / (1.0 + det_exp(-11.0 * (rate - target))) + 0.5;
}

// ------------------------------------------------------------------ host side: launch arguments and grid
inline GlmArgs glm_args(const KernelArgs& k, const GlmShape& g) {
    GlmArgs a;
    a.s = k.s;
    a.sa = k.sa;
    a.m = k.m;
    a.st = k.st;
    a.g = g;
    a.rec = LeapRec{};
    return a;
}

inline unsigned glm_grid(int64_t C, const GlmShape& g) {
    const int64_t chains_per_wg = 16 * g.tpw;
    return (unsigned)((C + chains_per_wg - 1) / chains_per_wg);
}

}  // namespace mcmc
