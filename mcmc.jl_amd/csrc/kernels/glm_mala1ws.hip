// glm_mala1ws.hip -- the wave-specialised single-slice regression MALA kernel (glm_mala1ws<NM>, d <= 128) in a
// translation unit of its own, built WITH machine LICM: the tile loop's fp64 polynomial constants and LDS addresses are
// hoisted out of it (this one-step kernel has the registers for them).  glm.o is built without machine LICM, which
// there keeps hoisted constants from pinning registers across the step loops of the other kernels (Makefile).
#include <type_traits>

#include "glm_device.hpp"

namespace mcmc {

// ------------------------------------------------------------------ batched proposal normals
// normals4 (detmath.hpp) of NB Philox blocks, bitwise -- the same operations on the same values -- with every
// table-row load of the 2 NB radii (bm_radius_u32's main rows) and the 2 NB angles (det_sincos2pi_u32's row) issued
// before the first is used.  normals4 waits for each radius's rows in turn, and the radius tail branch waits for
// every load in flight, so a wave drawing a 128-coordinate proposal from the global tables paid about four memory
// latencies per block; here the rows of all NB blocks are in flight together and only a (rare, 2^-11 per draw) tail
// lane costs a wait of its own.
template <int NB>
__device__ __forceinline__ void normals_batch(const u32x4 (&w)[NB], double (&z)[4 * NB]) {
    typedef double f64x2_t __attribute__((ext_vector_type(2)));
    constexpr int NR = 2 * NB;
    constexpr uint32_t kOff0 = 0u - ((uint32_t)((1023 + 21) << 5) << 4);
    constexpr uint32_t kOff1 = kOff0 + (uint32_t)(BM_RADP_NROWS / 2) * 16u;
    uint32_t wr[NR], wa[NR];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        wr[2 * b] = w[b].x; wa[2 * b] = w[b].y;
        wr[2 * b + 1] = w[b].z; wa[2 * b + 1] = w[b].w;
    }
    uint32_t vv[NR], smv[NR];
    bool tl[NR];
    double t[NR];
    f64x2_t c[NR][4];
#pragma unroll
    for (int k = 0; k < NR; ++k) {                                      // bm_radius_u32: the main-table rows
        const uint32_t sm = (uint32_t)((int32_t)wr[k] >> 31);
        const uint32_t v = wr[k] ^ sm;
        const double y = (double)v;
        const uint64_t b = d2bits(y);
        const uint32_t yh = (uint32_t)(b >> 32);
        tl[k] = v < (1u << 21);
        const uint32_t sel = (sm & kOff1) | (~sm & kOff0);
        uint32_t off = ((yh >> 15) << 4) + sel;
        const uint32_t th = (yh & 0x7fffu) | 0x3ff00000u;
        off = tl[k] ? 0u : off;
        t[k] = bits2d(((uint64_t)th << 32) | (b & 0xffffffffull)) - (1.0 + 1.0 / 64.0);
        const char* base = reinterpret_cast<const char*>(kBmRadPTab) + off;
        c[k][0] = *reinterpret_cast<const f64x2_t*>(base);
        c[k][1] = *reinterpret_cast<const f64x2_t*>(base + 16 * BM_RADP_NROWS);
        c[k][2] = *reinterpret_cast<const f64x2_t*>(base + 32 * BM_RADP_NROWS);
        c[k][3] = *reinterpret_cast<const f64x2_t*>(base + 48 * BM_RADP_NROWS);
        vv[k] = v;
        smv[k] = sm;
    }
    int32_t ji[NR];
    f64x2_t ar[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) {                                      // det_sincos2pi_u32: the (sin a, cos a) row
        ji[k] = ((int32_t)(wa[k] << 10)) >> 10;
        const uint32_t off = (wa[k] - (uint32_t)ji[k]) >> 18;
        ar[k] = *reinterpret_cast<const f64x2_t*>(reinterpret_cast<const char*>(kBmSinCos1024Tab) + off);
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {                                      // bm_radius_u32's tail, on the lanes in it
        if (tl[k]) {
            uint32_t v2 = vv[k];
            asm volatile("" : "+v"(v2));
            const double x = (double)v2 + 0.5;
            const uint64_t bx = d2bits(x);
            const uint32_t xh = (uint32_t)(bx >> 32);
            const uint32_t rw = (uint32_t)((int)(xh >> 15) - ((1023 - 1) << 5)) * 16u +
                                (smv[k] & (16u * (BM_RADT_NROWS / 2)));
            t[k] = bits2d(((uint64_t)((xh & 0x7fffu) | 0x3ff00000u) << 32) | (bx & 0xffffffffull)) - (1.0 + 1.0 / 64.0);
            asm volatile(
                "global_load_dwordx4 %0, %4, %5\n\t"
                "global_load_dwordx4 %1, %4, %6\n\t"
                "global_load_dwordx4 %2, %4, %7\n\t"
                "global_load_dwordx4 %3, %4, %8\n\t"
                "s_waitcnt vmcnt(0)"
                : "=&v"(c[k][0]), "=&v"(c[k][1]), "=&v"(c[k][2]), "=&v"(c[k][3])
                : "v"(rw), "s"(&kBmRadTTab[0][0]), "s"(&kBmRadTTab[BM_RADT_NROWS][0]),
                  "s"(&kBmRadTTab[2 * BM_RADT_NROWS][0]), "s"(&kBmRadTTab[3 * BM_RADT_NROWS][0])
                : "memory");
        }
    }
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        double q = __builtin_fma(c[k][3].y, t[k], c[k][3].x);           // the radius polynomial
        q = __builtin_fma(q, t[k], c[k][2].y);
        q = __builtin_fma(q, t[k], c[k][2].x);
        q = __builtin_fma(q, t[k], c[k][1].y);
        q = __builtin_fma(q, t[k], c[k][1].x);
        q = __builtin_fma(q, t[k], c[k][0].y);
        const double rad = __builtin_fma(q, t[k], c[k][0].x);
        const double j = (double)ji[k];                                 // the angle
        const double j2 = j * j;
        const double sr = j * __builtin_fma(j2, __builtin_fma(j2, kSinJ5, kSinJ3), kSinJ1);
        const double cr = __builtin_fma(j2, __builtin_fma(j2, kCosJ4, kCosJ2), 1.0);
        const double sn = __builtin_fma(ar[k].x, cr, ar[k].y * sr);
        const double cs = __builtin_fma(ar[k].y, cr, -(ar[k].x * sr));
        z[2 * k] = rad * cs;
        z[2 * k + 1] = rad * sn;
    }
}

// ------------------------------------------------------------------ wave-specialised single-slice MALA
// glm_mala1ws<NM>: glm_mala's step on one slice (d <= 128; config 3: logistic MALA, d = 128) with the work of a
// 16-chain tile split over two waves that share a SIMD (a 512-thread workgroup puts waves w and w + 4 on one SIMD):
//   wave w < 4   ("M", matrix): holds the tile's proposal (the B operands) and the gradient accumulators in registers
//                and issues every MFMA: eta_{t+1} = X_{t+1} beta and G += X_{t-1}^T r_{t-1};
//   wave w + 4   ("V", vector): the proposal (Philox, Box-Muller, MALA.jl:98-103), the X tile loads and, per
//                observation tile, the elementwise log-likelihood terms and residual weights r_t on eta_t.
// eta_t and r_t cross through LDS (double-buffered), one barrier per tile.  The fp64 matrix and vector pipes of a
// SIMD run concurrently for different waves (scripts/peak_f64.hip: MFMA-only and FMA-only waves paired on a SIMD
// take max, not sum, of their times), whereas the one-wave kernel this replaced (a wave per tile did both, 300 VGPRs)
// serialised its VALU work with its MFMAs.  One launch is one step (mcmc_glm_steps_per_launch): the per-chain scalars
// (lp, tuner state) round-trip through HBM per launch.  Every sum is formed by the same instructions in the same
// order as glm_eval1_tiles' chains (eta over (m, e, q); G over observations; a lane's likelihood terms in (t, r)
// order) with glm_finish's end and glm_mala's qf / qb, so the results are theirs bit for bit: orc_glm_eval restates
// the evaluation, and the parity tests pin the step against the oracle.
// LDS (doubles; XS = glm_tile_doubles(16 NM), X rows then Y): X slots 0, 1 | region R: X slots 2, 3, eta [2][4][64][4], r [2][4][64][4],
// which overlays the proposal [4 waves][4 NM][64] of the proposal phase | Y [4][16] | the logistic term's table
// (kSoftplusTab) | qf, lik [2][4][16] | M's partial qf [4][64].
template <int NM>
__host__ __device__ constexpr int glm_ws_region(int XS) {
    return (2 * XS + 4096) > (4 * 4 * NM * 64) ? (2 * XS + 4096) : (4 * 4 * NM * 64);
}
__host__ __device__ inline size_t glm_ws_lds_doubles(int nm) {
    const int XS = glm_tile_doubles(16 * nm);
    const int R = (2 * XS + 4096) > (4 * 4 * nm * 64) ? (2 * XS + 4096) : (4 * 4 * nm * 64);
    return (size_t)(2 * XS + R + 4 * 16 + SP_NROWS * 10 + 2 * 4 * 16 + 4 * 64)
#ifdef GLM_WS_STAMP
           + 512                                               // the phase stamps (dev build, scripts/ws_stamps.py)
#endif
        ;
}
template <int NM, bool UNITP = false>
__global__ __launch_bounds__(512) void glm_mala1ws(GlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int NS = 4 * NM;
    constexpr int KM = 4 * NM;
    const StepArgs& s = a.s;
    const SamplerArgs& sa = a.sa;
    const ModelArgs& M = a.m;
    const GlmShape& g = a.g;
    const int wv = (int)(threadIdx.x >> 6);
    const bool vwave = __builtin_amdgcn_readfirstlane(wv) >= 4;
    GlmPos p;
    p.lane = threadIdx.x & 63;
    p.q = p.lane >> 4;
    p.cl = p.lane & 15;
    p.tile = wv & 3;
    p.wave = p.tile;
    p.slice = 0;
    p.base = 0;
    p.c = ((int64_t)blockIdx.x * 4 + p.tile) * 16 + p.cl;
    p.live = p.c < s.C;
    constexpr int S = glm_row_stride(16 * NM);
    constexpr int XS = glm_tile_doubles(16 * NM);             // one staged tile: X rows, then Y
    constexpr int YO = glm_y_offset(16 * NM);
    constexpr int BO = glm_b_offset(16 * NM);
    double* const Xs = smem;                                   // 4 X tile slots: 0, 1 here, 2, 3 in region R
    double* const R = smem + 2 * XS;
    double* const Eb = R + 2 * XS;                             // eta [2][4 tiles][64 lanes][4]
    double* const Rb = Eb + 2048;                              // r   [2][4 tiles][64 lanes][4]
    double* const beta = R;                                    // proposal [4 tiles][NS][64] (proposal phase only)
    double* const Yb = R + glm_ws_region<NM>(XS);              // (unused: Y travels inside each staged tile)
    double* const ltabp = Yb + 64;                             // logistic term's table [SP_NROWS][10]
    double* const qfl = ltabp + SP_NROWS * 10;                 // qf [4][16], then lik [4][16]
    double* const likl = qfl + 64;
    double* const qpart = likl + 64;                           // M's partial qf per lane [4 tiles][64] (proposal phase)
#ifdef GLM_WS_STAMP
    unsigned* const wst = reinterpret_cast<unsigned*>(qpart + 256);
#endif
    auto xslot = [&](int64_t tt) -> double* { const int b = (int)(tt & 3); return b < 2 ? Xs + b * XS : R + (b - 2) * XS; };
    const Stream rs{s.key0, s.key1};
    const uint32_t chain = s.chain0 + (uint32_t)p.c;
    const int64_t cc = p.live ? p.c : 0;
    const size_t ld = (size_t)s.ld;
    const double* const xl = glm_lane_ptr(p, a.st.x, s.ld, cc);
    const double* const gl = glm_lane_ptr(p, a.st.g, s.ld, cc);
    const int64_t i = s.step_begin;                            // ONE step per launch
    const double h = sa.tuner ? a.st.t_step[cc] : sa.drift_step;
    const double half = h / 2.0;
    const double twoh = 2.0 * h;
    const double Lc = det_log(kTwoPi * h) / 2.0;
    const int64_t ntiles = g.n_pad / 16;
    const bool logi = M.kind == MK_LOGISTIC;
    // X / Y tiles 0 and 1, staged through registers by the 256 threads of the M waves in the proposal phase (u = thread
    // index within the role); the V waves stage every later tile by LDS-DMA inside the tile loop
    constexpr int kHalf = XS / 2;                              // f64x2 per staged tile
    constexpr int kPer = (kHalf + 255) / 256;
    const int u = (int)(threadIdx.x & 255);
    f64x2 xbuf[kPer];
    (void)Yb;
    auto load_tile = [&](int64_t tt) {                         // the tile image moves linearly (glm_layout.hpp)
        const f64x2* src = reinterpret_cast<const f64x2*>(M.X + (size_t)tt * XS);
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int e = u + 256 * j;
            xbuf[j] = src[e < kHalf ? e : 0];
        }
    };
    auto store_tile = [&](int64_t tt) {
        f64x2* dst = reinterpret_cast<f64x2*>(xslot(tt));
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int e = u + 256 * j;
            if (e < kHalf) dst[e] = xbuf[j];
        }
    };
    double* const xb = beta + (size_t)(p.tile * NS) * 64 + p.lane;   // this lane's proposal slots

    // ---- proposal phase: the proposal (MALA.jl:98-103) into LDS, its Philox blocks split between the tile's two
    //      waves (M: m < NM/2, V: the rest; the proposal is latency-bound -- table reads, state loads -- and the M
    //      waves had only the X tiles 0 and 1 to stage); qf's sum runs in slot order: M's partial over its slots
    //      crosses to V through LDS and V continues it over its own, so the sum is glm_mala's
    WS_WG(0);
    constexpr int m_split = NM / 2;
    double tv[NS];                                             // V: its slots' qf terms, summed after M's partial
    {
        double qf = 0.0;
        const double sq = __builtin_sqrt(h);
        // the wave's blocks [M0, M1): the blocks' normals with their table rows in flight together, then the state
        // (every load unconditional: an invalid slot reads the chain's row 0 and is zeroed)
        auto part = [&](auto m0c, auto m1c) {
            constexpr int M0 = decltype(m0c)::value, M1 = decltype(m1c)::value, NBK = M1 - M0;
            if constexpr (NBK > 0) {
                u32x4 w[NBK];
#pragma unroll
                for (int b = 0; b < NBK; ++b)                                  // coords 4*blk .. 4*blk+3
                    w[b] = rs.block(chain, (uint32_t)i, (uint32_t)(4 * (M0 + b) + p.q), TAG_NORMAL);
                double z[4 * NBK];
                normals_batch<NBK>(w, z);
#pragma unroll
                for (int k = 0; k < 4 * NBK; ++k) {
                    const int slot = 4 * M0 + k;
                    const bool v = glm_valid(a, p, slot);
                    const ptrdiff_t o = glm_slot_off(a, p, slot, ld);
                    // global loads (as flat loads, each LDS store of the proposal below would wait for them all)
                    typedef const __attribute__((address_space(1))) double gdouble;
                    const double xl0 = *(gdouble*)(xl + o), gl0 = *(gdouble*)(gl + o);
                    const double xv = v ? xl0 : 0.0;
                    const double gv = v ? gl0 : 0.0;
                    const double pm = xv + half * gv;                           // MALA.jl:98
                    const double xpv = pm + sq * (v ? z[k] : 0.0);              // MALA.jl:100
                    const double ee = pm - xpv;
                    const double term = (-(ee * ee)) / twoh - Lc;               // MALA.jl:103
                    if (vwave) tv[slot] = term;
                    else if (v) qf = qf + term;
                    xb[64 * slot] = xpv;
                }
            }
        };
        if (vwave) part(std::integral_constant<int, NM / 2>{}, std::integral_constant<int, NM>{});
        else part(std::integral_constant<int, 0>{}, std::integral_constant<int, NM / 2>{});
        WS_WG2(0);
        if (!vwave) qpart[p.tile * 64 + p.lane] = qf;
    }
    if (vwave) {
        if (logi) {
            for (int e = u; e < SP_NROWS * 10; e += 256) ltabp[e] = (&kSoftplusTab[0][0])[e];
        }
        WS_WG2(1);
    } else {
        load_tile(0);
        store_tile(0);
        if (ntiles > 1) {
            load_tile(1);
            store_tile(1);
        }
        WS_WG2(1);
    }
    __syncthreads();
    WS_WG(1);
    // ---- M: the proposal into registers, eta_0;  V: qf
    double bx[NS];
    f64x4 G[NM];
    if (!vwave) {
#pragma unroll
        for (int slot = 0; slot < NS; ++slot) bx[slot] = xb[64 * slot];
#pragma unroll
        for (int T = 0; T < NM; ++T) G[T] = f64x4{0.0, 0.0, 0.0, 0.0};
    } else {
        double qf = qpart[p.tile * 64 + p.lane];
#pragma unroll
        for (int slot = 4 * m_split; slot < NS; ++slot)
            if (glm_valid(a, p, slot)) qf = qf + tv[slot];
        qf = glm_sum(a, p, GlmLds{}, qf);
        if (p.q == 0) qfl[p.tile * 16 + p.cl] = qf;
        WS_WG2(2);
    }
    __syncthreads();                                           // the proposal area is free from here on
    WS_WG(2);
    f64x4* const Eq = reinterpret_cast<f64x4*>(Eb) + p.tile * 64 + p.lane;   // + 256 * buffer
    f64x4* const Rq = reinterpret_cast<f64x4*>(Rb) + p.tile * 64 + p.lane;
    auto eta_of = [&](int64_t tt) {                            // glm_eval1_tiles' eta chain, operands read ahead
        const double* xrow = xslot(tt) + p.cl * S + 4 * p.q;
        constexpr int kLA = 4;                                 // 8 and 12 measured the same (round 5)
        double av[KM];
#pragma unroll
        for (int m = 0; m < (kLA < KM ? kLA : KM); ++m) av[m] = xrow[glm_eta_off(m)];
        f64x4 e = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int m = 0; m < KM; ++m) {
            if (m + kLA < KM) av[m + kLA] = xrow[glm_eta_off(m + kLA)];
            e = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], bx[m], e, 0, 0, 0);
        }
        return e;
    };
    auto g_of = [&](int64_t tt) {                              // G += X_tt^T r_tt (glm_eval1_tiles' G product)
        const f64x4 rv = Rq[256 * (tt & 1)];
        const double* gcol = xslot(tt) + p.q * S + 4 * (p.cl & 3) + (p.cl >> 2);
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
            if (kk < 3) {
#pragma unroll
                for (int T = 0; T < NM; ++T) ga[T] = gn[T];
            }
        }
    };
    if (!vwave) Eq[0] = eta_of(0);
    __syncthreads();
    WS_WG(3);
    // ---- the observation tiles
    const double sn = M.noise_sigma, s2n = sn * sn;
    const double logsn = logi ? 0.0 : det_log(sn);
    const double isn = 1.0 / sn, is2n = 1.0 / s2n;
    const double (*sptab)[10] = reinterpret_cast<const double (*)[10]>(ltabp);
    const int64_t nfull = M.n / 16;
    // one loop per role, each with one barrier per tile (the same count): the roles' loop invariants (the V waves'
    // polynomial constants, the M waves' operand addresses) stay out of each other's register pressure
    double lik_part = 0.0;
    double ubnd = -__builtin_inf();                            // logistic: max of u + b over the lane's observations
    if (!vwave) {
        for (int64_t t = 0; t < ntiles; ++t) {
            WS_STAMP(0);
            if (t + 1 < ntiles) Eq[256 * ((t + 1) & 1)] = eta_of(t + 1);
            WS_STAMP(1);
            if (t >= 1) g_of(t - 1);
            WS_STAMP(2);
            __syncthreads();
            WS_STAMP(3);
        }
    } else {
        for (int64_t t = 0; t < ntiles; ++t) {
            WS_STAMP(0);
            // tile t+2 by LDS-DMA (no registers, no ds_write: +1.2 % on config 3 against staging it through registers,
            // profiles/r06_ab_glm.md); slot (t+2) % 4 held tile t-2: read before the last barrier
            if (t + 2 < ntiles)
                glm_dma_tile_w<XS, 4>(M.X + (size_t)(t + 2) * XS, xslot(t + 2), __builtin_amdgcn_readfirstlane(wv - 4));
            WS_STAMP(1);
            const f64x4 eta = Eq[256 * (t & 1)];
            const double* LY = xslot(t) + YO;
            double y[4], term[4], rv[4];                       // y: the response, for the logistic model w (det_logi)
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = LY[p.q + 4 * r];
            if (logi) {
                // prob = 1/(1+exp(-X*vars)); Y ~ Bernoulli(prob); its eta-derivative (MCMCDerivRules.jl:111)
                const double* LB = xslot(t) + BO;
                // two rows at a time: four rows' coefficient rows in flight at once spill the wave's registers
#pragma unroll
                for (int h = 0; h < 4; h += 2) {
                    LogiState E[2];
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        det_logi_s1(eta[h + r], y[h + r], E[r], sptab);
                        ubnd = __builtin_fmax(ubnd, E[r].u + LB[p.q + 4 * (h + r)]);   // the reference's -Inf
                    }
#pragma unroll
                    for (int r = 0; r < 2; ++r) det_logi_s2(E[r]);
#pragma unroll
                    for (int r = 0; r < 2; ++r) det_logi_fin(E[r], y[h + r], term[h + r], rv[h + r]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else if (M.kind == MK_PROBIT) {
#pragma unroll
                for (int r = 0; r < 4; ++r) glm_probit_obs(eta[r], y[r], term[r], rv[r]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double resid = y[r] - eta[r];                            // resid = Y - X*vars
                    const double zz = resid * isn;
                    term[r] = -0.5 * (zz * zz + kLog2Pi) - logsn;                  // resid ~ Normal(0, sn)
                    rv[r] = resid * is2n;
                }
            }
            if (t < nfull) {                                                       // uniform: no padded observation
#pragma unroll
                for (int r = 0; r < 4; ++r) lik_part = lik_part + term[r];         // the lane's terms in (t, r) order
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool in = t * 16 + p.q + 4 * r < M.n;
                    lik_part = in ? lik_part + term[r] : lik_part;
                    rv[r] = in ? rv[r] : 0.0;
                }
            }
            WS_STAMP(2);
            Rq[256 * (t & 1)] = f64x4{rv[0], rv[1], rv[2], rv[3]};
            WS_STAMP(3);
            glm_dma_wait();                                    // tile t+2 landed (the asm loads are not counted)
            __syncthreads();
            WS_STAMP(4);
        }
    }
    WS_WG(4);
#ifdef GLM_WS_STAMP
    if (blockIdx.x < 4)
        for (int j = p.lane; j < 128; j += 64) (&g_ws_stamps[blockIdx.x][wv][0][0])[j] = wst[wv * 128 + j];
#endif
    if (vwave) {
        const double lik = glm_sum(a, p, GlmLds{}, logi && ubnd >= 0.0 ? -__builtin_inf() : lik_part);
        if (p.q == 0) likl[p.tile * 16 + p.cl] = lik;
    } else {
        g_of(ntiles - 1);
    }
    __syncthreads();
    WS_WG(5);
    if (vwave) return;
    // ---- M waves: the end of the evaluation (glm_finish), MALA.jl:104-125
    // the current position (qb, and the kept rows of a rejected step), every load unconditional and issued first
    typedef const __attribute__((address_space(1))) double gdouble;   // global, not flat, loads (see the proposal)
    double xo[NS];
#pragma unroll
    for (int slot = 0; slot < NS; ++slot)
        xo[slot] = *(gdouble*)(xl + glm_slot_off(a, p, slot, ld));
    double lp = a.st.lp[cc];
    int32_t n_acc = sa.tuner ? a.st.t_acc[cc] : 0;
    int32_t n_prop = sa.tuner ? a.st.t_prop[cc] : 0;
    if (sa.tuner) n_prop += 1;
    const double qf = qfl[p.tile * 16 + p.cl];
    bool oos;
    double lpp;
    {
        const int d = M.d;
        const double lik = likl[p.tile * 16 + p.cl];
        const double sp = M.prior_sigma, s2p = sp * sp, logsp = det_log(sp);
        // the prior's divisions by sigma and sigma^2 (vars ~ Normal(0, sigma)) are exact no-ops at sigma = 1 (the
        // examples' prior, x / 1 == x for every double): the UNITP instance (launched when prior_sigma == 1) skips
        // them, bitwise the same (64 IEEE divisions a lane, a third of this phase)
        constexpr bool unit = UNITP;
        double pp = 0.0;
        if (unit) {
#pragma unroll
            for (int slot = 0; slot < NS; ++slot) {
                const int k = own_coord(p, slot);
                if (k < d) {
                    const double z = bx[slot] - 0.0;
                    pp = pp + (-0.5 * (z * z + kLog2Pi) - logsp);
                }
            }
        } else {
#pragma unroll
            for (int slot = 0; slot < NS; ++slot) {
                const int k = own_coord(p, slot);
                if (k < d) {
                    const double z = (bx[slot] - 0.0) / sp;
                    pp = pp + (-0.5 * (z * z + kLog2Pi) - logsp);
                }
            }
        }
        const double prior = glm_sum(a, p, GlmLds{}, pp);
        double acc = 0.0 + prior;                                           // LLAcc(0.) + ...
        bool bad = !(acc - acc == 0.0);
        acc = acc + lik;
        bad = bad || !(acc - acc == 0.0);
        oos = bad;
        if (bad) acc = -__builtin_inf();
        if (unit) {
#pragma unroll
            for (int slot = 0; slot < NS; ++slot)
                G[slot >> 2][slot & 3] = bad ? 0.0 : (0.0 - bx[slot]) + G[slot >> 2][slot & 3];
        } else {
#pragma unroll
            for (int slot = 0; slot < NS; ++slot)
                G[slot >> 2][slot & 3] = bad ? 0.0 : (0.0 - bx[slot]) / s2p + G[slot >> 2][slot & 3];
        }
        lpp = acc;                                                          // MALA.jl:101
    }
    WS_WG2(3);
    (void)oos;
    double qb = 0.0;
#pragma unroll
    for (int slot = 0; slot < NS; ++slot) {
        const bool v = glm_valid(a, p, slot);
        const double xv = v ? xo[slot] : 0.0;
        const double e = (bx[slot] + half * G[slot >> 2][slot & 3]) - xv;           // MALA.jl:104-105
        if (v) qb = qb + ((-(e * e)) / twoh - Lc);
    }
    qb = glm_sum(a, p, GlmLds{}, qb);
    WS_WG2(4);
    const double ratio = ((lpp + qb) - lp) - qf;                   // MALA.jl:107
    const bool acc = glm_mh_short_circuit(rs, chain, (uint32_t)i, ratio);
    WS_WG2(5);
    int64_t kk;
    const bool kept = kept_index(i - s.run_step0, s.burnin, s.thinning, s.len, &kk);
    double* const ks = kept && s.samples ? s.samples + (size_t)kk * (size_t)s.d * (size_t)s.C : nullptr;
    double* const kg = kept && s.grads ? s.grads + (size_t)kk * (size_t)s.d * (size_t)s.C : nullptr;
    if (p.live) {
        // an accepted proposal is the new state; a rejected one leaves the state in HBM as it is.  Kept steps (one in
        // `thinning`, wave-uniform) write the rows, a rejected lane's gradient reloaded in groups of 8 slots with
        // every load unconditional (a masked load per slot waited for each in turn)
        double* const xw = a.st.x + (size_t)(4 * p.q) * ld + (size_t)p.c;
        double* const gw = a.st.g + (size_t)(4 * p.q) * ld + (size_t)p.c;
        const size_t Cs = (size_t)s.C;
        if (acc) {
#pragma unroll
            for (int slot = 0; slot < NS; ++slot) {
                if (!glm_valid(a, p, slot)) continue;
                const size_t r = (size_t)(16 * (slot >> 2) + (slot & 3));
                xw[r * ld] = bx[slot];
                gw[r * ld] = G[slot >> 2][slot & 3];
            }
        }
        if (ks || kg) {
#pragma unroll
            for (int slot = 0; slot < NS; ++slot) {
                if (!glm_valid(a, p, slot)) continue;
                const size_t r = (size_t)(16 * (slot >> 2) + (slot & 3));
                const size_t ko = (size_t)(4 * p.q + r) * Cs + (size_t)p.c;
                if (ks) ks[ko] = acc ? bx[slot] : xo[slot];
                if (kg) kg[ko] = acc ? G[slot >> 2][slot & 3] : *(gdouble*)(gl + r * ld);
            }
        }
    }
    WS_WG2(6);
    double hn = h;
    if (acc) {
        lp = lpp;
        if (sa.tuner) n_acc += 1;
    }
    if (kept) glm_store_bit(a, p, kk, acc);
    if (sa.tuner && i <= s.tuner_burnin && (i % sa.adapt_step) == 0) {   // MALA.jl:116-118
        hn = h * glm_tune_factor(n_acc, n_prop, sa.target_rate);
        n_acc = 0;
        n_prop = 0;
    }
    if (p.live && p.q == 0) {
        a.st.lp[p.c] = lp;
        if (sa.tuner) {
            a.st.t_step[p.c] = hn;
            a.st.t_acc[p.c] = n_acc;
            a.st.t_prop[p.c] = n_prop;
        }
    }
    glm_count_evals(a, p, s.nsteps);
    WS_WG(6);
}

}  // namespace mcmc

hipError_t mcmc_launch_glm_mala1ws(const mcmc::GlmArgs& a, dim3 grid, hipStream_t st) {
    using namespace mcmc;
    const size_t lw = glm_ws_lds_doubles(a.g.nm) * sizeof(double);
    const bool unit = a.m.prior_sigma == 1.0;                 // the prior's divisions are exact no-ops (glm_mala1ws)
    switch (a.g.nm) {
        case 1: glm_mala1ws<1><<<grid, 512, lw, st>>>(a); break;
        case 2: glm_mala1ws<2><<<grid, 512, lw, st>>>(a); break;
        case 4: glm_mala1ws<4><<<grid, 512, lw, st>>>(a); break;
        case 8:
            if (unit) glm_mala1ws<8, true><<<grid, 512, lw, st>>>(a);
            else glm_mala1ws<8><<<grid, 512, lw, st>>>(a);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

