// rowtile_critic.cuh — the critic row tile (CriticSmem, critic_rowtile_body, its kernel entry points and
// launch_critic_t), shared by rowtile.hip, which instantiates the tiles without layer norm, and rowtile_ln.hip,
// which instantiates the LN axis. Two translation units on purpose: with the layer-normed instantiations in
// rowtile.hip's module the compiler allocated the registers of the OTHER row tiles differently (the actor's
// included), and this commit leaves those kernels as they were.
#pragma once
#include "dppo_ppo.h"
#include "rowtile_common.cuh"

// =============================================================================================
// critic
// =============================================================================================
// LN_SITES > 0 (a layer-normed critic image: 2 norms in the residual head, 3 in the plain one): + the norms'
// gamma / beta [2 LN_SITES][HC], the rows' mean and rstd per site [LN_SITES][2][ROWS] and four [LN_WAVES][ROWS] slots
// of cross-wave partials
constexpr int LN_WAVES = 8;
template <class P, int MT, int LN_SITES = 0>
struct CriticSmem {
    static constexpr int ROWS = 16 * MT;
    size_t tA, tB, a0, rn, rv, bias, total;
    size_t lnp, lnstat, lnred;
    __host__ __device__ CriticSmem(const CriticArgs& a) {
        using AT = typename P::AT;
        const int pad = lds_pad_elems<P>();
        const int ldh = a.HC + pad;
        const int ka = (a.L.ks_in > a.L.ks_out_t ? a.L.ks_in : a.L.ks_out_t) * P::KG + pad;
        size_t o = 0;
        tA = o; o += dppo_align16(sizeof(AT) * ROWS * ldh);
        tB = o; o += dppo_align16(sizeof(AT) * ROWS * ldh);
        a0 = o; o += dppo_align16(sizeof(AT) * ROWS * ka);
        rn = o; o += dppo_align16(4 * ROWS);
        rv = o; o += dppo_align16(4 * ROWS);
        bias = o; o += dppo_align16(4 * (3 * a.HC + 16));
        lnp = lnstat = lnred = o;
        if constexpr (LN_SITES > 0) {
            lnp = o; o += dppo_align16(4 * 2 * LN_SITES * a.HC);
            lnstat = o; o += dppo_align16(4 * LN_SITES * 2 * ROWS);
            lnred = o; o += dppo_align16(4 * 4 * LN_WAVES * ROWS);
        }
        total = o;
    }
};

// HEAD (DPPO_HEAD_*, the image's attribute): RESIDUAL is h3 = l2(u2) + h1, V = out(h3); PLAIN is the reference's
// MLP([SD, HC, HC, HC, 1]): h3 = l2(u2), u3 = mish(h3), V = out(u3). The PLAIN branches are `if constexpr`
// only, so the RESIDUAL instantiations are the code they were. A PLAIN TRAIN tile carries H3 to its backward
// beside H1 and H2 (4 MT NT more registers), writes u3 where the residual tile writes h3 (ch3T, the out-Dense
// gradient's operand) and a dh3 image (cdh3T): l2's weight gradient is a true product there
// LN (DPPO_LN_*, the image's second attribute): Keras' LayerNormalization between each hidden Dense and its Mish,
// y_k = LN_k(h_k), u_k = mish(y_k): three sites in the PLAIN head (eps 1e-3), the block's two pre-activation norms
// in the RESIDUAL head (eps 1e-6; the skip carries the raw h1). `if constexpr` only, so the instantiations without
// it are the code they were. H1 / H2 / H3 keep the RAW pre-activations as before and the rows' mean and rstd stay
// in LDS (768 B), so the backward recomputes x_hat and y with the forward's operations and the tile carries no
// more registers across the layers than without the norm. The backward of a site (ln_backward) leaves dh_k in
// the accumulators, which go to the images the dW reads as before, and adds the tile's dgamma_k / dbeta_k to the
// gradient tail a.gln
template <class P, int MT, int NT, bool TRAIN, int WAVES, int HEAD, bool LN = false>
__device__ __forceinline__ void critic_rowtile_body(const CriticArgs& a) {
    using AT = typename P::AT;
    constexpr int THREADS = 64 * WAVES;
    constexpr int ROWS = 16 * MT;
    static_assert(ROWS <= 64, "the epilogue maps one row per lane of wave 0");
    constexpr int KSH = ksh_for<P>(NT, WAVES);
    constexpr int NOK = nok_for<P>(NT);
    constexpr int KSI = 2, KSO = 2;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const MlpLayout& L = a.L;
    const CriticSmem<P, MT, LN ? (HEAD == DPPO_HEAD_PLAIN ? 3 : 2) : 0> S(a);
    static_assert(!LN || WAVES <= LN_WAVES, "CriticSmem sizes the cross-wave partials for LN_WAVES waves");
    const int pad = lds_pad_elems<P>();
    const int ldh = a.HC + pad;
    const int lda0 = (L.ks_in > L.ks_out_t ? L.ks_in : L.ks_out_t) * P::KG + pad;
    const int k1w = L.ks_in * P::KG, ktw = L.ks_out_t * P::KG;
    const int SD = a.SD;
    constexpr bool train = TRAIN;
    const int HC = a.HC;
    AT* tA = (AT*)(smem + S.tA);
    AT* tB = (AT*)(smem + S.tB);
    AT* a0 = (AT*)(smem + S.a0);
    int* rn = (int*)(smem + S.rn);
    float* bias = (float*)(smem + S.bias);
    float* part = (float*)(smem + S.tB);
    const size_t grow0 = (size_t)blockIdx.x * ROWS;
    int64_t nrows = a.nrows;
    if (train && a.crow_n) {
        // sample-weighted rows: the count is known on the device only; tiles past the 64-row
        // padded count exit (the dW launch reads images only that far, DWArgs::rows_dev)
        nrows = __builtin_amdgcn_readfirstlane(*a.crow_cnt);
        if ((int64_t)grow0 >= (nrows + 63) / 64 * 64) return;
    }
    for (int i = tid; i < 3 * HC + 16; i += THREADS) {
        const int seg = i < HC ? SEG_B_IN : (i < 2 * HC ? SEG_B_L1 : (i < 3 * HC ? SEG_B_L2 : SEG_B_OUT));
        const int j = i < 3 * HC ? i % HC : i - 3 * HC;
        bias[i] = ((const float*)(a.packed + L.off[seg]))[j];
    }
    constexpr bool plain = HEAD == DPPO_HEAD_PLAIN;
    constexpr int LN_SITES = LN ? (plain ? 3 : 2) : 0;
    [[maybe_unused]] float* lnp = (float*)(smem + S.lnp);       // gamma_k = lnp + 2 k HC, beta_k = lnp + (2 k + 1) HC
    [[maybe_unused]] float* lnstat = (float*)(smem + S.lnstat);
    [[maybe_unused]] float* lnred = (float*)(smem + S.lnred);
    [[maybe_unused]] const float ln_eps = critic_ln_eps(plain);
    if constexpr (LN) {   // the image's tail (dppo_layout.h critic_ln_*), visible after the barriers below
        const float* tail = (const float*)(a.packed + L.total);
        for (int i = tid; i < 2 * LN_SITES * HC; i += THREADS) lnp[i] = tail[i];
    }
    // site k's forward: acc = LN_k(h) (ln_fwd), and backward: acc = du_k -> dh_k (ln_bwd)
    [[maybe_unused]] auto ln_fwd = [&](int k, const f32x4 (&h)[MT][NT], f32x4 (&y)[MT][NT]) {
        ln_forward<MT, NT, WAVES>(h, y, lnp + 2 * k * HC, lnp + (2 * k + 1) * HC, lnstat + k * 2 * ROWS, lnred, ln_eps, HC,
                                  wave * NT, wave, lane);
    };
    [[maybe_unused]] auto ln_bwd = [&](int k, f32x4 (&d)[MT][NT], const f32x4 (&h)[MT][NT]) {
        ln_backward<MT, NT, WAVES>(d, h, lnp + 2 * k * HC, lnp + (2 * k + 1) * HC, lnstat + k * 2 * ROWS,
                                   lnred + 2 * WAVES * ROWS, a.gln + 2 * k * HC, a.gln + (2 * k + 1) * HC, a.ln_unscale, HC,
                                   wave * NT, wave, lane);
    };
    const __amdgpu_buffer_rsrc_t wsr = packed_rsrc(a.ws.base);
    const uint32_t ldm32 = (uint32_t)a.ws.ldm, grow32 = (uint32_t)grow0;

    if (tid < ROWS) {
        const int64_t gr = (int64_t)grow0 + tid;
        int n = -1;
        if (gr < nrows) {
            if (train && a.crow_n) {
                n = a.crow_n[gr];
            } else if (train) {
                const uint64_t idx = minibatch_row(a.row_index, (uint64_t)(a.start + gr), a.fk);
                if (idx < a.fk.n) n = (int)(idx / a.KF);
            } else {
                n = (int)gr;
            }
        }
        rn[tid] = n;
    }
    lds_sync();
    for (int i = tid; i < ROWS * k1w; i += THREADS) {
        const int r = i / k1w, c = i % k1w, n = rn[r];
        a0[r * lda0 + c] = P::cvt((n >= 0 && c < SD) ? a.obs[(size_t)n * SD + c] : 0.f);
    }
    lds_sync();
    if (train) {   // csT image (permuted row order, img_pos) from the input tile
        for (int i = tid; i < (ROWS / 8) * SD; i += THREADS) {
            const int c = i / (ROWS / 8), g = i % (ROWS / 8);
            store_img8<P>(a.ws.csT, a.ws.ldm, grow0, c, g, [&](int r) { return P::tof(a0[r * lda0 + c]); });
        }
    }

    const int ntile0 = wave * NT;
    const __amdgpu_buffer_rsrc_t rs = packed_rsrc(a.packed);
    auto W = [&](int seg) { return wsrc(rs, L.off[seg]); };
    f32x4 H1[MT][NT], H2[MT][NT], acc[MT][NT];
    [[maybe_unused]] f32x4 H3[MT][NT];   // PLAIN only: L3's accumulator, kept for B4 (RESIDUAL accumulates into acc)
    f32x4 (&h3)[MT][NT] = *[&] { if constexpr (plain) return &H3; else return &acc; }();
    WRing<NT> R;
    ring_prime(R, W(SEG_W_IN), KSI, ntile0, lane);
    ORing<NOK, 1> ob;
    out_prefetch<NOK, 1, WAVES>(ob, W(SEG_W_OUT), KSH, wave, lane);
    // L1: h1 = s W_in + b
    gemm_stream<P, MT, NT, KSI>(a0, lda0, W(SEG_W_IN), ntile0, H1, lane, R, NextLayer{W(SEG_W_L1), KSH, ntile0});
    add_bias(H1, bias, ntile0, lane);
    if constexpr (LN) ln_fwd(0, H1, acc);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (LN) acc[m][n][r] = mishf(acc[m][n][r]);
                else acc[m][n][r] = mishf(H1[m][n][r]);
            }
    store_acc_lds<P, MT, NT>(tA, ldh, ntile0, lane, acc);
    if constexpr (train) store_accT<P, MT, NT>(wsr, ws_off(a.ws, a.ws.cu1T), ldm32, ntile0, grow32, lane, acc);
    lds_sync();
    // L2: h2 = mish(h1) W_l1 + b
    gemm_stream<P, MT, NT, KSH>(tA, ldh, W(SEG_W_L1), ntile0, H2, lane, R, NextLayer{W(SEG_W_L2), KSH, ntile0});
    add_bias(H2, bias + HC, ntile0, lane);
    if constexpr (LN) ln_fwd(1, H2, acc);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (LN) acc[m][n][r] = mishf(acc[m][n][r]);
                else acc[m][n][r] = mishf(H2[m][n][r]);
            }
    store_acc_lds<P, MT, NT>(tB, ldh, ntile0, lane, acc);
    if constexpr (train) store_accT<P, MT, NT>(wsr, ws_off(a.ws, a.ws.cu2T), ldm32, ntile0, grow32, lane, acc);
    lds_sync();
    // L3: h3 = mish(h2) W_l2 + b + h1 (PLAIN: no + h1, and the out-Dense operand is u3 = mish(h3))
    gemm_stream<P, MT, NT, KSH>(tB, ldh, W(SEG_W_L2), ntile0, h3, lane, R,
                                train ? NextLayer{W(SEG_T_OUT), KSO, ntile0} : NextLayer{W(SEG_W_L2), KSH, ntile0});
    add_bias(h3, bias + 2 * HC, ntile0, lane);
    if constexpr (LN && plain) ln_fwd(2, H3, acc);   // (RESIDUAL: no norm here, and the skip is the raw h1)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (LN && plain) acc[m][n][r] = mishf(acc[m][n][r]);
                else if constexpr (plain) acc[m][n][r] = mishf(H3[m][n][r]);
                else acc[m][n][r] += H1[m][n][r];
            }
    store_acc_lds<P, MT, NT>(tA, ldh, ntile0, lane, acc);
    if constexpr (train) store_accT<P, MT, NT>(wsr, ws_off(a.ws, a.ws.ch3T), ldm32, ntile0, grow32, lane, acc);
    lds_sync();
    // L4: V = h3 W_out + b (PLAIN: u3)
    {
        f32x4 po[MT][1];
        gemm_narrow_pre<P, MT, NOK, 1, WAVES>(tA, ldh, ob, po, wave, lane);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[(wave * ROWS + m * 16 + crow(lane, r)) * 16 + ccol(lane)] = po[m][0][r];
    }
    lds_sync();
    if (wave == 0 && lane < ROWS) {
        const int r = lane, n = rn[r];
        float V = bias[3 * HC];
#pragma unroll
        for (int w = 0; w < WAVES; ++w) V += part[(w * ROWS + r) * 16];
        if (!train) {
            if (n >= 0) a.values[n] = V;
        } else {
            float vl = 0.f, dv = 0.f;
            if (n >= 0) {
                const float w = a.crow_mult ? (float)a.crow_mult[n] : 1.f;   // copies of the sample in the minibatch
                const float R = a.returns[n], diff = V - R;
                if (a.hp.clip_vloss > 0.f) {
                    // diffusion_ppo.py:110-116: 0.5 max((V-R)^2, (V_old + clip(V - V_old, -c, c) - R)^2); the
                    // gradient as TF routes it: tf.maximum's to its first argument on ties, clip_by_value's
                    // through where V - V_old lies in [-c, c] (bounds included), zero outside
                    const float c = a.hp.clip_vloss, old = a.hp.old_values[n], d = V - old;
                    const float vc = old + fminf(fmaxf(d, -c), c), dc = vc - R;
                    const float lu = diff * diff, lc = dc * dc;
                    vl = 0.5f * fmaxf(lu, lc) * w;
                    const float g = lu >= lc ? diff : ((d >= -c && d <= c) ? dc : 0.f);
                    dv = a.hp.vf_coef * g * a.hp.grad_scale * w;
                } else {
                    vl = 0.5f * diff * diff * w;                     // v_loss = 0.5 mean((V-R)^2), diffusion_ppo.py:118
                    dv = a.hp.vf_coef * diff * a.hp.grad_scale * w;  // loss = pg + vf_coef * v_loss (agent :340)
                }
            }
            for (int q = 0; q < ktw; ++q) a0[r * lda0 + q] = P::cvt(q == 0 ? dv : 0.f);
            ((AT*)a.ws.cdvT)[grow0 + img_pos(r)] = P::cvt(dv);
            vl = wave_sum(vl);
            if (lane == 0) atomic_add_metric(a.metrics, 1, vl);
        }
    }
    if constexpr (!train) return;
    lds_sync();
    // B4: dh3 = dV W_out^T (kept only in tB, re-read by B2; no image, as the actor's)
    // PLAIN: dh3 = (dV W_out^T) * mish'(h3), to tB and to the cdh3T image (l2's dW operand)
    gemm_stream<P, MT, NT, KSO>(a0, lda0, W(SEG_T_OUT), ntile0, acc, lane, R, NextLayer{W(SEG_T_L2), KSH, ntile0});
    if constexpr (LN && plain) {
        ln_bwd(2, acc, H3);
    } else if constexpr (plain) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[m][n][r] *= mish_gradf(H3[m][n][r]);
    }
    store_acc_lds<P, MT, NT>(tB, ldh, ntile0, lane, acc);
    if constexpr (plain) store_accT<P, MT, NT>(wsr, ws_off(a.ws, a.ws.cdh3T), ldm32, ntile0, grow32, lane, acc);
    lds_sync();
    // B3: dh2 = (dh3 W_l2^T) * mish'(h2)
    gemm_stream<P, MT, NT, KSH>(tB, ldh, W(SEG_T_L2), ntile0, acc, lane, R, NextLayer{W(SEG_T_L1), KSH, ntile0});
    if constexpr (LN) {
        ln_bwd(1, acc, H2);
    } else {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[m][n][r] *= mish_gradf(H2[m][n][r]);
    }
    store_acc_lds<P, MT, NT>(tA, ldh, ntile0, lane, acc);
    store_accT<P, MT, NT>(wsr, ws_off(a.ws, a.ws.cdh2T), ldm32, ntile0, grow32, lane, acc);
    lds_sync();
    // B2: dh1 = dh3 + (dh2 W_l1^T) * mish'(h1) (PLAIN: no dh3 term, tB is not re-read)
    gemm_stream<P, MT, NT, KSH>(tA, ldh, W(SEG_T_L1), ntile0, acc, lane, R, NextLayer{W(SEG_T_L1), KSH, ntile0});
    if constexpr (LN) ln_bwd(0, acc, H1);   // dh1's norm share; RESIDUAL adds the skip's dh3 below
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (LN && plain) {
                } else if constexpr (LN) {
                    acc[m][n][r] += P::tof(tB[(m * 16 + crow(lane, r)) * ldh + (ntile0 + n) * 16 + ccol(lane)]);
                } else if constexpr (plain) {
                    acc[m][n][r] *= mish_gradf(H1[m][n][r]);
                } else {
                    const float dh3 = P::tof(tB[(m * 16 + crow(lane, r)) * ldh + (ntile0 + n) * 16 + ccol(lane)]);
                    acc[m][n][r] = dh3 + acc[m][n][r] * mish_gradf(H1[m][n][r]);
                }
            }
    store_accT<P, MT, NT>(wsr, ws_off(a.ws, a.ws.cdh1T), ldm32, ntile0, grow32, lane, acc);
}

// Kernel entry points: the _o4 form caps registers at 128 (rowtile.hip); the _ln form is the LN axis on the plain
// 8-wave entry (its TRAIN tiles take 223-253 registers: no _o4 twin)
template <class P, int MT, int NT, bool TRAIN, int WAVES, int HEAD>
__global__ __launch_bounds__(64 * WAVES) void critic_rowtile_kernel(CriticArgs a) {
    critic_rowtile_body<P, MT, NT, TRAIN, WAVES, HEAD>(a);
}
template <class P, int MT, int NT, bool TRAIN, int WAVES, int HEAD>
__global__ __launch_bounds__(64 * WAVES) void critic_rowtile_kernel_ln(CriticArgs a) {
    critic_rowtile_body<P, MT, NT, TRAIN, WAVES, HEAD, true>(a);
}
template <class P, int MT, int NT, bool TRAIN, int WAVES, int HEAD>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(4))) void critic_rowtile_kernel_o4(CriticArgs a) {
    critic_rowtile_body<P, MT, NT, TRAIN, WAVES, HEAD>(a);
}

template <class P, int MT, int NT, bool TRAIN, int WAVES, bool O4, int HEAD, bool LN = false>
static int launch_critic_t(const CriticArgs& a, hipStream_t s, bool dry) {
    if (a.L.ks_in != 2 || a.L.ks_h != ksh_for<P>(NT, WAVES) || a.L.ks_out_t != 2 || a.L.ks_h != WAVES * nok_for<P>(NT))
        return dppo_set_error(DPPO_EUNSUPPORTED, "critic row tile: layout does not match the instantiation");
    const CriticSmem<P, MT, LN ? (HEAD == DPPO_HEAD_PLAIN ? 3 : 2) : 0> S(a);
    if (S.total > 160 * 1024) return dppo_set_error(DPPO_EUNSUPPORTED, "critic row tile needs %zu B LDS", S.total);
    if (LN && TRAIN && !a.gln) return dppo_set_error(DPPO_EINVAL, "critic row tile: a layer-normed image needs the gradient tail");
    if ((size_t)4 * WAVES * 16 * MT * 16 > sizeof(typename P::AT) * 16 * MT * (a.HC + lds_pad_elems<P>()))
        return dppo_set_error(DPPO_EUNSUPPORTED, "critic: partial buffer does not fit");
    if (dry) return DPPO_OK;
    // LN: the plain 8-wave entry only (no 128-register twin, see the entry points above)
    void (*k)(CriticArgs);
    if constexpr (LN) k = critic_rowtile_kernel_ln<P, MT, NT, TRAIN, WAVES, HEAD>;
    else k = O4 ? critic_rowtile_kernel_o4<P, MT, NT, TRAIN, WAVES, HEAD> : critic_rowtile_kernel<P, MT, NT, TRAIN, WAVES, HEAD>;
    { const int rc_ = dppo_func_lds((const void*)k, (size_t)S.total); if (rc_) return rc_; }
    // TRAIN mode covers every row of the 64-padded feature-major images (padding rows get
    // finite activations and zero gradients), so the dW kernel never reads unwritten memory
    const int64_t rows = a.mode == ROWS_TRAIN ? (int64_t)a.ws.ldm : a.nrows;
    const int64_t grid = (rows + 16 * MT - 1) / (16 * MT);
    if (grid == 0) return DPPO_OK;
    DppoKtScope kt(a.mode == ROWS_TRAIN ? KT_CRITIC_TRAIN : KT_CRITIC_FWD, s);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(64 * WAVES), S.total, s, a);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

