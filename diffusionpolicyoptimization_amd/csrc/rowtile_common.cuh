// rowtile_common.cuh — pieces shared by the row-tile kernels (rowtile.hip, rowtile128.hip): the
// permuted feature-major image layout, accumulator stores, bias add, metric atomics.
#pragma once
#include "dppo_ppo.h"

#define LOG_2PI_HALF 0.91893853320467274178f

// Feature-major images XT[col][row] hold the rows of each 16*MT-row tile in a PERMUTED order:
// position p of a tile holds row img_row(p), so that the 8 rows one lane holds for a column across
// an (even, odd) pair of MFMA tiles (rows 16m + 4j + 0..3 of tiles m = 2P, 2P+1, j = lane >> 4) are
// 8 consecutive positions and leave as ONE 16-byte store (8-byte per-lane stores made the image
// writes store-issue bound). Every image of a dW pair and the actor's seg[] use the same order;
// the dW GEMM sums over rows, so the order is invisible in its result.
__device__ inline int img_pos(int r) {
    const int m = r >> 4;
    return 32 * (m >> 1) + 8 * ((r >> 2) & 3) + 4 * (m & 1) + (r & 3);
}
__device__ inline int img_row(int p) {
    return 16 * (2 * (p >> 5) + ((p >> 2) & 1)) + 4 * ((p >> 3) & 3) + (p & 3);
}

// Accumulator tile -> feature-major image. Buffer stores through ONE resource for the whole
// workspace: the per-lane part of the offset is a single 32-bit VGPR, the image / tile parts are
// scalar, so no 64-bit address pairs are kept live across the unrolled layers.
template <class P, int MT, int NT>
__device__ inline void store_accT(__amdgpu_buffer_rsrc_t ws, uint32_t img_off, uint32_t ldm, int ntile0, uint32_t grow0,
                                  int lane, const f32x4 (&v)[MT][NT]) {
    static_assert(MT % 2 == 0, "image rows are permuted over MFMA tile pairs");
    using AT = typename P::AT;
    constexpr uint32_t es = sizeof(AT);
    const uint32_t vo = ((uint32_t)ccol(lane) * ldm + (uint32_t)((lane >> 4) << 3)) * es;
    const uint32_t so0 = img_off + ((uint32_t)ntile0 * 16u * ldm + grow0) * es;
#pragma unroll
    for (int mp = 0; mp < MT / 2; ++mp)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const uint32_t so = so0 + ((uint32_t)n * 16u * ldm + (uint32_t)mp * 32u) * es;
            const f32x4 lo = v[2 * mp][n], hi = v[2 * mp + 1][n];
            if constexpr (es == 2) {
                const u32x4 e = {P::pack2(lo[0], lo[1]), P::pack2(lo[2], lo[3]),
                                 P::pack2(hi[0], hi[1]), P::pack2(hi[2], hi[3])};
                // soffset must be the literal 0: with an SGPR there, hipcc (ROCm 7.2) does not guard
                // the >8-byte store-data hazard (a following VALU overwrote the 4th dword)
                __builtin_amdgcn_raw_buffer_store_b128(e, ws, vo + so, 0, 0);
            } else {
                // 8-B stores: the 16-B buffer_store form came out with a corrupted 4th dword under
                // hipcc 7.2 for gfx950 in the fp32 critic (a store-data hazard the compiler does
                // not guard); fp32 is the parity mode, so exactness wins here
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(lo[0]), __float_as_uint(lo[1])}, ws, vo, so, 0);
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(lo[2]), __float_as_uint(lo[3])}, ws, vo, so + 8, 0);
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(hi[0]), __float_as_uint(hi[1])}, ws, vo, so + 16, 0);
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(hi[2]), __float_as_uint(hi[3])}, ws, vo, so + 24, 0);
            }
        }
}

// image positions [8g, 8g + 8) of column c (rows img_row(p), value(r)) in one 16-B store (bf16)
// or four 8-B stores (fp32)
template <class P, class F>
__device__ inline void store_img8(void* img, size_t ldm, size_t grow0, int c, int g, F value) {
    using AT = typename P::AT;
    float e[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = value(img_row(8 * g + k));
    AT* dst = (AT*)img + (size_t)c * ldm + grow0 + 8 * g;
    if constexpr (sizeof(AT) == 2) {
        *(u32x4*)dst = u32x4{P::pack2(e[0], e[1]), P::pack2(e[2], e[3]),
                             P::pack2(e[4], e[5]), P::pack2(e[6], e[7])};
    } else {
#pragma unroll
        for (int k = 0; k < 8; k += 2) *(u32x2*)(dst + k) = u32x2{__float_as_uint(e[k]), __float_as_uint(e[k + 1])};
    }
}

template <class P, int MT, int NT>
__device__ inline void store_acc_lds(typename P::AT* T, int ld, int ntile0, int lane, const f32x4 (&v)[MT][NT]) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int col = (ntile0 + n) * 16 + ccol(lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) T[(m * 16 + crow(lane, r)) * ld + col] = P::cvt(v[m][n][r]);
        }
}

template <int MT, int NT>
__device__ inline void add_bias(f32x4 (&v)[MT][NT], const float* __restrict__ b, int ntile0, int lane) {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const float bv = b[(ntile0 + n) * 16 + ccol(lane)];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[m][n][r] += bv;
    }
}

__device__ inline void atomic_add_metric(double* m, int i, double v) { atomicAdd(m + i, v); }

// ------------------------------------------------------------------------------------------------
// Layer normalisation across a hidden width that is split over the waves of a row tile (the critic's
// LN axis). A lane holds, for each of its 4 MT rows, NT of the row's columns: a row statistic is summed over
// those in registers, over the 16 column lanes of the wave with DPP, and over the waves through one LDS
// round: lane column 0 of every wave stores its partial to red[wave][row], and after the barrier every lane
// adds the WAVES partials of its rows in wave order, so all waves hold the same bits. Statistics are fp32
// from the fp32 accumulators at every precision.
// ------------------------------------------------------------------------------------------------
__device__ inline float row16_sum(float v) {   // the sum over the 16 lanes that share lane >> 4, in all of them
    v += dpp_movf<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_movf<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_movf<0x141>(v);   // row_half_mirror
    v += dpp_movf<0x140>(v);   // row_mirror
    return v;
}

// v[m][r] (a per-row partial of this wave's columns) -> its sum over the whole row, through red [WAVES][16 MT]
template <int MT, int WAVES>
__device__ inline void ln_row_allsum(float (&v)[MT][4], float* red, int wave, int lane) {
    constexpr int ROWS = 16 * MT;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float s = row16_sum(v[m][r]);
            if (ccol(lane) == 0) red[wave * ROWS + m * 16 + crow(lane, r)] = s;
        }
    lds_sync();
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) s += red[w * ROWS + m * 16 + crow(lane, r)];
            v[m][r] = s;
        }
}

// the same for two partials at once (a and b, each through its own [WAVES][16 MT] slot of red): one barrier for both
template <int MT, int WAVES>
__device__ inline void ln_row_allsum2(float (&a)[MT][4], float (&b)[MT][4], float* red, int wave, int lane) {
    constexpr int ROWS = 16 * MT;
    float* redb = red + WAVES * ROWS;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float sa = row16_sum(a[m][r]), sb = row16_sum(b[m][r]);
            if (ccol(lane) == 0) {
                red[wave * ROWS + m * 16 + crow(lane, r)] = sa;
                redb[wave * ROWS + m * 16 + crow(lane, r)] = sb;
            }
        }
    lds_sync();
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float sa = 0.f, sb = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                sa += red[w * ROWS + m * 16 + crow(lane, r)];
                sb += redb[w * ROWS + m * 16 + crow(lane, r)];
            }
            a[m][r] = sa; b[m][r] = sb;
        }
}

// y = gamma * x_hat + beta of the pre-activations h, x_hat = (h - mean) * rstd with the row's mean and
// population variance (two passes: the mean, then the squared deviations, so a large mean costs no digits).
// stat [2][ROWS] keeps mean and rstd for the backward, which recomputes x_hat from h with the same operations.
// red: two [WAVES][ROWS] slots
template <int MT, int NT, int WAVES>
__device__ inline void ln_forward(const f32x4 (&h)[MT][NT], f32x4 (&y)[MT][NT], const float* gam, const float* bet,
                                  float* stat, float* red, float eps, int HC, int ntile0, int wave, int lane) {
    constexpr int ROWS = 16 * MT;
    const float inv = 1.f / (float)HC;
    float mean[MT][4], var[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s = 0.f;
#pragma unroll
            for (int n = 0; n < NT; ++n) s += h[m][n][r];
            mean[m][r] = s;
        }
    ln_row_allsum<MT, WAVES>(mean, red, wave, lane);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            mean[m][r] *= inv;
            float s = 0.f;
#pragma unroll
            for (int n = 0; n < NT; ++n) { const float d = h[m][n][r] - mean[m][r]; s += d * d; }
            var[m][r] = s;
        }
    ln_row_allsum<MT, WAVES>(var, red + WAVES * ROWS, wave, lane);
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float rstd = 1.f / sqrtf(var[m][r] * inv + eps);
            if (wave == 0 && ccol(lane) == 0) {
                stat[m * 16 + crow(lane, r)] = mean[m][r];
                stat[ROWS + m * 16 + crow(lane, r)] = rstd;
            }
            var[m][r] = rstd;
        }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int col = (ntile0 + n) * 16 + ccol(lane);
        const float g = gam[col], b = bet[col];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) y[m][n][r] = g * ((h[m][n][r] - mean[m][r]) * var[m][r]) + b;
    }
}

// The backward of u = mish(LN(h)): d holds du on entry and dh on return,
//   dy = du mish'(y),  g = dy gamma,  dh = rstd (g - mean_row(g) - x_hat mean_row(g x_hat)),
// and the tile's share of dgamma = sum_rows(dy x_hat), dbeta = sum_rows(dy) goes to ggam / gbet: summed over the
// wave's rows in registers and across its four row groups, then one fp32 atomic add per column and wave
// (a padded row has du = 0 exactly, so it adds +-0). unscale takes the backward seed scale out of those sums.
// red: two [WAVES][ROWS] slots (not the forward's)
template <int MT, int NT, int WAVES>
__device__ inline void ln_backward(f32x4 (&d)[MT][NT], const f32x4 (&h)[MT][NT], const float* gam, const float* bet,
                                   const float* stat, float* red, float* ggam, float* gbet, float unscale, int HC,
                                   int ntile0, int wave, int lane) {
    constexpr int ROWS = 16 * MT;
    const float inv = 1.f / (float)HC;
    float mean[MT][4], rstd[MT][4], sg[MT][4], sgx[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            mean[m][r] = stat[m * 16 + crow(lane, r)];
            rstd[m][r] = stat[ROWS + m * 16 + crow(lane, r)];
            sg[m][r] = 0.f; sgx[m][r] = 0.f;
        }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int col = (ntile0 + n) * 16 + ccol(lane);
        const float g = gam[col], b = bet[col];
        float dg = 0.f, db = 0.f;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float xh = (h[m][n][r] - mean[m][r]) * rstd[m][r];
                const float dy = d[m][n][r] * mish_gradf(g * xh + b);
                dg += dy * xh; db += dy;
                const float gv = dy * g;
                d[m][n][r] = gv;
                sg[m][r] += gv; sgx[m][r] += gv * xh;
            }
        dg += __shfl_xor(dg, 16, 64); dg += __shfl_xor(dg, 32, 64);
        db += __shfl_xor(db, 16, 64); db += __shfl_xor(db, 32, 64);
        if (lane < 16) {
            atomicAdd(ggam + col, dg * unscale);
            atomicAdd(gbet + col, db * unscale);
        }
    }
    ln_row_allsum2<MT, WAVES>(sg, sgx, red, wave, lane);   // the backward's one cross-wave round
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float xh = (h[m][n][r] - mean[m][r]) * rstd[m][r];
                d[m][n][r] = rstd[m][r] * (d[m][n][r] - sg[m][r] * inv - xh * (sgx[m][r] * inv));
            }
}
