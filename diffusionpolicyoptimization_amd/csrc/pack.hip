// pack.hip — flat fp32 Keras parameters -> packed MFMA fragment images (dppo_layout.h).
// Replaces the Keras variable storage of model/common/mlp.py:95-206 (kernels are [in,out]).
#include "dppo_common.cuh"
#include "dppo_internal.h"

// Every segment of the images being re-derived — the actor's and/or the critic's — and the actor's
// time tables (TEMB, TIN, B_OUT2) in ONE launch: the images are re-derived after every optimiser
// step, on the critical path of every PPO minibatch, where each extra launch is a kernel boundary.
// A job is either a packed matrix (one thread per (ntile, ks, lane) fragment slot, 16 B each) or a
// zero-padded fp32 copy; the time-table blocks follow the job blocks.
#define PACK_MAXJ 24
struct PackJob {
    int kind;            // 0 = packed matrix, 1 = fp32 copy with zero padding, 2 = zero n 4-byte words
    int K, N, transposed;
    int k_split, k_skip; // source row of packed row k: k < k_split ? k : k + k_skip (row subsets)
    int n, npad;         // copy: valid / padded element counts
    const float* src;    // source params (already offset)
    uint8_t* dst;        // destination in the image (already offset)
    int threads;         // work items of this job
};
// the actor's time tables: blocks [0, R) TEMB rows; with 2-byte operands also blocks [R, 2R) TIN
// rows and block 2R B_OUT2 (tables = 2R + 1, else R); and nfold blocks of FOLD / ROUT fragments (one
// 16-feature tile each). Launch order: fold blocks, table blocks, then the element jobs
struct TembArgs {
    const float* params;
    FlatOffsets F;
    int TD, stride, R, XD, H, nout, tables, nfold;
    int plain;            // DPPO_HEAD_PLAIN image: no l2 layer, no skip (dppo_layout.h "plain head")
    int first_table;      // table block b runs time_table_block(first_table + b): R skips the TEMB rows
    float *temb, *tin, *bout2;
    uint8_t *fold, *rout;
};
struct PackArgs {
    PackJob j[PACK_MAXJ];
    int start[PACK_MAXJ + 1];
    int njobs;
    int pack_blocks;     // blocks of the job part (256 threads each), after the time-table blocks
    TembArgs tb;
};

constexpr int PACK_THREADS = 256;

// t_emb(t) = Dense(2TD->TD)(mish(Dense(TD->2TD)(SinusoidalPosEmb(t)))) (mlp_diffusion.py:40-45,
// modules.py:4-15), one workgroup per table row; the arithmetic and its order match the oracle
// restatement. With ET = the 2-byte operand type (split-sampler tables) also TIN = b_in +
// sum_j rnd(t_emb_j) rnd(W_in[XD + j]) (each block re-derives its t_emb row) and B_OUT2 = b_out +
// sum_h b_l2[h] rnd(W_out[h]) with a fixed-order reduction (the sampler's h3 is fp32-accurate, so
// b_l2 enters the out-Dense unrounded). The first 128 threads work; all take part in barriers.
template <class ET>
__device__ void time_table_block(const TembArgs& b, int blk) {
    __shared__ float te[64];
    __shared__ float ta1[128];
    __shared__ float tr[64];
    __shared__ float red[128][33];
    const int tid = threadIdx.x;
    const float* params = b.params;
    const FlatOffsets& F = b.F;
    const int TD = b.TD, R = b.R, XD = b.XD, H = b.H;
    if (blk == 2 * R) {   // B_OUT2
        if (tid < 128) {
            float acc[32];
#pragma unroll
            for (int q = 0; q < 32; ++q) acc[q] = 0.f;
            for (int h = tid; h < H; h += 128) {
                const float bl2 = b.plain ? 0.f : params[F.l2_b + h];   // plain head: B_OUT2 = b_out
#pragma unroll
                for (int q = 0; q < 32; ++q)
                    if (q < XD) acc[q] += bl2 * (float)(ET)params[F.out_w + (size_t)h * XD + q];
            }
#pragma unroll
            for (int q = 0; q < 32; ++q) red[tid][q] = acc[q];
        }
        __syncthreads();
        if (tid < b.nout) {
            float s = tid < XD ? params[F.out_b + tid] : 0.f;
            if (tid < XD)
                for (int k = 0; k < 128; ++k) s += red[k][tid];
            b.bout2[tid] = s;
        }
        return;
    }
    const int row = blk % R, t = row * b.stride;   // row r holds t_emb(r * stride)
    if (tid < TD) te[tid] = temb_sinusoid(tid, t, TD);
    __syncthreads();
    if (tid < 2 * TD) ta1[tid] = temb_hidden(params, F.time_w1, F.time_b1, te, TD, tid);
    __syncthreads();
    if (tid < TD) {
        const float acc = temb_output(params, F.time_w2, F.time_b2, ta1, TD, tid);
        if (blk < R) b.temb[(size_t)row * TD + tid] = acc;
        tr[tid] = (float)(ET)acc;
    }
    if (blk < R) return;
    __syncthreads();
    for (int h = tid; h < H; h += PACK_THREADS) {
        float acc = params[F.in_b + h];
#pragma unroll 16                                  // the loads in flight together, not one round trip each
        for (int j = 0; j < TD; ++j) acc += tr[j] * (float)(ET)params[F.in_w + (size_t)(XD + j) * H + h];
        b.tin[(size_t)row * H + h] = acc;
    }
}

// FOLD / ROUT fragments of feature tile T (dppo_layout.h): M[f][o] = sum_j rnd(W_l2[f][j])
// rnd(W_out[j][o]) in fp32, then split into its 2-byte hi/lo pair; ROUT is rnd(W_out) rows 16T.. in
// the same fragment geometry. The tile's W_l2 rows and W_out are staged in LDS as the rounded 2-byte
// values (exact) in one round trip at hopper's out_dim <= 16 (chunks of 256 rows above);
// thread (g, f, oq) sums j-quarter g of each chunk for feature f and outs 4 oq.. (+16), so one
// broadcast read of W_l2 and one 8-B read of W_out feed 4 FMAs; the quarters are added in a fixed
// order at the end. These blocks come first in the launch (the split sampler's table refresh).
template <class ET>
__device__ void fold_block(const TembArgs& b, int T) {
    if constexpr (sizeof(ET) == 2) {
        constexpr int JMAX = 512;
        __shared__ ET fw2[16][JMAX + 8];
        __shared__ __attribute__((aligned(16))) ET wos[JMAX * 16];   // [jc][XDP]
        __shared__ float red[4][16][33];
        __shared__ float mv[16][33];
        const int tid = threadIdx.x, H = b.H, XD = b.XD, nt_out = b.nout / 16;
        const float* params = b.params;
        const FlatOffsets& F = b.F;
        const float* wo = params + F.out_w;
        if (b.plain) {   // plain head: M = rnd(W_out) (hi exact, lo zero), no residual term (ROUT zero)
            if (tid < 64 * nt_out) {
                const int lane = tid & 63, n = tid >> 6, o = 16 * n + (lane & 15), jq = lane >> 4;
                ET e[8], w[8];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int f = 16 * T + 4 * jq + q;
                    e[q] = (ET)((o < XD && f < H) ? wo[(size_t)f * XD + o] : 0.f);
                    e[4 + q] = (ET)0.f;
                    w[q] = w[4 + q] = (ET)0.f;
                }
                const size_t idx = ((size_t)T * nt_out + n) * 64 + lane;
                reinterpret_cast<u32x4*>(b.fold)[idx] = __builtin_bit_cast(u32x4, e);
                reinterpret_cast<u32x4*>(b.rout)[idx] = __builtin_bit_cast(u32x4, w);
            }
            return;   // the whole block: no barrier is skipped
        }
        const int XDP = XD <= 16 ? 16 : 32, JC = XD <= 16 ? JMAX : JMAX / 2;
        const int g = tid >> 6, fr = (tid & 63) >> 2, oq = tid & 3;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        auto ld4 = [&](int off) {                      // 4 staged W_out values as fp32
            const u32x2 w = *(const u32x2*)(wos + off);
            return f32x4{(float)__builtin_bit_cast(ET, (uint16_t)(w[0] & 0xffffu)),
                         (float)__builtin_bit_cast(ET, (uint16_t)(w[0] >> 16)),
                         (float)__builtin_bit_cast(ET, (uint16_t)(w[1] & 0xffffu)),
                         (float)__builtin_bit_cast(ET, (uint16_t)(w[1] >> 16))};
        };
        bool whole = false;                            // W_out fully staged (one chunk)
        for (int j0 = 0; j0 < H; j0 += JC) {
            const int nj = min(JC, H - j0);
            whole = j0 == 0 && nj == H;
            __syncthreads();
            // unrolled so that 16 loads per thread are in flight (a rolled loop pays one L2
            // round trip per element)
#pragma unroll 16
            for (int i = tid; i < 16 * JC; i += PACK_THREADS) {
                const int r = i / JC, jj = i % JC, f = 16 * T + r;
                fw2[r][jj] = (ET)((jj < nj && f < H) ? params[F.l2_w + (size_t)f * H + j0 + jj] : 0.f);
            }
#pragma unroll 16
            for (int i = tid; i < JC * XDP; i += PACK_THREADS) {
                const int jj = i / XDP, o = i % XDP;
                wos[i] = (ET)((jj < nj && o < XD) ? wo[(size_t)(j0 + jj) * XD + o] : 0.f);
            }
            __syncthreads();
            const int q = JC / 4, ja = g * q;           // rows past nj are zero in both operands
            if (XDP == 32) {
#pragma unroll 4
                for (int jj = ja; jj < ja + q; ++jj) {
                    const float w = (float)fw2[fr][jj];
                    const f32x4 u = ld4(jj * 32 + 4 * oq), v = ld4(jj * 32 + 16 + 4 * oq);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        acc0[e] = fmaf(w, u[e], acc0[e]);
                        acc1[e] = fmaf(w, v[e], acc1[e]);
                    }
                }
            } else {
#pragma unroll 8
                for (int jj = ja; jj < ja + q; ++jj) {
                    const float w = (float)fw2[fr][jj];
                    const f32x4 u = ld4(jj * 16 + 4 * oq);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc0[e] = fmaf(w, u[e], acc0[e]);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            red[g][fr][4 * oq + e] = acc0[e];
            red[g][fr][16 + 4 * oq + e] = acc1[e];
        }
        __syncthreads();
        for (int i = tid; i < 16 * 32; i += PACK_THREADS) {
            const int f = i >> 5, o = i & 31;
            mv[f][o] = ((red[0][f][o] + red[1][f][o]) + red[2][f][o]) + red[3][f][o];
        }
        __syncthreads();
        if (tid < 64 * nt_out) {
            const int lane = tid & 63, n = tid >> 6, o = 16 * n + (lane & 15), jq = lane >> 4;
            ET e[8], w[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int fl = 4 * jq + q, f = 16 * T + fl;
                const float m = o < XD ? mv[fl][o] : 0.f;
                const ET hi = (ET)m;
                e[q] = hi;
                e[4 + q] = (ET)(m - (float)hi);
                const ET wq = whole ? wos[f * XDP + o] : (ET)((o < XD && f < H) ? wo[(size_t)f * XD + o] : 0.f);
                w[q] = wq;
                w[4 + q] = wq;
            }
            const size_t idx = ((size_t)T * nt_out + n) * 64 + lane;
            reinterpret_cast<u32x4*>(b.fold)[idx] = __builtin_bit_cast(u32x4, e);
            reinterpret_cast<u32x4*>(b.rout)[idx] = __builtin_bit_cast(u32x4, w);
        }
    }
}

// The row tiles' fold (dppo_layout.h RT_*), one wave per tile, on the matrix cores from the image
// the same stream has just written (the pack launch, or a fused optimizer step): the cross-element
// products a per-element step cannot form.
//   M tile T (16 l2 inputs i): M[i][o] = sum_j rnd(W_l2[i][j]) rnd(W_out[j][o]) as 16x16 MFMA tiles whose
//     A operand is the T_L2 image's n-tile T (lane: W_l2[i][8 consecutive j]) and B the W_OUT image's
//     (lane: W_out[8 consecutive j][o]): KS_h k-steps, exact products summed in fp32 (the 2-byte
//     policies; fp32 images: the fp32 values);
//   M0 tile (16 in-Dense inputs i): the same with W_in's rows read from the fp32 parameters (i < in_dim;
//     rows up to RT_FOLD0's padded k range are zero);
//   the last block: RT_BOUT = b_out + sum_h (b_in + b_l2)[h] rnd(W_out[h][o]) (fixed-order reduction).
// The tile's M values go through LDS ([o][i]) into the RT_FOLD / RT_FOLD0 slots (hi, then lo) and the
// RT_TFOLD slots of n-tile T (hi at k = o, lo at k = LOK + o).
struct RtFoldArgs {
    uint8_t* img;
    const float* params;
    FlatOffsets F;
    size_t off_wout, off_tl2, off_fold, off_fold0, off_tfold, off_bout, off_temb;
    int H, XD, IN, nt_out, ks_h, ks_in, ks_out_t, nm, nm0;
    int TD, TS, R;        // the TEMB table's rows (row r = t_emb(r TS), r < R)
    int plain;            // DPPO_HEAD_PLAIN: M = rnd(W_out), M0 = 0, RT_BOUT = b_out (no MFMA, no bias fold)
};
// one M (M0) tile: NO out tiles, the k-steps in batches of KB whose loads are all issued before the
// batch's MFMAs, with no branch inside a batch (a conditional load made hipcc wait vmcnt(0) per k-step:
// a chain of KS_h global latencies, 17 us for the launch)
template <class P, int NO, int KB, bool M0>
__device__ inline void rt_fold_tile(const RtFoldArgs& a, const __amdgpu_buffer_rsrc_t& rs, int T, int lane,
                                    float (*sm)[17]) {
    using AT = typename P::AT;
    constexpr int KG = P::KG, EPL = P::EPL;
    const WSrc wo = wsrc(rs, a.off_wout), tl2 = wsrc(rs, a.off_tl2);
    const int H = a.H, i = 16 * T + (lane & 15);
    const bool irow = i < a.IN;
    const float* wrow = a.params + a.F.in_w + (size_t)(irow ? i : 0) * H + (lane >> 4) * EPL;   // 16-B aligned
    f32x4 acc[NO];
#pragma unroll
    for (int n = 0; n < NO; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < a.ks_h; kb += KB) {
        u32x4 av[KB], bv[NO][KB];
#pragma unroll
        for (int u = 0; u < KB; ++u) {
            if constexpr (!M0) {
                av[u] = load_bfrag_c(tl2, a.ks_h, T, kb + u, lane);
            } else {   // W_in[i][8 (4) consecutive j] from the fp32 parameters, rounded as the pack rounds
                const f32x4* src = (const f32x4*)(wrow + (kb + u) * KG);
                AT e[EPL];
#pragma unroll
                for (int q = 0; q < EPL / 4; ++q) {
                    const f32x4 x = src[q];
#pragma unroll
                    for (int c = 0; c < 4; ++c) e[4 * q + c] = (AT)(irow ? x[c] : 0.f);
                }
                __builtin_memcpy(&av[u], e, 16);
            }
#pragma unroll
            for (int n = 0; n < NO; ++n) bv[n][u] = load_bfrag_c(wo, a.ks_h, n, kb + u, lane);
        }
#pragma unroll
        for (int u = 0; u < KB; ++u)
#pragma unroll
            for (int n = 0; n < NO; ++n) acc[n] = P::mma(av[u], bv[n][u], acc[n]);
    }
    // C[m = i][n = o]: lane holds i = 4 (lane >> 4) + r, o = 16 n + (lane & 15)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) sm[16 * n + (lane & 15)][4 * (lane >> 4) + r] = n < NO ? acc[n < NO ? n : 0][r] : 0.f;
}

// RT_BOUT = b_out + sum_j (b_in + b_l2)[j] rnd(W_out[j][o]): lane (o = lane & 15, group jg = lane >> 4)
// takes rnd(W_out) from the W_OUT image's fragments (its EPL consecutive j per k-step, zero past out_dim)
// and the bias sums of those j, 4 k-steps per batch of loads; the 4 groups add through two lane swaps
template <class P, int NO>
__device__ inline void rt_fold_bias(const RtFoldArgs& a, const __amdgpu_buffer_rsrc_t& rs, int lane) {
    using AT = typename P::AT;
    constexpr int KG = P::KG, EPL = P::EPL, KB = 4;
    const WSrc wo = wsrc(rs, a.off_wout);
    const int jg = lane >> 4;
    const float* bi = a.params + a.F.in_b + jg * EPL;   // 16-B aligned (host-checked offsets)
    const float* bl = a.params + a.F.l2_b + jg * EPL;
    float acc[NO];
#pragma unroll
    for (int n = 0; n < NO; ++n) acc[n] = 0.f;
    for (int kb = 0; kb < a.ks_h; kb += KB) {
        u32x4 w[NO][KB];
        f32x4 vb[KB][EPL / 4], vl[KB][EPL / 4];
#pragma unroll
        for (int u = 0; u < KB; ++u) {
#pragma unroll
            for (int n = 0; n < NO; ++n) w[n][u] = load_bfrag_c(wo, a.ks_h, n, kb + u, lane);
#pragma unroll
            for (int q = 0; q < EPL / 4; ++q) {
                vb[u][q] = *(const f32x4*)(bi + (kb + u) * KG + 4 * q);
                vl[u][q] = *(const f32x4*)(bl + (kb + u) * KG + 4 * q);
            }
        }
#pragma unroll
        for (int u = 0; u < KB; ++u)
#pragma unroll
            for (int n = 0; n < NO; ++n) {
                AT e[EPL];
                __builtin_memcpy(e, &w[n][u], 16);
#pragma unroll
                for (int q = 0; q < EPL; ++q) acc[n] = fmaf(vb[u][q / 4][q % 4] + vl[u][q / 4][q % 4], (float)e[q], acc[n]);
            }
    }
    float* bout = (float*)(a.img + a.off_bout);
#pragma unroll
    for (int n = 0; n < NO; ++n) {
        float v = acc[n];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        const int o = 16 * n + (lane & 15);
        if (lane < 16) bout[o] = o < a.XD ? a.params[a.F.out_b + o] + v : 0.f;
    }
}

template <class P>
__global__ __launch_bounds__(64) void rt_fold_kernel(RtFoldArgs a) {
    using AT = typename P::AT;
    constexpr int KG = P::KG, EPL = P::EPL;
    constexpr bool TWO = sizeof(AT) == 2;
    constexpr int NHL = TWO ? 2 : 1, NLG = 16 / EPL;
    __shared__ float sm[32][17];   // [o][i] of the tile
    const int lane = threadIdx.x, b = (int)blockIdx.x;
    const int XD = a.XD, H = a.H;
    const float* prm = a.params;
    if (b > a.nm + a.nm0) {   // TEMB row r (the row tiles read their time embeddings from the table)
        const int r = b - a.nm - a.nm0 - 1, TD = a.TD;
        float* te = &sm[0][0];          // [TD]
        float* a1 = te + 64;            // [2 TD]
        if (lane < TD) te[lane] = temb_sinusoid(lane, r * a.TS, TD);
        __syncthreads();
        if (lane < 2 * TD) a1[lane] = temb_hidden(prm, a.F.time_w1, a.F.time_b1, te, TD, lane);
        __syncthreads();
        if (lane < TD) ((float*)(a.img + a.off_temb))[(size_t)r * TD + lane] = temb_output(prm, a.F.time_w2, a.F.time_b2, a1, TD, lane);
        return;
    }
    const __amdgpu_buffer_rsrc_t rs = packed_rsrc(a.img);
    if (b == a.nm + a.nm0) {   // RT_BOUT
        if (a.plain) {
            if (lane < 16 * a.nt_out) ((float*)(a.img + a.off_bout))[lane] = lane < XD ? prm[a.F.out_b + lane] : 0.f;
            return;
        }
        if (a.nt_out > 1) rt_fold_bias<P, 2>(a, rs, lane);
        else rt_fold_bias<P, 1>(a, rs, lane);
        return;
    }
    const bool m0 = b >= a.nm;
    const int T = m0 ? b - a.nm : b;
    const int kb4 = a.ks_h % 8 ? 4 : 8;   // k-steps per batch (H = 128 / 384 with 2-byte operands: 4)
    if (a.plain) {   // the tile's M values read off W_out (rounded as the pack rounds); M0 tiles are zero
        for (int idx = lane; idx < 32 * 16; idx += 64) {
            const int o = idx >> 4, i = idx & 15, f = 16 * T + i;
            sm[o][i] = (!m0 && o < XD && f < H) ? (float)(AT)prm[a.F.out_w + (size_t)f * XD + o] : 0.f;
        }
    } else if (m0) {
        if (a.nt_out > 1) { if (kb4 == 8) rt_fold_tile<P, 2, 8, true>(a, rs, T, lane, sm); else rt_fold_tile<P, 2, 4, true>(a, rs, T, lane, sm); }
        else { if (kb4 == 8) rt_fold_tile<P, 1, 8, true>(a, rs, T, lane, sm); else rt_fold_tile<P, 1, 4, true>(a, rs, T, lane, sm); }
    } else {
        if (a.nt_out > 1) { if (kb4 == 8) rt_fold_tile<P, 2, 8, false>(a, rs, T, lane, sm); else rt_fold_tile<P, 2, 4, false>(a, rs, T, lane, sm); }
        else { if (kb4 == 8) rt_fold_tile<P, 1, 8, false>(a, rs, T, lane, sm); else rt_fold_tile<P, 1, 4, false>(a, rs, T, lane, sm); }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // RT_FOLD / RT_FOLD0 slots of the tile: copy h, lane group lg of its k range, column c
    {
        const int KS = m0 ? a.ks_in : a.ks_h;
        uint8_t* dst = a.img + (m0 ? a.off_fold0 : a.off_fold);
        const size_t mat = (size_t)a.nt_out * KS * 64 * 16;
        const int h = lane / (NLG * 16), lgl = (lane / 16) % NLG, c = lane & 15;
        if (h < NHL) {
            const int f0 = 16 * T + lgl * EPL, ks = f0 / KG, sl = c + 16 * ((f0 % KG) / EPL);
            for (int n = 0; n < a.nt_out; ++n) {
                AT e[EPL];
#pragma unroll
                for (int q = 0; q < EPL; ++q) {
                    const float m = sm[16 * n + c][lgl * EPL + q];
                    const AT hi = (AT)m;
                    e[q] = h == 0 ? hi : (AT)(m - (float)hi);
                }
                u32x4 w;
                __builtin_memcpy(&w, e, 16);
                *reinterpret_cast<u32x4*>(dst + h * mat + (((size_t)n * KS + ks) * 64 + sl) * 16) = w;
            }
        }
    }
    if (!m0) {   // RT_TFOLD n-tile T
        const int LOK = rt_tfold_lok(a.ks_out_t, KG);
        for (int ks = 0; ks < a.ks_out_t; ++ks) {
            const int k0 = ks * KG + (lane >> 4) * EPL;
            AT e[EPL];
#pragma unroll
            for (int q = 0; q < EPL; ++q) {
                const int k = k0 + q;
                const bool lo = TWO && k >= LOK;
                const int o = lo ? k - LOK : k;
                const float m = o < XD ? sm[o][lane & 15] : 0.f;
                const AT hi = (AT)m;
                e[q] = lo ? (AT)(m - (float)hi) : hi;
            }
            u32x4 w;
            __builtin_memcpy(&w, e, 16);
            *reinterpret_cast<u32x4*>(a.img + a.off_tfold + (((size_t)T * a.ks_out_t + ks) * 64 + lane) * 16) = w;
        }
    }
}

template <int KG, int EPL, class ET = __bf16>
__global__ __launch_bounds__(PACK_THREADS) void pack_all_kernel(PackArgs a) {
    int blk = (int)blockIdx.x;                       // whole blocks take a branch: no barrier is skipped
    if (blk < a.tb.nfold) {
        fold_block<ET>(a.tb, blk);
        return;
    }
    blk -= a.tb.nfold;
    // the time-table blocks next (each a chain of dependent global round trips: the launch's long
    // pole), then the element jobs, which are one round trip each
    if (blk < a.tb.tables) {
        time_table_block<ET>(a.tb, a.tb.first_table + blk);
        return;
    }
    blk -= a.tb.tables;
    const int gid = blk * blockDim.x + threadIdx.x;
    if (gid >= a.start[a.njobs]) return;
    int ji = 0;
    while (ji + 1 < a.njobs && gid >= a.start[ji + 1]) ++ji;
    const PackJob& J = a.j[ji];
    const int t = gid - a.start[ji];
    const float* W = J.src;
    if (J.kind == 1) {
        reinterpret_cast<float*>(J.dst)[t] = t < J.n ? W[t] : 0.f;
        return;
    }
    if (J.kind == 2) {   // words [4t, 4t + 4) of the range
        uint32_t* q = reinterpret_cast<uint32_t*>(J.dst);
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (4 * t + w < J.n) q[4 * t + w] = 0u;
        return;
    }
    const int KS = packed_ksteps(J.K, KG);
    const int lane = t & 63;
    const int ks = (t >> 6) % KS;
    const int nt = (t >> 6) / KS;
    const int n = nt * 16 + (lane & 15);
    u32x4 v;
    if constexpr (EPL == 8) {
        ET e[8];                 // __bf16 or _Float16 (RNE)
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = ks * KG + (lane >> 4) * EPL + q;
            const int kr = k < J.k_split ? k : k + J.k_skip;
            float x = 0.f;
            if (k < J.K && n < J.N) x = J.transposed ? W[(size_t)n * J.K + k] : W[(size_t)kr * J.N + n];
            e[q] = (ET)x;
        }
        v = __builtin_bit_cast(u32x4, e);
    } else {
        float e[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = ks * KG + (lane >> 4) * EPL + q;
            const int kr = k < J.k_split ? k : k + J.k_skip;   // row subsets (W_XS) as the 2-byte branch
            float x = 0.f;
            if (k < J.K && n < J.N) x = J.transposed ? W[(size_t)n * J.K + k] : W[(size_t)kr * J.N + n];
            e[q] = x;
        }
        v = __builtin_bit_cast(u32x4, e);
    }
    reinterpret_cast<u32x4*>(J.dst)[t] = v;
}

static inline uint8_t* P_out(void* p) { return (uint8_t*)p; }

// The tensors of one network's image, the one list the pack launch (add_mlp_jobs' main jobs) and the fused
// optimizer step (dppo_fuse_jobs) both map to their job structs: where the tensor starts in the flat parameters
// and how many elements it has, the image's [K][N] and where it goes, and in which form.
enum { T_FWD, T_TRANS, T_COPY, T_ZERO };   // forward fragments / fragments of the transpose / fp32 copy / zero-fill
struct ImageTensor {
    int form;
    size_t src, count;   // flat offset and elements (T_ZERO: none)
    int K, N;            // fragments: the image is [K][N] (T_TRANS: of the row-major [N][K] tensor)
    int npad;            // T_COPY: fp32 slots written, zeros past count
    size_t dst;          // byte offset in the image
};
constexpr int IMG_MAXT = 13;
static int image_tensors(const NetSpec& s, ImageTensor* t) {
    const NetLayout L = make_mlp_layout(s);
    const NetOffsets F = make_flat_offsets(s);
    const int H = s.hidden, IN = s.in_dim, OUT = s.out_dim;
    int n = 0;
    auto mat = [&](int form, size_t src, int K, int N, int seg) { t[n++] = {form, src, (size_t)K * N, K, N, 0, L.off[seg]}; };
    auto cpy = [&](size_t src, size_t count, size_t npad, size_t dst) { t[n++] = {T_COPY, src, count, 0, 0, (int)npad, dst}; };
    if (s.actor()) cpy(F.time_w1, F.in_w - F.time_w1, F.in_w - F.time_w1, L.off[SEG_TIME]);
    mat(T_FWD, F.in_w, IN, H, SEG_W_IN);
    cpy(F.in_b, H, H, L.off[SEG_B_IN]);
    mat(T_FWD, F.l1_w, H, H, SEG_W_L1);
    cpy(F.l1_b, H, H, L.off[SEG_B_L1]);
    mat(T_FWD, F.l2_w, H, H, SEG_W_L2);
    cpy(F.l2_b, H, H, L.off[SEG_B_L2]);
    mat(T_FWD, F.out_w, H, OUT, SEG_W_OUT);
    cpy(F.out_b, OUT, 16 * L.nt_out, L.off[SEG_B_OUT]);
    // transposed images: W^T viewed as a [K'=out][N'=in] weight, i.e. element (k', n') = W[n'][k']. A plain-head
    // actor's dh3 = dy W_out^T is the skip's share of dh1: none (the whole segment is zero)
    if (s.actor() && s.plain()) t[n++] = {T_ZERO, 0, 0, OUT, H, 0, L.off[SEG_T_OUT]};
    else mat(T_TRANS, F.out_w, OUT, H, SEG_T_OUT);
    mat(T_TRANS, F.l2_w, H, H, SEG_T_L2);   // the actor's: the A operand of its fold (rt_fold_kernel)
    mat(T_TRANS, F.l1_w, H, H, SEG_T_L1);
    // a layer-normed critic's gamma / beta tail, one dense fp32 copy
    if (s.ln_sites()) cpy(F.ln, F.count_all - F.ln, (L.image_bytes - L.ln_off) / 4, L.ln_off);
    return n;
}

// what: PACK_ALL, PACK_UPDATE (everything but the split sampler's tables: W_XS, FOLD / ROUT, TIN, B_OUT2),
// PACK_SAMPLER (those tables only), PACK_SAMPLER_TEMB (those tables and the TEMB table: after a fused actor step,
// any precision). Every pack with the main jobs of an actor is followed by the row tiles' fold (dppo_pack_rt_fold).
// PACK_UPDATE leaves the TEMB rows out too: the row tiles derive theirs (writing them, the r04 pack, measured no
// different; profiles/r05h_pack_temb_ab.txt)
enum { PACK_ALL = 0, PACK_UPDATE = 1, PACK_SAMPLER = 2, PACK_SAMPLER_TEMB = 3 };
// the split sampler's tables (every precision since r06: fp32 runs the split kernel at P = 4, its fold
// from RT_FOLD and its residual from W_OUT, so only the 2-byte images carry FOLD / ROUT)
static bool packs_sampler_tables(const NetSpec& s, int what) {
    return s.actor() && s.temb_steps > 0 && (what == PACK_ALL || what == PACK_SAMPLER || what == PACK_SAMPLER_TEMB);
}
// the jobs add_mlp_jobs appends for a network: its tensors and the split sampler's W_XS
static int mlp_job_count(const NetSpec& s, int what) {
    ImageTensor t[IMG_MAXT];
    return ((what == PACK_ALL || what == PACK_UPDATE) ? image_tensors(s, t) : 0) + (packs_sampler_tables(s, what) ? 1 : 0);
}

// the jobs of one MLP image (and, for an actor, its time tables) appended to a PackArgs; returns DPPO_OK or an
// error code
static int add_mlp_jobs(PackArgs& a, const NetSpec& s, const float* params, void* packed, int what = PACK_ALL) {
    const NetLayout L = make_mlp_layout(s);
    const NetOffsets F = make_flat_offsets(s);
    const bool main_jobs = what == PACK_ALL || what == PACK_UPDATE;
    const bool sampler_tables = packs_sampler_tables(s, what);
    const bool temb_rows = L.temb_steps > 0 && what != PACK_UPDATE;
    if (a.njobs + mlp_job_count(s, what) > PACK_MAXJ) return dppo_set_error(DPPO_EINVAL, "pack: too many images in one launch");
    auto mat = [&](size_t src, int K, int N, bool tr, size_t dst) -> PackJob& {
        PackJob& J = a.j[a.njobs++];
        J.kind = 0; J.K = K; J.N = N; J.transposed = tr ? 1 : 0; J.src = params + src; J.dst = P_out(packed) + dst;
        J.k_split = K; J.k_skip = 0;
        J.threads = dppo_cdiv(N, 16) * packed_ksteps(K, L.KG) * 64;
        return J;
    };
    if (main_jobs) {
        ImageTensor t[IMG_MAXT];
        const int nt = image_tensors(s, t);
        for (int i = 0; i < nt; ++i) {
            const ImageTensor& T = t[i];
            if (T.form == T_FWD || T.form == T_TRANS) { mat(T.src, T.K, T.N, T.form == T_TRANS, T.dst); continue; }
            PackJob& J = a.j[a.njobs++];
            J.dst = P_out(packed) + T.dst;
            if (T.form == T_COPY) { J.kind = 1; J.n = (int)T.count; J.npad = T.npad; J.src = params + T.src; J.threads = T.npad; }
            else { J.kind = 2; J.n = (int)(packed_matrix_bytes(T.K, T.N, L.KG) / 4); J.threads = (J.n + 3) / 4; }
        }
    }
    if (sampler_tables) {   // split sampler: W_in rows [x ; state] (skipping the TD time-embedding rows)
        PackJob& J = mat(F.in_w, s.in_dim - s.time_dim, s.hidden, false, L.off[SEG_W_XS]);
        J.k_split = s.out_dim;
        J.k_skip = s.time_dim;
    }
    // PACK_UPDATE leaves TEMB to its consumers too: the row tiles derive their time embeddings from the
    // fp32 time MLP (rowtile.hip), the sampler's table refresh re-derives the table (r05: the TEMB
    // blocks were the pack launch's long pole on every minibatch)
    if (s.actor() && (temb_rows || sampler_tables)) {
        if (s.time_dim > 64 || s.out_dim > 32)
            return dppo_set_error(DPPO_EUNSUPPORTED, "time table: time_dim <= 64 and out_dim <= 32");
        if (a.tb.params) return dppo_set_error(DPPO_EINVAL, "pack: one actor per launch");
        TembArgs& b = a.tb;
        b.params = params; b.F = F; b.TD = s.time_dim; b.stride = s.time_stride; b.R = L.temb_steps; b.XD = s.out_dim;
        b.H = s.hidden; b.nout = 16 * L.nt_out; b.plain = s.plain() ? 1 : 0;
        b.temb = (float*)(P_out(packed) + L.off[SEG_TEMB]);
        b.tin = (float*)(P_out(packed) + L.off[SEG_TIN]);
        b.bout2 = (float*)(P_out(packed) + L.off[SEG_B_OUT2]);
        const bool fold2b = sampler_tables && dppo_prec_2b(s.precision);
        b.fold = fold2b ? P_out(packed) + L.off[SEG_FOLD] : nullptr;
        b.rout = fold2b ? P_out(packed) + L.off[SEG_ROUT] : nullptr;
        b.nfold = fold2b ? L.nt_h : 0;
        // table blocks: [0, R) TEMB rows, [R, 2R) TIN rows, 2R B_OUT2 (time_table_block)
        b.first_table = what == PACK_SAMPLER ? L.temb_steps : 0;   // PACK_SAMPLER_TEMB: the TEMB rows too
        b.tables = sampler_tables ? 2 * L.temb_steps + 1 - b.first_table : (temb_rows ? L.temb_steps : 0);
    }
    return DPPO_OK;
}

// the network's tensors (PACK_UPDATE's main jobs) as element ranges of the flat parameters, same segments and
// geometry; a zero-filled segment stays as the pack left it (a plain-head actor's T_OUT: W_out has no transposed
// slots to rewrite) and the TEMB table is derived separately (the fold launch)
int dppo_fuse_jobs(const NetSpec& s, void* packed, FuseJob* jobs) {
    const int KG = dppo_prec_2b(s.precision) ? 32 : 16;
    ImageTensor t[IMG_MAXT];
    const int nt = image_tensors(s, t);
    int n = 0;
    for (int i = 0; i < nt; ++i) {
        const ImageTensor& T = t[i];
        if (T.form == T_ZERO) continue;
        if (n == FUSE_MAXJ) return -1;
        FuseJob& J = jobs[n++];
        J.kind = T.form == T_FWD ? 0 : T.form == T_TRANS ? 1 : 2;
        J.IK = T.K; J.IN = T.N; J.KS = T.form == T_COPY ? 0 : packed_ksteps(T.K, KG);
        J.lo = (int64_t)T.src; J.hi = (int64_t)(T.src + T.count); J.dst = P_out(packed) + T.dst;
    }
    return n;
}

static int launch_pack(PackArgs& a, int precision, hipStream_t s) {
    a.start[0] = 0;
    for (int i = 0; i < a.njobs; ++i) a.start[i + 1] = a.start[i] + a.j[i].threads;
    a.pack_blocks = dppo_cdiv(a.start[a.njobs], PACK_THREADS);
    const int blocks = a.tb.nfold + a.pack_blocks + a.tb.tables;
    if (blocks == 0) return DPPO_OK;
    DppoKtScope kt(KT_PACK_ALL, s);
    if (precision == DPPO_BF16)
        hipLaunchKernelGGL((pack_all_kernel<32, 8, __bf16>), dim3(blocks), dim3(PACK_THREADS), 0, s, a);
    else if (precision == DPPO_F16)
        hipLaunchKernelGGL((pack_all_kernel<32, 8, _Float16>), dim3(blocks), dim3(PACK_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL((pack_all_kernel<16, 4, float>), dim3(blocks), dim3(PACK_THREADS), 0, s, a);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

// Actor images whose split-sampler tables are stale (packed with PACK_UPDATE by an optimizer step that deferred
// them, or stepped by the fused actor step): the sampler re-derives them on its own stream before its next launch
// that reads the image (dppo_refresh_sampler_tables). The PPO row tiles never read those tables, so a run of
// minibatches packs each actor image without them and the rollout after the update pays for them once. The record
// lives in the image's registry entry; stream order is the caller's. The latest update of an image decides what is
// stale: since r05 neither a PACK_UPDATE pack nor a fused actor step rewrites TEMB (temb = true)
int dppo_mark_tables_stale(const NetSpec& actor, const float* actor_params, const void* packed_actor, bool temb) {
    if (dppo_image_mark_stale(packed_actor, StaleTables{actor, actor_params, temb})) return DPPO_OK;
    return dppo_set_error(DPPO_EINVAL, "deferred sampler tables: more than %d stale images", DPPO_MAX_STALE);
}

extern "C" int dppo_forget_image(const void* packed) {
    if (packed) dppo_image_forget(packed);
    return DPPO_OK;
}

int dppo_pack_mlp(const NetSpec& net, const float* params, void* packed, hipStream_t s) {
    PackArgs a = {};
    int rc = add_mlp_jobs(a, net, params, packed);
    if (rc) return rc;
    if (net.temb_steps > 0) dppo_image_clear_stale(packed);
    rc = launch_pack(a, net.precision, s);
    if (rc) return rc;
    return dppo_pack_rt_fold(net, params, packed, s);
}

// the critic's jobs in a pack launch of their own
static int dppo_pack_critic_image(const NetSpec& critic, const float* params, void* packed, hipStream_t s) {
    PackArgs a = {};
    const int rc = add_mlp_jobs(a, critic, params, packed);
    return rc ? rc : launch_pack(a, critic.precision, s);
}

// the row tiles' fold segments of an actor image whose W_OUT / T_L2 slots are final on stream s (after
// its pack launch or a fused optimizer step): rt_fold_kernel, one wave per tile
int dppo_pack_rt_fold(const NetSpec& net, const float* actor_params, void* packed_actor, hipStream_t s) {
    const int hidden = net.hidden, out_dim = net.out_dim, time_dim = net.time_dim, precision = net.precision;
    const NetLayout L = make_mlp_layout(net);
    if (!net.actor()) return DPPO_OK;
    if (out_dim > 32 || (dppo_prec_2b(precision) && out_dim > rt_tfold_lok(L.ks_out_t, L.KG)))
        return dppo_set_error(DPPO_EUNSUPPORTED, "row-tile fold: out_dim %d > 32", out_dim);
    const NetOffsets F = make_flat_offsets(net);
    if (F.in_w % 4 || F.in_b % 4 || F.l2_b % 4 || hidden % 8)
        return dppo_set_error(DPPO_EUNSUPPORTED, "row-tile fold: W_in / biases not 16-B aligned (time_dim %d)", time_dim);
    RtFoldArgs a = {};
    a.img = (uint8_t*)packed_actor; a.params = actor_params;
    a.F = F;
    a.off_wout = L.off[SEG_W_OUT]; a.off_tl2 = L.off[SEG_T_L2]; a.off_fold = L.off[SEG_RT_FOLD];
    a.off_fold0 = L.off[SEG_RT_FOLD0]; a.off_tfold = L.off[SEG_RT_TFOLD]; a.off_bout = L.off[SEG_RT_BOUT];
    a.H = hidden; a.XD = out_dim; a.IN = net.in_dim; a.nt_out = L.nt_out; a.ks_h = L.ks_h; a.ks_in = L.ks_in;
    a.ks_out_t = L.ks_out_t;
    a.nm = L.nt_h;
    a.nm0 = L.ks_in * L.KG / 16;   // RT_FOLD0's padded k range, 16 rows per tile
    // and the TEMB table (one block per row): the row tiles read their time embeddings from it
    a.off_temb = L.off[SEG_TEMB]; a.TD = time_dim; a.TS = net.time_stride; a.R = L.temb_steps;
    a.plain = net.plain() ? 1 : 0;
    if (time_dim > 32) return dppo_set_error(DPPO_EUNSUPPORTED, "row-tile fold: time_dim %d > 32", time_dim);
    const dim3 grid(a.nm + a.nm0 + 1 + a.R);
    DppoKtScope kt(KT_PACK_ALL, s);
    if (precision == DPPO_BF16) hipLaunchKernelGGL(rt_fold_kernel<PolicyBF16>, grid, dim3(64), 0, s, a);
    else if (precision == DPPO_F16) hipLaunchKernelGGL(rt_fold_kernel<PolicyF16>, grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL(rt_fold_kernel<PolicyF32>, grid, dim3(64), 0, s, a);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

// the record carries the NetSpec its step built from the image's attributes, which only a pack changes
extern "C" int dppo_refresh_sampler_tables(const void* packed, void* stream) {
    StaleTables e;
    if (!packed || !dppo_image_take_stale(packed, &e)) return DPPO_OK;
    PackArgs a = {};
    const int rc = add_mlp_jobs(a, e.net, e.params, (void*)packed, e.temb ? PACK_SAMPLER_TEMB : PACK_SAMPLER);
    if (rc) return rc;
    return launch_pack(a, e.net.precision, (hipStream_t)stream);
}

static void add_zero_job(PackArgs& a, void* p, size_t bytes) {
    PackJob& J = a.j[a.njobs++];
    J.kind = 2; J.dst = (uint8_t*)p; J.n = (int)(bytes / 4); J.threads = (J.n + 3) / 4;
}

int dppo_pack_models(const NetSpec& actor, const float* actor_params, void* packed_actor, const NetSpec& critic,
                     const float* critic_params, void* packed_critic, hipStream_t s, bool defer_sampler_tables,
                     void* const* zero_ptrs, const size_t* zero_bytes, int n_zero) {
    PackArgs a = {};
    int rc;
    const bool has_actor = actor_params && packed_actor, has_critic = critic_params && packed_critic;
    const int actor_what = defer_sampler_tables ? PACK_UPDATE : PACK_ALL;
    // byte ranges zeroed by the same launch (4-byte words, < 2^33 bytes each): jobs of their own. Both networks'
    // images fill the job table on their own: ranges that would not fit beside them are zeroed by a launch of their
    // own first (the caller, staged_step, has already run AdamW: refusing would leave stale images)
    const int img_jobs = (has_actor ? mlp_job_count(actor, actor_what) : 0) + (has_critic ? mlp_job_count(critic, PACK_ALL) : 0);
    // a layer-normed critic's jobs do not fit beside the actor's: its image goes in a launch of its own
    const bool critic_alone = img_jobs > PACK_MAXJ;
    if (n_zero > PACK_MAXJ) return dppo_set_error(DPPO_EINVAL, "pack: too many jobs in one launch");
    if (n_zero > 0 && n_zero + img_jobs > PACK_MAXJ) {
        PackArgs z = {};
        for (int r = 0; r < n_zero; ++r) add_zero_job(z, zero_ptrs[r], zero_bytes[r]);
        rc = launch_pack(z, actor.precision, s);
        if (rc) return rc;
        n_zero = 0;
    }
    for (int r = 0; r < n_zero; ++r) add_zero_job(a, zero_ptrs[r], zero_bytes[r]);
    if (has_actor) {
        rc = add_mlp_jobs(a, actor, actor_params, packed_actor, actor_what);
        if (rc) return rc;
        if (defer_sampler_tables) rc = dppo_mark_tables_stale(actor, actor_params, packed_actor, true);
        else dppo_image_clear_stale(packed_actor);   // a full pack makes a pending refresh moot
        if (rc) return rc;
    }
    if (has_critic) {
        rc = critic_alone ? dppo_pack_critic_image(critic, critic_params, packed_critic, s)
                          : add_mlp_jobs(a, critic, critic_params, packed_critic);
        if (rc) return rc;
    }
    rc = launch_pack(a, actor.precision, s);
    if (rc || !has_actor) return rc;
    return dppo_pack_rt_fold(actor, actor_params, packed_actor, s);
}
