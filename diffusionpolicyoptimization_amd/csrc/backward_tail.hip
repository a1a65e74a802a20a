// backward_tail.hip — what follows the dW launches of a minibatch: l2's and W_out's weight gradients
// through the linear out layer (l2_back, out_back) and the time-MLP backward.
#include "dppo_update.h"
#include "dppo_packed.cuh"

// ---------------------------------------------------------------------------------------------
// time-MLP backward (mlp_diffusion.py:40-45) from the per-t bucket sums of dh1:
//   in_b' = sum_q G[q];  dtemb[q] = G[q] . W_in[XD:XD+TD]^T;  then Dense/mish/Dense backward.
// ---------------------------------------------------------------------------------------------
#ifndef TB_THREADS
#define TB_THREADS 1024
#endif
// l2's weight gradient through the linear out layer (mlp.py:186-206: h3 = l2(.) + h1 feeds
// output_layer and nothing else, so dh3 = dy W_out^T with the out-Dense's rounded W_out, as B4 of
// the row tile forms it): dW_l2[h][j] = sum_q pl2[h][q] rnd(W_out[j][q]) with pl2 = u2^T dy from the
// dW GEMM, db_l2[j] = sum_q db_out[q] rnd(W_out[j][q]). Replaces an [H x rows] dh3 image (written by
// the row tile, read back by the dW GEMM) and an H x H x rows GEMM by an H x N x rows one.
struct L2Back {
    const float* pl2;     // [H][N]
    const float* gob;     // [N] db_out (final: the dW launch before this one produced it)
    const uint8_t* wimg;  // the packed W_OUT image ([K = H][N] in fragment order, operands rounded)
    float* gw;            // [H][H] dW_l2
    float* gb;            // [H] db_l2
    int H, N, prec;       // prec: DPPO_BF16 / DPPO_F16 (2-byte fragments) or fp32
    // critic: the minibatch's sample counts to zero afterwards (cnt[crow_n[r]], r < *crow_cnt), or null
    uint32_t* zcnt;
    const int* zlist;
    const int* zn;
};
// Workgroup b forms rows [L2B_ROWS b, +L2B_ROWS) of dW_l2 (workgroup 0 also db_l2): thread t owns
// columns j = t, t + 256, ... with rnd(W_out[j][:]) in registers; the workgroup's pl2 rows are
// loaded up front (uniform addresses: one round trip for all of them, not one per row). No LDS and
// a few hundred FMAs per thread, so the launch fits beside the other stream's row tiles. (r03: inside
// time_bwd's single workgroup the H x H x N products took 210 us; as extra workgroups of that launch,
// inheriting its dynamic LDS, they waited for CUs, 48 us; one row's loads at a time, 33 us. r04's
// time_l2_bwd_kernel nevertheless runs them as extra workgroups of time_bwd's launch — one launch
// fewer on the chain measured faster at 6,250 rows, profiles/r04l_tail_ab.txt — and is used only by
// the default step path (DPPO_FUSED_STEP=critic) below 16,384 rows. Since ABI 12 the one-launch actor step
// runs the time-MLP backward itself and l2_back, when materialised, is this LDS-free launch alone.)
constexpr int L2B_ROWS = 4;   // rows h of dW_l2 per workgroup
constexpr int L2B_MAXN = 32;
template <int PREC, int NJ, int NQ>
__device__ inline void l2_back_cols(const L2Back& a, int b, int t, int nt) {
    // branch-free loads (a conditional load made hipcc wait for it alone): N is the instantiation's
    // width for the cfgs' widths (l2_back_rows_p), the workgroup's rows exist (b < H / L2B_ROWS), column
    // indices past H are clamped and their stores masked
    const int H = a.H, N = NQ < L2B_MAXN ? NQ : a.N;
    const int h0 = L2B_ROWS * b;
    float pv[L2B_ROWS + 1][NQ];   // the workgroup's pl2 rows, then db_out (stored by workgroup 0)
#pragma unroll
    for (int r = 0; r < L2B_ROWS; ++r)
#pragma unroll
        for (int q = 0; q < NQ; ++q) pv[r][q] = q < N ? a.pl2[(size_t)(h0 + r) * N + q] : 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) pv[L2B_ROWS][q] = q < N ? a.gob[q] : 0.f;
    // both columns' W_out values up front when they fit the registers (NQ <= 16), else one column at a
    // time (the 1024-thread time_l2_bwd workgroups have 128 VGPRs)
    constexpr int NW = NQ <= 16 ? NJ : 1;
    float w[NW][NQ];
    auto load_w = [&](int c, float* dst) {
        const int j = min(t + c * nt, H - 1);
#pragma unroll
        for (int q = 0; q < NQ; ++q) dst[q] = q < N ? packed_elem_t<PREC>(a.wimg, H, j, q) : 0.f;
    };
    if constexpr (NW == NJ) {
#pragma unroll
        for (int c = 0; c < NJ; ++c) load_w(c, w[c]);
    }
#pragma unroll
    for (int c = 0; c < NJ; ++c) {
        const int j = t + c * nt;
        if constexpr (NW != NJ) load_w(c, w[0]);
        const float* wc = w[NW == NJ ? c : 0];
        if (j >= H) continue;
#pragma unroll
        for (int r = 0; r <= L2B_ROWS; ++r) {
            float sum = 0.f;
#pragma unroll
            for (int q = 0; q < NQ; ++q) sum = fmaf(pv[r][q], wc[q], sum);
            if (r < L2B_ROWS) a.gw[(size_t)(h0 + r) * H + j] = sum;
            else if (b == 0) a.gb[j] = sum;
        }
    }
}
template <int PREC, int NQ>
__device__ inline void l2_back_n(const L2Back& a, int b, int t) {   // 256 threads per row group b
    if (a.H <= 256) l2_back_cols<PREC, 1, NQ>(a, b, t, 256);
    else l2_back_cols<PREC, 2, NQ>(a, b, t, 256);
}
// the kernels below are instantiated per precision and width NQ (the action-chunk widths of the cfgs:
// hopper 12, walker2d / halfcheetah 24, the critic's 1, any other N <= 32 zero-padded to 32): a runtime
// switch made hipcc outline the bodies as calls, and the unused widths' registers spilled in the
// 1024-thread time_l2_bwd workgroups
__host__ __device__ constexpr int l2_nq(int N) { return N == 1 ? 1 : (N == 12 ? 12 : (N == 24 ? 24 : L2B_MAXN)); }
// W_out's weight gradient through the folded forward (rowtile.hip: the row tiles never form h3,
// dppo_ppo.h pa0): dW_out[f][q] = sum_g rnd(W_l2[g][f]) pl2[g][q] + sum_i rnd(W_in[i][f]) pa0[i][q] +
// (b_l2[f] + b_in[f]) db_out[q], the oracle's h3^T dy with h3 = u2 rnd(W_l2) + b_l2 + a0 rnd(W_in) + b_in.
// A group of 256 threads forms OBR rows f (4 for N <= 16, else 2: 64 partial sums per thread either
// way): thread t takes rows g = t, t + 256 of W_l2 / pl2 (OBR features in one load) and row i = t of
// W_in / pa0, all loads issued before the FMAs (one round trip; a rolled loop waited for each row in
// turn); the 64 partial sums reduce over the lanes by recursive halving and then over the 4 waves
// through LDS in a fixed order. Sized for 128 VGPRs (time_l2_bwd's 1024-thread workgroups: the first
// form, 4 rows x 32 widths, spilled 1 KB per lane there).
struct OutBack {
    const float* prm;     // the actor's flat fp32 parameters
    FlatOffsets F;
    const float* pl2;     // [H][N] (the factored l2 region of the gradients when l2 is deferred)
    const float* pa0;     // [IN][N]
    const float* gob;     // [N] db_out (final: the dW launch before this one produced it)
    float* gw;            // [H][N] dW_out
    int H, IN, N, prec;
};
static OutBack make_out_back(const Dims& D, int precision, const float* actor_params, const float* pl2, const float* pa0,
                             float* ga) {
    const FlatOffsets FA = make_flat_offsets(actor_net(D));
    return OutBack{actor_params, FA, pl2, pa0, ga + FA.out_b, ga + FA.out_w, D.H, D.IN, D.XD, precision};
}
// (of the INSTANTIATED width l2_nq(N): the host's group count must use the same width as the kernel)
__host__ __device__ constexpr int ob_rows(int N) { return N <= 16 ? 4 : 2; }
template <int PREC, int NQ>
__device__ inline void out_back_n(const OutBack& a, int b, bool valid, int t, float* red) {
    constexpr int OBR = ob_rows(NQ), NQP = NQ <= 16 ? 16 : 32, V = OBR * NQP;   // V = 64
    static_assert(V == 64, "one value per lane after the halving");
    const int H = a.H, f0 = OBR * b, lane = t & 63, w = t >> 6;
    const int NE = NQ < L2B_MAXN ? NQ : a.N;   // the instantiation's width (out_back_group)
    float x[V];
#pragma unroll
    for (int v = 0; v < V; ++v) x[v] = 0.f;
    if (valid) {
        // batches of rows g = t + 512 c, t + 512 c + 256 of W_l2 / pl2, then row t of W_in / pa0
        const int nb = (H + 511) / 512;
        for (int c = 0; c <= nb; ++c) {
            constexpr int NU = 2;
            float wv[NU][OBR], pv[NU][NQ];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const bool l2 = c < nb;
                const int g = l2 ? t + 512 * c + 256 * u : t;
                const bool ok = l2 ? g < H : (u == 0 && g < a.IN);
                const float* W = (l2 ? a.prm + a.F.l2_w : a.prm + a.F.in_w) + (size_t)(ok ? g : 0) * H + f0;
                const float* P = (l2 ? a.pl2 : a.pa0) + (size_t)(ok ? g : 0) * NE;
                if constexpr (OBR == 4) {
                    const f32x4 w4 = *(const f32x4*)W;
#pragma unroll
                    for (int r = 0; r < OBR; ++r) wv[u][r] = ok ? round_prec<PREC>(w4[r]) : 0.f;
                } else {
                    const f32x2_t w2 = *(const f32x2_t*)W;
#pragma unroll
                    for (int r = 0; r < OBR; ++r) wv[u][r] = ok ? round_prec<PREC>(w2[r]) : 0.f;
                }
#pragma unroll
                for (int q = 0; q < NQ; ++q) pv[u][q] = (ok && q < NE) ? P[q] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < NU; ++u)
#pragma unroll
                for (int r = 0; r < OBR; ++r)
#pragma unroll
                    for (int q = 0; q < NQ; ++q) x[r * NQP + q] = fmaf(wv[u][r], pv[u][q], x[r * NQP + q]);
        }
    }
    // recursive halving over the 64 lanes: each xor step a lane keeps half of its vector and adds the
    // partner's copy of that half, so 6 steps leave lane l with the sum of value l (63 lane swaps,
    // against 11 dependent DPP / readlane ops per value for a whole-wave sum each)
#pragma unroll
    for (int st = 0; st < 6; ++st) {
        const int m = 32 >> st, half = V >> (st + 1);
        const bool up = (lane & m) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const float send = up ? x[i] : x[i + half];
            const float keep = up ? x[i + half] : x[i];
            x[i] = keep + __shfl_xor(send, m, 64);
        }
    }
    red[w * V + lane] = x[0];   // lane l: value l (the kept halves' offsets sum to l)
    __syncthreads();
    if (valid && t < OBR * NE) {
        const int r = t / NE, q = t % NE, f = f0 + r, v = r * NQP + q;
        if (f < H) {
            const float s = (red[v] + red[V + v]) + (red[2 * V + v] + red[3 * V + v]);
            const float bb = a.prm[a.F.l2_b + f] + a.prm[a.F.in_b + f];
            a.gw[(size_t)f * NE + q] = fmaf(bb, a.gob[q], s);
        }
    }
}
// out_back_n: every thread of the workgroup calls it (it holds a barrier); valid = the group has rows to
// form; red: OB_RED floats of LDS for this 256-thread group

constexpr int OB_RED = 4 * 64;   // floats of LDS per 256-thread group (4 waves x 64 values)

// block b: l2_back's row group b (b < l2_blocks), then the actor's out_back group b (b < ob_groups)
template <int PREC, int NQ>
__global__ __launch_bounds__(256) void l2_back_kernel(L2Back a, int l2_blocks, OutBack ob, int ob_groups) {
    if ((int)blockIdx.x < l2_blocks) l2_back_n<PREC, NQ>(a, (int)blockIdx.x, (int)threadIdx.x);
    if constexpr (NQ > 1) {   // (the critic's N = 1 has no out_back)
        if (ob_groups > 0) {
            __shared__ float red[OB_RED];
            out_back_n<PREC, NQ>(ob, (int)blockIdx.x, (int)blockIdx.x < ob_groups, (int)threadIdx.x, red);
        }
    }
    if (a.zcnt) {   // the critic's row tiles and dW (earlier on this stream) were the counts' last readers
        const int nz = *a.zn;
        for (int r = (int)(blockIdx.x * blockDim.x + threadIdx.x); r < nz; r += (int)(gridDim.x * blockDim.x))
            a.zcnt[a.zlist[r]] = 0u;
    }
}

// One workgroup; every parameter it reads (the TD temb rows of W_in and the time MLP) is staged into
// LDS in one batch of coalesced loads at the start, so the dependent phases below run from LDS and
// the kernel pays global-load latency about twice (staging, then G) instead of once per phase.
// after_stage() runs once every staged parameter is in LDS (the one-launch actor step steps W_in's
// time-embedding rows there: their old values are read, their gradient is the dW's)
// dtemb[q][0..16) = G[q] . W_in[XD + j] for TD = 16, H = 64 NU: one wave per bucket q, its G row
// loaded in one batch, 16 partial dot products per lane, reduced over the lanes by recursive halving
// (lane bits 5..2 pick the value's j, bits 1..0 are summed last)
template <int NU>
__device__ inline void dtemb_rows(const float* g0, const float* win, float* dtemb, int KF, int wave, int lane) {
    constexpr int H = 64 * NU;
    for (int q = wave; q < KF; q += TB_THREADS / 64) {
        const float* g = g0 + q * H + lane;
        float gv[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) gv[u] = g[64 * u];
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            float s = 0.f;
#pragma unroll
            for (int u = 0; u < NU; ++u) s += gv[u] * win[j * H + 64 * u + lane];
            v[j] = s;
        }
#pragma unroll
        for (int lvl = 0; lvl < 4; ++lvl) {
            const int half = 8 >> lvl, o = 32 >> lvl;
            const bool up = (lane & o) != 0;
#pragma unroll
            for (int k = 0; k < half; ++k) {
                const float keep = up ? v[k + half] : v[k], send = up ? v[k] : v[k + half];
                v[k] = keep + __shfl_xor(send, o);
            }
        }
        float t = v[0];
        t += __shfl_xor(t, 2);
        t += __shfl_xor(t, 1);
        const int j = ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
        if ((lane & 3) == 0) dtemb[q * 16 + j] = t;
    }
}

// timing build (-DDPPO_TB_TIMING): shader-clock cycles of each phase of the time-MLP backward as
// thread 0 sees them (barrier waits included), summed over launches (tools/bench_update.py reads them)
#ifdef DPPO_TB_TIMING
__device__ unsigned long long dppo_tb_cycles[8];
#define TBPH_START unsigned long long tb_t_ = __builtin_readcyclecounter()
#define TBPH(k)                                                                   \
    do {                                                                          \
        if (threadIdx.x == 0) {                                                   \
            const unsigned long long now_ = __builtin_readcyclecounter();         \
            atomicAdd(&dppo_tb_cycles[(k)], now_ - tb_t_);                         \
            tb_t_ = now_;                                                         \
        }                                                                         \
    } while (0)
extern "C" DPPO_API int dppo_debug_tb_cycles(unsigned long long* out, int reset) {
    DPPO_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(dppo_tb_cycles), sizeof(unsigned long long) * 8));
    if (reset) {
        unsigned long long z[8] = {};
        DPPO_HIP(hipMemcpyToSymbol(HIP_SYMBOL(dppo_tb_cycles), z, sizeof(z)));
    }
    return DPPO_OK;
}
#else
#define TBPH_START
#define TBPH(k) do {} while (0)
#endif

template <class AfterStage>
__device__ inline void time_bwd_body(const float* __restrict__ gseg, const float* prm, float* grad, const FlatOffsets& F,
                                     int XD, int TD, int H, int KF, int TS, int stage_g, float* sm, AfterStage&& after_stage) {
    float* win = sm;                    // [TD][H]   W_in rows XD .. XD+TD-1
    float* w1 = win + TD * H;           // [TD][2TD]
    float* b1 = w1 + TD * 2 * TD;       // [2TD]
    float* w2 = b1 + 2 * TD;            // [TD][2TD]: time_w2 transposed (da1's reads run along h, conflict-free)
    float* dtemb = w2 + 2 * TD * TD;    // [KF][TD]
    float* e = dtemb + KF * TD;         // [KF][TD]
    float* a1 = e + KF * TD;            // [KF][2TD]
    float* da1 = a1 + KF * 2 * TD;      // [KF][2TD]
    float* ma1 = da1 + KF * 2 * TD;     // [KF][2TD] mish(a1), once per element (time_w2's gradient reads it TD times)
    float* gs = stage_g ? ma1 + KF * 2 * TD : nullptr;   // [KF][H] copy of G when it fits
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    TBPH_START;
    // Staging: every global load of a chunk is issued before its first LDS store, so the phase pays
    // one load latency per chunk (one chunk at hopper's sizes) instead of one per array (separate
    // load-then-store loops waited out four round trips in a row)
    // in_b' = sum_q G[q] (G unstaged): thread n's KF bucket values ride in the staging batch, so the
    // sum pays no round trip of its own (clamped addresses: no branch between the loads)
    constexpr int GQ = 16;
    const bool pre_in = !gs && KF <= GQ && H <= TB_THREADS;
    float gin[GQ];
    {
        constexpr int U = 8;
        const int ng = gs ? KF * H : 0, nw = TD * H, nt = TD * 2 * TD;
        if (pre_in) {
            const int nn = tid < H ? tid : 0;
#pragma unroll
            for (int q = 0; q < GQ; ++q) gin[q] = gseg[(q < KF ? q : 0) * H + nn];
        }
        const float* wsrc = prm + F.in_w + (size_t)XD * H;
        for (int base = 0; base < ng || base < nw || base < nt; base += U * TB_THREADS) {
            float rg[U], rw[U], r1[U], r2[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = base + u * TB_THREADS + tid;
                rg[u] = i < ng ? gseg[i] : 0.f;
                rw[u] = i < nw ? wsrc[i] : 0.f;
                r1[u] = i < nt ? prm[F.time_w1 + i] : 0.f;
                r2[u] = i < nt ? prm[F.time_w2 + i] : 0.f;
            }
            const float rb = base == 0 && tid < 2 * TD ? prm[F.time_b1 + tid] : 0.f;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = base + u * TB_THREADS + tid;
                if (i < ng) gs[i] = rg[u];
                if (i < nw) win[i] = rw[u];
                if (i < nt) { w1[i] = r1[u]; w2[(i % TD) * 2 * TD + i / TD] = r2[u]; }
            }
            if (base == 0 && tid < 2 * TD) b1[tid] = rb;
        }
    }
    TBPH(0);
    const int half = TD / 2;
    const float lnf = logf(10000.f) / (float)(half - 1);
    for (int i = tid; i < KF * TD; i += TB_THREADS) {
        const int q = i / TD, j = i % TD;
        const float f = expf(-(float)(j % half) * lnf) * (float)(q * TS);   // bucket q = row q: t = q * TS
        e[i] = j < half ? sinf(f) : cosf(f);
    }
    if (pre_in) {
        if (tid < H) {
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < GQ; ++q)
                if (q < KF) s += gin[q];
            grad[F.in_b + tid] = s;
        }
    } else if (!gs) {
        for (int n = tid; n < H; n += TB_THREADS) {   // in_b' = sum_q G[q]
            float s = 0.f;
#pragma unroll 8
            for (int q = 0; q < KF; ++q) s += gseg[q * H + n];
            grad[F.in_b + n] = s;
        }
    }
    __syncthreads();
    after_stage();
    TBPH(1);
    if (gs) {   // from the staged copy: no second global round trip
        for (int n = tid; n < H; n += TB_THREADS) {
            float s = 0.f;
#pragma unroll 8
            for (int q = 0; q < KF; ++q) s += gs[q * H + n];
            grad[F.in_b + n] = s;
        }
    }
    // dtemb[q][j] = G[q] . W_in[XD + j], G from LDS when it was staged (gs != nullptr), W_in rows from
    // LDS: for TD = 16 one wave per bucket (dtemb_rows); otherwise one wave per (q, j) — a G load and a
    // whole-wave sum per pair, KF * TD / 16 rounds of both per wave (measured slower at TD = 16:
    // profiles/r05z_time_bwd_phases.txt)
    if (TD == 16 && H == 512) {
        dtemb_rows<8>(gs ? gs : gseg, win, dtemb, KF, wave, lane);
    } else
    for (int i = wave; i < KF * TD; i += TB_THREADS / 64) {
        const int q = i / TD, j = i % TD;
        const float* g = (gs ? gs : gseg) + q * H;
        float s = 0.f;
#pragma unroll 8
        for (int n = lane; n < H; n += 64) s += g[n] * win[j * H + n];
        s = wave_sum(s);
        if (lane == 0) dtemb[i] = s;
    }
    TBPH(2);
    for (int i = tid; i < KF * 2 * TD; i += TB_THREADS) {
        const int q = i / (2 * TD), h = i % (2 * TD);
        float s = b1[h];
        for (int k = 0; k < TD; ++k) s += e[q * TD + k] * w1[k * 2 * TD + h];
        a1[i] = s;
        ma1[i] = mishf(s);
    }
    __syncthreads();
    TBPH(3);
    for (int i = tid; i < KF * 2 * TD; i += TB_THREADS) {
        const int q = i / (2 * TD), h = i % (2 * TD);
        float dm = 0.f;
        for (int j = 0; j < TD; ++j) dm += dtemb[q * TD + j] * w2[j * 2 * TD + h];
        da1[i] = dm * mish_gradf(a1[i]);
    }
    for (int i = tid; i < 2 * TD * TD; i += TB_THREADS) {            // time_w2 [2TD][TD]
        const int h = i / TD, j = i % TD;
        float s = 0.f;
        for (int q = 0; q < KF; ++q) s += ma1[q * 2 * TD + h] * dtemb[q * TD + j];
        grad[F.time_w2 + i] = s;
    }
    for (int j = tid; j < TD; j += TB_THREADS) {
        float s = 0.f;
        for (int q = 0; q < KF; ++q) s += dtemb[q * TD + j];
        grad[F.time_b2 + j] = s;
    }
    __syncthreads();
    TBPH(4);
    for (int i = tid; i < TD * 2 * TD; i += TB_THREADS) {            // time_w1 [TD][2TD]
        const int k = i / (2 * TD), h = i % (2 * TD);
        float s = 0.f;
        for (int q = 0; q < KF; ++q) s += e[q * TD + k] * da1[q * 2 * TD + h];
        grad[F.time_w1 + i] = s;
    }
    for (int h = tid; h < 2 * TD; h += TB_THREADS) {
        float s = 0.f;
        for (int q = 0; q < KF; ++q) s += da1[q * 2 * TD + h];
        grad[F.time_b1 + h] = s;
    }
    TBPH(5);
}

// time_bwd, the actor's l2_back and its out_back in one launch (all follow the actor's dW and are
// independent of each other): workgroup 0 runs the time-MLP backward, the others TB_THREADS / 256 groups
// each, group g l2_back's row group g and then out_back's group g (as many workgroups as the larger
// count needs: extra workgroups waited for CUs beside the other stream's kernels)
template <int PREC, int NQ>
__global__ __launch_bounds__(TB_THREADS) void time_l2_bwd_kernel(const float* __restrict__ gseg,
                                                          const float* __restrict__ prm, float* __restrict__ grad,
                                                          FlatOffsets F, int XD, int TD, int H, int KF, int TS,
                                                          int stage_g, L2Back l2b, int l2_groups, OutBack ob,
                                                          int ob_groups) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    if (blockIdx.x == 0) {
        time_bwd_body(gseg, prm, grad, F, XD, TD, H, KF, TS, stage_g, sm, [] {});
        return;
    }
    constexpr int per = TB_THREADS / 256;
    const int grp = ((int)blockIdx.x - 1) * per + (int)threadIdx.x / 256;
    if (grp < l2_groups) l2_back_n<PREC, NQ>(l2b, grp, (int)threadIdx.x % 256);
    if (ob_groups > 0) out_back_n<PREC, NQ>(ob, grp, grp < ob_groups, (int)threadIdx.x % 256, sm + ((int)threadIdx.x / 256) * OB_RED);
}

// the (precision, width) instantiations of the l2_back / time_l2_bwd kernels
template <int PREC>
static void launch_l2_back_p(int nq, unsigned blocks, hipStream_t s, const L2Back& l2b, int l2g, const OutBack& ob, int obg) {
    switch (nq) {
        case 1: hipLaunchKernelGGL((l2_back_kernel<PREC, 1>), dim3(blocks), dim3(256), 0, s, l2b, l2g, ob, obg); break;
        case 12: hipLaunchKernelGGL((l2_back_kernel<PREC, 12>), dim3(blocks), dim3(256), 0, s, l2b, l2g, ob, obg); break;
        case 24: hipLaunchKernelGGL((l2_back_kernel<PREC, 24>), dim3(blocks), dim3(256), 0, s, l2b, l2g, ob, obg); break;
        default: hipLaunchKernelGGL((l2_back_kernel<PREC, L2B_MAXN>), dim3(blocks), dim3(256), 0, s, l2b, l2g, ob, obg); break;
    }
}
static void launch_l2_back(int prec, unsigned blocks, hipStream_t s, const L2Back& l2b, int l2g, const OutBack& ob, int obg) {
    const int nq = l2_nq(l2b.N);
    if (prec == DPPO_BF16) launch_l2_back_p<DPPO_BF16>(nq, blocks, s, l2b, l2g, ob, obg);
    else if (prec == DPPO_F16) launch_l2_back_p<DPPO_F16>(nq, blocks, s, l2b, l2g, ob, obg);
    else launch_l2_back_p<DPPO_F32>(nq, blocks, s, l2b, l2g, ob, obg);
}
template <int PREC>
static const void* time_l2_bwd_fn_p(int nq) {
    return nq == 12 ? (const void*)time_l2_bwd_kernel<PREC, 12> : nq == 24 ? (const void*)time_l2_bwd_kernel<PREC, 24>
         : (const void*)time_l2_bwd_kernel<PREC, L2B_MAXN>;
}
static const void* time_l2_bwd_fn(int prec, int nq) {
    return prec == DPPO_BF16 ? time_l2_bwd_fn_p<DPPO_BF16>(nq) : prec == DPPO_F16 ? time_l2_bwd_fn_p<DPPO_F16>(nq)
                                                                                : time_l2_bwd_fn_p<DPPO_F32>(nq);
}

// dynamic LDS of time_bwd_body over nb buckets; *stage_g = whether the bucket sums are staged too
static size_t time_bwd_lds(const Dims& D, int nb, int* stage_g) {
    size_t tsm = sizeof(float) * ((size_t)D.TD * D.H + 4 * (size_t)D.TD * D.TD + 2 * D.TD +
                                  (size_t)nb * (2 * D.TD + 3 * 2 * D.TD));
    // the bucket sums are staged only when the workgroup stays small enough to share a CU with the
    // critic's dW (its 101 KiB ring): waiting for a CU cost more than the extra global round trip
    // (staging whenever it fits, the r04 form, measured slower in r05)
    const size_t cap = 56 * 1024;
    *stage_g = tsm + sizeof(float) * (size_t)nb * D.H <= cap;
    if (*stage_g) tsm += sizeof(float) * (size_t)nb * D.H;
    return tsm;
}
// At the update entries' accepted geometries (time_dim <= 32, actor_hidden <= 512, nb <= 64) the
// workgroup needs at most 147,712 B (TD 32, H 512, nb 64; the bucket sums unstaged beyond the 56 KiB
// cap), so nothing accepted is refused here; the check keeps the entries' rule for any wider geometry
int time_bwd_check(const Dims& D, int nb) {
    int stage_g = 0;
    const size_t tsm = time_bwd_lds(D, nb, &stage_g);
    if (tsm > 160 * 1024) return dppo_set_error(DPPO_EUNSUPPORTED, "time_bwd needs %zu B LDS", tsm);
    return DPPO_OK;
}
// after the actor's dW: the time-MLP backward over nb buckets at t = q * TS (the bucket sums in gseg),
// W_out's gradient (out_back) and, unless the l2 gradient stays factored, l2's from pl2, in one launch
int launch_time_bwd(const Dims& D, int precision, const PpoWorkspace& ws, const void* packed_actor,
                    const float* actor_params, float* ga, int nb, int TS, hipStream_t s, bool l2_back, bool plain) {
    const FlatOffsets FA = make_flat_offsets(actor_net(D));
    const float* gseg = ws.gseg;
    const float* pl2 = l2_back ? ws.pl2 : ga + FA.l2_w;   // factored: the dW left pl2 in l2's own region
    const float* pa0 = ws.pa0;
    const MlpLayout L = make_mlp_layout(actor_net(D, precision));
    L2Back l2b = {pl2, ga + FA.out_b, (const uint8_t*)packed_actor + L.off[SEG_W_OUT], ga + FA.l2_w, ga + FA.l2_b, D.H,
                  D.XD, precision, nullptr, nullptr, nullptr};
    DPPO_CHECK(D.XD <= L2B_MAXN, "l2_back: action horizon x dim %d > %d", D.XD, L2B_MAXN);
    DPPO_CHECK(D.IN <= 256 && D.H % 4 == 0, "out_back: in_dim %d > 256", D.IN);
    // (time_bwd forked onto a side stream beside l2_back measured slower: 0.428 vs 0.406 ms per
    // minibatch, same box, tools/r03_ab2.sh; since r04 the two share one launch instead)
    int stage_g = 0;
    const size_t tsm0 = time_bwd_lds(D, nb, &stage_g);
    const size_t tsm = tsm0 > sizeof(float) * OB_RED * (TB_THREADS / 256) ? tsm0 : sizeof(float) * OB_RED * (TB_THREADS / 256);
    DPPO_CHECK(tsm <= 160 * 1024, "time_bwd: LDS staging %zu B exceeds 160 KB", tsm);
    const int per = TB_THREADS / 256;
    // a plain head has neither product: the dW wrote u2^T dy into W_out's own region and l2's stays zero, so
    // the launch is the time-MLP backward's workgroup alone
    const int l2g = l2_back && !plain ? dppo_cdiv(D.H, L2B_ROWS) : 0;
    const int obg = plain ? 0 : dppo_cdiv(D.H, ob_rows(l2_nq(D.XD)));
    const int nq = l2_nq(D.XD);
    const void* fn = time_l2_bwd_fn(precision, nq);
    { const int rc_ = dppo_func_lds(fn, tsm); if (rc_) return rc_; }
    DppoKtScope kt(KT_TIME_BWD, s);
    const OutBack ob = make_out_back(D, precision, actor_params, pl2, pa0, ga);
    const dim3 grid(1 + dppo_cdiv(l2g > obg ? l2g : obg, per));
    int XD = D.XD, TD = D.TD, H = D.H;
    FlatOffsets fa = FA;
    const float* prm = actor_params;
    void* args[] = {(void*)&gseg, (void*)&prm, (void*)&ga, (void*)&fa, (void*)&XD, (void*)&TD, (void*)&H, (void*)&nb,
                    (void*)&TS, (void*)&stage_g, (void*)&l2b, (void*)&l2g, (void*)&ob, (void*)&obg};
    DPPO_HIP(hipLaunchKernel(fn, grid, dim3(TB_THREADS), args, tsm, s));
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

// the critic's l2 weight gradient from cpl2 (N = 1). plain: no row group forms the product (the dW wrote l2's
// gradient; adding the factored one would count it twice), the launch only zeroes the sample counts, and
// without counts (dedup off) there is nothing to launch
int launch_critic_l2_back(const Dims& D, int precision, const PpoWorkspace& ws, const void* packed_critic, float* gc,
                          uint32_t* zcnt, hipStream_t s, bool plain) {
    if (plain && !zcnt) return DPPO_OK;
    const FlatOffsets FC = make_flat_offsets(critic_net(D));
    const MlpLayout L = make_mlp_layout(critic_net(D, precision));
    L2Back l2b = {ws.cpl2, gc + FC.out_b, (const uint8_t*)packed_critic + L.off[SEG_W_OUT], gc + FC.l2_w, gc + FC.l2_b,
                  D.HC, 1, precision, zcnt, ws.crow_n, ws.crow_cnt};
    DppoKtScope kt(KT_L2_BACK, s);
    launch_l2_back(precision, (unsigned)dppo_cdiv(D.HC, L2B_ROWS), s, l2b, plain ? 0 : dppo_cdiv(D.HC, L2B_ROWS), OutBack{}, 0);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}
extern "C" int dppo_materialize_l2(const dppo_dims* d, int precision, const void* packed_actor, float* grads,
                                   void* workspace, int batch_rows, void* stream) {
    Dims D;
    int rc = dppo_check_dims(d, &D);
    if (rc) return rc;
    DPPO_CHECK(dppo_prec_ok(precision), "bad precision %d", precision);
    DPPO_CHECK(packed_actor && grads && workspace && batch_rows > 0, "dppo_materialize_l2: bad arguments");
    // a plain-head image has no l2 layer: its minibatch deferred nothing and the l2 range is already its final zero
    if (dppo_image_attrs(packed_actor).head == DPPO_HEAD_PLAIN) return DPPO_OK;
    hipStream_t s = (hipStream_t)stream;
    const PpoWorkspace ws = make_ppo_workspace(D, precision, batch_rows, (uint8_t*)workspace);
    const FlatOffsets FA = make_flat_offsets(actor_net(D));
    DPPO_HIP(hipMemcpyAsync(ws.pl2, grads + FA.l2_w, sizeof(float) * (size_t)D.H * D.XD, hipMemcpyDeviceToDevice, s));
    const MlpLayout L = make_mlp_layout(actor_net(D, precision));
    L2Back l2b = {ws.pl2, grads + FA.out_b, (const uint8_t*)packed_actor + L.off[SEG_W_OUT], grads + FA.l2_w,
                  grads + FA.l2_b, D.H, D.XD, precision, nullptr, nullptr, nullptr};
    DPPO_CHECK(D.XD <= L2B_MAXN, "l2_back: action horizon x dim %d > %d", D.XD, L2B_MAXN);
    launch_l2_back(precision, (unsigned)dppo_cdiv(D.H, L2B_ROWS), s, l2b, dppo_cdiv(D.H, L2B_ROWS), OutBack{}, 0);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}
