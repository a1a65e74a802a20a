// sampler.hip — a9: VPGDiffusion.call (model/diffusion/diffusion_vpg.py:250-339), DDPM branch.
//
// One workgroup (8 waves) owns 16 env rows for ALL K denoising steps: rows are independent, so
// the K x 4 dependent GEMMs of a rollout step run without any inter-workgroup synchronisation.
// Per step: a0 = [x, t_emb(t), state] (mlp_diffusion.py:72-86) -> in-Dense -> relu -> l1 -> relu
// -> l2 + h1 (residual, mlp.py:186-206) -> out-Dense = eps; then the fused fp32 DDPM epilogue
// (diffusion_vpg.py:198-243, 301-320). Activations never leave LDS; weights stream from L2.
// The actor used at step t is actor_ft when t < K' else the frozen base actor (diffusion_vpg.py:161-180);
// the reference's always-computed base forward (:161) does not change the result and is skipped.
#include <stdlib.h>
#include "dppo_common.cuh"
#include "dppo_internal.h"
#include "dppo_sampler.h"

// phase timing for tuning builds (-DDPPO_SAMPLER_TIMING): wave 0 of every workgroup adds the
// shader-clock cycles of each phase of every denoising step (barrier waits included)
#ifdef DPPO_SAMPLER_TIMING
__device__ unsigned long long dppo_sampler_cycles[16];
#define SPHASE(k)                                                                 \
    do {                                                                          \
        if (threadIdx.x == 0) {                                                   \
            const unsigned long long now_ = __builtin_readcyclecounter();         \
            atomicAdd(&dppo_sampler_cycles[(k)], now_ - t_phase_);                \
            t_phase_ = now_;                                                      \
        }                                                                         \
    } while (0)
#define SPHASE_START unsigned long long t_phase_ = __builtin_readcyclecounter()
extern "C" DPPO_API int dppo_debug_sampler_cycles(unsigned long long* out, int reset) {
    DPPO_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(dppo_sampler_cycles), sizeof(unsigned long long) * 16));
    if (reset) {
        unsigned long long z[16] = {};
        DPPO_HIP(hipMemcpyToSymbol(HIP_SYMBOL(dppo_sampler_cycles), z, sizeof(z)));
    }
    return DPPO_OK;
}
#else
#define SPHASE(k) do {} while (0)
#define SPHASE_START do {} while (0)
#endif

// ---- the sampler's weight stream with resident fragments ----
// A CU streams its actor's weights from L2 every denoising step, and its vector-memory path
// (64 B/clk) is what bounds the kernel. Fragments that fit in the register file
// beside the working set are loaded once per actor instead ("resident"): the in-layer, the
// out-layer and the first RK k-steps of both hidden layers. Only the rest streams through the
// QD-deep queue. A streamed segment is {W: matrix offset advanced past its resident k-steps,
// KSF: the matrix's k-step count (the n-tile stride), KS: k-steps streamed}.
struct SSeg {
    WSrc W;
    int KSF, KS;
};
struct SNext {
    SSeg s1, s2;   // the two streamed segments after the current one
};
__device__ inline SSeg sseg(WSrc W, int KSF, int k0) { return SSeg{WSrc{W.rsrc, W.off + ((uint32_t)k0 << 10)}, KSF, KSF - k0}; }

template <int KS>
__device__ inline u32x4 sfrag(WSrc W, int KSF, const SNext& nx, int ntile, int j, int lane) {
    if (j < KS) return load_bfrag_c(W, KSF, ntile, j, lane);                 // compile-time branch
    const int j1 = j - KS;
    const bool first = j1 < nx.s1.KS;                                         // wave-uniform
    return first ? load_bfrag_c(nx.s1.W, nx.s1.KSF, ntile, j1, lane)
                 : load_bfrag_c(nx.s2.W, nx.s2.KSF, ntile, j1 - nx.s1.KS, lane);
}

template <int D, int NT>
__device__ inline void squeue_prime(WQueue<D, NT>& Q, const SSeg& s0, const SNext& nx, int ntile0, int lane) {
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int j = d;
            if (j < s0.KS) Q.b[d][n] = load_bfrag_c(s0.W, s0.KSF, ntile0 + n, j, lane);
            else if (j - s0.KS < nx.s1.KS) Q.b[d][n] = load_bfrag_c(nx.s1.W, nx.s1.KSF, ntile0 + n, j - s0.KS, lane);
            else Q.b[d][n] = load_bfrag_c(nx.s2.W, nx.s2.KSF, ntile0 + n, j - s0.KS - nx.s1.KS, lane);
        }
}

// acc = A[16 rows][KSF*KG] x W[:, ntile0*16 ..): k-steps [0, RKL) from the resident fragments
// (computed first: they cover the latency of the queue's first loads after the layer barrier),
// k-steps [RKL, KSF) from the queue, which keeps D k-steps of look-ahead into the next segments.
template <class P, int NT, int KSF, int RKL, int D>
__device__ inline void gemm_res(const typename P::AT* A, int lda, WSrc Ws, const u32x4 (*res)[NT],
                                int ntile0, f32x4 (&acc)[1][NT], int lane, WQueue<D, NT>& Q, const SNext& nx) {
    constexpr int KS = KSF - RKL;
#pragma unroll
    for (int n = 0; n < NT; ++n) zero_acc(acc[0][n]);
#pragma unroll
    for (int ks = 0; ks < RKL; ++ks) {
        const u32x4 a = lds_afrag<P>(A, lda, 0, ks, lane);
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[0][n] = P::mma(a, res[ks][n], acc[0][n]);
    }
#pragma unroll
    for (int j = 0; j < KS; ++j) {
        u32x4 c[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) c[n] = Q.b[0][n];
#pragma unroll
        for (int d = 0; d + 1 < D; ++d)
#pragma unroll
            for (int n = 0; n < NT; ++n) Q.b[d][n] = Q.b[d + 1][n];
#pragma unroll
        for (int n = 0; n < NT; ++n) Q.b[D - 1][n] = sfrag<KS>(Ws, KSF, nx, ntile0 + n, j + D, lane);
        const u32x4 a = lds_afrag<P>(A, lda, 0, RKL + j, lane);
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[0][n] = P::mma(a, c[n], acc[0][n]);
    }
}

// The two geometries the streaming kernel runs (r01 measured five other resident sets, among them
// hidden k-steps kept in LDS and the in- or out-layer resident alone, and two more 16-wave forms: all
// slower, removed; profiles/README.md "Retired build variants"): SW waves per workgroup, each owning
// NT = H/(16*SW) n-tiles of every hidden layer; RK hidden k-steps and (RES) the whole in- and out-layers
// resident in registers; QD k-steps of the rest in flight.
struct StreamGeom { int SW, RK; bool RES; int QD; };
constexpr StreamGeom STREAM_GEOM[2] = {
    {16, 0, false, 3},   // fp32, or H != 512: nothing resident
    {8, 2, true, 3},     // 2-byte operands at H = 512
};
constexpr const StreamGeom& stream_geom(bool two_byte, int H) { return STREAM_GEOM[two_byte && H == 512 ? 1 : 0]; }

// dynamic LDS of the streaming kernel for NO out n-tiles on SW waves
template <class P>
static size_t stream_lds_total(const SampleArgs& a, int NO, int SW) {
    const size_t ESZ = sizeof(typename P::AT);
    const int pad = lds_pad_elems<P>(), H = a.H, ldh = H + pad, lda0 = a.L.ks_in * P::KG + pad;
    const int XD = a.XD, SD = a.SD, TD = a.TD, K = a.K, NOC = 16 * NO;
    size_t o = 0;
#define DPPO_SUM(T, name, bytes) o += bytes;
    STREAM_LDS_REGIONS(DPPO_SUM)
#undef DPPO_SUM
    return o;
}

// the block's activation (ACT: DPPO_ACT_RELU, DPPO_ACT_MISH or DPPO_ACT_BY_ARG, which follows by_arg = the
// launch's a.act among ELU / GELU / Softplus) in fp32, rounded by the caller where relu's result is rounded
template <int ACT>
__device__ inline float stream_act(float x, int by_arg) {
    if constexpr (ACT == DPPO_ACT_RELU) return fmaxf(x, 0.f);
    else if constexpr (ACT == DPPO_ACT_BY_ARG) return smooth_act_by_arg(by_arg, x);
    else return smooth_actf<ACT>(x);
}

template <class P, int NT, int NO, int KSI, bool INJ, int QD, int SW, int RK, bool RES, int ACT, int HEAD>
__global__ __launch_bounds__(SW * 64) void sample_kernel(SampleArgs a) {
    SPHASE_START;
    using AT = typename P::AT;
    constexpr int ST = SW * 64;
    constexpr int KSH = ksh_for<P>(NT, SW);
    constexpr int NOK = KSH / SW;
    constexpr int RKI = RES ? KSI : 0;       // resident in-layer k-steps
    static_assert(RK < KSH, "at least one streamed hidden k-step");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int row0 = blockIdx.x * 16;
    const MlpLayout& L = a.L;
    const int pad = lds_pad_elems<P>();
    const int H = a.H;
    const int ldh = H + pad;
    const int k1w = L.ks_in * P::KG;
    const int lda0 = k1w + pad;
    const int XD = a.XD, SD = a.SD, TD = a.TD, K = a.K, KF = a.KF;
    const int NOC = 16 * NO;

    // ---- LDS carve (STREAM_LDS_REGIONS, dppo_sampler.h: all offsets multiples of 16 B) ----
    constexpr size_t ESZ = sizeof(AT);
    size_t o = 0;
#define DPPO_CARVE(T, name, bytes) T* name = (T*)(smem + o); o += bytes;
    STREAM_LDS_REGIONS(DPPO_CARVE)
#undef DPPO_CARVE

    const int ntile0 = wave * NT;
    const __amdgpu_buffer_rsrc_t rs_base = packed_rsrc(a.packed_base), rs_ft = packed_rsrc(a.packed_ft);
    // actor selection is wave-uniform: keep it scalar (readfirstlane), or hipcc may treat the buffer
    // resource as divergent and wrap every weight load in a waterfall loop
    auto W = [&](int ft, int seg) { return wsrc(ft ? rs_ft : rs_base, L.off[seg]); };
    // the streamed segments of a denoising step: [in (unless resident)], l1[RK..], l2[RK..]
    auto s_in = [&](int ft) { return sseg(W(ft, SEG_W_IN), KSI, 0); };
    auto s_l1 = [&](int ft) { return sseg(W(ft, SEG_W_L1), KSH, RK); };
    auto s_l2 = [&](int ft) { return sseg(W(ft, SEG_W_L2), KSH, RK); };

    // resident fragments of the actor in use (reloaded when the actor changes, once per launch)
    u32x4 r_in[RKI > 0 ? RKI : 1][NT], r_l1[RK > 0 ? RK : 1][NT], r_l2[RK > 0 ? RK : 1][NT];
    ORing<NOK, NO> r_out;
    auto load_resident = [&](int ft) {
#pragma unroll
        for (int k = 0; k < RKI; ++k)
#pragma unroll
            for (int n = 0; n < NT; ++n) r_in[k][n] = load_bfrag_c(W(ft, SEG_W_IN), KSI, ntile0 + n, k, lane);
#pragma unroll
        for (int k = 0; k < RK; ++k)
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                r_l1[k][n] = load_bfrag_c(W(ft, SEG_W_L1), KSH, ntile0 + n, k, lane);
                r_l2[k][n] = load_bfrag_c(W(ft, SEG_W_L2), KSH, ntile0 + n, k, lane);
            }
        if constexpr (RES) out_prefetch<NOK, NO, SW>(r_out, W(ft, SEG_W_OUT), L.ks_h, wave, lane);
    };
    // the weight stream starts with step 0 (t = K-1); its first loads and the resident set go out
    // before anything waits (noise, the host's observation)
    const int ft0 = __builtin_amdgcn_readfirstlane(K - 1 < KF ? 1 : 0);
    WQueue<QD, NT> R;
    if constexpr (RES) squeue_prime(R, s_l1(ft0), SNext{s_l2(ft0), s_l1(ft0)}, ntile0, lane);
    else squeue_prime(R, s_in(ft0), SNext{s_l1(ft0), s_l2(ft0)}, ntile0, lane);
    load_resident(ft0);
    int cur = ft0;

    // ---- prologue: schedule, biases, state, x_T, time-embedding table ----
    // All global loads go out first (16 B per lane), the Philox/Box-Muller noise is computed while
    // they are in flight, then everything lands in LDS: the prologue runs before the host's
    // observation arrives, and in a pipelined rollout it is what the env step has to cover.
    const int NB4 = 2 * (3 * H + NOC) / 4;                  // float4s of both actors' biases
    float4 bv[4];
    auto bias_src = [&](int i4) {
        const int w = i4 / ((3 * H + NOC) / 4), j = 4 * (i4 % ((3 * H + NOC) / 4));
        const uint8_t* PK = w ? a.packed_ft : a.packed_base;
        const int seg = j < H ? SEG_B_IN : (j < 2 * H ? SEG_B_L1 : (j < 3 * H ? SEG_B_L2 : SEG_B_OUT));
        const int jj = j < 3 * H ? j % H : j - 3 * H;
        return (const float4*)(PK + L.off[seg]) + jj / 4;
    };
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (tid + u * ST < NB4) bv[u] = *bias_src(tid + u * ST);
    float tv = 0.f;
    if (tid < K * TD) {
        const int t = tid / TD;
        tv = ((const float*)((t < KF ? a.packed_ft : a.packed_base) + L.off[SEG_TEMB]))[tid];
    }
    float scv = tid < K * DPPO_SCHED_COLS ? a.sched[tid] : 0.f;
    // noise: all K steps' draws up front, slot K is x_T (sampler_draw_noise)
    sampler_draw_noise<INJ, ST>(a, XD, row0, tid, zt, xs, KF == K && a.chains, [](float* p, float v) { *p = v; });
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (tid + u * ST < NB4) ((float4*)bias)[tid + u * ST] = bv[u];
    for (int i4 = tid + 4 * ST; i4 < NB4; i4 += ST) ((float4*)bias)[i4] = *bias_src(i4);
    // time embeddings t_emb(t) (mlp_diffusion.py:40-45) of the actor each step uses, from the
    // table the pack step derived (dppo_layout.h SEG_TEMB)
    if (tid < K * TD) temb[tid] = tv;
    for (int i = tid + ST; i < K * TD; i += ST)
        temb[i] = ((const float*)((i / TD < KF ? a.packed_ft : a.packed_base) + L.off[SEG_TEMB]))[i];
    if (tid < K * DPPO_SCHED_COLS) sch[tid] = scv;
    for (int i = tid + ST; i < K * DPPO_SCHED_COLS; i += ST) sch[i] = a.sched[i];
    // the resident set and the queue's first loads have landed by now; say so with a real wait
    // (not inline asm), or the waitcnt pass carries them into the loop as possibly in flight and
    // drains the queue before their first use in every layer
    __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0)
    // a pre-enqueued step waits here (everything above does not depend on the observation) for
    // the host to publish it; bounded: ~4 s, then the step runs on whatever is in the buffer and
    // flags the timeout in the high bit of *done so the host reports it
    if (a.cond_tagged) {
        sampler_load_state_tagged<ST>(a, row0, st, true, tid);
        for (int i = tid; i < 16 * SD; i += ST) {
            const int row = row0 + i / SD;
            if (a.cond_out && row < a.E) a.cond_out[(size_t)row * SD + i % SD] = st[i];
        }
    } else {
        if (a.go) sampler_wait_go(a, true, tid);
        for (int i = tid; i < 16 * SD; i += ST) {
            const int r = i / SD, c = i % SD, row = row0 + r;
            const float v = row < a.E ? a.cond[(size_t)row * SD + c] : 0.f;
            st[i] = v;
            if (a.cond_out && row < a.E) a.cond_out[(size_t)row * SD + c] = v;
        }
    }
    __syncthreads();
    // a0 = [x, temb(t), state, 0-pad] for step 0 (t = K-1); later steps get x and temb from the
    // DDPM epilogue of the step before, the state part never changes
    for (int idx = tid; idx < 16 * k1w; idx += ST) {
        const int r = idx / k1w, c = idx % k1w;
        float v = 0.f;
        if (c < XD) v = xs[r * XD + c];
        else if (c < XD + TD) v = temb[(K - 1) * TD + c - XD];
        else if (c < a.IN) v = st[r * SD + c - XD - TD];
        a0[r * lda0 + c] = P::cvt(v);
    }
    __syncthreads();

    for (int i = 0; i < K; ++i) {
        SPHASE(0);
        const int t = K - 1 - i;
        const int is_ft = t < KF;
        const int PK = __builtin_amdgcn_readfirstlane(is_ft);
        const int PKn = __builtin_amdgcn_readfirstlane(t - 1 >= 0 ? (t - 1 < KF ? 1 : 0) : is_ft);
        if (PK != cur) {                                    // the actor switch (t = K'-1): once per launch
            load_resident(PK);
            // wait for the reload HERE (a real s_waitcnt the waitcnt pass sees, not inline asm):
            // otherwise the pass treats the resident registers as possibly in flight on every
            // iteration and drains the weight queue before their first use in each layer
            __builtin_amdgcn_s_waitcnt(0x0F70);             // vmcnt(0)
            cur = PK;
        }
        const float* bb = bias + is_ft * (3 * H + NOC);
        ORing<NOK, NO> ob;                                 // out-layer fragments, consumed 3 layers later
        if constexpr (RES) ob = r_out;
        else out_prefetch<NOK, NO, SW>(ob, W(PK, SEG_W_OUT), L.ks_h, wave, lane);
        SPHASE(1);
        // b) in-Dense: h1 = a0 W_in + b_in  (no activation after the input layer, mlp.py:144)
        f32x4 h1[1][NT], acc[1][NT];
        gemm_res<P, NT, KSI, RKI, QD>(a0, lda0, W(PK, SEG_W_IN), r_in, ntile0, h1, lane, R, SNext{s_l1(PK), s_l2(PK)});
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int col = (ntile0 + n) * 16 + ccol(lane);
            const float bv = bb[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                h1[0][n][r] += bv;
                tA[crow(lane, r) * ldh + col] = P::cvt(stream_act<ACT>(h1[0][n][r], a.act));
            }
        }
        lds_sync();
        SPHASE(2);
        // c) l1: act(h1) W_l1 + b -> act -> tB   (pre-activation block, mlp.py:192-193,202-203)
        gemm_res<P, NT, KSH, RK, QD>(tA, ldh, s_l1(PK).W, r_l1, ntile0, acc, lane, R,
                                     RES ? SNext{s_l2(PK), s_l1(PKn)} : SNext{s_l2(PK), s_in(PKn)});
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int col = (ntile0 + n) * 16 + ccol(lane);
            const float bv = bb[H + col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (HEAD == DPPO_HEAD_PLAIN) {
                    // plain head (no l2 layer, no skip): the out-Dense's input is act(h2) itself, kept in the
                    // skip's registers past the l2 product, whose result this instantiation drops
                    h1[0][n][r] = stream_act<ACT>(acc[0][n][r] + bv, a.act);
                    tB[crow(lane, r) * ldh + col] = P::cvt(h1[0][n][r]);
                } else {
                    tB[crow(lane, r) * ldh + col] = P::cvt(stream_act<ACT>(acc[0][n][r] + bv, a.act));
                }
            }
        }
        lds_sync();
        SPHASE(3);
        // d) l2: act(h2) W_l2 + b + h1 (residual, mlp.py:206) -> tA; the stream moves on to the
        //    next denoising step (possibly the other actor)
        gemm_res<P, NT, KSH, RK, QD>(tB, ldh, s_l2(PK).W, r_l2, ntile0, acc, lane, R,
                                     RES ? SNext{s_l1(PKn), s_l2(PKn)} : SNext{s_in(PKn), s_l1(PKn)});
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int col = (ntile0 + n) * 16 + ccol(lane);
            const float bv = bb[2 * H + col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (HEAD == DPPO_HEAD_PLAIN) tA[crow(lane, r) * ldh + col] = P::cvt(h1[0][n][r]);
                else tA[crow(lane, r) * ldh + col] = P::cvt(acc[0][n][r] + bv + h1[0][n][r]);
            }
        }
        lds_sync();
        SPHASE(4);
        // e) out-Dense (N = XD <= 16*NO): k split over the waves, partials through LDS
        {
            f32x4 po[1][NO];
            gemm_narrow_pre<P, 1, NOK, NO, SW>(tA, ldh, ob, po, wave, lane);
#pragma unroll
            for (int n = 0; n < NO; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    part[(wave * 16 + crow(lane, r)) * NOC + n * 16 + ccol(lane)] = po[0][n][r];
        }
        lds_sync();
        SPHASE(5);
        // f) DDPM epilogue, fp32 (diffusion_vpg.py:198-243, 301-320)
        if (tid < 16 * XD) {
            const int r = tid / XD, q = tid % XD, row = row0 + r;
            float eps = bb[3 * H + q];
#pragma unroll
            for (int w = 0; w < SW; ++w) eps += part[(w * 16 + r) * NOC + q];
            const float* sc = sch + t * DPPO_SCHED_COLS;
            const float x = xs[tid];
            const float sd = sampler_noise_std(a, sc);
            float xn = ddpm_post(sc[0], sc[1], sc[2], sc[3], sd, x, eps, zt[i * 16 * XD + tid], a.x0_clip);   // (:198-242, :301-320)
            if (a.final_clip > 0.f && i == K - 1) xn = fminf(fmaxf(xn, -a.final_clip), a.final_clip);
            xs[tid] = xn;
            a0[r * lda0 + q] = P::cvt(xn);                      // next step's input
            if (row < a.E) {
                if (a.chains && t <= KF) a.chains[((size_t)row * (KF + 1) + (KF - t)) * XD + q] = xn;
                if (i == K - 1) {
                    a.actions[(size_t)row * XD + q] = xn;
                    if (a.actions_tagged)   // the action is its own flag: one aligned 8-B store
                        __hip_atomic_store(a.actions_tagged + (size_t)row * XD + q,
                                           ((uint64_t)a.cond_tag << 32) | __float_as_uint(xn), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
                    else if (a.actions_host) a.actions_host[(size_t)row * XD + q] = xn;
                }
            }
        } else if (t > 0) {                                     // the next step's time embedding
            for (int e = tid - 16 * XD; e < 16 * TD; e += ST - 16 * XD) {
                const int r = e / TD, c = e % TD;
                a0[r * lda0 + XD + c] = P::cvt(temb[(t - 1) * TD + c]);
            }
        }
        if constexpr (16 * 16 * NO >= ST) {   // XD = 32 on 8 waves: every thread finished a coordinate, none was spare
            if (16 * XD >= ST && t > 0)
                for (int e = tid; e < 16 * TD; e += ST) {
                    const int r = e / TD, c = e % TD;
                    a0[r * lda0 + XD + c] = P::cvt(temb[(t - 1) * TD + c]);
                }
        }
        lds_sync();
        SPHASE(6);
    }
    if (a.done) {   // publish: every writer's stores reach the system before the counter moves
        __threadfence_system();
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(a.done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// dry (every launcher below): run the instantiation's host checks only and launch nothing. sample_impl
// and dppo_sample_step ask first, so a geometry without an instantiation is refused before anything is
// enqueued (deferred tables, the observation's copy)
template <class P, int NT, int NO, int KSI, bool INJ, int QD, int SW, int RK, bool RES, int ACT, int HEAD>
static int launch_sample_q(const SampleArgs& a, hipStream_t s, bool dry) {
    if (a.L.ks_h != ksh_for<P>(NT, SW) || a.L.ks_in != KSI || a.L.ks_h % SW != 0)
        return dppo_set_error(DPPO_EUNSUPPORTED, "sampler: hidden %d not supported at this precision", a.H);
    const size_t lds = stream_lds_total<P>(a, NO, SW);
    if (lds > 160 * 1024) return dppo_set_error(DPPO_EUNSUPPORTED, "sampler needs %zu B of LDS", lds);
    if (dry) return DPPO_OK;
    auto k = sample_kernel<P, NT, NO, KSI, INJ, QD, SW, RK, RES, ACT, HEAD>;
    { const int rc_ = dppo_func_lds((const void*)k, (size_t)lds); if (rc_) return rc_; }
    DppoKtScope kt(KT_SAMPLER, s);
    hipLaunchKernelGGL(k, dim3(dppo_cdiv(a.E, 16)), dim3(SW * 64), lds, s, a);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

// Sampler selection (DPPO_SAMPLER_CFG, default "x"):
//   "x": the split register-resident kernel (sampler_split.hip) where it applies (2-byte operands,
//        H = 512, <= 512 envs), else the weight-streaming kernel above;
//   "r": the weight-streaming kernel always (STREAM_GEOM).
static char sampler_cfg() {
    static char c = [] {
        const char* e = getenv("DPPO_SAMPLER_CFG");
        return e && e[0] == 'r' ? 'r' : 'x';
    }();
    return c;
}

template <class P, int NT16, int NO, int KSI, bool INJ, int ACT, int HEAD>   // NT16: n-tiles per wave of a 16-wave layout
static int launch_sample_k(const SampleArgs& a, hipStream_t s, bool dry) {
    constexpr StreamGeom g = stream_geom(P::KG == 32, NT16 * 256);
    return launch_sample_q<P, NT16 * 16 / g.SW, NO, KSI, INJ, g.QD, g.SW, g.RK, g.RES, ACT, HEAD>(a, s, dry);
}

template <class P, int NT, int NO, int KSI, int ACT, int HEAD>
static int launch_sample(const SampleArgs& a, hipStream_t s, bool dry) {
    if (a.noise) return launch_sample_k<P, NT, NO, KSI, true, ACT, HEAD>(a, s, dry);
    return launch_sample_k<P, NT, NO, KSI, false, ACT, HEAD>(a, s, dry);
}

template <class P, int ACT, int HEAD>
static int dispatch_sample(const SampleArgs& a, hipStream_t s, bool dry) {
    const int NT = a.H / (16 * 16);   // n-tiles per wave of the 16-wave layout
    const int NO = dppo_cdiv(a.XD, 16);
    const int KSI = a.L.ks_in;
#define DPPO_SAMPLE_CASE(nt, no, ksi) \
    if (NT == nt && NO == no && KSI == ksi) return launch_sample<P, nt, no, ksi, ACT, HEAD>(a, s, dry);
    if constexpr (P::KG == 32) {   // bf16: H = 512 (NT 2)
        DPPO_SAMPLE_CASE(2, 1, 2) DPPO_SAMPLE_CASE(2, 2, 2) DPPO_SAMPLE_CASE(2, 1, 4) DPPO_SAMPLE_CASE(2, 2, 4)
    } else {                       // fp32: H = 512 or 256
        DPPO_SAMPLE_CASE(2, 1, 4) DPPO_SAMPLE_CASE(2, 2, 4) DPPO_SAMPLE_CASE(1, 1, 4) DPPO_SAMPLE_CASE(1, 2, 4)
    }
#undef DPPO_SAMPLE_CASE
    return dppo_set_error(DPPO_EUNSUPPORTED, "sampler: hidden %d / action chunk %d / in-layer k-steps %d not instantiated",
                          a.H, a.XD, KSI);
}

extern "C" int dppo_sampler_stream_bytes(const dppo_dims* d, int precision, int64_t* bytes_per_tile, int* waves) {
    Dims D;
    int rc = dppo_check_dims(d, &D);
    if (rc) return rc;
    DPPO_CHECK(bytes_per_tile, "dppo_sampler_stream_bytes: null output");
    DPPO_CHECK(dppo_prec_ok(precision), "dppo_sampler_stream_bytes: bad precision %d", precision);
    const MlpLayout L = make_mlp_layout(actor_net(D, precision));
    const StreamGeom& g = stream_geom(dppo_prec_2b(precision), D.H);
    const int64_t ntot = D.H / 16, no = dppo_cdiv(D.XD, 16);
    const int64_t in_f = (int64_t)L.ks_in * ntot, out_f = (int64_t)L.ks_h * no;
    const int64_t rio = g.RES ? in_f + out_f : 0;
    const int64_t per_step = in_f + out_f - rio + 2 * (L.ks_h - g.RK) * ntot;
    const int64_t resident = rio + 2 * (int64_t)g.RK * ntot;
    const int actors = (D.KF > 0 && D.KF < D.K) ? 2 : 1;        // the resident set is reloaded at the switch
    *bytes_per_tile = ((int64_t)D.K * per_step + actors * resident) * 1024;
    if (waves) *waves = g.SW;
    return DPPO_OK;
}

template <int ACT, int HEAD>
static int dispatch_stream_a(const SampleArgs& a, int precision, hipStream_t s, bool dry) {
    return precision == DPPO_BF16 ? dispatch_sample<PolicyBF16, ACT, HEAD>(a, s, dry)
         : precision == DPPO_F16  ? dispatch_sample<PolicyF16, ACT, HEAD>(a, s, dry)
                                  : dispatch_sample<PolicyF32, ACT, HEAD>(a, s, dry);
}
// The streaming kernel is instantiated per head: the plain head's two differences (which value rides the
// skip's registers, what the l2 epilogue stores) are compile-time, so the residual instantiations are the
// code they were before the plain head existed
template <int HEAD>
static int dispatch_stream_h(const SampleArgs& a, int precision, int act, hipStream_t s, bool dry) {
    switch (act) {   // dppo_act_ok's five values: the image registry holds no other
        case DPPO_ACT_RELU: return dispatch_stream_a<DPPO_ACT_RELU, HEAD>(a, precision, s, dry);
        case DPPO_ACT_MISH: return dispatch_stream_a<DPPO_ACT_MISH, HEAD>(a, precision, s, dry);
        case DPPO_ACT_ELU: case DPPO_ACT_GELU: case DPPO_ACT_SOFTPLUS:   // one set, which follows a.act
            return dispatch_stream_a<DPPO_ACT_BY_ARG, HEAD>(a, precision, s, dry);
    }
    return dppo_set_error(DPPO_EINVAL, "dppo_sample: bad activation %d", act);
}
static int dispatch_stream(const SampleArgs& a, int precision, int act, int head, hipStream_t s, bool dry) {
    return head == DPPO_HEAD_PLAIN ? dispatch_stream_h<DPPO_HEAD_PLAIN>(a, precision, act, s, dry)
                                   : dispatch_stream_h<DPPO_HEAD_RESIDUAL>(a, precision, act, s, dry);
}

// The network of a sampler launch: its two images' attributes (ReLU / RESIDUAL where none was recorded), which
// must agree: one instantiation runs both actors' steps. Fills a's dimension fields and layout from it
static int sample_net(const Dims& D, int precision, const void* packed_base, const void* packed_ft, SampleArgs& a,
                      int* act, int* head) {
    const ImageAttrs ft = dppo_image_attrs(packed_ft), base = dppo_image_attrs(packed_base);
    DPPO_CHECK(base.act == ft.act, "dppo_sample: the base and the fine-tuned actor images carry different activations");
    DPPO_CHECK(base.head == ft.head, "dppo_sample: the base and the fine-tuned actor images carry different heads");
    *act = a.act = ft.act; *head = ft.head;
    a.XD = D.XD; a.SD = D.SD; a.TD = D.TD; a.H = D.H; a.K = D.K; a.KF = D.KF; a.IN = D.IN;
    a.L = make_mlp_layout(actor_net(D, precision, ft));
    return DPPO_OK;
}

// Does a kernel take the shape (a: sample_net's fields and E)? The split kernel where its plan
// does, else the streaming kernel's instantiation checks (dry); launches and enqueues nothing.
static int sample_supported(const SampleArgs& a, int precision, int act, int head, bool* split) {
    *split = sampler_cfg() == 'x' && split_plan(precision, a.H, a.XD, a.SD, a.E, a.K, a.KF).P > 0;
    return *split ? DPPO_OK : dispatch_stream(a, precision, act, head, nullptr, true);
}

// The one launch path: `a` carries the caller's pointers and scalars (fields it does not use are
// zero); the dimension fields and the layout are filled here, a shape no kernel takes is refused,
// tables an optimizer step deferred are refreshed, and the split kernel or the streaming kernel runs.
// known: the table's record when the entry has read it already (the read-once rule)
static int sample_impl(const dppo_dims* d, int precision, SampleArgs a, void* stream, const SchedParams* known = nullptr) {
    Dims D;
    int rc = dppo_check_dims(d, &D);
    if (rc) return rc;
    DPPO_CHECK(a.E >= 0, "dppo_sample: n_envs < 0");
    DPPO_CHECK(dppo_prec_ok(precision), "dppo_sample: bad precision %d", precision);
    if (a.E == 0) return DPPO_OK;
    DPPO_CHECK(a.packed_base && a.packed_ft && a.sched && (a.cond || a.cond_tagged) && a.actions,
               "dppo_sample: null pointer argument");
    SchedParams sp;
    if (known) sp = *known;
    else if ((rc = dppo_sched_lookup(D, a.sched, "dppo_sample", &sp)) != DPPO_OK) return rc;
    a.x0_clip = sp.clip;
    int act = DPPO_ACT_RELU, head = DPPO_HEAD_RESIDUAL;
    rc = sample_net(D, precision, a.packed_base, a.packed_ft, a, &act, &head);
    if (rc) return rc;
    bool split = false;
    rc = sample_supported(a, precision, act, head, &split);
    if (rc) return rc;
    // tables an optimizer step deferred (DPPO_STEP_DEFER_SAMPLER_TABLES) are re-derived first, on this stream
    rc = dppo_refresh_sampler_tables(a.packed_ft, stream);
    if (rc) return rc;
    rc = dppo_refresh_sampler_tables(a.packed_base, stream);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (split) {
        // The split kernel reaches a plain head through the image alone (FOLD / RT_FOLD = rnd(W_out), ROUT
        // zero). Its fp32 form takes the skip's operand from W_OUT, which a plain image needs as it is: those
        // loads go to the image's T_OUT segment instead, all zero in a plain image and at least as large
        // (nt_h ks_out_t >= nt_out ks_h fragments at XD <= 32)
        SampleArgs as = a;
        if (head == DPPO_HEAD_PLAIN && !dppo_prec_2b(precision)) {
            DPPO_CHECK(packed_matrix_bytes(a.XD, a.H, a.L.KG) >= packed_matrix_bytes(a.H, a.XD, a.L.KG),
                       "dppo_sample: plain head: T_OUT is smaller than the W_OUT loads it stands in for");
            as.L.off[SEG_W_OUT] = as.L.off[SEG_T_OUT];
        }
        rc = launch_sample_split(as, precision, act, s);
        if (rc != DPPO_EUNSUPPORTED) return rc;
    }
    return dispatch_stream(a, precision, act, head, s, false);
}

// the three plan queries: dims checked and the split kernel's plan looked up once ({0, ...} under
// DPPO_SAMPLER_CFG=r)
static int plan_query(const dppo_dims* d, int precision, int n_envs, const void* out, const char* who, SplitPlan* plan) {
    Dims D;
    int rc = dppo_check_dims(d, &D);
    if (rc) return rc;
    DPPO_CHECK(out, "%s: null output", who);
    *plan = sampler_cfg() == 'x' ? split_plan(precision, D.H, D.XD, D.SD, n_envs, D.K, D.KF) : SplitPlan{};
    return DPPO_OK;
}

extern "C" int dppo_sampler_layout(const dppo_dims* d, int precision, int n_envs, int* members) {
    SplitPlan p;
    int rc = plan_query(d, precision, n_envs, members, "dppo_sampler_layout", &p);
    if (rc) return rc;
    *members = p.P * (p.dual ? 2 : 1);
    return DPPO_OK;
}

// The split kernel's members wait on each other inside a launch, so every active workgroup of a
// launch must be resident at once; a second launch in flight (the pipelined rollout's next step)
// must not take the CUs the first one still needs. One workgroup per CU (register budget), the plan's
// workgroups active per launch. The streaming kernel has no inter-workgroup wait.
extern "C" int dppo_sampler_max_in_flight(const dppo_dims* d, int precision, int n_envs, int* launches) {
    SplitPlan p;
    int rc = plan_query(d, precision, n_envs, launches, "dppo_sampler_max_in_flight", &p);
    if (rc) return rc;
    if (p.P == 0) *launches = 8;
    else *launches = p.cus > 0 ? (p.cus / p.blocks > 0 ? p.cus / p.blocks : 1) : 1;
    return DPPO_OK;
}

// plan[4] = kernel (0 weight streaming, 2 folded split; 1 and 3, the removed 8-member and pair
// kernels, are no longer returned), members P per set, member sets, workgroups per launch
extern "C" int dppo_sampler_plan(const dppo_dims* d, int precision, int n_envs, int* plan) {
    SplitPlan p;
    int rc = plan_query(d, precision, n_envs, plan, "dppo_sampler_plan", &p);
    if (rc) return rc;
    plan[0] = p.P ? 2 : 0;
    plan[1] = p.P;
    plan[2] = p.P ? (p.dual ? 2 : 1) : 0;
    plan[3] = p.P ? p.blocks : dppo_cdiv(n_envs, 16);
    return DPPO_OK;
}

extern "C" int dppo_sample(const dppo_dims* d, int precision, const void* packed_base, const void* packed_ft,
                           const float* sched, const float* cond, int n_envs, const float* x_T, const float* noise,
                           uint64_t seed, uint64_t call_id, int env_offset, int deterministic,
                           float min_sampling_std, float randn_clip, float final_clip,
                           float* actions, float* chains, void* stream) {
    return sample_impl(d, precision,
                       {.packed_base = (const uint8_t*)packed_base, .packed_ft = (const uint8_t*)packed_ft, .sched = sched,
                        .cond = cond, .x_T = x_T, .noise = noise, .actions = actions, .chains = chains, .seed = seed,
                        .call_id = (uint32_t)call_id, .E = n_envs, .env_offset = env_offset, .deterministic = deterministic,
                        .min_std = min_sampling_std, .randn_clip = randn_clip, .final_clip = final_clip},
                       stream);
}

// One rollout step's device work in one call (train_ppo_diffusion_agent.py:106-122): the sampler
// reads the observation straight from the mapped pinned buffer (and copies it into its rollout
// slot), writes the actions straight into the mapped pinned action buffer, and the host waits
// for the stream — no copy kernels in the step. Unmapped staging memory falls back to two
// hipMemcpyAsync around the launch.
extern "C" int dppo_sample_step(const dppo_dims* d, int precision, const void* packed_base, const void* packed_ft,
                                const float* sched, const float* cond_host, float* cond, int n_envs, uint64_t seed,
                                uint64_t call_id, int env_offset, int deterministic, float min_sampling_std,
                                float randn_clip, float final_clip, float* actions, float* actions_host,
                                float* chains, int synchronize, void* stream) {
    Dims D;
    int rc = dppo_check_dims(d, &D);
    if (rc) return rc;
    if (n_envs == 0) return DPPO_OK;
    DPPO_CHECK(cond_host && cond && actions && actions_host, "dppo_sample_step: null pointer argument");
    hipStream_t s = (hipStream_t)stream;
    const float* cond_dev_view = (const float*)mapped_ptr(cond_host);
    float* act_dev_view = (float*)mapped_ptr(actions_host);
    if (cond_dev_view && act_dev_view) {
        rc = sample_impl(d, precision,
                         {.packed_base = (const uint8_t*)packed_base, .packed_ft = (const uint8_t*)packed_ft, .sched = sched,
                          .cond = cond_dev_view, .actions = actions, .chains = chains, .cond_out = cond,
                          .actions_host = act_dev_view, .seed = seed, .call_id = (uint32_t)call_id, .E = n_envs,
                          .env_offset = env_offset, .deterministic = deterministic, .min_std = min_sampling_std,
                          .randn_clip = randn_clip, .final_clip = final_clip},
                         stream);
        if (rc) return rc;
    } else {
        // ask before the observation's copy is enqueued: a refused shape leaves cond as it was
        DPPO_CHECK(n_envs > 0, "dppo_sample: n_envs < 0");
        DPPO_CHECK(dppo_prec_ok(precision), "dppo_sample: bad precision %d", precision);
        SampleArgs q = {};
        q.E = n_envs;
        SchedParams sp;
        rc = dppo_sched_lookup(D, sched, "dppo_sample", &sp);   // read once here, handed to sample_impl below
        if (rc) return rc;
        int act = DPPO_ACT_RELU, head = DPPO_HEAD_RESIDUAL;
        rc = sample_net(D, precision, packed_base, packed_ft, q, &act, &head);
        if (rc) return rc;
        bool split = false;
        rc = sample_supported(q, precision, act, head, &split);
        if (rc) return rc;
        DPPO_HIP(hipMemcpyAsync(cond, cond_host, sizeof(float) * (size_t)n_envs * D.SD, hipMemcpyHostToDevice, s));
        rc = sample_impl(d, precision,
                         {.packed_base = (const uint8_t*)packed_base, .packed_ft = (const uint8_t*)packed_ft, .sched = sched,
                          .cond = cond, .actions = actions, .chains = chains, .seed = seed, .call_id = (uint32_t)call_id,
                          .E = n_envs, .env_offset = env_offset, .deterministic = deterministic,
                          .min_std = min_sampling_std, .randn_clip = randn_clip, .final_clip = final_clip},
                         stream, &sp);
        if (rc) return rc;
        DPPO_HIP(hipMemcpyAsync(actions_host, actions, sizeof(float) * (size_t)n_envs * D.XD, hipMemcpyDeviceToHost, s));
    }
    if (synchronize) DPPO_HIP(hipStreamSynchronize(s));
    return DPPO_OK;
}

// ---- pipelined rollout steps (see include/dppo.h) ----
extern "C" int dppo_rollout_enqueue(const dppo_dims* d, int precision, const void* packed_base, const void* packed_ft,
                                    const float* sched, const float* cond_host, float* cond, int n_envs, uint64_t seed,
                                    uint64_t call_id, int env_offset, int deterministic, float min_sampling_std,
                                    float randn_clip, float final_clip, float* actions, float* actions_host,
                                    float* chains, const uint32_t* go, uint32_t go_value, uint32_t* done, void* stream) {
    DPPO_CHECK(cond_host && cond && actions && actions_host && go && done, "dppo_rollout_enqueue: null pointer argument");
    const float* cond_dev = (const float*)mapped_ptr(cond_host);
    float* act_dev = (float*)mapped_ptr(actions_host);
    const uint32_t* go_dev = (const uint32_t*)mapped_ptr(go);
    uint32_t* done_dev = (uint32_t*)mapped_ptr(done);
    DPPO_CHECK(cond_dev && act_dev && go_dev && done_dev,
               "dppo_rollout_enqueue: staging buffers must come from dppo_host_alloc (mapped, coherent)");
    return sample_impl(d, precision,
                       {.packed_base = (const uint8_t*)packed_base, .packed_ft = (const uint8_t*)packed_ft, .sched = sched,
                        .cond = cond_dev, .actions = actions, .chains = chains, .cond_out = cond, .actions_host = act_dev,
                        .go = go_dev, .go_value = go_value, .done = done_dev, .seed = seed, .call_id = (uint32_t)call_id,
                        .E = n_envs, .env_offset = env_offset, .deterministic = deterministic,
                        .min_std = min_sampling_std, .randn_clip = randn_clip, .final_clip = final_clip},
                       stream);
}

extern "C" int dppo_rollout_enqueue_tagged(const dppo_dims* d, int precision, const void* packed_base,
                                           const void* packed_ft, const float* sched, const uint64_t* obs_tagged,
                                           float* cond, int n_envs, uint64_t seed, uint64_t call_id, int env_offset,
                                           int deterministic, float min_sampling_std, float randn_clip,
                                           float final_clip, float* actions, uint64_t* actions_tagged, float* chains,
                                           uint32_t tag, uint32_t* done, void* stream) {
    DPPO_CHECK(obs_tagged && cond && actions && actions_tagged && done,
               "dppo_rollout_enqueue_tagged: null pointer argument");
    DPPO_CHECK(tag != 0, "dppo_rollout_enqueue_tagged: tag 0 is the buffer's initial value");
    const uint64_t* obs_dev = (const uint64_t*)mapped_ptr(obs_tagged);
    uint64_t* act_dev = (uint64_t*)mapped_ptr(actions_tagged);
    uint32_t* done_dev = (uint32_t*)mapped_ptr(done);
    DPPO_CHECK(obs_dev && act_dev && done_dev,
               "dppo_rollout_enqueue_tagged: staging buffers must come from dppo_host_alloc (mapped, coherent)");
    return sample_impl(d, precision,
                       {.packed_base = (const uint8_t*)packed_base, .packed_ft = (const uint8_t*)packed_ft, .sched = sched,
                        .actions = actions, .chains = chains, .cond_out = cond, .actions_tagged = act_dev,
                        .done = done_dev, .cond_tagged = obs_dev, .cond_tag = tag, .seed = seed,
                        .call_id = (uint32_t)call_id, .E = n_envs, .env_offset = env_offset,
                        .deterministic = deterministic, .min_std = min_sampling_std, .randn_clip = randn_clip,
                        .final_clip = final_clip},
                       stream);
}
