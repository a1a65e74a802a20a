// sampler_split.hip — a9: VPGDiffusion.call (model/diffusion/diffusion_vpg.py:250-339) as a
// register-resident SPLIT kernel: the sampler for <= 512 envs per GPU (bf16 / fp16 at any action width
// with XD + SD <= 64, fp32 at hopper's; every other shape streams the weights, sampler.hip).
//
// Why: the weight-streaming kernel gives each 16-env tile one CU, which must pull the whole 1.1 MB bf16
// actor through its 64 B/clk load path every denoising step (~8 us a step at 64 envs). Here each 16-env
// group is owned by P workgroups (one per CU, "members": P = 2 for 2-byte operands, 8 for fp32) and
// member c keeps 1/P of l1 in its register file for the whole launch (the 1 MB bf16 / 2 MB fp32 l1 of
// one actor: 128 VGPRs of fragments per lane either way). The l2 layer is folded into the out-Dense
// (mlp.py:186-206: the residual block is linear from the l2 product to the out-Dense):
//   eps = W_out^T h1 + M^T relu(h2) + B_OUT2,   M = W_l2 W_out,   B_OUT2 = b_out + W_out^T b_l2
// so the only cross-CU traffic of a denoising step is one exchange of 16 x XD fp32 partial eps between
// the P members, and every member then runs the same fp32 DDPM epilogue on the same sum (fixed member
// order: bit-identical x on all of them).
//
// The exchange is in-launch (MI355X_MICROARCH.md "handoff-1to1"/R2 granules): each member stores its
// partials as 8-byte {tag, value} granules and every wave sweeps its slice of the group's granules with
// agent-scope (sc1, L1-bypassing) loads until every tag matches. Tags carry a per-launch sequence
// number and the step index, so nothing is zeroed between launches; slots alternate by step parity (a
// member can be at most one step ahead of a peer). The wait is bounded (100 ms): a launch that times
// out writes NaN actions and flags bit 31 of *done. Store flavour, chosen per group at run time (never
// assumed from blockIdx):
//   * every member reads its XCD from HW_REG_XCC_ID and announces it (sc1 granule) in the prologue;
//     the members sweep the announcements and agree on the mode;
//   * all on one XCD -> "L2-local": workgroup-scope (sc0) granule stores, which keep the line in that
//     XCD's L2, where the peers' sc1 loads find it (tools/xchg_probe2.hip: P = 2 0.59 us per exchange
//     step). These granules live in a region owned by that XCD alone ([xcc][slot][G][P][NV], fixed
//     stride), so no other XCD's L2 ever holds a copy of those lines;
//   * otherwise -> write-through agent-scope (sc1) stores into the shared region, the
//     placement-independent form.
// Block -> (group, member): members of a group share blockIdx % 8 (one XCD under the observed
// round-robin placement: a speed choice only; correctness does not depend on placement).
// (r06: the r01 8-member kernel with an l2 GEMM and the r03 pair kernel — two tiles per member pair —
// both measured slower than this one, were removed; DESIGN.md §3 keeps their numbers.)
#include <mutex>
#include <type_traits>
#include <stdlib.h>
#include <string.h>
#include "dppo_common.cuh"
#include "dppo_internal.h"
#include "dppo_sampler.h"

// phase timing for tuning builds (-DDPPO_SAMPLER_TIMING): thread 0 of every workgroup adds the
// shader-clock cycles of each phase (0 prologue, 1 actor switch, 2 in-Dense, 3 l1, 4 l2 + out,
// 5 publish + sweep, 6 epilogue); 11-15 split phases 2-5 at the point wave 0 reaches the barrier
// (11 in-Dense, 12 l1, 13 l2 GEMM, 14 out-Dense + partial store, 15 partial sum + publish)
#ifdef DPPO_SAMPLER_TIMING
__device__ unsigned long long dppo_split_cycles[16 + 64 * 8];
// [0, 16): phase sums over all workgroups; [16 + 8 i + k): phase k of step i of workgroup 0 alone
#define XPHASE(k)                                                                 \
    do {                                                                          \
        if (threadIdx.x == 0) {                                                   \
            const unsigned long long now_ = __builtin_readcyclecounter();         \
            atomicAdd(&dppo_split_cycles[(k)], now_ - t_phase_);                  \
            if (blockIdx.x == 0 && t_step_ < 64 && (k) < 8) dppo_split_cycles[16 + 8 * t_step_ + (k)] = now_ - t_phase_; \
            t_phase_ = now_;                                                      \
        }                                                                         \
    } while (0)
#define XPHASE_START unsigned long long t_phase_ = __builtin_readcyclecounter(); int t_step_ = 0
#define XSTEP(i) t_step_ = (i)
// groups that ran the exchange L2-local ([1]) or shared ([0]), summed over launches
__device__ unsigned dppo_split_xmode_groups[2];
extern "C" DPPO_API int dppo_debug_split_xmode(unsigned* out, int reset) {
    DPPO_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(dppo_split_xmode_groups), sizeof(unsigned) * 2));
    if (reset) {
        unsigned z[2] = {};
        DPPO_HIP(hipMemcpyToSymbol(HIP_SYMBOL(dppo_split_xmode_groups), z, sizeof(z)));
    }
    return DPPO_OK;
}
extern "C" DPPO_API int dppo_debug_split_cycles(unsigned long long* out, int reset) {
    DPPO_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(dppo_split_cycles), sizeof(unsigned long long) * (16 + 64 * 8)));
    if (reset) {
        unsigned long long z[16 + 64 * 8] = {};
        DPPO_HIP(hipMemcpyToSymbol(HIP_SYMBOL(dppo_split_cycles), z, sizeof(z)));
    }
    return DPPO_OK;
}
#else
#define XPHASE(k) do {} while (0)
#define XPHASE_START do {} while (0)
#define XSTEP(i) do {} while (0)
#endif

// Host hand-off of a pipelined step: a relaxed poll of go and one system acquire after it matches;
// the launch's device outputs are stored write-through (sc1, store_out), so the final system release
// has no dirty L2 lines to write back.
namespace {

// a store of a kernel output that leaves no dirty line in L2 (write-through; see the hand-off above)
__device__ inline void store_out(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int SPLIT_P = 8;         // the most members per 16-env group (fp32); the exchange regions' stride
constexpr int SPLIT_H = 512;       // actor hidden width the split layout is built for
constexpr int XMAX_NV = 16 * 32;   // granules per member per step at XD <= 32
constexpr int XMAX_G = 32;         // groups per launch (512 envs): 8*P*G/8 = 256 workgroups

constexpr size_t XREGION = (size_t)2 * XMAX_G * SPLIT_P * XMAX_NV;   // granules of one exchange region
// after the 9 exchange regions: the XCD announcements [XMAX_G * SPLIT_P], then the dual-set x
// hand-off [XMAX_G][XMAX_NV]
constexpr size_t XANN = 9 * XREGION;
constexpr size_t XHOFF = XANN + (size_t)XMAX_G * SPLIT_P;
constexpr size_t XTOTAL = XHOFF + (size_t)XMAX_G * XMAX_NV;

struct SplitArgs {
    SampleArgs a;
    uint64_t* xbuf;   // shared (sc1) region [2 slots][G][P][NV], then 8 XCD-owned (sc0) regions of
                      // XREGION granules each, then the XCD announcements [XMAX_G][P]
    uint32_t seq;     // launch sequence number (tag high bits)
    int G;            // 16-env groups
    uint32_t* xfail_host;  // mapped host word: set by a launch whose exchange timed out (lost
                           // co-residency); the next launch on the stream reports it as an error
    int dual;         // P = 4 kernel: the base actor's steps and the fine-tuned actor's steps run on
                      // two member sets, each with its actor resident for the whole launch
};

__device__ inline int xcc_id() {
    int x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x));
    return x;
}



// l1: u1 fragment reads kept in flight ahead of the MFMA chain (1 measured 46.8 us at hopper bf16
// against 47.1-47.9 for 2, 3, 4, 6 and 58.0 for 0; fp32 neutral; profiles/r06l_sampler_l1d_ab.txt)
constexpr int S4_L1D = 1;

// relu as one v_max_i32 on the bits (fmaxf(x, 0) canonicalises its MFMA-produced input first: two
// VALU ops per element); negative values and -0 map to +0, as fmaxf(x, 0) does up to the sign of 0
__device__ inline float relu_f(float x) { return __int_as_float(max(__float_as_int(x), 0)); }
// the block's activation at its two sites (ACT: DPPO_ACT_RELU, DPPO_ACT_MISH or DPPO_ACT_BY_ARG, which follows
// by_arg = the launch's a.act among ELU / GELU / Softplus), in fp32; the caller rounds it where relu's result is
// rounded
template <int ACT>
__device__ inline float act_f(float x, int by_arg) {
    if constexpr (ACT == DPPO_ACT_RELU) return relu_f(x);
    else if constexpr (ACT == DPPO_ACT_BY_ARG) return smooth_act_by_arg(by_arg, x);
    else return smooth_actf<ACT>(x);
}
// LDS_READY(...): an empty asm statement that "uses" its operands: every one of them is loaded
// before it, so their loads issue together and pay one LDS round trip (left alone, hipcc sank each
// read next to its use)

template <int CTRL>
__device__ inline float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}

// ------------------------------------------------------------------------------------------------
// P = 2 (2-byte operands) or 8 (fp32) members per 16-env group. Fewer members mean a
// cheaper exchange (tools/xchg_probe2.hip, sc0 one-XCD granules at 16 envs: P = 2 0.59 us per step, 4
// 0.98, 8 1.55) and less arrival skew, for more l1 MFMAs per wave. Member c
// keeps 1/P of l1 in registers (P = 2: 128 of hopper's 236 VGPRs), written below for P = 4:
//   in-Dense   W_in rows [x ; state] only (K = XD + SD <= 32 KX); the time part b_in + W_in^T
//              t_emb(t) is the pack step's TIN table (dppo_layout.h), the MFMA accumulator's start.
//              The 2-byte one-k-step form (hopper) holds the wave's 4 fragments in 16 VGPRs for the
//              launch (RIN: copied from the wave's LDS image once per actor); KX = 2 and fp32 read
//              them from LDS every step (16 / 32 more VGPRs do not fit beside their second k-step)
//   step head  nothing a step's epilogue reads besides eps depends on that step: schedule row, noise
//              and out bias of step i + 1 (and its TIN start where all K rows are in LDS) are read in
//              step i behind the publish store, under the exchange wait; x of a finishing lane's
//              coordinate is the y it stored itself and stays in a register
//   l1         output columns [128c, 128c+128): wave w owns n-tile w over ALL 512 inputs, so its
//              result is final (b_l1 is the accumulator's start): a = relu(h2), rounded as the
//              reference's l2 input
//   l2 + out   folded (mlp.py:186-206: the residual block is linear from the l2 product to the
//              out-Dense): eps = W_out^T h1 + M^T a + B_OUT2 with M = W_l2 W_out, packed per actor
//              (SEG_FOLD, hi/lo pairs). The member's partial eps is one MFMA per out tile on the l1
//              result straight from registers (its 4 features per lane are the MFMA's k-slots,
//              repeated against M's hi and lo halves), plus its share of the residual term: the
//              in-Dense tiles w*NTI + r*P + c (h1 hi/lo against SEG_ROUT). No l2 GEMM, no l2
//              weights resident, no LDS round trip or barrier between l1 and the exchange.
// so no wave adds a bias or a residual outside an MFMA, and no wave re-sums l1 partials.
// PM = members per group: 2 (the 2-byte default, S4_P: 1/2 of l1 per member, 2 l1 n-tiles per wave,
// a 2-member exchange; possible once l2 is folded away), 4, or 8 (fp32 with SWV = 4: one wave per
// SIMD, one l1 n-tile each; the member sum adds a third DPP level)
template <class Pol, int XQ, int KX, bool INJ, int SWV, int PM, int ACT>
__global__ __launch_bounds__(SWV * 64) void sample_split4_kernel(SplitArgs sa) {
    constexpr int P = PM;
    static_assert(P == 2 || P == 4 || P == 8, "members per group");
    constexpr int NO = (4 * XQ + 15) / 16;
    using AT = typename Pol::AT;
    // TWO: 2-byte operands (bf16 / fp16: the fold and residual as hi/lo pairs in one 16x16x32 MFMA); else
    // fp32 (r06, P = 8 on 4 waves or 4 on 8: the l1 slice is 128 VGPRs of fragments per lane as bf16's at P = 2;
    // 16x16x4 MFMAs, the fold from RT_FOLD and the residual from W_OUT, exact fp32 operands)
    constexpr bool TWO = sizeof(AT) == 2;
    constexpr int KGP = Pol::KG;
    const int by_arg = sa.a.act;           // read by act_f<DPPO_ACT_BY_ARG> only
    auto pack_bf16x2 = [](float lo, float hi) {
        if constexpr (TWO) return Pol::pack2(lo, hi);
        else return 0u;
    };
    constexpr int H = SPLIT_H, KSH = H / KGP;
    constexpr int HS = H / P;              // features per member slice (128)
    constexpr int SW = SWV;                // waves per member: 8 (2 per SIMD) or 4 (1 per SIMD)
    constexpr int NTI = 32 / SW;           // in-Dense n-tiles per wave
    constexpr int NL1 = (HS / 16) / SW;    // l1 n-tiles of the member slice per wave
    constexpr int NR = NTI / P;            // in-Dense tiles per wave whose residual term this member adds
    static_assert(NL1 * SW == HS / 16 && NTI * SW == 32 && NTI % P == 0, "split geometry");
    constexpr int NOC = 16 * NO;
    constexpr int ST = SW * 64;
    constexpr int pad = 16;
    constexpr int ldh = H + pad;           // u1 row stride (2-byte elements)
    constexpr int lda0 = KX * KGP + pad;   // a0 row stride
    constexpr int XD = 4 * XQ;
    constexpr int NV = 16 * XD;            // coordinates of a 16-env eps block
    constexpr int NVW = NV / SW;           // per wave: 2 XD
    constexpr int SL = 64 / P;             // sweep slots per wave (lane = P * slot + member)
    constexpr int KW = (NVW + SL - 1) / SL;  // sweep loads per lane
    static_assert(KW <= P, "the finishing lanes are the members' lanes");
    constexpr int NB = H + NOC;            // per-actor bias floats: b_l1 | B_OUT2
    // TIN rows in LDS: all K (hopper's KX = 1), or a 2-row ring refilled one step ahead by LDS-DMA
    // (KX = 2, walker2d / halfcheetah: the K rows' 40 KB on top of the 2-k-step in-Dense fragments
    // would exceed the CU's 160 KB, split_lds_total)
    constexpr bool TRING = KX == 2 || !TWO;

    const SampleArgs& a = sa.a;
    // dual: set 0 runs the base actor's steps (t >= K'), set 1 the fine-tuned actor's (t < K'), each
    // with its actor resident for the whole launch; set 0 hands x to set 1 once. Without it, one
    // set runs every step and reloads the resident fragments at the switch (~5 us per launch)
    const int per_set = 8 * P * ((sa.G + 7) / 8);
    const int set = sa.dual ? (int)blockIdx.x / per_set : 0;
    const int b = (int)blockIdx.x - set * per_set;
    const int g = (b / (8 * P)) * 8 + b % 8, c = (b / 8) % P;
    if (g >= sa.G) return;                 // whole workgroup: no barrier is skipped
    const int gx = g + set * sa.G, GX = sa.G * (sa.dual ? 2 : 1);   // group index in the exchange regions
    XPHASE_START;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int row0 = g * 16;
    const MlpLayout& L = a.L;
    const int SD = a.SD, K = a.K, KF = a.KF;
    const int KSX = packed_ksteps(XD + SD, KGP);  // k-step stride of the W_XS image
    const int i0 = sa.dual && set == 1 ? K - KF : 0, i1 = sa.dual && set == 0 ? K - KF : K;   // steps of this set

    // ---- LDS carve (SPLIT_LDS_REGIONS, dppo_sampler.h: all offsets multiples of 16 B) ----
    constexpr size_t ESZ = sizeof(AT);
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    size_t o = 0;
#define DPPO_CARVE(T, name, bytes) T* name = (T*)(smem + o); o += bytes;
    SPLIT_LDS_REGIONS(DPPO_CARVE)
#undef DPPO_CARVE
    // TRING: row t of the actor that runs it (fine-tuned below K'), as 2 KB of LDS-DMA by waves 0 and 1
    // (lane l's 16 B at slot + 16 l); waited for by the issuing wave's vmcnt(0) and published by a barrier
    auto tin_dma = [&](int tr, int slot) {
        if (wave < H / 256) {
            const uint8_t* src = (tr < KF ? a.packed_ft : a.packed_base) + L.off[SEG_TIN] + (size_t)tr * H * 4 + 1024 * wave + 16 * lane;
            __builtin_amdgcn_global_load_lds((void*)src, (__attribute__((address_space(3))) void*)(tin + slot * H + 256 * wave), 16, 0, 0);
        }
    };

    // ---- resident weight fragments (one actor at a time): l1 and the folded out-Dense in
    //      registers; the in-Dense fragments in this wave's own LDS (RIN: and from there in registers) ----
    const __amdgpu_buffer_rsrc_t rs_base = packed_rsrc(a.packed_base), rs_ft = packed_rsrc(a.packed_ft);
    auto W = [&](int ft, int seg) { return wsrc(ft ? rs_ft : rs_base, L.off[seg]); };
    u32x4 rl1[NL1][KSH], rfold[NL1][NO], rres[NR][NO];
    // RIN: the 2-byte one-k-step form (hopper) also keeps the current actor's NTI in-Dense fragments in
    // registers (16 VGPRs), copied once from this wave's LDS image after the DMA has landed: in the
    // prologue and after a non-dual actor switch. (KX = 2 spills with 16 more VGPRs; fp32's NTI = 8
    // fragments are 32.)
    constexpr bool RIN = TWO && KX == 1;
    u32x4 rin[RIN ? NTI : 1];
    // LDS-DMA of one 1 KiB fragment (lane l's 16 B land at dst + 16 l); wave-private destinations,
    // consumed only after this wave's vmcnt(0)
    auto dma_frag = [&](int ft, int seg, int KS, int ntile, int ks, u32x4* dst) {
        const uint8_t* src = (ft ? a.packed_ft : a.packed_base) + L.off[seg] + ((size_t)(ntile * KS + ks) << 10) + 16 * lane;
        __builtin_amdgcn_global_load_lds((void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    };
    auto load_in = [&](int ft) {
#pragma unroll
        for (int ks = 0; ks < KX; ++ks)
#pragma unroll
            for (int n = 0; n < NTI; ++n) dma_frag(ft, SEG_W_XS, KSX, NTI * wave + n, ks, wxs + ((wave * NTI + n) * KX + ks) * 64);
    };
    // RIN: this wave's landed in-Dense fragments, LDS -> registers (after the vmcnt(0) that covers load_in)
    auto take_in = [&]() {
        if constexpr (RIN)
#pragma unroll
            for (int n = 0; n < NTI; ++n) rin[n] = wxs[(wave * NTI + n) * KX * 64 + lane];
    };
    auto load_l1 = [&](int ft) {
#pragma unroll
        for (int t = 0; t < NL1; ++t)
#pragma unroll
            for (int j = 0; j < KSH; ++j) rl1[t][j] = load_bfrag_c(W(ft, SEG_W_L1), KSH, (HS / 16) * c + NL1 * wave + t, j, lane);
    };
    auto load_fold = [&](int ft) {
        if constexpr (TWO) {   // FOLD / ROUT: [feature tile][out tile] hi/lo fragments
#pragma unroll
            for (int tt = 0; tt < NL1; ++tt)
#pragma unroll
                for (int n = 0; n < NO; ++n) rfold[tt][n] = load_bfrag_c(W(ft, SEG_FOLD), NO, (HS / 16) * c + NL1 * wave + tt, n, lane);
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int n = 0; n < NO; ++n) rres[r][n] = load_bfrag_c(W(ft, SEG_ROUT), NO, NTI * wave + r * P + c, n, lane);
        } else {               // fp32: M (RT_FOLD) and W_out (W_OUT) as packed [K = H][N = out]: a 16-feature
                               // tile is one k-step
#pragma unroll
            for (int tt = 0; tt < NL1; ++tt)
#pragma unroll
                for (int n = 0; n < NO; ++n) rfold[tt][n] = load_bfrag_c(W(ft, SEG_RT_FOLD), L.ks_h, n, (HS / 16) * c + NL1 * wave + tt, lane);
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int n = 0; n < NO; ++n) rres[r][n] = load_bfrag_c(W(ft, SEG_W_OUT), L.ks_h, n, NTI * wave + r * P + c, lane);
        }
    };

    // announce this member's XCD (sc1 granule, tag = seq << 6: step tags are seq << 6 | i + 1)
    uint64_t* const xann = sa.xbuf + XANN + (size_t)gx * P;
    const uint32_t ann_tag = sa.seq << 6;
    if (tid == 0)
        __hip_atomic_store(xann + c, ((uint64_t)ann_tag << 32) | (uint32_t)xcc_id(), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    const int ft0 = __builtin_amdgcn_readfirstlane(sa.dual ? set : (K - 1 < KF ? 1 : 0));
    load_in(ft0); load_l1(ft0); load_fold(ft0);
    int cur = ft0;

    // ---- prologue: biases, in-Dense time tables, schedule, noise ----
    for (int i4 = tid; i4 < 2 * NB / 4; i4 += ST) {
        const int w = i4 / (NB / 4), j = 4 * (i4 % (NB / 4));
        const uint8_t* PK = w ? a.packed_ft : a.packed_base;
        ((float4*)bias)[i4] = j < H ? *((const float4*)(PK + L.off[SEG_B_L1]) + j / 4)
                                    : *((const float4*)(PK + L.off[SEG_B_OUT2]) + (j - H) / 4);
    }
    // TIN row t of the actor that runs step t (base for t >= K', fine-tuned below)
    if constexpr (TRING) {
        tin_dma(K - 1 - i0, i0 & 1);   // the set's first step; later rows one step ahead
    } else {
        for (int i4 = tid; i4 < K * H / 4; i4 += ST) {
            const int t = 4 * i4 / H;
            ((float4*)tin)[i4] = ((const float4*)((t < KF ? a.packed_ft : a.packed_base) + L.off[SEG_TIN]))[i4];
        }
    }
    // per-step epilogue constants [i][c0 c1 c2 c3 sd]: schedule row t = K-1-i and the noise rule
    // (sampler_noise_std)
    for (int i = tid; i < K; i += ST) {
        const float* sc = a.sched + (K - 1 - i) * DPPO_SCHED_COLS;
        const float sd = sampler_noise_std(a, sc);
        float* e = sch + i * DPPO_SCHED_COLS;
        e[0] = sc[0]; e[1] = sc[1]; e[2] = sc[2]; e[3] = sc[3]; e[4] = sd;
    }
    // the noise / x_T draws: this kernel's own copy of sampler_draw_noise (dppo_sampler.h), kept because
    // calling the helper moved this kernel's register allocation; chain row 0 goes out through store_out
    // from member 0
    const int XG = (XD + 3) / 4;
    for (int it = tid; it < (K + 1) * 16 * XG; it += ST) {
        const int step = it / (16 * XG), r = (it / XG) % 16, gq = it % XG, row = row0 + r;
        float z[4];
        if (step == K && a.x_T) {
#pragma unroll
            for (int k = 0; k < 4; ++k) z[k] = (row < a.E && 4 * gq + k < XD) ? a.x_T[(size_t)row * XD + 4 * gq + k] : 0.f;
        } else if (INJ && step < K) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                z[k] = (row < a.E && 4 * gq + k < XD) ? a.noise[((size_t)step * a.E + row) * XD + 4 * gq + k] : 0.f;
        } else {
            philox_normal4(a.seed, (uint32_t)gq, (uint32_t)(a.env_offset + row), (uint32_t)step, a.call_id, z);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = 4 * gq + k;
            if (q >= XD) break;
            if (step < K) {
                zt[(step * 16 + r) * XD + q] = fminf(fmaxf(z[k], -a.randn_clip), a.randn_clip);
            } else {
                xs[r * XD + q] = z[k];
                if (KF == K && c == 0 && a.chains && row < a.E) store_out(a.chains + ((size_t)row * (KF + 1) + 0) * XD + q, z[k]);
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0): the resident set has landed
    // the group's exchange mode from the members' announcements (bounded like the exchange): every
    // member sees the same P words, so all agree; a timeout selects the placement-independent form
    if (wave == 0) {
        const uint64_t t_end = __builtin_amdgcn_s_memrealtime() + 10000000ull;   // 100 ms
        uint64_t v = ((uint64_t)ann_tag << 32);
        bool ok = false;
        for (;;) {
            if (lane < P) v = __hip_atomic_load(xann + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__all(lane >= P || (uint32_t)(v >> 32) == ann_tag)) { ok = true; break; }
            if (__builtin_amdgcn_s_memrealtime() > t_end) break;
        }
        const int x0 = __builtin_amdgcn_readfirstlane((int)(uint32_t)v);
        const bool one_xcd = ok && __all(lane >= P || (int)(uint32_t)v == x0);
        if (lane == 0) xfail[1] = one_xcd ? 1 + x0 : 0;
#ifdef DPPO_SAMPLER_TIMING
        if (lane == 0 && c == 0) atomicAdd(&dppo_split_xmode_groups[one_xcd ? 1 : 0], 1u);
#endif
    }
    __syncthreads();
    take_in();
    // a0 = [x | state | 0]: everything but the state columns before the observation wait
    constexpr int k1w = KX * KGP;
    for (int idx = tid; idx < 16 * k1w; idx += ST) {
        const int r = idx / k1w, cc = idx % k1w;
        if (cc >= XD && cc < XD + SD) continue;              // state columns: after the wait
        a0[r * lda0 + cc] = Pol::cvt(cc < XD ? xs[r * XD + cc] : 0.f);
    }
    if (tid == 0) *xfail = 0;
    XPHASE(7);
    if (a.cond_tagged) {
        sampler_load_state_tagged<ST>(a, row0, st, c == 0, tid);
        XPHASE(8);
        for (int i = tid; i < 16 * SD; i += ST) {
            const int r = i / SD, cc = i % SD, row = row0 + r;
            a0[r * lda0 + XD + cc] = Pol::cvt(st[i]);
            if (a.cond_out && c == 0 && row < a.E) store_out(a.cond_out + (size_t)row * SD + cc, st[i]);
        }
    } else {
        if (a.go) sampler_wait_go(a, c == 0, tid);
        XPHASE(8);
        for (int i = tid; i < 16 * SD; i += ST) {
            const int r = i / SD, cc = i % SD, row = row0 + r;
            const float v = row < a.E ? a.cond[(size_t)row * SD + cc] : 0.f;
            st[i] = v;
            a0[r * lda0 + XD + cc] = Pol::cvt(v);
            if (a.cond_out && c == 0 && row < a.E) store_out(a.cond_out + (size_t)row * SD + cc, v);
        }
    }
    __syncthreads();
    uint64_t* const xh = sa.xbuf + XHOFF + (size_t)g * XMAX_NV;     // dual: x after the base actor's steps
    const uint32_t htag = (sa.seq << 6) | 63u;
    if (sa.dual && set == 1) {
        // the base set waits for the observation first, so this wait is bounded like that one (4 s)
        // plus margin; a timeout leaves x NaN and is flagged like an exchange failure
        if (tid < NV) {
            const uint64_t t_end = __builtin_amdgcn_s_memrealtime() + 500000000ull;   // 5 s
            uint64_t v;
            bool ok = true;
            for (;;) {
                v = __hip_atomic_load(xh + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((uint32_t)(v >> 32) == htag) break;
                if (__builtin_amdgcn_s_memrealtime() > t_end) { ok = false; break; }
                __builtin_amdgcn_s_sleep(1);
            }
            xs[tid] = ok ? __uint_as_float((uint32_t)v) : __builtin_nanf("");
            if (!ok) {
                *xfail = 1;
                __hip_atomic_store(sa.xfail_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        __syncthreads();
        for (int idx = tid; idx < NV; idx += ST) a0[(idx / XD) * lda0 + idx % XD] = Pol::cvt(xs[idx]);
        __syncthreads();
    }
    // fp32 at KX = 2 (hopper: XD + SD = 23 > 16): the in-Dense's second k-step reads state columns only
    // (XD <= KG), so its product is launch-constant per actor — formed once here (and again after a
    // non-dual actor switch) and added to the TIN row: 4 of the step's 16x16x4 MFMAs per in-Dense tile
    // and one LDS operand round trip fewer. (The 2-byte walker2d / halfcheetah form keeps its second
    // k-step: 16 more VGPRs spill it.)
    constexpr bool SBP = KX == 2 && !TWO;
    static_assert(!SBP || XD <= KGP, "x within the in-Dense's first k-step");
    f32x4 sb[SBP ? NTI : 1];
    auto state_part = [&]() {
        if constexpr (SBP) {
            const u32x4 af1 = lds_afrag<Pol>(a0, lda0, 0, 1, lane);
#pragma unroll
            for (int n = 0; n < NTI; ++n) {
                zero_acc(sb[n]);
                sb[n] = Pol::mma(wxs[((wave * NTI + n) * KX + 1) * 64 + lane], af1, sb[n]);
            }
        }
    };
    state_part();
    const int env = lane & 15, jq = lane >> 4;
    const int xmode = __builtin_amdgcn_readfirstlane(xfail[1]);
    uint64_t* const xregion = sa.xbuf + (size_t)xmode * XREGION;
    // this lane's exchange/epilogue coordinate (launch-constant): lane (slot sl, member m) finishes
    // coordinate sl + SL m of its wave's slice
    const int xm = lane & (P - 1), xsl = lane / P;
    const bool fin = xm < KW && xsl + SL * xm < NVW;
    const int ve = wave * NVW + (fin ? xsl + SL * xm : 0), re = ve / XD, qe = ve % XD;
    // The step head is software-pipelined: what a step's epilogue reads besides the exchanged eps
    // (schedule row, noise, out bias) and, where every TIN row is in LDS (!TRING), the in-Dense
    // accumulator's start depend on nothing the step computes, so step i + 1's are read in step i
    // behind the publish store, under the exchange wait; x of this lane's coordinate is the y the lane
    // itself stored in the step before (fin, ve are launch-constant) and stays in a register.
    constexpr bool TPF = !TRING;            // the accumulator start is prefetched too
    struct Head {
        f32x4 ec;                           // c0 c1 c2 c3
        float esd, ze, be;
        f32x4 h1s[TPF ? NTI : 1];           // TPF: TIN[t] of this wave's in-Dense tiles
    };
    auto read_head = [&](int ii) {          // ii in [i0, i1)
        const int tt = K - 1 - ii;
        const float* bh = bias + (sa.dual ? ft0 : (tt < KF ? 1 : 0)) * NB;
        Head h;
        h.ec = *(const f32x4*)(sch + ii * DPPO_SCHED_COLS);
        h.esd = sch[ii * DPPO_SCHED_COLS + 4];
        h.ze = zt[ii * 16 * XD + ve];
        h.be = bh[H + qe];
        if constexpr (TPF)
#pragma unroll
            for (int n = 0; n < NTI; ++n) h.h1s[n] = *(const f32x4*)(tin + tt * H + 16 * (NTI * wave + n) + 4 * jq);
        return h;
    };
    // the reads of a head issue together, ahead of whatever follows the pin
    auto pin_head = [&](const Head& h) {
        asm volatile("" ::"v"(h.ec), "v"(h.esd), "v"(h.ze), "v"(h.be));
        if constexpr (TPF)
#pragma unroll
            for (int n = 0; n < NTI; ++n) asm volatile("" ::"v"(h.h1s[n]));
    };
    Head hd = {};
    float xe = 0.f;
    if (i0 < i1) {
        hd = read_head(i0);
        xe = xs[ve];                        // x_T, or the base set's x (dual hand-off above)
    }
    XPHASE(0);
    for (int i = i0; i < i1; ++i) {
        XSTEP(i);
        const int t = K - 1 - i;
        const int PK = __builtin_amdgcn_readfirstlane(sa.dual ? cur : (t < KF ? 1 : 0));
        const int PKn = __builtin_amdgcn_readfirstlane(t >= 1 && t - 1 < KF ? 1 : 0);
        const bool pre = !sa.dual && t >= 1 && PKn != PK;   // this step is the last of its actor
        if (PK != cur) {
            __builtin_amdgcn_s_waitcnt(0x0F70);   // the other actor's fragments (load_in / load_l1 / load_fold)
            cur = PK;
            state_part();
            take_in();
        }
        XPHASE(1);
        const float* bb = bias + PK * NB;
        const f32x4 ec = hd.ec;
        const float esd = hd.esd, ze = hd.ze, be = hd.be;
        // ---- in-Dense (transposed): h1 = TIN[t] + W_xs^T [x; state]; no activation (mlp.py:144)
        f32x4 h1[NTI];
        {
            constexpr int KXS = SBP ? 1 : KX;   // k-steps run per step
            u32x4 af[KXS], wf[KXS][NTI];
#pragma unroll
            for (int ks = 0; ks < KXS; ++ks) af[ks] = lds_afrag<Pol>(a0, lda0, 0, ks, lane);
#pragma unroll
            for (int n = 0; n < NTI; ++n) {
                if constexpr (TPF) h1[n] = hd.h1s[n];
                else h1[n] = *(const f32x4*)(tin + (TRING ? (i & 1) : t) * H + 16 * (NTI * wave + n) + 4 * jq);
            }
#pragma unroll
            for (int n = 0; n < NTI; ++n) {
                if constexpr (RIN) wf[0][n] = rin[n];
                else wf[0][n] = wxs[((wave * NTI + n) * KX + 0) * 64 + lane];
            }
            // the in-Dense's LDS operands are left to the compiler's schedule (forced into one round trip,
            // the r02-r05 form, measured 46.8-47.0 against 46.0-46.3 us at hopper bf16 with l1 read-ahead 1:
            // profiles/r06m_sampler_knobs_ab.txt)
            // (2-byte KX = 2: the second k-step's operands are read after the first k-step's MFMAs, which
            // keeps the walker2d form within 256 VGPRs)
            if constexpr (SBP)
#pragma unroll
                for (int n = 0; n < NTI; ++n) h1[n] += sb[n];
#pragma unroll
            for (int n = 0; n < NTI; ++n) h1[n] = Pol::mma(wf[0][n], af[0], h1[n]);
            if constexpr (KXS == 2) {
#pragma unroll
                for (int n = 0; n < NTI; ++n) wf[1][n] = wxs[((wave * NTI + n) * KX + 1) * 64 + lane];
#pragma unroll
                for (int n = 0; n < NTI; ++n) h1[n] = Pol::mma(wf[1][n], af[1], h1[n]);
            }
            if (pre) load_in(PKn);
            if constexpr (TRING)   // the next step's row into the other slot (last read in step i - 1)
                if (i + 1 < i1) tin_dma(t - 1, (i + 1) & 1);
#pragma unroll
            for (int n = 0; n < NTI; ++n) {
                const int f = 16 * (NTI * wave + n) + 4 * jq;
                if constexpr (TWO) {
                    u32x2 pk;
                    pk[0] = pack_bf16x2(act_f<ACT>(h1[n][0], by_arg), act_f<ACT>(h1[n][1], by_arg));
                    pk[1] = pack_bf16x2(act_f<ACT>(h1[n][2], by_arg), act_f<ACT>(h1[n][3], by_arg));
                    *(u32x2*)(u1 + env * ldh + f) = pk;
                } else {
                    *(f32x4*)(u1 + env * ldh + f) = f32x4{act_f<ACT>(h1[n][0], by_arg), act_f<ACT>(h1[n][1], by_arg), act_f<ACT>(h1[n][2], by_arg), act_f<ACT>(h1[n][3], by_arg)};
                }
            }
        }
        // the residual term W_out^T h1 of this member's in-Dense tiles (h1 as a hi/lo pair against
        // ROUT's repeated W_out), issued under the barrier
        f32x4 po[NO];
#pragma unroll
        for (int n = 0; n < NO; ++n) zero_acc(po[n]);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            f32x4 hv = h1[r * P];
#pragma unroll
            for (int q = 1; q < P; ++q)
                if (c == q) hv = h1[r * P + q];
            u32x4 bh;
            if constexpr (TWO) {
                bh[0] = pack_bf16x2(hv[0], hv[1]);
                bh[1] = pack_bf16x2(hv[2], hv[3]);
                bh[2] = pack_bf16x2(hv[0] - Pol::lo2f(bh[0]), hv[1] - Pol::hi2f(bh[0]));
                bh[3] = pack_bf16x2(hv[2] - Pol::lo2f(bh[1]), hv[3] - Pol::hi2f(bh[1]));
            } else {
                bh = __builtin_bit_cast(u32x4, hv);   // h1's 4 features as the k-slots: exact
            }
#pragma unroll
            for (int n = 0; n < NO; ++n) po[n] = Pol::mma(rres[r][n], bh, po[n]);
        }
        XPHASE(11);
        lds_sync();
        XPHASE(2);
        // ---- l1 (transposed): n-tile `wave` of this member's output columns over all 512 inputs,
        //      from b_l1; a = relu(h2) feeds the folded l2 + out-Dense (mlp.py:202-206)
        {
            f32x4 acc[NL1];
#pragma unroll
            for (int tt = 0; tt < NL1; ++tt) acc[tt] = *(const f32x4*)(bb + HS * c + 16 * (NL1 * wave + tt) + 4 * jq);
            u32x4 fb[KSH];
#pragma unroll
            for (int j = 0; j < KSH; ++j) fb[j] = lds_afrag<Pol>(u1, ldh, 0, j, lane);
#pragma unroll
            for (int j = 0; j < KSH; ++j)
#pragma unroll
                for (int tt = 0; tt < NL1; ++tt) acc[tt] = Pol::mma(rl1[tt][j], fb[j], acc[tt]);
            // schedule: the bias and L1D fragment reads first, then one read per MFMA, so L1D reads
            // stay in flight ahead of the chain (left alone, hipcc issued read -> wait -> MFMA)
            constexpr int L1D = S4_L1D, MPC = TWO ? 1 : 4;   // hardware MFMAs per Pol::mma
            __builtin_amdgcn_sched_group_barrier(0x100, L1D + NL1, 0);
#pragma unroll
            for (int j = 0; j < KSH - L1D; ++j) {
                __builtin_amdgcn_sched_group_barrier(0x008, NL1 * MPC, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, NL1 * MPC * L1D, 0);
            if (pre) load_l1(PKn);
            // folded l2 + out-Dense: a = relu(h2) rounded once, its 4 features per lane as k-slots
            // 0-3 and again as 4-7, against M's hi and lo halves
#pragma unroll
            for (int tt = 0; tt < NL1; ++tt) {
                u32x4 ba;
                if constexpr (TWO) {
                    ba[0] = pack_bf16x2(act_f<ACT>(acc[tt][0], by_arg), act_f<ACT>(acc[tt][1], by_arg));
                    ba[1] = pack_bf16x2(act_f<ACT>(acc[tt][2], by_arg), act_f<ACT>(acc[tt][3], by_arg));
                    ba[2] = ba[0];
                    ba[3] = ba[1];
                } else {
                    ba = __builtin_bit_cast(u32x4, f32x4{act_f<ACT>(acc[tt][0], by_arg), act_f<ACT>(acc[tt][1], by_arg), act_f<ACT>(acc[tt][2], by_arg),
                                                         act_f<ACT>(acc[tt][3], by_arg)});
                }
#pragma unroll
                for (int n = 0; n < NO; ++n) po[n] = Pol::mma(rfold[tt][n], ba, po[n]);
            }
            if (pre) load_fold(PKn);
#pragma unroll
            for (int n = 0; n < NO; ++n)
                if (16 * n + 4 * jq < XD) *(f32x4*)(part + wave * NV + env * XD + 16 * n + 4 * jq) = po[n];
        }
        XPHASE(14);
        lds_sync();
        XPHASE(4);
        // ---- exchange + DDPM epilogue (as the P = 8 kernel; lane = P * slot + member, the member
        //      sum is log2 P DPP levels inside the quad)
        {
            const uint32_t tag = (sa.seq << 6) | (uint32_t)(i + 1);
            uint64_t* xb = xregion + ((size_t)((i & 1) * GX + gx) * P) * NV;
            const int vw = wave * NVW;
            if (lane < NVW) {
                float pp[SW];
#pragma unroll
                for (int w = 0; w < SW; ++w) pp[w] = part[w * NV + vw + lane];
                // the wave partials in one round trip
                asm volatile("" ::"v"(pp[0]), "v"(pp[1]), "v"(pp[2]), "v"(pp[3]));
                if constexpr (SW == 8) asm volatile("" ::"v"(pp[SW - 4]), "v"(pp[SW - 3]), "v"(pp[SW - 2]), "v"(pp[SW - 1]));
                float sum = pp[0];
#pragma unroll
                for (int w = 1; w < SW; ++w) sum += pp[w];
                const uint64_t gr = ((uint64_t)tag << 32) | __float_as_uint(sum);
                if (xmode)   // one XCD: the line stays in its L2, where the peers' sc1 loads read it
                    __hip_atomic_store(xb + (size_t)c * NV + vw + lane, gr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else
                    __hip_atomic_store(xb + (size_t)c * NV + vw + lane, gr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            XPHASE(15);
            // the next step's head (the last step re-reads its own: a valid slot, unused)
            const Head hn = read_head(i + 1 < i1 ? i + 1 : i);
            const float c0 = ec[0], c1 = ec[1], c2 = ec[2], c3 = ec[3], sd = esd;
            const int m = xm, sl = xsl;
            const uint64_t* src = xb + (size_t)m * NV + vw;
            const uint64_t t_end = __builtin_amdgcn_s_memrealtime() + 10000000ull;   // 100 ms
            float val[KW];
            bool failed = false;
            uint64_t xa[KW];
            for (;;) {
#pragma unroll
                for (int k = 0; k < KW; ++k) {
                    const int v = sl + SL * k < NVW ? sl + SL * k : NVW - 1;   // clamped lanes re-read a valid granule
                    xa[k] = __hip_atomic_load(src + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                pin_head(hn);   // behind the sweep's first loads: the head's LDS reads delay no poll
                bool ok = true;
#pragma unroll
                for (int k = 0; k < KW; ++k) ok &= (uint32_t)(xa[k] >> 32) == tag;
                if (__all(ok)) break;
                if (__builtin_amdgcn_s_memrealtime() > t_end) {
                    failed = true;
                    if (lane == 0) {
                        *xfail = 1;
                        __hip_atomic_store(sa.xfail_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                    break;
                }
            }
#pragma unroll
            for (int k = 0; k < KW; ++k) val[k] = __uint_as_float((uint32_t)xa[k]);
            // TRING: the next TIN row (issued before the poll's loads, so their vmcnt(0) already covered
            // it) has landed before this wave reaches the step-end barrier
            if constexpr (TRING)
                if (wave < H / 256) __builtin_amdgcn_s_waitcnt(0x0F70);
            XPHASE(5);
            // member sum: xor 1 (then xor 2) inside the quad, then across the two quads of 8 lanes (P = 8);
            // every lane adds the same two partial sums (a + b == b + a), so all P hold the same bits
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                val[k] += dpp_f32<0xB1>(val[k]);     // quad_perm [1,0,3,2]
                if constexpr (P >= 4) val[k] += dpp_f32<0x4E>(val[k]);     // quad_perm [2,3,0,1]
                if constexpr (P == 8) val[k] += dpp_f32<0x141>(val[k]);    // row_half_mirror: lane i <-> 7 - i
            }
            if (fin) {
                float ep = val[0];
#pragma unroll
                for (int k = 1; k < KW; ++k) ep = m == k ? val[k] : ep;
                const int v = ve, r = re, q = qe, row = row0 + r;
                ep += be;
                const float x = xe;
                float y = ddpm_post(c0, c1, c2, c3, sd, x, ep, ze, a.x0_clip);   // (:198-242, :301-320)
                if (a.final_clip > 0.f && i == K - 1) y = fminf(fmaxf(y, -a.final_clip), a.final_clip);
                if (failed) y = __builtin_nanf("");
                xe = y;
                xs[v] = y;
                a0[r * lda0 + q] = Pol::cvt(y);
                if (c == 0 && row < a.E) {
                    if (a.chains && t <= KF) store_out(a.chains + ((size_t)row * (KF + 1) + (KF - t)) * XD + q, y);
                    if (i == K - 1) {
                        store_out(a.actions + (size_t)row * XD + q, y);
                        if (a.actions_tagged)
                            __hip_atomic_store(a.actions_tagged + (size_t)row * XD + q,
                                               ((uint64_t)a.cond_tag << 32) | __float_as_uint(y), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_SYSTEM);
                        else if (a.actions_host) a.actions_host[(size_t)row * XD + q] = y;
                    }
                }
            }
            hd = hn;
        }
        lds_sync();
        XPHASE(6);
    }
    XPHASE(9);
    if (sa.dual && set == 0) {
        // hand x to the fine-tuned set (member 0 of the group: every member holds the same bits)
        if (c == 0 && tid < NV)
            __hip_atomic_store(xh + tid, ((uint64_t)htag << 32) | __float_as_uint(xs[tid]), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        if (c == 0 && tid == 0 && a.done && *xfail)
            __hip_atomic_fetch_or(a.done, 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    if (c == 0 && a.done) {
        __threadfence_system();
        __syncthreads();
        if (tid == 0) {
            if (*xfail) __hip_atomic_fetch_or(a.done, 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_fetch_add(a.done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    XPHASE(10);
}

__global__ void xchg_zero_kernel(uint64_t* p, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        __hip_atomic_store(p + i, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// exchange buffers: one per stream (launches on one stream are ordered, so they can share one).
// A slot is bound to one stream while `live`; dppo_sampler_release_stream unbinds it (the pipe that
// owned the stream is closed), and a new stream takes an unbound slot of its device first. A buffer
// is never freed: a rebound slot keeps its buffer and CONTINUES its launch sequence number, so no
// granule left in it by the previous stream can carry a tag the next launch waits for, and no
// zeroing (or device-wide synchronisation) is needed to hand it over.
struct XchgBuf {
    hipStream_t stream;
    int device;
    int live;
    uint64_t* buf;
    uint32_t seq;
    uint32_t* fail_host;   // mapped pinned word (SplitArgs::xfail_host)
    uint32_t* fail_dev;
};
std::mutex g_xmu;
XchgBuf g_xb[16];
int g_nxb = 0;
int g_cus = 0;

int xchg_for(hipStream_t s, uint64_t** buf, uint32_t* seq, uint32_t** fail_dev) {
    int dev = 0;
    DPPO_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_xmu);
    for (int i = 0; i < g_nxb; ++i)
        if (g_xb[i].live && g_xb[i].stream == s && g_xb[i].device == dev) {
            // an earlier launch on this stream lost its members' co-residency (another tenant took
            // the CUs it waited for) and wrote NaN actions: report it instead of sampling on
            if (__hip_atomic_load(g_xb[i].fail_host, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) {
                __hip_atomic_store(g_xb[i].fail_host, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                return dppo_set_error(DPPO_EHIP, "split sampler: a launch's partial-sum exchange timed out "
                                      "(its workgroups were not all resident at once); its actions are NaN");
            }
            *buf = g_xb[i].buf;
            *seq = g_xb[i].seq = (g_xb[i].seq + 1) & 0x03FFFFFFu;
            *fail_dev = g_xb[i].fail_dev;
            return DPPO_OK;
        }
    int slot = -1;
    for (int i = 0; i < g_nxb && slot < 0; ++i)       // a released slot of this device
        if (!g_xb[i].live && g_xb[i].device == dev) slot = i;
    if (slot < 0 && g_nxb == 16) {
        // every slot is bound to a live stream (a process with more than 16 sampling streams):
        // rebind the slot of a stream with no work pending; only when every such stream is busy,
        // wait for ONE of them (never the whole device: another stream may hold a pipelined launch
        // that waits for an observation the host publishes only after this call returns)
        // (a query that is neither done nor not-ready means the stream no longer exists — its owner
        // destroyed it without dppo_sampler_release_stream: its slot is free, nothing to wait for)
        for (int i = 0; i < 16 && slot < 0; ++i) {
            if (g_xb[i].device != dev) continue;
            const hipError_t q = hipStreamQuery(g_xb[i].stream);
            if (q != hipErrorNotReady) {
                (void)hipGetLastError();
                slot = i;
            }
        }
        if (slot < 0) {
            static int next_evict = 0;
            for (int k = 0; k < 16 && slot < 0; ++k) {
                const int i = (next_evict + k) % 16;
                if (g_xb[i].device == dev) slot = i;
            }
            if (slot < 0) return dppo_set_error(DPPO_EHIP, "split sampler: no exchange buffer slot for this device");
            next_evict = (slot + 1) % 16;
            DPPO_HIP(hipStreamSynchronize(g_xb[slot].stream));
        }
    }
    if (slot >= 0) {                                    // rebind: same buffer, sequence continues
        XchgBuf& x = g_xb[slot];
        __hip_atomic_store(x.fail_host, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        x.stream = s; x.live = 1;
        x.seq = (x.seq + 1) & 0x03FFFFFFu;
        *buf = x.buf;
        *seq = x.seq;
        *fail_dev = x.fail_dev;
        return DPPO_OK;
    }
    slot = g_nxb;
    XchgBuf& x = g_xb[slot];
    const size_t n = XTOTAL;
    DPPO_HIP(hipMalloc((void**)&x.buf, sizeof(uint64_t) * n));
    DPPO_HIP(hipHostMalloc((void**)&x.fail_host, sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
    *x.fail_host = 0;
    DPPO_HIP(hipHostGetDevicePointer((void**)&x.fail_dev, x.fail_host, 0));
    // zeroed with write-through stores: no XCD's L2 is left holding a dirty copy of any line
    hipLaunchKernelGGL(xchg_zero_kernel, dim3(1024), dim3(256), 0, s, x.buf, n);
    DPPO_HIP(hipGetLastError());
    x.stream = s; x.device = dev; x.seq = 1; x.live = 1;
    ++g_nxb;
    *buf = x.buf;
    *seq = x.seq;
    *fail_dev = x.fail_dev;
    return DPPO_OK;
}

}  // namespace

// ABI 10: unbind the exchange buffer of `stream` (its owner is done sampling on it): waits for the
// stream's work, then leaves the buffer to the next new stream of the device
extern "C" DPPO_API int dppo_sampler_release_stream(void* stream) {
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(g_xmu);
    for (int i = 0; i < g_nxb; ++i)
        if (g_xb[i].live && g_xb[i].stream == s) {
            DPPO_HIP(hipStreamSynchronize(s));
            g_xb[i].live = 0;
        }
    return DPPO_OK;
}

namespace {

int device_cus() {
    if (!g_cus) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
            g_cus = n;
    }
    return g_cus;
}

// waves per member of the 2-byte kernel: 8, two per SIMD (4, one wave per SIMD with 512 registers,
// measured 63.7 vs 59.3 us per launch: no second wave to hide its latencies;
// profiles/r05d_sampler_xreg_w4_ab.txt)
constexpr int S4_WAVES = 8;

template <class Pol, int XQ, int KX, bool INJ, int SWV, int PM, int ACT>
int launch_split4_kw(const SplitArgs& sa, hipStream_t s) {
    // the finishing lanes are the members' lanes: a wave's 16 x XD / SWV coordinates in (64 / PM)
    // slots at most PM deep
    constexpr int NVW = 16 * 4 * XQ / SWV, KW = (NVW + 64 / PM - 1) / (64 / PM);
    static_assert(KW <= PM, "the waves of a member do not cover XD");
    auto k = sample_split4_kernel<Pol, XQ, KX, INJ, SWV, PM, ACT>;
    const SampleArgs& a = sa.a;
    const size_t lds = split_lds_total(sizeof(typename Pol::AT), KX, a.XD, a.SD, a.K, SWV);
    if (lds > 160 * 1024) return dppo_set_error(DPPO_EUNSUPPORTED, "split sampler needs %zu B of LDS", lds);
    { const int rc_ = dppo_func_lds((const void*)k, (size_t)lds); if (rc_) return rc_; }
    const int blocks = 8 * PM * ((sa.G + 7) / 8) * (sa.dual ? 2 : 1);
    DppoKtScope kt(KT_SAMPLER, s);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(SWV * 64), lds, s, sa);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

// members per group of the 2-byte kernel: 2 (47.2 us per bench launch against 50.4 at 4;
// profiles/r06m_sampler_knobs_ab.txt)
constexpr int S4_P = 2;
// fp32: P = 8 members of 4 waves (one per SIMD: the 16x16x4 MFMA's 32-cycle issue is the step's bound,
// so halving each SIMD's l1 share pays for the 8-member exchange; P = 4 of 8 waves was the alternative)
constexpr int F32_P = 8, F32_WAVES = 4;

template <class Pol, int XQ, int KX, bool INJ, int ACT>
int launch_split4_k(const SplitArgs& sa, hipStream_t s) {
    return launch_split4_kw<Pol, XQ, KX, INJ, S4_WAVES, S4_P, ACT>(sa, s);
}

}  // namespace

// the split sampler's plan for a shape (SplitPlan, dppo_sampler.h). (r06: the r01 8-member kernel and the
// r03 pair kernel, both measured slower than this one, were removed; walker2d / halfcheetah run it since
// their TIN ring.)
SplitPlan split_plan(int precision, int H, int XD, int SD, int E, int K, int KF) {
    // fp32 (r06): the folded kernel at P = F32_P members (an fp32 l1 eighth on 4 waves is 128 VGPRs of
    // fragments per lane), for the instantiated width XD = 12 (hopper; other fp32 shapes stream
    // the weights, sampler.hip)
    const bool f32 = precision == DPPO_F32;
    if ((!dppo_prec_2b(precision) && !(f32 && XD == 12)) || H != SPLIT_H || XD % 4 != 0 || XD > 32 || K > 62)
        return {0, false, 0, 0};
    const int G = dppo_cdiv(E, 16);
    const int cus = device_cus();
    if (G < 1 || G > XMAX_G) return {0, false, 0, cus};
    const int P = f32 ? F32_P : S4_P;   // members per group
    const int KX = dppo_cdiv(XD + SD, f32 ? 16 : 32);
    // every workgroup of the launch co-resident (one per CU: the register budget)
    if (KX > 2 || split_lds_total(f32 ? 4 : 2, KX, XD, SD, K, f32 ? F32_WAVES : S4_WAVES) > 160 * 1024 ||
        (cus && 8 * P * ((G + 7) / 8) > cus))
        return {0, false, 0, cus};
    // two member sets (one per actor) only while two launches of them still fit side by side (the
    // pipelined rollout keeps the next step's launch resident while this one runs)
    const bool dual = KF > 0 && KF < K && (cus == 0 || 2 * 2 * 8 * P * ((G + 7) / 8) <= cus);
    return {P, dual, 8 * P * ((G + 7) / 8) * (dual ? 2 : 1), cus};
}

namespace {
template <int ACT>
int launch_sample_split_a(const SampleArgs& a, int precision, hipStream_t s) {
    const SplitPlan plan = split_plan(precision, a.H, a.XD, a.SD, a.E, a.K, a.KF);
    const int P = plan.P;
    if (!P) return DPPO_EUNSUPPORTED;
    SplitArgs sa;
    sa.a = a;
    sa.dual = plan.dual ? 1 : 0;
    sa.G = dppo_cdiv(a.E, 16);
    int rc = xchg_for(s, &sa.xbuf, &sa.seq, &sa.xfail_host);
    if (rc) return rc;
    const bool inj = a.noise != nullptr;
    const bool f16 = precision == DPPO_F16;
    if (precision == DPPO_F32) {   // split_plan took XD = 12 only
        if (a.XD != 12 || P != F32_P) return DPPO_EUNSUPPORTED;
        if (a.XD + a.SD > 16)
            return inj ? launch_split4_kw<PolicyF32, 3, 2, true, F32_WAVES, F32_P, ACT>(sa, s)
                       : launch_split4_kw<PolicyF32, 3, 2, false, F32_WAVES, F32_P, ACT>(sa, s);
        return inj ? launch_split4_kw<PolicyF32, 3, 1, true, F32_WAVES, F32_P, ACT>(sa, s)
                   : launch_split4_kw<PolicyF32, 3, 1, false, F32_WAVES, F32_P, ACT>(sa, s);
    }
    const bool kx2 = a.XD + a.SD > 32;
    switch (a.XD / 4) {
#define DPPO_SPLIT4_CASE(xq)                                                                                 \
    case xq:                                                                                                 \
        if (kx2) {                                                                                           \
            if (f16) return inj ? launch_split4_k<PolicyF16, xq, 2, true, ACT>(sa, s) : launch_split4_k<PolicyF16, xq, 2, false, ACT>(sa, s); \
            return inj ? launch_split4_k<PolicyBF16, xq, 2, true, ACT>(sa, s) : launch_split4_k<PolicyBF16, xq, 2, false, ACT>(sa, s); \
        }                                                                                                    \
        if (f16) return inj ? launch_split4_k<PolicyF16, xq, 1, true, ACT>(sa, s) : launch_split4_k<PolicyF16, xq, 1, false, ACT>(sa, s); \
        return inj ? launch_split4_k<PolicyBF16, xq, 1, true, ACT>(sa, s) : launch_split4_k<PolicyBF16, xq, 1, false, ACT>(sa, s);
        DPPO_SPLIT4_CASE(1) DPPO_SPLIT4_CASE(2) DPPO_SPLIT4_CASE(3) DPPO_SPLIT4_CASE(4)
        DPPO_SPLIT4_CASE(5) DPPO_SPLIT4_CASE(6) DPPO_SPLIT4_CASE(7) DPPO_SPLIT4_CASE(8)
#undef DPPO_SPLIT4_CASE
        default: return DPPO_EUNSUPPORTED;
    }
}
}  // namespace

int launch_sample_split(const SampleArgs& a, int precision, int act, hipStream_t s) {
    switch (act) {   // dppo_act_ok's five values: the image registry holds no other
        case DPPO_ACT_RELU: return launch_sample_split_a<DPPO_ACT_RELU>(a, precision, s);
        case DPPO_ACT_MISH: return launch_sample_split_a<DPPO_ACT_MISH>(a, precision, s);
        case DPPO_ACT_ELU: case DPPO_ACT_GELU: case DPPO_ACT_SOFTPLUS:   // one set, which follows a.act
            return launch_sample_split_a<DPPO_ACT_BY_ARG>(a, precision, s);
    }
    return dppo_set_error(DPPO_EINVAL, "dppo_sample: bad activation %d", act);
}
