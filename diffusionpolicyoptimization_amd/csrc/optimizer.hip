// optimizer.hip — AdamW over the flat fp32 parameters: the plain kernel, the fused one-launch steps
// that also write the packed images, the per-variable gradient-clip norms and the steps that apply
// their scales, and the learnable DDIM eta's step.
#include <limits.h>
#include <math.h>
#include "dppo_update.h"
#include "dppo_packed.cuh"

// ---------------------------------------------------------------------------------------------
// AdamW over a flat fp32 buffer
// ---------------------------------------------------------------------------------------------
// DPPO_STEP_L2_FROM_PL2: the actor's l2 gradient in its factored form (DPPO_PPO_L2_DEFERRED): the
// l2 weight region of g holds pl2 [H][XD]; AdamW forms dW_l2[h][j] = sum_q pl2[h][q] rnd(W_out[j][q])
// and db_l2[j] = sum_q db_out[q] rnd(W_out[j][q]) itself, in l2_back_cols' order of operations
struct L2Virt {
    int on;
    int64_t w_off, b_off, ob_off;   // l2_w, l2_b, out_b offsets in the optimizer range
    int H, XD, prec;
    const uint8_t* wimg;            // the actor image's W_OUT segment (not rewritten before the pack launch)
};
__device__ inline float l2_virtual_grad(const float* __restrict__ g, const L2Virt& vt, int64_t i) {
    const float* pv;
    int j;
    if (i < vt.b_off) {        // weight: row h of pl2
        const int64_t e = i - vt.w_off;
        const int h = (int)(e / vt.H);
        j = (int)(e - (int64_t)h * vt.H);
        pv = g + vt.w_off + (int64_t)h * vt.XD;
    } else {                   // bias: db_out
        j = (int)(i - vt.b_off);
        pv = g + vt.ob_off;
    }
    float sum = 0.f;
    for (int q = 0; q < vt.XD; ++q) sum = fmaf(pv[q], packed_elem(vt.wimg, vt.H, j, q, vt.prec), sum);
    return sum;
}

// dppo_optimizer_step_clip: the per-variable clip scales (dppo_grad_clip_scales) of the step's range.
// end[v] = one past variable v in the range (layout order), INT_MAX past the last variable. A step
// kernel instantiated with a ClipTab as its trailing argument reads each gradient as the rounded fp32
// product g[i] * scales[v]; instantiated without one it is the unclipped kernel, argument for argument.
constexpr int CLIP_MAXV = 26;   // 12 actor + 8 critic + up to 6 layer-norm vectors
struct ClipTab { const float* scales; int end[CLIP_MAXV]; };
__device__ inline int clip_var(const ClipTab& c, int i) {
    int v = 0;
#pragma unroll
    for (int k = 0; k < CLIP_MAXV - 1; ++k) v += i >= c.end[k];
    return v;
}
// g * s rounded to fp32 before AdamW uses it: the empty asm keeps the product out of any fused
// multiply-add with the moment updates (the step then equals a step on pre-multiplied gradients)
__device__ inline float clip_mul(float g, float s) {
    float x = g * s;
    asm("" : "+v"(x));
    return x;
}
__device__ inline float clip_scale_at(const ClipTab& c, int i) { return c.scales[clip_var(c, i)]; }

struct AdamHP { float lr, wd, b1, b2, eps, alpha, bc1, bc2; int mode; };
__device__ inline void adamw_elem(float& pi, float& mi, float& vi, float gi, const AdamHP& h) {
    if (h.mode == DPPO_ADAMW_KERAS) {
        // Keras 3: decoupled decay first (variable -= variable*wd*lr), then Adam with
        // m += (g-m)(1-b1); v += (g^2-v)(1-b2); p -= m*alpha/(sqrt(v)+eps), alpha = lr*sqrt(1-b2^t)/(1-b1^t)
        pi -= pi * h.wd * h.lr;
        mi += (gi - mi) * (1.f - h.b1);
        vi += (gi * gi - vi) * (1.f - h.b2);
        pi -= (mi * h.alpha) / (sqrtf(vi) + h.eps);
    } else {
        pi *= 1.f - h.lr * h.wd;
        mi = h.b1 * mi + (1.f - h.b1) * gi;
        vi = h.b2 * vi + (1.f - h.b2) * gi * gi;
        pi -= h.lr * (mi / h.bc1) / (sqrtf(vi / h.bc2) + h.eps);
    }
}
// the minibatch's metric sums ride along (dppo_optimizer_step): one launch fewer on the
// minibatch's critical path than a separate copy. With a tag, met_out[nmet] receives it after
// the sums (system-scope release), so the host polls host-mapped memory instead of recording
// and waiting on an event (a marker packet on the minibatch chain). Workgroup 0.
__device__ inline void copy_metrics(const double* met, double* met_out, int nmet, uint64_t tag) {
    if ((int)threadIdx.x < nmet) met_out[threadIdx.x] = met[threadIdx.x];
    if (tag) {
        __syncthreads();
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            __hip_atomic_store(reinterpret_cast<uint64_t*>(met_out + nmet), __builtin_bit_cast(uint64_t, (double)tag),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

template <class... C>   // C: nothing, or ClipTab
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, float lr, float wd, float b1, float b2,
                                                    float eps, float alpha, float bc1, float bc2, int mode,
                                                    const double* __restrict__ met, double* __restrict__ met_out, int nmet,
                                                    uint64_t tag, L2Virt vt, C... clip) {
    if (blockIdx.x == 0) copy_metrics(met, met_out, nmet, tag);
    const AdamHP h = {lr, wd, b1, b2, eps, alpha, bc1, bc2, mode};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float pi = p[i], mi = m[i], vi = v[i];
        const bool virt = vt.on && i >= vt.w_off && i < vt.b_off + vt.H;   // [l2_w | l2_b] are adjacent
        float gi = virt ? l2_virtual_grad(g, vt, i) : g[i];
        if constexpr (sizeof...(C) > 0) gi = clip_mul(gi, clip_scale_at(clip..., (int)i));
        adamw_elem(pi, mi, vi, gi, h);
        p[i] = pi; m[i] = mi; v[i] = vi;
    }
}

// ---------------------------------------------------------------------------------------------
// The fused optimizer step (ABI 11, DPPO_STEP_FUSED_PACK and/or DPPO_STEP_CLEAR_GRADS): one launch
// for AdamW + the network's image + the next minibatch's zeroing, which otherwise take three
// launches (adamw_kernel, pack_all_kernel, zero_kernel) on every minibatch's critical path:
//  * each element's thread stores its updated parameter into its slots of the images (the pack's
//    per-element values: the same RNE conversion, FuseJob in dppo_internal.h), and zeroes its
//    gradient after the read (CLEAR_GRADS);
//  * the caller's byte ranges (the next minibatch's metrics and workspace accumulators,
//    dppo_ppo_clear_ranges) are zeroed by the launch's LAST workgroup (per-XCD ticket counters), so
//    no range is cleared before every workgroup has read what it reads — the metric sums copied out
//    included, whichever ranges the caller passes.
// The actor's step is actor_tile_step_kernel below; it adds the W_out elements the virtual l2
// gradient reads; a critic's step is this kernel.
// ---------------------------------------------------------------------------------------------
struct StepFuse {
    int njobs;
    FuseJob j[FUSE_MAXJ];
    int clear_grads;
    void* clr[4];
    uint32_t clr_words[4];
    unsigned* ticket;               // zero between launches (the last workgroup resets it); null: no clears
};

template <class ET, int KG, int EPL>
__device__ inline void fuse_store(const FuseJob& J, int64_t e, float x) {
    if (J.kind == 2) {
        reinterpret_cast<float*>(J.dst)[e] = x;
        return;
    }
    // e < 2^31 (one weight tensor): 32-bit division
    int k, nn;
    if (J.kind == 0) { k = (int)e / J.IN; nn = (int)e - k * J.IN; }
    else { nn = (int)e / J.IK; k = (int)e - nn * J.IK; }
    const size_t slot = ((size_t)(nn >> 4) * J.KS + k / KG) * 64 + (nn & 15) + 16 * ((k % KG) / EPL);
    reinterpret_cast<ET*>(J.dst + slot * 16)[k % EPL] = (ET)x;
}
template <class ET, int KG, int EPL>
__device__ inline void fuse_all(const FuseJob* jobs, int njobs, int64_t i, float x) {
#pragma unroll 1
    for (int q = 0; q < njobs; ++q) {
        const FuseJob& J = jobs[q];
        if (i >= J.lo && i < J.hi) fuse_store<ET, KG, EPL>(J, i - J.lo, x);
    }
}

__device__ inline bool in_range(int64_t i, const int64_t* r) { return i >= r[0] && i < r[1]; }

// true in exactly one workgroup, the last to arrive (thread 0's view broadcast through LDS); the
// counters are per XCD first (blockIdx % 8), so no single address takes more than ~1/8 of the
// atomics, and the last workgroup resets them for the next launch on the stream
__device__ inline bool last_workgroup(unsigned* ticket) {
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned xcd = blockIdx.x & 7, per = (gridDim.x - xcd + 7) / 8;   // blocks counted on this XCD's ticket
        int l = 0;
        if (atomicAdd(ticket + 16 * xcd, 1u) == per - 1) {
            ticket[16 * xcd] = 0u;
            const unsigned nx = gridDim.x < 8 ? gridDim.x : 8;
            l = atomicAdd(ticket + 128, 1u) == nx - 1;
            if (l) ticket[128] = 0u;
        }
        last = l;
    }
    __syncthreads();
    return last != 0;
}
__device__ inline void clear_words(void* const* clr, const uint32_t* words) {
    for (int r = 0; r < 4; ++r)
        for (uint32_t i = threadIdx.x; i < words[r]; i += blockDim.x) reinterpret_cast<uint32_t*>(clr[r])[i] = 0u;
}

// The job loops stay rolled: unrolled they made the kernel ~20k instructions long.
constexpr int FUSE_BLOCKS = 1024;
template <class ET, int KG, int EPL, class... C>
__global__ __launch_bounds__(256) void adamw_fused_kernel(float* __restrict__ p, float* g, float* __restrict__ m,
                                                          float* __restrict__ v, int64_t n, AdamHP h,
                                                          const double* met, double* met_out, int nmet, uint64_t tag,
                                                          StepFuse f, C... clip) {
    if (blockIdx.x == 0) copy_metrics(met, met_out, nmet, tag);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float pi = p[i], mi = m[i], vi = v[i];
        float gi = g[i];
        if constexpr (sizeof...(C) > 0) gi = clip_mul(gi, clip_scale_at(clip..., (int)i));
        adamw_elem(pi, mi, vi, gi, h);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (f.clear_grads) g[i] = 0.f;
        fuse_all<ET, KG, EPL>(f.j, f.njobs, i, pi);
    }
    if (f.ticket && last_workgroup(f.ticket)) clear_words(f.clr, f.clr_words);
}

// ---------------------------------------------------------------------------------------------
// The actor's optimizer step as ONE coalesced launch (r05; the step without the time-MLP backward).
// r05's one-launch actor step stored each element into its image slots one 2-byte value at a time:
// two scattered stores per weight, slower than AdamW + the coalesced pack launch. Here every wave owns
// the elements of ONE 16-byte slot per lane of a weight tensor's packed image — a block of 16 outputs
// x KG inputs — steps them with AdamW, stores the slot (one coalesced 1 KiB wave store) and, through a
// wave-private LDS tile, the 64 slots the block covers in the transposed image; the remaining waves
// step the fp32 tensors (biases, time MLP) one element per lane and copy them into their fp32
// segments. The image bytes are the pack's (same (ET) conversion, zero padding). Under the virtual l2
// gradient (DPPO_STEP_L2_FROM_PL2) the W_out blocks and the zeroing of what the l2 elements read wait
// for the last workgroup; the caller's clear ranges too.
// ---------------------------------------------------------------------------------------------
struct TileMat {
    int64_t off;            // first element in the step's range
    int K, N, KS, KST;      // rows (inputs), columns (outputs), k-steps of the image and of the transposed one
    uint8_t* img;           // packed [K][N] image
    uint8_t* timg;          // packed image of the transpose ([N][K]), or null
    int nb;                 // 16-column blocks
};
struct TileCpy { int64_t lo, n; float* dst; };
constexpr int TILE_MAXM = 4, TILE_MAXC = 8, TILE_THREADS = 256;
struct TileStep {
    int nmat;
    TileMat mat[TILE_MAXM];
    int mstart[TILE_MAXM + 1];      // wave prefix over the mats the main grid steps
    int ncpy;
    TileCpy cpy[TILE_MAXC];
    int64_t cstart[TILE_MAXC + 1];  // element prefix over the copies
    int last_mat;                   // the mat the last workgroup steps (W_out under the virtual l2), or -1
    int64_t keep[2][2];             // read by every l2 element: zeroed by the last workgroup
    int clear_grads;
    void* clr[4];
    uint32_t clr_words[4];
    unsigned* ticket;
};
// CLIP: every gradient of the tensor is read times sc, its variable's clip scale
template <class ET, int KG, int EPL, bool CLIP = false>
__device__ inline void tile_block(float* p, float* g, float* m, float* v, const AdamHP& h, const L2Virt& vt,
                                  const TileStep& a, const TileMat& M, int b, ET* tile, int lane, float sc = 1.f) {
    static_assert(EPL * (int)sizeof(ET) == 16 && 4 * EPL == KG, "one 16-B slot per lane");
    const int nb = b % M.nb, kb = b / M.nb;
    const int n = 16 * nb + (lane & 15), jq = lane >> 4;
    ET val[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int k = KG * kb + EPL * jq + e;
        float x = 0.f;
        if (k < M.K && n < M.N) {
            const int64_t i = M.off + (int64_t)k * M.N + n;
            float pi = p[i], mi = m[i], vi = v[i];
            const bool virt = vt.on && i >= vt.w_off && i < vt.b_off + vt.H;
            float gi = virt ? l2_virtual_grad(g, vt, i) : g[i];
            if constexpr (CLIP) gi = clip_mul(gi, sc);
            if (a.clear_grads && !in_range(i, a.keep[0]) && !in_range(i, a.keep[1])) g[i] = 0.f;
            adamw_elem(pi, mi, vi, gi, h);
            p[i] = pi; m[i] = mi; v[i] = vi;
            x = pi;
        }
        val[e] = (ET)x;
    }
    u32x4 w;
    __builtin_memcpy(&w, val, 16);
    *reinterpret_cast<u32x4*>(M.img + ((((size_t)nb * M.KS + kb) << 6) + lane) * 16) = w;
    if (!M.timg) return;
    // the transposed image: tile[kl][nl] (KG x 16, wave-private) -> lane (kk, grp) reads row
    // kl = 16 (grp / NGRP) + kk, columns EPL ng .. EPL ng + EPL - 1, one T slot
#pragma unroll
    for (int e = 0; e < EPL; ++e) tile[(EPL * jq + e) * 16 + (lane & 15)] = val[e];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    constexpr int NGRP = 16 / EPL;
    const int kk = lane & 15, grp = lane >> 4;
    const int kl = 16 * (grp / NGRP) + kk, ng = grp % NGRP;
    const int k = KG * kb + kl, n0 = 16 * nb + EPL * ng;
    const u32x4 tv = *reinterpret_cast<const u32x4*>(tile + kl * 16 + EPL * ng);
    if (k < 16 * ((M.K + 15) / 16)) {
        const int ntp = k >> 4, ksp = n0 / KG, lanep = kk + 16 * ((n0 % KG) / EPL);
        *reinterpret_cast<u32x4*>(M.timg + ((((size_t)ntp * M.KST + ksp) << 6) + lanep) * 16) = tv;
    }
    __builtin_amdgcn_wave_barrier();   // the tile is rewritten by this wave's next block
}
template <class ET, int KG, int EPL, class... C>
__global__ __launch_bounds__(TILE_THREADS) void actor_tile_step_kernel(float* p, float* g, float* m, float* v, AdamHP h,
                                                                      const double* met, double* met_out, int nmet,
                                                                      uint64_t tag, L2Virt vt, TileStep a, C... clip) {
    constexpr bool CLIP = sizeof...(C) > 0;
    __shared__ __attribute__((aligned(16))) ET tiles[TILE_THREADS / 64][KG * 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0) copy_metrics(met, met_out, nmet, tag);
    const int gw = (int)blockIdx.x * (TILE_THREADS / 64) + wave;
    if (gw < a.mstart[a.nmat]) {
        int mi = 0;
        while (gw >= a.mstart[mi + 1]) ++mi;
        float sc = 1.f;   // a weight tensor is one variable: one scale per block
        if constexpr (CLIP) sc = clip_scale_at(clip..., (int)a.mat[mi].off);
        tile_block<ET, KG, EPL, CLIP>(p, g, m, v, h, vt, a, a.mat[mi], gw - a.mstart[mi], tiles[wave], lane, sc);
    } else {
        const int64_t e = (int64_t)(gw - a.mstart[a.nmat]) * 64 + lane;
        if (e < a.cstart[a.ncpy]) {
            int c = 0;
            while (e >= a.cstart[c + 1]) ++c;
            const int64_t local = e - a.cstart[c], i = a.cpy[c].lo + local;
            float pi = p[i], mi = m[i], vi = v[i];
            const bool virt = vt.on && i >= vt.w_off && i < vt.b_off + vt.H;
            float gi = virt ? l2_virtual_grad(g, vt, i) : g[i];
            if constexpr (CLIP) gi = clip_mul(gi, clip_scale_at(clip..., (int)i));   // the time MLP's copy spans 4 variables
            if (a.clear_grads && !in_range(i, a.keep[0]) && !in_range(i, a.keep[1])) g[i] = 0.f;
            adamw_elem(pi, mi, vi, gi, h);
            p[i] = pi; m[i] = mi; v[i] = vi;
            a.cpy[c].dst[local] = pi;
        }
    }
    if (!a.ticket || !last_workgroup(a.ticket)) return;
    if (a.last_mat >= 0) {
        const TileMat& M = a.mat[a.last_mat];
        const int nblk = M.nb * M.KS;
        // (the virtual l2 gradient's W_out pass: never with a clip, dppo_optimizer_step_clip refuses the pair)
        for (int b = wave; b < nblk; b += TILE_THREADS / 64) tile_block<ET, KG, EPL>(p, g, m, v, h, vt, a, M, b, tiles[wave], lane);
        __syncthreads();   // every W_out slot read by an l2 element was read before the ticket
    }
    if (a.clear_grads)
        for (int r = 0; r < 2; ++r)
            for (int64_t i = a.keep[r][0] + threadIdx.x; i < a.keep[r][1]; i += TILE_THREADS) g[i] = 0.f;
    clear_words(a.clr, a.clr_words);
}

// per (device, stream): the fused steps' zeroed ticket counter block (launches on one stream are
// ordered, so they share it; the critic's step on the side stream has its own)
static int step_ticket(hipStream_t s, unsigned** out) {
    // 8 per-XCD counters 64 B apart, the total at 512 B
    return stream_scratch(s, SCRATCH_TICKET, 1024, (void**)out);
}

// the step's hyperparameters with AdamW's bias corrections: fp64 pow, alpha rounded to float once
static AdamHP make_adam_hp(int64_t step, float lr, float weight_decay, float beta1, float beta2, float eps, int mode) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    return AdamHP{lr, weight_decay, beta1, beta2, eps, (float)((double)lr * sqrt(bc2) / bc1), (float)bc1, (float)bc2, mode};
}

// the metrics copy and tag every step kernel's workgroup 0 carries (copy_metrics)
static int check_metrics_copy(const double* met, const double* met_out, int nmet, uint64_t tag) {
    DPPO_CHECK(nmet >= 0 && nmet <= 256 && (nmet == 0 || (met && met_out)), "dppo_optimizer_step: bad metrics copy");
    DPPO_CHECK(tag == 0 || (met_out && tag < ((uint64_t)1 << 53)), "dppo_optimizer_step: a tag needs metrics_out and < 2^53");
    return DPPO_OK;
}

// f(ElemFmt) with the image element format of a precision: <__bf16, 32, 8>, <_Float16, 32, 8> or <float, 16, 4>
template <class T, int KG_, int EPL_> struct ElemFmt {
    using ET = T;
    static constexpr int KG = KG_, EPL = EPL_;
};
template <class F>
static void with_elem_fmt(int precision, F&& f) {
    if (precision == DPPO_BF16) f(ElemFmt<__bf16, 32, 8>{});
    else if (precision == DPPO_F16) f(ElemFmt<_Float16, 32, 8>{});
    else f(ElemFmt<float, 16, 4>{});
}

struct AdamwArgs {
    float* params; const float* grads; float* m; float* v;
    int64_t n, step;
    float lr, weight_decay, beta1, beta2, eps;
    int mode;
};
static int launch_adamw(const AdamwArgs& a, const double* met, double* met_out, int nmet, uint64_t tag, hipStream_t s,
                        const L2Virt& vt = L2Virt{}, const ClipTab* clip = nullptr) {
    DPPO_CHECK(a.n >= 0 && a.step >= 1, "dppo_adamw: n < 0 or step < 1");
    DPPO_CHECK(a.mode == DPPO_ADAMW_KERAS || a.mode == DPPO_ADAMW_TORCH, "dppo_adamw: bad mode");
    { const int rc_ = check_metrics_copy(met, met_out, nmet, tag); if (rc_) return rc_; }
    if (a.n == 0 && nmet == 0 && tag == 0) return DPPO_OK;
    DPPO_CHECK(a.n == 0 || (a.params && a.grads && a.m && a.v), "dppo_adamw: null pointer");
    const AdamHP h = make_adam_hp(a.step, a.lr, a.weight_decay, a.beta1, a.beta2, a.eps, a.mode);
    const int64_t blocks64 = (a.n + 255) / 256;
    const unsigned blocks = (unsigned)(blocks64 < 1 ? 1 : (blocks64 < 4096 ? blocks64 : 4096));
    DppoKtScope kt(KT_ADAMW, s);
    if (clip)
        hipLaunchKernelGGL((adamw_kernel<ClipTab>), dim3(blocks), dim3(256), 0, s, a.params, a.grads, a.m, a.v, a.n, h.lr,
                           h.wd, h.b1, h.b2, h.eps, h.alpha, h.bc1, h.bc2, h.mode, met, met_out, nmet, tag, vt, *clip);
    else
        hipLaunchKernelGGL((adamw_kernel<>), dim3(blocks), dim3(256), 0, s, a.params, a.grads, a.m, a.v, a.n, h.lr, h.wd,
                           h.b1, h.b2, h.eps, h.alpha, h.bc1, h.bc2, h.mode, met, met_out, nmet, tag, vt);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

extern "C" int dppo_adamw(float* params, const float* grads, float* m, float* v, int64_t n, int64_t step, float lr,
                          float weight_decay, float beta1, float beta2, float eps, int mode, void* stream) {
    return launch_adamw(AdamwArgs{params, grads, m, v, n, step, lr, weight_decay, beta1, beta2, eps, mode}, nullptr,
                        nullptr, 0, 0, (hipStream_t)stream);
}

// dppo_optimizer_step{,_ex}'s arguments (include/dppo.h), in their order
struct StepArgs {
    const dppo_dims* d;
    int precision;
    AdamwArgs w;
    const float* actor_params; void* packed_actor;
    const float* critic_params; void* packed_critic;
    const double* metrics; double* metrics_out; int n_metrics; uint64_t metrics_tag;
    void* const* clear_ptrs; const size_t* clear_bytes; int n_clear;
    void* stream;
    const float* clip_scales; int nets;   // dppo_optimizer_step_clip's (nets = 0: no clip)
};
// what the validated prologue derives from them
struct StepCtx {
    Dims D;
    hipStream_t s;
    double* mout;          // metrics_out's device address
    int mode;              // the AdamW mode, the DPPO_STEP_* flags taken out
    bool defer, l2v, fuse, clear_g;
    // the two networks: their images' attributes, read here once (a clipped critic range without an image: told by
    // its length); FC.count_all is the critic's parameters with their tail
    NetSpec anet, cnet;
    NetOffsets FA, FC;
    L2Virt vt;
    bool clipped;
    ClipTab clip;
};

// The variables of the chosen networks (DPPO_NET_*) in layout order: end[v] = one past variable v,
// counted from the start of the range; returns their number (12 actor, 8 critic + the vectors of a
// layer-normed critic's tail, each a variable of `hidden` elements)
static int net_var_ends(const FlatOffsets& FA, const NetOffsets& FC, int hidden, int nets, int64_t* end) {
    int nv = 0;
    int64_t base = 0;
    if (nets & DPPO_NET_ACTOR) {
        const size_t e[12] = {FA.time_b1, FA.time_w2, FA.time_b2, FA.in_w, FA.in_b, FA.l1_w,
                              FA.l1_b,    FA.l2_w,    FA.l2_b,    FA.out_w, FA.out_b, FA.count};
        for (size_t x : e) end[nv++] = (int64_t)x;
        base = (int64_t)FA.count;
    }
    if (nets & DPPO_NET_CRITIC) {
        const size_t e[8] = {FC.in_b, FC.l1_w, FC.l1_b, FC.l2_w, FC.l2_b, FC.out_w, FC.out_b, FC.count};
        for (size_t x : e) end[nv++] = base + (int64_t)x;
        for (size_t e = FC.ln + hidden; e <= FC.count_all; e += hidden) end[nv++] = base + (int64_t)e;
    }
    return nv;
}

static int step_prologue(const StepArgs& a, StepCtx& c) {
    int rc = dppo_check_dims(a.d, &c.D);
    if (rc) return rc;
    const Dims& D = c.D;
    DPPO_CHECK(dppo_prec_ok(a.precision), "bad precision %d", a.precision);
    DPPO_CHECK(!a.packed_actor == !a.actor_params && !a.packed_critic == !a.critic_params,
               "dppo_optimizer_step: a packed image needs its parameters");
    DPPO_CHECK(a.n_clear >= 0 && a.n_clear <= 4 && (a.n_clear == 0 || (a.clear_ptrs && a.clear_bytes)),
               "dppo_optimizer_step_ex: at most 4 clear ranges");
    for (int r = 0; r < a.n_clear; ++r)
        DPPO_CHECK(a.clear_ptrs[r] && ((uintptr_t)a.clear_ptrs[r] & 3) == 0 && a.clear_bytes[r] % 4 == 0 &&
                   a.clear_bytes[r] / 4 < ((size_t)1 << 32), "dppo_optimizer_step_ex: clear range %d must be 4-B aligned", r);
    c.s = (hipStream_t)a.stream;
    // metrics_out may be mapped host memory (dppo_host_alloc): the kernel stores through its
    // device address
    c.mout = a.metrics_out;
    if (c.mout) {
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, a.metrics_out, 0) == hipSuccess && dp) c.mout = (double*)dp;
        else (void)hipGetLastError();
    }
    c.defer = (a.w.mode & DPPO_STEP_DEFER_SAMPLER_TABLES) != 0;
    c.l2v = (a.w.mode & DPPO_STEP_L2_FROM_PL2) != 0;
    c.fuse = (a.w.mode & DPPO_STEP_FUSED_PACK) != 0;
    c.clear_g = (a.w.mode & DPPO_STEP_CLEAR_GRADS) != 0;
    c.mode = a.w.mode & ~(DPPO_STEP_DEFER_SAMPLER_TABLES | DPPO_STEP_L2_FROM_PL2 | DPPO_STEP_FUSED_PACK | DPPO_STEP_CLEAR_GRADS);
    const auto ln_critic = [&](int head) { return critic_net(D, a.precision, ImageAttrs{DPPO_ACT_RELU, head, DPPO_LN_ON}); };
    c.anet = actor_net(D, a.precision, a.packed_actor ? dppo_image_attrs(a.packed_actor) : ImageAttrs());
    c.cnet = critic_net(D, a.precision, a.packed_critic ? dppo_image_attrs(a.packed_critic) : ImageAttrs());
    c.FA = make_flat_offsets(c.anet);
    // The critic's layout follows its image's attributes. A clipped critic range without an image is told by its
    // length (the three layouts differ in it)
    if (!a.packed_critic && a.nets >= 1 && a.nets <= 3 && (a.nets & DPPO_NET_CRITIC)) {
        const int64_t ncritic = a.w.n - ((a.nets & DPPO_NET_ACTOR) ? (int64_t)c.FA.count : 0);
        for (int head : {DPPO_HEAD_RESIDUAL, DPPO_HEAD_PLAIN})
            if (ncritic == (int64_t)make_flat_offsets(ln_critic(head)).count_all) c.cnet = ln_critic(head);
    }
    c.FC = make_flat_offsets(c.cnet);
    if (a.packed_critic && a.critic_params && a.w.params && a.critic_params >= a.w.params &&
        a.critic_params < a.w.params + a.w.n) {
        // the range holds the critic from critic_params on: it must hold the layout of the image's attributes
        const int64_t room = a.w.n - (int64_t)(a.critic_params - a.w.params);
        DPPO_CHECK(c.cnet.ln_sites() == 0 || room >= (int64_t)c.FC.count_all,
                   "dppo_optimizer_step: the critic image is layer-normed (%zu parameters with its gamma / beta tail), the "
                   "range holds %lld from critic_params on: buffers sized for the layout without the tail", c.FC.count_all,
                   (long long)room);
        if (c.cnet.ln_sites() == 0 && !a.packed_actor && a.critic_params == a.w.params)
            for (int head : {DPPO_HEAD_RESIDUAL, DPPO_HEAD_PLAIN})
                DPPO_CHECK(a.w.n != (int64_t)make_flat_offsets(ln_critic(head)).count_all,
                           "dppo_optimizer_step: the range is a layer-normed critic's (%lld parameters), the critic image has "
                           "no layer norm (dppo_pack_critic_ln)", (long long)a.w.n);
    }
    c.vt = L2Virt{};
    if (c.l2v) {
        DPPO_CHECK(!a.packed_actor || !c.anet.plain(),
                   "dppo_optimizer_step: DPPO_STEP_L2_FROM_PL2 on a plain-head actor image (it has no l2 layer)");
        DPPO_CHECK(a.packed_actor && a.actor_params == a.w.params,
                   "dppo_optimizer_step: DPPO_STEP_L2_FROM_PL2 needs the actor's image and the actor range first");
        DPPO_CHECK(a.w.n >= (int64_t)c.FA.count, "dppo_optimizer_step: DPPO_STEP_L2_FROM_PL2 needs the whole actor range");
        DPPO_CHECK(c.FA.l2_b == c.FA.l2_w + (size_t)D.H * D.H, "l2 layout");
        const MlpLayout L = make_mlp_layout(c.anet);
        c.vt = L2Virt{1, (int64_t)c.FA.l2_w, (int64_t)c.FA.l2_b, (int64_t)c.FA.out_b, D.H, D.XD, a.precision,
                      (const uint8_t*)a.packed_actor + L.off[SEG_W_OUT]};
    }
    c.clipped = a.nets != 0;
    c.clip = ClipTab{};
    if (c.clipped) {
        DPPO_CHECK(a.nets >= 1 && a.nets <= 3, "dppo_optimizer_step_clip: nets %d outside 1..3", a.nets);
        DPPO_CHECK(a.clip_scales, "dppo_optimizer_step_clip: clip_scales is NULL");
        int64_t end[CLIP_MAXV];
        const int nv = net_var_ends(c.FA, c.FC, D.HC, a.nets, end);
        const float* crit = a.w.params ? a.w.params + ((a.nets & DPPO_NET_ACTOR) ? c.FA.count : 0) : nullptr;
        DPPO_CHECK(a.w.n == end[nv - 1] && ((a.nets & DPPO_NET_ACTOR) == 0 || !a.actor_params || a.actor_params == a.w.params) &&
                   ((a.nets & DPPO_NET_CRITIC) == 0 || !a.critic_params || a.critic_params == crit),
                   "dppo_optimizer_step_clip: the range must be exactly the network(s) nets = %d names", a.nets);
        c.clip.scales = a.clip_scales;
        for (int v = 0; v < CLIP_MAXV; ++v) c.clip.end[v] = v < nv ? (int)end[v] : INT_MAX;
    }
    return DPPO_OK;
}

// the critic's step in one launch (adamw_fused_kernel)
static int fused_critic_step(const StepArgs& a, const StepCtx& c, const AdamHP& h) {
    hipStream_t s = c.s;
    StepFuse f = {};
    f.njobs = dppo_fuse_jobs(c.cnet, a.packed_critic, f.j);
    DPPO_CHECK(f.njobs >= 0, "dppo_optimizer_step: fused pack jobs");
    f.clear_grads = c.clear_g ? 1 : 0;
    for (int r = 0; r < a.n_clear; ++r) { f.clr[r] = a.clear_ptrs[r]; f.clr_words[r] = (uint32_t)(a.clear_bytes[r] / 4); }
    if (a.n_clear > 0) {
        const int rc = step_ticket(s, &f.ticket);
        if (rc) return rc;
    }
    const int64_t blocks64 = (a.w.n + 255) / 256;
    const unsigned blocks = (unsigned)(blocks64 < FUSE_BLOCKS ? blocks64 : FUSE_BLOCKS);
    DppoKtScope kt(KT_ADAMW, s);
    with_elem_fmt(a.precision, [&](auto e) {
        using E = decltype(e);
        if (c.clipped)
            hipLaunchKernelGGL((adamw_fused_kernel<typename E::ET, E::KG, E::EPL, ClipTab>), dim3(blocks), dim3(256), 0, s,
                               a.w.params, const_cast<float*>(a.w.grads), a.w.m, a.w.v, a.w.n, h, a.metrics, c.mout,
                               a.n_metrics, a.metrics_tag, f, c.clip);
        else
            hipLaunchKernelGGL((adamw_fused_kernel<typename E::ET, E::KG, E::EPL>), dim3(blocks), dim3(256), 0, s, a.w.params,
                               const_cast<float*>(a.w.grads), a.w.m, a.w.v, a.w.n, h, a.metrics, c.mout, a.n_metrics,
                               a.metrics_tag, f);
    });
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

// the actor tile step's table: the weight tensors with their images, the fp32 tensors with their
// copies, what waits for the last workgroup
static int make_tile_step(const StepArgs& a, const StepCtx& c, TileStep& t) {
    const Dims& D = c.D;
    FuseJob jobs[FUSE_MAXJ];
    const int nj = dppo_fuse_jobs(c.anet, a.packed_actor, jobs);
    DPPO_CHECK(nj >= 0, "dppo_optimizer_step: fused pack jobs");
    t = TileStep{};
    t.last_mat = -1;
    for (int q = 0; q < nj; ++q) {
        const FuseJob& J = jobs[q];
        if (J.kind == 0) {
            DPPO_CHECK(t.nmat < TILE_MAXM, "actor tile step: too many weight tensors");
            TileMat& M = t.mat[t.nmat++];
            M.off = J.lo; M.K = J.IK; M.N = J.IN; M.KS = J.KS; M.img = J.dst; M.timg = nullptr; M.KST = 0;
            M.nb = dppo_cdiv(M.N, 16);
        } else if (J.kind == 2) {
            DPPO_CHECK(t.ncpy < TILE_MAXC, "actor tile step: too many fp32 tensors");
            t.cpy[t.ncpy++] = TileCpy{J.lo, J.hi - J.lo, (float*)J.dst};
        }
    }
    for (int q = 0; q < nj; ++q) {   // the transposed images, matched to their tensor
        const FuseJob& J = jobs[q];
        if (J.kind != 1) continue;
        int mi = 0;
        while (mi < t.nmat && t.mat[mi].off != J.lo) ++mi;
        DPPO_CHECK(mi < t.nmat && J.IK == t.mat[mi].N && J.IN == t.mat[mi].K, "actor tile step: transposed image");
        t.mat[mi].timg = J.dst; t.mat[mi].KST = J.KS;
    }
    for (int r = 0; r < 2; ++r) t.keep[r][0] = t.keep[r][1] = -1;
    if (c.l2v) {
        for (int mi = 0; mi < t.nmat; ++mi)
            if (t.mat[mi].off == (int64_t)c.FA.out_w) t.last_mat = mi;
        DPPO_CHECK(t.last_mat >= 0, "actor tile step: W_out");
        t.keep[0][0] = (int64_t)c.FA.l2_w; t.keep[0][1] = (int64_t)(c.FA.l2_w + (size_t)D.H * D.XD);
        t.keep[1][0] = (int64_t)c.FA.out_b; t.keep[1][1] = (int64_t)(c.FA.out_b + D.XD);
    }
    t.mstart[0] = 0;
    for (int mi = 0; mi < t.nmat; ++mi)
        t.mstart[mi + 1] = t.mstart[mi] + (mi == t.last_mat ? 0 : t.mat[mi].nb * t.mat[mi].KS);
    t.cstart[0] = 0;
    for (int i = 0; i < t.ncpy; ++i) t.cstart[i + 1] = t.cstart[i] + t.cpy[i].n;
    t.clear_grads = c.clear_g ? 1 : 0;
    for (int r = 0; r < a.n_clear; ++r) { t.clr[r] = a.clear_ptrs[r]; t.clr_words[r] = (uint32_t)(a.clear_bytes[r] / 4); }
    return DPPO_OK;
}

// the actor's step in one launch (actor_tile_step_kernel); it leaves the TEMB table and the
// split-sampler tables to the fold launch (the row tiles derive the time embeddings, the sampler
// re-derives the tables before its next launch)
static int fused_actor_step(const StepArgs& a, const StepCtx& c, const AdamHP& h) {
    hipStream_t s = c.s;
    TileStep t;
    int rc = make_tile_step(a, c, t);
    if (rc) return rc;
    if (c.l2v || a.n_clear > 0 || c.clear_g) {
        rc = step_ticket(s, &t.ticket);
        if (rc) return rc;
    }
    const int64_t waves = t.mstart[t.nmat] + (t.cstart[t.ncpy] + 63) / 64;
    const unsigned blocks = (unsigned)((waves + TILE_THREADS / 64 - 1) / (TILE_THREADS / 64));
    {
        DppoKtScope kt(KT_ADAMW, s);
        with_elem_fmt(a.precision, [&](auto e) {
            using E = decltype(e);
            if (c.clipped)
                hipLaunchKernelGGL((actor_tile_step_kernel<typename E::ET, E::KG, E::EPL, ClipTab>), dim3(blocks),
                                   dim3(TILE_THREADS), 0, s, a.w.params, const_cast<float*>(a.w.grads), a.w.m, a.w.v, h,
                                   a.metrics, c.mout, a.n_metrics, a.metrics_tag, c.vt, t, c.clip);
            else
                hipLaunchKernelGGL((actor_tile_step_kernel<typename E::ET, E::KG, E::EPL>), dim3(blocks), dim3(TILE_THREADS), 0,
                                   s, a.w.params, const_cast<float*>(a.w.grads), a.w.m, a.w.v, h, a.metrics, c.mout,
                                   a.n_metrics, a.metrics_tag, c.vt, t);
        });
    }
    DPPO_HIP(hipGetLastError());
    rc = dppo_pack_rt_fold(c.anet, a.actor_params, a.packed_actor, s);   // cross-element: not per element
    if (rc) return rc;
    return dppo_mark_tables_stale(c.anet, a.actor_params, a.packed_actor, true);
}

// the launch-per-stage form (any ranges and images): AdamW, then the pack, which also zeroes the
// gradients AdamW has read (DPPO_STEP_CLEAR_GRADS) and the caller's ranges
static int staged_step(const StepArgs& a, const StepCtx& c) {
    hipStream_t s = c.s;
    AdamwArgs w = a.w;
    w.mode = c.mode;
    int rc = launch_adamw(w, a.metrics, c.mout, a.n_metrics, a.metrics_tag, s, c.vt, c.clipped ? &c.clip : nullptr);
    if (rc) return rc;
    void* zp[5];
    size_t zb[5];
    int nz = 0;
    if (c.clear_g && w.n > 0) { zp[nz] = const_cast<float*>(w.grads); zb[nz] = (size_t)w.n * sizeof(float); ++nz; }
    for (int r = 0; r < a.n_clear; ++r) { zp[nz] = a.clear_ptrs[r]; zb[nz] = a.clear_bytes[r]; ++nz; }
    for (int r = 0; r < nz; ++r)
        DPPO_CHECK(zb[r] / 4 < ((size_t)1 << 31), "dppo_optimizer_step_ex: clear range %d too large", r);
    if (a.packed_actor || a.packed_critic)
        return dppo_pack_models(c.anet, a.actor_params, a.packed_actor, c.cnet, a.critic_params, a.packed_critic, s, c.defer,
                                zp, zb, nz);
    if (nz) {   // no image to pack: the clears alone
        ZeroArgs z = {};
        for (int r = 0; r < nz; ++r) {
            if (r == 4) {
                rc = launch_zero(z, 16, s);
                if (rc) return rc;
                z = ZeroArgs{};
            }
            z.p[r % 4] = zp[r]; z.n[r % 4] = zb[r];
        }
        DppoKtScope kt(KT_ZERO, s);
        return launch_zero(z, 16, s);
    }
    return DPPO_OK;
}

static int optimizer_step_impl(const StepArgs& a) {
    StepCtx c;
    const int rc = step_prologue(a, c);
    if (rc) return rc;
    const AdamwArgs& w = a.w;
    // the one-launch forms: a single network whose parameters are exactly the range
    const bool one_actor = a.packed_actor && !a.packed_critic && a.actor_params == w.params && w.n == (int64_t)c.FA.count;
    const bool one_critic = a.packed_critic && !a.packed_actor && a.critic_params == w.params && w.n == (int64_t)c.FC.count_all;
    if (!(c.fuse && (one_actor || one_critic) && w.n > 0)) return staged_step(a, c);
    { const int rc_ = check_metrics_copy(a.metrics, c.mout, a.n_metrics, a.metrics_tag); if (rc_) return rc_; }
    DPPO_CHECK(w.step >= 1 && (c.mode == DPPO_ADAMW_KERAS || c.mode == DPPO_ADAMW_TORCH), "dppo_adamw: bad step or mode");
    DPPO_CHECK(w.params && w.grads && w.m && w.v, "dppo_adamw: null pointer");
    const AdamHP h = make_adam_hp(w.step, w.lr, w.weight_decay, w.beta1, w.beta2, w.eps, c.mode);
    return one_critic ? fused_critic_step(a, c, h) : fused_actor_step(a, c, h);
}

extern "C" int dppo_optimizer_step(const dppo_dims* d, int precision, float* params, const float* grads, float* m,
                                   float* v, int64_t n, int64_t step, float lr, float weight_decay, float beta1,
                                   float beta2, float eps, int mode, const float* actor_params, void* packed_actor,
                                   const float* critic_params, void* packed_critic, const double* metrics,
                                   double* metrics_out, int n_metrics, uint64_t metrics_tag, void* stream) {
    DPPO_CHECK((mode & DPPO_STEP_CLEAR_GRADS) == 0, "dppo_optimizer_step: DPPO_STEP_CLEAR_GRADS needs dppo_optimizer_step_ex");
    return optimizer_step_impl(StepArgs{d, precision, {params, grads, m, v, n, step, lr, weight_decay, beta1, beta2, eps, mode},
                                        actor_params, packed_actor, critic_params, packed_critic, metrics, metrics_out,
                                        n_metrics, metrics_tag, nullptr, nullptr, 0, stream, nullptr, 0});
}

extern "C" int dppo_optimizer_step_ex(const dppo_dims* d, int precision, float* params, float* grads, float* m,
                                      float* v, int64_t n, int64_t step, float lr, float weight_decay, float beta1,
                                      float beta2, float eps, int mode, const float* actor_params, void* packed_actor,
                                      const float* critic_params, void* packed_critic, const double* metrics,
                                      double* metrics_out, int n_metrics, uint64_t metrics_tag, void* const* clear_ptrs,
                                      const size_t* clear_bytes, int n_clear, void* stream) {
    return optimizer_step_impl(StepArgs{d, precision, {params, grads, m, v, n, step, lr, weight_decay, beta1, beta2, eps, mode},
                                        actor_params, packed_actor, critic_params, packed_critic, metrics, metrics_out,
                                        n_metrics, metrics_tag, clear_ptrs, clear_bytes, n_clear, stream, nullptr, 0});
}

extern "C" int dppo_optimizer_step_clip(const dppo_dims* d, int precision, float* params, float* grads, float* m,
                                        float* v, int64_t n, int64_t step, float lr, float weight_decay, float beta1,
                                        float beta2, float eps, int mode, const float* actor_params, void* packed_actor,
                                        const float* critic_params, void* packed_critic, const double* metrics,
                                        double* metrics_out, int n_metrics, uint64_t metrics_tag, void* const* clear_ptrs,
                                        const size_t* clear_bytes, int n_clear, void* stream, const float* clip_scales,
                                        int nets) {
    DPPO_CHECK(nets >= 1 && nets <= 3, "dppo_optimizer_step_clip: nets %d outside 1..3", nets);
    DPPO_CHECK((mode & DPPO_STEP_L2_FROM_PL2) == 0, "dppo_optimizer_step_clip: no clip with DPPO_STEP_L2_FROM_PL2 (the "
               "factored l2 gradient has no norm before it is formed)");
    return optimizer_step_impl(StepArgs{d, precision, {params, grads, m, v, n, step, lr, weight_decay, beta1, beta2, eps, mode},
                                        actor_params, packed_actor, critic_params, packed_critic, metrics, metrics_out,
                                        n_metrics, metrics_tag, clear_ptrs, clear_bytes, n_clear, stream, clip_scales, nets});
}

// ---------------------------------------------------------------------------------------------
// Per-variable gradient norms and clip scales (dppo_grad_clip_scales): tf.clip_by_norm per variable
// (the reference's max_grad_norm branch, train_ppo_diffusion_agent.py:349-354) without a launch per
// variable. Every variable is cut into chunks of CLIP_CHUNK elements that never cross a variable
// boundary; one workgroup per chunk sums its squares in fp64 ((double)g * (double)g is exact) in a
// fixed order — per thread, then a wave64 shuffle tree, then the four waves in order — and stores ONE
// partial. The last workgroup to arrive (per-XCD tickets, as last_workgroup above, here with the
// agent-scope release / acquire the partials need) adds each variable's partials in chunk order
// and writes norm = sqrt(sum) and scale = clip / max(norm, clip). No floating-point atomics: two
// launches on the same data give the same bits. Bound by launch latency and the last workgroup's
// serial sum (at most 64 partials per variable), not by the 2.7 MB it reads.
// ---------------------------------------------------------------------------------------------
constexpr int CLIP_CHUNK = 4096, CLIP_MAXCH = 512, CLIP_THREADS = 256;
struct ClipVars {
    int nv;
    int end[CLIP_MAXV];          // one past variable v in the range
    int cstart[CLIP_MAXV + 1];   // chunk prefix: variable v owns workgroups [cstart[v], cstart[v + 1])
};

// last_workgroup for a launch whose last workgroup READS what the others stored: every arrival
// releases its stores at agent scope before its ticket add, and the chain's winners acquire
__device__ inline bool last_workgroup_acquire(unsigned* ticket) {
    __shared__ int last_acq;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned xcd = blockIdx.x & 7, per = (gridDim.x - xcd + 7) / 8;
        int l = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (__hip_atomic_fetch_add(ticket + 16 * xcd, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == per - 1) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            ticket[16 * xcd] = 0u;
            const unsigned nx = gridDim.x < 8 ? gridDim.x : 8;
            l = __hip_atomic_fetch_add(ticket + 128, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nx - 1;
            if (l) {
                ticket[128] = 0u;
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
        last_acq = l;
    }
    __syncthreads();
    return last_acq != 0;
}

__device__ inline double sq64(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(CLIP_THREADS) void grad_clip_kernel(const float* __restrict__ g, ClipVars cv, float clip,
                                                                 float* __restrict__ norms, float* __restrict__ scales,
                                                                 double* part, unsigned* ticket) {
    __shared__ double red[CLIP_MAXCH];
    __shared__ int cs[CLIP_MAXV + 1];
    const int t = threadIdx.x, b = blockIdx.x;
    int v = 0;
    while (b >= cv.cstart[v + 1]) ++v;                       // uniform: this workgroup's variable
    const int lo = (v ? cv.end[v - 1] : 0) + (b - cv.cstart[v]) * CLIP_CHUNK;
    const int len = min(cv.end[v] - lo, CLIP_CHUNK);
    const float* p = g + lo;
    // 16-byte loads over the aligned body; a head of up to 3 elements and a tail, one element per thread
    const int head = min((int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2), len);
    const int nvec = (len - head) >> 2, tail0 = head + 4 * nvec;
    double acc = 0.0;
    if (t < head) acc = sq64(p[t]);
    const float4* pv = reinterpret_cast<const float4*>(p + head);
    for (int i = t; i < nvec; i += CLIP_THREADS) {
        const float4 x = pv[i];
        acc += sq64(x.x); acc += sq64(x.y); acc += sq64(x.z); acc += sq64(x.w);
    }
    if (t < len - tail0) acc += sq64(p[tail0 + t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        const double s = ((red[0] + red[1]) + red[2]) + red[3];
        // an agent-scope (write-through) store: the partial is at the memory side before the ticket add
        __hip_atomic_store(reinterpret_cast<uint64_t*>(part + b), __builtin_bit_cast(uint64_t, s), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!last_workgroup_acquire(ticket)) return;
    // (the barriers inside last_workgroup_acquire separate red's two uses)
    const int nch = cv.cstart[cv.nv];
    for (int i = t; i < nch; i += CLIP_THREADS)
        red[i] = __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const uint64_t*>(part + i), __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_AGENT));
    if (t == 0) {
#pragma unroll
        for (int k = 0; k <= CLIP_MAXV; ++k) cs[k] = cv.cstart[k];
    }
    __syncthreads();
    if (t < cv.nv) {
        double s = 0.0;
        for (int c = cs[t]; c < cs[t + 1]; ++c) s += red[c];    // chunk order
        const float nf = (float)sqrt(s);
        if (norms) norms[t] = nf;
        scales[t] = __fdiv_rn(clip, fmaxf(nf, clip));            // exactly 1 when nf <= clip (a zero tensor too)
    }
}

static int make_clip_vars(const Dims& D, int nets, ClipVars& cv, ImageAttrs critic) {
    const NetOffsets FA = make_flat_offsets(actor_net(D)), FC = make_flat_offsets(critic_net(D, DPPO_F32, critic));
    int64_t end[CLIP_MAXV];
    cv = ClipVars{};
    cv.nv = net_var_ends(FA, FC, D.HC, nets, end);
    DPPO_CHECK(end[cv.nv - 1] < ((int64_t)1 << 31), "dppo_grad_clip: range too large");
    cv.cstart[0] = 0;
    for (int v = 0; v < CLIP_MAXV; ++v) {
        cv.end[v] = (int)end[v < cv.nv ? v : cv.nv - 1];
        const int n = v < cv.nv ? (int)(end[v] - (v ? end[v - 1] : 0)) : 0;
        cv.cstart[v + 1] = cv.cstart[v] + dppo_cdiv(n, CLIP_CHUNK);
    }
    DPPO_CHECK(cv.cstart[cv.nv] <= CLIP_MAXCH, "dppo_grad_clip: %d chunks exceed %d", cv.cstart[cv.nv], CLIP_MAXCH);
    return DPPO_OK;
}

extern "C" size_t dppo_grad_clip_workspace_bytes_ln(const dppo_dims* d, int nets, int critic_head, int critic_layernorm) {
    Dims D;
    ClipVars cv;
    if (dppo_check_dims(d, &D) || nets < 1 || nets > 3 || !dppo_head_ok(critic_head) || !dppo_ln_ok(critic_layernorm) ||
        make_clip_vars(D, nets, cv, ImageAttrs{DPPO_ACT_RELU, critic_head, critic_layernorm}))
        return 0;
    return (size_t)cv.cstart[cv.nv] * sizeof(double);
}
extern "C" size_t dppo_grad_clip_workspace_bytes(const dppo_dims* d, int nets) {
    return dppo_grad_clip_workspace_bytes_ln(d, nets, DPPO_HEAD_RESIDUAL, DPPO_LN_OFF);
}

extern "C" int dppo_grad_clip_scales(const dppo_dims* d, int nets, const float* grads, float clip_norm, float* norms,
                                     float* scales, void* workspace, void* stream) {
    return dppo_grad_clip_scales_ln(d, nets, DPPO_HEAD_RESIDUAL, DPPO_LN_OFF, grads, clip_norm, norms, scales, workspace,
                                    stream);
}

// the same over the variables of a critic with the given attributes: its gamma / beta vectors follow out_b, each
// with a norm and a scale of its own (8 + 4 residual, 8 + 6 plain)
extern "C" int dppo_grad_clip_scales_ln(const dppo_dims* d, int nets, int critic_head, int critic_layernorm,
                                        const float* grads, float clip_norm, float* norms, float* scales, void* workspace,
                                        void* stream) {
    Dims D;
    int rc = dppo_check_dims(d, &D);
    if (rc) return rc;
    DPPO_CHECK(dppo_head_ok(critic_head), "dppo_grad_clip_scales_ln: bad head %d (DPPO_HEAD_RESIDUAL or DPPO_HEAD_PLAIN)", critic_head);
    DPPO_CHECK(dppo_ln_ok(critic_layernorm), "dppo_grad_clip_scales_ln: bad layernorm %d (DPPO_LN_OFF or DPPO_LN_ON)",
               critic_layernorm);
    DPPO_CHECK(nets >= 1 && nets <= 3, "dppo_grad_clip_scales: nets %d outside 1..3", nets);
    DPPO_CHECK(clip_norm > 0.f && clip_norm <= 3.0e38f, "dppo_grad_clip_scales: clip_norm must be > 0 and finite");
    DPPO_CHECK(grads && scales, "dppo_grad_clip_scales: grads or scales is NULL");
    DPPO_CHECK(workspace && ((uintptr_t)workspace & 7) == 0, "dppo_grad_clip_scales: workspace must be 8-B aligned");
    DPPO_CHECK(((uintptr_t)grads & 3) == 0, "dppo_grad_clip_scales: grads must be 4-B aligned");
    ClipVars cv;
    rc = make_clip_vars(D, nets, cv, ImageAttrs{DPPO_ACT_RELU, critic_head, critic_layernorm});
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    unsigned* ticket = nullptr;
    rc = step_ticket(s, &ticket);
    if (rc) return rc;
    DppoKtScope kt(KT_GRAD_CLIP, s);
    hipLaunchKernelGGL(grad_clip_kernel, dim3((unsigned)cv.cstart[cv.nv]), dim3(CLIP_THREADS), 0, s, grads, cv, clip_norm,
                       norms, scales, (double*)workspace, ticket);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

// ---------------------------------------------------------------------------------------------
// Learnable DDIM eta (§8(f) row 4; the original DPPO's EtaFixed, parity unpinned: the reference's
// eta module is absent and its eta step is commented out, train_ppo_diffusion_agent.py:28-45,
// 358-359). state = {logit, m, v}; eta = eta_min + (eta_max - eta_min) (tanh(logit) + 1) / 2.
// One workgroup: thread 0 applies AdamW to the logit with d loss / d logit = metrics[8] d eta / d
// logit (metrics[8] = d loss / d eta from the DPPO_PPO_LEARN_ETA row tiles), then one thread per
// DDIM row rewrites the eta-dependent schedule columns c2, c3, logvar in ddim_buffers' fp32 order of
// operations (model/diffusion/sampling.py), from the eta-independent base rows
// {abar_prev, sqrt(abar_prev), sqrt(abar), sqrt(1 - abar), s}.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void eta_step_kernel(float* __restrict__ st, const double* __restrict__ met, int apply,
                                                     float lr, float wd, float b1, float b2, float eps, float alpha,
                                                     float bc1, float bc2, int mode, float emin, float emax,
                                                     const float* __restrict__ base, float* __restrict__ sched, int S,
                                                     float* __restrict__ eta_out) {
    __shared__ float eta_s;
    if (threadIdx.x == 0) {
        float th = st[0];
        if (apply) {
            const float tn = tanhf(th);
            const float gi = (float)met[8] * (0.5f * (emax - emin) * (1.f - tn * tn));
            float mi = st[1], vi = st[2];
            if (mode == DPPO_ADAMW_KERAS) {
                th -= th * wd * lr;
                mi += (gi - mi) * (1.f - b1);
                vi += (gi * gi - vi) * (1.f - b2);
                th -= (mi * alpha) / (sqrtf(vi) + eps);
            } else {
                th *= 1.f - lr * wd;
                mi = b1 * mi + (1.f - b1) * gi;
                vi = b2 * vi + (1.f - b2) * gi * gi;
                th -= lr * (mi / bc1) / (sqrtf(vi / bc2) + eps);
            }
            st[0] = th; st[1] = mi; st[2] = vi;
        }
        const float e = emin + (emax - emin) * (0.5f * (tanhf(th) + 1.f));
        eta_s = e;
        if (eta_out) *eta_out = e;
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j < S) {
        const float* b = base + 5 * j;   // abar_prev, sqrt(abar_prev), sqrt(abar), sqrt(1 - abar), s
        const float sig = fmaxf(__fmul_rn(eta_s, b[4]), 1e-10f);
        const float in = __fsub_rn(__fsub_rn(1.f, b[0]), __fmul_rn(sig, sig));
        const float dd = sqrtf(fminf(fmaxf(in, 0.f), 1e6f));
        float* r = sched + (size_t)j * DPPO_SCHED_COLS;
        r[2] = __fsub_rn(b[1], __fdiv_rn(__fmul_rn(dd, b[2]), b[3]));
        r[3] = __fdiv_rn(dd, b[3]);
        r[4] = logf(__fmul_rn(sig, sig));
    }
}

extern "C" int dppo_eta_step(float* eta_state, const double* metrics, int64_t step, float lr, float weight_decay,
                             float beta1, float beta2, float eps, int mode, float eta_min, float eta_max,
                             const float* ddim_base, float* sched, int ddim_steps, float* eta_out, void* stream) {
    DPPO_CHECK(eta_state && ddim_base && sched, "dppo_eta_step: null pointer");
    DPPO_CHECK(ddim_steps >= 1 && ddim_steps <= 64, "dppo_eta_step: ddim_steps %d outside [1, 64]", ddim_steps);
    DPPO_CHECK(eta_max > eta_min, "dppo_eta_step: eta_max must exceed eta_min");
    DPPO_CHECK(mode == DPPO_ADAMW_KERAS || mode == DPPO_ADAMW_TORCH, "dppo_eta_step: bad mode");
    const int apply = metrics != nullptr && step >= 1;
    // no step applied: the bias corrections are 1 (alpha = lr), unused by the kernel
    const AdamHP h = apply ? make_adam_hp(step, lr, weight_decay, beta1, beta2, eps, mode)
                           : AdamHP{lr, weight_decay, beta1, beta2, eps, lr, 1.f, 1.f, mode};
    hipLaunchKernelGGL(eta_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, eta_state, metrics, apply, h.lr, h.wd,
                       h.b1, h.b2, h.eps, h.alpha, h.bc1, h.bc2, h.mode, eta_min, eta_max, ddim_base, sched, ddim_steps,
                       eta_out);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}
