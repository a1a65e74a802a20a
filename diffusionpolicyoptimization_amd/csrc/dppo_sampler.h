// dppo_sampler.h — what the two sampler kernels share (sampler.hip: the weight-streaming kernel and the
// launch path; sampler_split.hip: the register-resident split kernel): the launch arguments
// (SampleArgs), each kernel's LDS layout (STREAM_LDS_REGIONS / SPLIT_LDS_REGIONS: the kernel takes its
// pointers and the launcher its byte count from the same list), the device helpers the kernels run
// (noise-std rule, the go wait, the tagged observation load; the noise draws) and the split kernel's plan
// (SplitPlan).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dppo_common.cuh"
#include "dppo_layout.h"

struct SampleArgs {
    const uint8_t* packed_base;
    const uint8_t* packed_ft;
    const float* sched;   // [K][8]
    const float* cond;    // [E][SD]
    const float* x_T;     // [E][XD] or null
    const float* noise;   // [K][E][XD] or null
    float* actions;       // [E][XD]
    float* chains;        // [E][KF+1][XD] or null
    float* cond_out;      // [E][SD] device copy of cond or null (cond may be mapped host memory)
    float* actions_host;  // [E][XD] mapped pinned host memory or null (zero-copy action hand-off)
    uint64_t* actions_tagged;  // [E][XD] tagged granules {cond_tag, fp32} in mapped host memory, or null
    // pre-enqueued rollout steps (dppo_rollout_*): wait until *go >= go_value before reading cond,
    // and add 1 to *done per workgroup after the actions are visible to the host (both counters
    // live in fine-grained host memory); null = an ordinary launch
    const uint32_t* go;
    uint32_t go_value;
    uint32_t* done;
    // tagged observation (dppo_rollout_enqueue_tagged): [E][SD] granules {tag << 32 | fp32 bits}
    // polled until every tag equals cond_tag (then cond is unused); null = cond / go as above
    const uint64_t* cond_tagged;
    uint32_t cond_tag;
    int act;              // the images' activation (DPPO_ACT_*), filled by sample_impl: read by the DPPO_ACT_BY_ARG
                          // instantiations only. It sits in the hole before `seed`: no other field moves
    uint64_t seed;
    uint32_t call_id;
    int E, env_offset, deterministic;
    float min_std, randn_clip, final_clip;
    float x0_clip;        // the table's denoised_clip_value (SchedParams; +inf = none), filled by sample_impl
    int XD, SD, TD, H, K, KF, IN;
    MlpLayout L;          // same layout for base and ft
};

// This workgroup's R (16 or 32) env rows of a TAGGED observation into st[R][SD]: every thread polls
// its granules (system-scope relaxed loads of mapped host memory) until each carries a.cond_tag — the
// value arrives with its own ready flag, so there is no separate flag round trip. Bounded (4 s):
// on timeout the step runs on what it read and (flag_timeout) sets bit 31 of *done.
template <int ST, int R = 16>
__device__ inline void sampler_load_state_tagged(const SampleArgs& a, int row0, float* st, bool flag_timeout, int tid) {
    const int SD = a.SD, n = R * SD;
    constexpr int NG = (R * 64 + ST - 1) / ST;      // SD <= 64 (dppo_check_dims)
    float v[NG];
    bool ok[NG];
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        const int i = tid + u * ST;
        ok[u] = !(i < n && row0 + i / SD < a.E);
        v[u] = 0.f;
    }
    const uint64_t t_end = __builtin_amdgcn_s_memrealtime() + 400000000ull;   // 100 MHz: 4 s
    for (;;) {
        bool all = true;
#pragma unroll
        for (int u = 0; u < NG; ++u) {
            const int i = tid + u * ST;
            if (!ok[u]) {
                const uint64_t x = __hip_atomic_load(a.cond_tagged + (size_t)(row0 + i / SD) * SD + i % SD,
                                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if ((uint32_t)(x >> 32) == a.cond_tag) {
                    ok[u] = true;
                    v[u] = __uint_as_float((uint32_t)x);
                }
            }
            all = all && ok[u];
        }
        if (__syncthreads_and(all)) break;
        if (__syncthreads_or(__builtin_amdgcn_s_memrealtime() > t_end)) {
            if (flag_timeout && tid == 0 && a.done)
                __hip_atomic_fetch_or(a.done, 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        __builtin_amdgcn_s_sleep(2);
    }
#pragma unroll
    for (int u = 0; u < NG; ++u) {
        const int i = tid + u * ST;
        if (i < n) st[i] = v[u];
    }
}

// ---- LDS layouts: byte offsets into the kernel's dynamic LDS (all multiples of 16) and their total ----
// Each kernel's regions in carve order, F(element type, name, bytes), over the kernel's own names. A list,
// not a function of offsets: the kernel expands it to the carve statements it was tuned with (a layout
// struct moved both kernels' register allocation), the launcher's *_lds_total to their sum.
// The streaming kernel: ESZ operand bytes, ldh / lda0 row strides of the hidden tiles and of a0, SW waves,
// NOC = 16 NO out columns.   bias [actor][in,l1,l2,out]; zt clipped noise [i][row][q]
#define STREAM_LDS_REGIONS(F)                                  \
    F(AT, tA, dppo_align16(ESZ * 16 * ldh))                    \
    F(AT, tB, dppo_align16(ESZ * 16 * ldh))                    \
    F(AT, a0, dppo_align16(ESZ * 16 * lda0))                   \
    F(float, xs, dppo_align16(4 * 16 * XD))                    \
    F(float, st, dppo_align16(4 * 16 * SD))                    \
    F(float, temb, dppo_align16(4 * K * TD))                   \
    F(float, part, dppo_align16(4 * SW * 16 * NOC))            \
    F(float, sch, dppo_align16(4 * K * DPPO_SCHED_COLS))       \
    F(float, bias, dppo_align16(4 * 2 * (3 * H + NOC)))        \
    F(float, zt, dppo_align16(4 * K * 16 * XD))
// The split kernel: ESZ operand bytes, lda0 / ldh row strides, SW waves, NV = 16 XD, TRING (TIN as a 2-row
// ring instead of all K rows), H, NB per-actor bias floats, NTI = 32 / SW in-Dense n-tiles per wave, KX
// in-Dense k-steps.
//   part [wave][16 x XD]; xfail [0] exchange failure, [1] exchange mode; wxs [wave][n][ks] in-Dense fragments
#define SPLIT_LDS_REGIONS(F)                                   \
    F(AT, a0, dppo_align16(ESZ * 16 * lda0))                   \
    F(AT, u1, dppo_align16(ESZ * 16 * ldh))                    \
    F(float, part, dppo_align16(4 * SW * NV))                  \
    F(int, xfail, 16)                                          \
    F(float, xs, dppo_align16(4 * 16 * XD))                    \
    F(float, st, dppo_align16(4 * 16 * SD))                    \
    F(float, tin, dppo_align16(4 * (TRING ? 2 : K) * H))       \
    F(float, sch, dppo_align16(4 * K * DPPO_SCHED_COLS))       \
    F(float, bias, dppo_align16(4 * 2 * NB))                   \
    F(float, zt, dppo_align16(4 * K * 16 * XD))                \
    F(u32x4, wxs, (size_t)SW * NTI * KX * 1024)
// dynamic LDS of the split kernel at H = 512: ESZ operand bytes, KX in-Dense k-steps, SW waves per member
inline size_t split_lds_total(size_t ESZ, int KX, int XD, int SD, int K, int SW) {
    const int H = 512, pad = 16, ldh = H + pad, lda0 = KX * (ESZ == 2 ? 32 : 16) + pad;
    const int NV = 16 * XD, NB = H + 16 * ((XD + 15) / 16), NTI = 32 / SW;
    const bool TRING = KX == 2 || ESZ == 4;
    size_t o = 0;
#define DPPO_SUM(T, name, bytes) o += bytes;
    SPLIT_LDS_REGIONS(DPPO_SUM)
#undef DPPO_SUM
    return o;
}

// ---- device helpers both kernels run (sampler_draw_noise: the streaming kernel; the split kernel keeps
//      its own copy of that loop, see there) ----
// All K steps' noise draws of this workgroup's 16 env rows up front (injected, or the Philox stream:
// one block gives the 4 normals of a group of 4 action coordinates), clipped to +-randn_clip
// (diffusion_vpg.py:319) into zt[step][row][q], so the denoising loop carries no RNG state; slot K is
// x_T into xs. chain0: this workgroup stores chain row 0 (x_T when every step is fine-tuned) with `store`.
template <bool INJ, int ST, class Store>
__device__ inline void sampler_draw_noise(const SampleArgs& a, int XD, int row0, int tid, float* zt, float* xs,
                                          bool chain0, Store store) {
    const int K = a.K, KF = a.KF;
    const int XG = (XD + 3) / 4;
    for (int it = tid; it < (K + 1) * 16 * XG; it += ST) {
        const int step = it / (16 * XG), r = (it / XG) % 16, g = it % XG, row = row0 + r;
        float z[4];
        if (step == K && a.x_T) {
#pragma unroll
            for (int k = 0; k < 4; ++k) z[k] = (row < a.E && 4 * g + k < XD) ? a.x_T[(size_t)row * XD + 4 * g + k] : 0.f;
        } else if (INJ && step < K) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                z[k] = (row < a.E && 4 * g + k < XD) ? a.noise[((size_t)step * a.E + row) * XD + 4 * g + k] : 0.f;
        } else {
            philox_normal4(a.seed, (uint32_t)g, (uint32_t)(a.env_offset + row), (uint32_t)step, a.call_id, z);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = 4 * g + k;
            if (q >= XD) break;
            if (step < K) {
                zt[(step * 16 + r) * XD + q] = fminf(fmaxf(z[k], -a.randn_clip), a.randn_clip);
            } else {
                xs[r * XD + q] = z[k];
                if (chain0 && row < a.E) store(a.chains + ((size_t)row * (KF + 1) + 0) * XD + q, z[k]);
            }
        }
    }
}

// the sampling std of schedule row sc (include/dppo.h: eval DDPM t = 0 or any DDIM row -> 0; other
// eval DDPM rows clip at the row's floor, 1e-3; train: min_std; diffusion_vpg.py:303-315)
__device__ inline float sampler_noise_std(const SampleArgs& a, const float* sc) {
    float sd = expf(0.5f * sc[4]);
    if (a.deterministic && sc[6] != 0.f) sd = 0.f;
    else if (a.deterministic) sd = fminf(fmaxf(sd, sc[5]), 1e6f);
    else sd = fminf(fmaxf(sd, a.min_std), 1e6f);
    return sd;
}

// Host hand-off of a pre-enqueued step (go protocol): thread 0 polls *go (relaxed) until it reaches
// go_value, then one system acquire after the match; everything before this call must not depend on the
// observation. Bounded (4 s): then the step runs on whatever the buffer holds and (flag_timeout) sets bit
// 31 of *done so the host reports it. Ends with the workgroup's barrier.
__device__ inline void sampler_wait_go(const SampleArgs& a, bool flag_timeout, int tid) {
    if (tid == 0) {
        const uint64_t t_end = __builtin_amdgcn_s_memrealtime() + 400000000ull;   // 100 MHz: 4 s
        while (__hip_atomic_load(a.go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < a.go_value) {
            __builtin_amdgcn_s_sleep(8);
            if (__builtin_amdgcn_s_memrealtime() > t_end) {
                if (flag_timeout) __hip_atomic_fetch_or(a.done, 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");    // one system acquire after the match
    }
    __syncthreads();
}

// ---- the split sampler (sampler_split.hip) ----
// Its plan for a shape: P members per 16-env group (2 for 2-byte operands, 8 for fp32; 0 = not taken:
// the weight-streaming kernel), whether the two actors run on two member sets (dual), blocks =
// workgroups of one launch, cus = CUs of the current device (0 if unknown).
struct SplitPlan { int P; bool dual; int blocks; int cus; };
SplitPlan split_plan(int precision, int H, int XD, int SD, int E, int K, int KF);
// returns DPPO_OK after launching, DPPO_EUNSUPPORTED (without touching the error message) when
// split_plan does not take the shape, or another error code
// act: the images' activation (DPPO_ACT_*): ReLU and Mish have an instantiation each, ELU / GELU / Softplus share
// DPPO_ACT_BY_ARG's (dppo_common.cuh) and follow a.act
int launch_sample_split(const SampleArgs& a, int precision, int act, hipStream_t s);
