// update.hip — minibatch statistics and row dedup, the dppo_ppo_minibatch orchestration
// (agent/finetune/train_ppo_diffusion_agent.py:287-356) and the pretraining minibatch. The kernels
// it orchestrates: rowtile.hip (row tiles), dw.hip (weight gradients), backward_tail.hip (what
// follows them); optimizer.hip holds the step.
#include <stdlib.h>
#include <mutex>
#include <vector>
#include "dppo_update.h"

// ---------------------------------------------------------------------------------------------
// minibatch advantage statistics {count, sum, sumsq} (for norm_adv, diffusion_ppo.py:74-75)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adv_stats_kernel(const float* __restrict__ adv, FeistelKey fk, int KF, int64_t start,
                                                        int rows, const int64_t* __restrict__ row_index,
                                                        double* __restrict__ stats) {
    __shared__ double sh[3][4];
    double c = 0.0, s = 0.0, s2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows; i += (int64_t)gridDim.x * 256) {
        const uint64_t idx = minibatch_row(row_index, (uint64_t)(start + i), fk);
        if (idx >= fk.n) continue;
        const double v = adv[idx / KF];
        c += 1.0; s += v; s2 += v * v;
    }
    c = wave_sumd(c); s = wave_sumd(s); s2 = wave_sumd(s2);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[0][w] = c; sh[1][w] = s; sh[2][w] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(stats + 0, sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3]);
        atomicAdd(stats + 1, sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3]);
        atomicAdd(stats + 2, sh[2][0] + sh[2][1] + sh[2][2] + sh[2][3]);
    }
}

// the advantage moments of every minibatch of an update phase in one launch: blockIdx.y = minibatch
// m = epoch * nbatch + batch; rows [batch * rows_full, min(+rows_full, total)) of epoch `epoch`'s
// permutation (the per-minibatch adv_stats_kernel, batched)
#define ADV_MAXE 64
struct AdvStatsAll {
    FeistelKey fk[ADV_MAXE];
    int nbatch, KF;
    int64_t rows_full, total;
};
__global__ __launch_bounds__(256) void adv_stats_all_kernel(const float* __restrict__ adv, AdvStatsAll a,
                                                            double* __restrict__ stats) {
    __shared__ double sh[3][4];
    const int m = blockIdx.y, e = m / a.nbatch, b = m % a.nbatch;
    const int64_t start = (int64_t)b * a.rows_full;
    const int64_t end = start + a.rows_full < a.total ? start + a.rows_full : a.total;
    const FeistelKey fk = a.fk[e];
    double c = 0.0, s = 0.0, s2 = 0.0;
    for (int64_t i = start + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (int64_t)gridDim.x * 256) {
        const uint64_t idx = minibatch_row(nullptr, (uint64_t)i, fk);
        if (idx >= fk.n) continue;
        const double v = adv[idx / a.KF];
        c += 1.0; s += v; s2 += v * v;
    }
    c = wave_sumd(c); s = wave_sumd(s); s2 = wave_sumd(s2);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[0][w] = c; sh[1][w] = s; sh[2][w] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(stats + 3 * m + 0, sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3]);
        atomicAdd(stats + 3 * m + 1, sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3]);
        atomicAdd(stats + 3 * m + 2, sh[2][0] + sh[2][1] + sh[2][2] + sh[2][3]);
    }
}

// zero up to 4 byte ranges (ZeroArgs, dppo_update.h) in one launch:
// 16-B stores over the 16-B aligned body of each range, 4-B stores over its head and tail (the
// grid is small: it runs while the other stream's row tiles hold most CUs)
__global__ __launch_bounds__(256) void zero_kernel(ZeroArgs z) {
    const size_t stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (int r = 0; r < 4; ++r) {
        if (!z.p[r]) continue;
        uint32_t* q = (uint32_t*)z.p[r];
        const size_t n = z.n[r] / 4;
        const size_t head = ((16 - ((uintptr_t)q & 15)) & 15) / 4 < n ? ((16 - ((uintptr_t)q & 15)) & 15) / 4 : n;
        const size_t n4 = (n - head) / 4;
        uint4* q4 = (uint4*)(q + head);
        for (size_t i = t0; i < n4; i += stride) q4[i] = uint4{0u, 0u, 0u, 0u};
        for (size_t i = t0; i < head; i += stride) q[i] = 0u;
        for (size_t i = head + 4 * n4 + t0; i < n; i += stride) q[i] = 0u;
    }
}
int launch_zero(const ZeroArgs& z, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(zero_kernel, dim3(blocks), dim3(256), 0, s, z);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

// ---------------------------------------------------------------------------------------------
// The critic's distinct samples of a minibatch. The value loss depends on the sample only (obs,
// returns: diffusion_ppo.py:108-118), and a minibatch of b rows drawn from S*E*K' (sample, step)
// pairs holds each sample ~b/(S*E) times (1.56x at the bench shape: 50,000 rows, 26k distinct
// samples), so the critic runs once per distinct sample with the multiplicity as the row weight:
// the same loss and gradient sums, ~half the critic row tiles and dW rows.
// crit_rows_kernel (one launch): cnt[sample] += 1 per row; the row that takes a count from 0 appends
// the sample to crow_n (one atomic per wave on crow_cnt: the wave's first-touch lanes are ranked by
// mbcnt). The list is in arrival order, so the critic's fp32 sums are accumulated in a run-dependent
// order, as the dW's split-K atomics already are. The critic's row tile reads the weights from cnt;
// the critic's last kernel (l2_back_kernel) zeroes the listed counts for the next minibatch.
// (It replaced a count launch + a one-workgroup ordered compaction: 6 + 27 us alone, 85 + 90 us
// beside the actor's row tiles.)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void crit_rows_kernel(const int64_t* __restrict__ row_index, int64_t start, int rows,
                                                        FeistelKey fk, int KF, uint32_t* __restrict__ cnt,
                                                        int* __restrict__ crow_n, int* __restrict__ crow_cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t n_iter = ((int64_t)rows + (int64_t)gridDim.x * 256 - 1) / ((int64_t)gridDim.x * 256);
    for (int64_t it = 0; it < n_iter; ++it) {   // uniform trip count: every lane reaches the ballot
        const int64_t i = (it * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        int s = -1;
        if (i < rows) {
            const uint64_t idx = minibatch_row(row_index, (uint64_t)(start + i), fk);
            if (idx < fk.n) s = (int)(idx / (uint64_t)KF);
        }
        const bool first = s >= 0 && atomicAdd(cnt + s, 1u) == 0u;
        const uint64_t m = __ballot(first);
        if (m == 0) continue;
        const int leader = __builtin_ctzll(m);
        int base = 0;
        if (lane == leader) base = atomicAdd(crow_cnt, __popcll(m));
        base = __shfl(base, leader, 64);
        if (first) crow_n[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = s;
    }
}

// Per-(device, stream) device scratch that kernels leave zeroed between uses (the fused steps' ticket
// counters, crit_rows_kernel's sample counts), created zeroed on first use and kept for the process:
// one process-wide table under a mutex, keyed by the stream's OWN device (not the caller's current
// one) and a kind. No eviction, so no device-wide wait: a pipelined sampler launch may be waiting for
// an observation the host publishes later. Growth waits for that stream alone (the only one that
// used the buffer).
int stream_scratch(hipStream_t s, int kind, size_t bytes, void** out) {
    struct Ent { int dev; hipStream_t s; int kind; void* p; size_t cap; };
    static std::mutex mu;
    static std::vector<Ent> ents;
    int dev = 0;
    DPPO_HIP(hipStreamGetDevice(s, &dev));
    std::lock_guard<std::mutex> lk(mu);
    size_t i = 0;
    while (i < ents.size() && !(ents[i].dev == dev && ents[i].s == s && ents[i].kind == kind)) ++i;
    if (i < ents.size() && ents[i].cap >= bytes) { *out = ents[i].p; return DPPO_OK; }
    int cur = 0;
    DPPO_HIP(hipGetDevice(&cur));
    if (cur != dev) DPPO_HIP(hipSetDevice(dev));
    hipError_t err = hipSuccess;
    if (i < ents.size()) {   // grow: the old buffer's last user is this stream
        err = hipStreamSynchronize(s);
        if (err == hipSuccess) (void)hipFree(ents[i].p);
        ents.erase(ents.begin() + (ptrdiff_t)i);
    }
    void* p = nullptr;
    if (err == hipSuccess) err = hipMalloc(&p, bytes);
    if (err == hipSuccess) err = hipMemsetAsync(p, 0, bytes, s);
    if (cur != dev) (void)hipSetDevice(cur);
    if (err != hipSuccess) {
        if (p) (void)hipFree(p);
        (void)hipGetLastError();
        return dppo_set_error(DPPO_EHIP, "stream scratch (kind %d, %zu B): %s", kind, bytes, hipGetErrorString(err));
    }
    ents.push_back(Ent{dev, s, kind, p, bytes});
    *out = p;
    return DPPO_OK;
}

// crit_rows_kernel's per-sample counts (zero between uses), grown on demand
static int crit_count_scratch(int64_t nsamp, hipStream_t s, uint32_t** out) {
    const int64_t cap = nsamp > 65536 ? nsamp : 65536;
    return stream_scratch(s, SCRATCH_CRIT_COUNT, (size_t)cap * 4, (void**)out);
}

// DPPO_CRITIC_DEDUP=0 runs the critic per minibatch row (measurement knob)
static bool crit_dedup() {
    static const bool on = [] { const char* e = getenv("DPPO_CRITIC_DEDUP"); return !e || atoi(e) != 0; }();
    return on;
}

__global__ void feistel_kernel(int64_t first, int64_t count, FeistelKey fk, int64_t* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) {
        const uint64_t v = feistel_permute((uint64_t)(first + i), fk);
        out[i] = v < fk.n ? (int64_t)v : -1;
    }
}
// one non-blocking side stream (+ fork/join events) per device and host thread, created on first use;
// null if creation fails (the caller then runs everything on its own stream)
// (the critic's half of a whole minibatch)
struct SideStream { hipStream_t stream; hipEvent_t fork, join; };
static SideStream* side_stream() {
    constexpr int MAXDEV = 16;
    thread_local SideStream ss[MAXDEV] = {};
    thread_local bool tried[MAXDEV] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return nullptr;
    SideStream& e = ss[dev];
    if (!tried[dev]) {
        tried[dev] = true;
        if (hipStreamCreateWithFlags(&e.stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&e.fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e.join, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            e.stream = nullptr;
        }
    }
    return e.stream ? &e : nullptr;
}
extern "C" int dppo_pack_all(const dppo_dims* d, int precision, const float* actor_params, void* packed_actor,
                             const float* critic_params, void* packed_critic, void* stream) {
    Dims D;
    int rc = dppo_check_dims(d, &D);
    if (rc) return rc;
    DPPO_CHECK(dppo_prec_ok(precision), "bad precision %d", precision);
    DPPO_CHECK(!packed_actor == !actor_params && !packed_critic == !critic_params,
               "dppo_pack_all: a packed image needs its parameters");
    // = dppo_pack_actor + dppo_pack_critic: ReLU / RESIDUAL for the actor, RESIDUAL / no layer norm for the critic
    rc = dppo_pack_models(actor_net(D, precision), actor_params, packed_actor, critic_net(D, precision), critic_params,
                          packed_critic, (hipStream_t)stream);
    if (rc != DPPO_OK) return rc;
    if (packed_actor) dppo_image_commit(packed_actor, ImageAttrs());
    if (packed_critic) dppo_image_commit(packed_critic, ImageAttrs());
    return DPPO_OK;
}

extern "C" int dppo_feistel_permute(int64_t first, int64_t count, int64_t n, uint64_t seed, int epoch, int64_t* out,
                                    void* stream) {
    DPPO_CHECK(n > 0 && count >= 0 && first >= 0, "dppo_feistel_permute: bad range");
    if (count == 0) return DPPO_OK;
    DPPO_CHECK(out, "dppo_feistel_permute: null out");
    const FeistelKey fk = feistel_key((uint64_t)n, seed, epoch);
    hipLaunchKernelGGL(feistel_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       first, count, fk, out);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

extern "C" int dppo_ppo_adv_stats(const float* advantages, int64_t total, int K_ft, uint64_t perm_seed, int epoch,
                                  int64_t start, int rows, const int64_t* row_index, double* adv_stats, void* stream) {
    DPPO_CHECK(advantages && adv_stats && total > 0 && K_ft > 0 && rows >= 0, "dppo_ppo_adv_stats: bad args");
    hipStream_t s = (hipStream_t)stream;
    DPPO_HIP(hipMemsetAsync(adv_stats, 0, 3 * sizeof(double), s));
    if (rows == 0) return DPPO_OK;
    const FeistelKey fk = feistel_key((uint64_t)total, perm_seed, epoch);
    const int blocks = dppo_cdiv(rows, 256) < 512 ? dppo_cdiv(rows, 256) : 512;
    hipLaunchKernelGGL(adv_stats_kernel, dim3(blocks), dim3(256), 0, s, advantages, fk, K_ft, start, rows, row_index,
                       adv_stats);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

extern "C" int dppo_ppo_adv_stats_all(const float* advantages, int64_t total, int K_ft, uint64_t perm_seed, int epoch0,
                                      int n_epochs, int64_t rows_full, int n_batch, double* adv_stats, void* stream) {
    DPPO_CHECK(advantages && adv_stats && total > 0 && K_ft > 0 && rows_full > 0 && n_batch > 0 && n_epochs > 0,
               "dppo_ppo_adv_stats_all: bad args");
    DPPO_CHECK(n_epochs <= ADV_MAXE, "dppo_ppo_adv_stats_all: at most %d epochs", ADV_MAXE);
    DPPO_CHECK((uint64_t)total < ((uint64_t)1 << 32), "dppo_ppo_adv_stats_all: total exceeds 2^32");
    hipStream_t s = (hipStream_t)stream;
    const int nm = n_epochs * n_batch;
    DPPO_HIP(hipMemsetAsync(adv_stats, 0, (size_t)3 * nm * sizeof(double), s));
    AdvStatsAll a = {};
    for (int e = 0; e < n_epochs; ++e) a.fk[e] = feistel_key((uint64_t)total, perm_seed, epoch0 + e);
    a.nbatch = n_batch; a.KF = K_ft; a.rows_full = rows_full; a.total = total;
    const int64_t bx = dppo_cdiv((int)(rows_full < total ? rows_full : total), 256);
    const int blocks = bx < 64 ? (int)bx : 64;
    DppoKtScope kt(KT_ADV_STATS, s);
    hipLaunchKernelGGL(adv_stats_all_kernel, dim3(blocks, nm), dim3(256), 0, s, advantages, a, adv_stats);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

extern "C" size_t dppo_ppo_workspace_bytes(const dppo_dims* d, int precision, int batch_rows) {
    Dims D;
    if (dppo_check_dims(d, &D) || batch_rows < 0) return 0;
    return make_ppo_workspace(D, precision, batch_rows, nullptr).total;
}
// the parts of a minibatch: the values of dppo_ppo_minibatch_part's `part` (include/dppo.h: each on
// the caller's stream, the caller overlaps them), and the whole minibatch (the critic's half on the
// internal side stream)
enum MbPart { MB_ACTOR = 1, MB_CRITIC = 2, MB_WHOLE = 3, MB_ACTOR_TILES = 4, MB_ACTOR_DW = 5 };

// the atomically accumulated outputs a minibatch half (or the whole) zeroes first: gradients (entry
// 0), metrics (actor: 0, 2..15; critic: 1), pl2 | bucket sums, cpl2 | stats | crow_cnt. Entries 1..3
// are what dppo_ppo_clear_ranges reports (the gradients are cleared by the optimizer step's AdamW)
// A layer-normed critic's gradient tail (dgamma / dbeta, added by the row tiles) follows the critic's eight tensors
// in `grads` and is zeroed with them
static ZeroArgs minibatch_zero_args(const Dims& D, const NetSpec& critic, const PpoWorkspace& ws, float* grads,
                                    double* metrics, MbPart part) {
    const size_t na = make_flat_offsets(actor_net(D)).count, nc = make_flat_offsets(critic).count_all;
    ZeroArgs z = {};
    // pl2 | pa0 | gseg: the bucket rows the dW adds into, whole wave rows of 16 (K' <= 64)
    const size_t actor_acc = (size_t)((const uint8_t*)(ws.gseg + (size_t)dppo_cdiv(D.KF, 16) * 16 * D.H) - (const uint8_t*)ws.pl2);
    const size_t critic_acc = (size_t)((const uint8_t*)(ws.crow_cnt + 1) - (const uint8_t*)ws.cpl2);
    if (part == MB_WHOLE) {
        z.p[0] = grads; z.n[0] = (na + nc) * sizeof(float);
        z.p[1] = metrics; z.n[1] = 16 * sizeof(double);
        z.p[2] = ws.pl2; z.n[2] = actor_acc;
        z.p[3] = ws.cpl2; z.n[3] = critic_acc;
    } else if (part == MB_ACTOR || part == MB_ACTOR_TILES) {
        z.p[0] = grads; z.n[0] = na * sizeof(float);
        z.p[1] = metrics; z.n[1] = sizeof(double);
        z.p[2] = metrics + 2; z.n[2] = 14 * sizeof(double);
        z.p[3] = ws.pl2; z.n[3] = actor_acc;
    } else if (part == MB_CRITIC) {
        z.p[0] = grads ? grads + na : nullptr; z.n[0] = nc * sizeof(float);
        z.p[1] = metrics + 1; z.n[1] = sizeof(double);
        z.p[2] = ws.cpl2; z.n[2] = critic_acc;
    }
    return z;
}

extern "C" int dppo_ppo_clear_ranges(const dppo_dims* d, int precision, int batch_rows, void* workspace,
                                     double* metrics, int part, void** ptrs, size_t* bytes, int* count) {
    Dims D;
    int rc = dppo_check_dims(d, &D);
    if (rc) return rc;
    DPPO_CHECK(dppo_prec_ok(precision), "bad precision %d", precision);
    DPPO_CHECK(workspace && metrics && ptrs && bytes && count && batch_rows > 0, "dppo_ppo_clear_ranges: bad arguments");
    DPPO_CHECK(part == 1 || part == 2 || part == 3 || part == 4, "dppo_ppo_clear_ranges: part must be 1, 2, 3 or 4");
    DPPO_CHECK(D.KF <= PPO_MAX_BUCKETS, "dppo_ppo_clear_ranges: ft_denoising_steps %d > %d", D.KF, PPO_MAX_BUCKETS);
    const PpoWorkspace ws = make_ppo_workspace(D, precision, batch_rows, (uint8_t*)workspace);
    const ZeroArgs z = minibatch_zero_args(D, critic_net(D), ws, nullptr, metrics, (MbPart)part);
    int n = 0;
    for (int r = 1; r < 4; ++r)
        if (z.p[r]) { ptrs[n] = z.p[r]; bytes[n] = z.n[r]; ++n; }
    *count = n;
    return DPPO_OK;
}
// the same for a critic with the given attributes. A layer-normed critic's dgamma / dbeta are accumulated in the
// gradient buffer's tail, which DPPO_STEP_CLEAR_GRADS clears with the range it steps: the ranges reported here
// (metrics and workspace accumulators) are the same ones
extern "C" int dppo_ppo_clear_ranges_ln(const dppo_dims* d, int precision, int critic_head, int critic_layernorm,
                                        int batch_rows, void* workspace, double* metrics, int part, void** ptrs,
                                        size_t* bytes, int* count) {
    DPPO_CHECK(dppo_head_ok(critic_head), "dppo_ppo_clear_ranges_ln: bad head %d (DPPO_HEAD_RESIDUAL or DPPO_HEAD_PLAIN)", critic_head);
    DPPO_CHECK(dppo_ln_ok(critic_layernorm), "dppo_ppo_clear_ranges_ln: bad layernorm %d (DPPO_LN_OFF or DPPO_LN_ON)",
               critic_layernorm);
    return dppo_ppo_clear_ranges(d, precision, batch_rows, workspace, metrics, part, ptrs, bytes, count);
}

// The weight gradients of one network are one grouped dW launch. No m-chunk under 768 rows in the PPO
// update: at small minibatches (6,250 rows, an 8-GPU rank's share) thinner chunks cost more in
// partial-tile atomics than they gain in parallelism (0.177 -> 0.154 ms per minibatch; more, thinner
// chunks measured slower on the emulated 8-rank line too, profiles/r05z_dw_chunks_ab.txt)
constexpr int PPO_MIN_CHUNK_ROWS = 768;
constexpr int PRETRAIN_MIN_CHUNK_ROWS = 64;

// The problems of the grouped dW launches (the launches and dppo_ppo_plan both build them here; the plan
// query passes a workspace without a base and null gradients, and reads the shapes only)
static float* grad_at(float* g, size_t off) { return g ? g + off : nullptr; }
// the actor's: PPO (the in-layer's bias and time-MLP gradients from the one-hot bucket rows) or
// pretraining (those come from K bucket sums, seg_reduce + time_bwd)
// plain (DPPO_HEAD_PLAIN image): u2^T dy IS W_out's gradient and goes straight to its region; the l2 region
// keeps the zeros of the minibatch's zeroing (no factored form to defer)
static void actor_dw_items(const Dims& D, const PpoWorkspace& ws, float* ga, bool pretrain, bool l2_def, DWItem (&it)[4],
                           bool plain = false) {
    const FlatOffsets FA = make_flat_offsets(actor_net(D));
    it[0] = pretrain ? DWItem{ws.a0T, D.IN, ws.dh1T, D.H, grad_at(ga, FA.in_w), EXTRA_NONE, nullptr}
                     : DWItem{ws.a0T, D.IN, ws.dh1T, D.H, grad_at(ga, FA.in_w), EXTRA_ONEHOT, ws.gseg, D.KF};
    it[1] = DWItem{ws.u1T, D.H, ws.dh2T, D.H, grad_at(ga, FA.l1_w), EXTRA_ONES, grad_at(ga, FA.l1_b)};
    it[2] = DWItem{ws.u2T, D.H, ws.dyT, D.XD, plain ? grad_at(ga, FA.out_w) : (l2_def ? grad_at(ga, FA.l2_w) : ws.pl2),
                   EXTRA_NONE, nullptr};   // l2 through the out layer (plain: W_out itself)
    // out through the fold (out_back). Plain: nothing reads pa0 (no out_back runs); the product is kept for its
    // EXTRA_ONES column sum, db_out, at the cost of one unused [IN][XD] GEMM per minibatch
    it[3] = DWItem{ws.a0T, D.IN, ws.dyT, D.XD, ws.pa0, EXTRA_ONES, grad_at(ga, FA.out_b)};
}
// the critic's. plain (DPPO_HEAD_PLAIN image): problem 2 is the true product cu2T^T cdh3T -> l2_w with its column
// sums -> l2_b, an HC x HC problem like problem 1 (cpl2 is not written: the out layer reads mish(h3), so there is
// no factored form), and ch3T holds u3
static void critic_dw_items(const Dims& D, const PpoWorkspace& ws, float* gc, DWItem (&it)[4], bool plain = false) {
    const FlatOffsets FC = make_flat_offsets(critic_net(D));
    it[0] = DWItem{ws.csT, D.SD, ws.cdh1T, D.HC, grad_at(gc, FC.in_w), EXTRA_ONES, grad_at(gc, FC.in_b)};
    it[1] = DWItem{ws.cu1T, D.HC, ws.cdh2T, D.HC, grad_at(gc, FC.l1_w), EXTRA_ONES, grad_at(gc, FC.l1_b)};
    it[2] = plain ? DWItem{ws.cu2T, D.HC, ws.cdh3T, D.HC, grad_at(gc, FC.l2_w), EXTRA_ONES, grad_at(gc, FC.l2_b)}
                  : DWItem{ws.cu2T, D.HC, ws.cdvT, 1, ws.cpl2, EXTRA_NONE, nullptr};
    it[3] = DWItem{ws.ch3T, D.HC, ws.cdvT, 1, grad_at(gc, FC.out_w), EXTRA_ONES, grad_at(gc, FC.out_b)};
}

extern "C" int dppo_ppo_plan(const dppo_dims* d, int precision, int rows, int mode, int* out) {
    return dppo_ppo_plan_act(d, precision, DPPO_ACT_RELU, rows, mode, out);
}

extern "C" int dppo_ppo_plan_act(const dppo_dims* d, int precision, int activation, int rows, int mode, int* out) {
    Dims D;
    int rc = dppo_check_dims(d, &D);
    if (rc) return rc;
    DPPO_CHECK(dppo_prec_ok(precision), "bad precision %d", precision);
    DPPO_CHECK(dppo_act_ok(activation), "dppo_ppo_plan_act: bad activation %d", activation);
    DPPO_CHECK(out && rows > 0, "dppo_ppo_plan: bad arguments");
    DPPO_CHECK(mode == DPPO_PLAN_TRAIN || mode == DPPO_PLAN_PRETRAIN || mode == DPPO_PLAN_LOGPROB,
               "dppo_ppo_plan: mode must be 0 (train), 1 (pretrain) or 2 (logprob)");
    const PpoWorkspace ws = make_ppo_workspace(D, precision, rows, nullptr);
    // the row counts launch_actor_rowtile sees: the 64-padded images, or the log-prob pass's rows as given
    const ActorTilePlan t = actor_tile_plan(precision, D.H, D.XD, mode == DPPO_PLAN_LOGPROB ? (int64_t)rows : (int64_t)ws.ldm,
                                            activation);
    out[0] = 16 * t.mt;
    out[1] = t.waves;
    out[2] = out[3] = out[4] = out[5] = 0;
    if (mode == DPPO_PLAN_LOGPROB) return DPPO_OK;
    DWItem it[4];
    actor_dw_items(D, ws, nullptr, mode == DPPO_PLAN_PRETRAIN, false, it);
    const DWPlan pa = dw_plan(DWTile::ACTOR, it, 4, ws.ldm, mode == DPPO_PLAN_PRETRAIN ? PRETRAIN_MIN_CHUNK_ROWS : PPO_MIN_CHUNK_ROWS);
    out[2] = pa.nchunks;
    out[3] = pa.mchunk;
    if (mode == DPPO_PLAN_PRETRAIN) return DPPO_OK;
    critic_dw_items(D, ws, nullptr, it);
    const DWPlan pc = dw_plan(DWTile::CRITIC, it, 4, ws.ldm, PPO_MIN_CHUNK_ROWS);
    out[4] = pc.nchunks;
    out[5] = pc.mchunk;
    return DPPO_OK;
}

// dppo_ppo_minibatch{,_part}'s arguments (include/dppo.h), in their order
struct MinibatchArgs {
    const dppo_dims* d;
    int precision;
    const dppo_ppo_hparams* hp;
    const void* packed_ft; const void* packed_critic;
    const float *actor_params, *sched, *obs, *chains, *lp_old_mean, *advantages, *returns;
    int64_t total;
    uint64_t perm_seed;
    int epoch;
    int64_t start;
    int rows;
    const int64_t* row_index;
    const double* adv_stats;
    void* workspace;
    float* grads;
    double* metrics;
    void* stream;
};

static int ppo_minibatch_impl(const MinibatchArgs& m, MbPart part) {
    Dims D;
    int rc = dppo_check_dims(m.d, &D);
    if (rc) return rc;
    const int precision = m.precision, rows = m.rows;
    const dppo_ppo_hparams* hp = m.hp;
    DPPO_CHECK(dppo_prec_ok(precision), "bad precision %d", precision);
    DPPO_CHECK(hp && m.packed_ft && m.packed_critic && m.actor_params && m.sched && m.obs && m.chains && m.lp_old_mean &&
               m.advantages && m.returns && m.workspace && m.grads && m.metrics, "dppo_ppo_minibatch: null pointer");
    DPPO_CHECK(m.total > 0 && m.total % D.KF == 0, "dppo_ppo_minibatch: total must be a positive multiple of K'");
    DPPO_CHECK(rows > 0 && m.start >= 0, "dppo_ppo_minibatch: bad rows/start");
    DPPO_CHECK(hp->global_rows > 0, "dppo_ppo_minibatch: global_rows must be > 0");
    // the dW forms the per-t bucket sums 16 to a wave row of its 256-row tile, and gseg holds 64 rows
    if (D.KF > PPO_MAX_BUCKETS)
        return dppo_set_error(DPPO_EUNSUPPORTED, "dppo_ppo_minibatch: ft_denoising_steps %d > %d unsupported (bucket sums)",
                              D.KF, PPO_MAX_BUCKETS);
    hipStream_t s = (hipStream_t)m.stream;
    const PpoWorkspace ws = make_ppo_workspace(D, precision, rows, (uint8_t*)m.workspace);
    DPPO_CHECK(ws.total < ((size_t)1 << 31), "dppo_ppo_minibatch: workspace for %d rows exceeds 2 GiB", rows);
    // the images' attributes, read once: everything below follows these two values
    const NetSpec anet = actor_net(D, precision, dppo_image_attrs(m.packed_ft));
    const NetSpec cnet = critic_net(D, precision, dppo_image_attrs(m.packed_critic));
    SchedParams sp;
    rc = dppo_sched_lookup(D, m.sched, "dppo_ppo_minibatch", &sp);
    if (rc) return rc;
    DPPO_CHECK(!(sp.predict_x0 && (hp->flags & DPPO_PPO_LEARN_ETA)),
               "dppo_ppo_minibatch: DPPO_PPO_LEARN_ETA on an x0-prediction schedule table (DDIM requires predicting epsilon)");
    const FlatOffsets FA = make_flat_offsets(anet);
    float* ga = m.grads;
    float* gc = m.grads + FA.count;
    DPPO_CHECK(part >= MB_ACTOR && part <= MB_ACTOR_DW, "dppo_ppo_minibatch: bad part %d", (int)part);
    const bool needs_adv = part == MB_WHOLE || part == MB_ACTOR || part == MB_ACTOR_TILES;   // runs the actor's row tiles
    DPPO_CHECK(part == MB_WHOLE || m.adv_stats || !needs_adv, "dppo_ppo_minibatch_part: the actor half needs adv_stats");
    DPPO_CHECK((hp->flags & ~(DPPO_PPO_L2_DEFERRED | DPPO_PPO_LEARN_ETA | DPPO_PPO_PRECLEARED | DPPO_PPO_ADV_CLIP)) == 0,
               "dppo_ppo_minibatch: unknown flags 0x%x", hp->flags);
    // the bounds follow the moments in the caller's table: there is none to compute locally (every part: the
    // critic's half of a clipped minibatch is handed the same pointer)
    DPPO_CHECK(!(hp->flags & DPPO_PPO_ADV_CLIP) || m.adv_stats,
               "dppo_ppo_minibatch: DPPO_PPO_ADV_CLIP needs adv_stats fp64[5] {count, sum, sumsq, lo, hi}");
    DPPO_CHECK((uint64_t)m.total < ((uint64_t)1 << 32), "dppo_ppo_minibatch: %lld samples x steps exceed 2^32",
               (long long)m.total);
    const FeistelKey fk = feistel_key((uint64_t)m.total, m.perm_seed, m.epoch);
    LossHP lh;
    lh.gamma_denoising = hp->gamma_denoising; lh.clip_coef = hp->clip_ploss_coef;
    lh.clip_coef_base = hp->clip_ploss_coef_base; lh.clip_coef_rate = hp->clip_ploss_coef_rate;
    lh.min_lp_std = hp->min_logprob_std; lh.vf_coef = hp->vf_coef; lh.norm_adv = hp->norm_adv;
    lh.reward_horizon = hp->reward_horizon;
    lh.adv_clip = (hp->flags & DPPO_PPO_ADV_CLIP) != 0;
    // fp16: the backward images carry GRAD_SCALE x the gradient (fp16 range); dW divides it out
    const float gscale = dppo_grad_scale_rows(precision, hp->global_rows);
    lh.grad_scale = hp->loss_scale / (float)hp->global_rows * gscale;
    lh.eta_unscale = (hp->flags & DPPO_PPO_LEARN_ETA) ? 1.f / gscale : 0.f;
    lh.clip_vloss = hp->clip_vloss_coef > 0.f && hp->old_values ? hp->clip_vloss_coef : 0.f;
    lh.old_values = lh.clip_vloss > 0.f ? hp->old_values : nullptr;
    // the actor's l2 gradient left factored in its own grads region (include/dppo.h)
    const bool plain = anet.plain();   // no l2: nothing to defer
    const bool l2_def = (hp->flags & DPPO_PPO_L2_DEFERRED) != 0 && !plain;
    const bool cplain = cnet.plain();
    const int cln_sites = cnet.ln_sites();   // > 0: the critic's gradients end in the norms' tail

    ActorArgs aa = {};
    aa.packed = (const uint8_t*)m.packed_ft;
    aa.L = make_mlp_layout(anet);
    aa.sched = m.sched; aa.obs = m.obs; aa.chains = m.chains;
    aa.XD = D.XD; aa.SD = D.SD; aa.TD = D.TD; aa.IN = D.IN; aa.H = D.H; aa.KF = D.KF; aa.Da = D.Da; aa.TS = D.TS;
    aa.mode = ROWS_TRAIN; aa.nrows = rows; aa.fk = fk; aa.start = m.start; aa.row_index = m.row_index;
    aa.lp_old = m.lp_old_mean; aa.adv = m.advantages; aa.hp = lh; aa.ws = ws; aa.metrics = m.metrics;
    aa.x0_clip = sp.clip;

    CriticArgs ca = {};
    ca.packed = (const uint8_t*)m.packed_critic;
    ca.L = make_mlp_layout(cnet);
    ca.obs = m.obs; ca.SD = D.SD; ca.HC = D.HC; ca.KF = D.KF; ca.mode = ROWS_TRAIN; ca.nrows = rows;
    ca.fk = fk; ca.start = m.start; ca.row_index = m.row_index; ca.returns = m.returns; ca.hp = lh; ca.ws = ws;
    ca.metrics = m.metrics;
    ca.gln = cln_sites ? gc + make_flat_offsets(cnet).ln : nullptr;
    ca.ln_unscale = 1.f / gscale;

    // Every row tile this part runs must have an instantiation before anything is launched: a geometry
    // the dispatch rejects leaves the gradients, the metrics and the stream's sample counts (which the
    // critic's last launch re-zeroes) as they were
    if (part != MB_CRITIC && part != MB_ACTOR_DW) {
        rc = launch_actor_rowtile(aa, anet, s, true);
        if (rc) return rc;
    }
    if (part == MB_CRITIC || part == MB_WHOLE) {
        rc = launch_critic_rowtile(ca, cnet, s, true);
        if (rc) return rc;
    }
    if (part != MB_CRITIC && part != MB_ACTOR_TILES) {   // the parts that end in the time-MLP backward
        rc = time_bwd_check(D, D.KF);
        if (rc) return rc;
    }
    // one launch zeroes the atomically accumulated outputs of the half (or whole) being run
    // (minibatch_zero_args) unless the caller's optimizer step already did (DPPO_PPO_PRECLEARED).
    // Few workgroups: the split update runs this while the other stream's row tiles hold most CUs,
    // and a 256-block grid waited ~25 us for slots. MB_ACTOR_DW continues the actor half whose
    // MB_ACTOR_TILES zeroed its outputs
    if (part != MB_ACTOR_DW && !(hp->flags & DPPO_PPO_PRECLEARED)) {
        DppoKtScope kt(KT_ZERO, s);
        rc = launch_zero(minibatch_zero_args(D, cnet, ws, m.grads, m.metrics, part), 16, s);
        if (rc) return rc;
    }
    const double* stats = m.adv_stats;
    if (!stats && needs_adv) {
        const int blocks = dppo_cdiv(rows, 256) < 512 ? dppo_cdiv(rows, 256) : 512;
        hipLaunchKernelGGL(adv_stats_kernel, dim3(blocks), dim3(256), 0, s, m.advantages, fk, D.KF, m.start, rows,
                           m.row_index, ws.stats);
        DPPO_HIP(hipGetLastError());
        stats = ws.stats;
    }
    aa.adv_stats = stats;
    // the critic's half on stream st: its distinct samples (sample-weighted value loss,
    // crit_rows_kernel), its row tiles, its dW (on the small ring, beside the actor's tail) and its
    // l2 gradient, which also zeroes the sample counts (a plain critic: the same last launch with the factored
    // product off, the dW formed l2's gradient)
    auto critic_half = [&](hipStream_t st) -> int {
        uint32_t* crit_cnt = nullptr;
        if (crit_dedup()) {
            const int rc_ = crit_count_scratch(m.total / D.KF, st, &crit_cnt);
            if (rc_) return rc_;
            const int blocks = dppo_cdiv(rows, 256) < 512 ? dppo_cdiv(rows, 256) : 512;
            DppoKtScope kt(KT_CRIT_ROWS, st);
            hipLaunchKernelGGL(crit_rows_kernel, dim3(blocks), dim3(256), 0, st, m.row_index, m.start, rows, fk, D.KF,
                               crit_cnt, ws.crow_n, ws.crow_cnt);
            DPPO_HIP(hipGetLastError());
            ca.crow_n = ws.crow_n; ca.crow_mult = crit_cnt; ca.crow_cnt = ws.crow_cnt;
        }
        int rc_ = launch_critic_rowtile(ca, cnet, st);
        if (rc_) return rc_;
        DWItem items[4];
        critic_dw_items(D, ws, gc, items, cplain);
        {
            DppoKtScope kt(KT_DW_CRITIC, st);
            rc_ = launch_dw(DWTile::CRITIC, precision, items, 4, ws, 1.f / gscale, ca.crow_cnt, PPO_MIN_CHUNK_ROWS, st);
        }
        if (rc_) return rc_;
        return launch_critic_l2_back(D, precision, ws, m.packed_critic, gc, crit_cnt, st, cplain);
    };
    auto actor_grads = [&]() -> int {
        DWItem items[4];
        actor_dw_items(D, ws, ga, false, l2_def, items, plain);
        DppoKtScope kt(KT_DW_ACTOR, s);
        return launch_dw(DWTile::ACTOR, precision, items, 4, ws, 1.f / gscale, nullptr, PPO_MIN_CHUNK_ROWS, s);
    };
    // after the actor's dW: the time-MLP backward, W_out's gradient and (materialised) l2's in one launch.
    // (Forking the time-MLP backward beside the dW (r05, profiles/r05y_tb_fork_ab.txt) and running it
    // inside a one-launch actor step (r06, profiles/r06de_actor_tail_ab.txt) were both measured slower.)
    auto actor_tail = [&]() -> int {
        return launch_time_bwd(D, precision, ws, m.packed_ft, m.actor_params, ga, D.KF, D.TS, s, !l2_def, plain);
    };

    if (part == MB_CRITIC) return critic_half(s);
    if (part != MB_WHOLE) {   // the actor's half, or its row tiles / its weight gradients alone
        if (part != MB_ACTOR_DW) {
            rc = launch_actor_rowtile(aa, anet, s);
            if (rc) return rc;
        }
        if (part == MB_ACTOR_TILES) return DPPO_OK;
        rc = actor_grads();
        if (rc) return rc;
        return actor_tail();
    }
    // The critic is independent of the actor: its row tiles and then its weight gradients run on a
    // side stream, filling the CUs the actor's row tiles leave idle (the actor's last partial round)
    // and overlapping the critic's HBM-bound dW with the actor's tiles. Joined before the
    // actor's dW completes the minibatch. Without a side stream everything runs on the caller's.
    if (SideStream* side = side_stream()) {
        DPPO_HIP(hipEventRecord(side->fork, s));
        DPPO_HIP(hipStreamWaitEvent(side->stream, side->fork, 0));
        rc = critic_half(side->stream);
        if (rc) return rc;
        DPPO_HIP(hipEventRecord(side->join, side->stream));
        rc = launch_actor_rowtile(aa, anet, s);
        if (rc) return rc;
        rc = actor_grads();
        if (rc) return rc;
        DPPO_HIP(hipStreamWaitEvent(s, side->join, 0));
    } else {
        rc = launch_actor_rowtile(aa, anet, s);
        if (rc) return rc;
        rc = critic_half(s);
        if (rc) return rc;
        rc = actor_grads();
        if (rc) return rc;
    }
    return actor_tail();
}

extern "C" int dppo_ppo_minibatch(const dppo_dims* d, int precision, const dppo_ppo_hparams* hp,
                                  const void* packed_ft, const void* packed_critic, const float* actor_params,
                                  const float* sched, const float* obs, const float* chains, const float* lp_old_mean,
                                  const float* advantages, const float* returns, int64_t total, uint64_t perm_seed,
                                  int epoch, int64_t start, int rows, const int64_t* row_index, const double* adv_stats,
                                  void* workspace, float* grads, double* metrics, void* stream) {
    return ppo_minibatch_impl(MinibatchArgs{d, precision, hp, packed_ft, packed_critic, actor_params, sched, obs, chains,
                                            lp_old_mean, advantages, returns, total, perm_seed, epoch, start, rows,
                                            row_index, adv_stats, workspace, grads, metrics, stream}, MB_WHOLE);
}

extern "C" int dppo_ppo_minibatch_part(const dppo_dims* d, int precision, const dppo_ppo_hparams* hp,
                                       const void* packed_ft, const void* packed_critic, const float* actor_params,
                                       const float* sched, const float* obs, const float* chains,
                                       const float* lp_old_mean, const float* advantages, const float* returns,
                                       int64_t total, uint64_t perm_seed, int epoch, int64_t start, int rows,
                                       const int64_t* row_index, const double* adv_stats, void* workspace,
                                       float* grads, double* metrics, int part, void* stream) {
    DPPO_CHECK(part == 1 || part == 2 || part == 4 || part == 5,
               "dppo_ppo_minibatch_part: part must be 1 (actor), 2 (critic), 4 (actor row tiles) or 5 (actor dW)");
    return ppo_minibatch_impl(MinibatchArgs{d, precision, hp, packed_ft, packed_critic, actor_params, sched, obs, chains,
                                            lp_old_mean, advantages, returns, total, perm_seed, epoch, start, rows,
                                            row_index, adv_stats, workspace, grads, metrics, stream}, (MbPart)part);
}

// ---------------------------------------------------------------------------------------------
// pretraining loss: DiffusionModel.p_losses / q_sample (diffusion.py:179-202)
// ---------------------------------------------------------------------------------------------
// per-t bucket sums of dh1 for t in [0, nb): G[q][n] = sum over rows with seg == q of dh1T[n][row].
// One workgroup per hidden unit n; each wave bins its rows in LDS (nb <= 64), then the waves' bins
// are added in a fixed order (no global atomics: one writer per (q, n)).
template <class AT>
__global__ __launch_bounds__(256) void seg_reduce_kernel(const AT* __restrict__ dT, const int8_t* __restrict__ seg,
                                                         size_t ldm, int nb, float* __restrict__ G, int H, float scale) {
    __shared__ float bins[4][64];
    const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < 4 * 64; i += 256) (&bins[0][0])[i] = 0.f;
    __syncthreads();
    const AT* row = dT + (size_t)n * ldm;
#pragma unroll 4
    for (size_t r = tid; r < ldm; r += 256) {
        const int q = seg[r];
        if (q >= 0 && q < nb) atomicAdd(&bins[wave][q], (float)row[r]);
    }
    __syncthreads();
    if (tid < nb) G[(size_t)tid * H + n] = ((bins[0][tid] + bins[1][tid]) + (bins[2][tid] + bins[3][tid])) * scale;
}

extern "C" int dppo_pretrain_minibatch(const dppo_dims* d, int precision, const void* packed_actor, const float* actor_params,
                                       const float* sched, const float* qsched, const float* x_start, const float* cond,
                                       const int32_t* t, const float* noise, int rows, int64_t global_rows,
                                       float loss_scale, void* workspace, float* grads, double* metrics, void* stream) {
    Dims D;
    int rc = dppo_check_dims(d, &D);
    if (rc) return rc;
    DPPO_CHECK(dppo_prec_ok(precision), "bad precision %d", precision);
    DPPO_CHECK(packed_actor && actor_params && sched && qsched && x_start && cond && t && noise && workspace && grads &&
               metrics, "dppo_pretrain_minibatch: null pointer");
    DPPO_CHECK(rows > 0 && global_rows >= rows, "dppo_pretrain_minibatch: bad rows / global_rows");
    DPPO_CHECK(D.TS == 1, "dppo_pretrain_minibatch: the time-embedding table must be unstrided (time_stride 1)");
    DPPO_CHECK(D.K <= 64, "dppo_pretrain_minibatch: denoising_steps > 64 unsupported (bucket sums)");
    hipStream_t s = (hipStream_t)stream;
    const PpoWorkspace ws = make_ppo_workspace(D, precision, rows, (uint8_t*)workspace);
    DPPO_CHECK(ws.total < ((size_t)1 << 31), "dppo_pretrain_minibatch: workspace for %d rows exceeds 2 GiB", rows);
    const NetSpec anet = actor_net(D, precision, dppo_image_attrs(packed_actor));
    SchedParams sp;
    rc = dppo_sched_lookup(D, sched, "dppo_pretrain_minibatch", &sp);
    if (rc) return rc;
    const FlatOffsets FA = make_flat_offsets(anet);
    float* ga = grads;
    ActorArgs aa = {};
    aa.packed = (const uint8_t*)packed_actor;
    aa.L = make_mlp_layout(anet);
    aa.sched = sched; aa.obs = cond; aa.chains = x_start;
    aa.XD = D.XD; aa.SD = D.SD; aa.TD = D.TD; aa.IN = D.IN; aa.H = D.H; aa.KF = D.K; aa.Da = D.Da; aa.TS = 1;
    aa.mode = ROWS_PRETRAIN; aa.nrows = rows; aa.ws = ws; aa.metrics = metrics;
    aa.tsteps = t; aa.noise = noise; aa.qsched = qsched;
    // pretraining never clips (p_losses has no x_recon); the table's record picks the target
    aa.x0_clip = sp.clip; aa.x0_target = sp.predict_x0;
    // loss = mean over global_rows * XD elements of (eps - noise)^2 (diffusion.py:192)
    const float gscale = dppo_grad_scale_rows(precision, global_rows);
    aa.pre_scale = 2.f * loss_scale / ((float)global_rows * (float)D.XD) * gscale;
    rc = launch_actor_rowtile(aa, anet, s, true);   // rejected geometries leave the outputs untouched
    if (rc) return rc;
    ZeroArgs z = {};
    z.p[0] = grads; z.n[0] = FA.count * sizeof(float);
    z.p[1] = metrics; z.n[1] = 16 * sizeof(double);
    z.p[2] = ws.pl2; z.n[2] = (size_t)((const uint8_t*)ws.gseg - (const uint8_t*)ws.pl2);   // pl2 | pa0
    rc = launch_zero(z, 256, s);
    if (rc) return rc;
    rc = launch_actor_rowtile(aa, anet, s);
    if (rc) return rc;

    // the in-layer's bias and time-MLP gradients come from K bucket sums (seg_reduce + time_bwd)
    DWItem items[4];
    const bool plain = anet.plain();
    actor_dw_items(D, ws, ga, true, false, items, plain);
    rc = launch_dw(DWTile::ACTOR, precision, items, 4, ws, 1.f / gscale, nullptr, PRETRAIN_MIN_CHUNK_ROWS, s);
    if (rc) return rc;
    const float inv = 1.f / gscale;
    if (precision == DPPO_BF16)
        hipLaunchKernelGGL(seg_reduce_kernel<__bf16>, dim3(D.H), dim3(256), 0, s, (const __bf16*)ws.dh1T, ws.seg, ws.ldm,
                           D.K, ws.gseg, D.H, inv);
    else if (precision == DPPO_F16)
        hipLaunchKernelGGL(seg_reduce_kernel<_Float16>, dim3(D.H), dim3(256), 0, s, (const _Float16*)ws.dh1T, ws.seg,
                           ws.ldm, D.K, ws.gseg, D.H, inv);
    else
        hipLaunchKernelGGL(seg_reduce_kernel<float>, dim3(D.H), dim3(256), 0, s, (const float*)ws.dh1T, ws.seg, ws.ldm,
                           D.K, ws.gseg, D.H, inv);
    DPPO_HIP(hipGetLastError());
    return launch_time_bwd(D, precision, ws, packed_actor, actor_params, ga, D.K, 1, s, true, plain);
}

// ---------------------------------------------------------------------------------------------
// the behaviour-cloning term of the PPO loss (include/dppo.h dppo_bc_minibatch; diffusion_ppo.py:63-71):
// the TRAIN row tile in mode ROWS_BC over n K' rows, then the actor's dW and time-MLP backward as in
// part 1 of a minibatch
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_into_kernel(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] += src[i];
}

extern "C" int dppo_bc_minibatch(const dppo_dims* d, int precision, const void* packed_ft, const float* actor_params,
                                 const float* sched, const float* cond, const float* chains, int n,
                                 int64_t global_samples, float min_logprob_std, float coeff, float loss_scale, int flags,
                                 void* workspace, float* grads, double* metrics, void* stream) {
    Dims D;
    int rc = dppo_check_dims(d, &D);
    if (rc) return rc;
    DPPO_CHECK(dppo_prec_ok(precision), "bad precision %d", precision);
    DPPO_CHECK(packed_ft && actor_params && sched && cond && chains && workspace && grads && metrics,
               "dppo_bc_minibatch: null pointer");
    DPPO_CHECK(n >= 1, "dppo_bc_minibatch: n < 1");
    DPPO_CHECK(global_samples >= n, "dppo_bc_minibatch: global_samples < n");
    DPPO_CHECK(coeff >= 0.f, "dppo_bc_minibatch: coeff must be >= 0");   // a NaN fails the comparison too
    DPPO_CHECK(!(flags & DPPO_PPO_LEARN_ETA),
               "dppo_bc_minibatch: DPPO_PPO_LEARN_ETA is not supported (the term's derivative with respect to a "
               "learnable eta is not built)");
    DPPO_CHECK((flags & ~(DPPO_PPO_L2_DEFERRED | DPPO_BC_ACCUMULATE)) == 0, "dppo_bc_minibatch: unknown flags 0x%x", flags);
    if (D.KF > PPO_MAX_BUCKETS)
        return dppo_set_error(DPPO_EUNSUPPORTED, "dppo_bc_minibatch: ft_denoising_steps %d > %d unsupported (bucket sums)",
                              D.KF, PPO_MAX_BUCKETS);
    DPPO_CHECK((int64_t)n * D.KF < ((int64_t)1 << 31), "dppo_bc_minibatch: %d samples x steps exceed 2^31", n);
    const int rows = n * D.KF;
    hipStream_t s = (hipStream_t)stream;
    const PpoWorkspace ws = make_ppo_workspace(D, precision, rows, (uint8_t*)workspace);
    DPPO_CHECK(ws.total < ((size_t)1 << 31), "dppo_bc_minibatch: workspace for %d rows exceeds 2 GiB", rows);
    const NetSpec anet = actor_net(D, precision, dppo_image_attrs(packed_ft));
    SchedParams sp;
    rc = dppo_sched_lookup(D, sched, "dppo_bc_minibatch", &sp);
    if (rc) return rc;
    const FlatOffsets FA = make_flat_offsets(anet);
    const bool plain = anet.plain();   // no l2: nothing to defer
    const bool l2_def = (flags & DPPO_PPO_L2_DEFERRED) != 0 && !plain;
    const bool accumulate = (flags & DPPO_BC_ACCUMULATE) != 0;
    ActorArgs aa = {};
    aa.packed = (const uint8_t*)packed_ft;
    aa.L = make_mlp_layout(anet);
    aa.sched = sched; aa.obs = cond; aa.chains = chains;
    aa.XD = D.XD; aa.SD = D.SD; aa.TD = D.TD; aa.IN = D.IN; aa.H = D.H; aa.KF = D.KF; aa.Da = D.Da; aa.TS = D.TS;
    aa.mode = ROWS_BC; aa.nrows = rows; aa.ws = ws; aa.metrics = metrics;
    aa.x0_clip = sp.clip;
    aa.hp.min_lp_std = min_logprob_std;
    aa.hp.reward_horizon = D.XD / D.Da;   // unread: the term takes every element
    // bc_loss = -sum clip(lp) / (global_samples K' XD): the row tile divides a row's seed by XD itself (phase C), so
    // the launch-uniform seed is d loss / d (the row's mean clipped log-prob); fp16: times the backward seed scale
    const int64_t global_rows = global_samples * D.KF;
    const float gscale = dppo_grad_scale_rows(precision, global_rows);
    aa.hp.grad_scale = -coeff * loss_scale / ((float)global_samples * (float)D.KF) * gscale;
    rc = launch_actor_rowtile(aa, anet, s, true);   // rejected geometries leave the outputs untouched
    if (rc) return rc;
    rc = time_bwd_check(D, D.KF);
    if (rc) return rc;
    // accumulate: the tail's kernels store their tensors (in_b, the time MLP, l2 and W_out through the fold), so
    // the call's gradient is formed apart, in a scratch buffer kept per stream, and added in one launch
    float* ga = grads;
    if (accumulate) {
        rc = stream_scratch(s, SCRATCH_BC_GRAD, FA.count * sizeof(float), (void**)&ga);
        if (rc) return rc;
    }
    ZeroArgs z = {};
    z.p[0] = ga; z.n[0] = FA.count * sizeof(float);
    z.p[1] = ws.pl2;   // pl2 | pa0 | gseg's bucket rows the dW adds into, as a minibatch's actor half zeroes them
    z.n[1] = (size_t)((const uint8_t*)(ws.gseg + (size_t)dppo_cdiv(D.KF, 16) * 16 * D.H) - (const uint8_t*)ws.pl2);
    if (!accumulate) { z.p[2] = metrics + DPPO_METRIC_BC_LOGPROB; z.n[2] = sizeof(double); }
    {
        DppoKtScope kt(KT_ZERO, s);
        rc = launch_zero(z, 64, s);
        if (rc) return rc;
    }
    rc = launch_actor_rowtile(aa, anet, s);
    if (rc) return rc;
    DWItem items[4];
    actor_dw_items(D, ws, ga, false, l2_def, items, plain);
    {
        DppoKtScope kt(KT_DW_ACTOR, s);
        rc = launch_dw(DWTile::ACTOR, precision, items, 4, ws, 1.f / gscale, nullptr, PPO_MIN_CHUNK_ROWS, s);
        if (rc) return rc;
    }
    rc = launch_time_bwd(D, precision, ws, packed_ft, actor_params, ga, D.KF, D.TS, s, !l2_def, plain);
    if (rc || !accumulate) return rc;
    const size_t cnt = FA.count;
    const unsigned blocks = (unsigned)(dppo_cdiv((int)((cnt + 255) / 256), 4) < 1024 ? dppo_cdiv((int)((cnt + 255) / 256), 4) : 1024);
    hipLaunchKernelGGL(add_into_kernel, dim3(blocks), dim3(256), 0, s, grads, (const float*)ga, cnt);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}
