// select.hip — exact per-minibatch quantiles of the advantages (the clip_advantage_*_quantile knobs of
// PPODiffusion): a multi-segment radix select, one segment per minibatch of an update phase, segments
// indexed as adv_stats_all_kernel (update.hip) indexes them.
//
// A segment's value multiset is {adv[perm_e(i) / K']: i in its window of the epoch's Feistel permutation}.
// Each value maps to an order-preserving 32-bit key; four passes of 8 bits, most significant first, narrow
// four targets per segment (the order statistics k and min(k + 1, n - 1) of q_lo and of q_hi) to their keys:
//   count (one launch over segments x chunks): every element is read once and compared against the four
//          targets' prefixes; a workgroup bins the matches in LDS (4 x 256 int) and flushes its non-zero
//          bins with integer atomics into counts[seg][4][256]. Integer sums: exact in any arrival order,
//          and a data-parallel caller SUM-all-reduces the table between count and pick.
//   pick  (one workgroup per segment, one wave per target): the bin that holds the target's remaining
//          rank extends its prefix by 8 bits; the counts are left zero for the next pass. The last pass
//          also interpolates the two bounds in fp64 and writes them (no further launch).
// 4 count + 4 pick launches (+ one memset) per update phase, none of which waits on the host.
#include <math.h>
#include "dppo_update.h"

constexpr int SEL_THREADS = DPPO_ADV_QUANTILES_BLOCK;
constexpr int SEL_MAX_CHUNKS = DPPO_ADV_QUANTILES_MAX_CHUNKS;
constexpr int SEL_MAXE = 64;      // epochs per launch (the Feistel keys travel as kernel arguments)
constexpr int SEL_STATE = 9;      // int64 per segment: {prefix, remaining rank} x 4 targets, n
static_assert(SEL_THREADS == 256, "one thread per bin, one wave per target");

struct SelectSegs {
    FeistelKey fk[SEL_MAXE];
    int nbatch, KF;
    int64_t rows_full, total;
};

// fp32 -> key with v < w <=> key(v) < key(w) (and key(-0) + 1 == key(+0)); NaN is out of scope
__device__ inline uint32_t sel_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float sel_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__global__ __launch_bounds__(256) void select_count_kernel(const float* __restrict__ adv, SelectSegs a, int pass,
                                                           const int64_t* __restrict__ state, int* __restrict__ counts) {
    __shared__ int hist[4][SEL_THREADS];
    const int m = blockIdx.y, e = m / a.nbatch, b = m % a.nbatch, tid = threadIdx.x;
    const int64_t start = (int64_t)b * a.rows_full;
    const int64_t end = start + a.rows_full < a.total ? start + a.rows_full : a.total;
    if (start + (int64_t)blockIdx.x * SEL_THREADS >= end) return;   // workgroup-uniform: nothing to bin
    const FeistelKey fk = a.fk[e];
    uint32_t pre[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        hist[t][tid] = 0;
        pre[t] = pass ? (uint32_t)state[(size_t)m * SEL_STATE + 2 * t] : 0u;
    }
    const uint32_t hi_mask = pass ? 0xFFFFFFFFu << (32 - 8 * pass) : 0u;   // the bits earlier passes fixed
    const int shift = 24 - 8 * pass;
    __syncthreads();
    for (int64_t i = start + (int64_t)blockIdx.x * SEL_THREADS + tid; i < end; i += (int64_t)gridDim.x * SEL_THREADS) {
        const uint64_t idx = minibatch_row(nullptr, (uint64_t)i, fk);
        if (idx >= fk.n) continue;
        const uint32_t key = sel_key(adv[idx / a.KF]);
        const int bin = (int)((key >> shift) & 255u);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (((key ^ pre[t]) & hi_mask) == 0u) atomicAdd(&hist[t][bin], 1);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int c = hist[t][tid];
        if (c) atomicAdd(counts + ((size_t)m * 4 + t) * 256 + tid, c);
    }
}

// Q(q) = v_k + (pos - k) (v_k1 - v_k), pos = q (n - 1), k = floor(pos), in fp64 with every rounding stated
// (numpy.quantile's linear method); equal neighbours and an integer pos return v_k itself
__device__ inline double sel_interp(double q, int64_t n, float vk, float vk1) {
#pragma clang fp contract(off)
    const double pos = q * (double)(n - 1);
    const double frac = pos - floor(pos);
    const double a = (double)vk, b = (double)vk1;
    if (frac == 0.0 || a == b) return a;
    const double d = b - a;
    const double t = frac * d;
    return a + t;
}

__global__ __launch_bounds__(256) void select_pick_kernel(int pass, double q_lo, double q_hi,
                                                          const int64_t* __restrict__ n_global, int64_t* __restrict__ state,
                                                          int* __restrict__ counts, double* __restrict__ bounds) {
    __shared__ uint32_t keys[4];
    const int m = blockIdx.x, t = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int64_t* st = state + (size_t)m * SEL_STATE;
    int4* c4 = (int4*)(counts + ((size_t)m * 4 + t) * 256);
    const int4 v = c4[lane];
    c4[lane] = make_int4(0, 0, 0, 0);   // the next pass's counts start from zero
    const int s = v.x + v.y + v.z + v.w;
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    int64_t n, rank;
    uint32_t prefix;
    if (pass == 0) {   // every element matched the empty prefix: the bins of a target sum to the segment's length
        n = n_global ? n_global[m] : (int64_t)__shfl(inc, 63, 64);
        const double q = t < 2 ? q_lo : q_hi;
        const int64_t k = n > 0 ? (int64_t)floor(q * (double)(n - 1)) : 0;
        rank = (t & 1) && k + 1 < n ? k + 1 : k;
        prefix = 0u;
        if (threadIdx.x == 0) st[8] = n;
    } else {
        n = st[8]; prefix = (uint32_t)st[2 * t]; rank = st[2 * t + 1];
    }
    const int64_t exc = (int64_t)(inc - s);
    if (n > 0 && exc <= rank && rank < (int64_t)inc) {   // this lane's four bins hold the target
        int r = (int)(rank - exc), bin = 4 * lane;
        if (r >= v.x) { r -= v.x; ++bin;
            if (r >= v.y) { r -= v.y; ++bin;
                if (r >= v.z) { r -= v.z; ++bin; } } }
        prefix |= (uint32_t)bin << (24 - 8 * pass);
        st[2 * t] = (int64_t)prefix;
        st[2 * t + 1] = (int64_t)r;
        keys[t] = prefix;
    }
    if (pass != 3) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        double lo = -INFINITY, hi = INFINITY;   // an empty segment clips nothing
        if (n > 0) {
            lo = sel_interp(q_lo, n, sel_value(keys[0]), sel_value(keys[1]));
            hi = sel_interp(q_hi, n, sel_value(keys[2]), sel_value(keys[3]));
        }
        bounds[2 * (size_t)m] = lo;
        bounds[2 * (size_t)m + 1] = hi;
    }
}

static size_t sel_counts_bytes(int64_t n_seg) { return dppo_align256((size_t)n_seg * 4 * 256 * sizeof(int)); }

extern "C" size_t dppo_ppo_adv_quantiles_workspace_bytes(int n_epochs, int n_batch) {
    if (n_epochs <= 0 || n_batch <= 0) return 0;
    const int64_t n_seg = (int64_t)n_epochs * n_batch;
    return sel_counts_bytes(n_seg) + (size_t)n_seg * SEL_STATE * sizeof(int64_t);
}

extern "C" int dppo_ppo_adv_quantiles_count(const float* advantages, int64_t total, int K_ft, uint64_t perm_seed,
                                            int epoch0, int n_epochs, int64_t rows_full, int n_batch, int pass,
                                            const int64_t* state, int* counts, void* stream) {
    DPPO_CHECK(advantages && state && counts && total > 0 && K_ft > 0 && rows_full > 0 && n_batch > 0 && n_epochs > 0,
               "dppo_ppo_adv_quantiles_count: bad args");
    DPPO_CHECK(pass >= 0 && pass < 4, "dppo_ppo_adv_quantiles_count: pass %d outside [0, 4)", pass);
    DPPO_CHECK(n_epochs <= SEL_MAXE, "dppo_ppo_adv_quantiles_count: at most %d epochs", SEL_MAXE);
    DPPO_CHECK((uint64_t)total < ((uint64_t)1 << 32), "dppo_ppo_adv_quantiles_count: total exceeds 2^32");
    DPPO_CHECK((int64_t)n_epochs * n_batch <= 65535, "dppo_ppo_adv_quantiles_count: more than 65535 segments");
    // the bins and the pick's scan are int32
    DPPO_CHECK((rows_full < total ? rows_full : total) < ((int64_t)1 << 31),
               "dppo_ppo_adv_quantiles_count: a segment of 2^31 rows or more");
    hipStream_t s = (hipStream_t)stream;
    SelectSegs a = {};
    for (int e = 0; e < n_epochs; ++e) a.fk[e] = feistel_key((uint64_t)total, perm_seed, epoch0 + e);
    a.nbatch = n_batch; a.KF = K_ft; a.rows_full = rows_full; a.total = total;
    const int64_t seg = rows_full < total ? rows_full : total;
    const int64_t bx = (seg + SEL_THREADS - 1) / SEL_THREADS;
    const int chunks = bx < SEL_MAX_CHUNKS ? (int)bx : SEL_MAX_CHUNKS;
    hipLaunchKernelGGL(select_count_kernel, dim3(chunks, n_epochs * n_batch), dim3(SEL_THREADS), 0, s, advantages, a,
                       pass, state, counts);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

extern "C" int dppo_ppo_adv_quantiles_pick(int n_epochs, int n_batch, double q_lo, double q_hi, int pass,
                                           const int64_t* n_global, int64_t* state, int* counts, double* bounds,
                                           void* stream) {
    DPPO_CHECK(state && counts && n_batch > 0 && n_epochs > 0, "dppo_ppo_adv_quantiles_pick: bad args");
    DPPO_CHECK(pass >= 0 && pass < 4, "dppo_ppo_adv_quantiles_pick: pass %d outside [0, 4)", pass);
    DPPO_CHECK(bounds || pass != 3, "dppo_ppo_adv_quantiles_pick: the last pass writes the bounds");
    DPPO_CHECK(q_lo >= 0.0 && q_lo < q_hi && q_hi <= 1.0, "dppo_ppo_adv_quantiles_pick: need 0 <= q_lo < q_hi <= 1");
    hipLaunchKernelGGL(select_pick_kernel, dim3(n_epochs * n_batch), dim3(SEL_THREADS), 0, (hipStream_t)stream, pass,
                       q_lo, q_hi, n_global, state, counts, bounds);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

extern "C" int dppo_ppo_adv_quantiles_all(const float* advantages, int64_t total, int K_ft, uint64_t perm_seed,
                                          int epoch0, int n_epochs, int64_t rows_full, int n_batch, double q_lo,
                                          double q_hi, void* workspace, double* bounds, void* stream) {
    DPPO_CHECK(advantages && workspace && bounds && total > 0 && K_ft > 0 && rows_full > 0 && n_batch > 0 && n_epochs > 0,
               "dppo_ppo_adv_quantiles_all: bad args");
    DPPO_CHECK(n_epochs <= SEL_MAXE, "dppo_ppo_adv_quantiles_all: at most %d epochs", SEL_MAXE);
    DPPO_CHECK((uint64_t)total < ((uint64_t)1 << 32), "dppo_ppo_adv_quantiles_all: total exceeds 2^32");
    DPPO_CHECK((int64_t)n_epochs * n_batch <= 65535, "dppo_ppo_adv_quantiles_all: more than 65535 segments");
    DPPO_CHECK((rows_full < total ? rows_full : total) < ((int64_t)1 << 31),
               "dppo_ppo_adv_quantiles_all: a segment of 2^31 rows or more");
    DPPO_CHECK(q_lo >= 0.0 && q_lo < q_hi && q_hi <= 1.0, "dppo_ppo_adv_quantiles_all: need 0 <= q_lo < q_hi <= 1");
    const int64_t n_seg = (int64_t)n_epochs * n_batch;
    int* counts = (int*)workspace;
    int64_t* state = (int64_t*)((uint8_t*)workspace + sel_counts_bytes(n_seg));
    DPPO_HIP(hipMemsetAsync(counts, 0, sel_counts_bytes(n_seg), (hipStream_t)stream));
    for (int pass = 0; pass < 4; ++pass) {
        int rc = dppo_ppo_adv_quantiles_count(advantages, total, K_ft, perm_seed, epoch0, n_epochs, rows_full, n_batch,
                                              pass, state, counts, stream);
        if (rc) return rc;
        rc = dppo_ppo_adv_quantiles_pick(n_epochs, n_batch, q_lo, q_hi, pass, nullptr, state, counts, bounds, stream);
        if (rc) return rc;
    }
    return DPPO_OK;
}
