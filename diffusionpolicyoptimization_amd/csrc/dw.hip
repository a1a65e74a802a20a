// dw.hip — the grouped split-K weight-gradient (dW) GEMM of the PPO update and of pretraining.
#include "dppo_update.h"

// ---------------------------------------------------------------------------------------------
// grouped split-K weight-gradient GEMM:  G[k][n] += sum_m XT[k][m] * DT[n][m]
// (dW = X^T dH in Keras [in,out] layout). A workgroup (one per CU) owns a WK x 128 output tile
// (WK = 256: 8 waves, the actor's; WK = 128: 4 waves, the critic's; DWGeom) and one m-chunk; each wave holds a 64x64
// sub-tile (4x4 MFMA tiles, 64 accumulator VGPRs).
// Both operands are feature-major, so a stage of BK rows is one 128-B line per feature: the stage
// is copied global -> LDS with 16-B global_load_lds (one 1 KiB wave-instruction = 8 features) into
// a ring of RING slots, RING - 1 stages in flight: each wave waits with a counted vmcnt for
// its own copies of the oldest stage only, then one barrier (the kernel reads ~470 MB of images
// per minibatch; one stage in flight behind a vmcnt(0) barrier left it latency bound at ~2.5 TB/s).
// The LDS image is linear per wave-instruction; the bank swizzle (16-B slot = chunk ^ (feature & 7))
// is applied on the global source address, which makes the fragment reads (ds_read_b128) conflict-free.
// The k-tile-0 workgroups also produce the "extra" rows:
//   ONES   -> bias gradient  sum_m DT[n][m]
//   ONEHOT -> per-bucket sums sum_{m: seg[m]=q} DT[n][m]  (actor in-layer: in_b and d t_emb); the
//             stage's 64 seg bytes travel in the same ring slot. Wave row wr forms buckets
//             q = 16 wr .. 16 wr + 15 (nb <= 64 buckets on the 256-row tile's four wave rows; wave
//             rows past the last bucket run the plain loop)
// Partial tiles are added with fp32 atomics (one add per element per m-chunk).
// ---------------------------------------------------------------------------------------------
#define DW_MAXP 8
#define DW_TN 128            // output tile edge along N (the gradient operand's features)
// bytes per feature per stage: 128, two MFMA k-steps, 64 bf16 rows (64-B stages, twice the ring at a
// barrier per 32 rows, measured slower: fused minibatch 0.535 vs 0.515 ms; no record in profiles/)
constexpr int DW_LINE = 128;
#define DW_CPL (DW_LINE / 16)       // 16-B chunks per feature line
#define DW_FPI (64 / DW_CPL)        // features per 1 KiB wave-instruction
#define DW_BOPB (DW_TN * DW_LINE)   // the B (gradient) operand's stage image

// Output tile = WK x 128: WK = 256 (8 waves, 4x2 of 64x64; ring of 3 slots, 2 stages in flight), the
// actor's, or WK = 128 (4 waves, 2x2 of 64x64), the critic's. The kernel is bound by the latency of
// its staged loads (Little's law over the LDS ring: about 96 KiB in flight per CU), so the 256-row
// tile's 1.33x MFMAs per staged byte is what it buys (a 128-row k-tile for the actor measured 0.557
// against 0.510 ms per minibatch; profiles/r02c_dw_tile_ab.log).
// RC caps the ring (the critic's dW runs beside the actor's time-MLP backward, whose workgroup needs
// LDS on the same CU: a 3-slot WK = 128 ring, 101 KiB, leaves it room)
template <int WK, int RC = 8> struct DWGeom {
    static constexpr int W = WK / 32;                    // waves: 4 or 8
    static constexpr int AOPB = WK * DW_LINE;            // A (activation) operand's stage image
    static constexpr int SLOT = AOPB + DW_BOPB + 1024;   // A | B | the stage's seg bytes (padded)
    static constexpr int RING0 = 160 * 1024 / SLOT < 8 ? 160 * 1024 / SLOT : 8;
    static constexpr int RING = RING0 < RC ? RING0 : RC;   // ring slots (RING - 1 in flight)
    static constexpr int AI = WK / DW_FPI / W;           // A wave-instructions per wave per stage
    static constexpr int BI = DW_TN / DW_FPI / W;        // B wave-instructions per wave per stage
    static_assert(RING * SLOT <= 160 * 1024, "dW ring exceeds the CU's LDS");
};

struct DWProb {
    const void* XT; const void* DT; float* G; float* Gx;
    int Kx, N, extra, ktiles, ntiles;
    int nb;                   // ONEHOT: buckets q < nb (<= 16 per wave row of the tile)
};
struct DWArgs {
    DWProb p[DW_MAXP];
    int tile_start[DW_MAXP + 1];
    int nprob, nchunks, mchunk;
    float out_scale;          // 1 / the backward seed scale (fp16 images), 1 otherwise
    size_t ldm;
    const int8_t* seg;
    const int* rows_dev;      // non-null: only the first ceil64(*rows_dev) rows are summed (the chunk
                              // edge is recomputed on the device from that count)
};

typedef __attribute__((address_space(3))) void lds_void_t;

// extra A fragment: row q of [ones] or [one-hot(seg == q)] over EPL consecutive rows; the
// chunk's seg bytes sit in LDS (staged before the glds pipeline starts). q >= 0, so a padding
// row's seg of -1 matches no bucket
template <class P>
__device__ inline u32x4 extra_frag(int extra, int q, const int8_t* seg_lds) {
    using AT = typename P::AT;
    AT e[P::EPL];
    if (extra == EXTRA_ONES) {
#pragma unroll
        for (int i = 0; i < P::EPL; ++i) e[i] = P::cvt(1.f);
    } else {   // EPL bytes in one LDS read (8-B / 4-B aligned by construction)
        const uint64_t w = P::EPL == 8 ? *reinterpret_cast<const uint64_t*>(seg_lds)
                                       : (uint64_t)*reinterpret_cast<const uint32_t*>(seg_lds);
#pragma unroll
        for (int i = 0; i < P::EPL; ++i) e[i] = P::cvt((int)(int8_t)(w >> (8 * i)) == q ? 1.f : 0.f);
    }
    return __builtin_bit_cast(u32x4, e);
}

// 16-B slot of chunk c of feature f in a staged line: a bank swizzle that makes the fragment reads
// (ds_read_b128: 16 features x 4 chunks per wave-instruction, serviced in 4 lane groups of 16)
// conflict-free: c ^ (f & 7).
__device__ inline int dw_swz(int f, int c) { return c ^ (f & 7); }
// fragment of a staged operand: feature f (within the tile), 16-B chunk c
__device__ inline u32x4 dw_lds_frag(const uint8_t* img, int f, int c) {
    return *reinterpret_cast<const u32x4*>(img + f * DW_LINE + (dw_swz(f, c) << 4));
}

// wait until at most N of this wave's vector-memory operations are outstanding
template <int N>
__device__ inline void vm_wait() {
    static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

// the main loop, with or without the extra (bias / bucket) rows: two straight copies, so the
// register allocator sees one uniform accumulator set per loop (a data-dependent MFMA inside
// one loop made hipcc shuttle the accumulators between AGPRs and VGPRs every k-step).
// SEGLD: this wave also copies the stage's seg bytes (ONEHOT extra rows: wave row 0's waves; the
// other wave rows with buckets read them after the stage's barrier like any staged operand, and
// count only their own A and B copies in OPS).
template <class P, int WK, int RC, bool EXTRA, bool SEGLD>
__device__ __forceinline__ void dw_loop(uint8_t* smem, const DWArgs& a, const DWProb& pr, int nst, size_t m_begin,
                                        int wave, int lane, const typename P::AT* const (&srcA)[DWGeom<WK, RC>::AI],
                                        const typename P::AT* const (&srcB)[DWGeom<WK, RC>::BI],
                                        f32x4 (&acc)[4][4], f32x4 (&acce)[4]) {
    using G = DWGeom<WK, RC>;
    constexpr int BK = DW_LINE / (int)sizeof(typename P::AT);
    constexpr int OPS = G::AI + G::BI + (SEGLD ? 1 : 0);      // vector-memory ops per stage per wave
    const int wr = wave >> 1, wc = wave & 1;
    const int fr = lane & 15, cq = lane >> 4;
    auto issue = [&](int st) {
        uint8_t* base = smem + (st % G::RING) * G::SLOT;
        const size_t off = (size_t)st * BK;
#pragma unroll
        for (int i = 0; i < G::AI; ++i)
            __builtin_amdgcn_global_load_lds((void*)(srcA[i] + off), (lds_void_t*)(base + (wave + G::W * i) * 1024), 16,
                                             0, 0);
#pragma unroll
        for (int i = 0; i < G::BI; ++i)
            __builtin_amdgcn_global_load_lds((void*)(srcB[i] + off),
                                             (lds_void_t*)(base + G::AOPB + (wave + G::W * i) * 1024), 16, 0, 0);
        if constexpr (SEGLD) {   // BK seg bytes, 4 per lane (lanes past BK/4 fetch bytes nobody reads)
            const int8_t* sg = a.seg + m_begin + off + 4 * (lane < BK / 4 ? lane : 0);
            __builtin_amdgcn_global_load_lds((void*)sg, (lds_void_t*)(base + G::AOPB + DW_BOPB), 4, 0, 0);
        }
    };
#pragma unroll
    for (int p = 0; p < G::RING - 1; ++p)
        if (p < nst) issue(p);
    for (int st = 0; st < nst; ++st) {
        // this wave's copies of stage st have landed once at most (stages issued after it) * OPS
        // operations are outstanding; the barrier then covers every wave's copies, and every wave
        // has finished reading stage st - 1, whose slot the next issue reuses
        const int ahead = nst - 1 - st;
        if (ahead >= G::RING - 2) vm_wait<(G::RING - 2) * OPS>();
        else if (ahead == 1) vm_wait<OPS>();
        else vm_wait<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (st + G::RING - 1 < nst) issue(st + G::RING - 1);
        const uint8_t* imA = smem + (st % G::RING) * G::SLOT;
        const uint8_t* imB = imA + G::AOPB;
        const int8_t* seg_lds = (const int8_t*)(imB + DW_BOPB);
#pragma unroll
        for (int ks = 0; ks < DW_LINE / 64; ++ks) {
            u32x4 A[4], B[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                A[i] = dw_lds_frag(imA, wr * 64 + i * 16 + fr, ks * 4 + cq);
                B[i] = dw_lds_frag(imB, wc * 64 + i * 16 + fr, ks * 4 + cq);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = P::mma(A[i], B[j], acc[i][j]);
            if constexpr (EXTRA) {
                const u32x4 AE = extra_frag<P>(pr.extra, 16 * wr + fr, seg_lds + ks * P::KG + cq * P::EPL);
#pragma unroll
                for (int j = 0; j < 4; ++j) acce[j] = P::mma(AE, B[j], acce[j]);
            }
        }
    }
}

static int dw_device_cus() {
    static int n = [] {
        int dev = 0, c = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            c = 256;
        return c > 0 ? c : 256;
    }();
    return n;
}

template <class P, int WK, int RC>
__global__ __launch_bounds__(WK / 32 * 64) void dw_kernel(DWArgs a) {   // DWGeom::W waves
    using AT = typename P::AT;
    using G = DWGeom<WK, RC>;
    constexpr int BK = DW_LINE / (int)sizeof(AT);     // rows per stage: 64 bf16 / 32 fp32
    constexpr int EPC = 16 / (int)sizeof(AT);         // elements per 16-B chunk
    // one LDS object (a second __shared__ array can make hipcc drain the glds queue at every
    // fragment read): the ring of [A | B | seg] stage slots
    __shared__ __attribute__((aligned(1024))) uint8_t smem[G::RING * G::SLOT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // XCD-aware order: block b runs on XCD b % 8; XCD x takes the contiguous logical range
    // [x*per, (x+1)*per) of the chunk-major order, so the tiles that share one m-chunk's operand
    // slabs run together on one XCD and re-read them from its L2 instead of HBM/MALL.
    const int tiles_all = a.tile_start[a.nprob];
    const int total = tiles_all * a.nchunks;
    const int per = (total + 7) >> 3;
    const int lg = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (lg >= total) return;
    const int chunk = lg / tiles_all;
    const int tile = lg % tiles_all;
    int pi = 0;
    while (pi + 1 < a.nprob && tile >= a.tile_start[pi + 1]) ++pi;
    const DWProb& pr = a.p[pi];
    const int lt = tile - a.tile_start[pi];
    const int kt = lt / pr.ntiles, nt = lt % pr.ntiles;
    const int k_base = kt * WK, n_base = nt * DW_TN;
    const int wr = wave >> 1, wc = wave & 1;
    size_t lim = a.ldm, mchunk = (size_t)a.mchunk;
    if (a.rows_dev) {
        const size_t d64 = (size_t)(__builtin_amdgcn_readfirstlane(*a.rows_dev) + 63) / 64 * 64;
        lim = d64 < lim ? d64 : lim;
        mchunk = (lim + (size_t)a.nchunks * 64 - 1) / ((size_t)a.nchunks * 64) * 64;
    }
    const size_t m_begin = (size_t)chunk * mchunk;
    const size_t m_end = m_begin + mchunk < lim ? m_begin + mchunk : lim;
    if (m_begin >= m_end) return;
    const int nst = (int)((m_end - m_begin) / BK);
    const AT* XT = (const AT*)pr.XT;
    const AT* DT = (const AT*)pr.DT;
    const bool wg_extra = pr.extra != EXTRA_NONE && kt == 0;      // uniform over the workgroup
    // extra rows of this wave row: ONES has one (row 0), ONEHOT buckets 16 wr .. < nb
    const int xrows = pr.extra == EXTRA_ONEHOT ? pr.nb : 1;
    const bool do_extra = wg_extra && 16 * wr < xrows;
    const bool seg_ld = wg_extra && wr == 0 && pr.extra == EXTRA_ONEHOT;

    // per-lane glds sources of this wave's A and B wave-instructions (features ins*8 + lane/8)
    const AT* srcA[G::AI];
    const AT* srcB[G::BI];
#pragma unroll
    for (int i = 0; i < G::AI; ++i) {
        const int f = (wave + G::W * i) * DW_FPI + lane / DW_CPL;
        const int c = dw_swz(f, lane % DW_CPL);
        int fa = k_base + f; fa = fa < pr.Kx ? fa : pr.Kx - 1;
        srcA[i] = XT + (size_t)fa * a.ldm + m_begin + c * EPC;
    }
#pragma unroll
    for (int i = 0; i < G::BI; ++i) {
        const int f = (wave + G::W * i) * DW_FPI + lane / DW_CPL;
        const int c = dw_swz(f, lane % DW_CPL);
        int fb = n_base + f; fb = fb < pr.N ? fb : pr.N - 1;
        srcB[i] = DT + (size_t)fb * a.ldm + m_begin + c * EPC;
    }
    f32x4 acc[4][4], acce[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        zero_acc(acce[i]);
#pragma unroll
        for (int j = 0; j < 4; ++j) zero_acc(acc[i][j]);
    }
    // the other waves of an extra tile run the plain loop; the barrier count per stage is identical
    if (seg_ld) dw_loop<P, WK, RC, true, true>(smem, a, pr, nst, m_begin, wave, lane, srcA, srcB, acc, acce);
    else if (do_extra) dw_loop<P, WK, RC, true, false>(smem, a, pr, nst, m_begin, wave, lane, srcA, srcB, acc, acce);
    else dw_loop<P, WK, RC, false, false>(smem, a, pr, nst, m_begin, wave, lane, srcA, srcB, acc, acce);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n_base + wc * 64 + j * 16 + ccol(lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = k_base + wr * 64 + i * 16 + crow(lane, r);
                if (k < pr.Kx && n < pr.N) atomicAdd(pr.G + (size_t)k * pr.N + n, acc[i][j][r] * a.out_scale);
            }
        }
    if (do_extra) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n_base + wc * 64 + j * 16 + ccol(lane);
            if (n >= pr.N) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = 16 * wr + crow(lane, r);
                if (pr.extra == EXTRA_ONES) {
                    if (q == 0) atomicAdd(pr.Gx + n, acce[j][r] * a.out_scale);
                } else if (q < pr.nb) {
                    atomicAdd(pr.Gx + (size_t)q * pr.N + n, acce[j][r] * a.out_scale);
                }
            }
        }
    }
}
template <class P>
static int launch_dw_p(const DWArgs& a, DWTile tile, hipStream_t s) {
    const int tiles = a.tile_start[a.nprob];
    const int64_t blocks = 8 * (((int64_t)tiles * a.nchunks + 7) / 8);   // whole XCD rounds
    if (tile == DWTile::ACTOR)
        hipLaunchKernelGGL((dw_kernel<P, 256, 8>), dim3((unsigned)blocks), dim3(DWGeom<256>::W * 64), 0, s, a);
    else
        hipLaunchKernelGGL((dw_kernel<P, 128, 3>), dim3((unsigned)blocks), dim3(DWGeom<128, 3>::W * 64), 0, s, a);
    DPPO_HIP(hipGetLastError());
    return DPPO_OK;
}

static int dw_item_tiles(DWTile tile, const DWItem& it) {
    return dppo_cdiv(it.Kx, tile == DWTile::ACTOR ? 256 : 128) * dppo_cdiv(it.N, DW_TN);
}

DWPlan dw_plan(DWTile tile, const DWItem* items, int n_items, size_t ldm, int min_chunk_rows) {
    DWPlan p = {};
    for (int i = 0; i < n_items; ++i) p.tiles += dw_item_tiles(tile, items[i]);
    // m-chunks: about one workgroup per CU (the ring takes most of its LDS) in a single round, but no
    // chunk under min_chunk_rows rows (a multiple of 64)
    const int span = (int)ldm;
    int nch = dw_device_cus() / p.tiles;
    if (nch > span / min_chunk_rows) nch = span / min_chunk_rows;
    if (nch < 1) nch = 1;
    p.mchunk = dppo_cdiv(span, nch * 64) * 64;
    p.nchunks = dppo_cdiv(span, p.mchunk);
    return p;
}

int launch_dw(DWTile tile, int precision, const DWItem* items, int n_items, const PpoWorkspace& ws, float out_scale,
              const int* rows_dev, int min_chunk_rows, hipStream_t s) {
    DPPO_CHECK(n_items >= 1 && n_items <= DW_MAXP, "dW: %d problems in one launch", n_items);
    const int tk = tile == DWTile::ACTOR ? 256 : 128;
    for (int i = 0; i < n_items; ++i)   // one 16-bucket one-hot tile per wave row of the output tile
        DPPO_CHECK(items[i].extra != EXTRA_ONEHOT || (items[i].nb >= 1 && items[i].nb <= tk / 4),
                   "dW: %d one-hot buckets on a %d-row tile", items[i].nb, tk);
    DWArgs w = {};
    for (int i = 0; i < n_items; ++i) {
        const DWItem& it = items[i];
        DWProb& p = w.p[i];
        p.XT = it.XT; p.DT = it.DT; p.G = it.G; p.Gx = it.Gx; p.Kx = it.Kx; p.N = it.N; p.extra = it.extra; p.nb = it.nb;
        p.ktiles = dppo_cdiv(it.Kx, tk); p.ntiles = dppo_cdiv(it.N, DW_TN);
        w.tile_start[i + 1] = w.tile_start[i] + dw_item_tiles(tile, it);
    }
    w.nprob = n_items;
    w.rows_dev = rows_dev;
    w.ldm = ws.ldm;
    w.seg = ws.seg;
    w.out_scale = out_scale;
    const DWPlan plan = dw_plan(tile, items, n_items, ws.ldm, min_chunk_rows);
    w.mchunk = plan.mchunk;
    w.nchunks = plan.nchunks;
    return precision == DPPO_BF16 ? launch_dw_p<PolicyBF16>(w, tile, s)
         : precision == DPPO_F16  ? launch_dw_p<PolicyF16>(w, tile, s) : launch_dw_p<PolicyF32>(w, tile, s);
}
