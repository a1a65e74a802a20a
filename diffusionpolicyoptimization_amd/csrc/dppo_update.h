// dppo_update.h — host-side declarations shared by the PPO update's translation units
// (dw.hip, backward_tail.hip, optimizer.hip, update.hip).
#pragma once
#include "dppo_ppo.h"

// ---- dw.hip: the grouped split-K weight-gradient GEMM -------------------------------------------
enum { EXTRA_NONE = 0, EXTRA_ONES = 1, EXTRA_ONEHOT = 2 };
// one problem of a grouped launch: G[Kx][N] += XT^T DT over the workspace rows, Gx its extra rows
// (EXTRA_ONEHOT: nb bucket rows Gx[q][N], q < nb <= 64 on the actor's tile; buckets past nb are not
// written)
struct DWItem {
    const void* XT; int Kx;
    const void* DT; int N;
    float* G;
    int extra;
    float* Gx;
    int nb;
};
// the output tile and LDS ring of a launch: the actor's 256-row tile on the full ring, or the critic's
// 128-row tile on a 3-slot ring (it runs beside the actor's time-MLP backward, which needs LDS too)
enum class DWTile { ACTOR, CRITIC };
// Launches the items (at most 8) as one kernel over the workspace's ldm rows, in m-chunks of at least
// min_chunk_rows rows, about one workgroup per CU. out_scale multiplies the outputs (1 / the backward
// seed scale); rows_dev, when non-null, is a device-side row count that caps the rows summed.
int launch_dw(DWTile tile, int precision, const DWItem* items, int n_items, const PpoWorkspace& ws, float out_scale,
              const int* rows_dev, int min_chunk_rows, hipStream_t s);
// The m-chunks launch_dw cuts the ldm rows into for these items (host arithmetic only: launch_dw and the
// plan query, dppo_ppo_plan, both take them from here): output tiles over all items, chunks, rows per
// chunk (a multiple of 64; the last chunk is shorter when nchunks * mchunk > ldm)
struct DWPlan { int tiles, nchunks, mchunk; };
DWPlan dw_plan(DWTile tile, const DWItem* items, int n_items, size_t ldm, int min_chunk_rows);

// ---- backward_tail.hip: what follows the dW launches -------------------------------------------
// after the actor's dW: the time-MLP backward over nb buckets at t = q * TS (the bucket sums in
// ws.gseg), W_out's gradient (out_back) and, with l2_back, l2's from ws.pl2, in one launch; without
// l2_back the l2 gradient stays factored in its own region of ga (DPPO_PPO_L2_DEFERRED); plain (a
// DPPO_HEAD_PLAIN image): the time-MLP backward alone (the dW left W_out's gradient in place, l2's is zero)
int launch_time_bwd(const Dims& D, int precision, const PpoWorkspace& ws, const void* packed_actor,
                    const float* actor_params, float* ga, int nb, int TS, hipStream_t s, bool l2_back = true,
                    bool plain = false);
// host check only: DPPO_EUNSUPPORTED ("time_bwd needs %zu B LDS") where launch_time_bwd's workgroup
// over nb buckets would not fit a CU's 160 KiB; callers ask before their first launch
int time_bwd_check(const Dims& D, int nb);
// the critic's l2 weight gradient from ws.cpl2 (N = 1); with zcnt, the launch also zeroes the
// minibatch's sample counts zcnt[ws.crow_n[r]], r < *ws.crow_cnt. plain (a DPPO_HEAD_PLAIN critic image, whose
// l2 gradient the dW formed): the same launch without the product, the zeroing alone
int launch_critic_l2_back(const Dims& D, int precision, const PpoWorkspace& ws, const void* packed_critic, float* gc,
                          uint32_t* zcnt, hipStream_t s, bool plain = false);

// ---- update.hip ---------------------------------------------------------------------------------
// zero up to 4 byte ranges (4-B aligned, sizes multiples of 4) in one launch of `blocks` workgroups
struct ZeroArgs { void* p[4]; size_t n[4]; };
int launch_zero(const ZeroArgs& z, unsigned blocks, hipStream_t s);
// Per-(device, stream) device scratch that kernels leave zeroed between uses, created zeroed on first
// use and kept for the process (one process-wide table, update.hip)
// (SCRATCH_BC_GRAD: dppo_bc_minibatch's accumulate form zeroes its own, the call's gradient before it is added)
enum { SCRATCH_TICKET = 0, SCRATCH_CRIT_COUNT = 1, SCRATCH_BC_GRAD = 2 };
int stream_scratch(hipStream_t s, int kind, size_t bytes, void** out);
