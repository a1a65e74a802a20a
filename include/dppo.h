/*
 * dppo.h — C ABI of libdppo_hip.so, the MI355X (gfx950) DPPO fine-tuning hot path.
 *
 * The TF reference has no native boundary: its hot path is TF/Keras/TFP ops called from Python.
 * Each entry point below replaces one reference interface (cited file:line, relative to the
 * reference repo root); the Python layer diffusionpolicyoptimization_amd/ (same class names and
 * kwargs as the reference) is the drop-in, and it binds these symbols with ctypes
 * (diffusionpolicyoptimization_amd/_lib.py). INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer argument is DEVICE memory owned by the caller unless it says "host";
 *   - every call is asynchronous on `stream` (a hipStream_t; 0 = null stream) and allocates
 *     nothing; scratch comes from a caller-owned workspace sized by the *_workspace_bytes query;
 *   - return 0 on success, a DPPO_E* code otherwise; dppo_last_error() gives the message
 *     (thread-local); no C++ exception crosses the ABI;
 *   - precision: DPPO_F32 = f32-input MFMA (exact fp32 products, the parity mode),
 *     DPPO_BF16 = bf16 MFMA with fp32 accumulation and an fp32 DDPM/loss epilogue, or
 *     DPPO_F16 = the same with fp16 operands (BASELINE config 5; the backward images carry the
 *     gradient times 4096 for fp16's range, removed exactly in the fp32 weight gradients);
 *   - flat parameter layout (fp32, Keras kernel [in,out] row-major, then bias [out]):
 *       actor : time_w1[TD,2TD] time_b1[2TD] time_w2[2TD,TD] time_b2[TD]
 *               in_w[XD+TD+SD, H] in_b[H] l1_w[H,H] l1_b[H] l2_w[H,H] l2_b[H] out_w[H,XD] out_b[XD]
 *       critic: in_w[SD,HC] in_b[HC] l1_w[HC,HC] l1_b[HC] l2_w[HC,HC] l2_b[HC] out_w[HC,1] out_b[1]
 *     with XD = horizon*action_dim, SD = cond_steps*obs_dim, TD = time_dim.
 *     A plain-head actor (DPPO_HEAD_PLAIN, dppo_pack_actor_head) keeps this layout with the l2_w / l2_b
 *     range unused: zero on creation, its gradient written as zero, so it stays zero under AdamW.
 */
#ifndef DPPO_H
#define DPPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 13: the actor image (dppo_actor_packed_bytes) holds the row tiles' l2 fold segments; a pack or
 * fused step of an actor image is followed by the fold launch (DPPO_STEP_FUSED_PACK above).
 * ABI 15: dppo_actor_step and DPPO_PPO_TIME_BWD_IN_STEP (ABI 12) are removed: the one-launch actor
 * tail was measured slower than the minibatch's time-MLP backward + the fused step;
 * the actor's one-launch step is dppo_optimizer_step_ex | DPPO_STEP_FUSED_PACK over its range. */
#define DPPO_ABI_VERSION 15

#if defined(__GNUC__)
#define DPPO_API __attribute__((visibility("default")))
#else
#define DPPO_API
#endif

enum { DPPO_OK = 0, DPPO_EINVAL = 1, DPPO_EHIP = 2, DPPO_EUNSUPPORTED = 3 };
enum { DPPO_F32 = 0, DPPO_BF16 = 1, DPPO_F16 = 2 };
enum { DPPO_ADAMW_KERAS = 0, DPPO_ADAMW_TORCH = 1 };
/* ABI 7: OR'd into dppo_optimizer_step's mode. The actor image is packed without the split
 * sampler's tables (W_XS, FOLD/ROUT, TIN, B_OUT2: nothing the PPO row tiles read) and marked stale;
 * the next sampler launch on that image (dppo_sample, dppo_sample_step, dppo_rollout_enqueue*)
 * re-derives them on its own stream first, or dppo_refresh_sampler_tables does it explicitly. The
 * actor parameters must stay allocated and unchanged until then (they are read at the refresh). */
enum { DPPO_STEP_DEFER_SAMPLER_TABLES = 0x100 };
/* ABI 8, OR'd into dppo_optimizer_step's mode: the actor's l2 gradient in grads is in the factored
 * form of DPPO_PPO_L2_DEFERRED; AdamW forms it from pl2, db_out and the actor image's rnd(W_out)
 * (needs actor_params == params and packed_actor). */
enum { DPPO_STEP_L2_FROM_PL2 = 0x200 };
/* ABI 11, OR'd into dppo_optimizer_step's mode. DPPO_STEP_FUSED_PACK: AdamW and the pack in ONE
 * launch when the step packs a single network whose flat parameters are exactly the range: each
 * element's thread stores its updated value into its slots of the images (the values the pack writes).
 * For an actor the launch leaves the split sampler's tables to the next sampler launch (or
 * dppo_refresh_sampler_tables), as after DPPO_STEP_DEFER_SAMPLER_TABLES; a second, small launch on the
 * same stream re-derives the cross-element segments the row tiles read (the l2 fold M = W_l2 W_out,
 * M0 = W_in W_out, the folded out bias and the TEMB table), as it does after every pack of an actor
 * image. The image must have been fully packed once before (its zero padding is not rewritten). Any
 * other combination runs the two launches.
 * DPPO_STEP_CLEAR_GRADS (dppo_optimizer_step_ex only): the step zeroes the range's gradients after
 * reading them, and the byte ranges given to dppo_optimizer_step_ex after every read of the launch
 * (by its last workgroup), so the next minibatch of this range may skip its zeroing launch
 * (DPPO_PPO_PRECLEARED). */
enum { DPPO_STEP_FUSED_PACK = 0x400, DPPO_STEP_CLEAR_GRADS = 0x800 };

/* Model / schedule dimensions (cfg keys of cfg/gym/finetune/hopper-v2/ft_ppo_diffusion_mlp.yaml:18-25,78-110). */
typedef struct dppo_dims {
    int32_t obs_dim;          /* Do */
    int32_t action_dim;       /* Da */
    int32_t horizon_steps;    /* Ta */
    int32_t cond_steps;       /* To */
    int32_t time_dim;         /* TD (16) */
    int32_t actor_hidden;     /* H  (512), multiple of 128 */
    int32_t critic_hidden;    /* HC (256), multiple of 128 */
    int32_t denoising_steps;  /* sampling steps: K (20) for DDPM, ddim_steps S (10) for DDIM */
    int32_t ft_denoising_steps; /* K' (10) */
    int32_t time_stride;      /* diffusion time of sampling row r = r * time_stride: 1 (or 0) for DDPM,
                                 K / S for DDIM (diffusion.py:76-82 uniform discretisation); since ABI 2 */
} dppo_dims;

/* Supported geometry of the update entries (dppo_logprob, dppo_critic_forward, dppo_ppo_minibatch,
 * dppo_pretrain_minibatch). The dimension check every entry shares is wider than what the row tiles
 * instantiate (it takes hidden widths 128/256/384/512, time_dim <= 64, any input width); the rest is
 * refused with DPPO_EUNSUPPORTED and the dispatch's message before anything is launched, outputs
 * untouched. With in = horizon_steps*action_dim + time_dim + cond_steps*obs_dim:
 *   actor, fp32:         actor_hidden 512;        33 <= in <= 64
 *   actor, bf16 / fp16:  actor_hidden 512, or 256 with horizon_steps*action_dim <= 16; in <= 128
 *   critic, fp32:        critic_hidden 256;       cond_steps*obs_dim <= 32
 *   critic, bf16 / fp16: critic_hidden 256;       cond_steps*obs_dim <= 64
 *   all: horizon_steps*action_dim <= 32, time_dim <= 32 (the image's fold), ft_denoising_steps <= 64
 *   in dppo_ppo_minibatch{,_part} (bucket sums: 16 per wave row of the dW's 256-row tile; above it
 *   "ft_denoising_steps %d > 64 unsupported (bucket sums)"), denoising_steps <= 64 in
 *   dppo_pretrain_minibatch.
 *   LDS that grows with K' (K in pretraining): the 64-row actor tile (bf16 / fp16, actor_hidden 512,
 *   horizon_steps*action_dim <= 16, minibatches of at least 64 x CU-count rows) keeps K' rows of time
 *   embeddings and schedule (K' (4 time_dim + 32) bytes) beside its activation tiles: hopper's
 *   geometry needs 161,616 + 96 K' bytes, so K' <= 23 fits the CU's 160 KiB there and K' >= 24 is
 *   refused with "actor row tile needs %zu B LDS" (the 32-row tile of smaller minibatches and of fp32
 *   takes every K' <= 64). The time-MLP backward's workgroup needs at most 147,712 B at the accepted
 *   geometries (time_dim 32, actor_hidden 512, K' 64), so it refuses none of them ("time_bwd needs
 *   %zu B LDS" otherwise, also before the first launch).
 * An actor rejection fails dppo_logprob, dppo_pretrain_minibatch and dppo_ppo_minibatch; a critic
 * rejection dppo_critic_forward and dppo_ppo_minibatch. tests/test_update_surface_gpu.py pins the
 * table, tests/test_update_ft_steps_gpu.py its K' lines.
 * A Mish actor image (dppo_pack_actor_act) is accepted and refused on the same lines, with the same
 * messages. Its row tile keeps the pre-activations h1, h2 in registers from the forward to the backward
 * (mish' cannot be read off the stored activation as relu' is), so it runs the 32-row tile on 8 waves at
 * every row count and precision: the 64-row tile of large 2-byte minibatches and the fp32 16-wave tile
 * (4 waves per SIMD, 128 registers) have no room for them and are not instantiated for Mish, and neither
 * is their K' <= 23 LDS line (a Mish actor takes every K' <= 64 at every row count). dppo_ppo_plan_act
 * reports the tile. tests/test_actor_mish_gpu.py pins this.
 * ELU, GELU and Softplus actor images (DPPO_ACT_ELU / _GELU / _SOFTPLUS) are Mish images in every respect
 * above: none of their derivatives can be read off the stored activation, so they carry h1 and h2, run
 * the same 32-row tile on 8 waves with the same plan, take every K' <= 64, and are accepted and refused
 * exactly where Mish images are, with the same messages (tests/test_actor_activations_gpu.py). */

/* Schedule table, one fp32 row per sampling row r (r = t for DDPM; the DDIM sub-sequence index for
 * DDIM): {c0, c1, c2, c3, logvar, eval_floor, eval_zero, 0} with
 *   x0 = clip(c0 x - c1 eps, -1, 1);  mu = c2 x0 + c3 x;  sigma = exp(logvar / 2)
 * and the eval-mode (deterministic) noise rule sigma = eval_zero ? 0 : clip(sigma, eval_floor, 1e6).
 *   DDPM (model/diffusion/diffusion.py:57-73, diffusion_vpg.py:198-243, 303-315): c0 = sqrt(1/abar_t),
 *     c1 = sqrt(1/abar_t - 1), c2 = mu_coef1, c3 = mu_coef2, logvar = logvar_clipped; eval_floor
 *     1e-3, eval_zero = (t == 0).
 *   DDIM (diffusion.py:76-96, diffusion_vpg.py:184-234, the documented formulas): with abar, abar_prev
 *     of the sub-sequence and eps' = (x - sqrt(abar) x0) / sqrt(1 - abar) after the clip,
 *     mu = sqrt(abar_prev) x0 + d eps', d = sqrt(max(1 - abar_prev - sigma^2, 0)), which is the same
 *     affine form: c2 = sqrt(abar_prev) - d sqrt(abar) / sqrt(1 - abar), c3 = d / sqrt(1 - abar);
 *     c0 = 1 / sqrt(abar), c1 = sqrt(1/abar - 1); logvar = log(sigma^2), sigma = max(eta sqrt((1 - abar_prev)
 *     / (1 - abar) (1 - abar / abar_prev)), 1e-10); eval_floor 0, eval_zero 1; column 7 = s =
 *     sqrt((1 - abar_prev) / (1 - abar) (1 - abar / abar_prev)) (sigma / eta: read only by the
 *     learnable-eta gradient, DPPO_PPO_LEARN_ETA; ABI 9; 0 for DDPM rows).
 *   x0-prediction (predict_epsilon=False, diffusion.py:117-134: x_recon is the network's output): the same
 *     affine form with c0 = 0, c1 = -1 in every row, c2 .. eval_zero as for DDPM: x0 = clip(out), and the update's
 *     d loss / d out = -c1 c2 dmu = c2 dmu under the same mask.
 *
 * The table's ATTRIBUTES (an addition within ABI 15) are {denoised_clip, predict_x0}: the bound c of
 * x0 = clip(c0 x - c1 out, -c, c) (diffusion_vpg.py:183-209 clips only `if denoised_clip_value is not None`) and
 * whether the network's output is x0. They live in a host table keyed by the table's device ADDRESS, like a
 * packed image's; an address nobody recorded reads as {1.0, epsilon}, which is every launch before this addition,
 * bit for bit. dppo_sched_set_params records them (host-only but for one blocking 32-byte read of row 0 when
 * predict_x0 is set, no launch: the caller has the table complete and visible to a blocking copy by then, i.e.
 * filled on the null stream or its stream synchronised, and passes the address of memory HIP allocated, or
 * plain host memory for a host-only description); denoised_clip 0 or an infinity of either sign means None (no clip: the kernels
 * take +inf as the bound). dppo_forget_sched erases the record (NULL is accepted) and is called before the
 * table's memory is released, as dppo_forget_image is for an image; the Python package does it when the tensor
 * is freed (ops.sched_set_params). dppo_eta_step rewrites a table in place and leaves its record alone.
 *   reads the record (once per call): dppo_sample, dppo_sample_step, dppo_rollout_enqueue{,_tagged} (the bound,
 *     in every sampler kernel), dppo_logprob and dppo_ppo_minibatch{,_part} (the bound: the same value clips
 *     x_recon, masks the backward and re-derives x0 in the learnable-eta term), dppo_pretrain_minibatch
 *     (predict_x0 picks the target: loss = mean((out - x_start)^2) instead of (out - noise)^2; pretraining never
 *     clips, so the bound changes nothing there).
 *   accepted: any bound > 0 or None, with epsilon-prediction on DDPM and DDIM tables; predict_x0 on a DDPM table
 *     (the caller gives it the x0 rows above).
 *   refused with DPPO_EINVAL and a message of its own, before anything is enqueued, outputs (or the record)
 *   untouched:
 *     dppo_sched_set_params: a NaN bound; a negative finite bound; predict_x0 outside {0, 1}; predict_x0 on a table
 *       whose row 0 has eval_floor 0, i.e. DDIM rows ("DDIM requires predicting epsilon", the reference's assert);
 *     every reading entry: predict_x0 with time_stride > 1;
 *     dppo_ppo_minibatch{,_part}: predict_x0 together with DPPO_PPO_LEARN_ETA.
 * tests/test_diffusion_param_gpu.py pins this. */
#define DPPO_SCHED_COLS 8

DPPO_API int         dppo_abi_version(void);
DPPO_API const char* dppo_last_error(void);
/* the schedule table's attributes (above) */
DPPO_API int dppo_sched_set_params(const float* sched, float denoised_clip, int predict_x0);
DPPO_API int dppo_forget_sched(const float* sched);

/* ---- parameter packing (replaces Keras variable storage; model/common/mlp.py:95-206) ---- */
DPPO_API size_t dppo_actor_param_count(const dppo_dims* d);
DPPO_API size_t dppo_critic_param_count(const dppo_dims* d);
/* bytes of the packed (MFMA fragment-ordered) device image of one actor / critic */
DPPO_API size_t dppo_actor_packed_bytes(const dppo_dims* d, int precision);
DPPO_API size_t dppo_critic_packed_bytes(const dppo_dims* d, int precision);
/* params: flat fp32 (layout above) -> packed image (forward + transposed fragments) */
DPPO_API int dppo_pack_actor(const dppo_dims* d, int precision, const float* params, void* packed, void* stream);
DPPO_API int dppo_pack_critic(const dppo_dims* d, int precision, const float* params, void* packed, void* stream);
/* The actor's activation (DiffusionMLP activation_type, model/diffusion/mlp_diffusion.py:21; ResidualMLP
 * applies it at both sites of the residual block, model/common/mlp.py:95-206: u1 = act(h1), a = act(h2)).
 * It is an attribute of the packed IMAGE, not of dppo_dims (an addition within ABI 15):
 * dppo_pack_actor_act packs like dppo_pack_actor and records `activation` for the image at `packed` in a
 * host table keyed by that address; dppo_pack_actor and dppo_pack_all record DPPO_ACT_RELU, so re-packing
 * a buffer resets the attribute. The optimizer steps (staged or DPPO_STEP_FUSED_PACK), the fold launch
 * and dppo_refresh_sampler_tables rewrite an image that was packed before and leave its attribute alone.
 * Every launcher that takes a packed actor image (dppo_sample, dppo_sample_step, dppo_rollout_enqueue*,
 * dppo_logprob, dppo_ppo_minibatch{,_part}, dppo_pretrain_minibatch) looks the image up (ReLU when it was
 * never packed through these entries) and runs that activation's kernels. An activation outside the
 * enum is refused with DPPO_EINVAL; so is a sampler launch whose base and fine-tuned images carry
 * different activations, before anything is enqueued. The critic is Mish always (critic.py:40-54).
 * The values follow the reference's activation_dict: relu; mish = x tanh(softplus(x)); elu with alpha = 1
 * (x > 0 ? x : expm1(x)); gelu in its erf form (x Phi(x), keras' approximate=False, not the tanh
 * approximation); softplus = log1p(e^x). Value 2 is RESERVED for Tanh and refused like any value outside
 * the enum ("dppo_pack_actor_act: bad activation 2 ..."): no kernel implements it yet, and its number is
 * kept so that a later Tanh does not renumber the values below. An activation has no parameters: the image
 * bytes of a pack do not depend on it. */
enum { DPPO_ACT_RELU = 0, DPPO_ACT_MISH = 1, /* 2 reserved, refused */ DPPO_ACT_ELU = 3, DPPO_ACT_GELU = 4,
       DPPO_ACT_SOFTPLUS = 5 };
DPPO_API int dppo_pack_actor_act(const dppo_dims* d, int precision, int activation, const float* params, void* packed,
                                 void* stream);
/* The actor's head (DiffusionMLP residual_style, model/diffusion/mlp_diffusion.py:12-25), the image's second
 * attribute (an addition within ABI 15). DPPO_HEAD_RESIDUAL is ResidualMLP (in-Dense, one two-Dense block with
 * its skip, out-Dense). DPPO_HEAD_PLAIN is the reference's MLP([in, h, h, out]) of the default mlp_dims = [h, h]
 * (model/common/mlp.py:35-92):
 *     h1 = in(x);  u1 = act(h1);  h2 = l1(u1);  a = act(h2);  eps = W_out^T a + b_out
 * i.e. the residual network with the l2 layer and the skip removed. dppo_pack_actor_head packs like
 * dppo_pack_actor_act and records both attributes; dppo_pack_actor, dppo_pack_actor_act and dppo_pack_all
 * record RESIDUAL, so re-packing a buffer through them resets the head. A head outside the enum is
 * DPPO_EINVAL; so is a sampler launch whose base and fine-tuned images carry different heads, before anything
 * is enqueued ("... carry different heads").
 * Flat layout: unchanged. A plain actor uses the actor layout above with the l2_w / l2_b range UNUSED:
 * dppo_dims, dppo_actor_param_count, every flat offset, the optimizer ranges and the data-parallel buckets
 * stay as they are. The caller creates that range as zero; every gradient entry writes it as zero (also
 * under DPPO_PPO_L2_DEFERRED, which has nothing to defer), and AdamW (Keras or torch mode) of a zero
 * parameter with a zero gradient is exactly zero, so it stays zero. The pack copies the range into the W_L2 /
 * T_L2 / B_L2 segments like any other, but no result on a plain image depends on those segments (the
 * streaming sampler is instantiated per head and its plain form drops the l2 product).
 * What the image holds, in the folded form the kernels compute (eps = W_out^T h1 + M^T a + B_OUT2; row tiles
 * eps = a M + a0 M0 + b): FOLD / RT_FOLD = rnd(W_out) (hi = rnd(W_out), lo = 0: exact), RT_TFOLD its
 * transpose, ROUT and RT_FOLD0 (the skip's operands) zero, B_OUT2 / RT_BOUT = b_out, T_OUT (the row tile's
 * dh3 = dy W_out^T operand, the skip's share of dh1) zero; W_L2 / T_L2 / B_L2 are the packed range (no result uses it).
 * The split sampler and the row tiles run a plain image unchanged (the fp32 split kernel takes its skip
 * operand from the zero T_OUT segment instead of W_OUT); the streaming sampler feeds act(h2) through its
 * skip path. In a minibatch dW_out = u2^T dy is written in place and no l2_back / out_back product runs;
 * the fused optimizer step leaves T_OUT zero and the fold launch derives M = rnd(W_out) again.
 * DPPO_STEP_L2_FROM_PL2 on a plain image is DPPO_EINVAL; dppo_materialize_l2 on one does nothing. The supported-geometry tables (sampler, update) and
 * dppo_ppo_plan_act apply to a plain image line for line, with the same messages. The critic's head is an
 * attribute of its own image (dppo_pack_critic_head below). */
enum { DPPO_HEAD_RESIDUAL = 0, DPPO_HEAD_PLAIN = 1 };
DPPO_API int dppo_pack_actor_head(const dppo_dims* d, int precision, int activation, int head, const float* params,
                                  void* packed, void* stream);
/* The critic's head (CriticObs residual_style, model/common/critic.py:15-38), an attribute of the packed critic
 * image recorded like the actor's, keyed by the image's address (an addition within ABI 15). DPPO_HEAD_RESIDUAL is
 * ResidualMLP; DPPO_HEAD_PLAIN is the reference's MLP([SD, HC, HC, HC, 1]) (model/common/mlp.py:35-92), the class
 * default with the cfgs' mlp_dims = [256, 256, 256], Mish:
 *     residual:  h1 = in(s); u1 = mish(h1); h2 = l1(u1); u2 = mish(h2); h3 = l2(u2) + h1;  V = out(h3)
 *     plain:     h1 = in(s); u1 = mish(h1); h2 = l1(u1); u2 = mish(h2); h3 = l2(u2); u3 = mish(h3); V = out(u3)
 * The four Dense layers have the same shapes in both, so the flat critic layout above (in_w ... out_b),
 * dppo_critic_param_count, dppo_critic_packed_bytes, the image's segments, the optimizer ranges, the clip norms
 * and the data-parallel buckets are unchanged, and the image BYTES of a plain pack equal those of a residual pack
 * of the same parameters: only the attribute differs. dppo_pack_critic_head packs like dppo_pack_critic and
 * records `head`; dppo_pack_critic and dppo_pack_all record RESIDUAL, so re-packing a buffer through them resets
 * it; the optimizer steps (staged or DPPO_STEP_FUSED_PACK) rewrite the image and leave the attribute alone; an
 * address never packed through these entries reads as RESIDUAL. A head outside the enum is DPPO_EINVAL.
 * dppo_critic_forward and dppo_ppo_minibatch{,_part} look the image up and run that head's row tile (the only
 * critic hidden width instantiated, 256, for both). In a minibatch a plain critic's l2 gradient is a true
 * weight-gradient product (u2^T dh3 from a dh3 image the row tile writes, dppo_ppo_workspace_bytes below), not
 * the factored form through the out layer; the critic's last launch then only re-zeroes the stream's sample counts. */
DPPO_API int dppo_pack_critic_head(const dppo_dims* d, int precision, int head, const float* params, void* packed,
                                   void* stream);
/* The critic's layer normalisation (CriticObs use_layernorm, model/common/critic.py:15-38; mlp.py:64-66, 174-176,
 * 190-202), the critic image's SECOND attribute, recorded like the head (an addition within ABI 15). With
 * DPPO_LN_ON every hidden Dense is followed by Keras' LayerNormalization before its Mish: over the last axis,
 * population variance, y = gamma (h - mean) rsqrt(var + eps) + beta:
 *     plain:     y_k = LN_k(h_k), u_k = mish(y_k), k = 1..3;  V = out(u3);            eps = 1e-3 (Keras' default)
 *     residual:  h1 = in(s); u1 = mish(LN_1(h1)); h2 = l1(u1); u2 = mish(LN_2(h2)); h3 = l2(u2) + h1; V = out(h3);
 *                eps = 1e-6; the skip carries the un-normalised h1
 * (no norm on the output layer). The statistics are fp32 from the fp32 accumulators at every precision; only the
 * operands of the next product are rounded to the 2-byte type.
 * Unlike the head this attribute LENGTHENS the critic's flat layout and image by a tail; every existing offset keeps
 * its value (the actor's, the critic's eight tensors, and the actor | critic concatenation in `grads`, where the
 * critic comes last):
 *   flat   ... out_b | ln1_g ln1_b ln2_g ln2_b (residual) | ln3_g ln3_b (plain too), each [critic_hidden] fp32;
 *          gamma is created as ones, beta as zeros
 *   image  the same vectors, fp32 and dense, in one segment behind the image's present ones (at
 *          dppo_critic_packed_bytes); the leading bytes equal those of a pack of the same eight tensors
 * dppo_critic_param_count_ln / dppo_critic_packed_bytes_ln give the sizes (0 for an attribute outside its enum);
 * with DPPO_LN_OFF they are dppo_critic_param_count / dppo_critic_packed_bytes for both heads.
 * dppo_pack_critic_ln packs like dppo_pack_critic_head and records both attributes; dppo_pack_critic,
 * dppo_pack_critic_head and dppo_pack_all record DPPO_LN_OFF; dppo_forget_image clears it; the optimizer steps
 * leave it alone. An attribute outside its enum is DPPO_EINVAL, nothing enqueued, the image's attributes kept.
 * Entries that receive the critic image read the attribute and use the longer layout: dppo_critic_forward,
 * dppo_ppo_minibatch{,_part} (the critic's gradients end in dln1_g, dln1_b, ...: the row tiles add each tile's
 * column sums into that tail with fp32 atomics, and the minibatch's zeroing launch covers it), and
 * dppo_optimizer_step{,_ex,_clip}: a staged step packs the tail, DPPO_STEP_FUSED_PACK steps a critic range of
 * dppo_critic_param_count_ln elements in one launch, DPPO_STEP_CLEAR_GRADS clears the range it steps, tail included.
 * gamma and beta are variables like any bias: AdamW with weight decay (Keras decays every variable), a clip norm
 * and scale each (8 + 4 or 8 + 6 critic variables, in layout order), part of the data-parallel bucket.
 * What an entry can see of a buffer sized for the other layout it refuses with DPPO_EINVAL before anything is
 * enqueued: an optimizer range that holds fewer elements from critic_params on than the layer-normed image's layout
 * ("... buffers sized for the layout without the tail"), a critic-only range of a layer-normed length on an image
 * without layer norm, a clipped range that is not exactly the networks' layouts. Raw device pointers carry no
 * size, so the Python package checks every tensor against the spec (ops.py).
 * Entries that see only dppo_dims have _ln forms that take the two attributes (dppo_grad_clip_workspace_bytes_ln,
 * dppo_grad_clip_scales_ln, dppo_ppo_clear_ranges_ln); the old forms keep their meaning exactly (no layer norm).
 * The supported-geometry table of the update entries above applies to a layer-normed critic line for line, with
 * the same messages (critic_hidden 256; cond_steps*obs_dim <= 32 in fp32, <= 64 in bf16 / fp16): the norm adds
 * 8,704 B (residual) or 11,008 B (plain) of LDS to the 32-row tile and no geometry-dependent limit. The layer-normed tile runs the plain 8-wave
 * kernel form, not the 128-register one (dppo_ppo_plan_critic reports it). tests/test_critic_layernorm_gpu.py pins this. */
enum { DPPO_LN_OFF = 0, DPPO_LN_ON = 1 };
DPPO_API size_t dppo_critic_param_count_ln(const dppo_dims* d, int head, int layernorm);
DPPO_API size_t dppo_critic_packed_bytes_ln(const dppo_dims* d, int precision, int head, int layernorm);
DPPO_API int dppo_pack_critic_ln(const dppo_dims* d, int precision, int head, int layernorm, const float* params,
                                 void* packed, void* stream);
/* The attributes above (an actor image's activation and head, a critic image's head) live in a host table keyed
 * by the image's ADDRESS, so they outlive the buffer: memory allocated at the same address later (a copy of an
 * image, which was never packed through these entries, for one) would read the old owner's attributes instead of
 * the defaults. A caller that releases an image buffer whose attributes are not the defaults calls
 * dppo_forget_image first: the address then reads as never packed (ReLU / RESIDUAL / RESIDUAL / LN_OFF, no pending
 * sampler-table refresh). Host-only, no launch; NULL is accepted (an addition within ABI 15). The Python package
 * does this when an image tensor it packed is freed (ops.pack_actor / ops.pack_critic). */
DPPO_API int dppo_forget_image(const void* packed);

/* ---- a9: diffusion-policy action sampler, VPGDiffusion.call (model/diffusion/diffusion_vpg.py:250-339) ----
 * All K DDPM steps for n_envs rows in ONE launch: DiffusionMLP forward on MFMA + fused DDPM
 * reparameterisation epilogue (diffusion_vpg.py:152-245, 301-320).
 *   cond     [n_envs, To*Do]
 *   x_T      [n_envs, Ta*Da] or NULL -> in-kernel Philox (seed, call_id) stream
 *   noise    [K, n_envs, Ta*Da] raw N(0,1) draws for loop index i (t = K-1-i), or NULL -> Philox
 *   env_offset: global row index of row 0 (Philox counter; multi-GPU shards stay distinct)
 *   final_clip <= 0 means None (cfg default)
 *   actions  [n_envs, Ta*Da]                 (Sample.trajectories)
 *   chains   [n_envs, K'+1, Ta*Da] or NULL   (Sample.chains)
 * Supported geometry (dppo_sample, dppo_sample_step, dppo_rollout_enqueue*). With XD =
 * horizon_steps*action_dim, SD = cond_steps*obs_dim, in = XD + time_dim + SD, K = denoising_steps,
 * the split register-resident kernel runs where all of its line hold, else the weight-streaming one:
 *   split, bf16 / fp16:     actor_hidden 512; XD % 4 == 0; XD + SD <= 64; K <= 62; n_envs <= 512
 *   split, fp32:            actor_hidden 512; XD == 12; XD + SD <= 32; K <= 62; n_envs <= 512 on 256
 *                           CUs (whatever time_dim is: a 31-input hopper variant runs here)
 *   both split lines:       the kernel's LDS <= 160 KiB (hopper's width stops at K = 60 in fp32 and
 *                           K = 35 in bf16 / fp16; cond_steps 2 reaches K = 62 in bf16 / fp16)
 *   streaming, bf16 / fp16: actor_hidden 512; in <= 128
 *   streaming, fp32:        actor_hidden 256 or 512; 33 <= in <= 64
 *   both streaming lines:   the kernel's LDS <= 160 KiB (K * XD: K = 100 at XD = 32 is over)
 * Everything else the dimension check takes (actor_hidden 128 / 384, 256 in bf16 / fp16, other input
 * widths) is refused with DPPO_EUNSUPPORTED and "sampler: hidden %d / action chunk %d / in-layer
 * k-steps %d not instantiated", "sampler: hidden %d not supported at this precision" (fp32 384) or
 * "sampler needs %zu B of LDS" before anything is enqueued: outputs, dppo_sample_step's device copy
 * of cond and the stream stay as they were. time_dim > 32 has no image (dppo_pack_actor refuses it).
 * tests/test_sampler_surface_gpu.py pins the table, geometry by geometry.
 * Mish actor images (dppo_pack_actor_act; both images of a launch carry the same activation, else
 * DPPO_EINVAL) run on every line above, on the same kernel (dppo_sampler_plan does not depend on the
 * activation), and are refused where ReLU images are, with the same messages
 * (tests/test_actor_mish_gpu.py). ELU, GELU and Softplus images run and are refused exactly where Mish
 * images are, with the same messages (tests/test_actor_activations_gpu.py).                    */
DPPO_API int dppo_sample(const dppo_dims* d, int precision, const void* packed_base, const void* packed_ft,
                const float* sched, const float* cond, int n_envs, const float* x_T, const float* noise,
                uint64_t seed, uint64_t call_id, int env_offset, int deterministic,
                float min_sampling_std, float randn_clip, float final_clip,
                float* actions, float* chains, void* stream);

/* Measurement aid (no reference counterpart): bytes of weight fragments one 16-env sampler tile
 * (one CU) loads per dppo_sample launch with the sampler geometry in use — every denoising step's
 * streamed k-steps plus the resident set, loaded once per actor. bench.py divides it by the launch
 * time for the per-CU load-path figure. Also returns the waves per workgroup. */
DPPO_API int dppo_sampler_stream_bytes(const dppo_dims* d, int precision, int64_t* bytes_per_tile, int* waves);

/* Which sampler layout dppo_sample runs for n_envs envs: *members = 0 for the weight-streaming
 * kernel (one workgroup per 16-env tile), or P > 0 for the split register-resident kernel (P
 * workgroups per 16-env tile, one in-launch partial-sum exchange per denoising step; bf16,
 * actor_hidden 512, horizon*action_dim a multiple of 4, <= 512 envs). The split kernel keeps one
 * 2 MiB exchange buffer per stream, allocated by the library on the first launch on that stream
 * (the one allocation outside a caller workspace). */
DPPO_API int dppo_sampler_layout(const dppo_dims* d, int precision, int n_envs, int* members);

/* How many dppo_sample / dppo_rollout_enqueue* launches of n_envs envs may be in flight at once on
 * the current device (on different streams) without one launch taking CUs another's split-kernel
 * members wait for: floor(CUs / active workgroups) for the split kernel (>= 1), 8 for the
 * weight-streaming kernel. The pipelined rollout (ops.RolloutPipe) uses at most this many streams. */
DPPO_API int dppo_sampler_max_in_flight(const dppo_dims* d, int precision, int n_envs, int* launches);

/* ABI 10: the caller is done sampling on `stream` (a closed rollout pipe): waits for the stream's
 * pending work, then unbinds the exchange buffer the split kernel keeps for it, so a later stream
 * reuses that buffer instead of a new allocation. Slots are also rebound, without a device-wide
 * synchronisation, when more than 16 streams sample. (No reference counterpart: the reference's
 * sampler is a TF call, diffusion_vpg.py:250-339.) */
/* A stream that sampled must be released before its owner destroys it (ops.RolloutPipe.close does);
 * a slot whose stream no longer answers hipStreamQuery is treated as released. */
DPPO_API int dppo_sampler_release_stream(void* stream);

/* Kernel timer (ABI 10, measurement): while enabled, the library brackets the launches of its
 * timed kernels (the sampler, the row tiles, dW, l2_back, time_bwd, AdamW, pack, GAE, the reward
 * scaler's three kernels, the gradient-clip norms, ...; dppo_kernel_timing_name(id) names id, NULL past the last) with HIP
 * events on the launch's own stream. dppo_kernel_timing(enable) switches it and clears the window;
 * dppo_kernel_timing_read(n, total_ms[n], launches[n]) waits for the window's launches, returns the
 * summed event time and launch count per id, and clears the window. Off by default: a disabled timer
 * is one flag test per launch. */
DPPO_API int dppo_kernel_timing(int enable);
DPPO_API const char* dppo_kernel_timing_name(int id);
DPPO_API int dppo_kernel_timing_read(int n, double* total_ms, int64_t* launches);

/* The sampler plan for n_envs envs (measurement aid, ABI 6): plan[0] = kernel (0 weight streaming,
 * 1 split with 8 members per 16-env tile, 2 folded split with P members per tile, 3 the pair kernel:
 * P = 2 members running two 16-env tiles half a denoising step apart), plan[1] = members per member
 * set, plan[2] = member sets (2: the base actor's and the fine-tuned actor's steps on separate
 * workgroups), plan[3] = workgroups per launch. */
DPPO_API int dppo_sampler_plan(const dppo_dims* d, int precision, int n_envs, int* plan);

/* One rollout step (agent/finetune/train_ppo_diffusion_agent.py:106-122) in one call:
 * hipMemcpyAsync(cond <- cond_host [host, pinned]), dppo_sample with the Philox noise, hipMemcpyAsync
 * (actions_host [host, pinned] <- actions), then hipStreamSynchronize when synchronize != 0. */
DPPO_API int dppo_sample_step(const dppo_dims* d, int precision, const void* packed_base, const void* packed_ft,
                const float* sched, const float* cond_host, float* cond, int n_envs, uint64_t seed,
                uint64_t call_id, int env_offset, int deterministic, float min_sampling_std,
                float randn_clip, float final_clip, float* actions, float* actions_host,
                float* chains, int synchronize, void* stream);

/* Pipelined rollout (the same step, with the launch taken off the host's critical path):
 * the host enqueues step t+1 BEFORE stepping the envs of step t; that launch does everything
 * that does not depend on the observation (noise, time embedding, weights in flight), then waits
 * until *go >= go_value, reads the observation from cond_host, and after writing the actions to
 * actions_host adds 1 per workgroup (ceil(n_envs/16)) to *done. cond_host, actions_host, go and
 * done must come from dppo_host_alloc (mapped, coherent pinned memory). The wait is bounded
 * (~4 s): on timeout the step proceeds and sets bit 31 of *done. */
DPPO_API int dppo_host_alloc(size_t bytes, void** ptr);
DPPO_API int dppo_host_free(void* ptr);
/* ABI 9: n <= 4 copies src_host[i] (dppo_host_alloc memory) -> dst[i] (device), bytes[i] each, in ONE
 * kernel launch on stream that reads the mapped memory over the bus (no copy engine): the rollout's
 * per-step rewards and flags into the update's device buffers (agent :232-263). */
DPPO_API int dppo_copy_from_host(int n, void* const* dst, const void* const* src_host, const size_t* bytes,
                                 void* stream);
DPPO_API int dppo_rollout_enqueue(const dppo_dims* d, int precision, const void* packed_base, const void* packed_ft,
                const float* sched, const float* cond_host, float* cond, int n_envs, uint64_t seed,
                uint64_t call_id, int env_offset, int deterministic, float min_sampling_std,
                float randn_clip, float final_clip, float* actions, float* actions_host,
                float* chains, const uint32_t* go, uint32_t go_value, uint32_t* done, void* stream);

/* The same pipelined step with a TAGGED observation (ABI 2): no go counter; the host writes each
 * observation value as an 8-byte granule {tag in the high 32 bits, fp32 bits in the low 32} into
 * obs_tagged ([n_envs][To*Do] uint64, from dppo_host_alloc), and the launch polls its envs'
 * granules until every tag equals `tag` (nonzero, unique among the tags the buffer may hold, e.g.
 * the step count). The observation carries its own ready flag: one PCIe round trip instead of a
 * flag poll followed by a read. The actions come back the same way: actions_tagged ([n_envs][Ta*Da]
 * uint64, from dppo_host_alloc) receives {tag, fp32} granules, so the host can poll the actions
 * themselves instead of waiting for *done (which still counts finished workgroups, and bit 31 still
 * flags a timeout). cond receives the device copy of the observation. */
DPPO_API int dppo_rollout_enqueue_tagged(const dppo_dims* d, int precision, const void* packed_base,
                const void* packed_ft, const float* sched, const uint64_t* obs_tagged, float* cond,
                int n_envs, uint64_t seed, uint64_t call_id, int env_offset, int deterministic,
                float min_sampling_std, float randn_clip, float final_clip, float* actions,
                uint64_t* actions_tagged, float* chains, uint32_t tag, uint32_t* done, void* stream);

/* ---- a10: VPGDiffusion.get_logprobs (diffusion_vpg.py:343-425) + the clip/mean of c_loss
 * (diffusion_ppo.py:50-59) for the old-logprob pass (agent/finetune/train_ppo_diffusion_agent.py:214-229).
 *   cond [n, To*Do], chains [n, K'+1, Ta*Da]
 *   lp_elem [n*K', Ta*Da] or NULL (row = sample*K' + j, t = K'-1-j)
 *   lp_mean [n, K'] or NULL: mean over the first reward_horizon Ta rows of clip(lp, -5, 2)   */
DPPO_API int dppo_logprob(const dppo_dims* d, int precision, const void* packed_ft, const float* sched,
                 const float* cond, const float* chains, int n, float min_logprob_std, int reward_horizon,
                 float* lp_elem, float* lp_mean, void* stream);

/* ---- a6: CriticObs forward (model/common/critic.py:40-54): values [n] ---- */
DPPO_API int dppo_critic_forward(const dppo_dims* d, int precision, const void* packed_critic, const float* cond,
                        int n, float* values, void* stream);

/* ---- a18: RunningRewardScaler.__call__ (util/reward_scaling.py:60-87), in place on device.
 *   reward [S, E] (time-major, fp64), first [S, E] (u8); ret_state [E] fp64 carried across calls;
 *   rms_state [3] fp64 {mean, var, count} (init {0, 1, 1e-4}); reward overwritten with the scaled value;
 *   workspace: dppo_reward_scale_workspace_doubles(S, E) fp64 */
DPPO_API size_t dppo_reward_scale_workspace_doubles(int S, int E);
DPPO_API int dppo_reward_scale(double* reward, const uint8_t* first, double* ret_state, double* rms_state, double* workspace,
                      int S, int E, double gamma, double cliprew, double epsilon, void* stream);
/* same, split for multi-GPU: pass 1 (returns local moments {n, mean, M2} in moments[3]) ... */
DPPO_API int dppo_reward_scale_moments(const double* reward, const uint8_t* first, double* ret_state, double* workspace,
                              double* moments, int S, int E, double gamma, void* stream);
/* ... caller all-reduces/merges moments into rms_state, then pass 2 */
DPPO_API int dppo_reward_scale_apply(double* reward, const double* rms_state, int S, int E, double cliprew,
                            double epsilon, void* stream);
/* ABI 12: RunningRewardScaler(per_env=True) (util/reward_scaling.py:51-66). The reference's
 * RunningMeanStd then has shape (num_envs,) and is updated by ret_rms.update(rets) with rets [E, S]:
 * the moments are taken over axis 0, the ENVS, one (mean, var) pair per time column with batch count
 * E, and NumPy broadcasting joins them to the state (so S must equal the state's length L, or one of
 * the two be 1); transform() divides reward [E, S] by sqrt(var + eps) along its last axis. Kept as
 * written, broadcasting errors included (DPPO_EINVAL "operands could not be broadcast together").
 *   rms_in / rms_out fp64 [1 + 2 L] = {count, mean[L], var[L]} (init {1e-4, 0..., 1...}, L = E);
 *   rms_out has L_out = broadcast(S, L_in) entries and must not alias rms_in;
 *   out [C, E] time-major (C = S, or L_out when S == 1 < L_out: the reference returns [E, L_out]); out
 *   may alias reward when C == S. reward / first / ret_state / workspace as dppo_reward_scale. */
DPPO_API int dppo_reward_scale_per_env(const double* reward, const uint8_t* first, double* ret_state,
                                       const double* rms_in, int L_in, double* rms_out, double* workspace, int S, int E,
                                       double gamma, double cliprew, double epsilon, double* out, void* stream);
/* ... the same split for multi-GPU: the scan and the per-column moments col_moments fp64 [S][2] =
 * {mean_t, var_t} over this rank's envs (the caller merges ranks and updates the state), then the scale */
DPPO_API int dppo_reward_scale_per_env_moments(const double* reward, const uint8_t* first, double* ret_state,
                                               double* workspace, double* col_moments, int S, int E, double gamma,
                                               void* stream);
DPPO_API int dppo_reward_scale_per_env_apply(const double* reward, const double* rms_state, int S, int E, int L,
                                             double cliprew, double epsilon, double* out, void* stream);

/* ---- a19: GAE (train_ppo_diffusion_agent.py:239-263). reward fp64 [S,E], values fp32 [S,E],
 * last_values fp32 [E], terminated u8 [S,E] -> advantages, returns fp32 [S,E] */
DPPO_API int dppo_gae(const double* reward, const float* values, const float* last_values, const uint8_t* terminated,
             int S, int E, double gamma, double lam, double reward_scale_const,
             float* advantages, float* returns, void* stream);

/* ---- a16: episode accounting (train_ppo_diffusion_agent.py:144-167) on the RAW rewards fp64 [S,E]
 * and the episode-start flags first u8 [S+1,E] (row S: the flags after the last step): per env,
 * out fp64 [E][4] = {episodes that start and end inside the rollout (consecutive starts s < en with
 * en - s > 1), sum of their returns, sum of their best rewards max(rew[s:en]) / act_steps, count of
 * best >= success_threshold}; the caller sums the rows in env order. (ABI 14) */
DPPO_API int dppo_episode_sums(const double* reward, const uint8_t* first, int S, int E, int act_steps,
                               double success_threshold, double* out, void* stream);

/* ---- a22: explained-variance moments (train_ppo_diffusion_agent.py:373-377) of y = returns and
 * d = returns - values over n rows: moments fp64[5] = {sum y, sum y^2, sum d, sum d^2, n}, one
 * deterministic workgroup; moments may be device or host-mapped memory (dppo_host_alloc). Summed
 * over ranks they give explained_var = 1 - Var(d) / Var(y). (ABI 5) */
DPPO_API int dppo_value_moments(const float* values, const float* returns, int64_t n, double* moments, void* stream);

/* ---- a12/a13/a20: one PPO minibatch: gather by permutation, PPODiffusion.c_loss forward + gradient
 * of pg_loss + vf_coef*v_loss w.r.t. actor_ft and critic (diffusion_ppo.py:32-132,
 * train_ppo_diffusion_agent.py:287-346).
 * Rollout buffers (sample index n = step*E + env, total = S*E*K'):
 *   obs [S*E, To*Do], chains [S*E, K'+1, Ta*Da], lp_old_mean [S*E, K'] (from dppo_logprob),
 *   advantages / returns [S*E] fp32.
 * Minibatch rows: perm(start .. start+rows-1) with perm = Feistel bijection of [0,total) keyed
 * by (perm_seed, epoch), unravelled to (n, j) = (idx / K', idx % K') (tf.unravel_index);
 * or, when row_index != NULL, idx = row_index[start + r] (host-chosen rows, e.g. c_loss on an
 * explicit batch or a replayed tf.random.shuffle permutation).
 * grads [actor_count + critic_count] fp32 are OVERWRITTEN (actor first). metrics (device, fp64[16]):
 *   {pg_loss, v_loss, approx_kl, clipfrac, ratio_mean, loss, adv_mean, adv_std, ...}.
 * adv_stats: fp64[3] {count, sum, sumsq} of the minibatch advantages, or NULL to compute locally;
 *   a multi-GPU caller computes them with dppo_ppo_adv_stats + all-reduce first. */
typedef struct dppo_ppo_hparams {
    float gamma_denoising, clip_ploss_coef, clip_ploss_coef_base, clip_ploss_coef_rate;
    float min_logprob_std, vf_coef;
    int32_t norm_adv, reward_horizon;
    float loss_scale;       /* multiplies 1/b (= 1/world_size for a DP all-reduce-sum) */
    int32_t global_rows;    /* b used in the 1/b means (rows over all ranks) */
    int32_t flags;          /* ABI 8: DPPO_PPO_* below (0: every gradient materialised) */
    /* ABI 14: the clipped value loss (diffusion_ppo.py:110-116) when clip_vloss_coef > 0:
     * v_loss = 0.5 mean(max((V - R)^2, (V_old + clip(V - V_old, -c, c) - R)^2)) with V_old = old_values[n],
     * the rollout's value pass (device fp32 [S*E]); clip_vloss_coef <= 0 (or old_values NULL): the plain
     * 0.5 mean((V - R)^2) of :118 (every shipped cfg: clip_vloss_coef null) */
    float clip_vloss_coef;
    const float* old_values;
} dppo_ppo_hparams;

/* ABI 8, dppo_ppo_hparams.flags. DPPO_PPO_L2_DEFERRED: the actor's l2 gradient is left in its
 * factored form. The l2 weight region of grads holds pl2 = u2^T dy as [H][XD] (row-major, the rest
 * of the region zero) and the l2 bias region is zero; the true values are pl2 rnd(W_out)^T and
 * db_out rnd(W_out)^T (the block's output feeds only the linear out layer). A following
 * dppo_optimizer_step with DPPO_STEP_L2_FROM_PL2 forms them inside its AdamW launch (one launch
 * fewer per minibatch); dppo_materialize_l2 forms them in place. The factored form is linear, so a
 * data-parallel caller all-reduces it like the other gradients. */
enum { DPPO_PPO_L2_DEFERRED = 1 };
/* ABI 9, dppo_ppo_hparams.flags. DPPO_PPO_LEARN_ETA: a learnable DDIM eta (the original DPPO's
 * EtaFixed; the reference's eta module is absent, so parity is unpinned): the actor's row tiles add
 * d loss / d eta into metrics[8] (fp64), through sigma = eta s and d = sqrt(clip(1 - abar_prev -
 * sigma^2, 0, 1e6)) of each row (schedule column 7 = s). dppo_eta_step applies it. */
enum { DPPO_PPO_LEARN_ETA = 2 };
/* ABI 11, dppo_ppo_hparams.flags. DPPO_PPO_PRECLEARED: the outputs this part would zero first (its
 * gradient range and the ranges dppo_ppo_clear_ranges reports for the same workspace, rows and
 * metrics) are already zero — the previous optimizer step of the range cleared them
 * (DPPO_STEP_CLEAR_GRADS) — so the part skips its zeroing launch. */
enum { DPPO_PPO_PRECLEARED = 4 };
/* An addition within ABI 15, dppo_ppo_hparams.flags. DPPO_PPO_ADV_CLIP: PPODiffusion's clip_advantage_lower_quantile /
 * clip_advantage_upper_quantile (the DPPO algorithm's live lines; the reference comments them out at
 * diffusion_ppo.py:77-80, so parity is unpinned). The adv_stats pointer of dppo_ppo_minibatch / _part then addresses
 * fp64[5] = {count, sum, sumsq, lo, hi} (launch-uniform), and the actor's TRAIN row tiles clamp each row's RAW
 * advantage to [lo, hi] (rounded to fp32) before the normalisation, which keeps the mean and std of the UNCLIPPED
 * minibatch ({count, sum, sumsq}), and before the denoising discount: in real arithmetic the reference's
 * normalise-then-clamp, and the same with norm_adv off. dppo_ppo_adv_quantiles_all computes lo, hi.
 *   accepted: every part, precision, row tile (32 and 64 rows), activation, head and DPPO_PPO_LEARN_ETA;
 *             (lo, hi) = (-inf, +inf) gives the bits of the flag unset.
 *   refused (DPPO_EINVAL, outputs untouched, nothing enqueued): the flag with adv_stats == NULL, in every part.
 *   not checked: lo and hi are device memory, read by the kernel alone; no entry waits on the device to look at
 *             them. lo > hi or a NaN bound is the caller's error (dppo_ppo_adv_quantiles_* never produce one).
 *             What the tile then computes is fminf(fmaxf(A, lo), hi) with IEEE minNum / maxNum: lo > hi gives every
 *             row the advantage hi; a NaN lo leaves only the upper clamp, a NaN hi only the lower one, two NaNs
 *             none. Nothing else is read or written differently. */
enum { DPPO_PPO_ADV_CLIP = 8 };

/* ABI 9: the learnable DDIM eta's optimizer step (the original DPPO's EtaFixed trained by its own
 * AdamW every eta_update_interval minibatches, train_ppo_diffusion_agent.py:28-45, 358-359 — the
 * reference's step is commented out and its eta module absent: parity unpinned). eta_state (device
 * fp32[3]) = {logit, m, v}, eta = eta_min + (eta_max - eta_min) (tanh(logit) + 1) / 2. With metrics
 * (device fp64[16], metrics[8] = d loss / d eta of a DPPO_PPO_LEARN_ETA minibatch) and step >= 1 it
 * applies AdamW (mode as dppo_adamw) to the logit; then (also with metrics == NULL: a refresh) it
 * rewrites columns c2, c3, logvar of the ddim_steps rows of sched for the current eta from ddim_base
 * (fp32 [ddim_steps][5] = {abar_prev, sqrt(abar_prev), sqrt(abar), sqrt(1 - abar), s}) and stores
 * eta to eta_out (device or mapped, may be NULL). One launch on stream. */
DPPO_API int dppo_eta_step(float* eta_state, const double* metrics, int64_t step, float lr, float weight_decay,
                           float beta1, float beta2, float eps, int mode, float eta_min, float eta_max,
                           const float* ddim_base, float* sched, int ddim_steps, float* eta_out, void* stream);

/* The workspace is sized before an image is known, so one size serves both critic heads: it ends with the plain
 * critic's dh3 image (critic_hidden x batch_rows rounded up to 64, operand elements: 2 B, fp32 4 B), which a
 * residual critic leaves unused. Every other offset is what it was before that image was added. */
DPPO_API size_t dppo_ppo_workspace_bytes(const dppo_dims* d, int precision, int batch_rows);
/* Which kernel paths a launch of `rows` rows takes on the current device (read-only host arithmetic,
 * the same functions the launchers call; no device work; an addition within ABI 15). mode: a
 * dppo_ppo_minibatch (DPPO_PLAN_TRAIN), a dppo_pretrain_minibatch (DPPO_PLAN_PRETRAIN) or a
 * dppo_logprob pass over rows = n * K' rows (DPPO_PLAN_LOGPROB). out[6] =
 *   {actor row tile's rows (32 or 64), its waves per workgroup,
 *    m-chunks of the actor's weight-gradient launch, rows per chunk (the last may be shorter),
 *    the same two of the critic's launch (host-side: with sample dedup the kernel re-cuts the same
 *    number of chunks over the device-side count of distinct samples)};
 * the weight-gradient fields are 0 where the mode has no such launch (logprob: all four; pretrain:
 * the critic's). The critic's two are those of the RESIDUAL critic's problem list (10 output tiles at
 * critic_hidden 256); a plain critic image's list has 12 (its l2 problem is HC x HC), so its launch may cut fewer
 * chunks on the same rows: this query takes no image and does not report that. */
enum { DPPO_PLAN_TRAIN = 0, DPPO_PLAN_PRETRAIN = 1, DPPO_PLAN_LOGPROB = 2 };
DPPO_API int dppo_ppo_plan(const dppo_dims* d, int precision, int rows, int mode, int* out);
/* the same for an actor image of the given activation (DPPO_ACT_*; dppo_ppo_plan is the ReLU plan): a
 * Mish, ELU, GELU or Softplus actor runs the 32-row tile on 8 waves at every row count (the table above) */
DPPO_API int dppo_ppo_plan_act(const dppo_dims* d, int precision, int activation, int rows, int mode, int* out);
/* The critic's row tile for an image of the given attributes (dppo_pack_critic_ln), which the six outputs above have
 * no field for; host arithmetic, no image, no device work (an addition within ABI 15). out[3] = {the tile's rows (32),
 * its waves per workgroup (8), 1 if it runs the 128-register kernel entry (two tiles per CU: every critic without
 * layer norm) or 0 if the uncapped one (a layer-normed critic, whose TRAIN tile needs 223-253 registers)}. An
 * attribute outside its enum is DPPO_EINVAL. */
DPPO_API int dppo_ppo_plan_critic(const dppo_dims* d, int precision, int critic_head, int critic_layernorm, int* out);
DPPO_API int dppo_ppo_adv_stats(const float* advantages, int64_t total, int K_ft, uint64_t perm_seed, int epoch,
                       int64_t start, int rows, const int64_t* row_index, double* adv_stats, void* stream);
/* The adv_stats of every minibatch of an update phase in one launch: minibatch m = e * n_batch + b
 * covers permutation positions [b * rows_full, min((b+1) * rows_full, total)) of epoch epoch0 + e;
 * adv_stats receives fp64 [n_epochs * n_batch][3]. Same values as n_epochs * n_batch calls of
 * dppo_ppo_adv_stats (row_index = NULL); a multi-GPU caller all-reduces the whole array once. */
DPPO_API int dppo_ppo_adv_stats_all(const float* advantages, int64_t total, int K_ft, uint64_t perm_seed, int epoch0,
                           int n_epochs, int64_t rows_full, int n_batch, double* adv_stats, void* stream);
/* The advantage quantiles of every minibatch of an update phase (DPPO_PPO_ADV_CLIP; an addition within ABI 15):
 * segments indexed as dppo_ppo_adv_stats_all indexes minibatches, each the multiset {advantages[row / K_ft]} over
 * the rows of its window (n of them). For q in {q_lo, q_hi}: pos = q (n - 1), k = floor(pos),
 *   Q(q) = v_k + (pos - k) (v_min(k+1, n-1) - v_k)
 * over the sorted values v, in fp64 (numpy.quantile's default linear method on the values as float64). The order
 * statistics are exact: an 8-bit-per-pass radix select over order-preserving 32-bit keys of the fp32 values, four
 * targets per segment. bounds receives fp64 [n_epochs * n_batch][2] = {Q(q_lo), Q(q_hi)}; a window past `total`
 * (an empty segment) gets (-inf, +inf). NaN advantages are out of scope. 4 count + 4 pick launches and one
 * memset on `stream`, nothing waits on the host. workspace: dppo_ppo_adv_quantiles_workspace_bytes(n_epochs,
 * n_batch) bytes, 16-B aligned, any contents.
 * Refused (DPPO_EINVAL, nothing enqueued, outputs untouched): a null pointer, total / K_ft / rows_full / n_batch /
 * n_epochs <= 0, n_epochs > 64, total >= 2^32, more than 65535 segments, a segment of 2^31 rows or more (the
 * bins are int32; a data-parallel caller keeps a segment's rows SUMMED OVER RANKS below 2^31 itself), and
 * anything but 0 <= q_lo < q_hi <= 1 (NaN included). */
DPPO_API size_t dppo_ppo_adv_quantiles_workspace_bytes(int n_epochs, int n_batch);
DPPO_API int dppo_ppo_adv_quantiles_all(const float* advantages, int64_t total, int K_ft, uint64_t perm_seed, int epoch0,
                               int n_epochs, int64_t rows_full, int n_batch, double q_lo, double q_hi,
                               void* workspace, double* bounds, void* stream);
/* The same pass by pass (pass = 0..3, most significant byte first), which dppo_ppo_adv_quantiles_all loops over, so
 * a data-parallel caller can SUM-all-reduce `counts` between a pass's count and its pick: every rank then picks
 * the same bins, and the bounds are those of the union of the ranks' rows.
 *   counts int32 [n_seg][4][256] (n_seg = n_epochs * n_batch; 16-B aligned): zero before the pass-0 count; each
 *     pick leaves it zero again. state int64 [n_seg][9]: written by the pass-0 pick, any contents before.
 *   count adds this rank's rows into counts (reads state from pass 1 on).
 *   pick advances state; n_global int64 [n_seg] is each segment's row count over all ranks, or NULL to take it
 *     from the pass-0 counts themselves (their sum per target, which after the all-reduce is the same number);
 *     pass 3 also writes bounds (may be NULL in passes 0..2).
 * DPPO_ADV_QUANTILES_BLOCK threads bin a chunk; a segment is cut into at most DPPO_ADV_QUANTILES_MAX_CHUNKS
 * workgroups, which stride over it (a segment longer than BLOCK * MAX_CHUNKS rows takes a second trip). */
enum { DPPO_ADV_QUANTILES_BLOCK = 256, DPPO_ADV_QUANTILES_MAX_CHUNKS = 16 };
DPPO_API int dppo_ppo_adv_quantiles_count(const float* advantages, int64_t total, int K_ft, uint64_t perm_seed,
                                 int epoch0, int n_epochs, int64_t rows_full, int n_batch, int pass,
                                 const int64_t* state, int* counts, void* stream);
DPPO_API int dppo_ppo_adv_quantiles_pick(int n_epochs, int n_batch, double q_lo, double q_hi, int pass,
                                const int64_t* n_global, int64_t* state, int* counts, double* bounds, void* stream);
DPPO_API int dppo_ppo_minibatch(const dppo_dims* d, int precision, const dppo_ppo_hparams* hp,
                       const void* packed_ft, const void* packed_critic, const float* actor_params,
                       const float* sched, const float* obs, const float* chains, const float* lp_old_mean,
                       const float* advantages, const float* returns, int64_t total, uint64_t perm_seed,
                       int epoch, int64_t start, int rows, const int64_t* row_index, const double* adv_stats,
                       void* workspace, float* grads, double* metrics, void* stream);

/* ---- §8(f) row 3: the pretraining loss DiffusionModel.c_loss -> p_losses / q_sample
 * (model/diffusion/diffusion.py:179-202), loss and actor gradients; the target is the noise, or x_start when
 * the schedule table's record says predict_x0 (dppo_sched_set_params; then read (eps - noise) below as (out - x_start)).
 * Replaces the TF tape over `self.model.c_loss(**batch)` in agent/pretrain/train_diffusion_agent.py.
 * Row r is sample r: x_start [rows][horizon*action_dim], cond [rows][cond_steps*obs_dim],
 * t [rows] int32 in [0, denoising_steps), noise [rows][horizon*action_dim] (the host draws t and
 * noise, tf.random.uniform / tf.random.normal at diffusion.py:182,187).
 * sched: the DDPM schedule table (denoising_steps rows); qsched [denoising_steps][2] fp32 =
 * {sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod)} (the TF buffers, diffusion.py:62-65).
 * loss = loss_scale * sum((eps - noise)^2) / (global_rows * horizon*action_dim): metrics[0] (fp64,
 * device) receives the local sum of squares; grads [actor_count] fp32 are OVERWRITTEN with
 * d loss / d params. Workspace: dppo_ppo_workspace_bytes(d, precision, rows). Requires
 * time_stride == 1 and denoising_steps <= 64 (each a DPPO_EINVAL with its own message, as is
 * global_rows < rows: "bad rows / global_rows"; outputs untouched).
 * Buffers: the workspace need not be initialised and may hold any bytes (NaN patterns, or an earlier,
 * larger batch's images under another row padding: the entry writes every byte it later reads). All 16
 * metric slots are zeroed before metrics[0] is summed, whatever they held. grads beyond the actor's
 * parameter count are not touched. t is NOT validated: a value outside [0, denoising_steps) indexes
 * qsched and the time-embedding table out of bounds and is the caller's error.
 * tests/test_pretrain_step_gpu.py pins this and the K lines of the geometry table above. ---- */
DPPO_API int dppo_pretrain_minibatch(const dppo_dims* d, int precision, const void* packed_actor, const float* actor_params,
                            const float* sched, const float* qsched, const float* x_start, const float* cond,
                            const int32_t* t, const float* noise, int rows, int64_t global_rows, float loss_scale,
                            void* workspace, float* grads, double* metrics, void* stream);

/* ---- the behaviour-cloning term of the PPO loss and its actor gradient (an addition within ABI 15):
 * loss = pg_loss + vf_coef v_loss + bc_loss_coeff bc_loss (the DPPO algorithm; the reference computes bc_loss at
 * model/diffusion/diffusion_ppo.py:63-71 and comments the term out of the loss at
 * agent/finetune/train_ppo_diffusion_agent.py:340-342, so parity is unpinned).
 * For n observations cond [n][cond_steps*obs_dim] and the chains [n][K'+1][horizon*action_dim] the caller sampled
 * from the frozen BASE policy (every denoising step on the base actor; dppo_sample with packed_ft = packed_base),
 * row g = (sample g / K', step j = g % K') as in dppo_logprob:
 *   lp[g][q] = Normal(mu_ft(chains[i][j], t = K'-1-j), clip(sigma_t, min_logprob_std, 1e6)).log_prob(chains[i][j+1])
 *   bc_loss  = -sum_{g,q} clip(lp, -5, 2) / (global_samples K' horizon*action_dim)     over EVERY element q
 * metrics[DPPO_METRIC_BC_LOGPROB] (fp64, device) receives this call's sum of clip(lp, -5, 2); grads[0 : actor_count]
 * receive coeff * loss_scale * d bc_loss / d actor_ft: d / d lp = -coeff loss_scale / (global_samples K' XD) where
 * -5 <= lp <= 2 (the bounds pass the gradient, as tf.clip_by_value does) and 0 elsewhere, then the PPO update's own
 * chain (mu, clip(x_recon) under the schedule table's record as in dppo_logprob, the row tile's backward, the
 * actor's weight-gradient launch and time-MLP backward). The chains are data and carry no gradient. It runs the
 * TRAIN instantiations of the actor row tile over rows = n K' rows: dppo_ppo_plan{,_act}(DPPO_PLAN_TRAIN, rows)
 * reports the tile. Workspace: dppo_ppo_workspace_bytes(d, precision, n * K'), any contents.
 * flags: DPPO_PPO_L2_DEFERRED (the factored l2 form of dppo_ppo_minibatch) and DPPO_BC_ACCUMULATE.
 *   without DPPO_BC_ACCUMULATE: grads[0 : actor_count] and the metric slot are OVERWRITTEN;
 *   with it: nothing is zeroed and both are ADDED to, so a caller puts the term on top of a PPO minibatch's actor
 *     gradients (both factored, or both materialised) or walks a large batch in chunks of samples over one
 *     workspace. The call forms its gradient in a per-stream scratch buffer the library keeps (actor_count floats,
 *     allocated on the stream's first such call) and adds it in one launch.
 *   grads beyond the actor's count and every other metric slot are untouched in both forms.
 *   accepted: every precision, both row tiles (32 and 64 rows), every activation, both heads, DDPM and DDIM tables,
 *     a table record with any bound or x0-prediction (as dppo_logprob), global_samples >= n (a data-parallel
 *     rank's share: global_samples over all ranks, loss_scale the minibatch's), coeff >= 0 (0: zero gradients).
 *   refused with DPPO_EINVAL and a message of its own, nothing enqueued, outputs untouched:
 *     a null pointer                          "dppo_bc_minibatch: null pointer"
 *     n < 1                                   "dppo_bc_minibatch: n < 1"
 *     global_samples < n                      "dppo_bc_minibatch: global_samples < n"
 *     a NaN or negative coeff                 "dppo_bc_minibatch: coeff must be >= 0"
 *     DPPO_PPO_LEARN_ETA                      "dppo_bc_minibatch: DPPO_PPO_LEARN_ETA is not supported ..." (the
 *                                             term's derivative with respect to a learnable eta is out of scope)
 *     any other flag bit                      "dppo_bc_minibatch: unknown flags 0x%x"
 *   refused with DPPO_EUNSUPPORTED on the lines of the geometry table above that dppo_ppo_minibatch's actor half is
 *   refused on: ft_denoising_steps > 64 ("dppo_bc_minibatch: ft_denoising_steps %d > 64 unsupported (bucket
 *   sums)"), a geometry without a TRAIN instantiation and the 64-row tile's LDS line ("actor row tile needs %zu B
 *   LDS"), the dispatch's own messages.
 * tests/test_bc_grad_gpu.py pins this. ---- */
enum { DPPO_METRIC_BC_LOGPROB = 9 };   /* metric slot: sum of clip(lp, -5, 2) over the call's (or calls') elements */
enum { DPPO_BC_ACCUMULATE = 16 };      /* dppo_bc_minibatch's flags; shares the bit space of DPPO_PPO_* */
DPPO_API int dppo_bc_minibatch(const dppo_dims* d, int precision, const void* packed_ft, const float* actor_params,
                               const float* sched, const float* cond, const float* chains, int n,
                               int64_t global_samples, float min_logprob_std, float coeff, float loss_scale, int flags,
                               void* workspace, float* grads, double* metrics, void* stream);

/* One half of dppo_ppo_minibatch on the caller's stream, so a caller can overlap the critic's half
 * of minibatch i+1 with the actor's tail of minibatch i: part 1 = the actor (zeroes the actor
 * gradients and metrics 0, 2..15; row tiles, dW, time-MLP backward; needs adv_stats), part 2 =
 * the critic (zeroes the critic gradients and metric 1; row tiles, dW). Part 1 also splits in two
 * (ABI 6): part 4 = the actor's zeroing + row tiles (its loss metrics are final after it), part 5 =
 * the actor's dW + time-MLP backward, so a data-parallel caller can all-reduce the metrics with the
 * critic's gradients while the actor's dW runs. Same arguments and results as dppo_ppo_minibatch,
 * which runs both halves (the critic on an internal side stream). */
/* ABI 11: the non-gradient byte ranges part (1/4 = actor, 2 = critic, 3 = whole) of a minibatch of
 * batch_rows rows zeroes before it runs (metric slots of `metrics`, workspace accumulators): up to 3,
 * their count in *count. A caller passes them to the preceding dppo_optimizer_step_ex to run that
 * minibatch with DPPO_PPO_PRECLEARED. */
DPPO_API int dppo_ppo_clear_ranges(const dppo_dims* d, int precision, int batch_rows, void* workspace, double* metrics,
                                   int part, void** ptrs, size_t* bytes, int* count);
/* The same for a critic with the given attributes (dppo_pack_critic_ln). A layer-normed critic's dgamma / dbeta
 * are accumulated in the tail of the gradient range, which the step's DPPO_STEP_CLEAR_GRADS clears with the range
 * it steps, so the ranges reported are dppo_ppo_clear_ranges'; an attribute outside its enum is DPPO_EINVAL. */
DPPO_API int dppo_ppo_clear_ranges_ln(const dppo_dims* d, int precision, int critic_head, int critic_layernorm,
                                      int batch_rows, void* workspace, double* metrics, int part, void** ptrs,
                                      size_t* bytes, int* count);
DPPO_API int dppo_ppo_minibatch_part(const dppo_dims* d, int precision, const dppo_ppo_hparams* hp,
                            const void* packed_ft, const void* packed_critic, const float* actor_params,
                            const float* sched, const float* obs, const float* chains, const float* lp_old_mean,
                            const float* advantages, const float* returns, int64_t total, uint64_t perm_seed,
                            int epoch, int64_t start, int rows, const int64_t* row_index, const double* adv_stats,
                            void* workspace, float* grads, double* metrics, int part, void* stream);

/* Feistel permutation used above, exposed for tests: out[i] = perm(first + i), i < count. */
DPPO_API int dppo_feistel_permute(int64_t first, int64_t count, int64_t n, uint64_t seed, int epoch, int64_t* out,
                         void* stream);

/* ---- a14: optimiser step over a flat fp32 buffer (Keras 3 AdamW semantics by default;
 * train_ppo_agent.py:45-49). step is 1-based. ---- */
DPPO_API int dppo_adamw(float* params, const float* grads, float* m, float* v, int64_t n, int64_t step, float lr,
               float weight_decay, float beta1, float beta2, float eps, int mode, void* stream);

/* Re-derive the packed images of the actor and/or the critic (either pair may be null) in ONE
 * launch; the actor's includes its time tables. = dppo_pack_actor + dppo_pack_critic. */
DPPO_API int dppo_pack_all(const dppo_dims* d, int precision, const float* actor_params, void* packed_actor,
                  const float* critic_params, void* packed_critic, void* stream);

/* One optimiser step after a PPO minibatch as two launches on `stream`
 * (train_ppo_diffusion_agent.py:346 apply_gradients, then the weight images every kernel reads):
 * dppo_adamw over the n elements at params/grads/m/v (a range of the flat [actor | critic]
 * buffer), which also copies n_metrics (<= 256) doubles of `metrics` to `metrics_out` (device or
 * host-mapped memory; the minibatch's metric sums for the host's target_kl check), then
 * dppo_pack_all of the given networks. ABI 5: a nonzero metrics_tag (< 2^53) is stored as the
 * double metrics_out[n_metrics] AFTER the n_metrics sums (system-scope release), so a host polling
 * host-mapped metrics_out for the tag reads complete sums without recording or waiting on an event
 * (metrics_out then holds n_metrics + 1 doubles; pass 0 for no tag). */
/* ABI 8: the actor's l2 gradient of a DPPO_PPO_L2_DEFERRED minibatch, formed in place in grads (the
 * actor range first) from the factored form; workspace = the minibatch's (its pl2 slot is the
 * staging copy). */
DPPO_API int dppo_materialize_l2(const dppo_dims* d, int precision, const void* packed_actor, float* grads,
                                 void* workspace, int batch_rows, void* stream);

/* Enqueue the split-sampler tables of an actor image on `stream` if an optimizer step with
 * DPPO_STEP_DEFER_SAMPLER_TABLES left them stale; a no-op otherwise (ABI 7). */
DPPO_API int dppo_refresh_sampler_tables(const void* packed_actor, void* stream);

/* Supported geometry of the optimizer step (dppo_optimizer_step, _ex and _clip, every form: staged,
 * DPPO_STEP_FUSED_PACK, DPPO_STEP_CLEAR_GRADS, DPPO_STEP_L2_FROM_PL2, the clip scales). The step kernels have
 * no per-geometry instantiations (the tile step takes each tensor's rows, columns and k-steps as arguments),
 * so the step runs wherever the dimension check and the pack of the images accept the model: hidden widths
 * 128/256/384/512, horizon_steps*action_dim <= 32, cond_steps*obs_dim <= 64, any input width, and for an
 * actor image time_dim <= 32 with time_dim a multiple of 4 (the fold that follows every actor pack wants
 * W_in 16-B aligned in the flat layout). That is wider than the row tiles' table above: an actor the update
 * entries refuse (actor_hidden 256 or fewer than 33 inputs in fp32) still steps and packs.
 *   geometry (tests/test_optimizer_step_gpu.py)      fp32   bf16   fp16
 *   hopper (XD 12, 39 inputs), walker (XD 24, 57)    runs   runs   runs
 *   horizon 8 x action 4 (XD 32)                     runs   runs   runs
 *   time_dim 32, actor_hidden 256                    runs   runs   runs
 *   cond_steps 2 walker (74 inputs), obs 3 action 1  runs   runs   runs
 * A staged step over [actor | critic] with both images and clear ranges zeroes the ranges in a launch of
 * its own (the two images fill the pack launch's job table). */
DPPO_API int dppo_optimizer_step(const dppo_dims* d, int precision, float* params, const float* grads, float* m,
                        float* v, int64_t n, int64_t step, float lr, float weight_decay, float beta1,
                        float beta2, float eps, int mode, const float* actor_params, void* packed_actor,
                        const float* critic_params, void* packed_critic, const double* metrics,
                        double* metrics_out, int n_metrics, uint64_t metrics_tag, void* stream);
/* ABI 11: dppo_optimizer_step that also zeroes n_clear (<= 4) byte ranges (4-B aligned, sizes multiples
 * of 4) after the launch's last read, and with DPPO_STEP_CLEAR_GRADS the gradients of the range. */
DPPO_API int dppo_optimizer_step_ex(const dppo_dims* d, int precision, float* params, float* grads, float* m,
                           float* v, int64_t n, int64_t step, float lr, float weight_decay, float beta1,
                           float beta2, float eps, int mode, const float* actor_params, void* packed_actor,
                           const float* critic_params, void* packed_critic, const double* metrics,
                           double* metrics_out, int n_metrics, uint64_t metrics_tag, void* const* clear_ptrs,
                           const size_t* clear_bytes, int n_clear, void* stream);

/* ---- a13, the clip branch: tf.clip_by_norm(grad, 1.0) per variable when train.max_grad_norm is set
 * (agent/finetune/train_ppo_diffusion_agent.py:349-354), as two device-side pieces so a clipped update
 * keeps the split, fused, pre-cleared schedule (additions within ABI 15).
 * dppo_grad_clip_scales: the clip scale of every variable of a network in ONE launch on stream. nets
 * ORs DPPO_NET_ACTOR (the 12 actor variables of the flat layout above) and DPPO_NET_CRITIC (the 8 critic
 * variables); 3 = the flat [actor | critic] range. grads is that range (fp32); norms (may be NULL) and
 * scales are device fp32, one entry per variable in layout order:
 *   norm[v] = sqrt(sum g^2),  scale[v] = clip_norm / max(norm[v], clip_norm)
 * so scale is exactly 1.0f where norm <= clip_norm (a zero tensor included) and grad * scale is
 * tf.clip_by_norm(grad, clip_norm). Every square is formed and summed in fp64 (exact products of fp32
 * inputs), in a fixed order without floating-point atomics: each variable is cut into chunks that never
 * cross a variable boundary, each chunk's workgroup stores one partial sum into workspace
 * (dppo_grad_clip_workspace_bytes(d, nets) bytes, 8-B aligned, contents don't matter), and the last
 * workgroup to arrive adds each variable's partials in chunk order. Two launches on the same data give
 * the same bits. clip_norm must be > 0. */
enum { DPPO_NET_ACTOR = 1, DPPO_NET_CRITIC = 2 };
DPPO_API size_t dppo_grad_clip_workspace_bytes(const dppo_dims* d, int nets);
DPPO_API int dppo_grad_clip_scales(const dppo_dims* d, int nets, const float* grads, float clip_norm, float* norms,
                                   float* scales, void* workspace, void* stream);
/* The same over a critic with the given attributes (dppo_pack_critic_ln): a layer-normed critic's gamma / beta
 * vectors are variables of their own behind out_b (8 + 4 residual, 8 + 6 plain: 12 or 14 critic entries, 24 or 26
 * with the actor). The forms above are these with DPPO_HEAD_RESIDUAL, DPPO_LN_OFF. */
DPPO_API size_t dppo_grad_clip_workspace_bytes_ln(const dppo_dims* d, int nets, int critic_head, int critic_layernorm);
DPPO_API int dppo_grad_clip_scales_ln(const dppo_dims* d, int nets, int critic_head, int critic_layernorm,
                                      const float* grads, float clip_norm, float* norms, float* scales, void* workspace,
                                      void* stream);
/* dppo_optimizer_step_ex whose AdamW reads each gradient as the fp32 product g[i] * clip_scales[v]
 * (rounded once, before any moment update: the step equals multiplying the gradients by the expanded
 * scale table and running dppo_optimizer_step_ex, bit for bit). clip_scales is device fp32, one per
 * variable of the range in layout order (dppo_grad_clip_scales' output; read by the launch, never by the
 * host); the range must be exactly the actor, the critic or [actor | critic], as nets says. Every path
 * (staged, DPPO_STEP_FUSED_PACK, DPPO_STEP_CLEAR_GRADS, the clear ranges, the metrics copy and its tag)
 * behaves as in dppo_optimizer_step_ex. DPPO_STEP_L2_FROM_PL2 is refused (DPPO_EINVAL): the factored l2
 * gradient has no norm before it is formed.
 * The critic's variables follow its image's attributes (8, or 12 / 14 for a layer-normed critic, dppo_pack_critic_ln).
 * Without a critic image (packed_critic NULL: a step that packs nothing) there is no attribute to read, and the
 * layout is told by n: a critic part of 8-tensor length plus 4 or 6 vectors of critic_hidden is taken as the
 * layer-normed residual or plain layout (the three lengths differ at every accepted geometry), any other length must
 * be the 8-tensor layout's. clip_scales must hold that layout's entries. */
DPPO_API int dppo_optimizer_step_clip(const dppo_dims* d, int precision, float* params, float* grads, float* m,
                           float* v, int64_t n, int64_t step, float lr, float weight_decay, float beta1,
                           float beta2, float eps, int mode, const float* actor_params, void* packed_actor,
                           const float* critic_params, void* packed_critic, const double* metrics,
                           double* metrics_out, int n_metrics, uint64_t metrics_tag, void* const* clear_ptrs,
                           const size_t* clear_bytes, int n_clear, void* stream, const float* clip_scales, int nets);

/* ---- ABI 12, §8(e): the data-parallel gradient all-reduce as one kernel over IPC-mapped peer
 * buffers (the reference has no collective: it applies gradients on one device,
 * train_ppo_diffusion_agent.py:345-356, script/run.py:82; RCCL's all_reduce is the default here).
 * Every rank allocates one region of dppo_ipc_region_bytes(capacity) with dppo_ipc_alloc (device
 * memory, zeroed; handle = 64 bytes for hipIpcOpenMemHandle), exchanges the handles out of band
 * (torch.distributed) and opens every peer's with dppo_ipc_open. dppo_ipc_allreduce then sums
 * data[0, n) (fp32, n <= capacity) over the ranks IN PLACE on every rank, in rank order 0..W-1 (so
 * every rank gets the same bits: a sequential fp32 sum): regions[x] = rank x's region as mapped in
 * this process (regions[rank] = the own one), world <= 8, generation = 1, 2, ... the same on every
 * rank for the same call; every rank must make the same calls in the same order, one launch each on
 * its stream. A barrier that waits more than ~2 s sets *fail_host (dppo_host_alloc memory) and the
 * next call returns DPPO_EHIP. */
DPPO_API size_t dppo_ipc_region_bytes(int64_t capacity);
DPPO_API int dppo_ipc_alloc(size_t bytes, void** ptr, void* handle);
DPPO_API int dppo_ipc_open(const void* handle, void** ptr);
DPPO_API int dppo_ipc_close(void* ptr);
DPPO_API int dppo_ipc_free(void* ptr);
DPPO_API int dppo_ipc_allreduce(void* const* regions, int world, int rank, int64_t capacity, float* data, int64_t n,
                                uint64_t generation, uint32_t* fail_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DPPO_H */
