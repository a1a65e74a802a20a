"""Cases, inputs and float64 references of the pretraining step (tests/test_pretrain_step_cpu.py,
tests/test_pretrain_step_gpu.py): dppo_pretrain_minibatch (csrc/update.hip) at its edges, and
TrainDiffusionAgent.train_epoch / run teacher-forced against the oracle step by step.

Every reference is oracle/ code: O.p_losses (with denom= for a data-parallel shard and rnd= for the kernels'
rounding points, round_fp16_rows included), O.keras_adamw_step through helpers.adamw_oracle. None calls the
library, and nothing here imports torch. The CPU file shows that the inputs are what the cases say and that
each check can fail; the GPU file runs the kernels on them.

Error measure, per gradient tensor: max |g - ref| / (max |ref| + 1e-12); the loss relative to the oracle's.
Bounds: fp32 2e-3; bf16 and fp16 1e-2 against the oracle rounding at the kernels' rounding points."""
import functools
import math

import numpy as np

from oracle import dppo_oracle as O
from tests.helpers import HOPPER, make_models, step_hp, to_f64

BOUND = {"fp32": 2e-3, "bf16": 1e-2, "fp16": 1e-2}
PRECISIONS = ("fp32", "bf16", "fp16")
FP16_MAX = 65504.0


def rnd_of(precision):
    """the oracle's rounding points of a precision (tests/test_kernels_gpu.py _rnd)"""
    return {"bf16": O.round_bf16, "fp16": O.round_fp16}.get(precision)


def dims_of(K):
    """hopper with K denoising steps (the pretraining entry reads denoising_steps only)"""
    return HOPPER if K == HOPPER["denoising_steps"] else dict(HOPPER, denoising_steps=K, ft_denoising_steps=1)


@functools.lru_cache(maxsize=None)
def model(K):
    """(the fine-tuned actor of helpers.make_models(0, dims_of(K)) in float64, the DDPM schedule over K steps):
    what tests/test_kernels_gpu.py _setup hands the kernels for the same dims"""
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    _, ft, _ = make_models(0, dims_of(K))
    return to_f64(ft), ddpm_buffers(K)


# ------------------------------------------------------------------------------------------------
# Part A: one launch of dppo_pretrain_minibatch per case
# ------------------------------------------------------------------------------------------------
XD, SD = HOPPER["horizon_steps"] * HOPPER["action_dim"], HOPPER["cond_steps"] * HOPPER["obs_dim"]

T_PATTERNS = ("cycle", "all0", "allK-1", "ends", "single7", "uniform")


def t_of(pattern, rows, K, rng=None):
    """cycle: arange(rows) % K (min(rows, K) buckets, each with rows // K or one more row); all0 / allK-1: one
    bucket; ends: {0, K - 1} alternating; single7: every row at t = 3 but row rows // 2 + 1 at t = 7;
    uniform: rng.integers (the recipe of test_pretrain_loss_grads)."""
    r = np.arange(rows)
    if pattern == "cycle":
        t = r % K
    elif pattern == "all0":
        t = np.zeros(rows)
    elif pattern == "allK-1":
        t = np.full(rows, K - 1)
    elif pattern == "ends":
        t = np.where(r % 2 == 0, 0, K - 1)
    elif pattern == "single7":
        t = np.full(rows, 3)
        t[rows // 2 + 1] = 7
    else:
        t = rng.integers(0, K, rows)
    return t.astype(np.int32)


def inputs(rows, K, pattern="cycle", seed=0, x0_edge=False, noise_scale=1.0):
    """fp32 (x0 [rows, XD] in [-1, 1], cond [rows, SD], t [rows] int32 in [0, K), noise [rows, XD]).
    x0_edge: x0 exactly +-1 (the clip edge of the data); noise_scale: noise ~ noise_scale N(0, 1)."""
    rng = np.random.default_rng([31, rows, K, T_PATTERNS.index(pattern), seed])
    x0 = rng.uniform(-1, 1, (rows, XD)).astype(np.float32)
    if x0_edge:
        x0 = np.where(x0 < 0, -1.0, 1.0).astype(np.float32)
    cond = rng.uniform(-1, 1, (rows, SD)).astype(np.float32)
    noise = (noise_scale * rng.standard_normal((rows, XD))).astype(np.float32)
    t = t_of(pattern, rows, K, rng)
    assert t.min() >= 0 and t.max() < K          # the entry does not validate t
    return dict(x0=x0, cond=cond, t=t, noise=noise)


def recipe150(dims=HOPPER):
    """the inputs of test_pretrain_loss_grads (tests/test_kernels_gpu.py): 150 rows, rng 21, t uniform"""
    rng = np.random.default_rng(21)
    rows, K = 150, dims["denoising_steps"]
    xd, sd = dims["horizon_steps"] * dims["action_dim"], dims["cond_steps"] * dims["obs_dim"]
    x0 = rng.uniform(-1, 1, (rows, xd)).astype(np.float32)
    cond = rng.uniform(-1, 1, (rows, sd)).astype(np.float32)
    t = rng.integers(0, K, rows).astype(np.int32)
    noise = rng.standard_normal((rows, xd)).astype(np.float32)
    return dict(x0=x0, cond=cond, t=t, noise=noise)


def reference(p, sched, inp, rnd=None, global_rows=None, loss_scale=1.0, dims=HOPPER):
    """(loss, gradients) of O.p_losses on the case's rows in float64, for the actor the dims describe: the mean over global_rows * XD elements
    (denom=, a data-parallel shard's share; fp16 then rounds its gradient images with round_fp16_rows(
    global_rows)), times loss_scale."""
    Ta, Da, To, Do = dims["horizon_steps"], dims["action_dim"], dims["cond_steps"], dims["obs_dim"]
    rows = inp["x0"].shape[0]
    f = lambda x, a, b: np.asarray(x, np.float64).reshape(rows, a, b)
    denom = None if global_rows is None else int(global_rows) * Ta * Da
    loss, g = O.p_losses(p, sched, f(inp["x0"], Ta, Da), f(inp["cond"], To, Do), inp["t"], f(inp["noise"], Ta, Da),
                         rnd=rnd, denom=denom, model=O.Model.from_dims(dims))
    return loss * loss_scale, {k: v * loss_scale for k, v in g.items()}


def errors(got, ref):
    """per tensor max |g - ref| / (max |ref| + 1e-12)"""
    return {k: float(np.abs(np.asarray(got[k], np.float64) - r).max() / (np.abs(r).max() + 1e-12)) for k, r in ref.items()}


def subset(inp, keep):
    return {k: v[keep] for k, v in inp.items()}


# 1. row counts around the 16 / 32-row tiles, the 64-padded ldm and the padded rows (segment id -1)
ROWS_CASES = [(rows, p) for rows in (1, 15, 16, 17, 33, 64, 65) for p in PRECISIONS
              if p != "fp16" or rows in (1, 17, 65)]
# 2. populations of t: K = 20, 70 rows
POP_ROWS, POP_PATTERNS, POP_PRECISIONS = 70, ("all0", "allK-1", "ends", "single7"), ("fp32", "bf16")
# 3. K edges: (K, rows); K = 64 fills every bin of the bucket sums and reaches the int8 id 63
K_CASES = [(1, 17), (2, 17), (64, 70)]
K_REJECTED = 65
# the 64-row tile's LDS line: hopper needs 161,616 + 96 K bytes, K = 23 the last that fits 160 KiB
TILE64_K_OK, TILE64_K_REFUSED = 23, 24
TILE64_LDS = lambda K: 161616 + 96 * K
# 4. a data-parallel shard: 40 of 160 rows, and a loss scale
SHARD_ROWS, SHARD_GLOBAL, SHARD_SCALES = 40, 160, (0.25, 3.0)
# 5. the buffer contract
CONTRACT_ROWS, CONTRACT_PRECISIONS, CONTRACT_TAIL = 70, ("fp32", "bf16"), 64
REUSE_ROWS = (256, 100)
# 7. fp16 at magnitude: x0 = +-1, noise at 3 N(0, 1) (the CPU file shows the oracle's rounded intermediates
# stay below 65504 at this scale)
MAG_ROWS, MAG_NOISE = (1, 17), 3.0


def recording_fp16(global_rows):
    """round_fp16_rows(global_rows) that records the largest magnitude handed to each of its two roundings, in
    the units the kernels store: forward operands as they are, gradient images times the row-tied scale."""
    base, sc = O.round_fp16_rows(global_rows), O.fp16_grad_scale(global_rows)
    peak = {"forward": 0.0, "backward": 0.0}

    def note(key, x, f):
        peak[key] = max(peak[key], float(np.abs(np.asarray(x, np.float64)).max()) * f)

    def rnd(x):
        note("forward", x, 1.0)
        return base(x)

    def grad_round(x):
        note("backward", x, sc)
        return base.grad_round(x)
    rnd.grad_round = grad_round
    return rnd, peak


# ------------------------------------------------------------------------------------------------
# Part B: the pretraining step over a run
# ------------------------------------------------------------------------------------------------
# cfg/gym/pretrain/hopper-medium-v2/pre_diffusion_mlp on synthetic_dataset(n_episodes=2, episode_len=40): 64
# windows, so batch_size 48 gives two batches per epoch, 48 rows and a short one of 16; three epochs = six
# optimizer steps, with the schedule's restart (first_cycle_steps 4) at step 5.
# weight_decay: the cfg's own 1e-6 moves a parameter by |p| 1e-6 lr = 7e-11 per step, a thousandth of one fp32
# rounding of p, so no bound could tell it from 0; the run overrides it to 0.1 (|p| 1e-4 per step), which
# differs from the cfg file's value, from AdamW's default 0.004 and from 0 by far more than the step's bound.
RUN = dict(n_episodes=2, episode_len=40, batch_size=48, n_epochs=3, epoch_start_ema=2, update_ema_freq=1,
           learning_rate=1e-3, first_cycle_steps=4, weight_decay=0.1)
RUN_OVERRIDES = [f"train.{k}={RUN[k]}" for k in ("batch_size", "n_epochs", "epoch_start_ema", "update_ema_freq",
                                                  "learning_rate", "weight_decay")] + \
    [f"train.lr_scheduler.first_cycle_steps={RUN['first_cycle_steps']}"]
BETA1, BETA2, EPS = 0.9, 0.999, 1e-7      # Keras AdamW as the agent constructs it


def lr_at(index, lr0, first_cycle_steps, min_lr):
    """tf.keras CosineDecayRestarts(lr0, first_cycle_steps, t_mul=1, m_mul=1, alpha=min_lr / lr0) at a 0-based
    optimizer iteration (agent/pretrain/train_agent.py:117-123), restated in float64"""
    alpha = min_lr / lr0
    frac = index / float(first_cycle_steps)
    frac -= math.floor(frac)
    return lr0 * ((1.0 - alpha) * 0.5 * (1.0 + math.cos(math.pi * frac)) + alpha)


def run_hp(i, lr0, first_cycle_steps, min_lr, wd):
    """the hyperparameters of 1-based step i as the kernel receives them"""
    return step_hp(lr_at(i - 1, lr0, first_cycle_steps, min_lr), wd, BETA1, BETA2, EPS)


def ema_expected(ema_prev, params, epoch, epoch_start_ema, decay):
    """(ema after the epoch's step_ema in float64, per-element tolerance): a copy of params before
    epoch_start_ema (tolerance 0), then decay ema + (1 - decay) params within 2 fp32 ulps of |ema| + |params|"""
    params = np.asarray(params, np.float64)
    if epoch < epoch_start_ema:
        return params, np.zeros_like(params)
    ema_prev = np.asarray(ema_prev, np.float64)
    mag = (np.abs(ema_prev) + np.abs(params)).astype(np.float32)
    return decay * ema_prev + (1.0 - decay) * params, 2.0 * np.spacing(mag).astype(np.float64)
