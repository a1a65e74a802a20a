"""The oracle side of the diffusion-parameterisation tests (tests/test_diffusion_param_cpu.py,
tests/test_diffusion_param_gpu.py): denoised_clip_value other than 1.0 (None included) and predict_epsilon=False.

The oracle itself is not edited. `param_oracle(clip, x0)` replaces O.p_mean_var for the duration of a case, in
the manner of tests/plain_oracle.py; O.sample, O.get_logprobs, O.c_loss, O.bc_loss and oracle/iteration.py all
reach it by module attribute.
  * a clip c (or inf for None) is forwarded as the oracle's own `denoised_clip` argument;
  * x0-prediction (reference model/diffusion/diffusion.py:117-134, x_recon = the network's output) hands the
    oracle's p_mean_var a schedule whose reconstruction coefficients are c1 = 0, c2 = -1 (the oracle's names:
    xr = c1 x - c2 eps), so xr = eps and deps = -c2 dxr = +dxr fall out of the oracle's own backward;
  * the learnable-eta term of O.c_loss re-derives x0 with a literal np.clip(..., -1.0, 1.0); `clip_eta=True`
    wraps that line's np.clip too (a clip whose bounds are exactly -1.0 / 1.0 gets the case's bound), for the
    DDIM learnable-eta case only.
`p_losses_x0` restates p_losses with target x_start (diffusion.py:186-194, predict_epsilon=False).

The inputs of the update cases are the regime tests' (tests/test_update_regimes_gpu.py _inputs) with the chains
at unit scale instead of 0.5, so that a tenth of the x_recon values and more lie between 1 and 2 as well as
between 0.5 and 1 (tests/test_diffusion_param_cpu.py asserts it)."""
import contextlib

import numpy as np

from oracle import dppo_oracle as O

INF = float("inf")
# (label, denoised_clip_value as the model takes it, predict_epsilon)
SETTINGS = [("clip0.5", 0.5, True), ("clip2", 2.0, True), ("noclip", None, True), ("x0", 1.0, False)]
SETTING_IDS = [s[0] for s in SETTINGS]


def bound_of(clip):
    return INF if clip is None else float(clip)


@contextlib.contextmanager
def param_oracle(clip=1.0, predict_epsilon=True, clip_eta=False):
    orig, orig_np = O.p_mean_var, O.np
    c = bound_of(clip)

    def p_mean_var(sched, eps, x, t, denoised_clip=1.0):
        if not predict_epsilon:
            n = len(sched["sqrt_recip_alphas_cumprod"])
            sched = dict(sched, sqrt_recip_alphas_cumprod=np.zeros(n), sqrt_recipm1_alphas_cumprod=-np.ones(n))
        return orig(sched, eps, x, t, denoised_clip=c)

    class _Np:   # the oracle module's `np`, with the learnable-eta line's clip at +-1 moved to the case's bound
        def __getattr__(self, name):
            return getattr(orig_np, name)

        @staticmethod
        def clip(a, lo, hi, *args, **kw):
            if isinstance(lo, float) and isinstance(hi, float) and lo == -1.0 and hi == 1.0:
                lo, hi = -c, c
            return orig_np.clip(a, lo, hi, *args, **kw)

    O.p_mean_var = p_mean_var
    if clip_eta:
        O.np = _Np()
    try:
        yield
    finally:
        O.p_mean_var = orig
        O.np = orig_np


def x_recon(sched, eps, x, t, predict_epsilon=True):
    """The unclipped reconstruction the clip acts on, in the oracle's arithmetic."""
    if not predict_epsilon:
        return np.asarray(eps, np.float64)
    sh = (-1,) + (1,) * (x.ndim - 1)
    c1 = sched["sqrt_recip_alphas_cumprod"].astype(np.float64)[np.asarray(t)].reshape(sh)
    c2 = sched["sqrt_recipm1_alphas_cumprod"].astype(np.float64)[np.asarray(t)].reshape(sh)
    return c1 * x - c2 * eps


def p_losses_x0(p, sched, x_start, state, t, noise, with_grad=True, rnd=None, denom=None, round_h3=False):
    """O.p_losses with the x0 target: loss = mean((network(q_sample(x_0, t, noise), t, cond) - x_0)^2)."""
    xn = O.q_sample(sched, x_start, np.asarray(t), noise)
    if rnd is O.round_fp16:
        xd = x_start.shape[1] * x_start.shape[2]
        rnd = O.round_fp16_rows(x_start.shape[0] if denom is None else denom // xd)
    out, cache = O.diffusion_mlp_forward(p, xn, np.asarray(t), state, rnd=rnd, round_h3=round_h3)
    e = out - x_start
    n = e.size if denom is None else denom
    loss = float((e ** 2).sum() / n)
    if not with_grad:
        return loss, None
    return loss, O.diffusion_mlp_backward(p, cache, 2.0 * e / n, x_start.shape[1] * x_start.shape[2])


ALPHA, SHRINK = 1.0 - 2.0 ** -4, 2.0 ** -10


def denoiser_like(p, alpha=ALPHA, shrink=SHRINK):
    """Seeded weights reshaped so that the network behaves like a denoiser near its fixed point, for the sampler
    cases WITHOUT the clip. The sampler surface's bounds are absolute and were set for chains that the clip keeps
    of order 1. Without it x_recon = c0 x - c1 eps is only of order 1 if eps tracks x: at t = K - 1, c0 = c1 = 406,
    and the seeded networks' epsilon of order 1 gives chains of 4.7e3, where the fp32 bound of 2e-4 is below half
    an ulp of the compared values. Here eps = alpha x + shrink (the seeded network's own non-linear output): the
    in-Dense copies x into hidden units 0 .. XD-1 (nothing else reaches them), the l2 branch into those units and
    the whole out-Dense are multiplied by `shrink`, and the out-Dense reads the units back with weight alpha. With
    alpha = 1 - 2^-4 (exact in bf16 and fp16) x_recon = (c0 - alpha c1) x - c1 shrink r is about 25 x at
    t = K - 1 and about x at t = 0: past the bound 1 for most elements of the first steps, so no clip and clip 1
    differ by fifty bounds in the stored chains (tests/test_diffusion_param_cpu.py asserts ten), while x_recon
    stays below 10^2 and the chains below 4. Every layer, both actors and
    the actor switch at t = K' still run on seeded values; the float64 oracle evaluates the same weights."""
    q = {k: np.array(v, copy=True) for k, v in p.items()}
    xd = q["out_w"].shape[1]
    i = np.arange(xd)
    q["in_w"][:, :xd] = 0
    q["in_w"][i, i] = 1
    q["in_b"][:xd] = 0
    q["l2_w"][:, :xd] *= shrink
    q["l2_b"][:xd] *= shrink
    q["out_w"] *= shrink
    q["out_b"] *= shrink
    q["out_w"][i, i] = alpha
    return {k: v.astype(p[k].dtype) for k, v in q.items()}


def sampler_models(inp, clip):
    """(base, ft) of a sampler case: the inputs' seeded models, denoiser_like without the clip."""
    if clip is None:
        return denoiser_like(inp.base), denoiser_like(inp.ft)
    return inp.base, inp.ft


def update_inputs(d, N, f32_draws=False):
    """tests/test_update_regimes_gpu.py _inputs with unit-scale chains (same generator, same order of draws)."""
    rng = np.random.default_rng(12)
    kf = d.ft_denoising_steps
    obs = rng.uniform(-1, 1, (N, d.sd)).astype(np.float32)
    chains = rng.standard_normal((N, kf + 1, d.xd)).astype(np.float32)
    adv = rng.normal(size=N).astype(np.float32)
    ret = rng.normal(size=N).astype(np.float32)
    return rng, obs, chains, adv, ret
