"""Test data of the model variants: dims, seeded models and inputs for the Mish / ELU / GELU / Softplus actors, the
plain actor head, the plain and the layer-normed critic, and the diffusion parameterisation (denoised_clip_value,
predict_epsilon). No oracle code lives here: the float64 oracle takes the variant as an argument
(O.Model.from_dims(dims), O.with_param(sched, clip, predict_epsilon))."""
import numpy as np

from tests.helpers import HOPPER, WALKER, make_models

MISH = dict(activation="Mish")
HOPPER_MISH = dict(HOPPER, **MISH)
WALKER_MISH = dict(WALKER, **MISH)
NEW_ACTIVATIONS = ("ELU", "GELU", "Softplus")
ALL_ACTIVATIONS = ("ReLU", "Mish") + NEW_ACTIVATIONS
PLAIN = dict(head="plain")
HOPPER_PLAIN = dict(HOPPER, **PLAIN)
WALKER_PLAIN = dict(WALKER, **PLAIN)
PLAIN_CRITIC = dict(critic_head="plain")
HOPPER_PLAIN_CRITIC = dict(HOPPER, **PLAIN_CRITIC)
HOPPER_LN = {"residual": dict(HOPPER, critic_layernorm=True),
             "plain": dict(HOPPER, critic_head="plain", critic_layernorm=True)}
# N(0, BIAS_SCALE) biases put h1 and h2 on both sides of zero and past x < -1, where mish' < 0
# (site_coverage asserts it on the oracle's cache; make_models' default 0.05 leaves h within +-1)
BIAS_SCALE = 1.0


def dims_of(name, dims=HOPPER, **extra):
    """dims with the `activation` key (and any other, e.g. head="plain")."""
    return dict(dims, activation=name, **extra)


def mish_models(seed=0, dims=HOPPER, bias_scale=BIAS_SCALE, ft_perturb=0.02):
    """tests.helpers.make_models with the Mish tests' bias scale."""
    return make_models(seed, dims, bias_scale=bias_scale, ft_perturb=ft_perturb)


def site_coverage(cache):
    """Fractions of h1 / h2 below -1 and above 0, asserted: >= 5 % and >= 20 % at both sites."""
    out = {}
    for k in ("h1", "h2"):
        h = np.asarray(cache[k])
        out[k] = (float((h < -1).mean()), float((h > 0).mean()))
        assert out[k][0] >= 0.05 and out[k][1] >= 0.20, (k, out[k])
    return out


def add_ln_params(critic, head, rng, scale=1.0):
    """The critic's eight tensors plus random norms: gamma ~ U(0.5, 1.5), beta ~ N(0, scale) (not 1 and 0)."""
    h = critic["in_b"].shape[0]
    out = dict(critic)
    for k in range(1, (3 if head == "plain" else 2) + 1):
        out[f"ln{k}_g"] = rng.uniform(0.5, 1.5, h).astype(np.float32)
        out[f"ln{k}_b"] = rng.normal(0, scale, h).astype(np.float32)
    return out


def sampler_self_noise(inputs, precision, seed, rel=2e-7):
    """The ORACLE's own sensitivity at its rounding points, no kernel involved: O.sample on `inputs` (a
    tests.test_sampler_surface_gpu._Inputs, under its dims' activation) against O.sample with every operand scaled
    by 1 + rel N(0, 1) just before it is rounded, in the sampler statistics (SS._stats).
    rel = 2e-7 is the size of the error an fp32 sum of a few hundred terms carries into the rounding that the
    float64 oracle does not: the only way the kernel and the oracle, which round the same operands at the same
    points, come to differ."""
    from tests import test_sampler_surface_gpu as SS
    clean = inputs.oracle(precision)
    R, rng, orig = SS._rnd(precision), np.random.default_rng(seed), SS._rnd

    def noisy(x):
        x = np.asarray(x, np.float64)
        return R(x * (1.0 + rel * rng.standard_normal(x.shape)))

    SS._rnd = lambda _precision: noisy
    try:
        other = inputs.oracle(precision)
    finally:
        SS._rnd = orig
    return SS._stats(other[0], other[1], clean[0], clean[1])


# ------------------------------------------------------------------------------------------------
# the diffusion parameterisation (tests/test_diffusion_param_cpu.py, tests/test_diffusion_param_gpu.py).
# The inputs of the update cases are the regime tests' (tests/test_update_regimes_gpu.py _inputs) with the chains
# at unit scale instead of 0.5, so that a tenth of the x_recon values and more lie between 1 and 2 as well as
# between 0.5 and 1 (tests/test_diffusion_param_cpu.py asserts it).
# ------------------------------------------------------------------------------------------------
INF = float("inf")
# (label, denoised_clip_value as the model takes it, predict_epsilon)
SETTINGS = [("clip0.5", 0.5, True), ("clip2", 2.0, True), ("noclip", None, True), ("x0", 1.0, False)]
SETTING_IDS = [s[0] for s in SETTINGS]


def bound_of(clip):
    return INF if clip is None else float(clip)


def x_recon(sched, eps, x, t, predict_epsilon=True):
    """The unclipped reconstruction the clip acts on, in the oracle's arithmetic."""
    if not predict_epsilon:
        return np.asarray(eps, np.float64)
    sh = (-1,) + (1,) * (x.ndim - 1)
    c1 = sched["sqrt_recip_alphas_cumprod"].astype(np.float64)[np.asarray(t)].reshape(sh)
    c2 = sched["sqrt_recipm1_alphas_cumprod"].astype(np.float64)[np.asarray(t)].reshape(sh)
    return c1 * x - c2 * eps


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
