"""Shared fixtures for the parity tests: seeded synthetic weights and inputs."""
import numpy as np

from oracle import dppo_oracle as O

HOPPER = dict(obs_dim=11, action_dim=3, horizon_steps=4, cond_steps=1, time_dim=16, actor_hidden=512,
              critic_hidden=256, denoising_steps=20, ft_denoising_steps=10)
WALKER = dict(HOPPER, obs_dim=17, action_dim=6)
# an action width the kernels do not specialise (XD = 8: padded to the generic 32-wide instantiation)
NARROW = dict(HOPPER, action_dim=2)
# BASELINE config 5: DDIM, 10 sampling rows over K = 20 (time stride 2), all fine-tuned
HOPPER_DDIM = dict(HOPPER, denoising_steps=10, ft_denoising_steps=10, time_stride=2)


def make_models(seed=0, dims=HOPPER, bias_scale=0.05, ft_perturb=0.02):
    rng = np.random.default_rng(seed)
    base = O.init_actor(rng, dims["obs_dim"], dims["action_dim"], dims["horizon_steps"], dims["cond_steps"],
                        dims["time_dim"], dims["actor_hidden"], bias_scale=bias_scale)
    ft = {k: (v + rng.normal(0, ft_perturb, v.shape).astype(np.float32)) for k, v in base.items()}
    critic = O.init_critic(rng, dims["obs_dim"], dims["cond_steps"], dims["critic_hidden"], bias_scale=bias_scale)
    return base, ft, critic


def to_f64(p):
    return {k: np.asarray(v, np.float64) for k, v in p.items()}


# ------------------------------------------------------------------------------------------------
# The optimizer step against the float64 oracle, one step at a time
# (tests/test_optimizer_step_cpu.py, tests/test_optimizer_step_gpu.py)
# ------------------------------------------------------------------------------------------------
U32 = 2.0 ** -24        # fp32 unit roundoff
STEP_C = 8.0            # roundings allowed per quantity (see adamw_oracle)
TINY = float(np.finfo(np.float32).tiny)
# name -> (lr, weight_decay, beta1, beta2, eps). "default" is the shipped optimizer; "off" moves every
# knob; its lr is large enough that weight_decay * lr (1e-3) is far above STEP_C * U32
STEP_HP = {
    "default": (1e-4, 0.004, 0.9, 0.999, 1e-7),
    "off": (1e-2, 0.1, 0.5, 0.9, 1e-3),
    "wd0": (1e-4, 0.0, 0.9, 0.999, 1e-7),
    "lr0": (0.0, 0.004, 0.9, 0.999, 1e-7),
}
STEP_NUMBERS = (1, 2, 1000, 100000)


def step_hp(lr, wd, beta1, beta2, eps):
    """The hyperparameters the kernel receives: each rounded to fp32 (the C ABI's floats), as float64."""
    r = lambda x: float(np.float64(np.float32(x)))
    return dict(lr=r(lr), wd=r(wd), beta1=r(beta1), beta2=r(beta2), eps=r(eps))


def step_inputs(n, seed=0):
    """(p, m, v, g) fp32 for an optimizer step over n elements: p, g ~ N(0, 0.05), m ~ N(0, 1e-3),
    v ~ U(1e-8, 1e-5); exact zeros in g (every 7th element), m = v = 0 as before a first step (every
    11th; both with g = 0 every 77th), |g| near 1e3 (every 97th). Element 0 is generic. No subnormals:
    every nonzero g^2 and v is in the fp32 normal range."""
    rng = np.random.default_rng(1000 + seed)
    p = rng.normal(0, 0.05, n).astype(np.float32)
    g = rng.normal(0, 0.05, n).astype(np.float32)
    m = rng.normal(0, 1e-3, n).astype(np.float32)
    v = rng.uniform(1e-8, 1e-5, n).astype(np.float32)
    i = np.arange(n)
    big = i % 97 == 5
    g[big] = (np.sign(g[big]) * 1e3 * (1 + np.abs(g[big]))).astype(np.float32)
    g[i % 7 == 3] = 0.0
    first = i % 11 == 4
    m[first] = 0.0
    v[first] = 0.0
    nz = g[g != 0]
    assert nz.size == 0 or float(np.abs(nz).min()) > 1e-18
    return p, m, v, g


def adamw_oracle(mode, p, m, v, g, step, hp, g_err=0.0):
    """One AdamW step in float64 (O.keras_adamw_step / O.torch_adamw_step) from the fp32 state (p, m, v, g)
    widened to float64, with hp = step_hp(...) and the bias corrections formed in float64 from those
    values (as make_adam_hp, csrc/optimizer.hip) -> ((p', m', v'), (bound p', bound m', bound v')).

    Bounds, per element, with u = 2^-24, C = 8 and the oracle's own intermediates (g_err: an absolute
    error already in the gradient the kernel uses, 0 for a stored gradient):
      err(m') = C u (|g| + |m|) + (1 - beta1) g_err
      err(v') = C u ((1 - beta2) g^2 + |v|) + (1 - beta2) (2 |g| g_err + g_err^2)
      err(p') = C u (|p| + |decay| + |update|) + gain err(m') + |update| err(v') / (2 v' + tiny)
    keras:  decay = p wd lr,  update = m' alpha / (sqrt(v') + eps),  gain = alpha / (sqrt(v') + eps),
            alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t)
    torch:  decay = p lr wd,  update = lr (m' / bc1) / (sqrt(v' / bc2) + eps),
            gain = (lr / bc1) / (sqrt(v' / bc2) + eps),  bc1 = 1 - beta1^t,  bc2 = 1 - beta2^t
    err(v') weighs g^2 by (1 - beta2), as both operation orders do before g^2 meets v (every rounding of
    v' is then at most u ((1 - beta2) g^2 + |v|), and there are at most four): C u (g^2 + |v|) would be a
    thousand times v' itself where v = 0, and would hide beta2 = 0.999 taken as a double (1 - beta2 off by
    1.3e-5 relative) in every element.
    The first term of each allows C roundings of the quantity's own operands (the compiler may contract
    multiply-adds; sqrtf and the fp32 division need not be correctly rounded; alpha, bc1 and bc2 reach the
    kernel rounded to fp32); the others carry the moments' errors through d update / d m' = gain and
    |d update / d v'| <= |update| / (2 v') (both modes: the eps in the denominator only lowers it)."""
    p, m, v, g = (np.asarray(x, np.float64) for x in (p, m, v, g))
    lr, wd, b1, b2, eps = hp["lr"], hp["wd"], hp["beta1"], hp["beta2"], hp["eps"]
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    if mode == "keras":
        p1, m1, v1 = O.keras_adamw_step(p, g, m, v, step, **hp)
        gain = (lr * np.sqrt(bc2) / bc1) / (np.sqrt(v1) + eps)
    else:
        p1, m1, v1 = O.torch_adamw_step(p, g, m, v, step, **hp)
        gain = (lr / bc1) / (np.sqrt(v1 / bc2) + eps)
    decay, upd = p * wd * lr, m1 * gain
    bm = STEP_C * U32 * (np.abs(g) + np.abs(m)) + (1 - b1) * g_err
    bv = STEP_C * U32 * ((1 - b2) * g * g + np.abs(v)) + (1 - b2) * (2 * np.abs(g) * g_err + g_err * g_err)
    bp = STEP_C * U32 * (np.abs(p) + np.abs(decay) + np.abs(upd)) + gain * bm + np.abs(upd) * bv / (2 * v1 + TINY)
    return (p1, m1, v1), (bp, bm, bv)


def step_ratios(got, ref, bounds):
    """max over elements of |got - ref| / bound for (p, m, v); a zero bound demands equality (ratio 0 or
    inf)."""
    out = []
    for a, r, b in zip(got, ref, bounds):
        e = np.abs(np.asarray(a, np.float64) - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(e == 0, 0.0, e / b)
        out.append(float(q.max()) if q.size else 0.0)
    return out
