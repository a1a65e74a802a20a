"""The ELU / GELU / Softplus oracle of the actor tests (tests/test_actor_activations_cpu.py,
tests/test_actor_activations_gpu.py).

The oracle's ACT dict holds (f, f') pairs for ReLU and Mish; its composed functions (sample, get_logprobs,
c_loss, p_losses, bc_loss, oracle/iteration.py) call diffusion_mlp_forward / diffusion_mlp_backward through
the module's globals with act="ReLU" defaulted. For the duration of a test `act_oracle(name)` adds the float64
pair of `name` to O.ACT and wraps those two functions, as tests/mish_oracle.py does, so that every composed
function runs that activation; `act_oracle(name, head="plain")` wraps the plain head of tests/plain_oracle.py
instead. The oracle itself is not edited. The call's value records the cache of the last forward (h1, h2: the
pre-activations at the block's two sites).

The float64 definitions are Keras':
    ELU       keras.activations.elu, alpha = 1:          x > 0 ? x : expm1(x);        x > 0 ? 1 : exp(x)
    GELU      keras.activations.gelu, approximate=False: x Phi(x);                    Phi(x) + x phi(x)
    Softplus  tf.math.softplus:                          max(x, 0) + log1p(e^-|x|);   sigmoid(x)
Phi(x) = (1 + erf(x / sqrt 2)) / 2 is evaluated as erfc(-x / sqrt 2) / 2, the same function without the
cancellation of 1 + erf in the negative tail. No exponential takes a positive argument, so none overflows."""
import math

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import plain_oracle as PO
from tests.helpers import HOPPER, HOPPER_DDIM, WALKER
from tests.mish_oracle import BIAS_SCALE, mish_models, site_coverage  # noqa: F401  (re-exported)

try:
    from scipy.special import erfc as _erfc
except ImportError:   # math.erfc, element by element
    _erfc = np.vectorize(math.erfc, otypes=[np.float64])

NEW_ACTIVATIONS = ("ELU", "GELU", "Softplus")
ALL_ACTIVATIONS = ("ReLU", "Mish") + NEW_ACTIVATIONS
_SQRT2, _SQRT2PI = math.sqrt(2.0), math.sqrt(2.0 * math.pi)


def _f64(x):
    return np.asarray(x, np.float64)


def elu(x):
    x = _f64(x)
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))


def elu_grad(x):
    x = _f64(x)
    return np.where(x > 0, 1.0, np.exp(np.minimum(x, 0.0)))


def _Phi(x):
    return 0.5 * _erfc(-x / _SQRT2)


def gelu(x):
    x = _f64(x)
    return x * _Phi(x)


def gelu_grad(x):
    x = _f64(x)
    xc = np.clip(x, -40.0, 40.0)            # e^-800 is 0 in float64, and x^2 cannot overflow
    return _Phi(x) + x * np.exp(-0.5 * xc * xc) / _SQRT2PI


def softplus(x):
    x = _f64(x)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def softplus_grad(x):
    x = _f64(x)
    u = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0, u) / (1.0 + u)


F64 = {"ELU": (elu, elu_grad), "GELU": (gelu, gelu_grad), "Softplus": (softplus, softplus_grad)}


def dims_of(name, dims=HOPPER, **extra):
    """dims with the Python-only `activation` key (and any other, e.g. head="plain")."""
    return dict(dims, activation=name, **extra)


class _Last:
    cache = None
    name = None


@pytest.fixture
def act_oracle(monkeypatch):
    """act_oracle(name, head="residual") -> the record of the last forward's cache; name may also be "ReLU" or
    "Mish" (the oracle's own pairs), so one test can walk every supported activation."""
    fwd, bwd = O.diffusion_mlp_forward, O.diffusion_mlp_backward
    last = _Last()

    def use(name, head="residual"):
        assert name in ALL_ACTIVATIONS and head in ("residual", "plain"), (name, head)
        for k, pair in F64.items():
            monkeypatch.setitem(O.ACT, k, pair)
        f, b = (fwd, bwd) if head == "residual" else (PO.diffusion_plain_forward, PO.diffusion_plain_backward)

        def forward(p, x, t, state, act="ReLU", rnd=None, round_h3=True):
            y, cache = f(p, x, t, state, name, rnd, round_h3)
            last.cache = cache
            return y, cache

        def backward(p, cache, deps, xdim, act="ReLU"):
            return b(p, cache, deps, xdim, name)

        monkeypatch.setattr(O, "diffusion_mlp_forward", forward)
        monkeypatch.setattr(O, "diffusion_mlp_backward", backward)
        last.name = name
        return last

    return use


def sampler_self_noise(inputs, precision, seed, rel=2e-7):
    """The ORACLE's own sensitivity at its rounding points, no kernel involved: O.sample on `inputs` (a
    tests.test_sampler_surface_gpu._Inputs, under whatever activation the fixture installed) against O.sample with
    every operand scaled by 1 + rel N(0, 1) just before it is rounded, in the sampler statistics (SS._stats).
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


__all__ = ["ALL_ACTIVATIONS", "BIAS_SCALE", "F64", "HOPPER", "HOPPER_DDIM", "NEW_ACTIVATIONS", "WALKER", "act_oracle",
           "dims_of", "mish_models", "sampler_self_noise", "site_coverage"]
