"""The Mish oracle of the actor tests (tests/test_actor_mish_cpu.py, tests/test_actor_mish_gpu.py).

The oracle's composed functions (sample, get_logprobs, c_loss, p_losses, bc_loss, oracle/iteration.py)
call diffusion_mlp_forward / diffusion_mlp_backward through the module's globals with act="ReLU"
defaulted. The `mish_oracle` fixture wraps those two for the duration of a test so that every composed
function runs a Mish actor; the oracle itself is not edited. The fixture's value records the cache of
the last forward (h1, h2: the pre-activations at the block's two sites)."""
import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests.helpers import HOPPER, WALKER, make_models

MISH = dict(activation="Mish")
HOPPER_MISH = dict(HOPPER, **MISH)
WALKER_MISH = dict(WALKER, **MISH)
# N(0, BIAS_SCALE) biases put h1 and h2 on both sides of zero and past x < -1, where mish' < 0
# (site_coverage asserts it on the oracle's cache; make_models' default 0.05 leaves h within +-1)
BIAS_SCALE = 1.0


class _Last:
    cache = None


@pytest.fixture
def mish_oracle(monkeypatch):
    fwd, bwd = O.diffusion_mlp_forward, O.diffusion_mlp_backward
    last = _Last()

    def forward(p, x, t, state, act="ReLU", rnd=None, round_h3=True):
        y, cache = fwd(p, x, t, state, "Mish", rnd, round_h3)
        last.cache = cache
        return y, cache

    def backward(p, cache, deps, xdim, act="ReLU"):
        return bwd(p, cache, deps, xdim, "Mish")

    monkeypatch.setattr(O, "diffusion_mlp_forward", forward)
    monkeypatch.setattr(O, "diffusion_mlp_backward", backward)
    return last


def mish_models(seed=0, dims=HOPPER, bias_scale=BIAS_SCALE, ft_perturb=0.02):
    """tests.helpers.make_models with the Mish tests' bias scale (dims may carry `activation`)."""
    return make_models(seed, {k: v for k, v in dims.items() if k != "activation"}, bias_scale=bias_scale,
                       ft_perturb=ft_perturb)


def site_coverage(cache):
    """Fractions of h1 / h2 below -1 and above 0, asserted: >= 5 % and >= 20 % at both sites."""
    out = {}
    for k in ("h1", "h2"):
        h = np.asarray(cache[k])
        out[k] = (float((h < -1).mean()), float((h > 0).mean()))
        assert out[k][0] >= 0.05 and out[k][1] >= 0.20, (k, out[k])
    return out
