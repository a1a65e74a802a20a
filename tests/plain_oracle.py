"""The plain-head oracle of the actor tests (tests/test_actor_plain_cpu.py, tests/test_actor_plain_gpu.py).

The reference's MLP([in, h, h, out]) (model/common/mlp.py:35-92, DiffusionMLP residual_style=False with the
default mlp_dims = [h, h]) in float64 with the oracle's rounding points:

    h1 = in(x);  u1 = act(h1);  h2 = l1(u1);  a = act(h2);  eps = W_out^T a + b_out

GEMM operands go through `rnd` (x, the weights, u1, and u2 = a, rounded as the l1 output is in the residual
oracle); biases and accumulators are not rounded; dx comes from the unrounded in_w (the kernels form d t_emb
from fp32 parameters). The parameter dict may carry l2_w / l2_b (tests.helpers.make_models does): a plain head
ignores them, and the backward returns no gradient for them (the GPU tests assert the flat l2 range is
exactly zero on its own).

The `plain_oracle` fixture wraps O.diffusion_mlp_forward / O.diffusion_mlp_backward for the duration of a
test, as tests/mish_oracle.py does, so that sample, get_logprobs, c_loss, p_losses, bc_loss and
oracle/iteration.py run a plain head; the oracle itself is not edited. The activation follows
`plain_oracle.act` ("ReLU" unless a test sets "Mish")."""
import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests.helpers import HOPPER, WALKER, make_models

PLAIN = dict(head="plain")
HOPPER_PLAIN = dict(HOPPER, **PLAIN)
WALKER_PLAIN = dict(WALKER, **PLAIN)
_PY_ONLY = ("activation", "head")


def plain_mlp_forward(p, x, act, rnd=None):
    a, _ = O.ACT[act]
    R = rnd or O._ident
    xr = R(x)
    h1 = xr @ R(p["in_w"]) + np.asarray(p["in_b"], np.float64)
    u1 = R(a(h1))
    h2 = u1 @ R(p["l1_w"]) + np.asarray(p["l1_b"], np.float64)
    u2 = R(a(h2))
    y = u2 @ R(p["out_w"]) + np.asarray(p["out_b"], np.float64)
    return y, dict(x=xr, h1=h1, u1=u1, h2=h2, u2=u2, R=R)


def plain_mlp_backward(p, cache, dy, act):
    """(grads, dx): the residual oracle's backward with the l2 layer and the skip removed."""
    _, ag = O.ACT[act]
    R = cache.get("R", O._ident)
    Rg = getattr(R, "grad_round", R)
    g = {}
    dyr = Rg(dy)
    g["out_w"] = cache["u2"].T @ dyr
    g["out_b"] = dyr.sum(0)
    du2 = dyr @ R(p["out_w"]).T
    dh2 = Rg(du2 * ag(cache["h2"]))
    g["l1_w"] = cache["u1"].T @ dh2
    g["l1_b"] = dh2.sum(0)
    du1 = dh2 @ R(p["l1_w"]).T
    dh1 = Rg(du1 * ag(cache["h1"]))
    g["in_w"] = cache["x"].T @ dh1
    g["in_b"] = dh1.sum(0)
    dx = dh1 @ np.asarray(p["in_w"], np.float64).T
    return g, dx


def diffusion_plain_forward(p, x, t, state, act="ReLU", rnd=None, round_h3=True):
    """O.diffusion_mlp_forward's signature; round_h3 has no meaning without h3."""
    B = x.shape[0]
    temb, tcache = O.time_mlp_forward(p, t, np.shape(p["time_w1"])[0])
    inp = np.concatenate([x.reshape(B, -1), temb, state.reshape(B, -1)], axis=-1).astype(np.float64)
    y, cache = plain_mlp_forward(p, inp, act, rnd)
    cache["time"] = tcache
    cache["t"] = np.asarray(t)
    return y.reshape(x.shape), cache


def diffusion_plain_backward(p, cache, deps, xdim, act="ReLU"):
    B = deps.shape[0]
    g, dinp = plain_mlp_backward(p, cache, deps.reshape(B, -1), act)
    tdim = p["time_w2"].shape[1]
    g.update(O.time_mlp_backward(p, cache["time"], dinp[:, xdim:xdim + tdim]))
    return g


class _Last:
    cache = None
    act = "ReLU"


@pytest.fixture
def plain_oracle(monkeypatch):
    last = _Last()

    def forward(p, x, t, state, act="ReLU", rnd=None, round_h3=True):
        y, cache = diffusion_plain_forward(p, x, t, state, last.act, rnd, round_h3)
        last.cache = cache
        return y, cache

    def backward(p, cache, deps, xdim, act="ReLU"):
        return diffusion_plain_backward(p, cache, deps, xdim, last.act)

    monkeypatch.setattr(O, "diffusion_mlp_forward", forward)
    monkeypatch.setattr(O, "diffusion_mlp_backward", backward)
    return last


def plain_models(seed=0, dims=HOPPER, bias_scale=0.05, ft_perturb=0.02):
    """tests.helpers.make_models for dims that may carry the Python-only `head` / `activation` keys."""
    return make_models(seed, {k: v for k, v in dims.items() if k not in _PY_ONLY}, bias_scale=bias_scale,
                       ft_perturb=ft_perturb)
