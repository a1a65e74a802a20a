"""The plain-critic oracle of tests/test_critic_plain_cpu.py and tests/test_critic_plain_gpu.py.

The reference's CriticObs(residual_style=False) (model/common/critic.py:15-38) builds MLP([Do To, h, h, h, 1], Mish)
(model/common/mlp.py:35-92). In float64 with the oracle's rounding points:

    h1 = in(s);  u1 = mish(h1);  h2 = l1(u1);  u2 = mish(h2);  h3 = l2(u2);  u3 = mish(h3);  V = out(u3)

GEMM operands go through `rnd` (s, the weights, u1, u2, u3); the gradient images dV, dh3, dh2, dh1 through
`rnd.grad_round` (fp16: the row-tied scale); biases and accumulators are not rounded. The parameter dict is the
residual critic's (the four Dense layers have the same shapes in both forms).

The `plain_critic_oracle` fixture replaces O.critic_forward and O.residual_mlp_backward for the duration of a test.
O.c_loss calls the latter directly for the critic, and the actor's backward calls it too, so the replacement takes
the plain path only for a cache that plain_critic_forward produced (it carries `plain_critic`) and falls through to
the original otherwise. oracle/iteration.py then runs a plain critic unedited."""
import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests.helpers import HOPPER

PLAIN_CRITIC = dict(critic_head="plain")
HOPPER_PLAIN_CRITIC = dict(HOPPER, **PLAIN_CRITIC)


def plain_critic_forward(pc, state, act="Mish", rnd=None):
    """O.critic_forward's signature: (V [B, 1], cache)."""
    a, _ = O.ACT[act]
    R = rnd or O._ident
    B = state.shape[0]
    xr = R(state.reshape(B, -1).astype(np.float64))
    h1 = xr @ R(pc["in_w"]) + np.asarray(pc["in_b"], np.float64)
    u1 = R(a(h1))
    h2 = u1 @ R(pc["l1_w"]) + np.asarray(pc["l1_b"], np.float64)
    u2 = R(a(h2))
    h3 = u2 @ R(pc["l2_w"]) + np.asarray(pc["l2_b"], np.float64)
    u3 = R(a(h3))
    v = u3 @ R(pc["out_w"]) + np.asarray(pc["out_b"], np.float64)
    return v, dict(x=xr, h1=h1, u1=u1, h2=h2, u2=u2, h3=h3, u3=u3, R=R, plain_critic=True)


def plain_critic_backward(pc, cache, dy, act="Mish"):
    """(grads, dx) of a plain_critic_forward cache."""
    _, ag = O.ACT[act]
    R = cache.get("R", O._ident)
    Rg = getattr(R, "grad_round", R)
    g = {}
    dyr = Rg(dy)
    g["out_w"] = cache["u3"].T @ dyr
    g["out_b"] = dyr.sum(0)
    du3 = dyr @ R(pc["out_w"]).T
    dh3 = Rg(du3 * ag(cache["h3"]))
    g["l2_w"] = cache["u2"].T @ dh3
    g["l2_b"] = dh3.sum(0)
    du2 = dh3 @ R(pc["l2_w"]).T
    dh2 = Rg(du2 * ag(cache["h2"]))
    g["l1_w"] = cache["u1"].T @ dh2
    g["l1_b"] = dh2.sum(0)
    du1 = dh2 @ R(pc["l1_w"]).T
    dh1 = Rg(du1 * ag(cache["h1"]))
    g["in_w"] = cache["x"].T @ dh1
    g["in_b"] = dh1.sum(0)
    dx = dh1 @ np.asarray(pc["in_w"], np.float64).T
    return g, dx


@pytest.fixture
def plain_critic_oracle(monkeypatch):
    original = O.residual_mlp_backward

    def backward(p, cache, dy, act, prefix):
        if cache.get("plain_critic"):
            assert prefix == ""
            return plain_critic_backward(p, cache, dy, act)
        return original(p, cache, dy, act, prefix)

    monkeypatch.setattr(O, "critic_forward", plain_critic_forward)
    monkeypatch.setattr(O, "residual_mlp_backward", backward)
    return plain_critic_forward
