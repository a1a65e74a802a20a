"""The layer-normed critic oracle of tests/test_critic_layernorm_cpu.py and tests/test_critic_layernorm_gpu.py.

The reference's CriticObs(use_layernorm=True) (model/common/critic.py:15-38) builds, in float64 with the oracle's
rounding points:

    plain     MLP([Do To, h, h, h, 1], Mish) (model/common/mlp.py:62-78): per hidden layer Dense ->
              LayerNormalization() -> Mish, Keras' default epsilon 1e-3, no norm on the output layer:
                  y_k = LN_k(h_k), u_k = mish(y_k), k = 1..3;  V = out(u3)
    residual  ResidualMLP (mlp.py:163-206): the block's pre-activation norms, epsilon 1e-6, the skip un-normalised:
                  h1 = in(s); u1 = mish(LN_1(h1)); h2 = l1(u1); u2 = mish(LN_2(h2)); h3 = l2(u2) + h1; V = out(h3)

LayerNormalization is Keras': over the last axis, population variance, y = gamma (h - mean) / sqrt(var + eps) + beta.
GEMM operands go through `rnd` (s, the weights, u_k, the residual h3); the gradient images dV, dh_k through
`rnd.grad_round`; biases, accumulators, the norm's statistics, y_k, dy_k, dgamma and dbeta are not rounded. The
parameter dict is the critic's eight tensors plus ln{k}_g / ln{k}_b (ops.critic_param_spec).

The `layernorm_critic_oracle` fixture replaces O.critic_forward and O.residual_mlp_backward for the duration of a
test, like tests/plain_critic_oracle.py: the replacement backward takes the layer-norm path only for a cache that
ln_critic_forward produced and falls through to the original otherwise. The head is told by the parameters: a
critic with ln3_g is the plain head."""
import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests.helpers import HOPPER

EPS = {"plain": 1e-3, "residual": 1e-6}
HOPPER_LN = {"residual": dict(HOPPER, critic_layernorm=True),
             "plain": dict(HOPPER, critic_head="plain", critic_layernorm=True)}


def head_of(pc):
    return "plain" if "ln3_g" in pc else "residual"


def add_ln_params(critic, head, rng, scale=1.0):
    """The critic's eight tensors plus random norms: gamma ~ U(0.5, 1.5), beta ~ N(0, scale) (not 1 and 0)."""
    h = critic["in_b"].shape[0]
    out = dict(critic)
    for k in range(1, (3 if head == "plain" else 2) + 1):
        out[f"ln{k}_g"] = rng.uniform(0.5, 1.5, h).astype(np.float32)
        out[f"ln{k}_b"] = rng.normal(0, scale, h).astype(np.float32)
    return out


def layer_norm(h, gamma, beta, eps):
    mean = h.mean(-1, keepdims=True)
    var = ((h - mean) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (h - mean) * rstd
    return np.asarray(gamma, np.float64) * xh + np.asarray(beta, np.float64), xh, rstd, var


def layer_norm_backward(dy, xh, rstd, gamma):
    """(dh, dgamma, dbeta) of y = gamma x_hat + beta."""
    g = dy * np.asarray(gamma, np.float64)
    dh = rstd * (g - g.mean(-1, keepdims=True) - xh * (g * xh).mean(-1, keepdims=True))
    return dh, (dy * xh).sum(0), dy.sum(0)


def ln_critic_forward(pc, state, act="Mish", rnd=None, eps=None):
    """O.critic_forward's signature: (V [B, 1], cache). eps: the norm's epsilon (default: the head's)."""
    a, _ = O.ACT[act]
    R = rnd or O._ident
    head = head_of(pc)
    eps = EPS[head] if eps is None else eps
    B = state.shape[0]
    c = dict(R=R, ln_critic=head, var=[])
    c["x"] = R(state.reshape(B, -1).astype(np.float64))
    prev, names = c["x"], ("in", "l1", "l2")
    for k in range(1, (3 if head == "plain" else 2) + 1):
        h = prev @ R(pc[names[k - 1] + "_w"]) + np.asarray(pc[names[k - 1] + "_b"], np.float64)
        y, xh, rstd, var = layer_norm(h, pc[f"ln{k}_g"], pc[f"ln{k}_b"], eps)
        prev = R(a(y))
        c.update({f"h{k}": h, f"y{k}": y, f"xh{k}": xh, f"rstd{k}": rstd, f"u{k}": prev})
        c["var"].append(var)
    if head == "residual":
        h3 = prev @ R(pc["l2_w"]) + np.asarray(pc["l2_b"], np.float64) + c["h1"]
        prev = c["h3"] = R(h3)
    v = prev @ R(pc["out_w"]) + np.asarray(pc["out_b"], np.float64)
    return v, c


def ln_critic_backward(pc, cache, dy, act="Mish"):
    """(grads, dx) of an ln_critic_forward cache."""
    _, ag = O.ACT[act]
    R = cache.get("R", O._ident)
    Rg = getattr(R, "grad_round", R)
    head = cache["ln_critic"]
    g = {}
    dyr = Rg(dy)
    wo = R(pc["out_w"])
    g["out_w"] = (cache["u3"] if head == "plain" else cache["h3"]).T @ dyr
    g["out_b"] = dyr.sum(0)
    dlast = dyr @ wo.T                                     # plain: du3; residual: dh3

    def site(k, du):
        dh, g[f"ln{k}_g"], g[f"ln{k}_b"] = layer_norm_backward(du * ag(cache[f"y{k}"]), cache[f"xh{k}"], cache[f"rstd{k}"],
                                                               pc[f"ln{k}_g"])
        return dh

    if head == "plain":
        dh3 = Rg(site(3, dlast))
        g["l2_w"] = cache["u2"].T @ dh3
        g["l2_b"] = dh3.sum(0)
        skip = 0.0
    else:
        dh3 = Rg(dlast)
        g["l2_w"] = (cache["u2"].T @ dyr) @ wo.T            # the factored form (oracle/dppo_oracle.py residual_mlp_backward)
        g["l2_b"] = g["out_b"] @ wo.T
        skip = dh3
    dh2 = Rg(site(2, dh3 @ R(pc["l2_w"]).T))
    g["l1_w"] = cache["u1"].T @ dh2
    g["l1_b"] = dh2.sum(0)
    dh1 = Rg(skip + site(1, dh2 @ R(pc["l1_w"]).T))
    g["in_w"] = cache["x"].T @ dh1
    g["in_b"] = dh1.sum(0)
    return g, dh1 @ np.asarray(pc["in_w"], np.float64).T


@pytest.fixture
def layernorm_critic_oracle(monkeypatch):
    original = O.residual_mlp_backward

    def backward(p, cache, dy, act, prefix):
        if cache.get("ln_critic"):
            assert prefix == ""
            return ln_critic_backward(p, cache, dy, act)
        return original(p, cache, dy, act, prefix)

    monkeypatch.setattr(O, "critic_forward", ln_critic_forward)
    monkeypatch.setattr(O, "residual_mlp_backward", backward)
    return ln_critic_forward
