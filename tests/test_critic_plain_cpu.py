"""Plain critic (CriticObs residual_style=False, mlp_dims [256, 256, 256]), the CPU half: the oracle's plain critic
(O.Model(critic_head="plain")) is right (finite differences) and moves V and every critic gradient tensor the GPU
file compares by at least ten times that quantity's bound; the Python containers accept exactly the supported
shape; the C ABI carries the new symbol within ABI 15; checkpoints round-trip and do not cross heads; the two new
cfgs load and resolve."""
import json
import os
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import test_update_surface_gpu as US
from tests.helpers import HOPPER, make_models, to_f64
from tests.variants import HOPPER_PLAIN_CRITIC

PLAIN_CRITIC = O.Model(critic_head="plain")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "cfg/gym/finetune/hopper-v2")


# ------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------
def test_plain_critic_backward_matches_finite_differences():
    """Every gradient tensor of L = sum(w * V) against central differences in float64 on a 3-input, 8-wide net,
    5 rows. Relative 1e-6 of the tensor's largest entry: float64 noise of a step-1e-6 central difference, not a
    measured quantity."""
    rng = np.random.default_rng(5)
    sd, h, B = 3, 8, 5
    p = {"in_w": rng.normal(0, .6, (sd, h)), "in_b": rng.normal(0, .5, h), "l1_w": rng.normal(0, .6, (h, h)),
         "l1_b": rng.normal(0, .5, h), "l2_w": rng.normal(0, .6, (h, h)), "l2_b": rng.normal(0, .5, h),
         "out_w": rng.normal(0, .6, (h, 1)), "out_b": rng.normal(0, .3, 1)}
    state, w = rng.normal(0, 1, (B, 1, sd)), rng.normal(0, 1, (B, 1))
    loss = lambda q: float((O.critic_forward(q, state, PLAIN_CRITIC)[0] * w).sum())
    _, cache = O.critic_forward(p, state, PLAIN_CRITIC)
    g, _ = O.critic_backward(p, cache, w, PLAIN_CRITIC)
    assert set(g) == set(p)
    errs = {}
    for k, v in p.items():
        num = np.zeros_like(v)
        for i in np.ndindex(v.shape):
            hi, lo = {**p, k: v.copy()}, {**p, k: v.copy()}
            hi[k][i] += 1e-6
            lo[k][i] -= 1e-6
            num[i] = (loss(hi) - loss(lo)) / 2e-6
        errs[k] = float(np.abs(num - g[k]).max() / np.abs(num).max())
    print(json.dumps({"case": "plain-critic-fd", "errs": errs}))
    assert all(e < 1e-6 for e in errs.values()), errs


def test_critic_backward_follows_the_model():
    """O.critic_backward takes the head from the model it is given: the residual critic's is O.residual_mlp_backward
    (which the actor's backward calls too), the plain critic's is O.plain_critic_backward."""
    rng = np.random.default_rng(3)
    _, _, critic = make_models(0, HOPPER)
    pc = to_f64(critic)
    state, dy = rng.uniform(-1, 1, (6, 1, 11)), rng.normal(0, 1, (6, 1))
    _, rcache = O.residual_mlp_forward(pc, state.reshape(6, -1), "Mish", "")
    g_res, _ = O.residual_mlp_backward(pc, rcache, dy, "Mish", "")
    assert np.array_equal(g_res["l2_w"], (rcache["u2"].T @ dy) @ pc["out_w"].T)      # the factored residual form
    g_dflt, _ = O.critic_backward(pc, O.critic_forward(pc, state)[1], dy)
    assert all(np.array_equal(g_dflt[k], g_res[k]) for k in g_res)
    _, pcache = O.critic_forward(pc, state, PLAIN_CRITIC)
    g_pl, _ = O.critic_backward(pc, pcache, dy, PLAIN_CRITIC)
    ref, _ = O.plain_critic_backward(pc, pcache, dy)
    assert all(np.array_equal(g_pl[k], ref[k]) for k in ref)
    assert not np.array_equal(g_pl["l2_w"], g_res["l2_w"])


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_plain_critic_oracle_moves_values_and_gradients(precision):
    """On the GPU tests' inputs (test_critic_forward's 77 states, the 150-row minibatch problem of
    tests/test_update_surface_gpu.py, whose samples and weights the GPU file's cases share) the plain and the
    residual oracle differ in V and in every critic gradient tensor by at least ten times that quantity's bound, so
    a GPU run on the wrong head cannot pass."""
    rnd = US._rnd(precision)
    _, _, critic = make_models(0, HOPPER)
    state = np.random.default_rng(5).uniform(-1, 1, (77, 1, 11)).astype(np.float32).astype(np.float64)
    p = US._Problem(HOPPER_PLAIN_CRITIC, precision)
    v_p = O.critic_forward(to_f64(critic), state, PLAIN_CRITIC, rnd=rnd)[0]
    met_p, ga_p, gc_p = p.oracle()
    v_r = O.critic_forward(to_f64(critic), state, rnd=rnd)[0]
    met_r, ga_r, gc_r = p.oracle(model=O.Model())
    tol_v = {"fp32": 1e-4, "bf16": 1e-3, "fp16": 1e-3}[precision]
    dv = float(np.abs(v_p - v_r).max())
    moved = {k: US._rel(gc_p[k], gc_r[k]) for k in gc_r}
    print(json.dumps({"case": f"plain-vs-residual-critic-{precision}", "dV": dv, "grads": moved,
                      "v_loss": [met_p["v_loss"], met_r["v_loss"]]}))
    assert set(gc_p) == set(gc_r) == {"in_w", "in_b", "l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"}
    assert dv >= 10 * tol_v * (1 + np.abs(v_r).max())
    assert all(v >= 10 * US.TOL[precision] for v in moved.values()), moved
    # (v_loss itself is printed, not asserted: against N(0, 1) returns it is dominated by the returns' own square)
    for k in ga_r:   # the actor's side of c_loss does not depend on the critic's head
        assert np.array_equal(ga_p[k], ga_r[k]), k


# ------------------------------------------------------------------------------------------------
# the Python containers
# ------------------------------------------------------------------------------------------------
def test_critic_obs_accepts_three_equal_hidden_layers():
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.model.common.critic import CriticObs
    from diffusionpolicyoptimization_amd.model.common.mlp import MLP
    c = CriticObs(cond_dim=11, mlp_dims=[256] * 3, residual_style=False)
    assert (c.head, c.hidden, type(c.net)) == ("plain", 256, MLP)
    assert CriticObs(cond_dim=11, mlp_dims=[256] * 3).head == "plain"                  # the class default
    assert CriticObs(cond_dim=11, mlp_dims=[256] * 3, residual_style=True).head == "residual"
    p = c.init_params(np.random.default_rng(0))
    spec = ops.critic_param_spec(ops.ModelDims(**HOPPER_PLAIN_CRITIC))
    assert list(p) == [n for n, _ in spec] and all(p[n].shape == tuple(s) for n, s in spec)
    for dims in ([256, 256], [256] * 4, [256, 128, 256], [256], [512] * 3):
        with pytest.raises(NotImplementedError, match=re.escape("mlp_dims = [256, 256, 256]")):
            CriticObs(cond_dim=11, mlp_dims=dims, residual_style=False)
    with pytest.raises(NotImplementedError, match=re.escape("mlp_dims = [256, 256, 256]")):
        CriticObs(cond_dim=11, mlp_dims=[256] * 3, residual_style=False, use_layernorm=True)
    with pytest.raises(NotImplementedError, match="Mish"):
        CriticObs(cond_dim=11, mlp_dims=[256] * 3, residual_style=False, activation_type="ReLU")
    # MLP itself: four layers only at out width 1 with Mish; the actor's shape check is what it was
    assert MLP([11, 256, 256, 256, 1], activation_type="Mish").hidden == 256
    for dims, act in (([11, 256, 256, 256, 1], "ReLU"), ([11, 256, 256, 256, 2], "Mish"), ([11, 256, 128, 256, 1], "Mish"),
                      ([11, 256, 256, 256, 256, 1], "Mish")):
        with pytest.raises(NotImplementedError, match=re.escape("[in, h, h, out]")):
            MLP(dims, activation_type=act)
    assert "l2_w" not in MLP([39, 512, 512, 12], activation_type="ReLU").init_params(np.random.default_rng(0))


def test_model_dims_critic_head():
    from diffusionpolicyoptimization_amd import ops
    d = ops.ModelDims(**HOPPER_PLAIN_CRITIC)
    assert d.critic_head == "plain" and d.head == "residual" and ops.ModelDims(**HOPPER).critic_head == "residual"
    assert bytes(d.c()) == bytes(ops.ModelDims(**HOPPER).c())                # Python-only: dppo_dims keeps its layout
    assert ops.critic_param_spec(d) == ops.critic_param_spec(ops.ModelDims(**HOPPER))
    with pytest.raises(ValueError, match="critic_head"):
        ops.ModelDims(critic_head="x")


def test_abi_carries_the_critic_head():
    """The new symbol is declared, bound and exported within ABI 15; the header describes the plain form."""
    from diffusionpolicyoptimization_amd import _lib
    src = open(os.path.join(ROOT, "include", "dppo.h")).read()
    declared = set(re.findall(r"DPPO_API\s+[\w\s\*]+?\b(dppo_\w+)\s*\(", src))
    assert "dppo_pack_critic_head" in declared and "dppo_pack_critic_head" in _lib.EXPORTED_SYMBOLS
    assert re.search(r"#define DPPO_ABI_VERSION 15\b", src)
    lib = _lib.load()
    assert lib.dppo_abi_version() == 15 and hasattr(lib, "dppo_pack_critic_head")
    assert "The critic has no plain" not in src and "u3 = mish(h3); V = out(u3)" in src
    # the table's eraser: host-only, so it runs without a device; any address, NULL included
    import ctypes
    assert "dppo_forget_image" in declared and "dppo_forget_image" in _lib.EXPORTED_SYMBOLS
    assert lib.dppo_forget_image(ctypes.c_void_p(0x1000)) == 0 and lib.dppo_forget_image(None) == 0


# ------------------------------------------------------------------------------------------------
# checkpoints
# ------------------------------------------------------------------------------------------------
def test_keras_weights_round_trip_and_cross_head_errors(tmp_path):
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util import keras_weights as KW
    from diffusionpolicyoptimization_amd.util.h5 import read_h5
    d = ops.ModelDims(**HOPPER_PLAIN_CRITIC)
    sa, sc = ops.actor_param_spec(d), ops.critic_param_spec(d)
    rng = np.random.default_rng(1)
    mk = lambda spec: {n: rng.normal(size=s).astype(np.float32) for n, s in spec}
    actor, critic = mk(sa), mk(sc)
    pl, rs = str(tmp_path / "plain.weights.h5"), str(tmp_path / "resid.weights.h5")
    KW.save_ppo_model(pl, actor, mk(sa), critic, critic_plain=True)
    KW.save_ppo_model(rs, actor, mk(sa), critic)
    names = [k for k in read_h5(pl) if k != "__groups__"]
    crit = sorted(k for k in names if k.startswith("critic/"))
    seq = lambda i: f"critic/Q1/module_list/sequential{'_%d' % i if i else ''}/layers/dense/vars/"
    assert crit == sorted(seq(i) + v for i in range(4) for v in "01")
    assert any("critic/Q1/residual_blocks" in k for k in read_h5(rs))
    w = KW.load_ppo_model(pl, sa, sc, critic_plain=True)
    assert set(w["critic"]) == set(critic) and all(np.array_equal(w["critic"][k], critic[k]) for k in critic)
    assert all(np.array_equal(w["actor"][k], actor[k]) for k in actor)
    with pytest.raises(ValueError, match="holds a residual .* critic, the model is plain"):
        KW.load_ppo_model(rs, sa, sc, critic_plain=True)
    with pytest.raises(ValueError, match="holds a plain .* critic, the model is residual"):
        KW.load_ppo_model(pl, sa, sc)
    w = KW.load_ppo_model(rs, sa, sc)
    assert all(np.array_equal(w["critic"][k], critic[k]) for k in critic)


def test_npz_cross_head_check():
    """The .npz rule: both heads hold the same tensors, so a plain critic's file carries critic.head."""
    from diffusionpolicyoptimization_amd import ops
    names = ["critic." + n for n, _ in ops.critic_param_spec(ops.ModelDims(**HOPPER))]
    ops.check_checkpoint_critic_head(names, "residual", "r.npz")
    ops.check_checkpoint_critic_head(names + [ops.CRITIC_HEAD_KEY], "plain", "p.npz", np.array("plain"))
    ops.check_checkpoint_critic_head(["actor.in_w"], "plain", "a.npz")          # no critic in the file
    with pytest.raises(ValueError, match="holds a residual critic, the model is plain"):
        ops.check_checkpoint_critic_head(names, "plain", "r.npz")
    with pytest.raises(ValueError, match="holds a plain critic, the model is residual"):
        ops.check_checkpoint_critic_head(names + [ops.CRITIC_HEAD_KEY], "residual", "p.npz", np.array("plain"))


# ------------------------------------------------------------------------------------------------
# cfgs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,actor_head", [("ft_ppo_diffusion_mlp_plain_critic", "residual"),
                                             ("ft_ppo_diffusion_mlp_plain_both", "plain")])
def test_new_cfgs_load_and_resolve(name, actor_head):
    from diffusionpolicyoptimization_amd.util.config import instantiate, load_config
    cfg = load_config(CFG_DIR, name, [])
    base = load_config(CFG_DIR, "ft_ppo_diffusion_mlp", [])
    assert cfg.model.critic.residual_style is False and list(cfg.model.critic.mlp_dims) == [256, 256, 256]
    assert cfg.model.critic.cond_dim == 11 and cfg.model.critic.activation_type == "Mish"
    critic, actor = instantiate(cfg.model.critic), instantiate(cfg.model.actor)
    assert (critic.head, critic.hidden, actor.head) == ("plain", 256, actor_head)
    assert list(cfg.model.actor.mlp_dims) == ([512, 512] if actor_head == "plain" else [512, 512, 512])
    assert dict(cfg.train) == dict(base.train) and cfg.env_name == base.env_name
