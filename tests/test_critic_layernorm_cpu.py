"""Layer-normed critic (CriticObs use_layernorm=True, both heads), the CPU half: the oracle's layer-normed critic
(O.Model(critic_layernorm=True)) is right (finite differences, gamma / beta included); turning the norm on, or
using the other head's epsilon, moves what the GPU file compares by at least ten times its bound; the Python
containers carry the tail without moving an existing offset; the C ABI carries the new symbols within ABI 15;
checkpoints round-trip and do not cross layouts; the two new cfgs load and resolve.

The GPU file's bounds are those of tests/test_critic_plain_gpu.py (V: 1e-4 / 1e-3 / 1e-3 of 1 + max|V|; gradients per
tensor: 2e-3 fp32, 1e-2 2-byte). The arithmetic they are held against, which O.ln_critic_forward / _backward state
with `rnd` at the kernel's rounding points: the row statistics (mean, then the mean of squared deviations) and
x_hat, y = gamma x_hat + beta, dy, dgamma, dbeta in the accumulators' precision, never rounded; only u_k = mish(y_k)
and the gradient images dh_k are rounded to the 2-byte type, as the operands of the next product."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import test_update_surface_gpu as US
from tests.helpers import HOPPER, make_models, to_f64
from tests.variants import HOPPER_LN, add_ln_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "cfg/gym/finetune/hopper-v2")
HEADS = ["residual", "plain"]
V_TOL = {"fp32": 1e-4, "bf16": 1e-3, "fp16": 1e-3}
EIGHT = ["in_w", "in_b", "l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b"]


def ln_models(seed=0, dims=HOPPER, in_scale=3.0, **kw):
    """tests.helpers.make_models with the critic the layer-norm tests use: for dims with critic_layernorm, W_in
    times in_scale (hidden rows of variance >= 100 epsilon at the first site too, asserted where used) and random
    norms, gamma ~ U(0.5, 1.5), beta ~ N(0, 1). The GPU file patches this in for the shared case classes."""
    base, ft, critic = make_models(seed, dims, **kw)
    if dims.get("critic_layernorm"):
        critic = dict(critic, in_w=(critic["in_w"] * np.float32(in_scale)).astype(np.float32))
        critic = add_ln_params(critic, dims.get("critic_head", "residual"), np.random.default_rng(77 + seed))
    return base, ft, critic


def near_eps_critic(head):
    """The wrong-epsilon case's critic: zero in-bias and W_in scaled so that the first site's hidden rows have a
    variance near 1e-3, where epsilon 1e-3 against 1e-6 changes rstd by about sqrt(2)."""
    _, _, critic = ln_models(0, HOPPER_LN[head], in_scale=0.2)
    return dict(critic, in_b=np.zeros_like(critic["in_b"]))


def states77():
    return np.random.default_rng(5).uniform(-1, 1, (77, 1, 11)).astype(np.float32).astype(np.float64)


def assert_variance(cache, head, factor=100.0):
    worst = min(float(v.min()) for v in cache["var"])
    assert worst >= factor * O.LN_EPS[head], (head, worst)
    return worst


# ------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS)
def test_ln_critic_backward_matches_finite_differences(head):
    """Every gradient tensor of L = sum(w * V), gamma and beta included, against central differences in float64 on
    a 3-input, 8-wide net, 5 rows. Relative 1e-6 of the tensor's largest entry: float64 noise of a step-1e-6 central
    difference, not a measured quantity."""
    rng = np.random.default_rng(5)
    sd, h, B = 3, 8, 5
    p = {"in_w": rng.normal(0, .6, (sd, h)), "in_b": rng.normal(0, .5, h), "l1_w": rng.normal(0, .6, (h, h)),
         "l1_b": rng.normal(0, .5, h), "l2_w": rng.normal(0, .6, (h, h)), "l2_b": rng.normal(0, .5, h),
         "out_w": rng.normal(0, .6, (h, 1)), "out_b": rng.normal(0, .3, 1)}
    for k in range(1, (3 if head == "plain" else 2) + 1):
        p[f"ln{k}_g"], p[f"ln{k}_b"] = rng.uniform(0.5, 1.5, h), rng.normal(0, 1, h)
    state, w = rng.normal(0, 1, (B, 1, sd)), rng.normal(0, 1, (B, 1))
    model = O.Model(critic_head=head, critic_layernorm=True)
    loss = lambda q: float((O.critic_forward(q, state, model)[0] * w).sum())
    _, cache = O.critic_forward(p, state, model)
    assert ("u3" in cache) == (head == "plain")          # a third normed site only under the plain head
    g, _ = O.critic_backward(p, cache, w, model)
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
    print(json.dumps({"case": f"ln-critic-fd-{head}", "errs": errs}))
    assert all(e < 1e-6 for e in errs.values()), errs


def test_layer_norm_is_keras():
    """Population variance over the last axis, epsilon inside the square root; gamma = 1, beta = 0 gives rows of mean
    0 and variance var / (var + eps)."""
    h = np.random.default_rng(0).normal(2.0, 3.0, (4, 16))
    y, xh, rstd, var = O.layer_norm(h, np.ones(16), np.zeros(16), 1e-3)
    assert np.allclose(var[:, 0], h.var(-1)) and np.allclose(y.mean(-1), 0, atol=1e-12)
    assert np.allclose(y.var(-1), h.var(-1) / (h.var(-1) + 1e-3))


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_layer_norm_moves_values_and_gradients(monkeypatch, precision, head):
    """On the GPU tests' inputs (77 states; the 150-row minibatch problem of tests/test_update_surface_gpu.py with
    ln_models' critic) the layer-normed oracle and the oracle of the same eight tensors without the norm differ in V
    and in every critic gradient tensor by at least ten times that quantity's bound, so a GPU run that skips the
    norm cannot pass. The hidden rows of both inputs have a variance of at least 100 epsilon at every site."""
    monkeypatch.setattr(US, "make_models", ln_models)
    rnd = US._rnd(precision)
    p = US._Problem(HOPPER_LN[head], precision)
    critic = to_f64(p.critic)
    v_ln, cache = O.critic_forward(critic, states77(), p.model, rnd=rnd)
    worst = assert_variance(cache, head)
    assert_variance(O.critic_forward(critic, p.state(p.obs[p.bi]), p.model, rnd=rnd)[1], head)
    _, _, gc_ln = p.oracle()
    off = O.Model(critic_head=head)                  # the same head without the norm
    eight = {k: critic[k] for k in EIGHT}
    v_off = O.critic_forward(eight, states77(), off, rnd=rnd)[0]
    p.critic = eight
    _, _, gc_off = p.oracle(model=off)
    dv = float(np.abs(v_ln - v_off).max())
    moved = {k: US._rel(gc_ln[k], gc_off[k]) for k in EIGHT}
    print(json.dumps({"case": f"ln-on-vs-off-{head}-{precision}", "dV": dv, "grads": moved, "min_var": worst}))
    assert set(gc_ln) == set(EIGHT) | {k for k in critic if k.startswith("ln")}
    assert dv >= 10 * V_TOL[precision] * (1 + np.abs(v_ln).max())
    assert all(v >= 10 * US.TOL[precision] for v in moved.values()), moved


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_wrong_epsilon_moves_the_values(precision, head):
    """near_eps_critic on the 77 states: the first site's hidden rows have a variance within [0.2, 5] x 1e-3
    (asserted), and V under the other head's epsilon is at least ten bounds away, so a tile that norms with the wrong
    head's epsilon cannot pass the GPU file's forward case on these inputs."""
    rnd = US._rnd(precision)
    critic = to_f64(near_eps_critic(head))
    model = O.Model(critic_head=head, critic_layernorm=True)
    v, cache = O.critic_forward(critic, states77(), model, rnd=rnd)
    var1 = cache["var"][0]
    assert 0.2e-3 <= float(var1.min()) and float(var1.max()) <= 5e-3, (float(var1.min()), float(var1.max()))
    other = O.LN_EPS["residual" if head == "plain" else "plain"]
    v_wrong, _ = O.critic_forward(critic, states77(), model, rnd=rnd, ln_eps=other)
    dv = float(np.abs(v - v_wrong).max() / (1 + np.abs(v).max()))
    print(json.dumps({"case": f"ln-wrong-eps-{head}-{precision}", "dV": dv, "bound": V_TOL[precision]}))
    assert dv >= 10 * V_TOL[precision]


# ------------------------------------------------------------------------------------------------
# the Python containers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS)
def test_spec_offsets_counts_and_flatten(head):
    from diffusionpolicyoptimization_amd import ops
    d, off = ops.ModelDims(**HOPPER_LN[head]), ops.ModelDims(**dict(HOPPER, critic_head=head))
    assert d.critic_layernorm is True and off.critic_layernorm is False
    assert bytes(d.c()) == bytes(off.c())                                    # Python-only: dppo_dims keeps its layout
    spec, spec_off = ops.critic_param_spec(d), ops.critic_param_spec(off)
    sites = 3 if head == "plain" else 2
    assert ops.critic_ln_sites(d) == sites and ops.critic_ln_sites(off) == 0
    assert spec[:8] == spec_off and [n for n, _ in spec_off] == EIGHT
    assert [n for n, _ in spec[8:]] == [f"ln{k}_{t}" for k in range(1, sites + 1) for t in "gb"]
    assert all(s == (256,) for _, s in spec[8:])
    r, r_off = list(ops.spec_ranges(spec)), list(ops.spec_ranges(spec_off))
    assert r[:8] == r_off                                                    # every existing offset keeps its value
    assert ops.spec_count(spec) == ops.spec_count(spec_off) + 2 * sites * 256
    assert ops.actor_param_spec(d) == ops.actor_param_spec(off)
    rng = np.random.default_rng(0)
    params = {n: rng.normal(size=s).astype(np.float32) for n, s in spec}
    flat = ops.flatten_params(spec, params)
    back = ops.unflatten_params(spec, flat)
    assert all(np.array_equal(back[n], params[n]) for n in params)
    assert np.array_equal(flat[:ops.spec_count(spec_off)], ops.flatten_params(spec_off, params))
    with pytest.raises(ValueError, match="critic_layernorm"):
        ops.ModelDims(critic_layernorm=1)


def test_containers_accept_layer_norm_for_the_two_shapes():
    """The critic classes take use_layernorm at the two shapes and create gamma ones, beta zeros under the spec's
    names: CriticObs for the residual head, CriticObsPlainLN for the plain one (CriticObs itself keeps refusing
    (residual_style=False, use_layernorm=True): tests/test_critic_plain_cpu.py pins that refusal, and the message
    names the class)."""
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.model.common.critic import CriticObs, CriticObsPlainLN
    from diffusionpolicyoptimization_amd.model.common.mlp import MLP, ResidualMLP
    from diffusionpolicyoptimization_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    c = CriticObs(cond_dim=11, mlp_dims=[256] * 3, residual_style=True, use_layernorm=True)
    assert (c.head, c.use_layernorm, c.hidden, type(c.net)) == ("residual", True, 256, ResidualMLP)
    q = CriticObsPlainLN(cond_dim=11, mlp_dims=[256] * 3, residual_style=False, use_layernorm=True)
    assert (q.head, q.use_layernorm, q.hidden, type(q.net)) == ("plain", True, 256, MLP) and isinstance(q, CriticObs)
    assert CriticObsPlainLN(cond_dim=11, mlp_dims=[256] * 3).use_layernorm
    for kw in (dict(residual_style=True), dict(use_layernorm=False)):
        with pytest.raises(ValueError, match="CriticObsPlainLN"):
            CriticObsPlainLN(cond_dim=11, mlp_dims=[256] * 3, **kw)
    with pytest.raises(NotImplementedError, match=re.escape("mlp_dims = [256, 256, 256]")):
        CriticObsPlainLN(cond_dim=11, mlp_dims=[512] * 3)
    nets = {"residual": c, "plain": q}
    for head in HEADS:
        p = nets[head].init_params(np.random.default_rng(0))
        spec = ops.critic_param_spec(ops.ModelDims(**HOPPER_LN[head]))
        assert list(p) == [n for n, _ in spec] and all(p[n].shape == tuple(s) for n, s in spec)
        assert all((p[n] == (1.0 if n.endswith("_g") else 0.0)).all() for n in p if n.startswith("ln"))
        assert not CriticObs(cond_dim=11, mlp_dims=[256] * 3, residual_style=head == "residual").use_layernorm
    with pytest.raises(NotImplementedError, match="CriticObsPlainLN"):
        CriticObs(cond_dim=11, mlp_dims=[256] * 3, residual_style=False, use_layernorm=True)
    # every other refusal stays: other widths, the final norm, dropout, the actor's norm
    with pytest.raises(NotImplementedError):
        CriticObs(cond_dim=11, mlp_dims=[512] * 3, residual_style=True, use_layernorm=True)
    with pytest.raises(NotImplementedError):
        CriticObs(cond_dim=11, mlp_dims=[512] * 3, residual_style=False, use_layernorm=True)
    for cls in (MLP, ResidualMLP):
        for kw in (dict(use_layernorm_final=True), dict(dropout=0.1), dict(use_layernorm=True, use_layernorm_final=True)):
            with pytest.raises(NotImplementedError):
                cls([11, 256, 256, 256, 1], activation_type="Mish", **kw)
    with pytest.raises(NotImplementedError):
        ResidualMLP([39, 512, 512, 512, 12], activation_type="ReLU", use_layernorm=True)
    with pytest.raises(NotImplementedError):
        MLP([39, 512, 512, 12], activation_type="ReLU", use_layernorm=True)
    for rs, dims in ((True, [512] * 3), (False, [512, 512]), (True, [256] * 3)):
        with pytest.raises(NotImplementedError):
            DiffusionMLP(3, 4, 11, mlp_dims=dims, residual_style=rs, use_layernorm=True)
    with pytest.raises(NotImplementedError):                                  # an actor whose shape is the critic's
        DiffusionMLP(1, 1, 11, time_dim=16, mlp_dims=[256] * 3, residual_style=True, activation_type="Mish", use_layernorm=True)


# ------------------------------------------------------------------------------------------------
# the C ABI (host-only entries: no device needed)
# ------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["dppo_ppo_plan_critic", "dppo_pack_critic_ln", "dppo_critic_param_count_ln", "dppo_critic_packed_bytes_ln",
               "dppo_grad_clip_workspace_bytes_ln", "dppo_grad_clip_scales_ln", "dppo_ppo_clear_ranges_ln"]


def test_abi_carries_the_layer_norm():
    from diffusionpolicyoptimization_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "dppo.h")).read()
    declared = set(re.findall(r"DPPO_API\s+[\w\s\*]+?\b(dppo_\w+)\s*\(", src))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define DPPO_ABI_VERSION 15\b", src) and lib.dppo_abi_version() == 15
    assert re.search(r"enum \{ DPPO_LN_OFF = 0, DPPO_LN_ON = 1 \}", src)
    c = ops.ModelDims(**HOPPER).c()
    n8 = lib.dppo_critic_param_count(ctypes.byref(c))
    assert n8 == 11 * 256 + 256 + 2 * (256 * 256 + 256) + 256 + 1
    for prec in (0, 1, 2):
        b8 = lib.dppo_critic_packed_bytes(ctypes.byref(c), prec)
        for head in (0, 1):   # layer norm off: today's figures for both heads
            assert lib.dppo_critic_param_count_ln(ctypes.byref(c), head, 0) == n8
            assert lib.dppo_critic_packed_bytes_ln(ctypes.byref(c), prec, head, 0) == b8
        for head, sites in ((0, 2), (1, 3)):
            assert lib.dppo_critic_param_count_ln(ctypes.byref(c), head, 1) == n8 + 2 * sites * 256
            assert lib.dppo_critic_packed_bytes_ln(ctypes.byref(c), prec, head, 1) == b8 + 4 * 2 * sites * 256
    # attributes outside their enums: the size queries say 0
    assert lib.dppo_critic_param_count_ln(ctypes.byref(c), 2, 0) == 0 and lib.dppo_critic_param_count_ln(ctypes.byref(c), 0, 2) == 0
    assert lib.dppo_critic_packed_bytes_ln(ctypes.byref(c), 0, 0, -1) == 0
    assert lib.dppo_grad_clip_workspace_bytes_ln(ctypes.byref(c), 2, 0, 2) == 0
    # the clip workspace: one partial per chunk, the tail's vectors one chunk each; the old form is (RESIDUAL, OFF)
    w8 = lib.dppo_grad_clip_workspace_bytes(ctypes.byref(c), 2)
    assert lib.dppo_grad_clip_workspace_bytes_ln(ctypes.byref(c), 2, 0, 0) == w8 == lib.dppo_grad_clip_workspace_bytes_ln(ctypes.byref(c), 2, 1, 0)
    assert lib.dppo_grad_clip_workspace_bytes_ln(ctypes.byref(c), 2, 0, 1) == w8 + 4 * 8
    assert lib.dppo_grad_clip_workspace_bytes_ln(ctypes.byref(c), 2, 1, 1) == w8 + 6 * 8
    assert lib.dppo_grad_clip_workspace_bytes_ln(ctypes.byref(c), 3, 1, 1) == lib.dppo_grad_clip_workspace_bytes(ctypes.byref(c), 3) + 6 * 8
    # the critic's tile: 32 rows on 8 waves, the 128-register entry unless layer-normed
    out = (ctypes.c_int * 3)()
    for head in (0, 1):
        for lnorm in (0, 1):
            assert lib.dppo_ppo_plan_critic(ctypes.byref(c), 1, head, lnorm, out) == 0 and list(out) == [32, 8, 1 - lnorm]
    assert lib.dppo_ppo_plan_critic(ctypes.byref(c), 1, 0, 2, out) == 1 and lib.dppo_ppo_plan_critic(ctypes.byref(c), 1, 3, 0, out) == 1
    assert ops.ppo_plan_critic(ops.ModelDims(**HOPPER_LN["plain"]), "bf16") == dict(critic_tile_rows=32, critic_waves=8, critic_tile_capped=False)
    assert ops.ppo_plan_critic(ops.ModelDims(**HOPPER), "bf16")["critic_tile_capped"] is True
    # Python's sizes are the library's
    for head in HEADS:
        d = ops.ModelDims(**HOPPER_LN[head])
        assert ops.spec_count(ops.critic_param_spec(d)) == lib.dppo_critic_param_count_ln(ctypes.byref(c), _lib.HEAD[head], 1)
        assert ops.critic_packed_bytes(d, "bf16") == lib.dppo_critic_packed_bytes_ln(ctypes.byref(c), 1, _lib.HEAD[head], 1)
        assert ops.grad_clip_workspace_bytes(d, "critic") == lib.dppo_grad_clip_workspace_bytes_ln(ctypes.byref(c), 2, _lib.HEAD[head], 1)


# ------------------------------------------------------------------------------------------------
# checkpoints
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS)
def test_npz_round_trip_and_cross_layout_refusals(tmp_path, head):
    """The .npz names are the spec's (critic.ln1_g, ...); a file whose layer-norm tensors are not exactly the
    configured critic's is refused in both directions, and so is the other head's count of norms."""
    from diffusionpolicyoptimization_amd import ops
    d, off = ops.ModelDims(**HOPPER_LN[head]), ops.ModelDims(**dict(HOPPER, critic_head=head))
    spec, spec_off = ops.critic_param_spec(d), ops.critic_param_spec(off)
    rng = np.random.default_rng(2)
    params = {n: rng.normal(size=s).astype(np.float32) for n, s in spec}
    path = str(tmp_path / "ln.npz")
    np.savez(path, **{"critic." + n: v for n, v in ops.unflatten_params(spec, ops.flatten_params(spec, params)).items()})
    with np.load(path) as f:
        ops.check_checkpoint_critic_layernorm(f.files, spec, path)
        back = ops.flatten_params(spec, {n: f["critic." + n] for n, _ in spec})
        assert np.array_equal(back, ops.flatten_params(spec, params))
        with pytest.raises(ValueError, match="holds a layer-normed critic .*ln1_g.*, the model is a critic without layer norm"):
            ops.check_checkpoint_critic_layernorm(f.files, spec_off, path)
        other = ops.critic_param_spec(ops.ModelDims(**HOPPER_LN["plain" if head == "residual" else "residual"]))
        with pytest.raises(ValueError, match="holds a layer-normed critic"):
            ops.check_checkpoint_critic_layernorm(f.files, other, path)
    names_off = ["critic." + n for n, _ in spec_off]
    ops.check_checkpoint_critic_layernorm(names_off, spec_off, "off.npz")
    ops.check_checkpoint_critic_layernorm(["actor.in_w"], spec, "a.npz")        # no critic in the file
    with pytest.raises(ValueError, match="holds a critic without layer norm, the model is a layer-normed critic"):
        ops.check_checkpoint_critic_layernorm(names_off, spec, "off.npz")


# ------------------------------------------------------------------------------------------------
# cfgs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,head", [("ft_ppo_diffusion_mlp_critic_ln", "residual"),
                                       ("ft_ppo_diffusion_mlp_plain_critic_ln", "plain")])
def test_new_cfgs_load_and_resolve(name, head):
    from diffusionpolicyoptimization_amd.util.config import instantiate, load_config
    cfg = load_config(CFG_DIR, name, [])
    base = load_config(CFG_DIR, "ft_ppo_diffusion_mlp", [])
    assert cfg.model.critic.use_layernorm is True and cfg.model.critic.residual_style is (head == "residual")
    assert list(cfg.model.critic.mlp_dims) == [256, 256, 256] and cfg.model.critic.activation_type == "Mish"
    critic, actor = instantiate(cfg.model.critic), instantiate(cfg.model.actor)
    assert (critic.head, critic.use_layernorm, critic.hidden, actor.head) == (head, True, 256, "residual")
    assert dict(cfg.train) == dict(base.train) and cfg.env_name == base.env_name
    assert dict(cfg.model.actor) == dict(base.model.actor)


@pytest.mark.parametrize("head", HEADS)
def test_keras_h5_maps_gamma_and_beta(tmp_path, head):
    """The .h5 form: gamma / beta are vars/0 and vars/1 of each LayerNormalization (the plain head's in each hidden
    layer's Sequential, the residual block's norm1 / norm2); the round trip is exact and neither layout loads the
    other's file."""
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util import keras_weights as KW
    from diffusionpolicyoptimization_amd.util.h5 import read_h5
    d, off = ops.ModelDims(**HOPPER_LN[head]), ops.ModelDims(**dict(HOPPER, critic_head=head))
    sa, sc, sc_off = ops.actor_param_spec(d), ops.critic_param_spec(d), ops.critic_param_spec(off)
    rng = np.random.default_rng(1)
    mk = lambda spec: {n: rng.normal(size=s).astype(np.float32) for n, s in spec}
    actor, critic = mk(sa), mk(sc)
    plain = head == "plain"
    ln5, off5 = str(tmp_path / "ln.weights.h5"), str(tmp_path / "off.weights.h5")
    KW.save_ppo_model(ln5, actor, mk(sa), critic, critic_plain=plain)
    KW.save_ppo_model(off5, actor, mk(sa), {n: critic[n] for n, _ in sc_off}, critic_plain=plain)
    norms = sorted(k for k in read_h5(ln5) if "norm" in k)
    sites = 3 if plain else 2
    assert len(norms) == 2 * sites and all(k.startswith("critic/Q1/") and k[-7:] in ("/vars/0", "/vars/1") for k in norms)
    assert not any("norm" in k for k in read_h5(off5))
    w = KW.load_ppo_model(ln5, sa, sc, critic_plain=plain)
    assert set(w["critic"]) == set(critic) and all(np.array_equal(w["critic"][k], critic[k]) for k in critic)
    with pytest.raises(ValueError, match="does not map"):
        KW.load_ppo_model(ln5, sa, sc_off, critic_plain=plain)
    with pytest.raises(ValueError, match="missing critic variables.*ln1_g|missing critic variables"):
        KW.load_ppo_model(off5, sa, sc, critic_plain=plain)
