"""Plain-head actor (DiffusionMLP residual_style=False, mlp_dims [h, h]), the CPU half: the oracle's plain head
(O.Model(head="plain")) is right (finite differences) and moves every quantity the GPU file compares by at
least ten times that quantity's bound; the Python containers accept exactly the supported shape; actor_spec
has no l2 and maps onto the residual offsets; the C ABI carries the new symbols within ABI 15; checkpoints
round-trip and do not cross heads."""
import json
import os
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import test_sampler_surface_gpu as SS
from tests import test_update_surface_gpu as US
from tests.helpers import HOPPER, to_f64
from tests.variants import HOPPER_PLAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["ReLU", "Mish"])
def test_plain_backward_matches_finite_differences(act):
    """Every gradient tensor of L = sum(w * eps) against central differences in float64 on a 7-input,
    8-wide net (2 x-coordinates, time_dim 4, 1 state value), 5 rows. Relative 1e-6 of the tensor's largest
    entry: float64 noise of a step-1e-6 central difference, not a measured quantity. (ReLU: the inputs keep
    every pre-activation at least 1e-3 from its kink, asserted.)"""
    rng = np.random.default_rng(5)
    td, xd, sd, h, B = 4, 2, 1, 8, 5
    p = {"time_w1": rng.normal(0, .5, (td, 2 * td)), "time_b1": rng.normal(0, .3, 2 * td),
         "time_w2": rng.normal(0, .5, (2 * td, td)), "time_b2": rng.normal(0, .3, td),
         "in_w": rng.normal(0, .6, (xd + td + sd, h)), "in_b": rng.normal(0, .5, h),
         "l1_w": rng.normal(0, .6, (h, h)), "l1_b": rng.normal(0, .5, h),
         "out_w": rng.normal(0, .6, (h, xd)), "out_b": rng.normal(0, .3, xd)}
    x, state = rng.normal(0, 1, (B, 1, xd)), rng.normal(0, 1, (B, 1, sd))
    t, w = rng.integers(0, 20, B), rng.normal(0, 1, (B, 1, xd))
    model = O.Model(act=act, head="plain")
    loss = lambda q: float((O.diffusion_mlp_forward(q, x, t, state, model)[0] * w).sum())
    _, cache = O.diffusion_mlp_forward(p, x, t, state, model)
    assert min(np.abs(cache["h1"]).min(), np.abs(cache["h2"]).min()) > 1e-3
    g = O.diffusion_mlp_backward(p, cache, w, xd, model)
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
    print(json.dumps({"case": f"plain-fd-{act}", "errs": errs}))
    assert all(e < 1e-6 for e in errs.values()), errs


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_plain_oracle_moves_the_sampler(precision):
    """O.sample with the plain head against the residual one, same weights and draws: actions and chains
    move by >= 10x the sampler bound."""
    inp = SS._Inputs(HOPPER_PLAIN, 17, seed=11)
    SS._assert_moved(f"plain-vs-residual-{precision}", precision, inp.oracle(precision), inp.oracle(precision, model=O.Model()))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_plain_oracle_moves_the_update(precision):
    """get_logprobs, the c_loss gradients per tensor and the pretrain loss with the plain head against the
    residual one on the same problem: >= 10x the bounds of the GPU cases."""
    p = US._Problem(HOPPER_PLAIN, precision)
    lp_p, ref_p = p.lp_ref, p.oracle()
    rng = np.random.default_rng(21)
    rows, d = 40, p.d
    sh = (rows, d.horizon_steps, d.action_dim)
    pre = lambda model: O.p_losses(to_f64(p.ft), p.sched, rng0["x0"], rng0["cond"], rng0["t"], rng0["z"],
                                   rnd=US._rnd(precision), model=model)
    rng0 = dict(x0=rng.uniform(-1, 1, sh), cond=rng.uniform(-1, 1, (rows, d.cond_steps, d.obs_dim)),
                t=rng.integers(0, d.denoising_steps, rows), z=rng.standard_normal(sh))
    loss_p, _ = pre(p.model)
    lp_r = O.get_logprobs(to_f64(p.ft), p.sched, p.state(p.obs), p.x(p.chains, p.kf + 1), p.kf, rnd=US._rnd(precision))
    ref_r = p.oracle(model=O.Model())
    loss_r, _ = pre(O.Model())
    tol_lp = {"fp32": 1e-3, "bf16": 2e-3}[precision]
    rel = np.abs(lp_p - lp_r) / (1 + np.abs(lp_r))
    moved = {k: US._rel(ref_p[1][k], ref_r[1][k]) for k in ref_p[1]}
    loss_moved = abs(loss_p - loss_r) / loss_r
    print(json.dumps({"case": f"plain-vs-residual-update-{precision}", "lp_q99": float(np.quantile(rel, 0.99)),
                      "grads": moved, "pretrain_loss": loss_moved}))
    assert set(ref_p[1]) == set(ref_r[1]) - {"l2_w", "l2_b"}
    assert np.quantile(rel, 0.99) >= 10 * tol_lp
    assert all(v >= 10 * US.TOL[precision] for v in moved.values()), moved
    assert loss_moved >= 10 * {"fp32": 2e-3, "bf16": 1e-2}[precision]


# ------------------------------------------------------------------------------------------------
# the Python containers
# ------------------------------------------------------------------------------------------------
def test_mlp_and_diffusion_mlp_accept_two_hidden_layers():
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.model.common.critic import CriticObs
    from diffusionpolicyoptimization_amd.model.common.mlp import MLP
    from diffusionpolicyoptimization_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    net = DiffusionMLP(action_dim=3, horizon_steps=4, cond_dim=11)            # the reference's own defaults
    assert (net.residual_style, net.mlp_dims, net.head, net.hidden, net.activation_type) == (False, [256, 256], "plain", 256, "Mish")
    assert net.get_config()["residual_style"] is False
    p = net.init_params(np.random.default_rng(0))
    assert "l2_w" not in p and p["out_w"].shape == (256, 12) and p["in_w"].shape == (12 + 16 + 11, 256)
    assert DiffusionMLP(3, 4, 11, mlp_dims=[512, 512, 512], residual_style=True).head == "residual"
    m = MLP([39, 512, 512, 12], activation_type="ReLU")
    assert m.hidden == 512
    for dims in ([39, 512, 12], [39, 512, 512, 512, 12], [39, 512, 256, 12]):
        with pytest.raises(NotImplementedError, match=re.escape("[in, h, h, out]")):
            MLP(dims, activation_type="ReLU")
    for kw in (dict(use_layernorm=True), dict(dropout=0.1), dict(append_dim=2, append_layers=[0]),
               dict(out_activation_type="Tanh")):
        with pytest.raises(NotImplementedError, match=re.escape("[in, h, h, out]")):
            MLP([39, 512, 512, 12], activation_type="ReLU", **kw)
    for kw in (dict(mlp_dims=[256]), dict(mlp_dims=[256, 256, 256]), dict(mlp_dims=[256, 128]), dict(use_layernorm=True),
               dict(cond_mlp_dims=[64, 32])):
        with pytest.raises(NotImplementedError):
            DiffusionMLP(3, 4, 11, **kw)
    with pytest.raises(NotImplementedError):                                 # the critic has no plain form
        CriticObs(cond_dim=11, mlp_dims=[256, 256], residual_style=False)
    d = ops.ModelDims(**HOPPER_PLAIN)
    assert d.head == "plain" and ops.ModelDims(**HOPPER).head == "residual"
    assert bytes(d.c()) == bytes(ops.ModelDims(**HOPPER).c())                # Python-only: dppo_dims keeps its layout
    with pytest.raises(ValueError):
        ops.ModelDims(head="deep")


def test_actor_spec_has_no_l2_and_keeps_the_residual_offsets():
    from diffusionpolicyoptimization_amd import ops
    plain, full = ops.actor_param_spec(ops.ModelDims(**HOPPER_PLAIN)), ops.actor_param_spec(ops.ModelDims(**HOPPER))
    assert [n for n, _ in plain] == [n for n, _ in full if n not in ("l2_w", "l2_b")]
    assert ops.spec_count(plain) == ops.spec_count(full)
    rng = np.random.default_rng(0)
    params = {n: rng.normal(size=s).astype(np.float32) for n, s in full}
    flat_full, flat_plain = ops.flatten_params(full, params), ops.flatten_params(plain, params)
    un = ops.unflatten_params(full, flat_plain)
    assert not un["l2_w"].any() and not un["l2_b"].any()
    for n, _ in plain:
        assert np.array_equal(un[n], params[n]) and np.array_equal(ops.unflatten_params(plain, flat_full)[n], params[n])
    assert set(ops.unflatten_params(plain, flat_plain)) == {n for n, _ in plain}


def test_abi_carries_the_head():
    """The new symbol and enum are declared and bound within ABI 15 (tests/test_host_cpu.py's nm test then
    covers the library's exports)."""
    from diffusionpolicyoptimization_amd import _lib
    src = open(os.path.join(ROOT, "include", "dppo.h")).read()
    declared = set(re.findall(r"DPPO_API\s+[\w\s\*]+?\b(dppo_\w+)\s*\(", src))
    assert "dppo_pack_actor_head" in declared and "dppo_pack_actor_head" in _lib.EXPORTED_SYMBOLS
    assert re.search(r"DPPO_HEAD_RESIDUAL\s*=\s*0\s*,\s*DPPO_HEAD_PLAIN\s*=\s*1", src)
    assert re.search(r"#define DPPO_ABI_VERSION 15\b", src)
    assert _lib.HEAD == {"residual": 0, "plain": 1}
    lib = _lib.load()
    assert lib.dppo_abi_version() == 15 and hasattr(lib, "dppo_pack_actor_head")
    assert "l2_w / l2_b" in src and "range unused" in src                     # the layout comment says so


# ------------------------------------------------------------------------------------------------
# checkpoints
# ------------------------------------------------------------------------------------------------
def test_keras_weights_round_trip_and_cross_head_errors(tmp_path):
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util import keras_weights as KW
    dp, dr = ops.ModelDims(**HOPPER_PLAIN), ops.ModelDims(**HOPPER)
    sp, sr, sc = ops.actor_param_spec(dp), ops.actor_param_spec(dr), ops.critic_param_spec(dp)
    rng = np.random.default_rng(1)
    mk = lambda spec: {n: rng.normal(size=s).astype(np.float32) for n, s in spec}
    plain, resid, critic = mk(sp), mk(sr), mk(sc)
    a, b, m = str(tmp_path / "plain.weights.h5"), str(tmp_path / "resid.weights.h5"), str(tmp_path / "ppo.weights.h5")
    KW.save_actor(a, plain)
    KW.save_actor(b, resid)
    got = KW.load_actor(a, sp)
    assert set(got) == set(plain) and all(np.array_equal(got[k], plain[k]) for k in plain)
    from diffusionpolicyoptimization_amd.util.h5 import read_h5
    names = [k for k in read_h5(a) if k != "__groups__"]
    assert "mlp_mean/module_list/sequential_2/layers/dense/vars/0" in names and not any("residual_blocks" in k for k in names)
    with pytest.raises(ValueError):
        KW.load_actor(b, sp)          # a residual file into a plain actor
    with pytest.raises(ValueError):
        KW.load_actor(a, sr)          # and the other way round
    KW.save_ppo_model(m, plain, mk(sp), critic)
    w = KW.load_ppo_model(m, sp, sc)
    assert all(np.array_equal(w["actor"][k], plain[k]) for k in plain) and "l2_w" not in w["actor_ft"]
    with pytest.raises(ValueError):
        KW.load_ppo_model(m, sr, sc)


def test_npz_names_and_cross_head_check(tmp_path):
    """The .npz rule both models apply: exactly the spec's tensors; a file of the other head raises."""
    from diffusionpolicyoptimization_amd import ops
    sp, sr = ops.actor_param_spec(ops.ModelDims(**HOPPER_PLAIN)), ops.actor_param_spec(ops.ModelDims(**HOPPER))
    ops.check_checkpoint_head(["actor." + n for n, _ in sp], sp, "p.npz", "actor.")
    ops.check_checkpoint_head(["actor." + n for n, _ in sr], sr, "r.npz", "actor.")
    with pytest.raises(ValueError, match="residual"):
        ops.check_checkpoint_head(["actor." + n for n, _ in sr], sp, "r.npz", "actor.")
    with pytest.raises(ValueError, match="plain"):
        ops.check_checkpoint_head(["actor." + n for n, _ in sp], sr, "p.npz", "actor.")
    # an unprefixed plain actor beside a critic: the critic's l2_w is not the actor's
    ops.check_checkpoint_head([n for n, _ in sp] + ["critic.l2_w"], sp, "p.npz")
    with pytest.raises(ValueError, match="plain"):
        ops.check_checkpoint_head([n for n, _ in sp] + ["critic.l2_w"], sr, "p.npz")
