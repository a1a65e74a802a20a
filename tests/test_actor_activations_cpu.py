"""ELU, GELU and Softplus actors, the CPU half: the oracle's float64 definitions (O.ACT) are what they
say (derivatives, no overflow), the Python containers take the three names and the critic still refuses them,
the oracle tells every pair of supported activations apart by at least ten times the bound
the GPU file uses, and the C ABI carries the new enum values within ABI 15."""
import json
import os
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import test_update_surface_gpu as US
from tests import test_sampler_surface_gpu as SS
from tests.helpers import HOPPER, to_f64
from tests.variants import ALL_ACTIVATIONS, NEW_ACTIVATIONS, dims_of, mish_models, sampler_self_noise, site_coverage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENUM = {"ELU": 3, "GELU": 4, "Softplus": 5}
KW = dict(action_dim=3, horizon_steps=4, cond_dim=11, time_dim=16)


@pytest.mark.parametrize("name", NEW_ACTIVATIONS)
def test_derivative_is_the_forwards(name):
    """f' against the central difference of f on [-8, 8] (step 1e-5: truncation h^2 |f'''| / 6 <= 1e-10 for
    these functions, rounding 2e-16 / 1e-5 per unit of |f|: bound 1e-8 (1 + |x|)); ELU's kink at 0, where no
    derivative exists, is stepped over."""
    f, g = O.ACT[name]
    x = np.linspace(-8, 8, 160001)
    h = 1e-5
    if name == "ELU":
        x = x[np.abs(x) > 2 * h]
    fd = (f(x + h) - f(x - h)) / (2 * h)
    err = np.abs(fd - g(x)) / (1 + np.abs(x))
    print(json.dumps({"case": f"derivative-{name}", "max_err": float(err.max())}))
    assert err.max() < 1e-8
    # the definitions at points known in closed form
    one = np.array([1.0])
    want = {"ELU": (np.expm1(-1.0), np.exp(-1.0)), "GELU": (-0.15865525393145707, 0.15865525393145707 - 0.24197072451914337),   # -Phi(-1), Phi(-1) - phi(1)
            "Softplus": (np.log1p(np.exp(-1.0)), 1 / (1 + np.e))}[name]
    assert abs(f(-one)[0] - want[0]) < 1e-14 and abs(g(-one)[0] - want[1]) < 1e-14
    assert f(np.zeros(1))[0] == {"ELU": 0.0, "GELU": 0.0, "Softplus": np.log(2.0)}[name]


@pytest.mark.parametrize("name", NEW_ACTIVATIONS)
def test_no_overflow(name):
    """+-1e4 (and +-1e300) with floating-point errors raised: finite, the asymptotes exactly."""
    f, g = O.ACT[name]
    x = np.array([-1e300, -1e4, 1e4, 1e300])
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        y, dy = f(x), g(x)
    lo = -1.0 if name == "ELU" else 0.0
    assert np.array_equal(y, [lo, lo, 1e4, 1e300]) and np.array_equal(dy, [0.0, 0.0, 1.0, 1.0]), (y, dy)


@pytest.mark.parametrize("name", NEW_ACTIVATIONS)
def test_constructors_take_the_activation(name):
    """DiffusionMLP with both heads, its config round trip, ops.ModelDims; the critic and Tanh still refuse."""
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd.model.common.critic import CriticObs
    from diffusionpolicyoptimization_amd.model.common.mlp import MLP, SUPPORTED_ACTIVATIONS, ResidualMLP
    from diffusionpolicyoptimization_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    assert tuple(SUPPORTED_ACTIVATIONS) == ALL_ACTIVATIONS
    for residual, mlp_dims, head in ((True, [512, 512, 512], "residual"), (False, [512, 512], "plain")):
        net = DiffusionMLP(activation_type=name, mlp_dims=mlp_dims, residual_style=residual, **KW)
        assert net.activation_type == name and net.head == head and net.mlp_mean.activation_type == name
        cfg = net.get_config()
        assert cfg["activation_type"] == name
        again = DiffusionMLP(**cfg)
        assert again.get_config() == cfg and again.activation_type == name
    d = ops.ModelDims(**dims_of(name))
    assert d.activation == name and bytes(d.c()) == bytes(ops.ModelDims(**HOPPER).c())
    assert _lib.ACTOR_ACTIVATION[name] == ENUM[name]
    # the critic is Mish only: CriticObs refuses the name, and a widened list lets no critic shape through
    for kw in (dict(residual_style=True), dict(residual_style=False), dict(residual_style=True, use_layernorm=True),
               dict(residual_style=False, use_layernorm=True)):
        with pytest.raises(NotImplementedError):
            CriticObs(cond_dim=11, mlp_dims=[256, 256, 256], activation_type=name, **kw)
    with pytest.raises(NotImplementedError):
        MLP([11, 256, 256, 256, 1], activation_type=name)                      # layers4 requires Mish
    with pytest.raises(NotImplementedError):
        MLP([11, 256, 256, 256, 1], activation_type=name, use_layernorm=True)
    with pytest.raises(NotImplementedError):
        ResidualMLP([11, 256, 256, 256, 1], activation_type=name, use_layernorm=True)   # _critic_ln_shape requires Mish
    # Tanh stays refused, with the five supported names in the text
    with pytest.raises(NotImplementedError, match="ReLU, Mish, ELU, GELU, Softplus"):
        DiffusionMLP(activation_type="Tanh", mlp_dims=[512, 512, 512], residual_style=True, **KW)
    with pytest.raises(ValueError):
        ops.ModelDims(activation="Tanh")


# One problem per precision (tests/test_update_surface_gpu.py _Problem: weights, chains), the N(0, 1) biases of the
# Mish tests; the log-probs of every supported activation on it, computed once
_LP = {}


def _logprobs(precision):
    if precision not in _LP:
        p = US._Problem(HOPPER, precision)
        _, ft, _ = mish_models(0, HOPPER)
        out = {}
        for name in ALL_ACTIVATIONS:
            caches = []
            out[name] = O.get_logprobs(to_f64(ft), p.sched, p.state(p.obs), p.x(p.chains, p.kf + 1), p.kf,
                                       rnd=US._rnd(precision), model=O.Model(act=name), caches=caches)
            site_coverage(caches[-1])
        _LP[precision] = out
    return _LP[precision]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", NEW_ACTIVATIONS)
def test_oracle_tells_the_activations_apart(name, precision):
    """The log-probs of `name` against those of every other supported activation, same weights and chains
    (test_mish_oracle_moves_the_update's measure): q99 of |d| / (1 + |other|) >= 10x the log-prob bound of
    the GPU cases (1e-3 fp32, 2e-3 bf16). A pair below it is named."""
    lp = _logprobs(precision)
    tol = {"fp32": 1e-3, "bf16": 2e-3}[precision]
    q = {o: float(np.quantile(np.abs(lp[name] - lp[o]) / (1 + np.abs(lp[o])), 0.99)) for o in ALL_ACTIVATIONS if o != name}
    print(json.dumps({"case": f"apart-{name}-{precision}", "q99": q, "needs": 10 * tol}))
    close = {f"{name} vs {o}": v for o, v in q.items() if not v >= 10 * tol}
    assert not close, close


def test_sampler_q99_scale_is_the_oracles_own():
    """The reason behind ACT_Q99_SCALE of tests/test_actor_activations_gpu.py, on the oracle alone
    (sampler_self_noise: O.sample in bf16 against itself with 2e-7 relative noise ahead of each rounding, hopper,
    the GPU cases' inputs). At E = 513 the actions' q99 of ELU and of Softplus is past the ReLU network's 2e-3 bound
    in the reference itself while ReLU's and GELU's are inside, and the ratios to ReLU's lie in (1, 2] and
    (2, 3]: the factors 2 and 3. At E = 17 the q99 is the third largest of 204 values: over 16 noise draws
    Softplus's reaches past 2e-3 and stays inside 3 x 2e-3, ELU's and ReLU's stay inside 2e-3 (no factor there)."""
    from tests.test_actor_activations_gpu import ACT_Q99_SCALE
    tol = SS.TOL["bf16"]
    big, small = {}, {}
    for name in ("ReLU", "GELU", "ELU", "Softplus"):
        big[name] = sampler_self_noise(SS._Inputs(dims_of(name), 513, seed=11), "bf16", 0)["act_q99"]
        if name in ("ReLU", "ELU", "Softplus"):
            inp = SS._Inputs(dims_of(name), 17, seed=11)
            small[name] = [sampler_self_noise(inp, "bf16", s)["act_q99"] for s in range(16)]
    spread = {k: (min(v), float(np.median(v)), max(v)) for k, v in small.items()}
    print(json.dumps({"case": "oracle self-noise, actions q99", "E513": big, "E17 min/median/max": spread}))
    assert all(big[n] < tol for n in ("ReLU", "GELU")), big
    assert tol < big["ELU"] and 1 < big["ELU"] / big["ReLU"] <= ACT_Q99_SCALE[("ELU", "hopper-bf16-E513")] == 2, big
    assert tol < big["Softplus"] and 2 < big["Softplus"] / big["ReLU"] <= ACT_Q99_SCALE[("Softplus", "hopper-bf16-E513")] == 3, big
    assert max(small["ReLU"]) < tol and max(small["ELU"]) < tol, spread
    assert tol < max(small["Softplus"]) < ACT_Q99_SCALE[("Softplus", "hopper-bf16-E17")] * tol, spread
    assert set(ACT_Q99_SCALE) == {("ELU", "hopper-bf16-E513"), ("Softplus", "hopper-bf16-E17"), ("Softplus", "hopper-bf16-E513")}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_swapped_derivative_moves_the_gradients(monkeypatch, precision):
    """A kernel that ran GELU's forward with Mish's derivative would fail the gradient cases: the oracle with that
    pair against the oracle with GELU's own, on the GPU cases' problem (tests/test_update_surface_gpu.py _Problem,
    N(0, 1) biases), moves every actor gradient tensor that holds the derivative (l1, in, the time MLP) by more than TWICE the
    per-tensor bound (2e-3 fp32, 1e-2 bf16). Twice is what guarantees the failure: a kernel with the wrong pair
    that were within one bound of the wrong oracle is then more than one bound from the right one. Measured: 40 to
    72 bounds in fp32, 9 to 19 in bf16."""
    monkeypatch.setattr(US, "make_models", mish_models)
    p = US._Problem(dims_of("GELU"), precision)
    right = p.oracle()
    monkeypatch.setitem(O.ACT, "GELU", (O.ACT["GELU"][0], O.ACT["Mish"][1]))   # fault injection: a wrong pair
    wrong = p.oracle()
    moved = {k: US._rel(wrong[1][k], right[1][k]) for k in right[1]}
    print(json.dumps({"case": f"gelu-forward-mish-derivative-{precision}", "moved": moved, "needs": 2 * US.TOL[precision]}))
    after = ("out_w", "out_b", "l2_w", "l2_b")        # behind both sites: no derivative of the activation in them
    assert all(moved[k] == 0 for k in after), moved
    assert all(v > 2 * US.TOL[precision] for k, v in moved.items() if k not in after), moved


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_elu_swapped_for_relu_moves_the_sampler(precision):
    """A kernel that ran ReLU where the image says ELU would fail the sampler cases: O.sample with ELU against
    O.sample with ReLU, the GPU cases' inputs (hopper, E = 17), differs by >= 10x the sampler bound
    (SS._assert_moved: test_mish_oracle_moves_the_sampler's measure)."""
    inp = SS._Inputs(dims_of("ELU"), 17, seed=11)
    SS._assert_moved(f"elu-vs-relu-{precision}", precision, inp.oracle(precision), inp.oracle(precision, model=O.Model()))


def test_header_and_abi():
    """include/dppo.h holds the three enum values beside the first two, keeps 2 out, and stays ABI 15."""
    from diffusionpolicyoptimization_amd import _lib
    src = open(os.path.join(ROOT, "include", "dppo.h")).read()
    for name, v in (("RELU", 0), ("MISH", 1), ("ELU", 3), ("GELU", 4), ("SOFTPLUS", 5)):
        assert re.search(rf"\bDPPO_ACT_{name}\s*=\s*{v}\b", src), name
    assert not re.search(r"\bDPPO_ACT_\w+\s*=\s*2\b", src) and "2 reserved, refused" in src
    assert re.search(r"#define\s+DPPO_ABI_VERSION\s+15\b", src)
    assert _lib.load().dppo_abi_version() == 15
    assert _lib.ACTOR_ACTIVATION == {"ReLU": 0, "Mish": 1, "ELU": 3, "GELU": 4, "Softplus": 5}


def test_plan_is_the_mish_plan():
    """dppo_ppo_plan_act (host arithmetic): the new values take Mish's plan at every row count; 2, 6 and -1 are
    DPPO_EINVAL."""
    import ctypes
    from diffusionpolicyoptimization_amd import _lib, ops
    lib = _lib.load()
    for precision, rows in (("bf16", 150), ("bf16", 64 * 1024), ("fp32", 150), ("fp16", 33)):
        want = ops.ppo_plan(ops.ModelDims(**dims_of("Mish")), precision, rows)
        assert (want["actor_tile_rows"], want["actor_waves"]) == (32, 8)
        for name in NEW_ACTIVATIONS:
            assert ops.ppo_plan(ops.ModelDims(**dims_of(name)), precision, rows) == want, (name, precision, rows)
    out = (ctypes.c_int * 6)()
    d = ops.ModelDims(**HOPPER)
    for bad in (2, 6, -1):
        assert lib.dppo_ppo_plan_act(ctypes.byref(d.c()), 1, bad, 150, 0, out) == 1   # DPPO_EINVAL
