"""Mish actor, the CPU half: the Python container takes the reference's default activation, the oracle's
Mish actor (O.Model(act="Mish")) moves every quantity the GPU file compares by at least ten times
the bound used there, and the C ABI carries the new entries within ABI 15."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import test_sampler_surface_gpu as SS
from tests import test_update_surface_gpu as US
from tests.helpers import HOPPER, to_f64
from tests.variants import HOPPER_MISH, mish_models, site_coverage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_diffusion_mlp_takes_mish():
    """DiffusionMLP at the reference's default activation (mlp_diffusion.py:21) constructs and reports
    it; an activation the kernels do not implement still raises."""
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.model.diffusion.mlp_diffusion import DiffusionMLP
    kw = dict(action_dim=3, horizon_steps=4, cond_dim=11, time_dim=16, mlp_dims=[512, 512, 512], residual_style=True)
    net = DiffusionMLP(activation_type="Mish", **kw)
    assert net.activation_type == "Mish" and net.get_config()["activation_type"] == "Mish"
    assert DiffusionMLP(**kw).activation_type == "Mish"          # the reference's default
    assert DiffusionMLP(activation_type="ReLU", **kw).activation_type == "ReLU"
    with pytest.raises(NotImplementedError):
        DiffusionMLP(activation_type="Tanh", **kw)
    # the activation travels with ops.ModelDims (Python-only: dppo_dims keeps its layout)
    d = ops.ModelDims(**HOPPER_MISH)
    assert d.activation == "Mish" and ops.ModelDims(**HOPPER).activation == "ReLU"
    assert bytes(d.c()) == bytes(ops.ModelDims(**HOPPER).c())
    with pytest.raises(ValueError):
        ops.ModelDims(activation="Tanh")


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_mish_oracle_moves_the_sampler(precision):
    """O.sample with the Mish actor against ReLU, same weights and draws: >= 10x the sampler bound."""
    inp = SS._Inputs(HOPPER_MISH, 17, seed=11)
    SS._assert_moved(f"mish-vs-relu-{precision}", precision, inp.oracle(precision), inp.oracle(precision, model=O.Model()))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_mish_oracle_moves_the_update(monkeypatch, precision):
    """get_logprobs and the c_loss gradients with the Mish actor against ReLU on the same problem
    (weights, rows, old log-probs): >= 10x the bounds of the GPU cases; and the Mish problem's
    pre-activations cover x < -1 and x > 0 at both sites."""
    monkeypatch.setattr(US, "make_models", mish_models)
    p = US._Problem(HOPPER_MISH, precision)
    caches = []
    lp_m, ref_m = p.lp_ref, p.oracle(caches=caches)
    cov = site_coverage(caches[-1])
    lp_r = O.get_logprobs(to_f64(p.ft), p.sched, p.state(p.obs), p.x(p.chains, p.kf + 1), p.kf, rnd=US._rnd(precision))
    ref_r = p.oracle(model=O.Model())
    tol_lp = {"fp32": 1e-3, "bf16": 2e-3}[precision]
    rel = np.abs(lp_m - lp_r) / (1 + np.abs(lp_r))
    moved = {k: US._rel(ref_m[1][k], ref_r[1][k]) for k in ref_r[1]}
    print(json.dumps({"case": f"mish-vs-relu-update-{precision}", "coverage": cov, "lp_q99": float(np.quantile(rel, 0.99)),
                      "grads": moved}))
    assert np.quantile(rel, 0.99) >= 10 * tol_lp
    assert all(v >= 10 * US.TOL[precision] for v in moved.values()), moved


def test_abi_carries_the_activation():
    """dppo_pack_actor_act and dppo_ppo_plan_act are declared, bound and exported; the ABI stays 15."""
    from diffusionpolicyoptimization_amd import _lib
    lib = _lib.load()
    assert lib.dppo_abi_version() == 15
    src = open(os.path.join(ROOT, "include", "dppo.h")).read()
    declared = set(re.findall(r"DPPO_API\s+[\w\s\*]+?\b(dppo_\w+)\s*\(", src))
    nm = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(dppo_\w+)\b", nm))
    for name in ("dppo_pack_actor_act", "dppo_ppo_plan_act"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and name in exported, name
    assert re.search(r"DPPO_ACT_RELU\s*=\s*0\s*,\s*DPPO_ACT_MISH\s*=\s*1", src)
    assert _lib.ACTIVATION == {"ReLU": 0, "Mish": 1}
    # the plan query needs no device memory: a Mish actor runs the 32-row tile at every row count
    from diffusionpolicyoptimization_amd import ops
    for precision, rows in (("bf16", 150), ("bf16", 64 * 1024), ("fp32", 150)):
        plan = ops.ppo_plan(ops.ModelDims(**HOPPER_MISH), precision, rows)
        assert (plan["actor_tile_rows"], plan["actor_waves"]) == (32, 8), plan
    out = (__import__("ctypes").c_int * 6)()
    d = ops.ModelDims(**HOPPER)
    assert lib.dppo_ppo_plan_act(__import__("ctypes").byref(d.c()), 1, 7, 150, 0, out) == 1   # DPPO_EINVAL
