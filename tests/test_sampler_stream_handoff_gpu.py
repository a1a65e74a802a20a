"""The weight-streaming sampler's host hand-off paths and its fp16 form.

Every other pipelined or bound-rollout test runs hopper at 512 envs or fewer, which the split kernel
takes. The cases here are shapes the split kernel refuses (each test asserts sampler_layout == 0), so
the streaming kernel's own `go` wait, tagged observation load, cond_out copy, mapped actions_host and
tagged actions are what runs: in its 16-wave form (walker2d fp32: one full and one ragged 16-row
tile) and its 8-wave resident form (hopper bf16 at 513 envs, the first size past the split kernel).
Each hand-off test compares bit for bit with model(obs, return_chain=True) on the same Philox draws.
"""
import os

import numpy as np
import pytest

from oracle import dppo_oracle as O
from oracle import philox as PX
from tests.helpers import HOPPER, make_models, to_f64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WALKER_F32 = ("walker2d-v2", "fp32", 17, 3)     # 16 waves, nothing resident
HOPPER_BF16 = ("hopper-v2", "bf16", 513, 2)     # 8 waves, in/out layers + 2 hidden k-steps resident


def _model(cuda, env, precision, E, seed):
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util.config import instantiate, load_config
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune", env), "ft_ppo_diffusion_mlp",
                      [f"model.precision={precision}"])
    model = instantiate(cfg.model, device=cuda, seed=seed)
    assert ops.sampler_layout(model.dims, precision, E) == 0      # the streaming kernel
    return model


def _check_against_model(cuda, model, cid0, obs, got, obs_traj, chains, deterministic=()):
    import torch
    d, E = model.dims, obs[0].shape[0]
    model._call_id = cid0
    for i, o in enumerate(obs):
        ref = model(torch.tensor(o, device=cuda), deterministic=i in deterministic, return_chain=True)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(obs_traj[i].cpu().numpy(), o)
        np.testing.assert_array_equal(got[i], ref.trajectories.reshape(E, -1).cpu().numpy())
        np.testing.assert_array_equal(chains[i].cpu().numpy(), ref.chains.reshape(E, -1, d.xd).cpu().numpy())


@pytest.mark.parametrize("protocol", ["tagged", "go"])
@pytest.mark.parametrize("env,precision,E,S", [WALKER_F32, HOPPER_BF16], ids=["walker-fp32-17", "hopper-bf16-513"])
def test_stream_pipelined_rollout_matches_model_call(cuda, env, precision, E, S, protocol, monkeypatch):
    """RolloutPipe on the streaming kernel, both observation protocols: tagged (the kernel polls
    tagged granules, stores tagged actions) and go (the go wait, then cond from mapped memory and
    actions into mapped memory); cond_out fills obs_traj either way."""
    import torch
    monkeypatch.setenv("DPPO_ROLLOUT_PROTOCOL", protocol)
    from diffusionpolicyoptimization_amd import ops
    model = _model(cuda, env, precision, E, seed=5)
    d = model.dims
    obs_traj = torch.zeros(S, E, d.sd, device=cuda)
    chains = torch.zeros(S, E, d.ft_denoising_steps + 1, d.xd, device=cuda)
    act = torch.empty(E, d.xd, device=cuda)
    pipe = ops.RolloutPipe(model, obs_traj, act, chains)
    assert pipe.protocol == protocol
    rng = np.random.default_rng(2)
    obs = [rng.uniform(-1, 1, (E, d.sd)).astype(np.float32) for _ in range(S)]
    cid0 = model._call_id
    pipe.obs.numpy()[:] = obs[0]
    pipe.begin()
    pipe.enqueue(0)
    pipe.publish()
    got = []
    for i in range(S):
        if i + 1 < S:
            pipe.enqueue(i + 1)
        pipe.wait()
        got.append(pipe.act.numpy().copy())
        if i + 1 < S:
            pipe.obs.numpy()[:] = obs[i + 1]
            pipe.publish()
    pipe.end()
    torch.cuda.synchronize()
    _check_against_model(cuda, model, cid0, obs, got, obs_traj, chains)
    pipe.close()


def test_stream_bound_rollout_step_matches_model_call(cuda):
    """SampleStepper (dppo_sample_step) with pinned buffers on the 16-wave streaming kernel: cond
    read from and actions written to mapped host memory, cond_out into the rollout slot."""
    import torch
    env, precision, E, S = WALKER_F32
    model = _model(cuda, env, precision, E, seed=3)
    d = model.dims
    obs_pin = torch.empty(E, d.sd, dtype=torch.float32).pin_memory()
    act_pin = torch.empty(E, d.xd, dtype=torch.float32).pin_memory()
    obs_traj = torch.zeros(S, E, d.sd, device=cuda)
    chains = torch.zeros(S, E, d.ft_denoising_steps + 1, d.xd, device=cuda)
    act = torch.empty(E, d.xd, device=cuda)
    step = model.bind_rollout(obs_pin, obs_traj, act, act_pin, chains)
    rng = np.random.default_rng(0)
    obs = [rng.uniform(-1, 1, (E, d.sd)).astype(np.float32) for _ in range(S)]
    cid0 = model._call_id
    got = []
    for i in range(S):
        obs_pin.numpy()[:] = obs[i]
        step(i, deterministic=(i == 2))
        got.append(act_pin.numpy().copy())
    assert model._call_id == cid0 + S
    _check_against_model(cuda, model, cid0, obs, got, obs_traj, chains, deterministic=(2,))


def test_stream_sampler_fp16_philox(cuda):
    """fp16 on the streaming kernel (hopper, 513 envs, the kernel's own Philox noise) against the
    oracle rounding operands to fp16 at the kernel's rounding points, as
    test_sampler_bf16_sizes_philox does for bf16, with test_sampler_fp16_ddim_config5's bounds."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    d = ops.ModelDims(**HOPPER)
    base, ft, _ = make_models(0, HOPPER)
    sched = ddpm_buffers(d.denoising_steps)
    tab = torch.tensor(ops.sched_table(sched), device=cuda)
    flat = lambda p: torch.tensor(ops.flatten_params(ops.actor_param_spec(d), p), device=cuda)
    E, seed, call = 513, 987654321, 3
    assert ops.sampler_layout(d, "fp16", E) == 0
    rng = np.random.default_rng(E)
    state = rng.uniform(-1, 1, (E, 1, d.obs_dim)).astype(np.float32)
    K = d.denoising_steps
    xT = PX.sampler_normals(seed, call, 0, E, d.xd, K).reshape(E, d.horizon_steps, d.action_dim)
    z = np.stack([PX.sampler_normals(seed, call, 0, E, d.xd, i) for i in range(K)])
    z = z.reshape(K, E, d.horizon_steps, d.action_dim)
    ref_a, ref_c = O.sample(to_f64(base), to_f64(ft), sched, state.astype(np.float64), xT, z, d.ft_denoising_steps,
                            rnd=O.round_fp16, round_h3=True)
    act, ch = ops.sample(d, "fp16", ops.pack_actor(d, flat(base), "fp16"), ops.pack_actor(d, flat(ft), "fp16"), tab,
                         torch.tensor(state.reshape(E, -1), device=cuda), seed=seed, call_id=call)
    torch.cuda.synchronize()
    act = act.cpu().numpy().reshape(ref_a.shape)
    ch = ch.cpu().numpy().reshape(ref_c.shape)
    assert np.isfinite(act).all() and np.isfinite(ch).all()
    dev = np.abs(act - ref_a)
    q99, mean_c = np.quantile(dev, 0.99), np.abs(ch - ref_c).mean()
    print(f"fp16 streaming E={E}: q99 {q99:.3e} chain mean {mean_c:.3e} max {dev.max():.3e}")
    assert q99 < 1e-3 and mean_c < 1e-3, (dev.max(), q99, mean_c)
    assert dev.max() < 0.1, dev.max()
