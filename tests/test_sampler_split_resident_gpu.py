"""Split sampler with register-resident in-Dense fragments and a software-pipelined step head.

The hopper 2-byte form keeps its in-Dense weight fragments in registers, every form reads the next
step's epilogue inputs (schedule row, noise, out bias) under the exchange wait and carries x in a
register, and the forms with every TIN row in LDS prefetch the next step's accumulator start. None
of this may change a value: the cases below run group boundaries (a partial group, one full group,
a boundary, the workload's 4 groups) against the oracle of tests/test_kernels_gpu.py with that
file's tolerances, for K' = 10 (two member sets, x handed over once), K' = K (no base steps) and
K' = 1 (the hand-over one step before the end). Each case launches twice on the same inputs and
requires bit-equal outputs: a prefetch that reads one step too far, or a stale carried x, shows up
there, against the oracle, or as NaN.

(The non-dual single-set path that switches actors mid-launch is chosen by the plan from the device's
CU count alone; nothing lets a test force it for 2-byte operands, so it is not covered here. fp32
hopper takes it from 9 groups (129 envs) to 32 on 256 CUs: tests/test_sampler_surface_gpu.py,
test_fp32_split_member_sets.)
"""
import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests.helpers import HOPPER, WALKER, make_models, to_f64

pytestmark = pytest.mark.gpu

TOL = {"fp32": 2e-4, "bf16": 2e-3, "fp16": 1e-3}     # tests/test_kernels_gpu.py::test_sampler_injected_noise
RND = {"bf16": O.round_bf16, "fp16": O.round_fp16}


def _run(cuda, dims, precision, E, seed):
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    d = ops.ModelDims(**dims)
    base, ft, _ = make_models(0, dims)
    sched = ddpm_buffers(d.denoising_steps)
    tab = torch.tensor(ops.sched_table(sched), device=cuda)
    flat = lambda p: torch.tensor(ops.flatten_params(ops.actor_param_spec(d), p), device=cuda)
    packb, packf = ops.pack_actor(d, flat(base), precision), ops.pack_actor(d, flat(ft), precision)
    K = d.denoising_steps
    rng = np.random.default_rng(seed)
    state = rng.uniform(-1, 1, (E, d.cond_steps, d.obs_dim)).astype(np.float32)
    xT = rng.standard_normal((E, d.horizon_steps, d.action_dim)).astype(np.float32)
    z = rng.standard_normal((K, E, d.horizon_steps, d.action_dim)).astype(np.float32)
    plan = ops.sampler_plan(d, precision, E)
    assert plan["kernel"] == 2, plan          # the folded split kernel
    ref_a, ref_c = O.sample(to_f64(base), to_f64(ft), sched, state.astype(np.float64), xT, z, d.ft_denoising_steps,
                            rnd=RND.get(precision), round_h3=False)
    outs = []
    for _ in range(2):
        act, ch = ops.sample(d, precision, packb, packf, tab, torch.tensor(state.reshape(E, -1), device=cuda),
                             x_T=torch.tensor(xT.reshape(E, -1), device=cuda),
                             noise=torch.tensor(z.reshape(K, E, -1), device=cuda))
        torch.cuda.synchronize()
        outs.append((act.cpu().numpy(), ch.cpu().numpy()))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    act, ch = outs[0][0].reshape(ref_a.shape), outs[0][1].reshape(ref_c.shape)
    assert ch.shape[1] == d.ft_denoising_steps + 1
    assert np.isfinite(act).all() and np.isfinite(ch).all()
    return plan, act, ch, ref_a, ref_c


@pytest.mark.parametrize("kf", [10, 20, 1])
@pytest.mark.parametrize("E", [1, 16, 17, 64])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_resident_hopper_two_byte(cuda, precision, E, kf):
    dims = dict(HOPPER, ft_denoising_steps=kf)
    plan, act, ch, ref_a, ref_c = _run(cuda, dims, precision, E, seed=1000 * kf + E)
    assert plan["members"] == 2 and plan["sets"] == (2 if kf < 20 else 1), plan
    tol = TOL[precision]
    # as test_sampler_injected_noise: the t = 19 x0 reconstruction amplifies eps differences by 406
    # before its clip, so a rare rounding-boundary flip can move one element
    q99 = np.quantile(np.abs(act - ref_a), 0.99)
    rows = np.abs(ch - ref_c).mean(axis=(0, 2, 3))      # every stored chain row
    print(f"{precision} E={E} K'={kf}: q99 {q99:.3e} max {np.abs(act - ref_a).max():.3e} chain rows max-mean {rows.max():.3e}")
    assert q99 < tol and np.abs(ch - ref_c).mean() < tol, (q99, np.abs(act - ref_a).max())
    assert (rows < tol).all(), rows


def test_pipelined_head_walker_bf16(cuda):
    """KX = 2 (walker2d): fragments stay in LDS and the TIN ring is untouched; the head is pipelined."""
    plan, act, ch, ref_a, ref_c = _run(cuda, WALKER, "bf16", 16, seed=7)
    q99 = np.quantile(np.abs(act - ref_a), 0.99)
    rows = np.abs(ch - ref_c).mean(axis=(0, 2, 3))
    print(f"walker bf16: q99 {q99:.3e} max {np.abs(act - ref_a).max():.3e} chain rows max-mean {rows.max():.3e}")
    assert q99 < TOL["bf16"] and (rows < TOL["bf16"]).all(), (q99, rows)


def test_pipelined_head_hopper_fp32(cuda):
    """fp32 (8 members of 4 waves, TIN ring): exact operands, checked on the maximum."""
    plan, act, ch, ref_a, ref_c = _run(cuda, HOPPER, "fp32", 16, seed=8)
    assert plan["members"] == 8, plan
    err_a, err_c = np.abs(act - ref_a).max(), np.abs(ch - ref_c).max()
    print(f"hopper fp32: max act {err_a:.3e} chains {err_c:.3e}")
    assert err_a < TOL["fp32"] and err_c < TOL["fp32"], (err_a, err_c)
