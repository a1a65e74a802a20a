"""Plain-head actor on the GPU: the entries that take a packed actor image, against the oracle's plain head
(O.Model(head="plain"), derived from the dims).

Bounds are the residual cases' of the same entry and path, unchanged (tests/test_actor_mish_gpu.py lists
them): the sampler's of tests/test_sampler_surface_gpu.py, test_logprob's, the per-tensor gradient bounds of
the update tests (2e-3 fp32, 1e-2 2-byte), test_split_update_matches_fused's for the agent. Every figure is
printed as a JSON line before it is asserted. Problems and device halves are the surface tests' with
`head="plain"` in the dims, so ops.pack_actor records the head with every image and the flat parameters keep
a zero l2 range. In every gradient case the l2 range of `grads` must be exactly zero."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import test_kernels_gpu as KG
from tests import test_sampler_surface_gpu as SS
from tests import test_update_regimes_gpu as UR
from tests import test_update_surface_gpu as US
from tests.helpers import HOPPER, HOPPER_DDIM, to_f64
from tests.variants import HOPPER_PLAIN, PLAIN, WALKER_PLAIN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOPPER_PLAIN_MISH = dict(HOPPER_PLAIN, activation="Mish")
HOPPER_DDIM_PLAIN = dict(HOPPER_DDIM, **PLAIN)
SPLIT, STREAM = 2, 0


def _l2_range(d):
    """[lo, hi) of l2_w | l2_b in the flat actor layout (the residual spec of the same dims)."""
    import dataclasses
    from diffusionpolicyoptimization_amd import ops
    o = 0
    for n, s in ops.actor_param_spec(dataclasses.replace(d, head="residual")):
        if n == "l2_w":
            return o, o + d.actor_hidden * d.actor_hidden + d.actor_hidden
        o += int(np.prod(s))


def _l2_is_zero(d, flat):
    lo, hi = _l2_range(d)
    seg = np.asarray(flat)[lo:hi]
    return seg.size == d.actor_hidden * (d.actor_hidden + 1) and not seg.any()


# ------------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------------
# (label, dims, precision, envs, kernel, oracle / launch keywords)
SAMPLER_CASES = [
    ("hopper-fp32-E16", HOPPER_PLAIN, "fp32", 16, SPLIT, {}),                 # one group; fp32 split (skip operand from T_OUT)
    ("hopper-bf16-E16", HOPPER_PLAIN, "bf16", 16, SPLIT, {}),
    ("hopper-fp16-E17", HOPPER_PLAIN, "fp16", 17, SPLIT, {}),                 # a second, partial group
    ("hopper-fp32-E17-mish", HOPPER_PLAIN_MISH, "fp32", 17, SPLIT, {}),
    ("hopper-bf16-E64-mish", HOPPER_PLAIN_MISH, "bf16", 64, SPLIT, {}),
    ("hopper-bf16-E64", HOPPER_PLAIN, "bf16", 64, SPLIT, {}),
    ("hopper-bf16-E513", HOPPER_PLAIN, "bf16", 513, STREAM, {}),              # the streaming kernel, 2-byte
    ("hopper-fp32-E513", HOPPER_PLAIN, "fp32", 513, STREAM, {}),              # the streaming kernel, fp32
    ("hopper-fp16-E513-mish", HOPPER_PLAIN_MISH, "fp16", 513, STREAM, {}),
    ("walker-bf16-E16", WALKER_PLAIN, "bf16", 16, SPLIT, {}),                 # two in-Dense k-steps
    ("walker-fp32-E16", WALKER_PLAIN, "fp32", 16, STREAM, {}),
    ("hopper-bf16-E16-eval", HOPPER_PLAIN, "bf16", 16, SPLIT, dict(deterministic=True)),
    ("hopper-fp16-E16-ddim", HOPPER_DDIM_PLAIN, "fp16", 16, SPLIT, {}),       # DDIM at stride 2
]


@pytest.mark.parametrize("label,dims,precision,E,kernel,kw", SAMPLER_CASES, ids=[c[0] for c in SAMPLER_CASES])
def test_sampler_matches_plain_oracle(cuda, label, dims, precision, E, kernel, kw):
    """dppo_sample on plain images, injected noise, against O.sample with the plain head: actions and every
    stored chain row; the plan is the residual plan of the same shape."""
    from diffusionpolicyoptimization_amd import ops
    inp = SS._Inputs(dims, E, seed=11)
    g = SS._Gpu(inp, precision, cuda)
    res_dims = {k: v for k, v in dims.items() if k not in ("activation", "head")}
    assert g.plan["kernel"] == kernel and g.plan == ops.sampler_plan(ops.ModelDims(**res_dims), precision, E), g.plan
    act, ch = g.twice(**kw)
    SS._check(f"plain {label}", precision, SS._stats(act, ch, *inp.oracle(precision, **kw)), plan=g.plan)


KF_EDGES = [("hopper", HOPPER_PLAIN, "bf16", 513, 20), ("hopper", HOPPER_PLAIN_MISH, "fp16", 513, 20),
            ("walker", WALKER_PLAIN, "fp32", 37, 20), ("hopper", HOPPER_PLAIN, "bf16", 513, 1)]


@pytest.mark.parametrize("name,dims,precision,E,kf", KF_EDGES,
                         ids=[f"{n}{'-mish' if 'activation' in d else ''}-{p}-E{e}-kf{k}" for n, d, p, e, k in KF_EDGES])
def test_streaming_kf_edges_plain(cuda, name, dims, precision, E, kf):
    """The streaming kernel's plain instantiation at K' = K (chain row 0 = x_T from the draw loop, no actor
    switch) and K' = 1 (the resident set reloaded before the last step): test_streaming_kf_edges on plain images."""
    inp = SS._Inputs(dict(dims, ft_denoising_steps=kf), E, seed=1000 * kf + E)
    g = SS._Gpu(inp, precision, cuda)
    assert g.plan["kernel"] == STREAM, g.plan
    act, ch = g.twice()
    assert ch.shape[1] == kf + 1
    if kf == 20:
        assert ch[:, 0].tobytes() == inp.xT.tobytes()
    SS._check(f"plain stream-{name}-{precision}-E{E}-kf{kf}", precision, SS._stats(act, ch, *inp.oracle(precision)), plan=g.plan)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sample_step_equals_sample_plain(cuda, precision):
    """dppo_sample_step on plain images at 16 envs through mapped staging memory: bit-equal to dppo_sample on
    the same Philox stream, and within the sampler's bound of the plain oracle."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import ptr, stream_handle
    E = 16
    inp = SS._Inputs(HOPPER_PLAIN, E, seed=11)
    g = SS._Gpu(inp, precision, cuda)
    d = inp.d
    mc, ma = ops.MappedArray((E, d.sd), np.float32), ops.MappedArray((E, d.xd), np.float32)
    mc.tensor.copy_(torch.from_numpy(inp.state.reshape(E, -1)))
    ma.tensor.fill_(SS.SENTINEL)
    cond = torch.full((E, d.sd), SS.SENTINEL, device=cuda)
    actions = torch.full((E, d.xd), SS.SENTINEL, device=cuda)
    chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SS.SENTINEL, device=cuda)
    host_ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.call("dppo_sample_step", ctypes.byref(d.c()), _lib.PRECISION[precision], ptr(g.packb), ptr(g.packf), ptr(g.tab),
              host_ptr(mc.tensor), ptr(cond), E, ctypes.c_uint64(SS.SEED), ctypes.c_uint64(SS.CALL), 0, 0, 0.1, 3.0, 0.0,
              ptr(actions), host_ptr(ma.tensor), ptr(chains), 1, stream_handle(cuda))
    torch.cuda.synchronize()
    a_ref, c_ref = g.sample(xT=None, z=None)
    assert np.array_equal(cond.cpu().numpy(), inp.state.reshape(E, -1))
    assert actions.cpu().numpy().tobytes() == a_ref.tobytes() and chains.cpu().numpy().tobytes() == c_ref.tobytes()
    assert ma.tensor.numpy().tobytes() == a_ref.tobytes()
    SS._check(f"plain step-{precision}", precision, SS._stats(a_ref, c_ref, *inp.oracle(precision, *inp.philox())))


def test_tagged_rollout_equals_model_call_plain(cuda, monkeypatch):
    """dppo_rollout_enqueue_tagged on the model of ft_ppo_diffusion_mlp_plain.yaml (bf16, 16 envs, two
    pre-enqueued steps): observations, actions and chains bit-equal to model(obs), which is dppo_sample."""
    import torch
    monkeypatch.setenv("DPPO_ROLLOUT_PROTOCOL", "tagged")
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util.config import instantiate, load_config
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp_plain", ["model.precision=bf16"])
    model = instantiate(cfg.model, device=cuda, seed=5)
    d = model.dims
    assert d.head == "plain"
    S, E = 2, 16
    obs_traj = torch.zeros(S, E, d.sd, device=cuda)
    chains = torch.zeros(S, E, d.ft_denoising_steps + 1, d.xd, device=cuda)
    act = torch.empty(E, d.xd, device=cuda)
    pipe = ops.RolloutPipe(model, obs_traj, act, chains)
    assert pipe.protocol == "tagged"
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
    model._call_id = cid0
    for i in range(S):
        ref = model(torch.tensor(obs[i], device=cuda), return_chain=True)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(obs_traj[i].cpu().numpy(), obs[i])
        np.testing.assert_array_equal(got[i], ref.trajectories.reshape(E, -1).cpu().numpy())
        np.testing.assert_array_equal(chains[i].cpu().numpy(), ref.chains.reshape(E, -1, d.xd).cpu().numpy())
    pipe.close()


@pytest.mark.parametrize("precision,E", [("bf16", 16), ("bf16", 513), ("fp32", 16)])
def test_sampler_refuses_mixed_heads(cuda, precision, E):
    """A residual base image with a plain fine-tuned image (and the reverse): DPPO_EINVAL before anything is
    enqueued, outputs left at the sentinel; the next accepted launch on the stream is unaffected."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd._lib import DppoError
    inp = SS._Inputs(HOPPER_PLAIN, E, seed=11)
    g = SS._Gpu(inp, precision, cuda)
    d = inp.d
    res = ops.ModelDims(**HOPPER)
    _, _, _, _, _, _, pb, pf, _ = KG._setup(HOPPER, cuda)
    for base, ft in ((ops.pack_actor(res, pb, precision), g.packf), (g.packb, ops.pack_actor(res, pf, precision))):
        actions = torch.full((E, d.xd), SS.SENTINEL, device=cuda)
        chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SS.SENTINEL, device=cuda)
        msg = "failed (1): dppo_sample: the base and the fine-tuned actor images carry different heads"
        with pytest.raises(DppoError, match=re.escape(msg)):
            ops.sample(d, precision, base, ft, g.tab, g.T(inp.state.reshape(E, -1)), x_T=g.T(inp.xT.reshape(E, -1)),
                       noise=g.T(inp.z.reshape(inp.K, E, -1)), actions=actions, chains=chains)
        torch.cuda.synchronize()
        assert bool((actions == SS.SENTINEL).all()) and bool((chains == SS.SENTINEL).all())
    g.sample()


# ------------------------------------------------------------------------------------------------
# dppo_logprob, dppo_ppo_minibatch, dppo_pretrain_minibatch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16", 2e-3)])
def test_logprob_matches_plain_oracle(cuda, precision, tol):
    """dppo_logprob on a plain image at n = 5 samples (50 rows: a partial 32-row tile)."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    d, _, ft, _, sched, tab, _, pf, _ = KG._setup(HOPPER_PLAIN, cuda)
    n, kf = 5, d.ft_denoising_steps
    rng = np.random.default_rng(4)
    state = rng.uniform(-1, 1, (n, 1, d.obs_dim)).astype(np.float32)
    chains = (rng.standard_normal((n, kf + 1, d.horizon_steps, d.action_dim)) * 0.5).astype(np.float32)
    ref = O.get_logprobs(to_f64(ft), sched, state.astype(np.float64), chains.astype(np.float64), kf, rnd=KG._rnd(precision),
                         model=O.Model.from_dims(d))
    lpe, lpm = ops.logprob(d, precision, ops.pack_actor(d, pf, precision), tab, torch.tensor(state.reshape(n, -1), device=cuda),
                           torch.tensor(chains.reshape(n, kf + 1, -1), device=cuda))
    torch.cuda.synchronize()
    lpe = lpe.cpu().numpy().reshape(ref.shape)
    ref_mean = np.clip(ref, -5, 2).mean(axis=(1, 2)).reshape(n, kf)
    q99 = float(np.quantile(np.abs(lpe - ref) / (1 + np.abs(ref)), 0.99))
    mean_err = float(np.abs(lpm.cpu().numpy() - ref_mean).max())
    print(json.dumps({"case": f"plain-logprob-{precision}", "q99": q99, "bound": tol, "mean_err": mean_err}))
    assert q99 < tol and mean_err < tol * 10


GRAD_CASES = [("fp32", HOPPER_PLAIN, 96, False), ("fp32", HOPPER_PLAIN, 100, False), ("bf16", HOPPER_PLAIN, 96, False),
              ("bf16", HOPPER_PLAIN, 100, True), ("fp16", HOPPER_PLAIN, 100, False), ("bf16", HOPPER_PLAIN_MISH, 100, False),
              ("bf16", WALKER_PLAIN, 100, False)]


@pytest.mark.parametrize("precision,dims,rows,deferred", GRAD_CASES,
                         ids=[f"{p}-{'walker' if d is WALKER_PLAIN else 'hopper'}{'-mish' if 'activation' in d else ''}-r{r}"
                              f"{'-l2def' if q else ''}" for p, d, r, q in GRAD_CASES])
def test_ppo_minibatch_grads_match_plain_oracle(cuda, precision, dims, rows, deferred):
    """dppo_ppo_minibatch on a plain image at rows = 96 (whole tiles) and 100 (a tile tail): the loss metrics
    and every gradient tensor against O.c_loss with the plain head (the regime tests' bounds); the l2 range of
    grads is exactly zero, also under DPPO_PPO_L2_DEFERRED (nothing to defer: dW_out is written in place)."""
    case = UR._Case(cuda, precision, dims, -(-(UR.START + rows) // 10) + 20)
    stats, mean_std = case.adv_stats(rows)
    met_ref, ga_ref, gc_ref = case.oracle(rows, adv_mean_std=mean_std)
    assert "l2_w" not in ga_ref and "out_w" in ga_ref
    g, m = case.launch(rows, UR.START, rows, stats=stats, l2_deferred=deferred)
    assert np.isfinite(g).all() and _l2_is_zero(case.d, g)
    UR._check_metrics(m / rows, met_ref, UR.TOL[precision], True, f"plain-{precision}-r{rows}")
    errs = UR._tensor_errs(case.d, g, ga_ref, gc_ref)
    print(json.dumps({"case": f"plain-grads-{precision}-r{rows}", "errs": errs}))
    UR._check_errs(errs, UR.TOL[precision], f"plain-{precision}-r{rows}")


def _grads_vs_oracle(case, rows, label, ratio1=True, **kw):
    """One whole minibatch of a UR._Case against its oracle at the regime tests' bounds; l2 range exactly zero."""
    stats, mean_std = case.adv_stats(rows)
    met_ref, ga_ref, gc_ref = case.oracle(rows, adv_mean_std=mean_std, eta_grad=kw.get("learn_eta", False))
    assert "l2_w" not in ga_ref and "out_w" in ga_ref
    g, m = case.launch(rows, UR.START, rows, stats=stats, **kw)
    assert np.isfinite(g).all() and _l2_is_zero(case.d, g)
    tol = UR.TOL[case.precision]
    UR._check_metrics(m / rows, met_ref, tol, ratio1, label)
    UR._check_errs(UR._tensor_errs(case.d, g, ga_ref, gc_ref), tol, label)
    return m, met_ref


FT_CASES = [("fp32", 1), ("bf16", 1), ("fp32", 17), ("bf16", 17)]


@pytest.mark.parametrize("precision,kf", FT_CASES, ids=[f"{p}-kf{k}" for p, k in FT_CASES])
def test_ppo_minibatch_ft_steps_plain(cuda, precision, kf):
    """dppo_ppo_minibatch on a plain image at K' = 1 (one bucket) and K' = 17 (bucket 16 alone in the dW's
    second wave row, tests/test_update_ft_steps_gpu.py): 150 rows, every gradient tensor. As in that file and in
    test_update_surface_gpu's ft1 line, fp32 takes perturbed old log-probs (rows on both clip branches; at
    K' = 1 the clip width is zero, so every row whose ratio is not exactly 1 counts as clipped) and the 2-byte
    case ratio 1 against the rounding oracle."""
    n = 160 if kf == 1 else 40
    f32 = precision == "fp32"
    case = UR._Case(cuda, precision, dict(HOPPER_PLAIN, ft_denoising_steps=kf), -(-UR.START // kf) + n,
                    lp="perturbed" if f32 else "ratio1")
    _grads_vs_oracle(case, 150, f"plain-{precision}-kf{kf}", ratio1=not f32)


def test_ppo_minibatch_learn_eta_ddim_plain(cuda):
    """DPPO_PPO_LEARN_ETA behind a plain forward (hopper DDIM, bf16, eta 0.6): metrics[8] against the oracle at
    the 64-row tile test's d_eta bound (3e-2 relative), and every gradient tensor."""
    rows = US.ROWS
    case = UR._Case(cuda, "bf16", HOPPER_DDIM_PLAIN, US.NSAMP, eta=0.6)
    m, met_ref = _grads_vs_oracle(case, rows, "plain-learn-eta", learn_eta=True)
    ref = met_ref["d_eta"]
    print(json.dumps({"case": "plain-learn-eta", "d_eta": float(m[8]), "ref": ref}))
    assert abs(ref) > 1e-3 and abs(m[8] - ref) <= 3e-2 * abs(ref), (m[8], ref)


def test_ppo_minibatch_parts_match_whole_plain(cuda):
    """dppo_ppo_minibatch_part on a plain image as actor row tiles (4), actor dW (5) and critic (2), bf16, 150
    rows: the parts against the oracle and against the whole call within test_ft20_parts_match_whole's bounds
    (median 1e-6, max 5e-3 absolute; metrics 1e-3 relative); the l2 range exactly zero on both."""
    from tests import test_update_ft_steps_gpu as FT
    rows = FT.ROWS
    case = UR._Case(cuda, "bf16", HOPPER_PLAIN, FT.NSAMP)
    whole, parts = FT._Out(case, rows), FT._Out(case, rows)
    FT._launch(case, whole, UR.START, rows)
    gw, mw = whole.read()
    st = FT._stats(case, UR.START, rows)
    for part in (4, 5, 2):
        FT._launch(case, parts, UR.START, rows, part=part, stats=st)
    gp, mp = parts.read()
    assert _l2_is_zero(case.d, gw) and _l2_is_zero(case.d, gp)
    met_ref, ga_ref, gc_ref = FT._oracle(case, UR.START, rows)
    UR._check_metrics(mp / rows, met_ref, UR.TOL["bf16"], True, "plain-parts")
    UR._check_errs(UR._tensor_errs(case.d, gp, ga_ref, gc_ref), UR.TOL["bf16"], "plain-parts")
    diff = np.abs(gp - gw)
    print(json.dumps({"case": "plain parts vs whole", "median": float(np.median(diff)), "max": float(diff.max())}))
    assert np.median(diff) < 1e-6 and diff.max() < 5e-3
    for slot in (0, 1):
        assert abs(mp[slot] - mw[slot]) <= 1e-3 * (abs(mw[slot]) + 1e-3), (slot, mp[slot], mw[slot])


def test_ppo_minibatch_multichunk_dw_plain(cuda):
    """1,600 rows, fp32 (test_multichunk_dw_grads_match_oracle's size): two actor dW m-chunks on 32-row tiles,
    both adding u2^T dy into W_out's own gradient range."""
    from diffusionpolicyoptimization_amd import ops
    rows = 1600
    case = UR._Case(cuda, "fp32", HOPPER_PLAIN, 170)
    plan = ops.ppo_plan(case.d, "fp32", rows)
    assert plan["actor_tile_rows"] == 32 and plan["dw_chunks_actor"] == 2, plan
    _grads_vs_oracle(case, rows, "plain-multichunk")


@pytest.mark.parametrize("deferred", [False, True], ids=["whole", "l2def"])
def test_ppo_minibatch_tile64_plain(cuda, deferred):
    """64 (C - 1) + 1 rows, C the CU count, bf16 ReLU: the smallest row count at which ops.ppo_plan reports the
    64-row tile (asserted: 64 rows fewer give the 32-row tile) with more than one dW m-chunk
    (test_actor_tile64_grads_match_oracle's R1); also under DPPO_PPO_L2_DEFERRED."""
    from diffusionpolicyoptimization_amd import ops
    rows = 64 * (UR._cus(cuda) - 1) + 1
    case = UR._Case(cuda, "bf16", HOPPER_PLAIN, -(-(UR.START + rows) // 10) + 50)
    plan = ops.ppo_plan(case.d, "bf16", rows)
    assert plan["actor_tile_rows"] == 64 and plan["actor_waves"] == 16 and plan["dw_chunks_actor"] > 1, plan
    assert ops.ppo_plan(case.d, "bf16", rows - 64)["actor_tile_rows"] == 32
    _grads_vs_oracle(case, rows, f"plain-tile64{'-l2def' if deferred else ''}", l2_deferred=deferred)


@pytest.mark.parametrize("precision,rtol", [("fp32", 2e-3), ("bf16", 1e-2)])
def test_pretrain_matches_plain_oracle(cuda, precision, rtol):
    """dppo_pretrain_minibatch on a plain image at 40 rows: loss and every actor gradient against O.p_losses
    with the plain head (test_pretrain_loss_grads' bounds); the l2 range is exactly zero."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    d, _, ft, _, sched, tab, _, pf, _ = KG._setup(HOPPER_PLAIN, cuda)
    rng = np.random.default_rng(21)
    rows, K = 40, d.denoising_steps
    x0 = rng.uniform(-1, 1, (rows, d.xd)).astype(np.float32)
    cond = rng.uniform(-1, 1, (rows, d.sd)).astype(np.float32)
    t = rng.integers(0, K, rows).astype(np.int32)
    noise = rng.standard_normal((rows, d.xd)).astype(np.float32)
    sh = (rows, d.horizon_steps, d.action_dim)
    loss_ref, g_ref = O.p_losses(to_f64(ft), sched, x0.reshape(sh).astype(np.float64),
                                 cond.reshape(rows, d.cond_steps, d.obs_dim).astype(np.float64), t,
                                 noise.reshape(sh).astype(np.float64), rnd=KG._rnd(precision), model=O.Model.from_dims(d))
    T = lambda x: torch.tensor(x, device=cuda)
    grads = torch.full((ops.spec_count(ops.actor_param_spec(d)),), 7.0, dtype=torch.float32, device=cuda)
    metrics = torch.zeros(16, dtype=torch.float64, device=cuda)
    loss = ops.pretrain_minibatch(d, precision, ops.pack_actor(d, pf, precision), pf, tab, T(ops.q_sched_table(sched)),
                                  T(x0), T(cond), T(t), T(noise), ops.ppo_workspace(d, precision, rows, cuda), grads, metrics)
    torch.cuda.synchronize()
    flat = grads.cpu().numpy()
    ga = ops.unflatten_params(ops.actor_param_spec(d), flat)
    errs = {k: float(np.abs(ga[k] - r).max() / (np.abs(r).max() + 1e-12)) for k, r in g_ref.items()}
    print(json.dumps({"case": f"plain-pretrain-{precision}", "loss": float(loss), "loss_ref": float(loss_ref), "errs": errs}))
    assert "l2_w" not in g_ref and _l2_is_zero(d, flat)
    assert abs(float(loss) - loss_ref) < rtol * loss_ref
    bad = {k: v for k, v in errs.items() if not v < rtol}
    assert not bad, (bad, errs)


# ------------------------------------------------------------------------------------------------
# optimizer steps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("form", ["staged", "fused", "fused-clear"])
def test_optimizer_steps_keep_the_plain_image(cuda, precision, form):
    """Three AdamW steps of the actor range on nonzero gradients (l2 range zero, as every gradient entry
    writes it): after each step the image is byte-identical to a fresh plain pack of the updated parameters
    (after the deferred sampler tables are refreshed), which catches a step that revives T_OUT / ROUT / RT_FOLD0;
    the l2 parameter range stays exactly zero. Re-packing the buffer with dppo_pack_actor resets the head:
    its bytes then equal a fresh residual pack."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import ptr, stream_handle
    d, _, _, _, _, _, _, pf, _ = KG._setup(HOPPER_PLAIN, cuda)
    n = pf.numel()
    # zeroed buffers: the bytes no pack writes (segment alignment padding, the 2-byte FOLD / ROUT slots of an
    # fp32 image) then compare equal too
    zeros = lambda: torch.zeros(ops.actor_packed_bytes(d, precision), dtype=torch.uint8, device=cuda)
    img = ops.pack_actor(d, pf, precision, out=zeros())
    m, v = torch.zeros_like(pf), torch.zeros_like(pf)
    lo, hi = _l2_range(d)
    gen = torch.Generator(device=cuda).manual_seed(3)
    for step in (1, 2, 3):
        grads = torch.randn(n, device=cuda, generator=gen) * 0.01
        grads[lo:hi] = 0
        mode = ops._step_mode("keras", fused_pack=form != "staged", clear_grads=form == "fused-clear")
        _lib.call("dppo_optimizer_step_ex", ctypes.byref(d.c()), _lib.PRECISION[precision], ptr(pf), ptr(grads), ptr(m), ptr(v),
                  n, step, 1e-3, 0.004, 0.9, 0.999, 1e-7, mode, ptr(pf), ptr(img), None, None, None, None, 0, 0, None, None,
                  0, stream_handle(cuda))
        _lib.call("dppo_refresh_sampler_tables", ptr(img), stream_handle(cuda))
        torch.cuda.synchronize()
        fresh = ops.pack_actor(d, pf, precision, out=zeros())
        torch.cuda.synchronize()
        assert _l2_is_zero(d, pf.cpu().numpy()), step
        assert torch.equal(img, fresh), (form, precision, step, int((img != fresh).sum()))
        if form == "fused-clear":
            assert not grads.any()
    res = ops.ModelDims(**HOPPER)
    _lib.call("dppo_pack_actor", ctypes.byref(res.c()), _lib.PRECISION[precision], ptr(pf), ptr(img), stream_handle(cuda))
    torch.cuda.synchronize()
    assert torch.equal(img, ops.pack_actor(res, pf, precision, out=zeros())) and not torch.equal(img, fresh)


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_plain_refusals(cuda):
    """A plain actor is refused where a residual actor is, with the dispatch's message and untouched outputs
    (the sampler at actor_hidden 384 in bf16, dppo_logprob at actor_hidden 256 in fp32); a head outside the
    enum is DPPO_EINVAL at the pack; DPPO_STEP_L2_FROM_PL2 on a plain image is DPPO_EINVAL."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import DppoError, ptr, stream_handle
    dims = dict(HOPPER_PLAIN, actor_hidden=384)
    inp = SS._Inputs(dims, 17, seed=11)
    g = SS._Gpu(inp, "bf16", cuda)
    d, E = inp.d, 17
    actions = torch.full((E, d.xd), SS.SENTINEL, device=cuda)
    chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SS.SENTINEL, device=cuda)
    SS._rejected(lambda: ops.sample(d, "bf16", g.packb, g.packf, g.tab, g.T(inp.state.reshape(E, -1)),
                                    x_T=g.T(inp.xT.reshape(E, -1)), noise=g.T(inp.z.reshape(inp.K, E, -1)),
                                    actions=actions, chains=chains), (actions, chains), SS._msg_inst(d, "bf16"))
    dims = dict(HOPPER_PLAIN, actor_hidden=256)
    d, _, _, _, _, tab, _, pf, _ = KG._setup(dims, cuda)
    n, kf = 37, d.ft_denoising_steps
    lpe = torch.full((n * kf, d.xd), SS.SENTINEL, device=cuda)
    lpm = torch.full((n, kf), SS.SENTINEL, device=cuda)
    packf = ops.pack_actor(d, pf, "fp32")
    call = lambda: _lib.call("dppo_logprob", ctypes.byref(d.c()), _lib.PRECISION["fp32"], ptr(packf), ptr(tab),
                             ptr(torch.zeros(n, d.sd, device=cuda)), ptr(torch.zeros(n, kf + 1, d.xd, device=cuda)), n,
                             0.1, 4, ptr(lpe), ptr(lpm), stream_handle(cuda))
    US._rejected(call, (lpe, lpm), US._actor_msg({k: v for k, v in dims.items() if k != "head"}, "fp32"))
    with pytest.raises(DppoError, match=re.escape("failed (1): dppo_pack_actor_head: bad head 2")):
        _lib.call("dppo_pack_actor_head", ctypes.byref(d.c()), _lib.PRECISION["fp32"], 0, 2, ptr(pf), ptr(packf),
                  stream_handle(cuda))
    d, _, _, _, _, _, _, pf, _ = KG._setup(HOPPER_PLAIN, cuda)
    img = ops.pack_actor(d, pf, "bf16")
    before = pf.clone()
    z = torch.zeros_like(pf)
    with pytest.raises(DppoError, match=re.escape("failed (1): dppo_optimizer_step: DPPO_STEP_L2_FROM_PL2 on a plain-head")):
        _lib.call("dppo_optimizer_step", ctypes.byref(d.c()), _lib.PRECISION["bf16"], ptr(pf), ptr(z), ptr(z.clone()),
                  ptr(z.clone()), pf.numel(), 1, 1e-3, 0.004, 0.9, 0.999, 1e-7, ops._step_mode("keras", l2_from_pl2=True),
                  ptr(pf), ptr(img), None, None, None, None, 0, 0, stream_handle(cuda))
    torch.cuda.synchronize()
    assert torch.equal(pf, before)


SAMPLER_REFUSED = [(g, p) for g, p in SS.B_PARAMS if SS.expected(g, p)[3]]


@pytest.mark.parametrize("geometry,precision", SAMPLER_REFUSED, ids=["-".join(x) for x in SAMPLER_REFUSED])
def test_sampler_geometry_refusals_plain(cuda, geometry, precision):
    """Every refused line of the sampler's geometry table (tests/test_sampler_surface_gpu.py GEOMETRIES) with
    plain images: the unsupported-configuration error with the residual head's message, outputs untouched."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    dims, E, _, msg = SS.expected(geometry, precision)
    inp = SS._Inputs(dict(dims, **PLAIN), E, seed=11)
    g = SS._Gpu(inp, precision, cuda)
    d = inp.d
    actions = torch.full((E, d.xd), SS.SENTINEL, device=cuda)
    chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SS.SENTINEL, device=cuda)
    SS._rejected(lambda: ops.sample(d, precision, g.packb, g.packf, g.tab, g.T(inp.state.reshape(E, -1)),
                                    x_T=g.T(inp.xT.reshape(E, -1)), noise=g.T(inp.z.reshape(inp.K, E, -1)),
                                    actions=actions, chains=chains), (actions, chains), msg)


UPDATE_REFUSED = [(g, p) for g in US.GEOMETRIES for p in ("fp32", "bf16", "fp16") if US.expected_rejection(g, p, "logprob")]


@pytest.mark.parametrize("geometry,precision", UPDATE_REFUSED, ids=["-".join(x) for x in UPDATE_REFUSED])
def test_update_geometry_refusals_plain(cuda, geometry, precision):
    """Every line of the update's geometry table (tests/test_update_surface_gpu.py GEOMETRIES) that refuses the
    actor, with a plain image: dppo_logprob, dppo_ppo_minibatch and dppo_pretrain_minibatch give the
    unsupported-configuration error with the residual head's message and leave their outputs untouched."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    res_dims = US.GEOMETRIES[geometry][0]
    msg = US.expected_rejection(geometry, precision, "logprob")
    assert msg == US.expected_rejection(geometry, precision, "pretrain_minibatch") == US.expected_rejection(geometry, precision, "ppo_minibatch")
    d, _, _, _, sched, tab, _, pf, pc = KG._setup(dict(res_dims, **PLAIN), cuda)
    full = lambda *shape, dtype=torch.float32: torch.full(shape, US.SENTINEL, dtype=dtype, device=cuda)
    zeros = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=cuda)
    packf = ops.pack_actor(d, pf, precision)
    n, kf, rows = 37, d.ft_denoising_steps, 150
    lpe, lpm = full(n * kf, d.xd), full(n, kf)
    US._rejected(lambda: ops.logprob(d, precision, packf, tab, zeros(n, d.sd), zeros(n, kf + 1, d.xd), lp_elem=lpe, lp_mean=lpm),
                 (lpe, lpm), msg)
    na, nc = ops.spec_count(ops.actor_param_spec(d)), ops.spec_count(ops.critic_param_spec(d))
    grads, metrics = full(na + nc), full(16, dtype=torch.float64)
    N = 40
    US._rejected(lambda: ops.ppo_minibatch(d, precision, ops.ppo_hparams(global_rows=rows), packf, ops.pack_critic(d, pc, precision),
                                           pf, tab, zeros(N, d.sd), zeros(N, kf + 1, d.xd), zeros(N, kf), zeros(N), zeros(N),
                                           UR.SEED, UR.EPOCH, UR.START, rows, ops.ppo_workspace(d, precision, rows, cuda),
                                           grads, metrics), (grads, metrics), msg)
    ga, met = full(na), full(16, dtype=torch.float64)
    US._rejected(lambda: ops.pretrain_minibatch(d, precision, packf, pf, tab, torch.tensor(ops.q_sched_table(sched), device=cuda),
                                                zeros(rows, d.xd), zeros(rows, d.sd), zeros(rows, dtype=torch.int32),
                                                zeros(rows, d.xd), ops.ppo_workspace(d, precision, rows, cuda), ga, met),
                 (ga, met), msg)


# ------------------------------------------------------------------------------------------------
# agents
# ------------------------------------------------------------------------------------------------
def test_plain_iteration_matches_oracle(cuda, tmp_path, monkeypatch):
    """An eval and a training iteration of the fp32 agent from ft_ppo_diffusion_mlp_plain.yaml (seed 42, the
    shapes of tests/test_iteration_gpu.py) against oracle/iteration.py with the plain head, at that file's
    bounds: chains, rewards and returns of both; values, old log-probs, advantages, returns, the last
    minibatch's losses, the number of applied minibatches and the parameter change of the training one. The
    oracle's flat parameters are the plain spec's tensors back to back; the agent's are gathered from the
    residual layout, whose l2 range must still be exactly zero."""
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util import config
    from tests import test_iteration_gpu as IT
    load = config.load_config
    monkeypatch.setattr(config, "load_config", lambda root, name, ov: load(root, name + "_plain", ov))
    a, orc = IT._agent_and_oracle(42, tmp_path)
    m = a.model
    assert m.dims.head == "plain" and "l2_w" not in dict(m.actor_spec)
    idx = np.concatenate([np.arange(o, o + k) for _, _, o, k in ops.spec_ranges(m.actor_spec)] +
                         [m.n_actor + np.arange(ops.spec_count(m.critic_spec))])
    assert idx.size == orc.theta.size
    compact = lambda: m.train_params.cpu().numpy().astype(np.float64)[idx]
    np.testing.assert_array_equal(compact(), orc.theta)
    for it in range(2):
        p0, th0, n0 = compact(), orc.theta.copy(), a.timing["n_updates"]
        res, ref = a.iteration(), orc.iteration()
        assert res["eval"] == ref["eval"] == (it == 0)
        np.testing.assert_array_equal(a.firsts, ref["firsts"])
        S, E = a.n_steps, a.n_envs
        e = {"itr": it, "chains_abs": float(np.abs(a.chains_traj.cpu().numpy().reshape(ref["chains"].shape) - ref["chains"]).max()),
             "rewards_rel": IT._rel(a.reward_pin.numpy(), ref["rewards"])}
        ep = ref["episodes"]
        assert res["num_episode_finished"] == ep["num_episode_finished"] > 0
        e["return_rel"] = abs(res["avg_episode_reward"] - ep["avg_episode_reward"]) / abs(ep["avg_episode_reward"])
        if it == 1:
            e["values_abs"] = float(np.abs(a.values.cpu().numpy().reshape(S, E) - ref["values"]).max())
            e["lp_old_abs"] = float(np.abs(a.lp_old.cpu().numpy() - ref["lp_old"]).max())
            e["adv_rel"], e["ret_rel"] = IT._rel(a.adv.cpu().numpy(), ref["adv"]), IT._rel(a.ret.cpu().numpy(), ref["ret"])
            last = ref["metrics"][-1]
            e["n_updates"] = (a.timing["n_updates"] - n0, len(ref["metrics"]))
            e["losses"] = [(float(res[k]), float(last[k])) for k in ("pg_loss", "v_loss")]
            dg, dr = compact() - p0, orc.theta - th0
            diff, scale = np.abs(dg - dr), np.abs(dr).max()
            e["param_delta"] = dict(median=float(np.median(diff) / scale), p99=float(np.quantile(diff, 0.99) / scale),
                                    max=float(diff.max() / scale), l2=float(np.linalg.norm(dg - dr) / np.linalg.norm(dr)))
        print(json.dumps({"case": "plain-iteration", **e}))
        assert e["chains_abs"] <= 2e-5 and e["rewards_rel"] <= 1e-5 and e["return_rel"] <= 1e-5, e
        if it == 1:
            assert e["n_updates"][0] == e["n_updates"][1] > 0 and scale > 0, e
            assert e["values_abs"] <= 1e-4 and e["lp_old_abs"] <= 1e-4 and e["adv_rel"] <= 1e-4 and e["ret_rel"] <= 1e-4, e
            assert abs(res["v_loss"] - last["v_loss"]) <= 1e-3 * abs(last["v_loss"]) + 1e-7, e
            assert abs(res["pg_loss"] - last["pg_loss"]) <= 1e-3 * abs(last["pg_loss"]) + 1e-6, e
            pd = e["param_delta"]
            assert pd["median"] <= 1e-4 and pd["p99"] <= 1e-3 and pd["l2"] <= 5e-3 and pd["max"] <= 0.1, e
        assert _l2_is_zero(m.dims, m.train_params.cpu().numpy()[:m.n_actor])


def test_plain_agent_split_update_matches_fused(cuda, tmp_path, monkeypatch):
    """TrainPPODiffusionAgent from ft_ppo_diffusion_mlp_plain.yaml on the synthetic env, two iterations through
    the fused and through the split update: finite, moved parameters that agree within
    test_mish_agent_split_update_matches_fused's bounds; the l2 range is still exactly zero."""
    import torch
    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("DPPO_SPLIT_UPDATE", flag)
        cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp_plain",
                          ["model.precision=fp32", "train.n_steps=20", "train.batch_size=200", "train.n_train_itr=2",
                           "train.val_freq=100", f"logdir={tmp_path}/{flag}"])
        a = get_class(cfg._target_)(cfg)
        assert a.model.dims.head == "plain" and "l2_w" not in dict(a.model.actor_spec)
        p_init = a.model.train_params.cpu().numpy().copy()
        res = a.run()
        torch.cuda.synchronize()
        out[flag] = (a.model.train_params.cpu().numpy().copy(), res[-1], a.timing["n_updates"])
        assert np.isfinite(out[flag][0]).all() and np.abs(out[flag][0] - p_init).max() > 0
        assert _l2_is_zero(a.model.dims, out[flag][0][:a.model.n_actor])
    (p1, r1, n1), (p0, r0, n0) = out["1"], out["0"]
    assert n1 == n0
    dlt = np.abs(p1 - p0)
    print(json.dumps({"case": "plain-agent split vs fused", "median": float(np.median(dlt)), "max": float(dlt.max())}))
    assert np.median(dlt) < 1e-6 and dlt.max() < 5e-3, (float(np.median(dlt)), float(dlt.max()))
    for k in ("pg_loss", "v_loss"):
        assert abs(r1[k] - r0[k]) <= 1e-3 * (abs(r0[k]) + 1e-3), (k, r1[k], r0[k])


def test_plain_pretrain_agent_loss_falls(cuda, tmp_path):
    """TrainDiffusionAgent from pre_diffusion_mlp_plain.yaml on a synthetic dataset: the loss on a fixed batch
    is lower after one epoch; its .npz checkpoint holds no l2, loads back bit for bit, and DiffusionModel /
    PPODiffusion refuse a file of the other head on loading (both ways round)."""
    import torch
    from diffusionpolicyoptimization_amd.agent.dataset.sequence import synthetic_dataset
    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    data = synthetic_dataset(str(tmp_path / "train.npz"), n_episodes=6, episode_len=160, seed=1)
    cfg = load_config(os.path.join(ROOT, "cfg/gym/pretrain/hopper-medium-v2"), "pre_diffusion_mlp_plain",
                      [f"train_dataset_path={data}", f"logdir={tmp_path}/log", "train.n_epochs=1", "train.batch_size=256",
                       "train.learning_rate=1e-3"])
    agent = get_class(cfg._target_)(cfg)
    assert agent.model.network.head == "plain"
    b = next(agent.dataset_train.batches(512))
    t = torch.randint(0, 20, (512,), device=cuda, dtype=torch.int32)
    z = torch.randn(512, 12, device=cuda)
    first = float(agent.model.p_losses(b["actions"], b["conditions"], t, z))
    assert agent.model.pre_dims.head == "plain"
    last_epoch = agent.run()
    last = float(agent.model.p_losses(b["actions"], b["conditions"], t, z))
    print(json.dumps({"case": "plain-pretrain-agent", "first": first, "last": last}))
    assert np.isfinite(last_epoch) and last < first, (first, last)
    ck = str(tmp_path / "net.npz")
    agent.model.save_network(ck)
    with np.load(ck) as f:
        assert not any("l2" in k for k in f.files) and "network.out_w" in f.files
    # the call sites: the plain file into residual models (pretrain and fine-tune), a residual file into plain ones
    pre_res = load_config(os.path.join(ROOT, "cfg/gym/pretrain/hopper-medium-v2"), "pre_diffusion_mlp",
                          [f"train_dataset_path={data}", f"logdir={tmp_path}/log2"])
    ft_dir = os.path.join(ROOT, "cfg/gym/finetune/hopper-v2")
    from diffusionpolicyoptimization_amd.util.config import instantiate
    with pytest.raises(ValueError, match="holds a plain"):
        instantiate(pre_res.model, device=cuda, seed=1, network_path=ck)._pretrain_init()   # loads on first use
    with pytest.raises(ValueError, match="holds a plain"):
        instantiate(load_config(ft_dir, "ft_ppo_diffusion_mlp", []).model, device=cuda, seed=1, network_path=ck)
    res = instantiate(pre_res.model, device=cuda, seed=1)
    res._pretrain_init()
    ck_res = str(tmp_path / "net_res.npz")
    res.save_network(ck_res)
    with pytest.raises(ValueError, match="holds a residual"):
        instantiate(cfg.model, device=cuda, seed=1, network_path=ck_res)._pretrain_init()
    with pytest.raises(ValueError, match="holds a residual"):
        instantiate(load_config(ft_dir, "ft_ppo_diffusion_mlp_plain", []).model, device=cuda, seed=1, network_path=ck_res)
    same = instantiate(cfg.model, device=cuda, seed=1, network_path=ck)
    same._pretrain_init()
    assert torch.equal(same.params, agent.model.params)
