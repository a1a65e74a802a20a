"""Mish actor on the GPU: every entry that takes a packed actor image, against the oracle's Mish actor
(O.Model(act="Mish"), derived from the dims).

Bounds are the ReLU cases' of the same entry and path, unchanged: the sampler's of
tests/test_sampler_surface_gpu.py (fp32 2e-4 absolute on actions and chains; 2-byte q99 / means 2e-3
bf16, 1e-3 fp16), test_logprob's (q99 of |d| / (1 + |ref|) 1e-3 fp32, 2e-3 2-byte; the row mean ten
times that), test_ppo_minibatch_grads' / test_pretrain_loss_grads' per tensor (2e-3 fp32, 1e-2 2-byte),
test_split_update_matches_fused's for the agent. The critic's Mish bounds (test_critic_forward fp32
1e-4 (1 + max|ref|), its gradients 2e-3) are no looser at these magnitudes. Every figure is printed
as a JSON line before it is asserted.

Problems and device halves are the surface tests' (_Inputs / _Gpu of test_sampler_surface_gpu, _Problem
/ _Gpu of test_update_surface_gpu, _Case of test_update_regimes_gpu) with `activation="Mish"` in the
dims, so ops.pack_actor records Mish with every image. The update problems take N(0, 1) biases
(mish_models), asserted on the oracle's cache to put >= 5 % of h1 and of h2 below -1 (mish' < 0 there)
and >= 20 % above 0.

Refusals: a Mish actor is refused on the same lines as a ReLU one with the same messages
(include/dppo.h); test_mish_refusals pins one sampler line and one update line, and the two EINVAL
rules of the attribute (mixed images, an activation outside the enum)."""
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
from tests.helpers import HOPPER, HOPPER_DDIM, WALKER, to_f64
from tests.variants import HOPPER_MISH, MISH, WALKER_MISH, mish_models, site_coverage

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOPPER_DDIM_MISH = dict(HOPPER_DDIM, **MISH)
SPLIT, STREAM = 2, 0


# ------------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------------
# (label, dims, precision, envs, kernel, oracle / launch keywords, eta)
SAMPLER_CASES = [
    ("hopper-fp32-E17", HOPPER_MISH, "fp32", 17, SPLIT, {}, 1.0),          # split, P = 8 form
    ("hopper-bf16-E17", HOPPER_MISH, "bf16", 17, SPLIT, {}, 1.0),          # split, KX = 1 form
    ("hopper-fp16-E17", HOPPER_MISH, "fp16", 17, SPLIT, {}, 1.0),
    ("walker-bf16-E17", WALKER_MISH, "bf16", 17, SPLIT, {}, 1.0),          # split, KX = 2 form
    ("walker-fp32-E17", WALKER_MISH, "fp32", 17, STREAM, {}, 1.0),         # streaming, fp32
    ("hopper-bf16-E513", HOPPER_MISH, "bf16", 513, STREAM, {}, 1.0),       # streaming, 2-byte
    ("hopper-bf16-E17-eval", HOPPER_MISH, "bf16", 17, SPLIT, dict(deterministic=True), 1.0),
    ("hopper-fp16-E17-ddim", HOPPER_DDIM_MISH, "fp16", 17, SPLIT, {}, 1.0),
]


@pytest.mark.parametrize("label,dims,precision,E,kernel,kw,eta", SAMPLER_CASES, ids=[c[0] for c in SAMPLER_CASES])
def test_sampler_matches_mish_oracle(cuda, label, dims, precision, E, kernel, kw, eta):
    """dppo_sample on Mish images, injected noise, against O.sample with the Mish actor: actions and every
    stored chain row; the plan is the ReLU plan of the same shape."""
    from diffusionpolicyoptimization_amd import ops
    inp = SS._Inputs(dims, E, seed=11, eta=eta)
    g = SS._Gpu(inp, precision, cuda)
    relu_dims = {k: v for k, v in dims.items() if k != "activation"}
    assert g.plan["kernel"] == kernel and g.plan == ops.sampler_plan(ops.ModelDims(**relu_dims), precision, E), g.plan
    act, ch = g.twice(**kw)
    SS._check(f"mish {label}", precision, SS._stats(act, ch, *inp.oracle(precision, **kw)), plan=g.plan)


def _einval(call, outputs, msg):
    """call() raises DPPO_EINVAL (code 1) with the message and leaves the sentinel-filled outputs."""
    import torch
    from diffusionpolicyoptimization_amd._lib import DppoError
    with pytest.raises(DppoError, match=re.escape(f"failed (1): {msg}")):
        call()
    torch.cuda.synchronize()
    for o in outputs:
        assert bool((o == SS.SENTINEL).all()), "a refused call wrote its outputs"


@pytest.mark.parametrize("precision,E", [("bf16", 17), ("bf16", 513), ("fp32", 17)])
def test_sampler_refuses_mixed_images(cuda, precision, E):
    """A ReLU base image with a Mish fine-tuned image (and the reverse): DPPO_EINVAL before anything is
    enqueued, outputs left at the sentinel; the next accepted launch on the stream is unaffected."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    inp = SS._Inputs(HOPPER_MISH, E, seed=11)
    g = SS._Gpu(inp, precision, cuda)
    d = inp.d
    relu = ops.ModelDims(**HOPPER)
    _, _, _, _, _, _, pb, pf, _ = KG._setup(HOPPER, cuda)
    for base, ft in ((ops.pack_actor(relu, pb, precision), g.packf), (g.packb, ops.pack_actor(relu, pf, precision))):
        actions = torch.full((E, d.xd), SS.SENTINEL, device=cuda)
        chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SS.SENTINEL, device=cuda)
        call = lambda: ops.sample(d, precision, base, ft, g.tab, g.T(inp.state.reshape(E, -1)),
                                  x_T=g.T(inp.xT.reshape(E, -1)), noise=g.T(inp.z.reshape(inp.K, E, -1)),
                                  actions=actions, chains=chains)
        _einval(call, (actions, chains), "dppo_sample: the base and the fine-tuned actor images carry different activations")
    g.sample()


def test_attribute_follows_the_image(cuda):
    """A buffer packed with Mish samples as Mish; re-packed in place by plain dppo_pack_actor it samples
    as a fresh ReLU image does, bit for bit (and differs from its Mish result)."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import ptr, stream_handle
    inp = SS._Inputs(HOPPER_MISH, 17, seed=11)
    g = SS._Gpu(inp, "bf16", cuda)
    a_mish, c_mish = g.sample()
    SS._check("attribute: mish", "bf16", SS._stats(a_mish, c_mish, *inp.oracle("bf16")))
    relu = ops.ModelDims(**HOPPER)
    _, _, _, _, _, _, pb, pf, _ = KG._setup(HOPPER, cuda)
    for params, img in ((pb, g.packb), (pf, g.packf)):      # the C entry itself, in place
        _lib.call("dppo_pack_actor", ctypes.byref(relu.c()), _lib.PRECISION["bf16"], ptr(params), ptr(img),
                  stream_handle(params.device))
    a_again, c_again = g.sample()
    fresh = SS._Gpu(SS._Inputs(HOPPER, 17, seed=11), "bf16", cuda)
    a_relu, c_relu = fresh.sample()
    assert a_again.tobytes() == a_relu.tobytes() and c_again.tobytes() == c_relu.tobytes()
    assert a_again.tobytes() != a_mish.tobytes()
    # and that is the ReLU oracle's result
    SS._check("attribute: relu after re-pack", "bf16", SS._stats(a_again, c_again, *fresh.inp.oracle("bf16")))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# dppo_logprob
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16", 2e-3)])
@pytest.mark.parametrize("n", [48, 45])
def test_logprob_matches_mish_oracle(cuda, monkeypatch, precision, tol, n):
    """dppo_logprob on a Mish image: 48 samples x K' = 10 = fifteen 32-row tiles, 45 a partial last tile;
    lp_elem and lp_mean against O.get_logprobs with the Mish actor (test_logprob's measures and bounds)."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    monkeypatch.setattr(KG, "make_models", mish_models)
    d, _, ft, _, sched, tab, _, pf, _ = KG._setup(HOPPER_MISH, cuda)
    kf = d.ft_denoising_steps
    rng = np.random.default_rng(4)
    state = rng.uniform(-1, 1, (n, 1, d.obs_dim)).astype(np.float32)
    chains = (rng.standard_normal((n, kf + 1, d.horizon_steps, d.action_dim)) * 0.5).astype(np.float32)
    caches = []
    ref = O.get_logprobs(to_f64(ft), sched, state.astype(np.float64), chains.astype(np.float64), kf, rnd=KG._rnd(precision),
                         model=O.Model.from_dims(d), caches=caches)
    cov = site_coverage(caches[-1])
    assert ops.ppo_plan(d, precision, n * kf, mode="logprob")["actor_tile_rows"] == 32
    lpe, lpm = ops.logprob(d, precision, ops.pack_actor(d, pf, precision), tab,
                           torch.tensor(state.reshape(n, -1), device=cuda),
                           torch.tensor(chains.reshape(n, kf + 1, -1), device=cuda))
    torch.cuda.synchronize()
    lpe = lpe.cpu().numpy().reshape(ref.shape)
    ref_mean = np.clip(ref, -5, 2).mean(axis=(1, 2)).reshape(n, kf)
    q99 = float(np.quantile(np.abs(lpe - ref) / (1 + np.abs(ref)), 0.99))
    mean_err = float(np.abs(lpm.cpu().numpy() - ref_mean).max())
    print(json.dumps({"case": f"mish-logprob-{precision}-n{n}", "q99": q99, "bound": tol, "mean_err": mean_err,
                      "mean_bound": tol * 10, "coverage": cov}))
    assert q99 < tol and mean_err < tol * 10


# ------------------------------------------------------------------------------------------------
# dppo_ppo_minibatch / dppo_pretrain_minibatch
# ------------------------------------------------------------------------------------------------
GRAD_CASES = [("hopper", HOPPER_MISH, "fp32"), ("hopper", HOPPER_MISH, "bf16"), ("hopper", HOPPER_MISH, "fp16"),
              ("walker", WALKER_MISH, "bf16")]


@pytest.mark.parametrize("name,dims,precision", GRAD_CASES, ids=[f"{n}-{p}" for n, _, p in GRAD_CASES])
def test_ppo_minibatch_grads_match_mish_oracle(cuda, monkeypatch, name, dims, precision):
    """dppo_ppo_minibatch on a Mish image at the surface tests' NSAMP / ROWS: the loss metrics and every
    gradient tensor against O.c_loss with the Mish actor; h1 and h2 cover x < -1 and x > 0."""
    monkeypatch.setattr(US, "make_models", mish_models)
    p = US._Problem(dims, precision)
    caches = []
    ref = p.oracle(caches=caches)
    cov = site_coverage(caches[-1])
    gpu = US._Gpu(p, cuda)
    from diffusionpolicyoptimization_amd import ops
    plan = ops.ppo_plan(p.d, precision, US.ROWS)
    assert (plan["actor_tile_rows"], plan["actor_waves"]) == (32, 8), plan
    m, g = gpu.minibatch()
    print(json.dumps({"case": f"mish-grads-{name}-{precision}", "coverage": cov}))
    US._compare(f"mish-{name}-{precision}", gpu, m, g, ref, US.TOL[precision])


def test_ppo_minibatch_learn_eta_ddim_mish(cuda, monkeypatch):
    """DPPO_PPO_LEARN_ETA behind a Mish forward (hopper DDIM, bf16, eta 0.6): metrics[8] and every
    gradient tensor against the oracle (the 64-row tile test's d_eta bound, 3e-2 relative)."""
    monkeypatch.setattr(KG, "make_models", mish_models)
    rows = US.ROWS
    case = UR._Case(cuda, "bf16", HOPPER_DDIM_MISH, US.NSAMP, eta=0.6)
    stats, mean_std = case.adv_stats(rows)
    caches = []
    met_ref, ga_ref, gc_ref = case.oracle(rows, adv_mean_std=mean_std, eta_grad=True, caches=caches)
    cov = site_coverage(caches[-1])
    g, m = case.launch(rows, UR.START, rows, stats=stats, learn_eta=True)
    ref = met_ref["d_eta"]
    print(json.dumps({"case": "mish-learn-eta", "d_eta": float(m[8]), "ref": ref, "coverage": cov}))
    UR._check_metrics(m / rows, met_ref, UR.TOL["bf16"], True, "mish-learn-eta")
    assert abs(ref) > 1e-3 and abs(m[8] - ref) <= 3e-2 * abs(ref), (m[8], ref)
    UR._check_errs(UR._tensor_errs(case.d, g, ga_ref, gc_ref), UR.TOL["bf16"], "mish-learn-eta")


@pytest.mark.parametrize("precision,rtol", [("fp32", 2e-3), ("bf16", 1e-2)])
def test_pretrain_matches_mish_oracle(cuda, monkeypatch, precision, rtol):
    """dppo_pretrain_minibatch on a Mish image: loss and every actor gradient against O.p_losses with
    the Mish actor (test_pretrain_loss_grads' shapes and bounds)."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    monkeypatch.setattr(KG, "make_models", mish_models)
    d, _, ft, _, sched, tab, _, pf, _ = KG._setup(HOPPER_MISH, cuda)
    rng = np.random.default_rng(21)
    rows, K = 150, d.denoising_steps
    x0 = rng.uniform(-1, 1, (rows, d.xd)).astype(np.float32)
    cond = rng.uniform(-1, 1, (rows, d.sd)).astype(np.float32)
    t = rng.integers(0, K, rows).astype(np.int32)
    noise = rng.standard_normal((rows, d.xd)).astype(np.float32)
    sh = (rows, d.horizon_steps, d.action_dim)
    caches = []
    loss_ref, g_ref = O.p_losses(to_f64(ft), sched, x0.reshape(sh).astype(np.float64),
                                 cond.reshape(rows, d.cond_steps, d.obs_dim).astype(np.float64), t,
                                 noise.reshape(sh).astype(np.float64), rnd=KG._rnd(precision), model=O.Model.from_dims(d),
                                 caches=caches)
    cov = site_coverage(caches[-1])
    T = lambda x: torch.tensor(x, device=cuda)
    grads = torch.zeros(ops.spec_count(ops.actor_param_spec(d)), dtype=torch.float32, device=cuda)
    metrics = torch.zeros(16, dtype=torch.float64, device=cuda)
    loss = ops.pretrain_minibatch(d, precision, ops.pack_actor(d, pf, precision), pf, tab, T(ops.q_sched_table(sched)),
                                  T(x0), T(cond), T(t), T(noise), ops.ppo_workspace(d, precision, rows, cuda), grads, metrics)
    torch.cuda.synchronize()
    ga = ops.unflatten_params(ops.actor_param_spec(d), grads.cpu().numpy())
    errs = {k: float(np.abs(ga[k] - r).max() / (np.abs(r).max() + 1e-12)) for k, r in g_ref.items()}
    print(json.dumps({"case": f"mish-pretrain-{precision}", "loss": float(loss), "loss_ref": float(loss_ref), "errs": errs,
                      "coverage": cov}))
    assert abs(float(loss) - loss_ref) < rtol * loss_ref
    bad = {k: v for k, v in errs.items() if not v < rtol}
    assert not bad, (bad, errs)


def test_large_minibatch_runs_the_32_row_tile(cuda, monkeypatch):
    """One round of 64-row tiles for a ReLU actor (64 (C - 1) + 1 rows, C the CU count: the smallest size
    of test_actor_tile64_grads_match_oracle), bf16 TRAIN with a Mish actor: the 64-row tile is not
    instantiated for Mish, ops.ppo_plan says 32 rows on 8 waves, and every gradient tensor matches the
    oracle at the regime tests' bound."""
    from diffusionpolicyoptimization_amd import ops
    monkeypatch.setattr(KG, "make_models", mish_models)
    C = UR._cus(cuda)
    rows = 64 * (C - 1) + 1
    case = UR._Case(cuda, "bf16", HOPPER_MISH, -(-(UR.START + rows) // 10) + 50)
    plan = ops.ppo_plan(case.d, "bf16", rows)
    assert ops.ppo_plan(ops.ModelDims(**HOPPER), "bf16", rows)["actor_tile_rows"] == 64
    assert (plan["actor_tile_rows"], plan["actor_waves"]) == (32, 8) and plan["dw_chunks_actor"] > 1, plan
    stats, mean_std = case.adv_stats(rows)
    caches = []
    met_ref, ga_ref, gc_ref = case.oracle(rows, adv_mean_std=mean_std, caches=caches)
    cov = site_coverage(caches[-1])
    g, m = case.launch(rows, UR.START, rows, stats=stats)
    print(json.dumps({"case": "mish-large-minibatch", "rows": rows, "plan": plan, "coverage": cov}))
    assert np.isfinite(g).all()
    UR._check_metrics(m / rows, met_ref, UR.TOL["bf16"], True, "mish-large")
    UR._check_errs(UR._tensor_errs(case.d, g, ga_ref, gc_ref), UR.TOL["bf16"], "mish-large")


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_mish_refusals(cuda):
    """A Mish actor is refused where a ReLU actor is, with the dispatch's message and untouched outputs:
    the sampler at actor_hidden 384 (bf16) and dppo_logprob at actor_hidden 256 in fp32; and an
    activation outside the enum is DPPO_EINVAL at the pack, which records nothing."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import DppoError, ptr, stream_handle
    dims = dict(HOPPER_MISH, actor_hidden=384)
    inp = SS._Inputs(dims, 17, seed=11)
    g = SS._Gpu(inp, "bf16", cuda)
    d, E = inp.d, 17
    actions = torch.full((E, d.xd), SS.SENTINEL, device=cuda)
    chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SS.SENTINEL, device=cuda)
    SS._rejected(lambda: ops.sample(d, "bf16", g.packb, g.packf, g.tab, g.T(inp.state.reshape(E, -1)),
                                    x_T=g.T(inp.xT.reshape(E, -1)), noise=g.T(inp.z.reshape(inp.K, E, -1)),
                                    actions=actions, chains=chains), (actions, chains), SS._msg_inst(d, "bf16"))
    dims = dict(HOPPER_MISH, actor_hidden=256)
    d, _, _, _, _, tab, _, pf, _ = KG._setup(dims, cuda)
    n, kf = 37, d.ft_denoising_steps
    lpe = torch.full((n * kf, d.xd), SS.SENTINEL, device=cuda)
    lpm = torch.full((n, kf), SS.SENTINEL, device=cuda)
    packf = ops.pack_actor(d, pf, "fp32")
    call = lambda: _lib.call("dppo_logprob", ctypes.byref(d.c()), _lib.PRECISION["fp32"], ptr(packf), ptr(tab),
                             ptr(torch.zeros(n, d.sd, device=cuda)), ptr(torch.zeros(n, kf + 1, d.xd, device=cuda)), n,
                             0.1, 4, ptr(lpe), ptr(lpm), stream_handle(cuda))
    US._rejected(call, (lpe, lpm), US._actor_msg(dims, "fp32"))
    with pytest.raises(DppoError, match=re.escape("failed (1): dppo_pack_actor_act: bad activation 2")):
        _lib.call("dppo_pack_actor_act", ctypes.byref(d.c()), _lib.PRECISION["fp32"], 2, ptr(pf), ptr(packf),
                  stream_handle(cuda))


# ------------------------------------------------------------------------------------------------
# agents
# ------------------------------------------------------------------------------------------------
def test_model_call_matches_mish_oracle(cuda, tmp_path):
    """The model built from ft_ppo_diffusion_mlp_mish.yaml: model(cond) on injected draws equals the Mish
    oracle's sample (fp32, the sampler's bound)."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util.config import instantiate, load_config
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp_mish",
                      ["model.precision=fp32", f"logdir={tmp_path}"])
    m = instantiate(cfg.model)
    d = m.dims
    assert d.activation == "Mish" and m.actor.activation_type == "Mish"
    E, K = 17, d.denoising_steps
    rng = np.random.default_rng(3)
    state = rng.uniform(-1, 1, (E, d.cond_steps, d.obs_dim)).astype(np.float32)
    xT = rng.standard_normal((E, d.horizon_steps, d.action_dim)).astype(np.float32)
    z = rng.standard_normal((K, E, d.horizon_steps, d.action_dim)).astype(np.float32)
    T = lambda x: torch.tensor(x, device=cuda)
    act, ch = m(T(state), x_T=T(xT.reshape(E, -1)), noise=T(z.reshape(K, E, -1)))
    torch.cuda.synchronize()
    un = lambda flat, spec: to_f64(ops.unflatten_params(spec, flat.cpu().numpy()))
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    ref_a, ref_c = O.sample(un(m.base_params, m.actor_spec), un(m.actor_ft_params, m.actor_spec), ddpm_buffers(K),
                            state.astype(np.float64), xT, z, d.ft_denoising_steps,
                            min_std=m.get_min_sampling_denoising_std(), randn_clip=m.randn_clip_value, round_h3=False,
                            model=O.Model.from_dims(d))
    st = SS._stats(act.cpu().numpy().reshape(ref_a.shape), ch.cpu().numpy().reshape(ref_c.shape), ref_a, ref_c)
    SS._check("mish model(cond)", "fp32", st)


def test_mish_agent_split_update_matches_fused(cuda, tmp_path, monkeypatch):
    """TrainPPODiffusionAgent from ft_ppo_diffusion_mlp_mish.yaml on the synthetic env, two iterations
    through the fused and through the split update: finite, moved parameters that agree within
    test_split_update_matches_fused's bounds."""
    import torch
    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("DPPO_SPLIT_UPDATE", flag)
        cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp_mish",
                          ["model.precision=fp32", "train.n_steps=20", "train.batch_size=200", "train.n_train_itr=2",
                           "train.val_freq=100", f"logdir={tmp_path}/{flag}"])
        a = get_class(cfg._target_)(cfg)
        assert a.model.dims.activation == "Mish"
        p_init = a.model.train_params.cpu().numpy().copy()
        res = a.run()
        torch.cuda.synchronize()
        out[flag] = (a.model.train_params.cpu().numpy().copy(), res[-1], a.timing["n_updates"])
        assert np.isfinite(out[flag][0]).all() and np.abs(out[flag][0] - p_init).max() > 0
    (p1, r1, n1), (p0, r0, n0) = out["1"], out["0"]
    assert n1 == n0
    dlt = np.abs(p1 - p0)
    print(json.dumps({"case": "mish-agent split vs fused", "median": float(np.median(dlt)), "max": float(dlt.max())}))
    assert np.median(dlt) < 1e-6 and dlt.max() < 5e-3, (float(np.median(dlt)), float(dlt.max()))
    for k in ("pg_loss", "v_loss"):
        assert abs(r1[k] - r0[k]) <= 1e-3 * (abs(r0[k]) + 1e-3), (k, r1[k], r0[k])


def test_mish_pretrain_agent_loss_falls(cuda, tmp_path):
    """TrainDiffusionAgent from pre_diffusion_mlp_mish.yaml on a synthetic dataset: the loss on a fixed
    batch is lower after one epoch."""
    import torch
    from diffusionpolicyoptimization_amd.agent.dataset.sequence import synthetic_dataset
    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    data = synthetic_dataset(str(tmp_path / "train.npz"), n_episodes=6, episode_len=160, seed=1)
    cfg = load_config(os.path.join(ROOT, "cfg/gym/pretrain/hopper-medium-v2"), "pre_diffusion_mlp_mish",
                      [f"train_dataset_path={data}", f"logdir={tmp_path}/log", "train.n_epochs=1", "train.batch_size=256",
                       "train.learning_rate=1e-3"])
    agent = get_class(cfg._target_)(cfg)
    assert agent.model.network.activation_type == "Mish"
    b = next(agent.dataset_train.batches(512))
    t = torch.randint(0, 20, (512,), device=cuda, dtype=torch.int32)
    z = torch.randn(512, 12, device=cuda)
    first = float(agent.model.p_losses(b["actions"], b["conditions"], t, z))
    assert agent.model.pre_dims.activation == "Mish"
    last_epoch = agent.run()
    last = float(agent.model.p_losses(b["actions"], b["conditions"], t, z))
    print(json.dumps({"case": "mish-pretrain-agent", "first": first, "last": last}))
    assert np.isfinite(last_epoch) and last < first, (first, last)
