"""denoised_clip_value in {0.5, 2.0, None} and predict_epsilon=False on the GPU: every entry that takes a schedule
table, against the float64 oracle on a schedule that carries the same setting (O.with_param).

Hopper's geometry throughout (obs 11, action 3, horizon 4, hidden 512, K = 20, K' = 10). Each comparison uses the
bound of the existing case it mirrors, taken from that case's helper: the sampler's SS._check / SS.TOL
(tests/test_sampler_surface_gpu.py), the update's UR.TOL / UR._check_errs / UR._check_metrics
(tests/test_update_regimes_gpu.py), the pretraining step's PT._check / C.BOUND (tests/test_pretrain_step_gpu.py);
dppo_logprob's are test_logprob's parametrize literals (tests/test_kernels_gpu.py: fp32 1e-3, bf16 2e-3 on the
q99 of |lp - ref| / (1 + |ref|), ten times that on the clipped means), which no helper exports. Every figure is
printed as a JSON line before it is asserted. tests/test_diffusion_param_cpu.py shows on the same inputs that each
setting moves every compared quantity by ten bounds and more, and that no x_recon sits on a clip edge.

The sampler cases without the clip run the same seeded models reshaped to behave like a denoiser
(tests/variants.py denoiser_like: eps = alpha x + 2^-10 of the seeded network's own output): the sampler surface's
bounds are absolute and presuppose chains of order 1, which only the clip gives a seeded, untrained network (its
unclipped chains reach 4.7e3, where the fp32 bound of 2e-4 is below half an ulp of the compared values). Bounds, cases
and reference are unchanged. Measured on an MI355X without the clip, error / bound: fp32 max 3.5e-6 / 2e-4; bf16
actions q99 6.4e-4 / 2e-3, max 1.3e-3 / 0.1, chain mean 6.1e-5 / 2e-3; fp16 q99 1.8e-4 / 1e-3, chain mean 3.2e-5 / 1e-3.
Under that reshaping an error of the MLP path reaches the compared values through the factor 2^-10, so the seeded
networks without the clip are compared as well, at their own scale (test_sampler_noclip_seeded_scale)."""
import ctypes
import gc
import json
import os
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import variants as PO
from tests import pretrain_cases as C
from tests import test_kernels_gpu as KG
from tests import test_pretrain_step_gpu as PT
from tests import test_sampler_surface_gpu as SS
from tests import test_update_regimes_gpu as UR
from tests import test_update_surface_gpu as US
from tests.helpers import HOPPER, HOPPER_DDIM, to_f64
from tests.variants import HOPPER_MISH, HOPPER_PLAIN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT, STREAM = 2, 0
LOGPROB_TOL = {"fp32": 1e-3, "bf16": 2e-3}     # test_logprob's (tests/test_kernels_gpu.py)
SETTING = {s[0]: s for s in PO.SETTINGS}


def _table(cuda, sched, clip, pe, like=None):
    """The product's table of a DDPM schedule with its record set (x0 rows when not pe); like: a copy of that
    table (a DDIM one, which has no x0 form) instead."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    tab = like.clone() if like is not None else torch.tensor(ops.sched_table(sched, pe), device=cuda)
    return ops.sched_set_params(tab, clip, pe)


def _gpu(cuda, dims, precision, E, clip, pe, seed=11):
    """The sampler surface's inputs and device half with the setting's table; without the clip, on the
    denoiser-like reshaping of the same seeded models (PO.denoiser_like says why), oracle and images alike."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    inp = SS._Inputs(dims, E, seed=seed)
    g = SS._Gpu(inp, precision, cuda)
    g.tab = _table(cuda, inp.sched, clip, pe)
    inp.sched = O.with_param(inp.sched, clip, pe)
    if clip is None:
        inp.base, inp.ft = PO.sampler_models(inp, clip)
        spec = ops.actor_param_spec(inp.d)
        flat = lambda p: torch.tensor(ops.flatten_params(spec, p), device=cuda)
        g.packb, g.packf = ops.pack_actor(inp.d, flat(inp.base), precision), ops.pack_actor(inp.d, flat(inp.ft), precision)
    return inp, g


# ------------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------------
# (setting, precision, envs, K', kernel, launch / oracle keywords)
SAMPLER_CASES = [(s, p, E, 10, SPLIT, {}) for s in PO.SETTING_IDS for p, E in (("fp32", 16), ("bf16", 17), ("fp16", 16))]
SAMPLER_CASES += [
    ("clip0.5", "fp32", 17, 10, SPLIT, dict(deterministic=True)),
    ("x0", "bf16", 16, 10, SPLIT, dict(deterministic=True)),
    ("clip2", "bf16", 16, 10, SPLIT, dict(final_clip=0.7)),
    # the streaming kernel (more than 512 envs), at K' = K (chain row 0 from the draw loop) and K' = 1
    ("clip0.5", "bf16", 513, 20, STREAM, {}),
    ("x0", "fp32", 513, 1, STREAM, {}),
    ("noclip", "fp16", 513, 20, STREAM, {}),
    ("clip2", "fp32", 513, 1, STREAM, dict(deterministic=True)),
]
SAMPLER_IDS = [f"{s}-{p}-E{E}-kf{kf}" + "".join(f"-{k}" for k in kw) for s, p, E, kf, _, kw in SAMPLER_CASES]


@pytest.mark.parametrize("setting,precision,E,kf,kernel,kw", SAMPLER_CASES, ids=SAMPLER_IDS)
def test_sampler_matches_param_oracle(cuda, setting, precision, E, kf, kernel, kw):
    """dppo_sample, injected noise, on a table with the setting recorded: actions and every stored chain row
    against O.sample on the setting's schedule, at the sampler surface's bounds; two launches bit-identical."""
    _, clip, pe = SETTING[setting]
    inp, g = _gpu(cuda, dict(HOPPER, ft_denoising_steps=kf), precision, E, clip, pe)
    assert g.plan["kernel"] == kernel, g.plan
    act, ch = g.twice(**kw)
    ref = inp.oracle(precision, **kw)
    SS._check(f"param {setting} E{E} kf{kf}", precision, SS._stats(act, ch, *ref), plan=g.plan)


@pytest.mark.parametrize("setting,precision", [("clip0.5", "fp32"), ("x0", "bf16"), ("noclip", "bf16")])
def test_sample_step_equals_sample(cuda, setting, precision):
    """dppo_sample_step through mapped staging memory, 16 envs: bit-equal to dppo_sample on the same Philox stream
    and the same table."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import ptr, stream_handle
    _, clip, pe = SETTING[setting]
    E = 16
    inp, g = _gpu(cuda, HOPPER, precision, E, clip, pe)
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
    assert actions.cpu().numpy().tobytes() == a_ref.tobytes() and chains.cpu().numpy().tobytes() == c_ref.tobytes()
    assert ma.tensor.numpy().tobytes() == a_ref.tobytes()
    # and the setting is in force: the default table gives other bits
    g.tab = _table(cuda, inp.sched, 1.0, True)
    assert g.sample(xT=None, z=None)[0].tobytes() != a_ref.tobytes()


@pytest.mark.parametrize("cfg_name", ["ft_ppo_diffusion_mlp_x0", "ft_ppo_diffusion_mlp_noclip"])
def test_tagged_rollout_equals_model_call(cuda, monkeypatch, cfg_name):
    """dppo_rollout_enqueue_tagged on the model of each new fine-tune cfg (bf16, 16 envs, two pre-enqueued steps):
    observations, actions and chains bit-equal to model(obs), which is dppo_sample on the model's table."""
    import torch
    monkeypatch.setenv("DPPO_ROLLOUT_PROTOCOL", "tagged")
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util.config import instantiate, load_config
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), cfg_name, ["model.precision=bf16"])
    model = instantiate(cfg.model, device=cuda, seed=5)
    d = model.dims
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


# ------------------------------------------------------------------------------------------------
# dppo_logprob
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 77])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("setting", PO.SETTING_IDS)
def test_logprob_matches_param_oracle(cuda, setting, precision, n):
    """dppo_logprob at 33 and 77 samples (330 / 770 rows: ragged 32-row tiles) on unit-scale chains."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    _, clip, pe = SETTING[setting]
    d, _, ft, _, sched, _, _, pf, _ = KG._setup(HOPPER, cuda)
    tab = _table(cuda, sched, clip, pe)
    kf = d.ft_denoising_steps
    _, obs, chains, _, _ = PO.update_inputs(d, n)
    ref = O.get_logprobs(to_f64(ft), O.with_param(sched, clip, pe), obs.reshape(n, 1, -1).astype(np.float64),
                         chains.reshape(n, kf + 1, d.horizon_steps, d.action_dim).astype(np.float64), kf,
                         rnd=KG._rnd(precision))
    lpe, lpm = ops.logprob(d, precision, ops.pack_actor(d, pf, precision), tab, torch.tensor(obs, device=cuda),
                           torch.tensor(chains, device=cuda))
    torch.cuda.synchronize()
    lpe = lpe.cpu().numpy().reshape(ref.shape)
    ref_mean = np.clip(ref, -5, 2).mean(axis=(1, 2)).reshape(n, kf)
    tol = LOGPROB_TOL[precision]
    q99 = float(np.quantile(np.abs(lpe - ref) / (1 + np.abs(ref)), 0.99))
    mean_err = float(np.abs(lpm.cpu().numpy() - ref_mean).max())
    print(json.dumps({"case": f"param-logprob-{setting}-{precision}-n{n}", "q99": q99, "bound": tol, "mean_err": mean_err}))
    assert q99 < tol and mean_err < tol * 10


# ------------------------------------------------------------------------------------------------
# dppo_ppo_minibatch
# ------------------------------------------------------------------------------------------------
def _case(monkeypatch, cuda, precision, dims, N, clip, pe, **kw):
    """A UR._Case on unit-scale chains whose table and oracle schedule carry the setting (the case's own
    constructor already launches dppo_logprob on it)."""
    setup = UR._setup

    def setup_with_record(dims_, cuda_, **skw):
        out = list(setup(dims_, cuda_, **skw))
        out[5] = _table(cuda_, out[4], clip, pe, like=out[5] if pe else None)
        out[4] = O.with_param(out[4], clip, pe)
        return tuple(out)

    monkeypatch.setattr(UR, "_setup", setup_with_record)
    monkeypatch.setattr(UR, "_inputs", PO.update_inputs)
    return UR._Case(cuda, precision, dims, N, **kw)


def _grads_vs_oracle(case, rows, label, learn_eta=False, indexed=True):
    """One minibatch of `rows` permutation rows from START (through a row_index when indexed) against the case's
    oracle at the regime tests' bounds."""
    import torch
    from oracle import philox as PX
    stats, mean_std = case.adv_stats(rows)
    met_ref, ga_ref, gc_ref = case.oracle(rows, adv_mean_std=mean_std, eta_grad=learn_eta)
    index = None
    if indexed:
        index = torch.tensor(PX.feistel_permute(np.arange(UR.START + rows), case.total, UR.SEED, UR.EPOCH).astype(np.int64),
                             device=case.cuda)
    g, m = case.launch(rows, UR.START, rows, stats=stats, row_index=index, learn_eta=learn_eta)
    assert np.isfinite(g).all()
    tol = UR.TOL[case.precision]
    UR._check_metrics(m / rows, met_ref, tol, True, label)
    UR._check_errs(UR._tensor_errs(case.d, g, ga_ref, gc_ref), tol, label)
    return m, met_ref


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("setting", PO.SETTING_IDS)
def test_minibatch_grads_match_param_oracle(cuda, monkeypatch, setting, precision):
    """77 rows through a row_index (two whole 32-row tiles and a 13-row tail), ratio 1: the loss metrics and every
    actor and critic gradient tensor."""
    _, clip, pe = SETTING[setting]
    case = _case(monkeypatch, cuda, precision, HOPPER, -(-(UR.START + 77) // 10) + 20, clip, pe)
    _grads_vs_oracle(case, 77, f"param-{setting}-{precision}-r77")


def test_minibatch_grads_mish_x0(cuda, monkeypatch):
    _, clip, pe = SETTING["x0"]
    case = _case(monkeypatch, cuda, "bf16", HOPPER_MISH, -(-(UR.START + 77) // 10) + 20, clip, pe)
    _grads_vs_oracle(case, 77, "param-x0-mish-bf16-r77")


def test_minibatch_grads_plain_clip(cuda, monkeypatch):
    _, clip, pe = SETTING["clip0.5"]
    case = _case(monkeypatch, cuda, "fp32", HOPPER_PLAIN, -(-(UR.START + 77) // 10) + 20, clip, pe)
    _grads_vs_oracle(case, 77, "param-clip0.5-plain-fp32-r77")


def test_minibatch_grads_tile64_clip2(cuda, monkeypatch):
    """The bf16 minibatch of 64 x CU-count rows, which takes the 64-row tile, at clip 2."""
    from diffusionpolicyoptimization_amd import ops
    _, clip, pe = SETTING["clip2"]
    rows = 64 * UR._cus(cuda)
    case = _case(monkeypatch, cuda, "bf16", HOPPER, -(-(UR.START + rows) // 10) + 50, clip, pe)
    plan = ops.ppo_plan(case.d, "bf16", rows)
    assert plan["actor_tile_rows"] == 64 and plan["actor_waves"] == 16, plan
    _grads_vs_oracle(case, rows, "param-clip2-tile64", indexed=False)


def test_minibatch_learn_eta_ddim_clip(cuda, monkeypatch):
    """DPPO_PPO_LEARN_ETA under DDIM (bf16, eta 0.6) at clip 0.5: metrics[8] against the oracle's eta_grad, whose
    x0 is clipped at the schedule's bound, at the 64-row tile test's d_eta bound (3e-2 relative)."""
    _, clip, pe = SETTING["clip0.5"]
    case = _case(monkeypatch, cuda, "bf16", HOPPER_DDIM, US.NSAMP, clip, pe, eta=0.6)
    m, met_ref = _grads_vs_oracle(case, US.ROWS, "param-clip0.5-learn-eta", learn_eta=True, indexed=False)
    ref = met_ref["d_eta"]
    print(json.dumps({"case": "param-learn-eta", "d_eta": float(m[8]), "ref": ref}))
    assert abs(ref) > 1e-3 and abs(m[8] - ref) <= 3e-2 * abs(ref), (m[8], ref)


# ------------------------------------------------------------------------------------------------
# dppo_pretrain_minibatch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", C.PRECISIONS)
@pytest.mark.parametrize("rows", [1, 33, 65])
def test_pretrain_x0_target(cuda, rows, precision):
    """The x0 target at 1, 33 and 65 rows: the loss and every gradient tensor against O.p_losses on an x0 schedule."""
    p = PT._Problem(cuda, HOPPER)
    p.tab = _table(cuda, p.sched, 1.0, False)
    inp = C.inputs(rows, 20)
    loss, g, _, _ = PT._run(p, precision, inp)
    loss_ref, g_ref = C.reference(p.ft, O.with_param(p.sched, 1.0, False), inp, rnd=PT._rnd(precision))
    PT._check(f"x0-rows{rows}", precision, loss, g, loss_ref, g_ref)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pretrain_epsilon_noclip_is_bit_equal(cuda, precision):
    """Pretraining never clips: the epsilon target on a table recorded as {None, epsilon} gives the bits of an
    unrecorded table."""
    p = PT._Problem(cuda, HOPPER)
    inp = C.inputs(65, 20)
    loss0, _, grads0, met0 = PT._run(p, precision, inp)
    p.tab = _table(cuda, p.sched, None, True)
    loss1, _, grads1, met1 = PT._run(p, precision, inp)
    assert loss0 == loss1 and grads0.cpu().numpy().tobytes() == grads1.cpu().numpy().tobytes()
    assert met0.cpu().numpy().tobytes() == met1.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------
# the attribute
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,E", [("fp32", 16), ("bf16", 17), ("bf16", 513)])
def test_explicit_default_record_is_bit_equal(cuda, precision, E):
    """A table set explicitly to {1.0, epsilon} gives the bits of an unrecorded table."""
    from diffusionpolicyoptimization_amd import ops
    inp = SS._Inputs(HOPPER, E, seed=11)
    g = SS._Gpu(inp, precision, cuda)
    a0, c0 = g.sample()
    ops.sched_set_params(g.tab, 1.0, True)
    a1, c1 = g.sample()
    assert a0.tobytes() == a1.tobytes() and c0.tobytes() == c1.tobytes()


def test_record_is_erased_with_the_tensor(cuda):
    """The record goes when the table's tensor is freed: a new table at the same address reads as the default.
    Unreachable cycles of earlier tests (models, rollout pipes) are collected first: collected by the gc.collect()
    below instead, their device blocks would join the free list between the table's release and the clones, ahead
    of the table's block, and whether an automatic collection has run by then depends on how many Python objects
    the tests before this one happened to allocate."""
    import torch
    gc.collect()
    inp = SS._Inputs(HOPPER, 16, seed=11)
    g = SS._Gpu(inp, "fp32", cuda)
    a_def, _ = g.sample()
    default_tab = g.tab
    g.tab = _table(cuda, inp.sched, 0.5, True)
    address = g.tab.data_ptr()
    assert g.sample()[0].tobytes() != a_def.tobytes()
    g.tab = default_tab
    gc.collect()
    # the caching allocator hands the freed block back to one of the next allocations of its size
    held = []
    for _ in range(256):
        held.append(default_tab.clone())
        if held[-1].data_ptr() == address:
            break
    reused = held[-1]
    assert reused.data_ptr() == address, "the allocator did not reuse the block; the check needs the same address"
    g.tab = reused
    assert g.sample()[0].tobytes() == a_def.tobytes()


def _sentinel_sample(g, inp, d=None):
    import torch
    from diffusionpolicyoptimization_amd import ops
    d = d or inp.d
    E = inp.E
    actions = torch.full((E, d.xd), SS.SENTINEL, device=g.cuda)
    chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SS.SENTINEL, device=g.cuda)
    call = lambda: ops.sample(d, g.precision, g.packb, g.packf, g.tab, g.T(inp.state.reshape(E, -1)),
                              x_T=g.T(inp.xT.reshape(E, -1)), noise=g.T(inp.z.reshape(inp.K, E, -1)), actions=actions,
                              chains=chains)
    return call, (actions, chains)


def _refused(call, outputs, msg):
    import torch
    from diffusionpolicyoptimization_amd._lib import DppoError
    with pytest.raises(DppoError, match=re.escape(f"failed (1): {msg}")):
        call()
    torch.cuda.synchronize()
    for o in outputs:
        assert bool((o == SS.SENTINEL).all()), "a refused call wrote its outputs"


def test_set_params_refusals_keep_the_record(cuda):
    """A NaN or negative finite clip, and predict_x0 on DDIM rows: DPPO_EINVAL, the record as it was."""
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import DppoError, ptr
    inp, g = _gpu(cuda, HOPPER, "fp32", 16, 0.5, True)
    a_half, _ = g.sample()
    for clip, msg in ((float("nan"), "dppo_sched_set_params: denoised_clip is NaN"),
                      (-0.5, "dppo_sched_set_params: negative denoised_clip -0.5")):
        with pytest.raises(DppoError, match=re.escape(f"failed (1): {msg}")):
            _lib.call("dppo_sched_set_params", ptr(g.tab), clip, 0)
        assert g.sample()[0].tobytes() == a_half.tobytes()
    ddim = SS._Gpu(SS._Inputs(HOPPER_DDIM, 16, seed=11), "fp32", cuda)
    with pytest.raises(DppoError, match=re.escape("failed (1): dppo_sched_set_params: DDIM requires predicting epsilon")):
        _lib.call("dppo_sched_set_params", ptr(ddim.tab), 1.0, 1)
    a_ddim, _ = ddim.sample()
    ops.sched_set_params(ddim.tab, 1.0, True)
    assert ddim.sample()[0].tobytes() == a_ddim.tobytes()
    # 0 and the infinities mean None
    ref = None
    for none in (0.0, float("inf"), float("-inf")):
        _lib.call("dppo_sched_set_params", ptr(g.tab), none, 0)
        a = g.sample()[0].tobytes()
        ref = ref or a
        assert a == ref and a != a_half.tobytes()


@pytest.mark.parametrize("precision,E", [("fp32", 16), ("bf16", 513)])
def test_x0_with_time_stride_is_refused(cuda, precision, E):
    """An x0 table under dims with time_stride 2: every entry refuses before anything is enqueued."""
    import dataclasses
    import torch
    from diffusionpolicyoptimization_amd import ops
    inp, g = _gpu(cuda, HOPPER, precision, E, 1.0, False)
    strided = dataclasses.replace(inp.d, time_stride=2)
    msg = "DDIM requires predicting epsilon (an x0-prediction schedule table with time_stride 2)"
    call, outs = _sentinel_sample(g, inp, strided)
    _refused(call, outs, "dppo_sample: " + msg)
    n, kf = 5, strided.ft_denoising_steps
    lpe = torch.full((n * kf, strided.xd), SS.SENTINEL, device=cuda)
    lpm = torch.full((n, kf), SS.SENTINEL, device=cuda)
    _refused(lambda: ops.logprob(strided, precision, g.packf, g.tab, torch.zeros(n, strided.sd, device=cuda),
                                 torch.zeros(n, kf + 1, strided.xd, device=cuda), lp_elem=lpe, lp_mean=lpm),
             (lpe, lpm), "dppo_logprob: " + msg)
    g.sample()


def test_x0_with_learn_eta_is_refused(cuda, monkeypatch):
    """DPPO_PPO_LEARN_ETA on an x0 table: DPPO_EINVAL, gradients and metrics at their sentinels."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    _, clip, pe = SETTING["x0"]
    case = _case(monkeypatch, cuda, "bf16", HOPPER, 40, clip, pe)
    rows = 77
    grads = torch.full((case.na + case.nc,), SS.SENTINEL, dtype=torch.float32, device=cuda)
    met = torch.full((16,), SS.SENTINEL, dtype=torch.float64, device=cuda)
    ws = ops.ppo_workspace(case.d, "bf16", rows, cuda)
    hp = ops.ppo_hparams(global_rows=rows, learn_eta=True)
    _refused(lambda: ops.ppo_minibatch(case.d, "bf16", hp, case.packf, case.packc, case.pf, case.tab, *case.args, UR.SEED,
                                       UR.EPOCH, UR.START, rows, ws, grads, met),
             (grads, met), "dppo_ppo_minibatch: DPPO_PPO_LEARN_ETA on an x0-prediction schedule table")


def test_x0_with_time_stride_is_refused_by_every_entry(cuda, monkeypatch):
    """The other entries that read the record, under dims with time_stride 2 on an x0 table: dppo_sample_step
    (mapped and unmapped staging memory), dppo_rollout_enqueue_tagged, dppo_ppo_minibatch and
    dppo_pretrain_minibatch (whose own time_stride check fires first): outputs at their sentinels."""
    import dataclasses
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import ptr, stream_handle
    precision, E = "bf16", 16
    inp, g = _gpu(cuda, HOPPER, precision, E, 1.0, False)
    d = dataclasses.replace(inp.d, time_stride=2)
    msg = "dppo_sample: DDIM requires predicting epsilon (an x0-prediction schedule table with time_stride 2)"
    host_ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    mc, ma = ops.MappedArray((E, d.sd), np.float32), ops.MappedArray((E, d.xd), np.float32)
    plain_c, plain_a = torch.zeros(E, d.sd), torch.full((E, d.xd), SS.SENTINEL)
    mc.tensor.zero_()
    for cond_h, act_h in ((mc.tensor, ma.tensor), (plain_c, plain_a)):
        act_h.fill_(SS.SENTINEL)
        cond = torch.full((E, d.sd), SS.SENTINEL, device=cuda)
        actions = torch.full((E, d.xd), SS.SENTINEL, device=cuda)
        chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SS.SENTINEL, device=cuda)
        _refused(lambda: _lib.call("dppo_sample_step", ctypes.byref(d.c()), _lib.PRECISION[precision], ptr(g.packb),
                                   ptr(g.packf), ptr(g.tab), host_ptr(cond_h), ptr(cond), E, ctypes.c_uint64(SS.SEED),
                                   ctypes.c_uint64(SS.CALL), 0, 0, 0.1, 3.0, 0.0, ptr(actions), host_ptr(act_h),
                                   ptr(chains), 1, stream_handle(cuda)),
                 (cond, actions, chains, act_h), msg)
    # the tagged enqueue: observation granules, action granules and the done counter in mapped memory
    obs_t, act_t = ops.MappedArray((E, d.sd), np.uint64), ops.MappedArray((E, d.xd), np.uint64)
    done = ops.MappedArray((1,), np.uint32)
    addr = lambda mapped: ctypes.c_void_p(mapped.address)          # created zeroed
    cond = torch.full((E, d.sd), SS.SENTINEL, device=cuda)
    actions = torch.full((E, d.xd), SS.SENTINEL, device=cuda)
    chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SS.SENTINEL, device=cuda)
    _refused(lambda: _lib.call("dppo_rollout_enqueue_tagged", ctypes.byref(d.c()), _lib.PRECISION[precision], ptr(g.packb),
                               ptr(g.packf), ptr(g.tab), addr(obs_t), ptr(cond), E, ctypes.c_uint64(SS.SEED),
                               ctypes.c_uint64(SS.CALL), 0, 0, 0.1, 3.0, 0.0, ptr(actions), addr(act_t),
                               ptr(chains), ctypes.c_uint32(7), addr(done), stream_handle(cuda)),
             (cond, actions, chains), msg)
    assert not act_t.array.any() and not done.array.any()
    # the update entries
    _, clip, pe = SETTING["x0"]
    case = _case(monkeypatch, cuda, precision, HOPPER, 40, clip, pe)
    rows = 77
    grads = torch.full((case.na + case.nc,), SS.SENTINEL, dtype=torch.float32, device=cuda)
    met = torch.full((16,), SS.SENTINEL, dtype=torch.float64, device=cuda)
    ws = ops.ppo_workspace(d, precision, rows, cuda)
    _refused(lambda: ops.ppo_minibatch(d, precision, ops.ppo_hparams(global_rows=rows), case.packf, case.packc, case.pf,
                                       case.tab, *case.args, UR.SEED, UR.EPOCH, UR.START, rows, ws, grads, met),
             (grads, met), "dppo_ppo_minibatch: DDIM requires predicting epsilon (an x0-prediction schedule table with "
             "time_stride 2)")
    p = PT._Problem(cuda, HOPPER)
    p.tab = _table(cuda, p.sched, 1.0, False)
    inp_p = C.inputs(33, 20)
    g_pre, m_pre = PT._sentinels(p)
    T = lambda x: torch.tensor(x, device=cuda)
    _refused(lambda: ops.pretrain_minibatch(d, precision, p.packed(precision), p.pf, p.tab, p.qs, T(inp_p["x0"]),
                                            T(inp_p["cond"]), T(inp_p["t"]), T(inp_p["noise"]),
                                            ops.ppo_workspace(d, precision, 33, cuda), g_pre, m_pre),
             (g_pre, m_pre), "dppo_pretrain_minibatch: the time-embedding table must be unstrided (time_stride 1)")
    g.sample()


# ------------------------------------------------------------------------------------------------
# the no-clip sampler at the seeded networks' own scale
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,E,kf,kernel", [("fp32", 16, 10, SPLIT), ("bf16", 17, 10, SPLIT), ("fp16", 513, 20, STREAM)])
def test_sampler_noclip_seeded_scale(cuda, precision, E, kf, kernel):
    """The seeded, untrained models without the clip (chains of 10^3): the sampler surface's statistics and bounds on
    actions and chains divided by s = max |reference chain|. The absolute bounds were set for chains the clip keeps
    of order 1; dividing by s puts these chains on that scale, and an error of the MLP path is not attenuated as
    under PO.denoiser_like."""
    inp = SS._Inputs(dict(HOPPER, ft_denoising_steps=kf), E, seed=11)
    g = SS._Gpu(inp, precision, cuda)
    g.tab = _table(cuda, inp.sched, None, True)
    inp.sched = O.with_param(inp.sched, None, True)
    assert g.plan["kernel"] == kernel, g.plan
    act, ch = g.twice()
    ref_a, ref_c = inp.oracle(precision)
    s = float(np.abs(ref_c).max())
    assert s > 100.0, s
    SS._check(f"param noclip seeded-scale E{E} kf{kf}", precision, SS._stats(act / s, ch / s, ref_a / s, ref_c / s), plan=g.plan, s=s)


# ------------------------------------------------------------------------------------------------
# agents
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting,suffix", [("x0", "_x0"), ("noclip", "_noclip")])
def test_finetune_iterations_match_oracle(cuda, tmp_path, monkeypatch, setting, suffix):
    """TrainPPODiffusionAgent from each new fine-tune cfg (fp32, seed 42, the shapes of tests/test_iteration_gpu.py):
    an eval iteration and two training iterations against oracle/iteration.py on the model's setting, at that file's own
    bounds (IT._run_and_compare): rollout chains through the model's sched / sched_eval, old log-probs, the update's
    minibatches and the parameter change. The no-clip agent starts from a denoiser-like base policy checkpoint
    (PO.denoiser_like of the seeded weights), for the reason given there."""
    from diffusionpolicyoptimization_amd.util import config
    from tests import test_iteration_gpu as IT
    from tests.helpers import make_models
    _, clip, pe = SETTING[setting]
    load = config.load_config
    monkeypatch.setattr(config, "load_config", lambda root, name, ov: load(root, name + suffix, ov))
    extra = []
    if clip is None:
        base, _, _ = make_models(0, HOPPER)
        ck = str(tmp_path / "denoiser_like.npz")
        np.savez(ck, **{"network." + k: v for k, v in PO.denoiser_like(base).items()})
        extra = [f"base_policy_path={ck}"]
    a, orc = IT._agent_and_oracle(42, tmp_path, extra)
    m = a.model
    assert m.predict_epsilon == pe and m.denoised_clip_value == clip
    assert (orc.sched["denoised_clip"], orc.sched["predict_epsilon"]) == (PO.bound_of(clip), pe)
    errs = IT._run_and_compare(a, orc, n_itr=3)
    print(json.dumps({"case": f"param-iteration-{setting}", "iterations": errs}))
    assert [e["eval"] for e in errs] == [True, False, False]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pretrain_x0_steps_follow_the_oracle(cuda, tmp_path, monkeypatch, precision):
    """TrainDiffusionAgent.run() from pre_diffusion_mlp_x0.yaml over three epochs, teacher-forced exactly as
    tests/test_pretrain_step_gpu.py test_pretrain_steps_follow_the_oracle does (that test's body, with the cfg name
    replaced; the reference follows the model's predict_epsilon): every step's loss and gradient against O.p_losses
    with the x0 target."""
    from diffusionpolicyoptimization_amd.util import config
    load = config.load_config
    seen = []

    def load_x0(root, name, ov):
        cfg = load(root, name + "_x0", ov)
        seen.append(cfg.model["predict_epsilon"])
        return cfg

    monkeypatch.setattr(config, "load_config", load_x0)
    PT.test_pretrain_steps_follow_the_oracle(cuda, tmp_path, precision)
    assert seen == [False]
