"""ELU, GELU and Softplus actors on the GPU: every entry that takes a packed actor image, against the oracle
with that activation (O.Model(act=<name>), derived from the dims).

Each case mirrors a case of tests/test_actor_mish_gpu.py at the same shape with the same bound, through the same
helpers (_Inputs / _Gpu / _check of test_sampler_surface_gpu, _Problem / _Gpu / _compare of
test_update_surface_gpu, _Case of test_update_regimes_gpu, _setup of test_kernels_gpu): the sampler's fp32 2e-4
absolute on actions and chains, 2-byte q99 / means 2e-3 bf16; dppo_logprob's q99 of |d| / (1 + |ref|) 1e-3 fp32,
2e-3 bf16, the row mean ten times that; per gradient tensor 2e-3 fp32, 1e-2 2-byte; d_eta 3e-2 relative. One
statistic of three sampler cases has a bound of its own (ACT_Q99_SCALE below, with its reason); no other bound
here is new. Every figure is printed as a JSON line before it is asserted.

The update problems take N(0, 1) biases (mish_models), asserted on the oracle's cache to put >= 5 % of h1 and of
h2 below -1 and >= 20 % above 0 (site_coverage): where the five activations differ.

The dims carry `activation=<name>`, so ops.pack_actor records it with every image (dppo_pack_actor_head)."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import test_iteration_gpu as IT
from tests import test_kernels_gpu as KG
from tests import test_sampler_surface_gpu as SS
from tests import test_update_regimes_gpu as UR
from tests import test_update_surface_gpu as US
from tests.helpers import HOPPER, HOPPER_DDIM, WALKER, to_f64
from tests.variants import NEW_ACTIVATIONS, dims_of, mish_models, site_coverage

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT, STREAM = 2, 0
ACTS = pytest.mark.parametrize("name", NEW_ACTIVATIONS)


# ------------------------------------------------------------------------------------------------
# sampler (test_actor_mish_gpu.py SAMPLER_CASES / test_sampler_matches_mish_oracle; the plain case:
# test_actor_plain_gpu.py "hopper-bf16-E64-mish")
# ------------------------------------------------------------------------------------------------
# (label, dims, extra dims keys, precision, envs, kernel)
# Every bound is SS._check's, the ReLU and Mish cases', but ONE statistic of THREE cases: the bf16 q99 of the actions
# at hopper E = 513 for ELU (times 2) and at hopper E = 17 and E = 513 for Softplus (times 3). The kernel and the
# oracle round the same operands at the same points and differ only where an fp32 sum's error tips a bf16 rounding
# the other way; how far twenty denoising steps carry such a decision depends on the network, and the 2e-3 bound is
# the ReLU network's. ELU and Softplus do not vanish on the negative side (-1, and ln 2 at 0), so every hidden unit
# carries a bf16 half-ulp of 1e-3 to 2e-3 where relu, mish and gelu carry zeros or small values. The ORACLE ALONE
# shows it (tests.variants.sampler_self_noise: O.sample against itself with 2e-7 relative noise ahead of each
# rounding; tests/test_actor_activations_cpu.py::test_sampler_q99_scale_is_the_oracles_own pins these figures):
#   E = 513 (q99 of 6,156 actions, a stable statistic): ReLU 1.21e-3, Mish 1.19e-3, GELU 0.95e-3, ELU 2.02e-3 (1.67 x
#     ReLU), Softplus 3.18e-3 (2.63 x ReLU): ELU and Softplus are past ReLU's bound in the reference itself; the
#     factors are those ratios rounded up, 2 and 3. The kernels measured 2.07e-3 and 2.93e-3.
#   E = 17 (q99 of 204 actions = the third largest: a few single rounding decisions): over 16 noise draws the
#     oracle's own q99 runs 2.0e-4 .. 5.8e-4 for ReLU, 4.3e-4 .. 1.13e-3 for ELU (inside 2e-3: no factor; the kernel
#     measured 1.10e-3) and 7.8e-4 .. 2.69e-3 for Softplus (median 1.28e-3 = 3.2 x ReLU's 3.96e-4): ReLU's bound lies
#     inside the reference's own spread there; the kernel measured 2.34e-3. Same factor 3.
# Every other statistic (act_max, the chain means), fp32, fp16, GELU, walker and the plain head keep SS._check's
# bounds as they are.
ACT_Q99_SCALE = {("ELU", "hopper-bf16-E513"): 2.0, ("Softplus", "hopper-bf16-E17"): 3.0, ("Softplus", "hopper-bf16-E513"): 3.0}


def _check_sampler(label, name, case, precision, st, **extra):
    """SS._check with the bound on act_q99 times ACT_Q99_SCALE[(name, case)] where there is one."""
    b = SS._bounds(precision)
    if (name, case) in ACT_Q99_SCALE:
        b["act_q99"] *= ACT_Q99_SCALE[(name, case)]
    print(json.dumps(dict(case=label, precision=precision, observed=st, bound=b, **extra)))
    bad = {k: (st[k], v) for k, v in b.items() if not st[k] < v}
    assert not bad, (label, bad)


SAMPLER_CASES = [
    ("hopper-fp32-E17", HOPPER, {}, "fp32", 17, SPLIT),            # split, P = 8 form; a ragged second group
    ("hopper-bf16-E17", HOPPER, {}, "bf16", 17, SPLIT),            # split, KX = 1 form
    ("hopper-bf16-E513", HOPPER, {}, "bf16", 513, STREAM),         # the weight-streaming kernel
    ("walker-bf16-E64", WALKER, {}, "bf16", 64, SPLIT),            # split, KX = 2 form
    ("hopper-fp16-E17-ddim", HOPPER_DDIM, {}, "fp16", 17, SPLIT),
    ("hopper-bf16-E64-plain", HOPPER, dict(head="plain"), "bf16", 64, SPLIT),
    ("hopper-fp32-E513-plain", HOPPER, dict(head="plain"), "fp32", 513, STREAM),
]


@ACTS
@pytest.mark.parametrize("label,dims,extra,precision,E,kernel", SAMPLER_CASES, ids=[c[0] for c in SAMPLER_CASES])
def test_sampler_matches_oracle(cuda, name, label, dims, extra, precision, E, kernel):
    """dppo_sample on images of the activation, injected noise, against O.sample with the activation: actions and
    every stored chain row (SS._check's bounds, the ReLU and Mish cases'; ACT_Q99_SCALE above for one statistic of
    three cases); the plan is the ReLU plan of the shape."""
    from diffusionpolicyoptimization_amd import ops
    inp = SS._Inputs(dims_of(name, dims, **extra), E, seed=11)
    g = SS._Gpu(inp, precision, cuda)
    assert g.plan["kernel"] == kernel and g.plan == ops.sampler_plan(ops.ModelDims(**dims), precision, E), g.plan
    act, ch = g.twice()
    _check_sampler(f"{name} {label}", name, label, precision, SS._stats(act, ch, *inp.oracle(precision)), plan=g.plan)


def _einval(call, outputs, msg):
    """call() raises DPPO_EINVAL (code 1) with the message and leaves the sentinel-filled outputs."""
    import torch
    from diffusionpolicyoptimization_amd._lib import DppoError
    with pytest.raises(DppoError, match=re.escape(f"failed (1): {msg}")):
        call()
    torch.cuda.synchronize()
    for o in outputs:
        assert bool((o == SS.SENTINEL).all()), "a refused call wrote its outputs"


@pytest.mark.parametrize("precision,E", [("bf16", 17), ("bf16", 513)])
def test_sampler_refuses_mixed_images(cuda, precision, E):
    """A Mish base image with a GELU fine-tuned image, the reverse, and ELU with GELU (which share the sampler's
    instantiation): DPPO_EINVAL with the existing message before anything is enqueued, outputs at the sentinel."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    inp = SS._Inputs(dims_of("GELU"), E, seed=11)
    g = SS._Gpu(inp, precision, cuda)
    d = inp.d
    _, _, _, _, _, _, pb, pf, _ = KG._setup(HOPPER, cuda)
    mish, elu = ops.ModelDims(**dims_of("Mish")), ops.ModelDims(**dims_of("ELU"))
    pairs = ((ops.pack_actor(mish, pb, precision), g.packf), (g.packb, ops.pack_actor(mish, pf, precision)),
             (ops.pack_actor(elu, pb, precision), g.packf))
    for base, ft in pairs:
        actions = torch.full((E, d.xd), SS.SENTINEL, device=cuda)
        chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SS.SENTINEL, device=cuda)
        call = lambda: ops.sample(d, precision, base, ft, g.tab, g.T(inp.state.reshape(E, -1)),
                                  x_T=g.T(inp.xT.reshape(E, -1)), noise=g.T(inp.z.reshape(inp.K, E, -1)),
                                  actions=actions, chains=chains)
        _einval(call, (actions, chains), "dppo_sample: the base and the fine-tuned actor images carry different activations")
    g.sample()


# ------------------------------------------------------------------------------------------------
# dppo_logprob (test_logprob_matches_mish_oracle; both heads)
# ------------------------------------------------------------------------------------------------
@ACTS
@pytest.mark.parametrize("head", ["residual", "plain"])
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-3), ("bf16", 2e-3)])
@pytest.mark.parametrize("n", [48, 45])
def test_logprob_matches_oracle(cuda, monkeypatch, name, head, precision, tol, n):
    """48 samples x K' = 10 = fifteen 32-row tiles, 45 a partial last tile; lp_elem (q99) and lp_mean against
    O.get_logprobs with the activation and the head."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    monkeypatch.setattr(KG, "make_models", mish_models)
    d, _, ft, _, sched, tab, _, pf, _ = KG._setup(dims_of(name, head=head), cuda)
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
    print(json.dumps({"case": f"{name}-logprob-{head}-{precision}-n{n}", "q99": q99, "bound": tol, "mean_err": mean_err,
                      "mean_bound": tol * 10, "coverage": cov}))
    assert q99 < tol and mean_err < tol * 10


# ------------------------------------------------------------------------------------------------
# dppo_ppo_minibatch / dppo_pretrain_minibatch
# ------------------------------------------------------------------------------------------------
GRAD_CASES = [("hopper", HOPPER, "fp32"), ("hopper", HOPPER, "bf16"), ("hopper", HOPPER, "fp16"), ("walker", WALKER, "bf16")]


@ACTS
@pytest.mark.parametrize("geo,dims,precision", GRAD_CASES, ids=[f"{n}-{p}" for n, _, p in GRAD_CASES])
def test_ppo_minibatch_grads_match_oracle(cuda, monkeypatch, name, geo, dims, precision):
    """test_ppo_minibatch_grads_match_mish_oracle: the surface tests' 150 rows (four 32-row tiles and a ragged
    fifth): the loss metrics and every gradient tensor against O.c_loss with the activation."""
    from diffusionpolicyoptimization_amd import ops
    monkeypatch.setattr(US, "make_models", mish_models)
    p = US._Problem(dims_of(name, dims), precision)
    caches = []
    ref = p.oracle(caches=caches)
    cov = site_coverage(caches[-1])
    gpu = US._Gpu(p, cuda)
    plan = ops.ppo_plan(p.d, precision, US.ROWS)
    assert (plan["actor_tile_rows"], plan["actor_waves"]) == (32, 8), plan
    m, g = gpu.minibatch()
    print(json.dumps({"case": f"{name}-grads-{geo}-{precision}", "coverage": cov}))
    US._compare(f"{name}-{geo}-{precision}", gpu, m, g, ref, US.TOL[precision])


@ACTS
@pytest.mark.parametrize("size", ["33", "round+1"])
def test_ppo_minibatch_row_edges(cuda, monkeypatch, name, size):
    """33 rows (one 32-row tile and one row of a second) and 32 C + 1 rows (C the CU count: one full round of
    32-row tiles and one row more), bf16: metrics and every gradient tensor at the regime tests' bound
    (test_large_minibatch_runs_the_32_row_tile's checks)."""
    from diffusionpolicyoptimization_amd import ops
    monkeypatch.setattr(KG, "make_models", mish_models)
    rows = 33 if size == "33" else 32 * UR._cus(cuda) + 1
    case = UR._Case(cuda, "bf16", dims_of(name), -(-(UR.START + rows) // 10) + 5)
    plan = ops.ppo_plan(case.d, "bf16", rows)
    assert (plan["actor_tile_rows"], plan["actor_waves"]) == (32, 8), plan
    stats, mean_std = case.adv_stats(rows)
    caches = []
    met_ref, ga_ref, gc_ref = case.oracle(rows, adv_mean_std=mean_std, caches=caches)
    cov = site_coverage(caches[-1])
    g, m = case.launch(rows, UR.START, rows, stats=stats)
    print(json.dumps({"case": f"{name}-rows-{size}", "rows": rows, "plan": plan, "coverage": cov}))
    assert np.isfinite(g).all()
    UR._check_metrics(m / rows, met_ref, UR.TOL["bf16"], True, f"{name}-rows-{size}")
    UR._check_errs(UR._tensor_errs(case.d, g, ga_ref, gc_ref), UR.TOL["bf16"], f"{name}-rows-{size}")


def test_ppo_minibatch_learn_eta_ddim_gelu(cuda, monkeypatch):
    """test_ppo_minibatch_learn_eta_ddim_mish with GELU: metrics[8] and every gradient tensor (d_eta 3e-2 relative)."""
    monkeypatch.setattr(KG, "make_models", mish_models)
    rows = US.ROWS
    case = UR._Case(cuda, "bf16", dims_of("GELU", HOPPER_DDIM), US.NSAMP, eta=0.6)
    stats, mean_std = case.adv_stats(rows)
    caches = []
    met_ref, ga_ref, gc_ref = case.oracle(rows, adv_mean_std=mean_std, eta_grad=True, caches=caches)
    cov = site_coverage(caches[-1])
    g, m = case.launch(rows, UR.START, rows, stats=stats, learn_eta=True)
    ref = met_ref["d_eta"]
    print(json.dumps({"case": "GELU-learn-eta", "d_eta": float(m[8]), "ref": ref, "coverage": cov}))
    UR._check_metrics(m / rows, met_ref, UR.TOL["bf16"], True, "GELU-learn-eta")
    assert abs(ref) > 1e-3 and abs(m[8] - ref) <= 3e-2 * abs(ref), (m[8], ref)
    UR._check_errs(UR._tensor_errs(case.d, g, ga_ref, gc_ref), UR.TOL["bf16"], "GELU-learn-eta")


@ACTS
@pytest.mark.parametrize("precision,rtol", [("fp32", 2e-3), ("bf16", 1e-2)])
@pytest.mark.parametrize("rows", [1, 33, 65])
def test_pretrain_matches_oracle(cuda, monkeypatch, name, precision, rtol, rows):
    """dppo_pretrain_minibatch at 1, 33 and 65 rows: loss and every actor gradient against O.p_losses with the
    activation (test_pretrain_matches_mish_oracle's inputs and bounds). One row covers little of the activation's
    range, so the coverage is asserted from 33 rows on."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    monkeypatch.setattr(KG, "make_models", mish_models)
    d, _, ft, _, sched, tab, _, pf, _ = KG._setup(dims_of(name), cuda)
    rng = np.random.default_rng(21)
    K = d.denoising_steps
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
    cov = site_coverage(caches[-1]) if rows >= 33 else None
    T = lambda x: torch.tensor(x, device=cuda)
    grads = torch.zeros(ops.spec_count(ops.actor_param_spec(d)), dtype=torch.float32, device=cuda)
    metrics = torch.zeros(16, dtype=torch.float64, device=cuda)
    loss = ops.pretrain_minibatch(d, precision, ops.pack_actor(d, pf, precision), pf, tab, T(ops.q_sched_table(sched)),
                                  T(x0), T(cond), T(t), T(noise), ops.ppo_workspace(d, precision, rows, cuda), grads, metrics)
    torch.cuda.synchronize()
    ga = ops.unflatten_params(ops.actor_param_spec(d), grads.cpu().numpy())
    errs = {k: float(np.abs(ga[k] - r).max() / (np.abs(r).max() + 1e-12)) for k, r in g_ref.items()}
    print(json.dumps({"case": f"{name}-pretrain-{precision}-rows{rows}", "loss": float(loss), "loss_ref": float(loss_ref),
                      "errs": errs, "coverage": cov}))
    assert abs(float(loss) - loss_ref) < rtol * loss_ref
    bad = {k: v for k, v in errs.items() if not v < rtol}
    assert not bad, (bad, errs)


# ------------------------------------------------------------------------------------------------
# the attribute
# ------------------------------------------------------------------------------------------------
def test_attribute_follows_the_image(cuda):
    """The same weights packed as ELU into one pair of buffers and as GELU into another: each launch runs its own
    activation (each within the sampler's bound of its own oracle, and the two results differ); fresh ELU, GELU
    and Softplus packs are SHA-equal to the Mish pack of the same weights; re-packed in place by plain dppo_pack_actor the ELU
    buffers sample as fresh ReLU images do, bit for bit."""
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import ptr, stream_handle
    sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    out = {}
    for name in ("ELU", "GELU"):
        inp = SS._Inputs(dims_of(name), 17, seed=11)
        g = SS._Gpu(inp, "bf16", cuda)
        out[name] = (g, *g.sample())
        SS._check(f"attribute: {name}", "bf16", SS._stats(out[name][1], out[name][2], *inp.oracle("bf16")))
    g_elu, a_elu, _ = out["ELU"]
    g_gelu, a_gelu, _ = out["GELU"]
    assert a_elu.tobytes() != a_gelu.tobytes()
    a_again, c_again = g_elu.sample()                 # the GELU packs in between changed nothing for the ELU buffers
    assert a_again.tobytes() == a_elu.tobytes()
    _, _, _, _, _, _, pb, pf, _ = KG._setup(HOPPER, cuda)
    # an activation has no parameters: fresh packs of the same weights hold the same bytes whatever they record
    digests = {n: sha(ops.pack_actor(ops.ModelDims(**dims_of(n)), pf, "bf16")) for n in ("Mish", "ELU", "GELU", "Softplus")}
    print(json.dumps({"case": "attribute: image digests", **digests}))
    assert len(set(digests.values())) == 1, digests
    relu = ops.ModelDims(**HOPPER)
    for params, img in ((pb, g_elu.packb), (pf, g_elu.packf)):      # the C entry itself, in place
        _lib.call("dppo_pack_actor", ctypes.byref(relu.c()), _lib.PRECISION["bf16"], ptr(params), ptr(img),
                  stream_handle(params.device))
    a_re, c_re = g_elu.sample()
    fresh = SS._Gpu(SS._Inputs(HOPPER, 17, seed=11), "bf16", cuda)
    a_relu, c_relu = fresh.sample()
    assert a_re.tobytes() == a_relu.tobytes() and c_re.tobytes() == c_relu.tobytes()
    assert a_re.tobytes() != a_elu.tobytes()


# ------------------------------------------------------------------------------------------------
# refusals (test_mish_refusals)
# ------------------------------------------------------------------------------------------------
@ACTS
def test_refusals(cuda, name):
    """An image of the activation is refused where a Mish image is, with the dispatch's message and untouched
    outputs: the sampler at actor_hidden 384 (bf16), dppo_logprob at actor_hidden 256 in fp32. Activation values
    2 (reserved), 6 and -1 are DPPO_EINVAL at the pack and record nothing: the buffer keeps its attribute."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import DppoError, ptr, stream_handle
    dims = dims_of(name, actor_hidden=384)
    inp = SS._Inputs(dims, 17, seed=11)
    g = SS._Gpu(inp, "bf16", cuda)
    d, E = inp.d, 17
    actions = torch.full((E, d.xd), SS.SENTINEL, device=cuda)
    chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SS.SENTINEL, device=cuda)
    SS._rejected(lambda: ops.sample(d, "bf16", g.packb, g.packf, g.tab, g.T(inp.state.reshape(E, -1)),
                                    x_T=g.T(inp.xT.reshape(E, -1)), noise=g.T(inp.z.reshape(inp.K, E, -1)),
                                    actions=actions, chains=chains), (actions, chains), SS._msg_inst(d, "bf16"))
    dims = dims_of(name, actor_hidden=256)
    d, _, _, _, _, tab, _, pf, _ = KG._setup(dims, cuda)
    n, kf = 37, d.ft_denoising_steps
    lpe = torch.full((n * kf, d.xd), SS.SENTINEL, device=cuda)
    lpm = torch.full((n, kf), SS.SENTINEL, device=cuda)
    packf = ops.pack_actor(d, pf, "fp32")
    call = lambda: _lib.call("dppo_logprob", ctypes.byref(d.c()), _lib.PRECISION["fp32"], ptr(packf), ptr(tab),
                             ptr(torch.zeros(n, d.sd, device=cuda)), ptr(torch.zeros(n, kf + 1, d.xd, device=cuda)), n,
                             0.1, 4, ptr(lpe), ptr(lpm), stream_handle(cuda))
    US._rejected(call, (lpe, lpm), US._actor_msg(dims, "fp32"))
    # a refused pack records nothing: a mixed launch against the buffer is still refused as mixed afterwards
    inp = SS._Inputs(dims_of(name), 17, seed=11)
    g = SS._Gpu(inp, "bf16", cuda)
    d = inp.d
    _, _, _, _, _, _, pb, _, _ = KG._setup(HOPPER, cuda)
    before = g.packb.clone()
    for bad in (2, 6, -1):
        with pytest.raises(DppoError, match=re.escape(f"failed (1): dppo_pack_actor_act: bad activation {bad}")):
            _lib.call("dppo_pack_actor_act", ctypes.byref(d.c()), _lib.PRECISION["bf16"], bad, ptr(pb), ptr(g.packb),
                      stream_handle(cuda))
    torch.cuda.synchronize()
    assert torch.equal(before, g.packb)
    relu_ft = ops.pack_actor(ops.ModelDims(**HOPPER), pb, "bf16")
    actions = torch.full((E, d.xd), SS.SENTINEL, device=cuda)
    chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SS.SENTINEL, device=cuda)
    _einval(lambda: ops.sample(d, "bf16", g.packb, relu_ft, g.tab, g.T(inp.state.reshape(E, -1)),
                               x_T=g.T(inp.xT.reshape(E, -1)), noise=g.T(inp.z.reshape(inp.K, E, -1)),
                               actions=actions, chains=chains), (actions, chains),
            "dppo_sample: the base and the fine-tuned actor images carry different activations")


# ------------------------------------------------------------------------------------------------
# agents
# ------------------------------------------------------------------------------------------------
CFG = {"ELU": "elu", "GELU": "gelu", "Softplus": "softplus"}


@ACTS
def test_model_call_matches_oracle(cuda, tmp_path, name):
    """test_model_call_matches_mish_oracle on the model built from the activation's cfg."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    from diffusionpolicyoptimization_amd.util.config import instantiate, load_config
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), f"ft_ppo_diffusion_mlp_{CFG[name]}",
                      ["model.precision=fp32", f"logdir={tmp_path}"])
    m = instantiate(cfg.model)
    d = m.dims
    assert d.activation == name and m.actor.activation_type == name
    E, K = 17, d.denoising_steps
    rng = np.random.default_rng(3)
    state = rng.uniform(-1, 1, (E, d.cond_steps, d.obs_dim)).astype(np.float32)
    xT = rng.standard_normal((E, d.horizon_steps, d.action_dim)).astype(np.float32)
    z = rng.standard_normal((K, E, d.horizon_steps, d.action_dim)).astype(np.float32)
    T = lambda x: torch.tensor(x, device=cuda)
    act, ch = m(T(state), x_T=T(xT.reshape(E, -1)), noise=T(z.reshape(K, E, -1)))
    torch.cuda.synchronize()
    un = lambda flat, spec: to_f64(ops.unflatten_params(spec, flat.cpu().numpy()))
    ref_a, ref_c = O.sample(un(m.base_params, m.actor_spec), un(m.actor_ft_params, m.actor_spec), ddpm_buffers(K),
                            state.astype(np.float64), xT, z, d.ft_denoising_steps,
                            min_std=m.get_min_sampling_denoising_std(), randn_clip=m.randn_clip_value, round_h3=False,
                            model=O.Model.from_dims(d))
    st = SS._stats(act.cpu().numpy().reshape(ref_a.shape), ch.cpu().numpy().reshape(ref_c.shape), ref_a, ref_c)
    SS._check(f"{name} model(cond)", "fp32", st)


@ACTS
def test_iteration_matches_oracle(cuda, tmp_path, monkeypatch, name):
    """An eval and a training iteration of the fp32 agent from the activation's cfg (seed 42, n_steps 8, batch
    size 160) against oracle/iteration.py with the activation, at tests/test_iteration_gpu.py's own bounds,
    unchanged (_run_and_compare: chains 2e-5 absolute, rewards, values, old log-probs, advantages, returns, the last
    minibatch's losses, the number of applied minibatches, the parameter change). Measured chains: ELU 2.9e-6,
    GELU 2.2e-6, Softplus 5.3e-6."""
    from diffusionpolicyoptimization_amd.util import config
    load = config.load_config
    monkeypatch.setattr(config, "load_config", lambda root, cfg, ov: load(root, f"{cfg}_{CFG[name]}", ov))
    a, orc = IT._agent_and_oracle(42, tmp_path, ["train.n_steps=8", "train.batch_size=160"])
    assert a.model.dims.activation == name and a.n_steps == 8 and a.batch_size == 160
    errs = IT._run_and_compare(a, orc, n_itr=2, need_episodes=False)
    print(json.dumps({"case": f"{name}-iteration", "iterations": errs}))
    assert [e["eval"] for e in errs] == [True, False]


def test_agent_split_update_matches_fused(cuda, tmp_path, monkeypatch):
    """test_mish_agent_split_update_matches_fused from ft_ppo_diffusion_mlp_gelu.yaml, at its bounds."""
    import torch
    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("DPPO_SPLIT_UPDATE", flag)
        cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp_gelu",
                          ["model.precision=fp32", "train.n_steps=8", "train.batch_size=160", "train.n_train_itr=2",
                           "train.val_freq=100", f"logdir={tmp_path}/{flag}"])
        a = get_class(cfg._target_)(cfg)
        assert a.model.dims.activation == "GELU"
        p_init = a.model.train_params.cpu().numpy().copy()
        res = a.run()
        torch.cuda.synchronize()
        out[flag] = (a.model.train_params.cpu().numpy().copy(), res[-1], a.timing["n_updates"])
        assert np.isfinite(out[flag][0]).all() and np.abs(out[flag][0] - p_init).max() > 0
    (p1, r1, n1), (p0, r0, n0) = out["1"], out["0"]
    assert n1 == n0
    dlt = np.abs(p1 - p0)
    print(json.dumps({"case": "GELU-agent split vs fused", "median": float(np.median(dlt)), "max": float(dlt.max())}))
    assert np.median(dlt) < 1e-6 and dlt.max() < 5e-3, (float(np.median(dlt)), float(dlt.max()))
    for k in ("pg_loss", "v_loss"):
        assert abs(r1[k] - r0[k]) <= 1e-3 * (abs(r0[k]) + 1e-3), (k, r1[k], r0[k])


def test_pretrain_agent_loss_falls_and_checkpoint_round_trips(cuda, tmp_path):
    """TrainDiffusionAgent from pre_diffusion_mlp_gelu.yaml on a synthetic dataset, three epochs: the loss on a
    fixed batch falls; its .npz checkpoint loads back bit for bit into a fresh model, which gives the same loss, and
    into the fine-tune cfg of the same activation."""
    import torch
    from diffusionpolicyoptimization_amd.agent.dataset.sequence import synthetic_dataset
    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    data = synthetic_dataset(str(tmp_path / "train.npz"), n_episodes=6, episode_len=160, seed=1)
    cfg = load_config(os.path.join(ROOT, "cfg/gym/pretrain/hopper-medium-v2"), "pre_diffusion_mlp_gelu",
                      [f"train_dataset_path={data}", f"logdir={tmp_path}/log", "train.n_epochs=3", "train.batch_size=256",
                       "train.learning_rate=1e-3"])
    agent = get_class(cfg._target_)(cfg)
    assert agent.model.network.activation_type == "GELU" and agent.model.pre_dims.activation == "GELU"
    b = next(agent.dataset_train.batches(512))
    t = torch.randint(0, 20, (512,), device=cuda, dtype=torch.int32)
    z = torch.randn(512, 12, device=cuda)
    first = float(agent.model.p_losses(b["actions"], b["conditions"], t, z))
    last_epoch = agent.run()
    last = float(agent.model.p_losses(b["actions"], b["conditions"], t, z))
    print(json.dumps({"case": "GELU-pretrain-agent", "first": first, "last": last}))
    assert np.isfinite(last_epoch) and last < first, (first, last)
    ck = str(tmp_path / "net.npz")
    agent.model.save_network(ck)
    from diffusionpolicyoptimization_amd.util.config import instantiate
    same = instantiate(cfg.model, device=cuda, seed=1, network_path=ck)
    same._pretrain_init()
    assert same.network.activation_type == "GELU" and torch.equal(same.params, agent.model.params)
    assert float(same.p_losses(b["actions"], b["conditions"], t, z)) == last
    # the fine-tune cfg of the same activation loads it as its base policy
    ft = instantiate(load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp_gelu", []).model,
                     device=cuda, seed=1, network_path=ck)
    assert ft.dims.activation == "GELU"
