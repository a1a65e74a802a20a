"""Plain critic on the GPU: the entries that take a packed critic image, against the oracle's plain critic
(O.Model(critic_head="plain"), derived from the dims).

Hopper dims (SD = 11, HC = 256) at fp32, bf16 and fp16. Bounds are the residual critic's of the same entry,
unchanged: test_critic_forward's for V (1e-4 / 1e-3 / 1e-3 of 1 + max|V|), test_ppo_minibatch_grads's per tensor
for the gradients (2e-3 fp32, 1e-2 2-byte; l2_w / l2_b take l1_w / l1_b's, being the same kind of product now: an
activation image times a rounded gradient image), test_ft20_parts_match_whole's for a part against the whole,
tests/test_iteration_gpu.py's for the iteration, test_split_update_matches_fused's for the agents. Every figure is
printed as a JSON line before it is asserted. The dims carry `critic_head="plain"`, so ops.pack_critic records
the head with every image."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from oracle import philox as PX
from tests import test_kernels_gpu as KG
from tests import test_update_ft_steps_gpu as FT
from tests import test_update_regimes_gpu as UR
from tests.helpers import HOPPER, to_f64
from tests.variants import HOPPER_PLAIN_CRITIC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V_TOL = {"fp32": 1e-4, "bf16": 1e-3, "fp16": 1e-3}          # test_critic_forward's
PRECISIONS = ["fp32", "bf16", "fp16"]
CRITIC_TENSORS = {"critic." + n for n in ("in_w", "in_b", "l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b")}


def _lp(precision):
    """fp32: perturbed old log-probs (rows on both clip branches); 2-byte: ratio 1 against the rounding oracle."""
    return "perturbed" if precision == "fp32" else "ratio1"


def _states(n, d):
    return np.random.default_rng(5).uniform(-1, 1, (n, 1, d.obs_dim)).astype(np.float32)


def _forward_err(d, precision, img, critic, n, cuda, model=None):
    """max|V - ref| / (1 + max|ref|) of dppo_critic_forward on n states against O.critic_forward for `model`
    (default: the critic the dims describe)."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    state = _states(n, d)
    ref, _ = O.critic_forward(to_f64(critic), state.astype(np.float64), model or O.Model.from_dims(d), rnd=KG._rnd(precision))
    v = ops.critic_forward(d, precision, img, torch.tensor(state.reshape(n, -1), device=cuda))
    torch.cuda.synchronize()
    v = v.cpu().numpy()
    assert v.shape == (n,) and np.isfinite(v).all()
    return float(np.abs(v - ref[:, 0]).max() / (1 + np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------
# dppo_critic_forward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 33, 77])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_critic_forward_matches_plain_oracle(cuda, precision, n):
    """n = 1 (one lane), 31 (one short of a 32-row tile), 33 (one over), 77 (a partial third tile)."""
    from diffusionpolicyoptimization_amd import ops
    d, _, _, critic, _, _, _, _, pc = KG._setup(HOPPER_PLAIN_CRITIC, cuda)
    err = _forward_err(d, precision, ops.pack_critic(d, pc, precision), critic, n, cuda)
    print(json.dumps({"case": f"plain-critic-forward-{precision}-n{n}", "err": err, "bound": V_TOL[precision]}))
    assert err < V_TOL[precision]


# ------------------------------------------------------------------------------------------------
# dppo_ppo_minibatch
# ------------------------------------------------------------------------------------------------
def _with_residual_critic(case, fn):
    """fn() with the case's critic image swapped for a residual pack of the same parameters."""
    from diffusionpolicyoptimization_amd import ops
    plain = case.packc
    case.packc = ops.pack_critic(ops.ModelDims(**HOPPER), case.pc, case.precision)
    try:
        return fn()
    finally:
        case.packc = plain


def _index(case, rows):
    import torch
    return torch.tensor(PX.feistel_permute(np.arange(UR.START + rows), case.total, UR.SEED, UR.EPOCH).astype(np.int64),
                        device=case.cuda)


# (label, rows, samples, explicit row_index, clipped value loss)
GRAD_REGIMES = {"r96-index": (96, 34, True, False), "r100": (100, 34, False, False), "r1600": (1600, 170, False, False),
                "r100-clipv": (100, 34, False, True)}
GRAD_CASES = [(p, r) for r in ("r96-index", "r100", "r1600") for p in PRECISIONS] + [("bf16", "r100-clipv")]


@pytest.mark.parametrize("precision,regime", GRAD_CASES, ids=[f"{p}-{r}" for p, r in GRAD_CASES])
def test_ppo_minibatch_critic_grads_match_plain_oracle(cuda, precision, regime):
    """One whole dppo_ppo_minibatch with a plain critic image: the value loss and every critic gradient tensor
    against O.c_loss with the plain critic; the actor's tensors and the other metrics against the same oracle too.
      r96-index:  96 rows (whole 32-row tiles) through an explicit row_index;
      r100:       100 rows over 34 samples, not a multiple of 32: every sample about three times, so the
                  sample-weighted rows and their multiplicities run (asserted);
      r1600:      1,600 rows over 170 samples: two dW m-chunks at the 768-row minimum on the host's plan, which the
                  critic's launch re-cuts on the device over its <= 170 distinct samples (192 image rows: chunks of
                  128 and 64 rows);
      r100-clipv: the clipped value loss (clip_vloss_coef 0.2), once.
    The same call with a residual image of the same critic parameters must leave the actor's gradient range
    bit-equal (its launches add each element once per m-chunk onto zero, at most two chunks here: order-free)
    and the metrics other than v_loss equal to 1e-12 relative (double atomics over the row tiles, in arrival
    order); the critic's range must differ."""
    from diffusionpolicyoptimization_amd import ops
    rows, N, use_index, clipv = GRAD_REGIMES[regime]
    case = UR._Case(cuda, precision, HOPPER_PLAIN_CRITIC, N, lp=_lp(precision))
    if clipv:
        case.old_values()
    bi, _ = case.rows_of(rows)
    mult = np.unique(bi, return_counts=True)[1]
    assert mult.max() > 1 and len(mult) < rows
    plan = ops.ppo_plan(case.d, precision, rows)
    if rows == 1600:
        assert plan["dw_chunks_critic"] == 2 and plan["dw_chunk_rows_critic"] >= 768, plan
        assert UR._device_chunks(len(mult), 1600, 2) == (128, 2)
    else:
        assert plan["dw_chunks_critic"] == 1, plan
    stats, mean_std = case.adv_stats(rows)
    met_ref, ga_ref, gc_ref = case.oracle(rows, adv_mean_std=mean_std)
    kw = dict(stats=stats, row_index=_index(case, rows) if use_index else None)
    g, m = case.launch(rows, UR.START, rows, **kw)
    assert np.isfinite(g).all() and np.isfinite(m).all()
    tol = UR.TOL[precision]
    label = f"plain-critic-{precision}-{regime}"
    UR._check_metrics(m / rows, met_ref, tol, precision != "fp32", label)
    errs = UR._tensor_errs(case.d, g, ga_ref, gc_ref)
    assert CRITIC_TENSORS <= set(errs)
    UR._check_errs(errs, tol, label)
    g_res, m_res = _with_residual_critic(case, lambda: case.launch(rows, UR.START, rows, **kw))
    others = [i for i in range(16) if i != 1]
    met_rel = float(np.abs(m[others] - m_res[others]).max() / (np.abs(m_res[others]).max() + 1e-300))
    crit_moved = float(np.abs(g[case.na:] - g_res[case.na:]).max() / np.abs(g_res[case.na:]).max())
    print(json.dumps({"case": label + " vs residual image", "actor_equal": bool(np.array_equal(g[:case.na], g_res[:case.na])),
                      "actor_max_abs": float(np.abs(g[:case.na] - g_res[:case.na]).max()), "metrics_rel": met_rel,
                      "critic_moved": crit_moved}))
    assert np.array_equal(g[:case.na], g_res[:case.na])
    assert met_rel <= 1e-12
    assert crit_moved >= 10 * tol


@pytest.mark.parametrize("precision", PRECISIONS)
def test_back_to_back_minibatches_rezero_the_sample_counts(cuda, precision):
    """Two minibatches on one stream into the same outputs, rows [37, 137) and [97, 197) of one permutation over 34
    samples (they share samples: asserted). The plain critic's last launch forms no factored product but must
    still zero the stream's per-sample counts: stale counts would double the second minibatch's row weights. The
    second's value loss and critic gradients against the oracle on its own rows."""
    rows, N, second = 100, 34, UR.START + 60
    case = UR._Case(cuda, precision, HOPPER_PLAIN_CRITIC, N, lp=_lp(precision))
    b1, b2 = FT._rows_of(case, UR.START, rows)[0], FT._rows_of(case, second, rows)[0]
    assert len(set(b1) & set(b2)) > 10
    out = FT._Out(case, rows)
    FT._launch(case, out, UR.START, rows)
    FT._launch(case, out, second, rows)
    g, m = out.read()
    met_ref, ga_ref, gc_ref = FT._oracle(case, second, rows)
    tol = UR.TOL[precision]
    print(json.dumps({"case": f"plain-critic-back-to-back-{precision}", "v_loss": float(m[1] / rows), "ref": met_ref["v_loss"]}))
    assert abs(m[1] / rows - met_ref["v_loss"]) < tol * (abs(met_ref["v_loss"]) + 1e-2)
    UR._check_errs(UR._tensor_errs(case.d, g, ga_ref, gc_ref), tol, f"plain-critic-back-to-back-{precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_critic_part_matches_whole(cuda, precision):
    """dppo_ppo_minibatch_part's critic half (part 2) alone against the whole minibatch, 150 rows: the critic's
    gradient range within test_ft20_parts_match_whole's bounds (median 1e-6, max 5e-3 absolute), v_loss 1e-3
    relative, and the part against the oracle; the part leaves the actor's range and the other metrics untouched."""
    rows = FT.ROWS
    case = UR._Case(cuda, precision, HOPPER_PLAIN_CRITIC, FT.NSAMP, lp=_lp(precision))
    whole, part = FT._Out(case, rows), FT._Out(case, rows, fill=7.0)
    FT._launch(case, whole, UR.START, rows)
    gw, mw = whole.read()
    FT._launch(case, part, UR.START, rows, part=2)
    gp, mp = part.read()
    assert (gp[:case.na] == 7.0).all() and (np.delete(mp, 1) == 7.0).all()
    _, _, gc_ref = FT._oracle(case, UR.START, rows)
    UR._check_errs(UR._tensor_errs(case.d, gp, {}, gc_ref), UR.TOL[precision], f"plain-critic-part-{precision}", only="critic.")
    diff = np.abs(gp[case.na:] - gw[case.na:])
    print(json.dumps({"case": f"plain-critic part vs whole {precision}", "median": float(np.median(diff)),
                      "max": float(diff.max()), "v_loss": [float(mp[1]), float(mw[1])]}))
    assert np.median(diff) < 1e-6 and diff.max() < 5e-3
    assert abs(mp[1] - mw[1]) <= 1e-3 * (abs(mw[1]) + 1e-3)


# ------------------------------------------------------------------------------------------------
# pack and optimizer steps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("form", ["staged", "fused"])
def test_optimizer_steps_keep_the_plain_critic_image(cuda, precision, form):
    """Three AdamW steps of the critic range (staged, and DPPO_STEP_FUSED_PACK): after each the image is
    byte-identical to a fresh dppo_pack_critic_head pack of the stepped parameters, and its head is still PLAIN:
    dppo_critic_forward on it matches the plain oracle of the stepped parameters at test_critic_forward's bound
    (the residual oracle is ten bounds away, tests/test_critic_plain_cpu.py)."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import ptr, stream_handle
    d, _, _, _, _, _, _, _, pc = KG._setup(HOPPER_PLAIN_CRITIC, cuda)
    n = pc.numel()
    zeros = lambda: torch.zeros(ops.critic_packed_bytes(d, precision), dtype=torch.uint8, device=cuda)
    img = ops.pack_critic(d, pc, precision, out=zeros())
    m, v = torch.zeros_like(pc), torch.zeros_like(pc)
    gen = torch.Generator(device=cuda).manual_seed(3)
    for step in (1, 2, 3):
        grads = torch.randn(n, device=cuda, generator=gen) * 0.01
        mode = ops._step_mode("keras", fused_pack=form == "fused")
        _lib.call("dppo_optimizer_step_ex", ctypes.byref(d.c()), _lib.PRECISION[precision], ptr(pc), ptr(grads), ptr(m), ptr(v),
                  n, step, 1e-3, 0.004, 0.9, 0.999, 1e-7, mode, None, None, ptr(pc), ptr(img), None, None, 0, 0, None, None,
                  0, stream_handle(cuda))
        torch.cuda.synchronize()
        fresh = ops.pack_critic(d, pc, precision, out=zeros())
        torch.cuda.synchronize()
        assert torch.equal(img, fresh), (form, precision, step, int((img != fresh).sum()))
    stepped = ops.unflatten_params(ops.critic_param_spec(d), pc.cpu().numpy())
    err = _forward_err(d, precision, img, stepped, 77, cuda)
    print(json.dumps({"case": f"plain-critic-steps-{form}-{precision}", "err": err, "bound": V_TOL[precision]}))
    assert err < V_TOL[precision]


def test_pack_critic_head_attribute(cuda):
    """A head outside the enum is DPPO_EINVAL; the bytes of a plain pack are those of a residual pack; re-packing
    the same buffer through dppo_pack_critic resets the head: the forward then matches the RESIDUAL oracle, and
    dppo_pack_critic_head(PLAIN) on it the plain one again."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import DppoError, ptr, stream_handle
    precision = "fp32"
    d, _, _, critic, _, _, _, _, pc = KG._setup(HOPPER_PLAIN_CRITIC, cuda)
    res = ops.ModelDims(**HOPPER)
    zeros = lambda: torch.zeros(ops.critic_packed_bytes(d, precision), dtype=torch.uint8, device=cuda)
    img = ops.pack_critic(d, pc, precision, out=zeros())
    assert torch.equal(img, ops.pack_critic(res, pc, precision, out=zeros()))
    with pytest.raises(DppoError, match=re.escape("failed (1): dppo_pack_critic_head: bad head 2")):
        _lib.call("dppo_pack_critic_head", ctypes.byref(d.c()), _lib.PRECISION[precision], 2, ptr(pc), ptr(img), stream_handle(cuda))
    e_plain = _forward_err(d, precision, img, critic, 77, cuda)                      # the refused pack left the head
    _lib.call("dppo_pack_critic", ctypes.byref(d.c()), _lib.PRECISION[precision], ptr(pc), ptr(img), stream_handle(cuda))
    e_res = _forward_err(d, precision, img, critic, 77, cuda, model=O.Model())
    e_cross = _forward_err(d, precision, img, critic, 77, cuda)
    _lib.call("dppo_pack_critic_head", ctypes.byref(d.c()), _lib.PRECISION[precision], 1, ptr(pc), ptr(img), stream_handle(cuda))
    e_back = _forward_err(d, precision, img, critic, 77, cuda)
    print(json.dumps({"case": "plain-critic-attribute", "plain": e_plain, "residual_after_repack": e_res,
                      "plain_oracle_after_repack": e_cross, "plain_again": e_back}))
    assert e_plain < V_TOL[precision] and e_res < V_TOL[precision] and e_back < V_TOL[precision]
    assert e_cross >= 10 * V_TOL[precision]


def test_freed_image_leaves_no_attribute_behind(cuda):
    """The attributes are keyed by the image's address: when a tensor ops.pack_critic / ops.pack_actor packed is
    freed, its entry goes with it (dppo_forget_image), so whatever is allocated at that address next, a clone of a
    residual image for one, reads as never packed. Checked without relying on the allocator: the tensor's
    finalizer is registered once, fires on `del`, and fired by hand on a live plain image it makes that buffer read
    as RESIDUAL (the forward then matches the residual oracle, and the plain one by no less than ten bounds)."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    precision = "fp32"
    d, _, _, critic, _, _, _, pf, pc = KG._setup(dict(HOPPER_PLAIN_CRITIC, head="plain", activation="Mish"), cuda)
    img = ops.pack_critic(d, pc, precision)
    fin = img._dppo_forget
    assert fin.alive and ops.pack_critic(d, pc, precision, out=img)._dppo_forget is fin
    assert _forward_err(d, precision, img, critic, 33, cuda) < V_TOL[precision]
    fin()
    e_res = _forward_err(d, precision, img, critic, 33, cuda, model=O.Model())
    e_plain = _forward_err(d, precision, img, critic, 33, cuda)
    print(json.dumps({"case": "forgotten plain critic image", "residual": e_res, "plain": e_plain}))
    assert e_res < V_TOL[precision] and e_plain >= 10 * V_TOL[precision]
    for pack, params in ((ops.pack_critic, pc), (ops.pack_actor, pf)):
        image = pack(d, params, precision)
        fin = image._dppo_forget
        assert fin.alive
        torch.cuda.synchronize()
        del image
        assert not fin.alive


# ------------------------------------------------------------------------------------------------
# agents
# ------------------------------------------------------------------------------------------------
def test_plain_critic_iteration_matches_oracle(cuda, tmp_path, monkeypatch):
    """An eval and a training iteration of the fp32 agent from ft_ppo_diffusion_mlp_plain_critic.yaml (seed 42, the
    shapes and bounds of tests/test_iteration_gpu.py) against oracle/iteration.py with the plain critic."""
    from diffusionpolicyoptimization_amd.util import config
    from tests import test_iteration_gpu as IT
    load = config.load_config
    monkeypatch.setattr(config, "load_config", lambda root, name, ov: load(root, name + "_plain_critic", ov))
    a, orc = IT._agent_and_oracle(42, tmp_path)
    assert a.model.dims.critic_head == "plain" and a.model.dims.head == "residual"
    errs = IT._run_and_compare(a, orc, n_itr=2)
    print(json.dumps({"case": "plain-critic-iteration", "iterations": errs}))
    assert [e["eval"] for e in errs] == [True, False]


@pytest.mark.parametrize("name,actor_head", [("ft_ppo_diffusion_mlp_plain_critic", "residual"),
                                             ("ft_ppo_diffusion_mlp_plain_both", "plain")])
def test_plain_critic_agent_split_update_matches_fused(cuda, tmp_path, monkeypatch, name, actor_head):
    """TrainPPODiffusionAgent from each new cfg on the synthetic env, two training iterations through the fused and
    through the split update: finite, moved parameters that agree within test_split_update_matches_fused's bounds."""
    import torch
    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("DPPO_SPLIT_UPDATE", flag)
        cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), name,
                          ["model.precision=fp32", "train.n_steps=20", "train.batch_size=200", "train.n_train_itr=2",
                           "train.val_freq=100", f"logdir={tmp_path}/{flag}"])
        a = get_class(cfg._target_)(cfg)
        assert (a.model.dims.critic_head, a.model.dims.head) == ("plain", actor_head)
        p_init = a.model.train_params.cpu().numpy().copy()
        res = a.run()
        torch.cuda.synchronize()
        out[flag] = (a.model.train_params.cpu().numpy().copy(), res[-1], a.timing["n_updates"])
        assert np.isfinite(out[flag][0]).all() and np.abs(out[flag][0][a.model.n_actor:] - p_init[a.model.n_actor:]).max() > 0
    (p1, r1, n1), (p0, r0, n0) = out["1"], out["0"]
    assert n1 == n0
    dlt = np.abs(p1 - p0)
    print(json.dumps({"case": f"{name} split vs fused", "median": float(np.median(dlt)), "max": float(dlt.max())}))
    assert np.median(dlt) < 1e-6 and dlt.max() < 5e-3, (float(np.median(dlt)), float(dlt.max()))
    for k in ("pg_loss", "v_loss"):
        assert abs(r1[k] - r0[k]) <= 1e-3 * (abs(r0[k]) + 1e-3), (k, r1[k], r0[k])
