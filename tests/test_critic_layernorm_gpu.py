"""Layer-normed critic on the GPU: the entries that take a packed critic image, against the oracle's layer-normed
critic (O.Model(critic_head=..., critic_layernorm=True), derived from the dims).

Hopper dims (SD = 11, HC = 256) at fp32, bf16 and fp16, both heads. The critic is tests/test_critic_layernorm_cpu.py's
ln_models: random gamma ~ U(0.5, 1.5), beta ~ N(0, 1), W_in times 3, so that every hidden row's variance is at least
100 epsilon at every site (asserted on the oracle's side in each comparison). Bounds are those of the corresponding
cases of tests/test_critic_plain_gpu.py, unchanged: V 1e-4 / 1e-3 / 1e-3 of 1 + max|V|, the gradients per tensor
2e-3 fp32 and 1e-2 2-byte (ln*_g / ln*_b take the same), a part against the whole median 1e-6 / max 5e-3, the
iteration tests/test_iteration_gpu.py's. Every figure is printed as a JSON line before it is asserted."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from oracle import philox as PX
from tests import test_critic_layernorm_cpu as LC
from tests import test_kernels_gpu as KG
from tests import test_update_ft_steps_gpu as FT
from tests import test_update_regimes_gpu as UR
from tests import test_update_surface_gpu as US
from tests.helpers import HOPPER, to_f64
from tests.variants import HOPPER_LN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V_TOL = LC.V_TOL
PRECISIONS = ["fp32", "bf16", "fp16"]
HEADS = LC.HEADS
LN_NAMES = {"residual": ["ln1_g", "ln1_b", "ln2_g", "ln2_b"], "plain": ["ln1_g", "ln1_b", "ln2_g", "ln2_b", "ln3_g", "ln3_b"]}


@pytest.fixture
def ln(monkeypatch):
    """ln_models in place of make_models for the shared case classes."""
    for mod in (KG, US):
        monkeypatch.setattr(mod, "make_models", LC.ln_models)


def _lp(precision):
    return "perturbed" if precision == "fp32" else "ratio1"


def _off(head):
    """The dims of the same head without layer norm."""
    return dict(HOPPER, critic_head=head)


def _flat_critic(d, critic, cuda):
    import torch
    from diffusionpolicyoptimization_amd import ops
    return torch.tensor(ops.flatten_params(ops.critic_param_spec(d), critic), device=cuda)


def _forward_err(d, precision, img, critic, state, cuda, head=None, min_var=100.0):
    """max|V - ref| / (1 + max|ref|) of dppo_critic_forward against the layer-norm oracle; the element behind
    `values` must stay as it was."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    n = state.shape[0]
    ref, cache = O.critic_forward(to_f64(critic), state.astype(np.float64), O.Model.from_dims(d), rnd=KG._rnd(precision))
    if head is not None:
        LC.assert_variance(cache, head, min_var)
    buf = torch.full((n + 1,), 7.5, dtype=torch.float32, device=cuda)
    v = ops.critic_forward(d, precision, img, torch.tensor(state.reshape(n, -1).astype(np.float32), device=cuda), values=buf[:n])
    torch.cuda.synchronize()
    assert float(buf[n]) == 7.5
    v = v.cpu().numpy()
    assert v.shape == (n,) and np.isfinite(v).all()
    return float(np.abs(v - ref[:, 0]).max() / (1 + np.abs(ref).max()))


# ------------------------------------------------------------------------------------------------
# dppo_critic_forward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 33, 77])
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_critic_forward_matches_ln_oracle(cuda, ln, precision, head, n):
    """n = 1 (one lane, 31 padded rows), 31 (one short of a 32-row tile), 33 (one over), 77 (a partial third tile)."""
    from diffusionpolicyoptimization_amd import ops
    d, _, _, critic, _, _, _, _, pc = KG._setup(HOPPER_LN[head], cuda)
    err = _forward_err(d, precision, ops.pack_critic(d, pc, precision), critic, LC.states77()[:n], cuda, head)
    print(json.dumps({"case": f"ln-critic-forward-{head}-{precision}-n{n}", "err": err, "bound": V_TOL[precision]}))
    assert err < V_TOL[precision]


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_critic_forward_uses_the_heads_epsilon(cuda, ln, precision, head):
    """near_eps_critic (first-site variance near 1e-3): the other head's epsilon is ten bounds away on these inputs
    (tests/test_critic_layernorm_cpu.py), so only the right one passes."""
    from diffusionpolicyoptimization_amd import ops
    d = ops.ModelDims(**HOPPER_LN[head])
    critic = LC.near_eps_critic(head)
    img = ops.pack_critic(d, _flat_critic(d, critic, cuda), precision)
    err = _forward_err(d, precision, img, critic, LC.states77(), cuda)
    print(json.dumps({"case": f"ln-critic-forward-near-eps-{head}-{precision}", "err": err, "bound": V_TOL[precision]}))
    assert err < V_TOL[precision]


# ------------------------------------------------------------------------------------------------
# dppo_ppo_minibatch
# ------------------------------------------------------------------------------------------------
def _with_unnormed_critic(case, head, fn):
    """fn() with the case's critic swapped for the same eight tensors without layer norm (image and dims)."""
    from diffusionpolicyoptimization_amd import ops
    keep = (case.d, case.packc, case.nc, case.pc)
    case.d = ops.ModelDims(**_off(head))
    case.nc = ops.spec_count(ops.critic_param_spec(case.d))
    case.pc = keep[3][:case.nc].clone()
    case.packc = ops.pack_critic(case.d, case.pc, case.precision)
    try:
        return fn()
    finally:
        case.d, case.packc, case.nc, case.pc = keep


def _index(case, rows):
    import torch
    return torch.tensor(PX.feistel_permute(np.arange(UR.START + rows), case.total, UR.SEED, UR.EPOCH).astype(np.int64),
                        device=case.cuda)


def _assert_rows_variance(case, head, bi):
    _, cache = O.critic_forward(to_f64(case.critic), case.obs[np.unique(bi)].reshape(-1, 1, 11).astype(np.float64),
                                case.model, rnd=KG._rnd(case.precision))
    return LC.assert_variance(cache, head)


# (label, rows, samples, explicit row_index, clipped value loss)
GRAD_REGIMES = {"r77-index": (77, 34, True, False), "r100": (100, 34, False, False), "r1600": (1600, 170, False, False),
                "r100-clipv": (100, 34, False, True)}
GRAD_CASES = [(p, h, r) for r in ("r77-index", "r100", "r1600") for h in HEADS for p in PRECISIONS] + \
             [("bf16", h, "r100-clipv") for h in HEADS]


@pytest.mark.parametrize("precision,head,regime", GRAD_CASES, ids=[f"{p}-{h}-{r}" for p, h, r in GRAD_CASES])
def test_ppo_minibatch_critic_grads_match_ln_oracle(cuda, ln, precision, head, regime):
    """One whole dppo_ppo_minibatch with a layer-normed critic image: the value loss and every critic gradient
    tensor, ln*_g / ln*_b included, against O.c_loss with the layer-normed critic.
      r77-index:  77 rows (a partial third tile: padded rows) through an explicit row_index;
      r100:       100 rows over 34 samples: every sample about three times, so the dedup multiplicities run;
      r1600:      1,600 rows over 170 samples: two dW m-chunks on the host's plan, re-cut on the device over the
                  distinct samples (tests/test_critic_plain_gpu.py's case);
      r100-clipv: the clipped value loss (clip_vloss_coef 0.2), once per head.
    The same call on an image of the same eight tensors without layer norm must leave the actor's gradient range
    bit-equal and move the critic's."""
    from diffusionpolicyoptimization_amd import ops
    rows, N, use_index, clipv = GRAD_REGIMES[regime]
    case = UR._Case(cuda, precision, HOPPER_LN[head], N, lp=_lp(precision))
    assert case.d.critic_layernorm and case.nc == ops.spec_count(ops.critic_param_spec(ops.ModelDims(**_off(head)))) + \
        256 * len(LN_NAMES[head])
    if clipv:
        case.old_values()
    bi, _ = case.rows_of(rows)
    mult = np.unique(bi, return_counts=True)[1]
    assert mult.max() > 1 and len(mult) < rows
    min_var = _assert_rows_variance(case, head, bi)
    plan = ops.ppo_plan(case.d, precision, rows)
    if rows == 1600:
        assert plan["dw_chunks_critic"] == 2 and UR._device_chunks(len(mult), 1600, 2) == (128, 2)
    stats, mean_std = case.adv_stats(rows)
    met_ref, ga_ref, gc_ref = case.oracle(rows, adv_mean_std=mean_std)
    kw = dict(stats=stats, row_index=_index(case, rows) if use_index else None)
    g, m = case.launch(rows, UR.START, rows, **kw)
    assert np.isfinite(g).all() and np.isfinite(m).all()
    tol = UR.TOL[precision]
    label = f"ln-critic-{head}-{precision}-{regime}"
    UR._check_metrics(m / rows, met_ref, tol, precision != "fp32", label)
    errs = UR._tensor_errs(case.d, g, ga_ref, gc_ref)
    assert {"critic." + n for n in LC.EIGHT + LN_NAMES[head]} <= set(errs)
    print(json.dumps({"case": label, "min_var": min_var}))
    UR._check_errs(errs, tol, label)
    g_off, _ = _with_unnormed_critic(case, head, lambda: case.launch(rows, UR.START, rows, **kw))
    n8 = len(g_off) - case.na
    crit_moved = float(np.abs(g[case.na:case.na + n8] - g_off[case.na:]).max() / np.abs(g_off[case.na:]).max())
    print(json.dumps({"case": label + " vs image without layer norm", "actor_equal": bool(np.array_equal(g[:case.na], g_off[:case.na])),
                      "critic_moved": crit_moved}))
    assert np.array_equal(g[:case.na], g_off[:case.na])
    assert crit_moved >= 10 * tol


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_back_to_back_minibatches_start_from_zero_dgamma(cuda, ln, precision, head):
    """Two minibatches on one stream into the same outputs (shared samples: asserted): the second must start from
    zeroed dgamma / dbeta, which the tiles accumulate with atomics. Its value loss and critic gradients against the
    oracle on its own rows, and the actor's gradients bit-equal to the same two launches on an image without layer
    norm. Then the same second minibatch's critic half under DPPO_PPO_PRECLEARED after an optimizer
    step with DPPO_STEP_CLEAR_GRADS over the critic range (lr 0: the parameters stay) and the part's clear ranges."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    rows, N, second = 100, 34, UR.START + 60
    case = UR._Case(cuda, precision, HOPPER_LN[head], N, lp=_lp(precision))
    b1, b2 = FT._rows_of(case, UR.START, rows)[0], FT._rows_of(case, second, rows)[0]
    assert len(set(b1) & set(b2)) > 10
    _assert_rows_variance(case, head, np.concatenate([b1, b2]))
    out = FT._Out(case, rows)
    FT._launch(case, out, UR.START, rows)
    FT._launch(case, out, second, rows)
    g, m = out.read()
    met_ref, ga_ref, gc_ref = FT._oracle(case, second, rows)
    tol = UR.TOL[precision]
    label = f"ln-critic-back-to-back-{head}-{precision}"
    print(json.dumps({"case": label, "v_loss": float(m[1] / rows), "ref": met_ref["v_loss"]}))
    assert abs(m[1] / rows - met_ref["v_loss"]) < tol * (abs(met_ref["v_loss"]) + 1e-2)
    UR._check_errs(UR._tensor_errs(case.d, g, ga_ref, gc_ref), tol, label)

    def unnormed_pair():   # the same two launches on an image of the same eight tensors without the norm
        o = FT._Out(case, rows)
        FT._launch(case, o, UR.START, rows)
        FT._launch(case, o, second, rows)
        return o.read()[0]
    g_off = _with_unnormed_critic(case, head, unnormed_pair)
    assert np.array_equal(g[:case.na], g_off[:case.na])                  # the actor's gradients: bit-equal
    # pre-cleared: the critic's step clears its gradient range (tail included) and the part's ranges
    FT._launch(case, out, UR.START, rows, part=2)
    mm, vv = torch.zeros_like(case.pc), torch.zeros_like(case.pc)
    step = ops.BoundOptimizerStep(case.d, precision, case.pc, out.grads[case.na:], mm, vv, 0.0, 0.9, 0.999, 1e-7, "keras",
                                  critic_params=case.pc, packed_critic=case.packc, fused_pack=True, clear_grads=True)
    before = case.pc.clone()
    step(1, 0.0, clear=ops.ClearRanges(case.d, precision, rows, out.ws, out.met, 2))
    torch.cuda.synchronize()
    assert torch.equal(case.pc, before) and float(out.grads[case.na:].abs().max()) == 0.0
    FT._launch(case, out, second, rows, part=2, precleared=True)
    gp, mp = out.read()
    UR._check_errs(UR._tensor_errs(case.d, gp, {}, gc_ref), tol, label + "-precleared", only="critic.")
    assert abs(mp[1] / rows - met_ref["v_loss"]) < tol * (abs(met_ref["v_loss"]) + 1e-2)


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_critic_part_matches_whole(cuda, ln, precision, head):
    """dppo_ppo_minibatch_part's critic half alone against the whole minibatch, 150 rows: the critic's gradient range,
    tail included, within test_ft20_parts_match_whole's bounds, and the part against the oracle; the part leaves the
    actor's range and the other metrics untouched, and the whole's actor gradients are bit-equal to the same call on an
    image without layer norm."""
    rows = FT.ROWS
    case = UR._Case(cuda, precision, HOPPER_LN[head], FT.NSAMP, lp=_lp(precision))
    whole, part = FT._Out(case, rows), FT._Out(case, rows, fill=7.0)
    FT._launch(case, whole, UR.START, rows)
    gw, mw = whole.read()
    FT._launch(case, part, UR.START, rows, part=2)
    gp, mp = part.read()
    assert (gp[:case.na] == 7.0).all() and (np.delete(mp, 1) == 7.0).all()
    _, _, gc_ref = FT._oracle(case, UR.START, rows)
    UR._check_errs(UR._tensor_errs(case.d, gp, {}, gc_ref), UR.TOL[precision], f"ln-critic-part-{head}-{precision}", only="critic.")
    diff = np.abs(gp[case.na:] - gw[case.na:])
    print(json.dumps({"case": f"ln-critic part vs whole {head} {precision}", "median": float(np.median(diff)),
                      "max": float(diff.max())}))
    assert np.median(diff) < 1e-6 and diff.max() < 5e-3
    assert abs(mp[1] - mw[1]) <= 1e-3 * (abs(mw[1]) + 1e-3)

    def unnormed_whole():   # the whole minibatch on an image of the same eight tensors without the norm
        o = FT._Out(case, rows)
        FT._launch(case, o, UR.START, rows)
        return o.read()[0]
    g_off = _with_unnormed_critic(case, head, unnormed_whole)
    assert np.array_equal(gw[:case.na], g_off[:case.na])                 # the actor's gradients: bit-equal


# ------------------------------------------------------------------------------------------------
# pack, optimizer steps, attributes, refusals
# ------------------------------------------------------------------------------------------------
def _step_ex(d, precision, pc, grads, m, v, step, mode, img, cuda, n=None):
    from diffusionpolicyoptimization_amd import _lib
    from diffusionpolicyoptimization_amd._lib import ptr, stream_handle
    return _lib.load().dppo_optimizer_step_ex(
        ctypes.byref(d.c()), _lib.PRECISION[precision], ptr(pc), ptr(grads), ptr(m), ptr(v), pc.numel() if n is None else n, step,
        1e-3, 0.004, 0.9, 0.999, 1e-7, mode, None, None, ptr(pc), ptr(img), None, None, 0, 0, None, None, 0, stream_handle(cuda))


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("form", ["staged", "fused"])
def test_optimizer_steps_keep_the_ln_critic_image(cuda, ln, precision, form, head):
    """Three AdamW steps of the critic range, tail included (staged, and DPPO_STEP_FUSED_PACK; the third through the
    clip entry with per-variable scales): after each the image is byte-identical to a fresh dppo_pack_critic_ln pack
    of the stepped parameters, gamma and beta moved (decayed like every variable), and the attribute survived:
    dppo_critic_forward on the image matches the layer-norm oracle of the stepped parameters."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    d, _, _, _, _, _, _, _, pc = KG._setup(HOPPER_LN[head], cuda)
    n, n8 = pc.numel(), ops.spec_count(ops.critic_param_spec(ops.ModelDims(**_off(head))))
    zeros = lambda: torch.zeros(ops.critic_packed_bytes(d, precision), dtype=torch.uint8, device=cuda)
    img = ops.pack_critic(d, pc, precision, out=zeros())
    tail0 = pc[n8:].clone()
    m, v = torch.zeros_like(pc), torch.zeros_like(pc)
    gen = torch.Generator(device=cuda).manual_seed(3)
    for step in (1, 2, 3):
        grads = torch.randn(n, device=cuda, generator=gen) * 0.01
        if step < 3:
            assert _step_ex(d, precision, pc, grads, m, v, step, ops._step_mode("keras", fused_pack=form == "fused"), img, cuda) == 0
        else:
            norms, scales = ops.grad_clip_scales(d, "critic", grads, 0.05)
            assert scales.numel() == 8 + len(LN_NAMES[head]) and float(scales.min()) < 1.0
            ops.BoundOptimizerStep(d, precision, pc, grads, m, v, 0.004, 0.9, 0.999, 1e-7, "keras", critic_params=pc,
                                   packed_critic=img, fused_pack=form == "fused", clip_scales=scales)(step, 1e-3)
        torch.cuda.synchronize()
        fresh = ops.pack_critic(d, pc, precision, out=zeros())
        torch.cuda.synchronize()
        assert torch.equal(img, fresh), (form, precision, step, int((img != fresh).sum()))
    assert float((pc[n8:] - tail0).abs().min()) > 0
    stepped = ops.unflatten_params(ops.critic_param_spec(d), pc.cpu().numpy())
    err = _forward_err(d, precision, img, stepped, LC.states77(), cuda)
    print(json.dumps({"case": f"ln-critic-steps-{form}-{head}-{precision}", "err": err, "bound": V_TOL[precision]}))
    assert err < V_TOL[precision]


@pytest.mark.parametrize("head", HEADS)
def test_attribute_is_reset_by_repacking_and_forgetting(cuda, ln, head):
    """The leading bytes of a layer-normed pack are those of a pack of the same eight tensors. dppo_pack_critic /
    dppo_pack_critic_head on the buffer record no layer norm, and so does dppo_forget_image: the forward then
    matches the oracle WITHOUT the norm (and the layer-norm oracle by no less than ten bounds); dppo_pack_critic_ln
    on it brings the norm back."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import ptr, stream_handle
    precision = "fp32"
    d, _, _, critic, _, _, _, _, pc = KG._setup(HOPPER_LN[head], cuda)
    doff = ops.ModelDims(**_off(head))
    n8, b8 = ops.spec_count(ops.critic_param_spec(doff)), ops.critic_packed_bytes(doff, precision)
    zeros = lambda dd: torch.zeros(ops.critic_packed_bytes(dd, precision), dtype=torch.uint8, device=cuda)   # (the segments' padding)
    img = ops.pack_critic(d, pc, precision, out=zeros(d))
    assert img.numel() == b8 + 4 * 256 * len(LN_NAMES[head])
    assert torch.equal(img[:b8], ops.pack_critic(doff, pc[:n8].clone(), precision, out=zeros(doff)))
    assert torch.equal(img[b8:].view(torch.float32), pc[n8:])
    state = LC.states77()
    eight = {k: critic[k] for k in LC.EIGHT}

    def errs():
        v = ops.critic_forward(d, precision, img, torch.tensor(state.reshape(77, -1).astype(np.float32), device=cuda)).cpu().numpy()
        r_ln = O.critic_forward(to_f64(critic), state, O.Model.from_dims(d))[0][:, 0]
        r_off = O.critic_forward(to_f64(eight), state, O.Model(critic_head=head))[0][:, 0]
        return (float(np.abs(v - r_ln).max() / (1 + np.abs(r_ln).max())), float(np.abs(v - r_off).max() / (1 + np.abs(r_off).max())))

    tol = V_TOL[precision]
    e = errs()
    assert e[0] < tol and e[1] >= 10 * tol, e
    hd = _lib.HEAD[head]
    _lib.call("dppo_pack_critic_head", ctypes.byref(d.c()), 0, hd, ptr(pc), ptr(img), stream_handle(cuda))
    e = errs()
    assert e[1] < tol and e[0] >= 10 * tol, e
    _lib.call("dppo_pack_critic_ln", ctypes.byref(d.c()), 0, hd, 1, ptr(pc), ptr(img), stream_handle(cuda))
    assert errs()[0] < tol
    _lib.call("dppo_forget_image", ptr(img))
    e = errs()
    v = ops.critic_forward(d, precision, img, torch.tensor(state.reshape(77, -1).astype(np.float32), device=cuda)).cpu().numpy()
    r = O.critic_forward(to_f64(eight), state)[0][:, 0]                       # forgotten: RESIDUAL, no layer norm
    assert float(np.abs(v - r).max() / (1 + np.abs(r).max())) < tol and e[0] >= 10 * tol
    ops.pack_critic(d, pc, precision, out=img)
    assert errs()[0] < tol
    if head == "residual":   # dppo_pack_critic itself
        _lib.call("dppo_pack_critic", ctypes.byref(d.c()), 0, ptr(pc), ptr(img), stream_handle(cuda))
        e = errs()
        assert e[1] < tol and e[0] >= 10 * tol, e


def test_refusals_leave_outputs_untouched(cuda, ln):
    """An attribute outside its enum is DPPO_EINVAL in every entry that takes one, the image's attributes kept;
    an optimizer range sized for the other layout is refused in both directions with the parameters, moments and
    image unchanged; the Python surface refuses tensors sized for the other layout."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import DppoError, ptr, stream_handle
    precision, head = "fp32", "plain"
    d, _, _, critic, _, _, _, _, pc = KG._setup(HOPPER_LN[head], cuda)
    doff = ops.ModelDims(**_off(head))
    n8 = ops.spec_count(ops.critic_param_spec(doff))
    img = ops.pack_critic(d, pc, precision)
    img0, pc0 = img.clone(), pc.clone()
    with pytest.raises(DppoError, match=re.escape("failed (1): dppo_pack_critic_ln: bad layernorm 2")):
        _lib.call("dppo_pack_critic_ln", ctypes.byref(d.c()), 0, 1, 2, ptr(pc), ptr(img), stream_handle(cuda))
    with pytest.raises(DppoError, match=re.escape("failed (1): dppo_pack_critic_head: bad head 2")):
        _lib.call("dppo_pack_critic_ln", ctypes.byref(d.c()), 0, 2, 1, ptr(pc), ptr(img), stream_handle(cuda))
    g = torch.randn(pc.numel(), device=cuda)
    sc, ws = torch.full((26,), 3.0, device=cuda), torch.zeros(64, dtype=torch.float64, device=cuda)
    with pytest.raises(DppoError, match="bad layernorm 3"):
        _lib.call("dppo_grad_clip_scales_ln", ctypes.byref(d.c()), 2, 1, 3, ptr(g), 1.0, None, ptr(sc), ptr(ws), stream_handle(cuda))
    met = torch.zeros(16, dtype=torch.float64, device=cuda)
    wsp = ops.ppo_workspace(d, precision, 100, cuda)
    ptrs, nbytes, cnt = (ctypes.c_void_p * 4)(), (ctypes.c_size_t * 4)(), ctypes.c_int(0)
    with pytest.raises(DppoError, match="bad head 5"):
        _lib.call("dppo_ppo_clear_ranges_ln", ctypes.byref(d.c()), 0, 5, 1, 100, ptr(wsp), ptr(met), 2, ptrs, nbytes, ctypes.byref(cnt))
    torch.cuda.synchronize()
    assert torch.equal(img, img0) and (sc == 3.0).all()
    assert _forward_err(d, precision, img, critic, LC.states77(), cuda) < V_TOL[precision]      # attributes kept
    # the clear ranges of a layer-normed critic are the plain form's (the tail is in the gradient range)
    a, b = ops.ClearRanges(d, precision, 100, wsp, met, 2).ranges(), ops.ClearRanges(doff, precision, 100, wsp, met, 2).ranges()
    assert a == b and len(a) == 2
    # the optimizer range: a layer-normed image with a range without the tail, staged and fused
    m, v = torch.zeros_like(pc), torch.zeros_like(pc)
    for fused in (False, True):
        rc = _step_ex(d, precision, pc, g, m, v, 1, ops._step_mode("keras", fused_pack=fused), img, cuda, n=n8)
        assert rc == 1 and "sized for the layout without the tail" in _lib.load().dppo_last_error().decode()
    # ... and an image without layer norm with a layer-normed critic's range
    img8 = ops.pack_critic(doff, pc[:n8].clone(), precision)
    img8_0 = img8.clone()
    rc = _step_ex(doff, precision, pc, g, m, v, 1, ops._step_mode("keras", fused_pack=True), img8, cuda)
    assert rc == 1 and "has no layer norm" in _lib.load().dppo_last_error().decode()
    # a clipped range that is not the layout's: the critic alone under nets = 3 (actor | critic)
    with pytest.raises(DppoError, match="the range must be exactly the network"):
        _lib.call("dppo_optimizer_step_clip", ctypes.byref(d.c()), 0, ptr(pc), ptr(g), ptr(m), ptr(v), pc.numel(), 1, 1e-3, 0.004,
                  0.9, 0.999, 1e-7, 0, None, None, ptr(pc), ptr(img), None, None, 0, 0, None, None, 0, stream_handle(cuda), ptr(sc), 3)
    torch.cuda.synchronize()
    assert torch.equal(pc, pc0) and torch.equal(img, img0) and torch.equal(img8, img8_0)
    assert float(m.abs().max()) == 0 and float(v.abs().max()) == 0
    # Python: every tensor is checked against the spec
    with pytest.raises(ValueError, match="critic params"):
        ops.pack_critic(d, pc[:n8].clone(), precision)
    with pytest.raises(ValueError, match="critic params"):
        ops.pack_critic(doff, pc, precision)
    with pytest.raises(ValueError, match="packed critic"):
        ops.pack_critic(d, pc, precision, out=img8)
    with pytest.raises(ValueError, match="packed_critic"):
        ops.critic_forward(d, precision, img8, torch.zeros(3, 11, device=cuda))
    with pytest.raises(ValueError, match="grads"):
        ops.BoundGradClip(d, "critic", g[:n8], 1.0)


def test_layer_norm_off_is_todays_layout(cuda):
    """With layer norm off, ModelDims, the spec count, the packed bytes and the image bytes equal today's, through
    dppo_pack_critic_ln(LN_OFF) as through dppo_pack_critic_head."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import ptr, stream_handle
    for head in HEADS:
        d = ops.ModelDims(**_off(head))
        _, _, _, _, _, _, _, _, pc = KG._setup(_off(head), cuda)
        assert d == ops.ModelDims(**dict(_off(head), critic_layernorm=False))
        for precision in PRECISIONS:
            c = d.c()
            nb = _lib.query("dppo_critic_packed_bytes", ctypes.byref(c), _lib.PRECISION[precision])
            assert ops.critic_packed_bytes(d, precision) == nb and pc.numel() == _lib.query("dppo_critic_param_count", ctypes.byref(c))
            a = ops.pack_critic(d, pc, precision, out=torch.zeros(nb, dtype=torch.uint8, device=cuda))   # (the segments' padding)
            b = torch.zeros_like(a)
            _lib.call("dppo_pack_critic_head", ctypes.byref(c), _lib.PRECISION[precision], _lib.HEAD[head], ptr(pc), ptr(b), stream_handle(cuda))
            torch.cuda.synchronize()
            assert a.numel() == nb and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
# agents
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,head", [("_critic_ln", "residual"), ("_plain_critic_ln", "plain")])
def test_ln_critic_iteration_matches_oracle(cuda, tmp_path, monkeypatch, name, head):
    """An eval and a training iteration of the fp32 agent from each new cfg (seed 42, the shapes and bounds of
    tests/test_iteration_gpu.py) against oracle/iteration.py with the model's critic."""
    from diffusionpolicyoptimization_amd.util import config
    from tests import test_iteration_gpu as IT
    load = config.load_config
    monkeypatch.setattr(config, "load_config", lambda root, nm, ov: load(root, nm + name, ov))
    a, orc = IT._agent_and_oracle(42, tmp_path)
    assert (a.model.dims.critic_head, a.model.dims.critic_layernorm) == (head, True)
    assert [n for n, _ in a.model.critic_spec][8:] == LN_NAMES[head]
    errs = IT._run_and_compare(a, orc, n_itr=2)
    print(json.dumps({"case": f"ln-critic-iteration-{head}", "iterations": errs}))
    assert [e["eval"] for e in errs] == [True, False]


@pytest.mark.parametrize("name,head", [("ft_ppo_diffusion_mlp_critic_ln", "residual"),
                                       ("ft_ppo_diffusion_mlp_plain_critic_ln", "plain")])
def test_ln_critic_agent_runs_and_checkpoints(cuda, tmp_path, name, head):
    """TrainPPODiffusionAgent from each new cfg on the synthetic env, two training iterations at the cfg's
    precision: finite losses, moved gamma / beta; its .npz checkpoint holds the tail under the spec's names, loads
    back bit-equal, and is refused by an agent whose critic has no layer norm (and the other way round); the
    Keras .h5 file maps gamma / beta and does the same."""
    import torch
    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    ov = ["train.n_steps=20", "train.batch_size=200", "train.n_train_itr=2", "train.val_freq=100"]
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), name, ov + [f"logdir={tmp_path}/ln"])
    a = get_class(cfg._target_)(cfg)
    m = a.model
    assert (m.dims.critic_head, m.dims.critic_layernorm) == (head, True)
    n8 = m.n_critic - 256 * len(LN_NAMES[head])
    tail0 = m.critic_params[n8:].cpu().numpy().copy()
    assert set(np.unique(tail0)) == {0.0, 1.0}
    res = a.run()
    torch.cuda.synchronize()
    p = m.train_params.cpu().numpy()
    assert np.isfinite(p).all() and all(np.isfinite(res[-1][k]) for k in ("pg_loss", "v_loss"))
    assert np.abs(p[m.n_actor + n8:] - tail0).min() > 0
    path = str(tmp_path / "ln.npz")
    m.save_weights(path)
    with np.load(path) as f:
        assert {"critic." + n for n in LN_NAMES[head]} <= set(f.files)
    m.critic_params.zero_()
    m.load_weights(path)
    assert np.array_equal(m.train_params.cpu().numpy(), p)
    h5 = str(tmp_path / "ln.weights.h5")
    m.save_weights(h5)
    m.critic_params.zero_()
    m.load_weights(h5)
    assert np.array_equal(m.train_params.cpu().numpy(), p)
    base = "ft_ppo_diffusion_mlp" + ("_plain_critic" if head == "plain" else "")
    b = get_class(cfg._target_)(load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), base, ov + [f"logdir={tmp_path}/off"]))
    with pytest.raises(ValueError, match="holds a layer-normed critic"):
        b.model.load_weights(path)
    off = str(tmp_path / "off.npz")
    b.model.save_weights(off)
    with pytest.raises(ValueError, match="holds a critic without layer norm"):
        m.load_weights(off)
    with pytest.raises(ValueError, match="PPODiffusion model"):       # the norms are datasets the model does not read
        b.model.load_weights(h5)
    off5 = str(tmp_path / "off.weights.h5")
    b.model.save_weights(off5)
    with pytest.raises(ValueError, match="missing critic variables"):
        m.load_weights(off5)
