"""The optimizer step (csrc/optimizer.hip) against the float64 oracle, per tensor and geometry.

Every kernel family of the file — adamw_kernel, adamw_fused_kernel, actor_tile_step_kernel, the virtual
l2 gradient and the clipped instantiations — is compared with O.keras_adamw_step / O.torch_adamw_step one
step at a time from identical inputs (tests/helpers.py adamw_oracle, which states the bounds): the
oracle starts from the GPU's own fp32 (p, m, v, g) before the step and takes the fp32-rounded
hyperparameters the kernel receives, so nothing accumulates over a run of steps and the bound is a few
roundings per quantity (C = 8, u = 2^-24), not the 1e-5 of test_adamw.
tests/test_optimizer_step_cpu.py shows on the CPU that a NumPy fp32 emulation of adamw_elem stays under
half of every bound and that each listed mistake moves the oracle past ten times it.

1. dppo_adamw over mode x hyperparameter set (STEP_HP) x step number (STEP_NUMBERS) x size; the last
   size, 2 * 4096 * 256 + 5, is the smallest at which the grid-stride loop (4096 workgroups of 256)
   takes a second and a partial third trip.
2. every form of dppo_optimizer_step_ex / _clip (FORMS) at the geometries of GEOMETRIES, in fp32, bf16 and
   fp16: parameters and moments per tensor, the image byte-identical to a fresh pack, the gradients and
   the clear ranges zeroed exactly where the flags say, three steps in a row on one stream.
3. the metrics copy at n_metrics 0, 1 and 256, its tag, and its refusals.

Accept / refuse table of the optimizer step (what ran on an MI355X; the host arithmetic is
test_step_table_matches_host_arithmetic in tests/test_optimizer_step_cpu.py). The step has no
per-geometry instantiations: the tile kernels take K, N and the k-steps as arguments, so it runs wherever
dppo_check_dims and the pack accept the model, including geometries whose row tiles are refused
(tests/test_update_surface_gpu.py: ah256 / cond2-walker / tiny in fp32):

  geometry                                   fp32   bf16   fp16
  hopper (XD 12, 39 inputs)                  runs   runs   runs
  walker (XD 24, 57 inputs)                  runs   runs   runs
  h8a4 (XD 32, the bound)                    runs   runs   runs
  td32 (time_dim 32, 55 inputs)              runs   runs   runs
  ah256 (actor_hidden 256)                   runs   runs   runs
  cond2-walker (SD 34, 74 inputs)            runs   runs   runs
  tiny (XD 4, 23 inputs)                     runs   runs   runs

A refused case must raise DppoError before anything is written (parameters, moments, gradients, images
and clear ranges bit-identical to before the call); the table must agree with what the library did.
"""
import ctypes
import json

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests.helpers import (HOPPER, STEP_HP, STEP_NUMBERS, U32, WALKER, adamw_oracle, make_models, step_hp, step_inputs,
                           step_ratios)
from tests.test_update_surface_gpu import GEOMETRIES as SURFACE

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


# ------------------------------------------------------------------------------------------------
# 1. dppo_adamw
# ------------------------------------------------------------------------------------------------
SIZES = (1, 255, 256, 257, 100003)
GRID_STRIDE_N = 2 * 4096 * 256 + 5
ADAMW_PARAMS = [(mode, hp, n) for mode in ("keras", "torch") for hp in STEP_HP for n in SIZES]
ADAMW_PARAMS += [("keras", "default", GRID_STRIDE_N), ("keras", "off", GRID_STRIDE_N)]


@pytest.mark.parametrize("mode,hpname,n", ADAMW_PARAMS, ids=[f"{m}-{h}-{n}" for m, h, n in ADAMW_PARAMS])
def test_adamw_per_element(cuda, mode, hpname, n):
    """dppo_adamw at every step number of STEP_NUMBERS from the same inputs (step_inputs: exact zeros in
    g, m = v = 0 elements, |g| near 1e3), each element of p', m', v' within adamw_oracle's bounds; the
    gradients are not written. At lr = 0 the parameters are bit-unchanged and the moments still step."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    raw = STEP_HP[hpname]
    hp = step_hp(*raw)
    p, m, v, g = step_inputs(n, seed=n % 1000)
    ratios, bound = {}, None
    for step in STEP_NUMBERS:
        P, M, V, G = (torch.tensor(x, device=cuda) for x in (p, m, v, g))
        ops.adamw(P, G, M, V, step, *raw, mode)
        torch.cuda.synchronize()
        got = [x.cpu().numpy() for x in (P, M, V)]
        ref, bounds = adamw_oracle(mode, p, m, v, g, step, hp)
        ratios[step] = step_ratios(got, ref, bounds)
        bound = [float(b.max()) for b in bounds]
        assert np.array_equal(G.cpu().numpy().view(np.uint32), g.view(np.uint32))
        if hp["lr"] == 0.0:
            assert np.array_equal(got[0].view(np.uint32), p.view(np.uint32)), "lr = 0 moved a parameter"
            assert not np.array_equal(got[1], m) and not np.array_equal(got[2], v), "lr = 0 froze the moments"
    print(json.dumps({"case": f"adamw-{mode}-{hpname}-{n}", "ratio_p_m_v": ratios, "max_bound_p_m_v": bound}))
    bad = {s: r for s, r in ratios.items() if not max(r) <= 1.0}
    assert not bad, bad


def test_adamw_noop_and_refusals(cuda):
    """n = 0 is a no-op; step < 1 and an unknown mode are refused with the library's message; the
    sentinel-filled buffers stay untouched by all three."""
    import torch
    from diffusionpolicyoptimization_amd import _lib
    from diffusionpolicyoptimization_amd._lib import DppoError, ptr, stream_handle
    bufs = [torch.full((300,), SENTINEL, device=cuda) for _ in range(4)]
    P, G, M, V = bufs
    call = lambda n, step, mode: _lib.call("dppo_adamw", ptr(P), ptr(G), ptr(M), ptr(V), n, step, 1e-3, 0.004, 0.9, 0.999,
                                           1e-7, mode, stream_handle(cuda))
    call(0, 1, _lib.DPPO_ADAMW_KERAS)
    with pytest.raises(DppoError, match="dppo_adamw: n < 0 or step < 1"):
        call(300, 0, _lib.DPPO_ADAMW_KERAS)
    with pytest.raises(DppoError, match="dppo_adamw: n < 0 or step < 1"):
        call(300, -3, _lib.DPPO_ADAMW_TORCH)
    with pytest.raises(DppoError, match="dppo_adamw: bad mode"):
        call(300, 1, 7)
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == SENTINEL).all())


# ------------------------------------------------------------------------------------------------
# 2. every step form at the geometries the update accepts
# ------------------------------------------------------------------------------------------------
# names as tests/test_update_surface_gpu.py's GEOMETRIES (hopper and walker are its helpers' base dims)
GEOMETRIES = {"hopper": HOPPER, "walker": WALKER, "h8a4": SURFACE["h8a4"][0], "td32": SURFACE["td32"][0],
              "ah256": SURFACE["ah256"][0], "cond2-walker": SURFACE["cond2-walker"][0], "tiny": SURFACE["tiny"][0]}
PRECISIONS = ("fp32", "bf16", "fp16")
RUNS, REFUSED = "runs", "refused"
# the table of the module docstring: (geometry, precision) -> outcome of every form
STEP_TABLE = {(g, pr): RUNS for g in GEOMETRIES for pr in PRECISIONS}
# name -> the range ("actor", "critic", "both": [actor | critic] with both images) and the flags
FORMS = {
    "staged-actor": dict(net="actor"),
    "staged-both": dict(net="both"),
    "clear": dict(net="actor", clear_grads=True, defer_sampler_tables=True),
    "fused-actor": dict(net="actor", fused_pack=True, clear_grads=True),
    "fused-critic": dict(net="critic", fused_pack=True, clear_grads=True),
    "l2v-staged": dict(net="actor", l2_from_pl2=True),
    "l2v-fused": dict(net="actor", l2_from_pl2=True, fused_pack=True, clear_grads=True),
    "clip-staged": dict(net="both", clip=True),
    "clip-fused-actor": dict(net="actor", clip=True, fused_pack=True, clear_grads=True),
    "clip-fused-critic": dict(net="critic", clip=True, fused_pack=True, clear_grads=True),
}
# (step, lr) of the three consecutive steps; the l2-virtual forms use learning rates large enough that
# reading the stepped W_out would show (test_l2_virtual_reads_the_old_w_out, CPU)
STEPS3 = ((1, 1e-4), (2, 3e-4), (1000, 1e-3))
STEPS3_L2V = ((2, 1e-1), (3, 5e-2), (1000, 1e-1))
STEP_REST = STEP_HP["default"][1:]     # weight_decay, beta1, beta2, eps
# hand-written clip scales, one per variable in layout order (12 actor, then 8 critic)
CLIP_SCALES = np.array([1.0, 0.37, 1.0, 0.052, 0.9, 1.0, 0.25, 1.0, 0.6, 0.013, 1.0, 0.5,
                        0.75, 1.0, 0.11, 1.0, 1.0, 0.3, 0.8, 1.0], np.float32)
STEP_PARAMS = [(g, pr, f, "keras") for g in GEOMETRIES for pr in PRECISIONS for f in FORMS]
STEP_PARAMS += [(g, pr, f, "torch") for g in ("hopper", "walker") for pr in PRECISIONS for f in FORMS]


class _StepProblem:
    """The CPU half of a step case: the model of a geometry, its flat [actor | critic] state and the
    oracle's view of the gradient each form steps with. No GPU needed."""

    def __init__(self, geometry, precision):
        from diffusionpolicyoptimization_amd import ops
        self.geometry, self.precision = geometry, precision
        self.dims = GEOMETRIES[geometry]
        self.d = d = ops.ModelDims(**self.dims)
        _, ft, critic = make_models(0, self.dims)
        self.aspec, self.cspec = ops.actor_param_spec(d), ops.critic_param_spec(d)
        self.na, self.nc = ops.spec_count(self.aspec), ops.spec_count(self.cspec)
        self.P0 = np.concatenate([ops.flatten_params(self.aspec, ft), ops.flatten_params(self.cspec, critic)])
        _, self.M0, self.V0, self.G0 = step_inputs(self.na + self.nc, seed=sum(map(ord, geometry)))
        # (tensor, offset in [actor | critic], count), in layout order: the variables of the clip scales
        self.tensors = [("actor." + n, o, k) for n, _, o, k in ops.spec_ranges(self.aspec)]
        self.tensors += [("critic." + n, self.na + o, k) for n, _, o, k in ops.spec_ranges(self.cspec)]
        self.off = {n: (o, k) for n, o, k in self.tensors}
        # the factored l2 gradient: pl2 [H][XD] at the start of the l2_w range, nothing else in [l2_w | l2_b]
        self.G0_l2v = self.G0.copy()
        l2w, nl2 = self.off["actor.l2_w"]
        self.G0_l2v[l2w + d.actor_hidden * d.xd:l2w + nl2 + d.actor_hidden] = 0.0

    def range(self, net):
        return {"actor": slice(0, self.na), "critic": slice(self.na, self.na + self.nc),
                "both": slice(0, self.na + self.nc)}[net]

    def l2_virtual(self, P, G):
        """The gradient a DPPO_STEP_L2_FROM_PL2 step uses, in float64, from the actor's pre-step
        parameters P and stored gradient G: dW_l2 = pl2 rnd(W_out)^T, db_l2 = db_out rnd(W_out)^T with
        W_out rounded to the image's precision -> (gradient, its error XD u sum|terms|)."""
        d = self.d
        H, XD = d.actor_hidden, d.xd
        rnd = {"bf16": O.round_bf16, "fp16": O.round_fp16}.get(self.precision, lambda x: np.asarray(x, np.float64))
        ow, l2w, l2b, ob = (self.off["actor." + k][0] for k in ("out_w", "l2_w", "l2_b", "out_b"))
        W = rnd(P[ow:ow + H * XD]).reshape(H, XD)                     # [j][q]
        pl2 = np.asarray(G[l2w:l2w + H * XD], np.float64).reshape(H, XD)   # [h][q]
        dbo = np.asarray(G[ob:ob + XD], np.float64)
        ge = np.asarray(G, np.float64).copy()
        err = np.zeros_like(ge)
        ge[l2w:l2w + H * H] = (pl2 @ W.T).reshape(-1)                 # [h][j]
        err[l2w:l2w + H * H] = XD * U32 * (np.abs(pl2) @ np.abs(W).T).reshape(-1)
        ge[l2b:l2b + H] = W @ dbo
        err[l2b:l2b + H] = XD * U32 * (np.abs(W) @ np.abs(dbo))
        return ge, err

    def clipped(self, G, sl):
        """The gradient a clipped step uses over the range sl: g * scale[variable] in float64 (the kernel
        rounds the product to fp32 once: error u |g scale|)."""
        s = np.concatenate([np.full(k, CLIP_SCALES[i], np.float64) for i, (_, _, k) in enumerate(self.tensors)])[sl]
        ge = np.asarray(G, np.float64) * s
        return ge, U32 * np.abs(ge)

    def effective_grad(self, form, P, G):
        """(gradient, error) the oracle steps with for a form, from the range's pre-step P and G."""
        f = FORMS[form]
        if f.get("l2_from_pl2"):
            return self.l2_virtual(P, G)
        if f.get("clip"):
            return self.clipped(G, self.range(f["net"]))
        return np.asarray(G, np.float64), 0.0

    def per_tensor(self, sl, got, ref, bounds):
        """{tensor: [ratio p, ratio m, ratio v]} over the tensors of the range sl."""
        out = {}
        for name, o, k in self.tensors:
            if o < sl.start or o + k > sl.stop:
                continue
            t = slice(o - sl.start, o - sl.start + k)
            out[name] = step_ratios([a[t] for a in got], [r[t] for r in ref], [b[t] for b in bounds])
        return out


_PROBLEMS = {}


def step_problem(geometry, precision):
    key = (geometry, precision)
    if key not in _PROBLEMS:
        _PROBLEMS.clear()       # one at a time: the parametrisation visits a key's forms in a row
        _PROBLEMS[key] = _StepProblem(geometry, precision)
    return _PROBLEMS[key]


class _Clear:
    """Three byte ranges of a sentinel-filled scratch buffer, as dppo_ppo_clear_ranges would give them
    (BoundOptimizerStep reads .args): [0, 8), [2400, 4800) and [4816, 5816)."""
    RANGES = ((0, 8), (2400, 2400), (4816, 1000))

    def __init__(self, cuda):
        import torch
        self.scratch = torch.empty(900, dtype=torch.float64, device=cuda)
        base = self.scratch.data_ptr()
        self._ptrs = (ctypes.c_void_p * 4)(*[base + o for o, _ in self.RANGES])
        self._bytes = (ctypes.c_size_t * 4)(*[b for _, b in self.RANGES])
        self.args = (self._ptrs, self._bytes, len(self.RANGES))
        self.inside = np.zeros(7200, bool)
        for o, b in self.RANGES:
            self.inside[o:o + b] = True

    def fill(self):
        self.scratch.fill_(7.0)

    def check(self, label):
        """Exactly the ranges are zero: every other byte group still holds the fill."""
        import torch
        words = self.scratch.view(torch.uint8).cpu().numpy()
        fill = np.full(900, 7.0).view(np.uint8)
        assert not words[self.inside].any(), (label, "a clear range was not zeroed")
        assert np.array_equal(words[~self.inside], fill[~self.inside]), (label, "bytes outside the clear ranges changed")


def _snapshot(tensors):
    return [t.clone() for t in tensors]


@pytest.mark.parametrize("geometry,precision,form,mode", STEP_PARAMS, ids=["-".join(x) for x in STEP_PARAMS])
def test_step_form(cuda, geometry, precision, form, mode):
    """One form of the optimizer step (FORMS) at one geometry and precision: three steps in a row on one
    stream with (step, lr) changing, each compared per tensor with the oracle restarted from the GPU's own
    pre-step state; gradients and clear ranges zeroed exactly where the flags say; the image byte-identical
    to a fresh pack of the stepped parameters — or the whole case refused before anything is written,
    as STEP_TABLE says."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd._lib import DppoError
    pb = step_problem(geometry, precision)
    d, f = pb.d, FORMS[form]
    net, l2v = f["net"], bool(f.get("l2_from_pl2"))
    sl = pb.range(net)
    label = f"step-{geometry}-{precision}-{form}-{mode}"
    T = lambda x: torch.tensor(np.ascontiguousarray(x), device=cuda)
    G0 = T((pb.G0_l2v if l2v else pb.G0)[sl])
    P, M, V, G = T(pb.P0[sl]), T(pb.M0[sl]), T(pb.V0[sl]), G0.clone()
    pa = P[:pb.na] if net in ("actor", "both") else None
    pc = P[-pb.nc:] if net in ("critic", "both") else None
    # the images before the step are the packs of the pre-step parameters (the virtual l2 reads W_OUT)
    img_a = ops.pack_actor(d, pa, precision) if pa is not None else None
    img_c = ops.pack_critic(d, pc, precision) if pc is not None else None
    scales = T(CLIP_SCALES[{"actor": slice(0, 12), "critic": slice(12, 20), "both": slice(0, 20)}[net]]) if f.get("clip") else None
    flags = {k: bool(f.get(k)) for k in ("defer_sampler_tables", "l2_from_pl2", "fused_pack", "clear_grads")}
    step = ops.BoundOptimizerStep(d, precision, P, G, M, V, *STEP_REST, mode, pa, img_a, pc, img_c, clip_scales=scales,
                                  **flags)
    clear = _Clear(cuda)
    state = [t for t in (P, M, V, G, img_a, img_c, clear.scratch) if t is not None]
    ratios, bound, outcome = {}, [0.0, 0.0, 0.0], RUNS
    for it, (stepno, lr) in enumerate(STEPS3_L2V if l2v else STEPS3):
        G.copy_(G0)
        clear.fill()
        torch.cuda.synchronize()
        before = _snapshot(state)
        pre = [x.cpu().numpy() for x in (P, M, V, G)]
        try:
            step(stepno, lr, clear=clear)
        except DppoError as e:
            torch.cuda.synchronize()
            assert it == 0, (label, "refused after a step ran", str(e))
            for a, b in zip(state, before):
                assert torch.equal(a, b), (label, "a refused step wrote", str(e))
            outcome = REFUSED
            break
        torch.cuda.synchronize()
        got = [x.cpu().numpy() for x in (P, M, V)]
        ge, gerr = pb.effective_grad(form, pre[0], pre[3])
        ref, bounds = adamw_oracle(mode, *pre[:3], ge, stepno, step_hp(lr, *STEP_REST), g_err=gerr)
        for name, r in pb.per_tensor(sl, got, ref, bounds).items():
            ratios[name] = [max(a, b) for a, b in zip(ratios.get(name, [0.0] * 3), r)]
        bound = [max(a, float(b.max())) for a, b in zip(bound, bounds)]
        bad = {k: r for k, r in ratios.items() if not max(r) <= 1.0}
        assert not bad, (label, f"step {stepno}", bad)
        g_after = G.cpu().numpy()
        if flags["clear_grads"]:
            assert not g_after.any(), (label, "gradients not zeroed")
        else:
            assert np.array_equal(g_after.view(np.uint32), pre[3].view(np.uint32)), (label, "gradients written")
        clear.check(label)
    print(json.dumps({"case": label, "outcome": outcome, "worst": max([max(r) for r in ratios.values()], default=0.0),
                      "ratio_p_m_v": ratios, "max_bound_p_m_v": bound}))
    assert outcome == STEP_TABLE[(geometry, precision)], (label, outcome)
    if outcome == REFUSED:
        return
    if img_a is not None:
        ops.refresh_sampler_tables(img_a)
        fresh = img_a.clone()           # a clone: the same bytes in the gaps between segments
        ops.pack_actor(d, pa, precision, out=fresh)
        torch.cuda.synchronize()
        assert torch.equal(img_a, fresh), (label, "actor image differs from a fresh pack")
    if img_c is not None:
        fresh = img_c.clone()
        ops.pack_critic(d, pc, precision, out=fresh)
        torch.cuda.synchronize()
        assert torch.equal(img_c, fresh), (label, "critic image differs from a fresh pack")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fused", [False, True], ids=["staged", "fused"])
def test_clip_with_l2_virtual_refused(cuda, precision, fused):
    """The clipped step and the virtual l2 gradient together are refused with the library's message (the
    factored gradient has no norm before it is formed), before anything is written."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd._lib import DppoError
    pb = step_problem("hopper", precision)
    sl = pb.range("actor")
    T = lambda x: torch.tensor(np.ascontiguousarray(x), device=cuda)
    P, M, V, G = T(pb.P0[sl]), T(pb.M0[sl]), T(pb.V0[sl]), T(pb.G0_l2v[sl])
    img = ops.pack_actor(pb.d, P, precision)
    step = ops.BoundOptimizerStep(pb.d, precision, P, G, M, V, *STEP_REST, "keras", P, img, l2_from_pl2=True,
                                  fused_pack=fused, clear_grads=fused, clip_scales=T(CLIP_SCALES[:12]))
    torch.cuda.synchronize()
    before = _snapshot([P, M, V, G, img])
    with pytest.raises(DppoError, match="dppo_optimizer_step_clip: no clip with DPPO_STEP_L2_FROM_PL2"):
        step(2, 1e-3)
    torch.cuda.synchronize()
    for a, b in zip([P, M, V, G, img], before):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------
# 3. the metrics copy at its edges
# ------------------------------------------------------------------------------------------------
METRIC_FORMS = ("staged-actor", "fused-actor", "fused-critic")


def _metrics_step(cuda, form):
    import torch
    from diffusionpolicyoptimization_amd import ops
    pb = step_problem("hopper", "fp32")
    f = FORMS[form]
    sl = pb.range(f["net"])
    T = lambda x: torch.tensor(np.ascontiguousarray(x), device=cuda)
    P, M, V, G = T(pb.P0[sl]), T(pb.M0[sl]), T(pb.V0[sl]), T(pb.G0[sl])
    actor = f["net"] == "actor"
    img = ops.pack_actor(pb.d, P, "fp32") if actor else ops.pack_critic(pb.d, P, "fp32")
    packs = (P, img, None, None) if actor else (None, None, P, img)
    flags = {k: bool(f.get(k)) for k in ("fused_pack", "clear_grads")}
    step = ops.BoundOptimizerStep(pb.d, "fp32", P, G, M, V, *STEP_REST, "keras", *packs, **flags)
    return step, [P, M, V, G, img]


@pytest.mark.parametrize("n_metrics", [0, 1, 256])
@pytest.mark.parametrize("form", METRIC_FORMS)
def test_metrics_copy_edges(cuda, form, n_metrics):
    """n_metrics doubles reach host-mapped metrics_out and the tag lands after them, at metrics_out[n]
    (0: the tag alone; 256: the limit, every thread of workgroup 0 copies one); nothing past the tag is
    written. The same copy without a tag into device memory leaves metrics_out[n:] alone."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    step, state = _metrics_step(cuda, form)
    met = torch.arange(256, dtype=torch.float64, device=cuda) * 0.5 + 0.25
    want = met.cpu().numpy()
    out = ops.MappedDoubles(260)
    step(1, 1e-4, metrics=met, metrics_out=out.address, n_metrics=n_metrics, metrics_tag=9)
    out.wait_tag(n_metrics, 9, timeout_s=10.0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.array[:n_metrics], want[:n_metrics])
    assert not out.array[n_metrics + 1:].any()
    dev = torch.full((260,), SENTINEL, dtype=torch.float64, device=cuda)
    step(2, 1e-4, metrics=met, metrics_out=dev, n_metrics=n_metrics)
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    np.testing.assert_array_equal(got[:n_metrics], want[:n_metrics])
    assert (got[n_metrics:] == SENTINEL).all()
    if form == "fused-actor":
        ops.refresh_sampler_tables(state[4])
        torch.cuda.synchronize()


@pytest.mark.parametrize("form", METRIC_FORMS)
def test_metrics_copy_refusals(cuda, form):
    """257 metrics, a tag without metrics_out and a tag >= 2^53 are refused with the library's messages,
    before anything is written."""
    import torch
    from diffusionpolicyoptimization_amd._lib import DppoError
    step, state = _metrics_step(cuda, form)
    met = torch.zeros(300, dtype=torch.float64, device=cuda)
    dev = torch.full((300,), SENTINEL, dtype=torch.float64, device=cuda)
    torch.cuda.synchronize()
    before = _snapshot(state + [dev])
    with pytest.raises(DppoError, match="dppo_optimizer_step: bad metrics copy"):
        step(1, 1e-4, metrics=met, metrics_out=dev, n_metrics=257)
    with pytest.raises(DppoError, match="dppo_optimizer_step: a tag needs metrics_out and < 2\\^53"):
        step(1, 1e-4, metrics_tag=5)
    with pytest.raises(DppoError, match="dppo_optimizer_step: a tag needs metrics_out and < 2\\^53"):
        step(1, 1e-4, metrics=met, metrics_out=dev, n_metrics=4, metrics_tag=2 ** 53)
    torch.cuda.synchronize()
    for a, b in zip(state + [dev], before):
        assert torch.equal(a, b)
