"""The packed images, and everything an optimizer step writes, byte for byte against recorded digests.

tests/golden/image_bytes_parent.json holds SHA-256 digests of what the library wrote at the commit the fixture
names (its "commit" field), recorded there twice; an output whose two runs disagreed is in its "unstable" list
and is not compared. The host code that describes a network and lists an image's tensors (csrc/dppo_layout.h
NetSpec, csrc/image_registry, csrc/pack.hip) may be rearranged freely; the bytes may not move.

Every image buffer starts zero-filled: the pack does not write the padding between segments. Dims are hopper's
and hopper's DDIM variant (time stride 2: the TEMB rows), at fp32 / bf16 / fp16.
  pack    each of the 4 actor (activation, head) pairs and the 4 critic (head, layernorm) pairs through the entry
          that takes exactly its attributes, and dppo_pack_all: the image. Then, attributes still steering the
          kernels: dppo_critic_forward at n = 33 (one full 32-row tile and one row), dppo_logprob's lp_mean at
          n = 4 and dppo_sample's actions at 16 envs with a fixed seed.
  staged  dppo_optimizer_step_ex over [actor | critic] with a residual and with a layer-normed plain critic (its
          12 jobs do not fit beside the actor's 13: the critic-alone launch), without clear ranges and with
          DPPO_STEP_CLEAR_GRADS + 4 ranges (5 zero jobs: the zero-first launch), with and without
          DPPO_STEP_DEFER_SAMPLER_TABLES: parameters, moments, both images, gradients, the ranges, and the actor
          image again after dppo_refresh_sampler_tables.
  fused   DPPO_STEP_FUSED_PACK over the actor range (4 pairs, and DPPO_STEP_L2_FROM_PL2 on the residual ones) and
          over the critic range (4 pairs): parameters, moments, the image, the actor image after the refresh.
`collect(cuda, dims_name, precision)` computes every digest of one (dims, precision); the fixture is its output."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from tests.helpers import HOPPER, HOPPER_DDIM, STEP_HP, make_models, step_inputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_bytes_parent.json")
DIMS = {"hopper": HOPPER, "hopper-ddim": HOPPER_DDIM}
PRECISIONS = ("fp32", "bf16", "fp16")
ACTORS = [(a, h) for a in ("ReLU", "Mish") for h in ("residual", "plain")]
CRITICS = [(h, ln) for h in ("residual", "plain") for ln in (False, True)]
STEP_REST = STEP_HP["default"][1:]
# the only outputs that may be run-to-run unstable (the row tiles and the sampler; pack.hip and optimizer.hip
# have no floating-point atomics)
KERNEL_OUTPUTS = ("values", "lp_mean", "actions")


def _sha(t):
    import torch
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


class _Case:
    """The models and buffers of one (dims, precision), built once."""

    def __init__(self, cuda, dims_name, precision):
        import torch
        from diffusionpolicyoptimization_amd import ops
        self.cuda, self.precision, self.base = cuda, precision, DIMS[dims_name]
        self.ops, self.torch = ops, torch
        self.raw = make_models(0, self.base)
        self.rng_seed = sum(map(ord, dims_name + precision))

    def dims(self, actor=("ReLU", "residual"), critic=("residual", False)):
        return self.ops.ModelDims(**self.base, activation=actor[0], head=actor[1], critic_head=critic[0],
                                  critic_layernorm=critic[1])

    def flat(self, spec, params, seed):
        """The flat fp32 parameters of a spec; tensors the model lacks (the norms' gamma / beta) are seeded."""
        rng = np.random.default_rng(seed)
        full = dict(params)
        for n, s in spec:
            if n not in full:
                full[n] = ((1.0 if n.endswith("_g") else 0.0) + 0.1 * rng.standard_normal(s)).astype(np.float32)
        return self.torch.tensor(self.ops.flatten_params(spec, full), device=self.cuda)

    def actor_params(self, d, which=1):
        return self.flat(self.ops.actor_param_spec(d), self.raw[which], 1)

    def critic_params(self, d):
        return self.flat(self.ops.critic_param_spec(d), self.raw[2], 2)

    def zeros(self, d, net):
        nbytes = (self.ops.actor_packed_bytes if net == "actor" else self.ops.critic_packed_bytes)(d, self.precision)
        return self.torch.zeros(nbytes, dtype=self.torch.uint8, device=self.cuda)

    def pack_actor(self, d, params, entry=None):
        """Through the entry that takes exactly d's attributes (or the one named)."""
        from diffusionpolicyoptimization_amd import _lib
        img = self.zeros(d, "actor")
        act, head = _lib.ACTIVATION[d.activation], _lib.HEAD[d.head]
        entry = entry or ("dppo_pack_actor_head" if head else "dppo_pack_actor_act" if act else "dppo_pack_actor")
        attrs = {"dppo_pack_actor": (), "dppo_pack_actor_act": (act,), "dppo_pack_actor_head": (act, head)}[entry]
        _lib.call(entry, ctypes.byref(d.c()), _lib.PRECISION[self.precision], *attrs, _lib.ptr(params), _lib.ptr(img),
                  _lib.stream_handle(self.cuda))
        self.ops._forget_on_free(img)
        return img

    def pack_critic(self, d, params):
        from diffusionpolicyoptimization_amd import _lib
        img = self.zeros(d, "critic")
        head, ln = _lib.HEAD[d.critic_head], _lib.LAYERNORM[d.critic_layernorm]
        entry = "dppo_pack_critic_ln" if ln else "dppo_pack_critic_head" if head else "dppo_pack_critic"
        attrs = {"dppo_pack_critic": (), "dppo_pack_critic_head": (head,), "dppo_pack_critic_ln": (head, ln)}[entry]
        _lib.call(entry, ctypes.byref(d.c()), _lib.PRECISION[self.precision], *attrs, _lib.ptr(params), _lib.ptr(img),
                  _lib.stream_handle(self.cuda))
        self.ops._forget_on_free(img)
        return img


def _pack_digests(c):
    torch, ops = c.torch, c.ops
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddim_buffers, ddpm_buffers
    out = {}
    d0 = c.dims()
    K, TS = d0.denoising_steps, d0.time_stride
    sched = ddpm_buffers(K) if TS == 1 else ddim_buffers(K * TS, K)
    tab = torch.tensor(ops.sched_table(sched), device=c.cuda)
    rng = np.random.default_rng(c.rng_seed)
    T = lambda x: torch.tensor(np.ascontiguousarray(x, np.float32), device=c.cuda)
    cond33, cond16 = T(rng.uniform(-1, 1, (33, d0.sd))), T(rng.uniform(-1, 1, (16, d0.sd)))
    cond4, chains4 = cond33[:4].contiguous(), T(rng.standard_normal((4, d0.ft_denoising_steps + 1, d0.xd)))
    for pair in ACTORS:
        d = c.dims(actor=pair)
        key = "pack/actor-%s-%s" % pair
        base, ft = c.pack_actor(d, c.actor_params(d, 0)), c.pack_actor(d, c.actor_params(d, 1))
        out[key + "/image"] = _sha(ft)
        out[key + "/lp_mean"] = _sha(ops.logprob(d, c.precision, ft, tab, cond4, chains4, want_elem=False)[1])
        out[key + "/actions"] = _sha(ops.sample(d, c.precision, base, ft, tab, cond16, seed=1234, want_chains=False)[0])
    for pair in CRITICS:
        d = c.dims(critic=pair)
        key = "pack/critic-%s-%s" % (pair[0], "ln" if pair[1] else "noln")
        img = c.pack_critic(d, c.critic_params(d))
        out[key + "/image"] = _sha(img)
        out[key + "/values"] = _sha(ops.critic_forward(d, c.precision, img, cond33))
    pa, pc = c.actor_params(d0), c.critic_params(d0)
    ia, ic = c.zeros(d0, "actor"), c.zeros(d0, "critic")
    ops.pack_all(d0, c.precision, pa, ia, pc, ic)
    out["pack/all/actor-image"], out["pack/all/critic-image"] = _sha(ia), _sha(ic)
    return out


class _Clear4:
    """Four byte ranges of a scratch buffer filled with 7.0 (a step's `clear` argument)."""
    RANGES = ((0, 8), (2400, 2400), (4816, 1000), (6000, 1200))

    def __init__(self, c):
        self.scratch = c.torch.full((900,), 7.0, dtype=c.torch.float64, device=c.cuda)
        base = self.scratch.data_ptr()
        self._ptrs = (ctypes.c_void_p * 4)(*[base + o for o, _ in self.RANGES])
        self._bytes = (ctypes.c_size_t * 4)(*[b for _, b in self.RANGES])
        self.args = (self._ptrs, self._bytes, 4)


def _step_digests(c, key, d, net, flags, with_clear):
    """One step of the form `flags` over the range `net`, from images packed of the pre-step parameters."""
    torch, ops = c.torch, c.ops
    pa0, pc0 = c.actor_params(d), c.critic_params(d)
    na, nc = pa0.numel(), pc0.numel()
    P = {"actor": pa0, "critic": pc0, "both": torch.cat([pa0, pc0])}[net].clone()
    _, m, v, g = step_inputs(P.numel(), seed=7)
    if flags.get("l2_from_pl2"):   # the factored l2 gradient: pl2 [H][XD] at l2_w, nothing else in [l2_w | l2_b]
        off = {n: o for n, _, o, _ in ops.spec_ranges(ops.actor_param_spec(d))}
        H = d.actor_hidden
        g[off["l2_w"] + H * d.xd:off["l2_w"] + H * H + H] = 0.0
    M, V, G = (torch.tensor(x, device=c.cuda) for x in (m, v, g))
    pa = P[:na] if net in ("actor", "both") else None
    pc = P[-nc:] if net in ("critic", "both") else None
    ia = c.pack_actor(d, pa, entry="dppo_pack_actor_head") if pa is not None else None
    ic = c.pack_critic(d, pc) if pc is not None else None
    step = ops.BoundOptimizerStep(d, c.precision, P, G, M, V, *STEP_REST, "keras", pa, ia, pc, ic, **flags)
    clear = _Clear4(c) if with_clear else None
    step(3, 3e-4, clear=clear)
    out = {key + "/params": _sha(P), key + "/m": _sha(M), key + "/v": _sha(V), key + "/grads": _sha(G)}
    if clear is not None:
        out[key + "/clear-ranges"] = _sha(clear.scratch)
    if ic is not None:
        out[key + "/critic-image"] = _sha(ic)
    if ia is not None:
        out[key + "/actor-image"] = _sha(ia)
        ops.refresh_sampler_tables(ia)
        out[key + "/actor-image-refreshed"] = _sha(ia)
    return out


def _staged_digests(c):
    out = {}
    for critic in (("residual", False), ("plain", True)):
        for with_clear in (False, True):
            for defer in (False, True):
                key = "staged/critic-%s-%s/%s/%s" % (critic[0], "ln" if critic[1] else "noln",
                                                     "clear4" if with_clear else "noclear", "defer" if defer else "full")
                flags = dict(defer_sampler_tables=defer, clear_grads=with_clear)
                out.update(_step_digests(c, key, c.dims(critic=critic), "both", flags, with_clear))
    return out


def _fused_digests(c):
    out = {}
    for pair in ACTORS:
        forms = [("", {})] + ([("-l2v", dict(l2_from_pl2=True))] if pair[1] == "residual" else [])
        for tag, extra in forms:
            flags = dict(fused_pack=True, clear_grads=True, **extra)
            out.update(_step_digests(c, "fused/actor-%s-%s%s" % (pair + (tag,)), c.dims(actor=pair), "actor", flags, True))
    for pair in CRITICS:
        key = "fused/critic-%s-%s" % (pair[0], "ln" if pair[1] else "noln")
        out.update(_step_digests(c, key, c.dims(critic=pair), "critic", dict(fused_pack=True, clear_grads=True), True))
    return out


PARTS = {"pack": _pack_digests, "staged": _staged_digests, "fused": _fused_digests}


def collect(cuda, dims_name, precision, parts=tuple(PARTS)):
    """{"<dims>/<precision>/<part>/...": digest} of the named parts."""
    c = _Case(cuda, dims_name, precision)
    out = {}
    for part in parts:
        out.update({"%s/%s/%s" % (dims_name, precision, k): h for k, h in PARTS[part](c).items()})
    return out


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_is_sound():
    """Only kernel outputs may be listed unstable: no image, parameter, gradient or clear-range digest."""
    g = _golden()
    assert len(g["commit"]) >= 7 and g["digests"]
    bad = [k for k in g["unstable"] if k.rsplit("/", 1)[1] not in KERNEL_OUTPUTS]
    assert not bad, bad


@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("dims_name", list(DIMS))
def test_bytes_match_recorded(cuda, dims_name, precision, part):
    g = _golden()
    got = collect(cuda, dims_name, precision, (part,))
    prefix = "%s/%s/%s/" % (dims_name, precision, part)
    want = {k: h for k, h in g["digests"].items() if k.startswith(prefix)}
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    stable = [k for k in got if k not in g["unstable"]]
    assert len(stable) >= len(got) - sum(k.rsplit("/", 1)[1] in KERNEL_OUTPUTS for k in got)
    diff = sorted(k for k in stable if got[k] != want[k])
    assert not diff, ("bytes differ from commit " + g["commit"], diff)
