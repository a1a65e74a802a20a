"""Thin torch-tensor wrappers over the C ABI (include/dppo.h).

Tensors are device tensors owned by the caller; every op is enqueued on the current torch
stream of the tensor's device. Shapes/dtypes are checked here before any launch so that a bad
call can never reach a kernel with mismatched extents.
"""
import ctypes
import functools
import os
import math
import time
import weakref
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream_handle


@dataclass(frozen=True)
class ModelDims:
    obs_dim: int = 11
    action_dim: int = 3
    horizon_steps: int = 4
    cond_steps: int = 1
    time_dim: int = 16
    actor_hidden: int = 512
    critic_hidden: int = 256
    denoising_steps: int = 20       # sampling steps (DDIM: ddim_steps)
    ft_denoising_steps: int = 10
    time_stride: int = 1            # diffusion time of sampling row r is r * time_stride (DDIM: K / S)
    # the actor's activation_type, a key of _lib.ACTOR_ACTIVATION ("ReLU", "Mish", "ELU", "GELU", "Softplus").
    # Python-only: it is no field of dppo_dims; pack_actor
    # records it with the packed image (dppo_pack_actor_act) and every kernel launch follows the image
    activation: str = "ReLU"
    # the actor's head, "residual" (ResidualMLP) or "plain" (MLP([in, h, h, out]), residual_style=False).
    # Python-only like the activation: pack_actor records it with the image (dppo_pack_actor_head). The flat
    # layout is the same; a plain actor leaves its l2 range unused and zero (actor_param_spec)
    head: str = "residual"
    # the critic's head, "residual" (ResidualMLP) or "plain" (MLP([sd, h, h, h, 1]), CriticObs residual_style=False).
    # Python-only: pack_critic records it with the critic image (dppo_pack_critic_head). Layout, spec and image
    # bytes are the same for both
    critic_head: str = "residual"
    # the critic's layer normalisation (CriticObs use_layernorm), Python-only like critic_head: pack_critic records it
    # with the critic image (dppo_pack_critic_ln). Unlike the head it lengthens the critic's spec, flat layout and
    # image by the norms' gamma / beta tail (critic_param_spec); every other offset keeps its value
    critic_layernorm: bool = False

    def __post_init__(self):
        if self.activation not in _lib.ACTOR_ACTIVATION:
            raise ValueError(f"activation must be one of {sorted(_lib.ACTOR_ACTIVATION)}, got {self.activation!r}")
        if self.head not in _lib.HEAD:
            raise ValueError(f"head must be one of {sorted(_lib.HEAD)}, got {self.head!r}")
        if self.critic_head not in _lib.HEAD:
            raise ValueError(f"critic_head must be one of {sorted(_lib.HEAD)}, got {self.critic_head!r}")
        if not isinstance(self.critic_layernorm, bool):
            raise ValueError(f"critic_layernorm must be a bool, got {self.critic_layernorm!r}")

    @property
    def xd(self):
        return self.horizon_steps * self.action_dim

    @property
    def sd(self):
        return self.cond_steps * self.obs_dim

    @property
    def actor_in(self):
        return self.xd + self.time_dim + self.sd

    def c(self):
        return _lib.DppoDims(self.obs_dim, self.action_dim, self.horizon_steps, self.cond_steps, self.time_dim,
                             self.actor_hidden, self.critic_hidden, self.denoising_steps, self.ft_denoising_steps,
                             self.time_stride)


class ParamSpec(list):
    """[(name, shape)] of the tensors a network HAS, each with its element offset in a flat layout of
    `total` elements that may hold ranges no tensor uses (a plain-head actor: the residual layout without
    l2). flatten_params leaves such ranges zero; unflatten_params skips them; spec_count is `total`."""

    def __init__(self, items, offsets, total):
        super().__init__(items)
        self.offsets, self.total = dict(offsets), int(total)


def actor_param_spec(d: ModelDims):
    """Flat fp32 layout of include/dppo.h (Keras kernels [in,out]). A plain-head actor (d.head == "plain")
    lists the time MLP, in, l1 and out at the SAME offsets and total: its l2 range is unused and zero."""
    td, h, xd = d.time_dim, d.actor_hidden, d.xd
    full = [("time_w1", (td, 2 * td)), ("time_b1", (2 * td,)), ("time_w2", (2 * td, td)), ("time_b2", (td,)),
            ("in_w", (d.actor_in, h)), ("in_b", (h,)), ("l1_w", (h, h)), ("l1_b", (h,)),
            ("l2_w", (h, h)), ("l2_b", (h,)), ("out_w", (h, xd)), ("out_b", (xd,))]
    if d.head != "plain":
        return full
    offsets, o = {}, 0
    for n, s in full:
        offsets[n] = o
        o += int(np.prod(s))
    return ParamSpec([(n, s) for n, s in full if n not in ("l2_w", "l2_b")], offsets, o)


def critic_ln_sites(d: ModelDims):
    """The norms of the critic: one per hidden layer of the plain head, the residual block's two, none without
    layer norm."""
    return (3 if d.critic_head == "plain" else 2) if d.critic_layernorm else 0


def critic_param_spec(d: ModelDims):
    """The critic's eight tensors, then the tail of a layer-normed critic: ln1_g, ln1_b, ln2_g, ln2_b (and ln3_g,
    ln3_b for the plain head), each [critic_hidden] (include/dppo.h dppo_pack_critic_ln)."""
    h = d.critic_hidden
    spec = [("in_w", (d.sd, h)), ("in_b", (h,)), ("l1_w", (h, h)), ("l1_b", (h,)),
            ("l2_w", (h, h)), ("l2_b", (h,)), ("out_w", (h, 1)), ("out_b", (1,))]
    for k in range(1, critic_ln_sites(d) + 1):
        spec += [(f"ln{k}_g", (h,)), (f"ln{k}_b", (h,))]
    return spec


def spec_ranges(spec):
    """(name, shape, offset, count) of each tensor of a spec in its flat layout: consecutive for a list, a
    ParamSpec's own offsets (which skip its unused ranges)."""
    o = 0
    for n, s in spec:
        k = int(np.prod(s))
        if isinstance(spec, ParamSpec):
            o = spec.offsets[n]
        yield n, s, o, k
        o += k


def spec_count(spec):
    """Elements of the flat layout (a ParamSpec's total counts its unused ranges)."""
    if isinstance(spec, ParamSpec):
        return spec.total
    return int(sum(int(np.prod(s)) for _, s in spec))


# Per-dims constants of the hot host paths, computed once: the update loop calls the minibatch,
# optimiser and repack wrappers ~10x per PPO minibatch, and at the per-rank minibatch of an 8-GPU
# run (6,250 rows) their Python cost, not the GPU, set the pace.
@functools.lru_cache(maxsize=None)
def _dims_c(d):
    return d.c()


@functools.lru_cache(maxsize=None)
def _n_params(d):
    return spec_count(actor_param_spec(d)), spec_count(critic_param_spec(d))


@functools.lru_cache(maxsize=None)
def _packed_bytes(d, prec):
    return (int(_lib.query("dppo_actor_packed_bytes", ctypes.byref(_dims_c(d)), prec)),
            int(_lib.query("dppo_critic_packed_bytes_ln", ctypes.byref(_dims_c(d)), prec, _lib.HEAD[d.critic_head],
                           _lib.LAYERNORM[d.critic_layernorm])))


@functools.lru_cache(maxsize=None)
def _workspace_bytes(d, prec, rows):
    return int(_lib.query("dppo_ppo_workspace_bytes", ctypes.byref(_dims_c(d)), prec, int(rows)))


def flatten_params(spec, params):
    flat = np.zeros(spec_count(spec), np.float32)
    for n, _, o, k in spec_ranges(spec):
        flat[o:o + k] = np.asarray(params[n], np.float32).reshape(-1)
    return flat


def unflatten_params(spec, flat):
    flat = np.asarray(flat)
    return {n: flat[o:o + k].reshape(s) for n, s, o, k in spec_ranges(spec)}


def check_checkpoint_head(names, spec, path, prefix=""):
    """A checkpoint's actor tensors (the file's names under `prefix`) must be the spec's head: a residual file
    (it has `prefix`l2_w) does not load into a plain actor, nor a plain file into a residual one. Another
    network's l2_w in the same file (the critic's) does not count."""
    has, wants = prefix + "l2_w" in set(names), any(n == "l2_w" for n, _ in spec)
    if has != wants:
        kind = lambda l2: "residual (with l2)" if l2 else "plain (no l2)"
        raise ValueError(f"{path}: the checkpoint holds a {kind(has)} actor, the model is {kind(wants)}")


CRITIC_HEAD_KEY = "critic.head"   # .npz checkpoints: present ("plain") only for a plain critic


def check_checkpoint_critic_head(names, head, path, file_head=None):
    """A .npz checkpoint's critic must be the model's head. Both heads have the same tensors, so a plain critic's
    file carries CRITIC_HEAD_KEY = "plain" (file_head: its value when the caller has read it); a file without the
    key holds a residual critic. A file without a critic passes."""
    names = set(names)
    if not any(n.startswith("critic.") for n in names):
        return
    has = (str(file_head) if file_head is not None else "plain") if CRITIC_HEAD_KEY in names else "residual"
    if has != head:
        raise ValueError(f"{path}: the checkpoint holds a {has} critic, the model is {head}")


def check_checkpoint_critic_layernorm(names, spec, path, prefix="critic."):
    """A .npz checkpoint's critic must hold exactly the model's layer-norm tensors (ln{k}_g / ln{k}_b of the spec): a
    file with norms the configured critic lacks (or with another head's count of them) and a file without the norms
    the configured critic has are both refused. A file without a critic passes."""
    names = set(names)
    if not any(n.startswith(prefix) for n in names):
        return
    is_ln = lambda n: n.startswith("ln") and n[-2:] in ("_g", "_b")
    has = sorted(n[len(prefix):] for n in names if n.startswith(prefix) and is_ln(n[len(prefix):]))
    wants = sorted(n for n, _ in spec if is_ln(n))
    if has != wants:
        kind = lambda v: f"a layer-normed critic ({', '.join(v)})" if v else "a critic without layer norm"
        raise ValueError(f"{path}: the checkpoint holds {kind(has)}, the model is {kind(wants)}")


def _check(t, shape, dtype, name):
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a device tensor")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")


def _prec(precision):
    return _lib.PRECISION[precision] if isinstance(precision, str) else int(precision)


# ------------------------------------------------------------------------------------------------
# packing
# ------------------------------------------------------------------------------------------------
def actor_packed_bytes(d: ModelDims, precision):
    return _packed_bytes(d, _prec(precision))[0]


def critic_packed_bytes(d: ModelDims, precision):
    return _packed_bytes(d, _prec(precision))[1]


def _step_mode(mode, defer_sampler_tables=False, l2_from_pl2=False, fused_pack=False, clear_grads=False):
    """The mode word of dppo_optimizer_step*: the AdamW flavour OR'd with the DPPO_STEP_* flags."""
    return ((_lib.DPPO_ADAMW_KERAS if mode == "keras" else _lib.DPPO_ADAMW_TORCH) |
            (_lib.DPPO_STEP_DEFER_SAMPLER_TABLES if defer_sampler_tables else 0) |
            (_lib.DPPO_STEP_L2_FROM_PL2 if l2_from_pl2 else 0) |
            (_lib.DPPO_STEP_FUSED_PACK if fused_pack else 0) |
            (_lib.DPPO_STEP_CLEAR_GRADS if clear_grads else 0))


def _address(x):
    """A void* argument given as a raw address (a dppo_host_alloc block or a precomputed device
    address), a tensor or None (NULL, as is address 0)."""
    a = x if isinstance(x, int) or x is None else x.data_ptr()
    return ctypes.c_void_p(a) if a else None


def pack_all(d: ModelDims, precision, actor_params=None, packed_actor=None, critic_params=None, packed_critic=None):
    """Both images (either pair may be None) in one launch (dppo_pack_all)."""
    p = _prec(precision)
    na, nc = _n_params(d)
    ab, cb = _packed_bytes(d, p)
    _check(actor_params, (na,), torch.float32, "actor params")
    _check(packed_actor, (ab,), torch.uint8, "packed actor")
    _check(critic_params, (nc,), torch.float32, "critic params")
    _check(packed_critic, (cb,), torch.uint8, "packed critic")
    t = actor_params if actor_params is not None else critic_params
    if actor_params is not None and (d.activation != "ReLU" or d.head != "residual"):
        # dppo_pack_all records ReLU / RESIDUAL for the actor image (= dppo_pack_actor): a Mish or plain-head
        # actor packs on its own
        pack_actor(d, actor_params, precision, out=packed_actor)
        if critic_params is not None:
            pack_critic(d, critic_params, precision, out=packed_critic)
        return
    if critic_params is not None and (d.critic_head != "residual" or d.critic_layernorm):
        # dppo_pack_all records RESIDUAL / no layer norm for the critic image too (= dppo_pack_critic): a plain or
        # layer-normed critic packs on its own
        if actor_params is not None:
            pack_actor(d, actor_params, precision, out=packed_actor)
        pack_critic(d, critic_params, precision, out=packed_critic)
        return
    _lib.call("dppo_pack_all", ctypes.byref(_dims_c(d)), p, ptr(actor_params), ptr(packed_actor), ptr(critic_params),
              ptr(packed_critic), stream_handle(t.device))


def optimizer_step(d: ModelDims, precision, params, grads, m, v, step, lr, weight_decay, beta1, beta2, eps, mode,
                   actor_params=None, packed_actor=None, critic_params=None, packed_critic=None, metrics=None,
                   metrics_out=None, n_metrics=0, metrics_tag=0, defer_sampler_tables=False, clip_scales=None):
    """AdamW over params/grads/m/v (equal-length flat ranges), the metric sums copied to
    metrics_out (a device tensor or a dppo_host_alloc address), then the given images re-derived:
    two launches on the current stream (dppo_optimizer_step). A nonzero metrics_tag is stored as
    metrics_out[n_metrics] after the sums (the host polls it instead of an event).
    defer_sampler_tables: the actor image's split-sampler tables are left stale and re-derived by
    the next sampler launch on it (DPPO_STEP_DEFER_SAMPLER_TABLES; the PPO kernels never read them).
    clip_scales: the per-variable clip scales of the range (grad_clip_scales), applied as the step reads
    each gradient (dppo_optimizer_step_clip; the range must be the actor, the critic or both)."""
    n = params.numel()
    for t, nm in ((grads, "grads"), (m, "m"), (v, "v")):
        if t.numel() != n:
            raise ValueError(f"{nm}: expected {n} elements")
    p = _prec(precision)
    args = (ctypes.byref(_dims_c(d)), p, ptr(params), ptr(grads), ptr(m), ptr(v), int(n),
            int(step), float(lr), float(weight_decay), float(beta1), float(beta2), float(eps),
            _step_mode(mode, defer_sampler_tables), ptr(actor_params), ptr(packed_actor),
            ptr(critic_params), ptr(packed_critic), ptr(metrics), _address(metrics_out),
            int(n_metrics), ctypes.c_uint64(int(metrics_tag)))
    if clip_scales is None:
        _lib.call("dppo_optimizer_step", *args, stream_handle(params.device))
    else:
        _lib.call("dppo_optimizer_step_clip", *args, None, None, 0, stream_handle(params.device), ptr(clip_scales),
                  _clip_nets(d, n, clip_scales))


def _net_vars(d):
    """Variables per DPPO_NET_* value: 12 actor, 8 critic plus the layer-norm tail's vectors, and both."""
    nc = 8 + 2 * critic_ln_sites(d)
    return {_lib.DPPO_NET_ACTOR: 12, _lib.DPPO_NET_CRITIC: nc, _lib.DPPO_NET_ACTOR | _lib.DPPO_NET_CRITIC: 12 + nc}


_NET_NAMES = {"actor": _lib.DPPO_NET_ACTOR, "critic": _lib.DPPO_NET_CRITIC, "both": 3}


def _clip_nets(d, n, clip_scales):
    """The DPPO_NET_* value of a clipped step from its scale table's length (12 actor, 8 critic, 20
    both; a layer-normed critic has 4 or 6 more); the library checks the range against it."""
    _check(clip_scales, (clip_scales.numel(),), torch.float32, "clip_scales")
    nvs = _net_vars(d)
    if nvs[1] == nvs[2]:   # a 12-variable critic: the range's length tells it from the actor
        nvs = {nets: nv for nets, nv in nvs.items() if nets == 3 or n == _n_params(d)[nets - 1]}
    for nets, nv in nvs.items():
        if clip_scales.numel() == nv:
            return nets
    raise ValueError(f"clip_scales: expected {_net_vars(d)[1]} (actor), {_net_vars(d)[2]} (critic) or {_net_vars(d)[3]} (both) "
                     f"entries, got {clip_scales.numel()}")


def grad_clip_workspace_bytes(d: ModelDims, nets):
    return int(_lib.query("dppo_grad_clip_workspace_bytes_ln", ctypes.byref(_dims_c(d)), int(_NET_NAMES.get(nets, nets)),
                          _lib.HEAD[d.critic_head], _lib.LAYERNORM[d.critic_layernorm]))


class BoundGradClip:
    """grad_clip_scales over fixed buffers, validated and marshalled once: a call enqueues the one norm
    launch on `stream` (a raw handle; default: the current stream). nets: "actor", "critic", "both" or
    the DPPO_NET_* value; grads: the flat fp32 range of those networks. The norm, scale and workspace
    buffers are allocated here unless given (norms=False: no norm table)."""

    def __init__(self, d: ModelDims, nets, grads, clip_norm, norms=None, scales=None, workspace=None):
        nets = int(_NET_NAMES.get(nets, nets))
        if nets not in _net_vars(d):
            raise ValueError(f"nets: expected 1 (actor), 2 (critic) or 3 (both), got {nets}")
        na, nc = _n_params(d)
        n = (na if nets & 1 else 0) + (nc if nets & 2 else 0)
        nv = _net_vars(d)[nets]
        _check(grads, (n,), torch.float32, "grads")
        dev = grads.device
        if norms is None:
            norms = torch.zeros(nv, dtype=torch.float32, device=dev)
        elif norms is False:
            norms = None
        _check(norms, (nv,), torch.float32, "norms")
        if scales is None:
            scales = torch.ones(nv, dtype=torch.float32, device=dev)
        _check(scales, (nv,), torch.float32, "scales")
        need = grad_clip_workspace_bytes(d, nets)
        if workspace is None:
            workspace = torch.empty(need // 8, dtype=torch.float64, device=dev)
        if not workspace.is_cuda or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need:
            raise ValueError(f"workspace: needs {need} contiguous device bytes")
        if not float(clip_norm) > 0:
            raise ValueError("clip_norm must be > 0")
        self.nets, self.norms, self.scales, self.workspace = nets, norms, scales, workspace
        self._lib = _lib.load()
        self._args = (ctypes.byref(_dims_c(d)), nets, _lib.HEAD[d.critic_head], _lib.LAYERNORM[d.critic_layernorm],
                      ptr(grads), float(clip_norm), ptr(norms), ptr(scales), ptr(workspace))
        self._dev = dev
        self._keep = (grads,)

    def __call__(self, stream=None):
        _lib.check(self._lib.dppo_grad_clip_scales_ln(*self._args, stream_handle(self._dev) if stream is None else stream),
                   "dppo_grad_clip_scales")
        return self.scales


def grad_clip_scales(d: ModelDims, nets, grads, clip_norm, norms=None, scales=None, workspace=None, stream=None):
    """tf.clip_by_norm per variable as a scale table (dppo_grad_clip_scales, one launch): norm[v] =
    sqrt(sum g^2) in fp64, scale[v] = clip_norm / max(norm[v], clip_norm), one entry per variable of
    `nets` ("actor": 12, "critic": 8, "both": 20) in layout order. Returns (norms, scales); buffers not
    given are allocated. BoundGradClip is the per-minibatch form."""
    b = BoundGradClip(d, nets, grads, clip_norm, norms=norms, scales=scales, workspace=workspace)
    b(stream)
    return b.norms, b.scales


def refresh_sampler_tables(packed_actor):
    """Re-derive an actor image's split-sampler tables on the current stream if an optimizer step
    deferred them (no-op otherwise); sampler launches do this themselves (dppo_refresh_sampler_tables)."""
    _lib.call("dppo_refresh_sampler_tables", ptr(packed_actor), stream_handle(packed_actor.device))


def episode_sums(reward, firsts, act_steps, success_threshold, out):
    """a16 (train_ppo_diffusion_agent.py:144-167) on the device: reward fp64 [S,E] (raw), firsts u8
    [S+1,E] -> out fp64 [E,4] rows {episodes, sum of returns, sum of best rewards, successes} per env
    (dppo_episode_sums); sum the rows in env order."""
    S, E = reward.shape
    if reward.dtype != torch.float64 or firsts.dtype != torch.uint8 or tuple(firsts.shape) != (S + 1, E):
        raise ValueError("episode_sums: reward fp64 [S,E] and firsts u8 [S+1,E] expected")
    if out.dtype != torch.float64 or tuple(out.shape) != (E, 4) or not (reward.is_contiguous() and firsts.is_contiguous()
                                                                          and out.is_contiguous()):
        raise ValueError("episode_sums: out fp64 [E,4], all contiguous")
    _lib.call("dppo_episode_sums", ptr(reward), ptr(firsts), int(S), int(E), int(act_steps), float(success_threshold),
              ptr(out), stream_handle(reward.device))
    return out


def value_moments(values, returns, out_address):
    """{sum y, sum y^2, sum d, sum d^2, n} of y = returns, d = returns - values (fp64) into 5 doubles
    at out_address (host-mapped, dppo_host_alloc) or a device tensor (dppo_value_moments)."""
    n = values.numel()
    if returns.numel() != n:
        raise ValueError("values / returns: length mismatch")
    _lib.call("dppo_value_moments", ptr(values), ptr(returns), int(n), _address(out_address), stream_handle(values.device))


class _HostBlock:
    """Owner of one dppo_host_alloc block: freed (dppo_host_free) when the last view of it is gone.
    The ctypes array every NumPy / torch view is built on holds it, so no view outlives the memory."""

    def __init__(self, nbytes):
        p = ctypes.c_void_p()
        _lib.call("dppo_host_alloc", ctypes.c_size_t(nbytes), ctypes.byref(p))
        self.address, self.nbytes = p.value, nbytes

    def view(self):
        buf = (ctypes.c_uint8 * self.nbytes).from_address(self.address)
        buf.owner = self
        return np.ctypeslib.as_array(buf)

    def __del__(self):
        if getattr(self, "address", None) and _lib._lib is not None:
            _lib.query("dppo_host_free", ctypes.c_void_p(self.address))
            self.address = None


class MappedArray:
    """A NumPy array (and a torch CPU view of it) over coherent mapped pinned memory
    (dppo_host_alloc): the host writes it, copy_from_host moves it to the device in one kernel.
    The memory is freed when the MappedArray and every array / tensor view of it are gone; a
    pending device copy from it must be complete by then (the owner synchronises first)."""

    def __init__(self, shape, dtype):
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        block = _HostBlock(max(1, nbytes))
        self.address = block.address
        self.array = block.view()[:nbytes].view(dtype).reshape(shape)
        self.array[...] = 0
        self.tensor = torch.from_numpy(self.array)


class MappedRef:
    """address + size of a dppo_host_alloc buffer owned elsewhere (copy_from_host source)."""

    def __init__(self, address, nbytes):
        self.address, self.nbytes = address, nbytes


def copy_from_host(pairs, stream=None):
    """[(device tensor, MappedArray | MappedRef)] -> one dppo_copy_from_host launch on the current
    stream."""
    if not pairs:
        return
    if len(pairs) > 4:
        raise ValueError("copy_from_host: at most 4 ranges per launch")
    n = len(pairs)
    dst = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _ in pairs])
    src = (ctypes.c_void_p * n)(*[m.address for _, m in pairs])
    nb = (ctypes.c_size_t * n)()
    for i, (t, m) in enumerate(pairs):
        n_src = m.nbytes if isinstance(m, MappedRef) else m.array.nbytes
        if not t.is_cuda or not t.is_contiguous() or t.numel() * t.element_size() != n_src:
            raise ValueError("copy_from_host: destination must be a contiguous device tensor of the source's size")
        nb[i] = n_src
    _lib.call("dppo_copy_from_host", n, dst, src, nb, stream_handle(pairs[0][0].device) if stream is None else stream)


class MappedDoubles:
    """n doubles of coherent mapped pinned memory (dppo_host_alloc) the device stores into and the
    host reads as a numpy array (the PPO metric sums of dppo_optimizer_step)."""

    def __init__(self, n):
        block = _HostBlock(8 * n)           # zeroed by dppo_host_alloc; the array's base holds the block
        self.address = block.address
        self.array = block.view().view(np.float64)

    def wait_tag(self, index, tag, timeout_s=30.0):
        """Spin until array[index] == tag (a tag the device stores after the data it guards)."""
        a = self.array
        if a[index] == tag:
            return
        t_end = time.perf_counter() + timeout_s
        while a[index] != tag:
            if time.perf_counter() > t_end:
                raise _lib.DppoError(f"mapped tag {tag} not seen within {timeout_s} s (found {a[index]})")


def _forget_image(address):
    try:
        _lib.call("dppo_forget_image", ctypes.c_void_p(address))
    except Exception:   # interpreter shutdown: the library may be gone, and so is its table
        pass


def _forget_on_free(img):
    """The library keeps an image's attributes (activation, heads) in a host table keyed by the image's ADDRESS.
    When the image tensor dies its memory returns to the allocator, and another tensor at that address (a clone
    of an image, say) would inherit the attributes: the entry is erased with the tensor (dppo_forget_image). An
    image that is a view of a larger buffer lives as long as that buffer does: the entry then goes with the base."""
    if img._base is not None:
        fins = img._base.__dict__.setdefault("_dppo_forget_views", {})
        fin = fins.get(img.data_ptr())
        if fin is None or not fin.alive:
            fins[img.data_ptr()] = fin = weakref.finalize(img._base, _forget_image, img.data_ptr())
            fin.atexit = False
        return
    fin = getattr(img, "_dppo_forget", None)
    if fin is None or not fin.alive:
        img._dppo_forget = weakref.finalize(img, _forget_image, img.data_ptr())
        img._dppo_forget.atexit = False


def pack_actor(d: ModelDims, params_flat, precision, out=None):
    """The packed image of an actor; d.activation and d.head are recorded with it (dppo_pack_actor_head) and
    decide which kernels every later launch on the image runs."""
    p = _prec(precision)
    _check(params_flat, (_n_params(d)[0],), torch.float32, "actor params")
    if out is None:
        out = torch.empty(_packed_bytes(d, p)[0], dtype=torch.uint8, device=params_flat.device)
    else:
        _check(out, (_packed_bytes(d, p)[0],), torch.uint8, "packed actor")
    _lib.call("dppo_pack_actor_head", ctypes.byref(_dims_c(d)), p, _lib.ACTOR_ACTIVATION[d.activation], _lib.HEAD[d.head],
              ptr(params_flat), ptr(out), stream_handle(params_flat.device))
    _forget_on_free(out)
    return out


def pack_critic(d: ModelDims, params_flat, precision, out=None):
    """The packed image of a critic; d.critic_head and d.critic_layernorm are recorded with it (dppo_pack_critic_ln)
    and decide which row tile and weight-gradient problems every later launch on the image runs, and whether the
    parameters and the image end in the norms' gamma / beta tail."""
    p = _prec(precision)
    _check(params_flat, (_n_params(d)[1],), torch.float32, "critic params")
    if out is None:
        out = torch.empty(_packed_bytes(d, p)[1], dtype=torch.uint8, device=params_flat.device)
    else:
        _check(out, (_packed_bytes(d, p)[1],), torch.uint8, "packed critic")
    _lib.call("dppo_pack_critic_ln", ctypes.byref(_dims_c(d)), p, _lib.HEAD[d.critic_head],
              _lib.LAYERNORM[d.critic_layernorm], ptr(params_flat), ptr(out), stream_handle(params_flat.device))
    _forget_on_free(out)
    return out


# ------------------------------------------------------------------------------------------------
# sampler / logprob / critic
# ------------------------------------------------------------------------------------------------
def sample(d: ModelDims, precision, packed_base, packed_ft, sched, cond, x_T=None, noise=None, seed=0, call_id=0,
           env_offset=0, deterministic=False, min_sampling_std=0.1, randn_clip=3.0, final_clip=None,
           actions=None, chains=None, want_chains=True):
    E = cond.shape[0]
    dev = cond.device
    _check(cond, (E, d.sd), torch.float32, "cond")
    _check(sched, (d.denoising_steps, _lib.SCHED_COLS), torch.float32, "sched")
    _check(x_T, (E, d.xd), torch.float32, "x_T")
    _check(noise, (d.denoising_steps, E, d.xd), torch.float32, "noise")
    _check(packed_base, (actor_packed_bytes(d, precision),), torch.uint8, "packed_base")
    _check(packed_ft, (actor_packed_bytes(d, precision),), torch.uint8, "packed_ft")
    if actions is None:
        actions = torch.empty(E, d.xd, dtype=torch.float32, device=dev)
    if chains is None and want_chains:
        chains = torch.empty(E, d.ft_denoising_steps + 1, d.xd, dtype=torch.float32, device=dev)
    _check(actions, (E, d.xd), torch.float32, "actions")
    _check(chains, (E, d.ft_denoising_steps + 1, d.xd), torch.float32, "chains")
    _lib.call("dppo_sample", ctypes.byref(_dims_c(d)), _prec(precision), ptr(packed_base), ptr(packed_ft), ptr(sched),
              ptr(cond), E, ptr(x_T), ptr(noise), ctypes.c_uint64(seed & (2 ** 64 - 1)), ctypes.c_uint64(call_id),
              int(env_offset), int(bool(deterministic)), float(min_sampling_std), float(randn_clip),
              float(final_clip) if final_clip is not None else 0.0, ptr(actions), ptr(chains), stream_handle(dev))
    return actions, chains


def sampler_layout(d: ModelDims, precision, n_envs):
    """Workgroups per 16-env tile of the sampler dppo_sample runs for n_envs envs: 0 = the
    weight-streaming kernel, P > 0 = the split register-resident kernel (include/dppo.h)."""
    m = ctypes.c_int()
    _lib.call("dppo_sampler_layout", ctypes.byref(d.c()), _prec(precision), int(n_envs), ctypes.byref(m))
    return m.value


def sampler_max_in_flight(d: ModelDims, precision, n_envs):
    """Sampler launches of n_envs envs that may be in flight together (include/dppo.h), divided
    among the ranks that share this GPU (DPPO_SINGLE_DEVICE rehearsals: every rank's launches need
    their co-resident workgroups at once)."""
    m = ctypes.c_int()
    _lib.call("dppo_sampler_max_in_flight", ctypes.byref(d.c()), _prec(precision), int(n_envs), ctypes.byref(m))
    sharing = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))) \
        if os.environ.get("DPPO_SINGLE_DEVICE") else 1
    return max(1, m.value // max(1, sharing))


def sampler_plan(d: ModelDims, precision, n_envs):
    """The sampler the library runs for n_envs envs (dppo_sampler_plan): dict(kernel, members,
    sets, workgroups); kernel: 0 weight streaming, 2 folded split (one 16-env tile per member
    set; kernel ids 1 and 3, the r01 P = 8 and r03 pair kernels, were measured slower and removed)."""
    out = (ctypes.c_int * 4)()
    _lib.call("dppo_sampler_plan", ctypes.byref(d.c()), _prec(precision), int(n_envs), out)
    return dict(kernel=out[0], members=out[1], sets=out[2], workgroups=out[3])


def _stream_ring(d, precision, E, dev):
    """(torch streams, their handles) of a rollout's launches. Consecutive launches alternate over
    DPPO_ROLLOUT_STREAMS streams (default 2): launch t+1 is dispatched, and runs its
    observation-independent prologue (resident weights, noise), while launch t still runs, instead of
    after it retires. begin() / end() order them against the caller's stream around a rollout. Two
    launches in flight must both fit on the device (the split sampler's members wait for each other
    inside a launch): above that size, one stream."""
    nst = max(1, int(os.environ.get("DPPO_ROLLOUT_STREAMS", "2")))
    nst = min(nst, sampler_max_in_flight(d, precision, E))
    streams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(device=dev) for _ in range(nst - 1)]
    return streams, [ctypes.c_void_p(st.cuda_stream) for st in streams]


def _step_args(m, dims, deterministic):
    """A rollout step's model arguments in the C ABI's order: (dims, precision, images, schedule) and
    (seed, call id, env offset, mode, min std, clips)."""
    fc = m.final_action_clip_value
    return ((ctypes.byref(dims), _prec(m.precision), ptr(m.packed_base), ptr(m.packed_ft), ptr(m.sched_for(deterministic))),
            (ctypes.c_uint64(m.seed & (2 ** 64 - 1)), ctypes.c_uint64(m._call_id), m._env_offset,
             int(bool(deterministic)), float(m.get_min_sampling_denoising_std()), float(m.randn_clip_value),
             float(fc) if fc is not None else 0.0))


class SampleStepper:
    """dppo_sample_step with every argument but the step index, call counter and mode bound once
    (the rollout's buffers never move), so a rollout step costs one ctypes call."""

    def __init__(self, model, cond_host, obs_traj, actions, actions_host, chains_traj):
        d = model.dims
        S, E = obs_traj.shape[0], obs_traj.shape[1]
        _check(obs_traj, (S, E, d.sd), torch.float32, "obs_traj")
        _check(chains_traj, (S, E, d.ft_denoising_steps + 1, d.xd), torch.float32, "chains_traj")
        _check(actions, (E, d.xd), torch.float32, "actions")
        if cond_host.is_cuda or actions_host.is_cuda or not (cond_host.is_pinned() and actions_host.is_pinned()):
            raise ValueError("cond_host / actions_host must be pinned host tensors")
        if cond_host.numel() != E * d.sd or actions_host.numel() != E * d.xd:
            raise ValueError("cond_host / actions_host sizes do not match the rollout")
        self.model, self.S, self.E = model, S, E
        self._fn = _lib.load().dppo_sample_step
        self._dims = d.c()
        self._keep = (cond_host, obs_traj, actions, actions_host, chains_traj)
        self._obs0, self._obs_step = obs_traj.data_ptr(), E * d.sd * 4
        self._ch0, self._ch_step = chains_traj.data_ptr(), E * (d.ft_denoising_steps + 1) * d.xd * 4
        self._fixed = (ptr(cond_host), ptr(actions), ptr(actions_host))
        self._tstreams, self._handles = _stream_ring(d, model.precision, E, obs_traj.device)
        self._stream = self._handles[0]

    def __call__(self, i, deterministic=False):
        if not 0 <= i < self.S:
            raise IndexError(f"rollout step {i} outside [0, {self.S})")
        m = self.model
        cond_host, actions, actions_host = self._fixed
        common, scalars = _step_args(m, self._dims, deterministic)
        _lib.check(self._fn(*common, cond_host, ctypes.c_void_p(self._obs0 + i * self._obs_step), self.E, *scalars,
                            actions, actions_host, ctypes.c_void_p(self._ch0 + i * self._ch_step), 1, self._stream),
                   "dppo_sample_step")
        m._call_id += 1


class RolloutPipe:
    """Pipelined rollout steps (dppo_rollout_enqueue). The observation and action staging buffers
    and two step counters live in coherent mapped pinned memory (dppo_host_alloc); the launch of
    step t+1 is enqueued BEFORE the host steps the envs of step t and waits on the `go` counter, so
    the launch latency overlaps host work and the host learns that step t is done by polling the
    `done` counter instead of a stream synchronisation.
        pipe.enqueue(i, det)   step i's launch (waits until its observation is published)
        pipe.publish()         the observation buffer holds the next step's input
        pipe.wait()            block until the oldest unfinished step has written its actions
    obs / act are torch views over the staging memory ([E, SD] / [E, XD] float32)."""

    def __init__(self, model, obs_traj, actions, chains_traj):
        d = model.dims
        S, E = obs_traj.shape[0], obs_traj.shape[1]
        _check(obs_traj, (S, E, d.sd), torch.float32, "obs_traj")
        _check(chains_traj, (S, E, d.ft_denoising_steps + 1, d.xd), torch.float32, "chains_traj")
        _check(actions, (E, d.xd), torch.float32, "actions")
        lib = _lib.load()
        self._lib, self.model, self.S, self.E = lib, model, S, E
        # the five staging blocks (observation, actions, counters, tagged observation, tagged actions)
        self._blocks = [_HostBlock(n) for n in (4 * E * d.sd, 4 * E * d.xd, 256, 8 * E * d.sd, 8 * E * d.xd)]
        po, pa, pc, pt, pat = (b.address for b in self._blocks)
        # the observation protocol: "tagged" (default: the observation is published as tagged
        # granules the launch polls itself, dppo_rollout_enqueue_tagged) or "go" (a go counter, then
        # the launch reads the float buffer); DPPO_ROLLOUT_PROTOCOL=go selects the latter
        self.protocol = os.environ.get("DPPO_ROLLOUT_PROTOCOL", "tagged")
        if self.protocol not in ("tagged", "go"):
            raise ValueError(f"DPPO_ROLLOUT_PROTOCOL must be 'tagged' or 'go', got {self.protocol!r}")
        self._obs_tag = np.ctypeslib.as_array((ctypes.c_uint64 * (E * d.sd)).from_address(pt))
        # tagged actions (tagged protocol): the host polls the actions themselves
        self._act_tag = np.ctypeslib.as_array((ctypes.c_uint64 * (E * d.xd)).from_address(pat))
        self.obs = torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * (E * d.sd)).from_address(po))).view(E, d.sd)
        self.obs_mapped = MappedRef(po, 4 * E * d.sd)   # for copy_from_host
        self.act = torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * (E * d.xd)).from_address(pa))).view(E, d.xd)
        ctr = np.ctypeslib.as_array((ctypes.c_uint32 * 64).from_address(pc))
        self._go, self._done = ctr[0:1], ctr[16:17]          # separate 64-B lines
        self._p = dict(obs=ctypes.c_void_p(po), act=ctypes.c_void_p(pa), go=ctypes.c_void_p(pc),
                       done=ctypes.c_void_p(pc + 64), obs_tag=ctypes.c_void_p(pt), act_tag=ctypes.c_void_p(pat))
        self._fn = lib.dppo_rollout_enqueue_tagged if self.protocol == "tagged" else lib.dppo_rollout_enqueue
        self._dims = d.c()
        self._keep = (obs_traj, actions, chains_traj)
        self._obs0, self._obs_step = obs_traj.data_ptr(), E * d.sd * 4
        self._ch0, self._ch_step = chains_traj.data_ptr(), E * (d.ft_denoising_steps + 1) * d.xd * 4
        self._actions = ptr(actions)
        self._tstreams, self._handles = _stream_ring(d, model.precision, E, obs_traj.device)
        self._stream = self._handles[0]
        self.nwg = (E + 15) // 16
        self.enqueued = 0      # steps launched so far (step s waits for go >= s + 1)
        self.published = 0
        self.finished = 0

    def enqueue(self, i, deterministic=False):
        if not 0 <= i < self.S:
            raise IndexError(f"rollout step {i} outside [0, {self.S})")
        m = self.model
        p = self._p
        self._stream = self._handles[self.enqueued % len(self._handles)]
        self.enqueued += 1
        common, scalars = _step_args(m, self._dims, deterministic)
        tail = (self.E, *scalars, self._actions, p["act"], ctypes.c_void_p(self._ch0 + i * self._ch_step))
        obs_dev = ctypes.c_void_p(self._obs0 + i * self._obs_step)
        if self.protocol == "tagged":   # step s waits for granules tagged s + 1 (= its publish count)
            tail_t = tail[:-2] + (p["act_tag"],) + tail[-1:]          # tagged actions replace actions_host
            rc = self._fn(*common, p["obs_tag"], obs_dev, *tail_t, ctypes.c_uint32(self.enqueued), p["done"],
                          self._stream)
        else:
            rc = self._fn(*common, p["obs"], obs_dev, *tail, p["go"], ctypes.c_uint32(self.enqueued), p["done"],
                          self._stream)
        _lib.check(rc, "dppo_rollout_enqueue")
        m._call_id += 1

    def launch_event(self, ev=None):
        """An event recorded on the stream of the most recent launch (its completion); ev: an
        event to re-record (a caller's ring: creating and destroying one per step cost ~3 us of
        host time each, ~1.5 ms per 500-step rollout when the list was freed)."""
        if ev is None:
            ev = torch.cuda.Event()
        ev.record(self._tstreams[(self.enqueued - 1) % len(self._tstreams)])
        return ev

    def begin(self):
        """Before a rollout: split-sampler tables an optimizer step deferred are re-derived on the
        caller's stream, then the launch streams wait for it (updated weights and tables). A launch
        reads its resident tables in its prologue, before its observation wait, so the refresh must
        precede every stream, not only the first launch's."""
        with torch.cuda.stream(self._tstreams[0]):
            refresh_sampler_tables(self.model.packed_ft)
            refresh_sampler_tables(self.model.packed_base)
        for st in self._tstreams[1:]:
            st.wait_stream(self._tstreams[0])

    def end(self):
        """After a rollout: the caller's stream waits for every launch stream."""
        for st in self._tstreams[1:]:
            self._tstreams[0].wait_stream(st)

    def publish(self):
        self.published += 1
        if self.protocol == "tagged":         # one aligned 8-byte store per value: never torn
            bits = self.obs.numpy().reshape(-1).view(np.uint32).astype(np.uint64)
            self._obs_tag[:] = (np.uint64(self.published) << np.uint64(32)) | bits
        else:
            self._go[0] = self.published      # x86 stores are ordered: the observation is visible first

    def gate(self, publish, timeout_s=30.0):
        """Arguments of a gated env step (env.step(..., gate=...)): the native stepper waits for
        this step's done count itself and, if publish, releases the next launch. Call
        published() after a step that did publish, publish() after one that did not."""
        self.finished += 1
        if self.protocol == "tagged":   # the finished launch's actions carry its tag (= finished)
            pub = (self._p["obs_tag"], self.published + 1) if publish else (None, 0)
            return ("tagged", self._p["done"], self._p["act_tag"], ctypes.c_uint32(self.finished), pub[0],
                    ctypes.c_uint32(pub[1]), ctypes.c_double(timeout_s))
        pub = (self._p["go"], self.published + 1) if publish else (None, 0)
        return ("go", self._p["done"], ctypes.c_uint32(self.finished * self.nwg), pub[0],
                ctypes.c_uint32(pub[1]), ctypes.c_double(timeout_s))

    def published_by_gate(self):
        self.published += 1

    def wait(self, timeout_s=30.0):
        self.finished += 1
        target = self.finished * self.nwg
        done = self._done
        tagged = self.protocol == "tagged"
        t0 = None
        while True:
            v = int(done[0])
            if v & 0x80000000:
                raise _lib.DppoError("rollout step timed out waiting for its observation")
            if tagged:   # the launch stores its actions as {tag, bits} granules (no host float copy)
                x = self._act_tag.copy()
                if ((x >> np.uint64(32)) == np.uint64(self.finished)).all():
                    self.act.numpy().reshape(-1).view(np.uint32)[:] = (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)
                    return
            elif v >= target:
                return
            if t0 is None:
                t0 = time.perf_counter()
            elif time.perf_counter() - t0 > timeout_s:
                raise _lib.DppoError(f"rollout step {self.finished - 1} did not finish within {timeout_s} s")

    def close(self):
        for st in self._tstreams:
            st.synchronize()
        for h in self._handles:     # the split sampler's exchange buffers of these streams go back to the pool
            _lib.call("dppo_sampler_release_stream", h)
        self._blocks = []     # freed here unless a view still holds one (each block frees itself)

    def __del__(self):
        try:
            if self._blocks:
                self.close()
        except Exception:
            pass


def logprob(d: ModelDims, precision, packed_ft, sched, cond, chains, min_logprob_std=0.1, reward_horizon=None,
            want_elem=True, want_mean=True, lp_elem=None, lp_mean=None):
    n = cond.shape[0]
    dev = cond.device
    kf = d.ft_denoising_steps
    _check(cond, (n, d.sd), torch.float32, "cond")
    _check(chains, (n, kf + 1, d.xd), torch.float32, "chains")
    _check(sched, (d.denoising_steps, _lib.SCHED_COLS), torch.float32, "sched")
    _check(packed_ft, (actor_packed_bytes(d, precision),), torch.uint8, "packed_ft")
    if want_elem and lp_elem is None:
        lp_elem = torch.empty(n * kf, d.xd, dtype=torch.float32, device=dev)
    if want_mean and lp_mean is None:
        lp_mean = torch.empty(n, kf, dtype=torch.float32, device=dev)
    _check(lp_elem, (n * kf, d.xd), torch.float32, "lp_elem")
    _check(lp_mean, (n, kf), torch.float32, "lp_mean")
    rh = d.horizon_steps if reward_horizon is None else int(reward_horizon)
    _lib.call("dppo_logprob", ctypes.byref(_dims_c(d)), _prec(precision), ptr(packed_ft), ptr(sched), ptr(cond),
              ptr(chains), n, float(min_logprob_std), rh, ptr(lp_elem), ptr(lp_mean), stream_handle(dev))
    return lp_elem, lp_mean


def critic_forward(d: ModelDims, precision, packed_critic, cond, values=None):
    n = cond.shape[0]
    _check(cond, (n, d.sd), torch.float32, "cond")
    _check(packed_critic, (critic_packed_bytes(d, precision),), torch.uint8, "packed_critic")
    if values is None:
        values = torch.empty(n, dtype=torch.float32, device=cond.device)
    _check(values, (n,), torch.float32, "values")
    _lib.call("dppo_critic_forward", ctypes.byref(_dims_c(d)), _prec(precision), ptr(packed_critic), ptr(cond), n,
              ptr(values), stream_handle(cond.device))
    return values


# ------------------------------------------------------------------------------------------------
# scans
# ------------------------------------------------------------------------------------------------
def gae(reward, values, last_values, terminated, gamma=0.99, lam=0.95, reward_scale_const=1.0, adv=None, ret=None):
    S, E = reward.shape
    _check(reward, (S, E), torch.float64, "reward")
    _check(values, (S, E), torch.float32, "values")
    _check(last_values, (E,), torch.float32, "last_values")
    _check(terminated, (S, E), torch.uint8, "terminated")
    if adv is None:
        adv = torch.empty(S, E, dtype=torch.float32, device=reward.device)
    if ret is None:
        ret = torch.empty(S, E, dtype=torch.float32, device=reward.device)
    _lib.call("dppo_gae", ptr(reward), ptr(values), ptr(last_values), ptr(terminated), S, E, float(gamma), float(lam),
              float(reward_scale_const), ptr(adv), ptr(ret), stream_handle(reward.device))
    return adv, ret


def reward_scale_workspace(S, E, device):
    n = int(_lib.query("dppo_reward_scale_workspace_doubles", S, E))
    return torch.empty(n, dtype=torch.float64, device=device)


def reward_scale(reward, first, ret_state, rms_state, workspace=None, gamma=0.99, cliprew=10.0, epsilon=1e-8):
    """In place: reward [S,E] fp64 is replaced by the scaled reward (RunningRewardScaler.__call__)."""
    S, E = reward.shape
    _check(reward, (S, E), torch.float64, "reward")
    _check(first, (S, E), torch.uint8, "first")
    _check(ret_state, (E,), torch.float64, "ret_state")
    _check(rms_state, (3,), torch.float64, "rms_state")
    if workspace is None:
        workspace = reward_scale_workspace(S, E, reward.device)
    _lib.call("dppo_reward_scale", ptr(reward), ptr(first), ptr(ret_state), ptr(rms_state), ptr(workspace), S, E,
              float(gamma), float(cliprew), float(epsilon), stream_handle(reward.device))
    return reward


def reward_scale_moments(reward, first, ret_state, moments, workspace, gamma=0.99):
    S, E = reward.shape
    _lib.call("dppo_reward_scale_moments", ptr(reward), ptr(first), ptr(ret_state), ptr(workspace), ptr(moments), S, E,
              float(gamma), stream_handle(reward.device))
    return moments


def reward_scale_apply(reward, rms_state, cliprew=10.0, epsilon=1e-8):
    S, E = reward.shape
    _lib.call("dppo_reward_scale_apply", ptr(reward), ptr(rms_state), S, E, float(cliprew), float(epsilon),
              stream_handle(reward.device))
    return reward


def _bcast_len(S, L):
    if S == L or S == 1:
        return L
    if L == 1:
        return S
    raise ValueError(f"operands could not be broadcast together with shapes ({S},) ({L},)")


def reward_scale_per_env(reward, first, ret_state, rms_in, L_in, rms_out, workspace, out, gamma=0.99, cliprew=10.0,
                         epsilon=1e-8):
    """RunningRewardScaler(per_env=True).__call__ (reference util/reward_scaling.py:51-66), time-major:
    reward / first [S,E], rms_in / rms_out fp64 [1 + 2 L] = {count, mean[L], var[L]} (distinct buffers),
    out [C, E] (C = S, or the new state length when S == 1). Returns the new state length."""
    S, E = reward.shape
    _check(reward, (S, E), torch.float64, "reward")
    _check(first, (S, E), torch.uint8, "first")
    _check(ret_state, (E,), torch.float64, "ret_state")
    Lo = _bcast_len(S, L_in)
    C = S if (S > 1 or Lo == 1) else Lo
    _check(out, (C, E), torch.float64, "out")
    if rms_in.numel() < 1 + 2 * L_in or rms_out.numel() < 1 + 2 * Lo:
        raise ValueError("rms state buffers too small")
    _lib.call("dppo_reward_scale_per_env", ptr(reward), ptr(first), ptr(ret_state), ptr(rms_in), int(L_in), ptr(rms_out),
              ptr(workspace), S, E, float(gamma), float(cliprew), float(epsilon), ptr(out), stream_handle(reward.device))
    return Lo


def reward_scale_per_env_moments(reward, first, ret_state, workspace, col_moments, gamma=0.99):
    S, E = reward.shape
    _check(col_moments, (S, 2), torch.float64, "col_moments")
    _lib.call("dppo_reward_scale_per_env_moments", ptr(reward), ptr(first), ptr(ret_state), ptr(workspace),
              ptr(col_moments), S, E, float(gamma), stream_handle(reward.device))
    return col_moments


def reward_scale_per_env_apply(reward, rms_state, L, out, cliprew=10.0, epsilon=1e-8):
    S, E = reward.shape
    _lib.call("dppo_reward_scale_per_env_apply", ptr(reward), ptr(rms_state), S, E, int(L), float(cliprew),
              float(epsilon), ptr(out), stream_handle(reward.device))
    return out


# ------------------------------------------------------------------------------------------------
# update
# ------------------------------------------------------------------------------------------------
def feistel_permute(first, count, n, seed, epoch, device):
    out = torch.empty(count, dtype=torch.int64, device=device)
    _lib.call("dppo_feistel_permute", int(first), int(count), int(n), ctypes.c_uint64(seed), int(epoch), ptr(out),
              stream_handle(device))
    return out


def ppo_workspace(d: ModelDims, precision, rows, device):
    return torch.empty(_workspace_bytes(d, _prec(precision), int(rows)), dtype=torch.uint8, device=device)


_PLAN_MODES = {"train": 0, "pretrain": 1, "logprob": 2}


def ppo_plan(d: ModelDims, precision, rows, mode="train"):
    """The kernel paths a launch of `rows` rows takes on the current device (dppo_ppo_plan: the host
    functions the launchers themselves call): dict(actor_tile_rows (32 or 64), actor_waves,
    dw_chunks_actor, dw_chunk_rows_actor, dw_chunks_critic, dw_chunk_rows_critic). mode: "train"
    (ppo_minibatch), "pretrain" (pretrain_minibatch) or "logprob" (rows = samples x K'); the dW fields
    are 0 where the mode has no such launch. The plan is d.activation's (dppo_ppo_plan_act): a Mish actor
    runs the 32-row tile on 8 waves at every row count. The critic's row tile: ppo_plan_critic."""
    out = (ctypes.c_int * 6)()
    _lib.call("dppo_ppo_plan_act", ctypes.byref(d.c()), _prec(precision), _lib.ACTOR_ACTIVATION[d.activation], int(rows),
              _PLAN_MODES[mode], out)
    return dict(actor_tile_rows=out[0], actor_waves=out[1], dw_chunks_actor=out[2], dw_chunk_rows_actor=out[3],
                dw_chunks_critic=out[4], dw_chunk_rows_critic=out[5])


def ppo_plan_critic(d: ModelDims, precision):
    """The critic's row tile for d.critic_head / d.critic_layernorm (dppo_ppo_plan_critic): dict(critic_tile_rows,
    critic_waves, critic_tile_capped). capped = the 128-register kernel entry (two tiles per CU), which every critic
    without layer norm runs and a layer-normed one does not."""
    c = (ctypes.c_int * 3)()
    _lib.call("dppo_ppo_plan_critic", ctypes.byref(d.c()), _prec(precision), _lib.HEAD[d.critic_head],
              _lib.LAYERNORM[d.critic_layernorm], c)
    return dict(critic_tile_rows=c[0], critic_waves=c[1], critic_tile_capped=bool(c[2]))


def ppo_adv_stats(advantages, total, kf, perm_seed, epoch, start, rows, out, row_index=None):
    _lib.call("dppo_ppo_adv_stats", ptr(advantages), int(total), int(kf), ctypes.c_uint64(perm_seed), int(epoch),
              int(start), int(rows), ptr(row_index), ptr(out), stream_handle(advantages.device))
    return out


def ppo_adv_stats_all(advantages, total, kf, perm_seed, epoch0, n_epochs, rows_full, n_batch, out):
    """out fp64 [n_epochs * n_batch, 3]: every minibatch's advantage moments in one launch."""
    _check(out, (n_epochs * n_batch, 3), torch.float64, "out")
    _lib.call("dppo_ppo_adv_stats_all", ptr(advantages), int(total), int(kf), ctypes.c_uint64(perm_seed), int(epoch0),
              int(n_epochs), int(rows_full), int(n_batch), ptr(out), stream_handle(advantages.device))
    return out


def _check_quantiles(q_lo, q_hi):
    if not 0.0 <= float(q_lo) < float(q_hi) <= 1.0:
        raise ValueError(f"advantage quantiles: need 0 <= lower < upper <= 1, got ({q_lo}, {q_hi})")


def ppo_adv_quantiles_workspace(n_epochs, n_batch, device):
    nbytes = _lib.query("dppo_ppo_adv_quantiles_workspace_bytes", int(n_epochs), int(n_batch))
    if nbytes == 0:
        raise ValueError("ppo_adv_quantiles_workspace: n_epochs and n_batch must be > 0")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def ppo_adv_quantiles_all(advantages, total, kf, perm_seed, epoch0, n_epochs, rows_full, n_batch, q_lo, q_hi, out,
                          workspace=None):
    """out fp64 [n_epochs * n_batch, 2]: every minibatch's
    advantage quantiles {Q(q_lo), Q(q_hi)} (dppo_ppo_adv_quantiles_all: numpy.quantile's linear method in fp64 on
    exact order statistics; an empty window gets (-inf, +inf)). About ten launches, no host wait."""
    n_seg = int(n_epochs) * int(n_batch)
    _check_quantiles(q_lo, q_hi)
    if workspace is None:
        workspace = ppo_adv_quantiles_workspace(n_epochs, n_batch, advantages.device)
    if out.dtype != torch.float64 or tuple(out.shape) != (n_seg, 2) or not out.is_contiguous():
        raise ValueError(f"out: expected contiguous fp64 [{n_seg}, 2]")
    _lib.call("dppo_ppo_adv_quantiles_all", ptr(advantages), int(total), int(kf), ctypes.c_uint64(perm_seed), int(epoch0),
              int(n_epochs), int(rows_full), int(n_batch), float(q_lo), float(q_hi), ptr(workspace), ptr(out),
              stream_handle(advantages.device))
    return out


def ppo_adv_quantiles_state(n_epochs, n_batch, device):
    """(counts int32 [n_seg, 4, 256] zeroed, state int64 [n_seg, 9]) for the pass-level pair below."""
    n_seg = int(n_epochs) * int(n_batch)
    return (torch.zeros(n_seg, 4, 256, dtype=torch.int32, device=device),
            torch.zeros(n_seg, 9, dtype=torch.int64, device=device))


def ppo_adv_quantiles_count(advantages, total, kf, perm_seed, epoch0, n_epochs, rows_full, n_batch, pass_, state,
                            counts):
    """Pass pass_ (0..3) of the select: adds this rank's rows into counts (zero before pass 0; every pick leaves it
    zero). A data-parallel caller SUM-all-reduces counts before ppo_adv_quantiles_pick."""
    n_seg = int(n_epochs) * int(n_batch)
    _check(counts, (n_seg, 4, 256), torch.int32, "counts")
    _check(state, (n_seg, 9), torch.int64, "state")
    _lib.call("dppo_ppo_adv_quantiles_count", ptr(advantages), int(total), int(kf), ctypes.c_uint64(perm_seed),
              int(epoch0), int(n_epochs), int(rows_full), int(n_batch), int(pass_), ptr(state), ptr(counts),
              stream_handle(advantages.device))


def ppo_adv_quantiles_pick(n_epochs, n_batch, q_lo, q_hi, pass_, state, counts, out=None, n_global=None):
    """Advances every segment's four targets by pass pass_'s byte; pass 3 writes out fp64 [n_seg, 2]. n_global
    int64 [n_seg]: the segments' row counts over all ranks (None: the pass-0 counts' own sum)."""
    n_seg = int(n_epochs) * int(n_batch)
    _check_quantiles(q_lo, q_hi)
    _check(counts, (n_seg, 4, 256), torch.int32, "counts")
    _check(state, (n_seg, 9), torch.int64, "state")
    if out is not None and (out.dtype != torch.float64 or tuple(out.shape) != (n_seg, 2) or not out.is_contiguous()):
        raise ValueError(f"out: expected contiguous fp64 [{n_seg}, 2]")
    if n_global is not None:
        _check(n_global, (n_seg,), torch.int64, "n_global")
    _lib.call("dppo_ppo_adv_quantiles_pick", int(n_epochs), int(n_batch), float(q_lo), float(q_hi), int(pass_),
              ptr(n_global), ptr(state), ptr(counts), ptr(out), stream_handle(counts.device))
    return out


def ppo_hparams(gamma_denoising=0.99, clip_ploss_coef=0.01, clip_ploss_coef_base=0.01, clip_ploss_coef_rate=3.0,
                min_logprob_std=0.1, vf_coef=0.5, norm_adv=True, reward_horizon=4, loss_scale=1.0, global_rows=1,
                l2_deferred=False, learn_eta=False, clip_vloss_coef=None, old_values=None, adv_clip=False):
    """l2_deferred (ABI 8, DPPO_PPO_L2_DEFERRED): the actor's l2 gradient is left factored in grads
    for an optimizer step with l2_from_pl2 (or materialize_l2). learn_eta (ABI 9,
    DPPO_PPO_LEARN_ETA): the row tiles add d loss / d eta of a DDIM schedule into metrics[8].
    clip_vloss_coef (ABI 14, diffusion_ppo.py:110-116): the clipped value loss against old_values, the
    rollout's value pass (device fp32 [S*E], indexed by sample; the caller keeps it alive).
    adv_clip (DPPO_PPO_ADV_CLIP): the minibatch's adv_stats is fp64[5] {count, sum, sumsq, lo, hi} and the row
    tiles clamp the raw advantage to [lo, hi] (ppo_adv_quantiles_all computes the bounds)."""
    flags = (_lib.DPPO_PPO_L2_DEFERRED if l2_deferred else 0) | (_lib.DPPO_PPO_LEARN_ETA if learn_eta else 0) | (
        _lib.DPPO_PPO_ADV_CLIP if adv_clip else 0)
    clip = clip_vloss_coef is not None
    if clip and (old_values is None or old_values.dtype != torch.float32 or not old_values.is_cuda):
        raise ValueError("clip_vloss_coef needs the rollout's old values (fp32 device tensor)")
    if clip and not float(clip_vloss_coef) > 0:
        raise ValueError("clip_vloss_coef must be > 0")
    return _lib.DppoPpoHparams(float(gamma_denoising), float(clip_ploss_coef), float(clip_ploss_coef_base),
                               float(clip_ploss_coef_rate), float(min_logprob_std), float(vf_coef), int(bool(norm_adv)),
                               int(reward_horizon), float(loss_scale), int(global_rows), flags,
                               float(clip_vloss_coef) if clip else 0.0, old_values.data_ptr() if clip else None)


def ddim_eta_base(schedule):
    """fp32 [S][5] eta-independent rows of a DDIM schedule (ddim_buffers) for dppo_eta_step:
    {abar_prev, sqrt(abar_prev), sqrt(abar), sqrt(1 - abar), s = sigma / eta}."""
    return np.stack([schedule["ddim_alphas_prev"], schedule["ddim_sqrt_alphas_prev"], schedule["ddim_sqrt_alphas"],
                     schedule["ddim_sqrt_1m_alphas"], schedule["ddim_sfac"]], axis=1).astype(np.float32)


def eta_step(eta_state, metrics, step, lr, weight_decay, eta_min, eta_max, ddim_base, sched, eta_out=None,
             beta1=0.9, beta2=0.999, eps=1e-7, mode=0):
    """dppo_eta_step on the current stream: AdamW on the eta logit from metrics[8] (metrics=None:
    only re-derive the schedule's eta columns), then the DDIM rows of sched for the new eta."""
    _check(eta_state, (3,), torch.float32, "eta_state")
    _check(sched, (sched.shape[0], _lib.SCHED_COLS), torch.float32, "sched")
    _check(ddim_base, (sched.shape[0], 5), torch.float32, "ddim_base")
    if metrics is not None:
        _check(metrics, (16,), torch.float64, "metrics")
    _lib.call("dppo_eta_step", ptr(eta_state), ptr(metrics), int(step), float(lr), float(weight_decay), float(beta1),
              float(beta2), float(eps), int(mode), float(eta_min), float(eta_max), ptr(ddim_base), ptr(sched),
              int(sched.shape[0]), ptr(eta_out), stream_handle(eta_state.device))


def materialize_l2(d: ModelDims, precision, packed_actor, grads, workspace, batch_rows):
    """The actor's l2 gradient of an l2_deferred minibatch formed in place (dppo_materialize_l2)."""
    _lib.call("dppo_materialize_l2", ctypes.byref(_dims_c(d)), _prec(precision), ptr(packed_actor), ptr(grads),
              ptr(workspace), int(batch_rows), stream_handle(grads.device))


def _check_minibatch_buffers(d, precision, obs, chains, lp_old_mean, advantages, returns, actor_params, grads,
                             workspace, rows):
    """The buffers every PPO minibatch launch reads and writes, against the rollout's sample count n
    (returned) and the workspace a launch of `rows` rows needs."""
    n = obs.shape[0]
    kf = d.ft_denoising_steps
    _check(obs, (n, d.sd), torch.float32, "obs")
    _check(chains, (n, kf + 1, d.xd), torch.float32, "chains")
    _check(lp_old_mean, (n, kf), torch.float32, "lp_old_mean")
    _check(advantages, (n,), torch.float32, "advantages")
    _check(returns, (n,), torch.float32, "returns")
    na, nc = _n_params(d)
    _check(actor_params, (na,), torch.float32, "actor_params")
    _check(grads, (na + nc,), torch.float32, "grads")
    need = _workspace_bytes(d, _prec(precision), int(rows))
    if workspace.numel() < need:
        raise ValueError(f"workspace too small: {workspace.numel()} < {need}")
    return n


def ppo_minibatch(d: ModelDims, precision, hp, packed_ft, packed_critic, actor_params, sched, obs, chains, lp_old_mean,
                  advantages, returns, perm_seed, epoch, start, rows, workspace, grads, metrics, adv_stats=None,
                  row_index=None, part=None):
    n = _check_minibatch_buffers(d, precision, obs, chains, lp_old_mean, advantages, returns, actor_params, grads,
                                 workspace, rows)
    kf = d.ft_denoising_steps
    _check(metrics, (16,), torch.float64, "metrics")
    if row_index is not None:
        _check(row_index, (row_index.numel(),), torch.int64, "row_index")
        if row_index.numel() < start + rows:
            raise ValueError("row_index shorter than start + rows")
    args = (ctypes.byref(_dims_c(d)), _prec(precision), ctypes.byref(hp), ptr(packed_ft), ptr(packed_critic),
            ptr(actor_params), ptr(sched), ptr(obs), ptr(chains), ptr(lp_old_mean), ptr(advantages), ptr(returns),
            int(n * kf), ctypes.c_uint64(perm_seed), int(epoch), int(start), int(rows), ptr(row_index), ptr(adv_stats),
            ptr(workspace), ptr(grads), ptr(metrics))
    if part is None:
        _lib.call("dppo_ppo_minibatch", *args, stream_handle(obs.device))
    else:   # 1 = actor half, 2 = critic half, on the current stream (dppo_ppo_minibatch_part)
        _lib.call("dppo_ppo_minibatch_part", *args, int(part), stream_handle(obs.device))


class BoundMinibatch:
    """ppo_minibatch with the arguments that stay fixed over an update phase (rollout buffers,
    weights and images, workspace, gradients) validated and marshalled once; a call passes what
    changes per minibatch. The host's enqueue time per minibatch matters where minibatches are
    small (an 8-GPU rank's 6,250 rows: ~0.13 ms of GPU time each)."""

    def __init__(self, d: ModelDims, precision, packed_ft, packed_critic, actor_params, sched, obs, chains,
                 lp_old_mean, advantages, returns, perm_seed, workspace, grads, max_rows):
        n = _check_minibatch_buffers(d, precision, obs, chains, lp_old_mean, advantages, returns, actor_params, grads,
                                     workspace, max_rows)
        kf = d.ft_denoising_steps
        self.max_rows = int(max_rows)
        self._lib = _lib.load()
        self._dims = _dims_c(d)
        self._prec = _prec(precision)
        self._mid = (ptr(packed_ft), ptr(packed_critic), ptr(actor_params), ptr(sched), ptr(obs), ptr(chains),
                     ptr(lp_old_mean), ptr(advantages), ptr(returns), int(n * kf), ctypes.c_uint64(int(perm_seed)))
        self._tail = (ptr(workspace), ptr(grads))
        self._dev = obs.device
        self._keep = (packed_ft, packed_critic, actor_params, sched, obs, chains, lp_old_mean, advantages, returns,
                      workspace, grads)   # the pointers above stay valid while this object lives

    def __call__(self, hp, epoch, start, rows, metrics, adv_stats=None, part=None, stream=None):
        """metrics / adv_stats: device tensors, or device addresses (ints) of fp64[16] / fp64[3]
        (the update loop passes precomputed addresses); stream: a raw stream handle (default: the
        current stream)."""
        if not 0 < rows <= self.max_rows:
            raise ValueError(f"rows {rows} outside (0, {self.max_rows}]")
        if isinstance(metrics, torch.Tensor):
            if metrics.dtype != torch.float64 or metrics.numel() < 16:
                raise ValueError("metrics: expected fp64[16]")
            metrics = metrics.data_ptr()
        if isinstance(adv_stats, torch.Tensor):
            adv_stats = adv_stats.data_ptr()
        args = (ctypes.byref(self._dims), self._prec, ctypes.byref(hp)) + self._mid + (
            int(epoch), int(start), int(rows), None, adv_stats) + self._tail + (metrics,)
        st = stream_handle(self._dev) if stream is None else stream
        if part is None:
            rc = self._lib.dppo_ppo_minibatch(*args, st)
        else:
            rc = self._lib.dppo_ppo_minibatch_part(*args, int(part), st)
        _lib.check(rc, "dppo_ppo_minibatch")


class BoundOptimizerStep:
    """optimizer_step over a fixed range and fixed images, validated and marshalled once; a call
    passes the step, learning rate, metric source and tag (see BoundMinibatch)."""

    def __init__(self, d: ModelDims, precision, params, grads, m, v, weight_decay, beta1, beta2, eps, mode,
                 actor_params=None, packed_actor=None, critic_params=None, packed_critic=None,
                 defer_sampler_tables=False, l2_from_pl2=False, fused_pack=False, clear_grads=False, clip_scales=None):
        """fused_pack (ABI 11, DPPO_STEP_FUSED_PACK): AdamW and the image in one launch where the
        library can (one network whose parameters are the range); clear_grads (DPPO_STEP_CLEAR_GRADS):
        the step zeroes the range's gradients and the `clear` ranges of each call after reading them.
        clip_scales: the range's per-variable clip scales (grad_clip_scales; a device tensor the launch
        reads at run time), applied as the step reads each gradient (dppo_optimizer_step_clip)."""
        n = params.numel()
        for t, nm in ((grads, "grads"), (m, "m"), (v, "v")):
            if t.numel() != n:
                raise ValueError(f"{nm}: expected {n} elements")
        self._lib = _lib.load()
        self._dims = _dims_c(d)
        mode_i = _step_mode(mode, defer_sampler_tables, l2_from_pl2, fused_pack, clear_grads)
        self._head = (ctypes.byref(self._dims), _prec(precision), ptr(params), ptr(grads), ptr(m), ptr(v), int(n))
        self._hp = (float(weight_decay), float(beta1), float(beta2), float(eps), mode_i, ptr(actor_params),
                    ptr(packed_actor), ptr(critic_params), ptr(packed_critic))
        self._dev = params.device
        self._keep = (params, grads, m, v, actor_params, packed_actor, critic_params, packed_critic, clip_scales)
        self._fn = self._lib.dppo_optimizer_step_ex
        self._clip = ()
        if clip_scales is not None:
            self._fn = self._lib.dppo_optimizer_step_clip
            self._clip = (ptr(clip_scales), _clip_nets(d, n, clip_scales))

    def __call__(self, step, lr, metrics=None, metrics_out=None, n_metrics=0, metrics_tag=0, stream=None, clear=None):
        """metrics_out: a device tensor or a dppo_host_alloc address (as optimizer_step); metrics: a
        device tensor or address; stream: a raw stream handle (default: the current stream); clear: a
        ClearRanges (byte ranges zeroed after the step's last read, dppo_optimizer_step_ex)."""
        cp, cb, cn = (None, None, 0) if clear is None else clear.args
        _lib.check(self._fn(*self._head, int(step), float(lr), *self._hp, _address(metrics), _address(metrics_out),
                            int(n_metrics), ctypes.c_uint64(int(metrics_tag)), cp, cb, cn,
                            stream_handle(self._dev) if stream is None else stream, *self._clip),
                   "dppo_optimizer_step")


class ClearRanges:
    """The non-gradient byte ranges a minibatch part zeroes first (dppo_ppo_clear_ranges: metric slots
    of `metrics`, the workspace's accumulators for `rows`), marshalled for dppo_optimizer_step_ex, so
    the optimizer step before that minibatch clears them and the minibatch runs with
    DPPO_PPO_PRECLEARED. metrics: a device address or fp64[16] tensor; workspace: the uint8 tensor."""

    def __init__(self, d: ModelDims, precision, rows, workspace, metrics, part):
        lib = _lib.load()
        self._ptrs = (ctypes.c_void_p * 4)()
        self._bytes = (ctypes.c_size_t * 4)()
        cnt = ctypes.c_int(0)
        _lib.check(lib.dppo_ppo_clear_ranges_ln(ctypes.byref(_dims_c(d)), _prec(precision), _lib.HEAD[d.critic_head],
                                                _lib.LAYERNORM[d.critic_layernorm], int(rows), ptr(workspace),
                                                _address(metrics), int(part), self._ptrs, self._bytes, ctypes.byref(cnt)),
                   "dppo_ppo_clear_ranges")
        self.count = cnt.value
        self.args = (self._ptrs, self._bytes, self.count)
        self._keep = (workspace, metrics)

    def ranges(self):
        return [(int(self._ptrs[i]), int(self._bytes[i])) for i in range(self.count)]


def q_sched_table(schedule):
    """[K][2] fp32 {sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod)}: the q_sample buffers of
    diffusion.py:62-65 (computed in fp32 like the TF buffers)."""
    ac = np.asarray(schedule["alphas_cumprod"], np.float32)
    return np.stack([np.sqrt(ac), np.sqrt(np.float32(1.0) - ac)], axis=1).astype(np.float32)


def pretrain_minibatch(d: ModelDims, precision, packed_actor, actor_params, sched, qsched, x_start, cond, t, noise,
                       workspace, grads, metrics, global_rows=None, loss_scale=1.0):
    """p_losses (diffusion.py:186-194) and its actor gradient for one batch; see include/dppo.h.
    Returns the loss as a device scalar (metrics[0] / (global_rows * xd) * loss_scale).
    The workspace may hold any bytes; all 16 metrics are zeroed first; grads beyond the actor's count are not
    touched; t is not validated (a value outside [0, denoising_steps) is the caller's error)."""
    n = x_start.shape[0]
    g = n if global_rows is None else int(global_rows)
    _check(x_start, (n, d.xd), torch.float32, "x_start")
    _check(cond, (n, d.sd), torch.float32, "cond")
    _check(t, (n,), torch.int32, "t")
    _check(noise, (n, d.xd), torch.float32, "noise")
    _check(qsched, (d.denoising_steps, 2), torch.float32, "qsched")
    na = _n_params(d)[0]
    _check(actor_params, (na,), torch.float32, "actor_params")
    if grads.numel() < na:
        raise ValueError("grads: needs at least the actor parameter count")
    _check(metrics, (16,), torch.float64, "metrics")
    need = _workspace_bytes(d, _prec(precision), int(n))
    if workspace.numel() < need:
        raise ValueError(f"workspace too small: {workspace.numel()} < {need}")
    _lib.call("dppo_pretrain_minibatch", ctypes.byref(_dims_c(d)), _prec(precision), ptr(packed_actor), ptr(actor_params),
              ptr(sched), ptr(qsched), ptr(x_start), ptr(cond), ptr(t), ptr(noise), int(n), int(g), float(loss_scale),
              ptr(workspace), ptr(grads), ptr(metrics), stream_handle(x_start.device))
    return metrics[0] * (float(loss_scale) / (g * d.xd))


# bc_chunk's default workspace budget: a dppo_bc_minibatch over n samples takes a PPO workspace of n * K' rows
# (about 7.3 KB a row in the 2-byte precisions at hopper's widths, 14.6 KB in fp32), and the entry refuses one of
# 2 GiB or more
BC_WORKSPACE_BYTES = 1 << 29


def bc_chunk(d: ModelDims, precision, n, budget=BC_WORKSPACE_BYTES):
    """Samples per dppo_bc_minibatch call when n samples are walked in accumulate calls over one workspace of at
    most `budget` bytes (dppo_ppo_workspace_bytes(chunk * K') <= budget < 2 GiB): n itself where that fits, else
    the calls' even share, ceil(n / calls) with the fewest calls that fit. Host arithmetic only."""
    n, kf, prec = int(n), d.ft_denoising_steps, _prec(precision)
    if n < 1 or not 0 < budget < (1 << 31):
        raise ValueError(f"bc_chunk: need n >= 1 and 0 < budget < 2 GiB, got n = {n}, budget = {budget}")
    fits = lambda s: _workspace_bytes(d, prec, s * kf) <= budget
    if fits(n):
        return n
    if not fits(1):
        raise ValueError(f"bc_chunk: one sample's workspace ({_workspace_bytes(d, prec, kf)} B) exceeds the budget {budget}")
    lo, hi = 1, n          # fits(lo), not fits(hi): the workspace grows with the rows
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    calls = -(-n // lo)
    return -(-n // calls)


def bc_minibatch(d: ModelDims, precision, packed_ft, actor_params, sched, cond, chains, workspace, grads, metrics,
                 coeff, min_logprob_std=0.1, global_samples=None, loss_scale=1.0, accumulate=False, l2_deferred=False):
    """The behaviour-cloning term coeff * bc_loss (diffusion_ppo.py:63-71) and its actor gradient for n
    observations cond [n, SD] and their base-policy chains [n, K'+1, XD]; see include/dppo.h. The sum of the
    clipped log-probs lands in metrics[DPPO_METRIC_BC_LOGPROB]; accumulate adds to it and to grads[:actor count]
    instead of overwriting them. grads beyond the actor's count and every other metric slot are not touched.
    Returns bc_loss of what the slot holds so far as a device scalar (-slot / (global_samples * K' * xd))."""
    n = cond.shape[0]
    g = n if global_samples is None else int(global_samples)
    kf = d.ft_denoising_steps
    _check(cond, (n, d.sd), torch.float32, "cond")
    _check(chains, (n, kf + 1, d.xd), torch.float32, "chains")
    na = _n_params(d)[0]
    _check(actor_params, (na,), torch.float32, "actor_params")
    for t, nm in ((packed_ft, "packed_ft"), (sched, "sched"), (workspace, "workspace"), (grads, "grads")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{nm}: expected a device tensor")
    if grads.dtype != torch.float32 or not grads.is_contiguous() or grads.numel() < na:
        raise ValueError("grads: needs contiguous fp32 of at least the actor parameter count")
    _check(metrics, (16,), torch.float64, "metrics")
    for t, nm in ((chains, "chains"), (actor_params, "actor_params"), (grads, "grads"), (metrics, "metrics"),
                  (workspace, "workspace"), (packed_ft, "packed_ft"), (sched, "sched")):
        if t.device != cond.device:
            raise ValueError(f"{nm}: on {t.device}, cond on {cond.device}")
    need = _workspace_bytes(d, _prec(precision), int(n * kf))
    if workspace.numel() < need:
        raise ValueError(f"workspace too small: {workspace.numel()} < {need}")
    flags = (_lib.DPPO_BC_ACCUMULATE if accumulate else 0) | (_lib.DPPO_PPO_L2_DEFERRED if l2_deferred else 0)
    _lib.call("dppo_bc_minibatch", ctypes.byref(_dims_c(d)), _prec(precision), ptr(packed_ft), ptr(actor_params),
              ptr(sched), ptr(cond), ptr(chains), int(n), int(g), float(min_logprob_std), float(coeff),
              float(loss_scale), int(flags), ptr(workspace), ptr(grads), ptr(metrics), stream_handle(cond.device))
    return metrics[_lib.DPPO_METRIC_BC_LOGPROB] * (-1.0 / (g * kf * d.xd))


def adamw(params, grads, m, v, step, lr, weight_decay=0.004, beta1=0.9, beta2=0.999, eps=1e-7, mode="keras"):
    n = params.numel()
    for t, nm in ((grads, "grads"), (m, "m"), (v, "v")):
        _check(t, (n,), torch.float32, nm)
    _lib.call("dppo_adamw", ptr(params), ptr(grads), ptr(m), ptr(v), int(n), int(step), float(lr), float(weight_decay),
              float(beta1), float(beta2), float(eps),
              _lib.DPPO_ADAMW_KERAS if mode == "keras" else _lib.DPPO_ADAMW_TORCH, stream_handle(params.device))


def _forget_sched(address):
    try:
        _lib.call("dppo_forget_sched", ctypes.c_void_p(address))
    except Exception:   # interpreter shutdown: the library may be gone, and so is its table
        pass


def sched_set_params(sched, denoised_clip_value=1.0, predict_epsilon=True):
    """Record a schedule table's attributes (dppo_sched_set_params, include/dppo.h): the clip bound of x_recon
    (None = no clip) and the parameterisation. The library keys the record by the table's ADDRESS, so it is erased
    when the tensor is freed (dppo_forget_sched), as an image's attributes are. Returns sched."""
    if (not isinstance(sched, torch.Tensor) or sched.dtype != torch.float32 or sched.dim() != 2
            or sched.shape[1] != _lib.SCHED_COLS or not sched.is_contiguous()):
        raise ValueError(f"sched: expected a contiguous float32 [rows, {_lib.SCHED_COLS}] tensor")   # host or device
    clip = 0.0 if denoised_clip_value is None else float(denoised_clip_value)
    _lib.call("dppo_sched_set_params", ptr(sched), clip, int(not predict_epsilon))
    fin = getattr(sched, "_dppo_forget", None)
    if fin is None or not fin.alive:
        sched._dppo_forget = weakref.finalize(sched, _forget_sched, sched.data_ptr())
        sched._dppo_forget.atexit = False
    return sched


def sched_table(schedule, predict_epsilon=True):
    """[rows][8] fp32 table (include/dppo.h) from the fp32 DDPM buffers, or from the DDIM
    sub-sequence coefficients (model/diffusion/sampling.py: ddpm_buffers / ddim_buffers).
    predict_epsilon=False (diffusion.py:117-134, x_recon = the network's output): the x0 rows c0 = 0, c1 = -1, the
    rest as for DDPM; the table's record must say so too (sched_set_params)."""
    if "ddim_c0" in schedule:
        assert predict_epsilon, "DDIM requires predicting epsilon for now."
        tab = np.zeros((len(schedule["ddim_c0"]), _lib.SCHED_COLS), np.float32)
        for j, k in enumerate(("ddim_c0", "ddim_c1", "ddim_c2", "ddim_c3", "ddim_logvar")):
            tab[:, j] = schedule[k]
        tab[:, 5] = 0.0                      # eval: no noise on any DDIM row (diffusion_vpg.py:303-306)
        tab[:, 6] = 1.0
        tab[:, 7] = schedule["ddim_sfac"]    # sigma / eta: the learnable-eta gradient's row factor
        return tab
    K = len(schedule["betas"])
    tab = np.zeros((K, _lib.SCHED_COLS), np.float32)
    if predict_epsilon:
        tab[:, 0] = schedule["sqrt_recip_alphas_cumprod"]
        tab[:, 1] = schedule["sqrt_recipm1_alphas_cumprod"]
    else:
        tab[:, 1] = -1.0
    tab[:, 2] = schedule["ddpm_mu_coef1"]
    tab[:, 3] = schedule["ddpm_mu_coef2"]
    tab[:, 4] = schedule["ddpm_logvar_clipped"]
    tab[:, 5] = 1e-3                         # eval: t > 0 clips at 1e-3, t = 0 has no noise (:308-312)
    tab[0, 6] = 1.0
    return tab


def adam_alpha(lr, beta1, beta2, step):
    return lr * math.sqrt(1 - beta2 ** step) / (1 - beta1 ** step)
