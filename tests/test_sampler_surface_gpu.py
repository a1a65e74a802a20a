"""The sampler's knobs, geometry and kernel paths against the float64 oracle.

The other GPU files run dppo_sample at the shipped hopper / walker shapes with every knob at its
default. Part A moves every knob of dppo_sample off its default, one per case, on the split kernel
(csrc/sampler_split.hip) and on the weight-streaming kernel (csrc/sampler.hip); part B runs
dppo_sample (and dppo_sample_step) at geometries that reach the remaining instantiations, or pins
that a geometry without one is refused before anything is enqueued; part C runs the kernel paths the
plan chooses from the env count and K'.

Reference: oracle.dppo_oracle.sample in float64; for 2-byte operands it rounds at the kernel's
rounding points (rnd = _rnd(precision), round_h3 = not split, as test_sampler_injected_noise).
Inputs are injected x_T and noise unless a case says Philox. Every figure is printed before it is
asserted (pytest -s shows them). Bounds (tests/test_kernels_gpu.py, test_sampler_split_resident_gpu.py):

  precision  actions                  chains
  fp32       max < 2e-4               max < 2e-4
  bf16       q99 < 2e-3, max < 0.1    mean < 2e-3, and the mean of every stored chain row
  fp16       q99 < 1e-3, max < 0.1    mean < 1e-3, and the mean of every stored chain row

For K != 20 every bound scales by c1(K) / c1(20), c1 = sqrt(1 / abar_{K-1} - 1) the factor the first
x0 reconstruction multiplies eps errors by (406 at K = 20), read from the schedule table
(_k_scale: K = 62 and 63 give 1258 / 406 = 3.10 and 1278 / 406 = 3.15).

Part A (hopper E = 37 in fp32 / bf16 / fp16 on the split kernel; the streaming kernel in-process:
walker fp32 E = 37 and hopper bf16 E = 513). Each case that moves a value proves on the CPU that it
can fail (_assert_moved): the oracle at the case's setting and at the default, on the same inputs,
differ by >= 10x the bound in the statistics the GPU comparison uses (fp32: max of actions and of
chains; 2-byte: q99 of actions and the chain mean).

  case               setting                                  narrowed
  final-clip0.5      final_clip = 0.5
  final-clip-off     final_clip 0.0 and -1.0 == None, bitwise
  randn-clip1        randn_clip = 1.0
  min-std0.4         min_sampling_std = 0.4
  min-std0           min_sampling_std = 0.0 (the schedule's)  fp32 only (*)
  eval               deterministic = True (DDPM)              fp32 only (*)
  eval-final-clip    deterministic = True, final_clip = 0.5
  env-offset48       Philox noise, env_offset = 48; and rows [16, E + 16) of an env_offset = 0 launch
                     over E + 16 envs against an env_offset = 16 launch of E
  xT-injected        x_T injected, Philox step noise
  noise-injected     step noise injected, Philox x_T          fp32 and fp16 (**)
  no-chains          want_chains = False: actions bit-equal to the launch with chains

(*) min_sampling_std = 0 and the eval rule change the std of the last steps only (where the schedule's
std is below 0.1): the chain mean moves 0.0093, under 10x the bf16 (0.02) and fp16 (0.01) bounds, so
these run in fp32 (eval with final_clip moves the last row enough and runs everywhere). (**) x_T's
influence decays over the ten base steps: against the injected x_T the chain mean moves 0.0196 to 0.0205,
not safely 10x the bf16 bound (0.02) but 10x fp16's (0.01).

Part B: accept / reject table of dppo_sample (read from dispatch_sample, launch_sample_q,
split_plan; validate_dims, csrc/api.hip, is wider). "in" = XD + time_dim + SD; k = in-layer k-steps
(packed_ksteps: 16 inputs per k-step in fp32, 32 in 2-byte, rounded up to even). E = 17 unless stated.

  split kernel, 2-byte: H = 512, XD % 4 == 0, XD + SD <= 64, K <= 62, E <= 512, its LDS <= 160 KiB
  split kernel, fp32:   H = 512, XD == 12, XD + SD <= 32, K <= 62, <= 32 groups (256 CUs), LDS <= 160 KiB
                        (whatever time_dim is: the time part of the in-layer is a packed table)
  streaming, 2-byte:    H = 512, k in {2, 4} (in <= 128), LDS <= 160 KiB
  streaming, fp32:      H in {256, 512}, k == 4 (33 <= in <= 64), LDS <= 160 KiB

  geometry                                     fp32                  2-byte
  narrow: action 2 (XD 8)                      streams               split
  xd3: action 1 x horizon 3 (in 30)            REJECTED (k = 2)      streams (XD % 4)
  h8a3: horizon 8 (XD 24)                      streams               split
  h8a4: horizon 8 x action 4 (XD 32)           streams               split
  h8a4-e513: the same at E = 513               streams               streams (16 XD = the block)
  td8 / td32: time_dim 8 / 32                  split                 split
  narrow-td32: XD 8, time_dim 32 (in 51)       streams               split
  cond2-hopper: cond_steps 2 (SD 22)           streams               split
  cond2-walker: cond_steps 2 (SD 34, in 74)    REJECTED (k = 6)      split (XD + SD = 58)
  cond2-walker-e513: the same at E = 513       REJECTED (k = 6)      streams, k = 4
  tiny: obs 3, action 1 (in 23)                REJECTED (k = 2)      split
  obs3: obs 3, XD 12 (in 31)                   split                 split
  ah256: actor_hidden 256                      streams               REJECTED
  ah256-walker: the same at XD 24              streams               REJECTED
  ah128                                        REJECTED              REJECTED
  ah384                                        REJECTED (layout)     REJECTED
  k62: denoising_steps 62, K' 10               streams (split LDS)   streams (split LDS)
  k62-cond2: K 62, cond_steps 2                streams               split (its last K)
  k62-obs3: K 62, obs 3                        split (its last K)    streams (split LDS)
  k63: denoising_steps 63, K' 10               streams               streams
  k100-h8a4: K 100, XD 32                      REJECTED (LDS)        REJECTED (LDS)
  in128: time_dim 32, SD 64, XD 32             REJECTED (k = 8)      streams, k = 4 (the widest)
  in160: time_dim 64, SD 64, XD 32             no image: dppo_pack_actor refuses time_dim > 32

Messages (code DPPO_EUNSUPPORTED = 3): "sampler: hidden %d / action chunk %d / in-layer k-steps %d
not instantiated"; "sampler needs %zu B of LDS"; fp32 actor_hidden 384 passes the dispatch's
H / 256 == 1 and is refused by the launcher's layout check, "sampler: hidden 384 not supported at
this precision". A refusal leaves actions, chains (and dppo_sample_step's device copy of cond and the
host actions) untouched and the stream usable.

Part C: fp32 hopper at E = 130 and 512 (one member set that switches actors mid-launch: K' = 10, 1,
19) and E = 128 (two member sets); the streaming kernel at K' = K and K' = 1; DDIM eval in 2-byte and
DDIM with final_clip. Each launch runs twice on the same inputs and must be bit-identical.

Observed on an MI355X (256 CUs), largest over a part's cases, observed | bound:
  A fp32  actions max 2.2e-6 | 2e-4, chains max 2.2e-6 | 2e-4
  A bf16  q99 1.7e-3 | 2e-3, max 4.8e-3 | 0.1, chain mean 1.8e-4 | 2e-3, worst row 2.0e-4 | 2e-3
  A fp16  q99 4.0e-5 | 1e-3, max 1.6e-4 | 0.1, chain mean 2.1e-6 | 1e-3, worst row 2.9e-6 | 1e-3
  B fp32  actions max 2.5e-5 | 2e-4, chains max 2.5e-5 | 2e-4
  B bf16  q99 9.2e-4 | 2e-3, max 4.3e-3 | 0.1, chain mean 4.4e-5 | 2e-3, worst row 4.8e-5 | 2e-3
  B fp16  q99 2.6e-4 | 1e-3, max 1.1e-3 | 0.1, chain mean 2.1e-5 | 1e-3, worst row 2.8e-5 | 1e-3
  B K = 62 / 63 (bounds x 3.10 / 3.15): fp32 max 9.5e-7 | 6.2e-4; bf16 q99 2.4e-4 | 6.2e-3, chain mean
          3.2e-5 | 6.2e-3; fp16 q99 6.3e-5 | 3.1e-3, chain mean 9.2e-6 | 3.1e-3 (none needed the factor)
  C fp32  actions max 4.2e-6 | 2e-4, chains max 6.9e-6 | 2e-4
  C bf16  q99 1.4e-3 | 2e-3, max 3.6e-3 | 0.1, chain mean 1.3e-4 | 2e-3, worst row 1.3e-4 | 2e-3
  C fp16  q99 1.5e-4 | 1e-3, max 8.8e-4 | 0.1, chain mean 8.5e-6 | 1e-3, worst row 1.3e-5 | 1e-3
The env_offset shards were bit-equal in all five configs. Plans of part C (kernel, members, sets,
workgroups): fp32 hopper E = 130: (2, 8, 1, 128) at K' = 10, 1, 19; E = 512: (2, 8, 1, 256) at the same;
E = 128: (2, 8, 2, 128); streaming hopper bf16 / fp16 E = 513: (0, 0, 0, 33); walker fp32 E = 37:
(0, 0, 0, 3); DDIM eval bf16 / fp16 E = 37: (2, 2, 1, 16); DDIM final_clip fp32: (2, 8, 1, 64).
h8a4-e513 in bf16 / fp16 failed before the streaming kernel's fix (XD = 32 on 8 waves left no thread
to refresh the time embedding: every step ran with t_emb(K - 1)): q99 0.64, chain mean 0.065. in128
takes the same path.
"""
import functools
import json
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from oracle import philox as PX
from tests.helpers import HOPPER, HOPPER_DDIM, NARROW, WALKER, make_models, to_f64
from tests.test_kernels_gpu import _rnd, _setup

gpu = pytest.mark.gpu

PRECISIONS = ("fp32", "bf16", "fp16")
TOL = {"fp32": 2e-4, "bf16": 2e-3, "fp16": 1e-3}
MAX_2B = 0.1
SEED, CALL = 987654321, 3
SENTINEL = -7.25


# ------------------------------------------------------------------------------------------------
# CPU half: inputs, the oracle, the statistics
# ------------------------------------------------------------------------------------------------
def _dims(dims):
    from diffusionpolicyoptimization_amd import ops
    return ops.ModelDims(**dims)


def _split(dims, precision, E):
    """Does the plan pick the split kernel (host arithmetic: no launch)?"""
    from diffusionpolicyoptimization_amd import ops
    return ops.sampler_plan(_dims(dims), precision, E)["kernel"] == 2


@functools.lru_cache(maxsize=None)
def _c1(K):
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    return float(ddpm_buffers(K)["sqrt_recipm1_alphas_cumprod"][K - 1])


def _k_scale(dims):
    """Bound factor of a DDPM geometry with K != 20: c1(K) / c1(20)."""
    K = dims["denoising_steps"]
    return 1.0 if K == 20 or dims.get("time_stride", 1) > 1 else _c1(K) / _c1(20)


class _Inputs:
    """Seeded models, schedule, state, x_T and step noise of (dims, E); no GPU needed. The models and
    the schedule are _setup's (tests/test_kernels_gpu.py) for the same dims, seed 0."""

    def __init__(self, dims, E, seed=1, eta=1.0):
        from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
        self.dims, self.E, self.eta = dims, E, eta
        self.d = d = _dims(dims)
        self.model = O.Model.from_dims(dims)
        self.base, self.ft, _ = make_models(0, {k: v for k, v in dims.items() if k != "time_stride"})
        self.K = K = d.denoising_steps
        self.sched = O.ddim_schedule(K * d.time_stride, K, eta) if d.time_stride > 1 else ddpm_buffers(K)
        rng = np.random.default_rng(seed)
        self.state = rng.uniform(-1, 1, (E, d.cond_steps, d.obs_dim)).astype(np.float32)
        self.xT = rng.standard_normal((E, d.horizon_steps, d.action_dim)).astype(np.float32)
        self.z = rng.standard_normal((K, E, d.horizon_steps, d.action_dim)).astype(np.float32)

    def philox(self, env_offset=0, E=None):
        """(x_T, z) the kernel draws itself for (SEED, CALL, env_offset)."""
        d, K, E = self.d, self.K, E or self.E
        sh = (E, d.horizon_steps, d.action_dim)
        xT = PX.sampler_normals(SEED, CALL, env_offset, E, d.xd, K).reshape(sh)
        z = np.stack([PX.sampler_normals(SEED, CALL, env_offset, E, d.xd, i).reshape(sh) for i in range(K)])
        return xT, z

    def oracle(self, precision, xT=None, z=None, state=None, **kw):
        split = _split(self.dims, precision, self.E)
        return O.sample(to_f64(self.base), to_f64(self.ft), self.sched,
                        (self.state if state is None else state).astype(np.float64),
                        self.xT if xT is None else xT, self.z if z is None else z, self.d.ft_denoising_steps,
                        rnd=_rnd(precision), round_h3=not split, **{"model": self.model, **kw})


def _stats(act, ch, ref_a, ref_c):
    """The statistics of the bounds table: actions max / q99, chains max / mean / per stored row mean."""
    da, dc = np.abs(act - ref_a), np.abs(ch - ref_c)
    rows = dc.mean(axis=(0, 2, 3))
    return dict(act_max=float(da.max()), act_q99=float(np.quantile(da, 0.99)), chain_max=float(dc.max()),
                chain_mean=float(dc.mean()), chain_row_max=float(rows.max()), chain_last_row=float(rows[-1]))


def _bounds(precision, scale=1.0):
    t = TOL[precision] * scale
    if precision == "fp32":
        return dict(act_max=t, chain_max=t)
    return dict(act_q99=t, act_max=MAX_2B * scale, chain_mean=t, chain_row_max=t)


def _check(label, precision, st, scale=1.0, **extra):
    b = _bounds(precision, scale)
    print(json.dumps(dict(case=label, precision=precision, observed=st, bound=b, **extra)))
    bad = {k: (st[k], v) for k, v in b.items() if not st[k] < v}
    assert not bad, (label, bad)


def _assert_moved(label, precision, case, other):
    """The oracle results `case` and `other` ((actions, chains)) differ by >= 10x the bound in the
    statistics the GPU comparison uses."""
    st = _stats(case[0], case[1], other[0], other[1])
    t = 10 * TOL[precision]
    if precision == "fp32":
        need = dict(act_max=t, chain_max=t)
    else:
        need = dict(act_q99=t, chain_mean=t)
    print(json.dumps(dict(case=label, precision=precision, moved=st, needs=need)))
    bad = {k: (st[k], v) for k, v in need.items() if not st[k] >= v}
    assert not bad, (label, bad)


# ------------------------------------------------------------------------------------------------
# GPU half
# ------------------------------------------------------------------------------------------------
class _Gpu:
    """The device half of an _Inputs at one precision: _setup's images and tables."""

    def __init__(self, inp, precision, cuda):
        import torch
        from diffusionpolicyoptimization_amd import ops
        self.inp, self.precision, self.cuda = inp, precision, cuda
        d, base, ft, _, sched, tab, pb, pf, _ = _setup(inp.dims, cuda, eta=inp.eta)
        assert d == inp.d and all(np.array_equal(ft[k], inp.ft[k]) for k in ft)
        self.d, self.tab = d, tab
        self.packb, self.packf = ops.pack_actor(d, pb, precision), ops.pack_actor(d, pf, precision)
        self.T = lambda x: torch.tensor(np.ascontiguousarray(x, np.float32), device=cuda)
        self.plan = ops.sampler_plan(d, precision, inp.E)

    def sample(self, xT="inj", z="inj", state=None, E=None, **kw):
        """One dppo_sample -> (actions, chains | None) as float32 arrays in the oracle's shapes; xT / z:
        'inj' (the inputs'), None (the kernel's Philox draws) or an array."""
        import torch
        from diffusionpolicyoptimization_amd import ops
        inp, d = self.inp, self.d
        E = E or inp.E
        state = inp.state if state is None else state
        xT = inp.xT if isinstance(xT, str) else xT
        z = inp.z if isinstance(z, str) else z
        act, ch = ops.sample(d, self.precision, self.packb, self.packf, self.tab, self.T(state.reshape(E, -1)),
                             x_T=None if xT is None else self.T(xT.reshape(E, -1)),
                             noise=None if z is None else self.T(z.reshape(inp.K, E, -1)),
                             seed=SEED, call_id=CALL, **kw)
        torch.cuda.synchronize()
        act = act.cpu().numpy().reshape(E, d.horizon_steps, d.action_dim)
        if ch is not None:
            ch = ch.cpu().numpy().reshape(E, d.ft_denoising_steps + 1, d.horizon_steps, d.action_dim)
            assert np.isfinite(ch).all()
        assert np.isfinite(act).all()
        return act, ch

    def twice(self, **kw):
        """Two launches on the same inputs, bit-identical."""
        a0, c0 = self.sample(**kw)
        a1, c1 = self.sample(**kw)
        assert a0.tobytes() == a1.tobytes() and c0.tobytes() == c1.tobytes(), "two launches on the same inputs differ"
        return a0, c0


# ------------------------------------------------------------------------------------------------
# A. every knob off its default, one per case
# ------------------------------------------------------------------------------------------------
# (dims name, precision, E, kernel the plan must pick)
A_CONFIGS = [("hopper", "fp32", 37, 2), ("hopper", "bf16", 37, 2), ("hopper", "fp16", 37, 2),
             ("walker", "fp32", 37, 0), ("hopper", "bf16", 513, 0)]
A_DIMS = dict(hopper=HOPPER, walker=WALKER)
FP32_ONLY = ("fp32",)
# name -> (ops.sample keywords, does the oracle move against the default (else: no proof), precisions)
A_CASES = {
    "final-clip0.5": (dict(final_clip=0.5), "all", PRECISIONS),
    "final-clip-off": ({}, None, PRECISIONS),
    "randn-clip1": (dict(randn_clip=1.0), "all", PRECISIONS),
    "min-std0.4": (dict(min_sampling_std=0.4), "all", PRECISIONS),
    "min-std0": (dict(min_sampling_std=0.0), "all", FP32_ONLY),
    "eval": (dict(deterministic=True), "all", FP32_ONLY),
    "eval-final-clip": (dict(deterministic=True, final_clip=0.5), "all", PRECISIONS),
    "env-offset48": (dict(env_offset=48), "all", PRECISIONS),
    "xT-injected": ({}, "all", PRECISIONS),
    "noise-injected": ({}, "all", ("fp32", "fp16")),
    "no-chains": ({}, None, PRECISIONS),
}
A_PARAMS = [(c, n, p, E) for c, (_, _, precs) in A_CASES.items() for n, p, E, _ in A_CONFIGS if p in precs]
A_IDS = [f"{c}-{n}-{p}-E{E}" for c, n, p, E in A_PARAMS]
_ORACLE_KW = dict(min_sampling_std="min_std")


def _okw(kw):
    return {_ORACLE_KW.get(k, k): v for k, v in kw.items() if k != "env_offset"}


@functools.lru_cache(maxsize=None)
def _a_inputs(name, E):
    return _Inputs(A_DIMS[name], E)


@functools.lru_cache(maxsize=None)
def a_reference(case, name, precision, E):
    """The CPU half of a part-A case: (inputs, (x_T, z) fed to the oracle, oracle at the case), with
    the case's discriminating power asserted (_assert_moved). Callable without a GPU."""
    kw, moves, _ = A_CASES[case]
    inp = _a_inputs(name, E)
    xT, z = inp.xT, inp.z
    if case == "env-offset48":
        xT, z = inp.philox(48)
    elif case == "xT-injected":
        z = inp.philox()[1]
    elif case == "noise-injected":
        xT = inp.philox()[0]
    ref = inp.oracle(precision, xT, z, **_okw(kw))
    label = f"{case}-{name}-{precision}-E{E}"
    if case == "env-offset48":        # against the draws of env_offset 0
        other = inp.oracle(precision, *inp.philox(0))
    elif case in ("xT-injected", "noise-injected"):   # against both sources injected: a launch that took the wrong one
        other = inp.oracle(precision)
    elif moves:
        other = inp.oracle(precision, xT, z)
    if moves:
        _assert_moved(label, precision, ref, other)
    if case == "eval-final-clip":     # each of the two knobs alone moves it too
        _assert_moved(label + " vs eval", precision, ref, inp.oracle(precision, deterministic=True))
        if precision == "fp32":
            _assert_moved(label + " vs final_clip", precision, ref, inp.oracle(precision, final_clip=0.5))
    if case == "randn-clip1":         # about a third of the draws clip, on either side
        frac = float((np.abs(inp.z) > 1.0).mean())
        assert 0.25 < frac < 0.4 and (inp.z > 1.0).any() and (inp.z < -1.0).any(), frac
    if case in ("min-std0", "min-std0.4", "eval"):   # the clamp holds for some steps and not for others
        std = np.exp(0.5 * np.asarray(inp.sched["ddpm_logvar_clipped"], np.float64))
        lo = {"min-std0": 0.1, "min-std0.4": 0.4, "eval": 0.1}[case]
        assert (std < lo).any() and (std > lo).any(), std
    return inp, (xT, z), ref


@pytest.mark.parametrize("case,name,precision,E", A_PARAMS, ids=A_IDS)
def test_knob_moves_the_oracle(case, name, precision, E):
    """CPU: the part-A case can fail (a_reference's _assert_moved); no launch."""
    a_reference(case, name, precision, E)


@gpu
@pytest.mark.parametrize("case,name,precision,E", A_PARAMS, ids=A_IDS)
def test_knob_off_default(cuda, case, name, precision, E):
    """dppo_sample with one knob off its default (A_CASES) on the kernel the plan picks for the
    config (A_CONFIGS: the split kernel, or the weight-streaming kernel) against O.sample at the same
    setting: actions and every stored chain row."""
    kw = A_CASES[case][0]
    inp, (xT, z), ref = a_reference(case, name, precision, E)
    g = _Gpu(inp, precision, cuda)
    want = next(k for n, p, e, k in A_CONFIGS if (n, p, e) == (name, precision, E))
    assert g.plan["kernel"] == want, g.plan
    label = f"A {case}-{name}-{precision}-E{E}"
    src = dict(xT="inj", z="inj")
    if case == "env-offset48":
        src = dict(xT=None, z=None)
    elif case == "xT-injected":
        src = dict(z=None)
    elif case == "noise-injected":
        src = dict(xT=None)
    act, ch = g.sample(**src, **kw)
    _check(label, precision, _stats(act, ch, *ref), plan=g.plan)
    if case == "final-clip-off":      # 0.0 and -1.0 mean "no clip": the launch without one, bit for bit
        for fc in (0.0, -1.0):
            a2, c2 = g.sample(final_clip=fc)
            assert a2.tobytes() == act.tobytes() and c2.tobytes() == ch.tobytes(), fc
    if case in ("final-clip0.5", "eval-final-clip"):
        assert np.abs(act).max() <= 0.5 and np.abs(ch[:, -1]).max() <= 0.5 and np.abs(ch[:, :-1]).max() > 0.5
        assert np.array_equal(act, ch[:, -1])
    if case == "no-chains":
        a2, c2 = g.sample(want_chains=False)
        assert c2 is None and a2.tobytes() == act.tobytes()
    if case == "env-offset48":
        # shards: rows [16, E + 16) of an env_offset = 0 launch over E + 16 envs are an env_offset = 16 launch of E
        big = np.random.default_rng(5).uniform(-1, 1, (E + 16,) + inp.state.shape[1:]).astype(np.float32)
        from diffusionpolicyoptimization_amd import ops
        assert ops.sampler_plan(g.d, precision, E + 16)["kernel"] == want
        a0, c0 = g.sample(xT=None, z=None, state=big, E=E + 16)
        a1, c1 = g.sample(xT=None, z=None, state=big[16:], env_offset=16)
        equal = a0[16:].tobytes() == a1.tobytes() and c0[16:].tobytes() == c1.tobytes()
        _check(label + " shard", precision, _stats(a1, c1, a0[16:], c0[16:]), bit_equal=equal)


# ------------------------------------------------------------------------------------------------
# B. geometry: the accept / reject table
# ------------------------------------------------------------------------------------------------
def _ksteps(width, precision):
    """packed_ksteps (csrc/dppo_layout.h): k-steps of a layer of `width` inputs, rounded up to even."""
    kg = 16 if precision == "fp32" else 32
    return ((width + kg - 1) // kg + 1) & ~1


def _a16(n):
    return (n + 15) // 16 * 16


def _stream_lds(d, precision):
    """STREAM_LDS_REGIONS (csrc/dppo_sampler.h) summed as stream_lds_total does."""
    two = precision != "fp32"
    esz, kg = (2, 32) if two else (4, 16)
    pad, H, K, xd, sd = 32 // esz, d.actor_hidden, d.denoising_steps, d.xd, d.sd
    sw = 8 if two and H == 512 else 16
    noc = 16 * ((xd + 15) // 16)
    lda0 = _ksteps(d.actor_in, precision) * kg + pad
    return (2 * _a16(esz * 16 * (H + pad)) + _a16(esz * 16 * lda0) + _a16(64 * xd) + _a16(64 * sd) + _a16(4 * K * d.time_dim)
            + _a16(4 * sw * 16 * noc) + _a16(32 * K) + _a16(8 * (3 * H + noc)) + _a16(64 * K * xd))


def _split_lds(d, precision):
    """SPLIT_LDS_REGIONS summed as split_lds_total does (H = 512)."""
    f32 = precision == "fp32"
    esz, kg, sw = (4, 16, 4) if f32 else (2, 32, 8)
    K, xd, sd = d.denoising_steps, d.xd, d.sd
    kx = (xd + sd + kg - 1) // kg
    tring = kx == 2 or f32
    nb = 512 + 16 * ((xd + 15) // 16)
    return (_a16(esz * 16 * (kx * kg + 16)) + _a16(esz * 16 * 528) + _a16(4 * sw * 16 * xd) + 16 + _a16(64 * xd) + _a16(64 * sd)
            + _a16(4 * (2 if tring else K) * 512) + _a16(32 * K) + _a16(8 * nb) + _a16(64 * K * xd) + sw * (32 // sw) * kx * 1024)


def _msg_inst(d, precision):
    return (f"sampler: hidden {d.actor_hidden} / action chunk {d.xd} / in-layer k-steps {_ksteps(d.actor_in, precision)} "
            "not instantiated")


def _msg_lds(d, precision):
    return f"sampler needs {_stream_lds(d, precision)} B of LDS"


def _msg_layout(d, precision):
    return f"sampler: hidden {d.actor_hidden} not supported at this precision"


SPLIT, STREAM = "split", "stream"
K10 = dict(ft_denoising_steps=10)
# name -> (dims, E, fp32: SPLIT | STREAM | the rejection's message, 2-byte: the same, what it reaches)
GEOMETRIES = {
    "narrow": (NARROW, 17, STREAM, SPLIT, "XD 8: the split kernel's XQ = 2 form; half an out tile in the streaming kernel"),
    "xd3": (dict(HOPPER, action_dim=1, horizon_steps=3), 17, _msg_inst, STREAM,
            "XD not a multiple of 4: the draw loops' partial group of 4; fp32 has 30 inputs, 2 k-steps"),
    "h8a3": (dict(HOPPER, horizon_steps=8), 17, STREAM, SPLIT, "XD 24: two out tiles, the second half empty"),
    "h8a4": (dict(HOPPER, horizon_steps=8, action_dim=4), 17, STREAM, SPLIT, "XD 32: two full out tiles, the bound"),
    "h8a4-e513": (dict(HOPPER, horizon_steps=8, action_dim=4), 513, STREAM, STREAM,
                  "2-byte streaming at 16 XD = 512 = the block: no thread is spare for the time embedding"),
    "td8": (dict(HOPPER, time_dim=8), 17, SPLIT, SPLIT, "time_dim 8: fp32 has 31 inputs and runs through the split kernel"),
    "td32": (dict(HOPPER, time_dim=32), 17, SPLIT, SPLIT, "time_dim 32 in the packed TIN table"),
    "narrow-td32": (dict(NARROW, time_dim=32), 17, STREAM, SPLIT, "time_dim 32 in the streaming kernel's a0 (51 inputs)"),
    "cond2-hopper": (dict(HOPPER, cond_steps=2), 17, STREAM, SPLIT, "SD 22: the split kernel's second in-Dense k-step at XD 12"),
    "cond2-walker": (dict(WALKER, cond_steps=2), 17, _msg_inst, SPLIT, "SD 34, XD + SD = 58: the split kernel's widest in-Dense"),
    "cond2-walker-e513": (dict(WALKER, cond_steps=2), 513, _msg_inst, STREAM, "74 inputs: the 2-byte streaming k = 4 cases"),
    "tiny": (dict(HOPPER, obs_dim=3, action_dim=1), 17, _msg_inst, SPLIT, "23 inputs; XD 4: the split kernel's XQ = 1 form"),
    "obs3": (dict(HOPPER, obs_dim=3), 17, SPLIT, SPLIT, "31 inputs: fp32 through the split kernel's one-k-step form"),
    "ah256": (dict(HOPPER, actor_hidden=256), 17, STREAM, _msg_inst, "fp32 H = 256: DPPO_SAMPLE_CASE(1, 1, 4)"),
    "ah256-walker": (dict(WALKER, actor_hidden=256), 17, STREAM, _msg_inst, "fp32 H = 256, two out tiles: DPPO_SAMPLE_CASE(1, 2, 4)"),
    "ah128": (dict(HOPPER, actor_hidden=128), 17, _msg_inst, _msg_inst, ""),
    "ah384": (dict(HOPPER, actor_hidden=384), 17, _msg_layout, _msg_inst, ""),
    "k62": (dict(HOPPER, denoising_steps=62, **K10), 17, STREAM, STREAM, "K 62 at hopper's width: the split kernel's LDS is over"),
    "k62-cond2": (dict(HOPPER, denoising_steps=62, cond_steps=2, **K10), 17, STREAM, SPLIT, "the split kernel's last K, 2-byte"),
    "k62-obs3": (dict(HOPPER, denoising_steps=62, obs_dim=3, **K10), 17, SPLIT, STREAM, "the split kernel's last K, fp32"),
    "k63": (dict(HOPPER, denoising_steps=63, **K10), 17, STREAM, STREAM, "the first K that streams whatever the width"),
    "k100-h8a4": (dict(HOPPER, denoising_steps=100, horizon_steps=8, action_dim=4, **K10), 17, _msg_lds, _msg_lds, ""),
    "in128": (dict(HOPPER, time_dim=32, obs_dim=32, cond_steps=2, horizon_steps=8, action_dim=4), 17, _msg_inst, STREAM,
              "128 inputs: the widest 2-byte in-layer (k = 4), again at 16 XD = the block"),
}
B_PARAMS = [(g, p) for g in GEOMETRIES for p in PRECISIONS]
B_IDS = ["-".join(x) for x in B_PARAMS]


def expected(geometry, precision):
    """(dims, E, SPLIT | STREAM | None, the rejection's message | None)."""
    dims, E, f32, two, _ = GEOMETRIES[geometry]
    e = f32 if precision == "fp32" else two
    if callable(e):
        return dims, E, None, e(_dims(dims), precision)
    return dims, E, e, None


def test_geometry_table_matches_host_arithmetic():
    """The table against the layout's k-steps, the two LDS sums and ops.sampler_plan (host arithmetic;
    no launch): the docstring's four rules decide every row."""
    from diffusionpolicyoptimization_amd import ops
    for name, precision in B_PARAMS:
        dims, E, kernel, msg = expected(name, precision)
        d = _dims(dims)
        f32 = precision == "fp32"
        ks, H, K, G = _ksteps(d.actor_in, precision), d.actor_hidden, d.denoising_steps, (E + 15) // 16
        if f32:
            split = H == 512 and d.xd == 12 and d.xd + d.sd <= 32 and K <= 62 and G <= 32
            stream = H in (256, 512) and ks == 4
        else:
            split = H == 512 and d.xd % 4 == 0 and d.xd + d.sd <= 64 and K <= 62 and G <= 32
            stream = H == 512 and ks in (2, 4)
        split = split and _split_lds(d, precision) <= 160 * 1024
        stream = stream and _stream_lds(d, precision) <= 160 * 1024
        want = SPLIT if split else STREAM if stream else None
        assert kernel == want, (name, precision, kernel, want, ks)
        assert (ops.sampler_plan(d, precision, E)["kernel"] == 2) == split, (name, precision)
        if msg and "LDS" in msg:
            assert _stream_lds(d, precision) > 160 * 1024
    assert _ksteps(30, "fp32") == 2 and _ksteps(74, "fp32") == 6 and _ksteps(74, "bf16") == 4 and _ksteps(160, "bf16") == 6
    # K = 62 at hopper's width: both precisions miss the split kernel by its LDS alone
    for precision in ("fp32", "bf16"):
        d = _dims(GEOMETRIES["k62"][0])
        assert _split_lds(d, precision) > 160 * 1024 >= _split_lds(_dims(dict(GEOMETRIES["k62"][0], denoising_steps=20)), precision)
    assert abs(_c1(20) - 406) < 1 and _c1(62) > _c1(20)


@functools.lru_cache(maxsize=2)
def _b_inputs(geometry):
    dims, E = GEOMETRIES[geometry][:2]
    return _Inputs(dims, E, seed=11)


def _rejected(call, outputs, msg):
    """call() raises the library's unsupported-configuration error (code 3) with the dispatch's message
    and leaves the sentinel-filled outputs untouched."""
    import torch
    from diffusionpolicyoptimization_amd._lib import DppoError
    with pytest.raises(DppoError, match=re.escape(f"failed (3): {msg}")):
        call()
    torch.cuda.synchronize()
    for o in outputs:
        assert bool((o == SENTINEL).all()), "a rejected call wrote its outputs"


def _hopper_after(cuda, precision):
    """An accepted dppo_sample on the same stream after a refusal: matches the oracle."""
    inp = _Inputs(HOPPER, 17, seed=11)
    g = _Gpu(inp, precision, cuda)
    act, ch = g.sample()
    _check(f"B after a refusal-{precision}", precision, _stats(act, ch, *inp.oracle(precision)))


@gpu
@pytest.mark.parametrize("geometry,precision", B_PARAMS, ids=B_IDS)
def test_geometry(cuda, geometry, precision):
    """dppo_sample at one geometry of GEOMETRIES on the kernel the table names (asserted on the plan)
    against the oracle, actions and every chain row, at the existing bound (times c1(K) / c1(20) for
    K != 20) — or, where the table says REJECTED, the unsupported-configuration error with the
    dispatch's message, untouched outputs and a following accepted launch that matches the oracle."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    dims, E, kernel, msg = expected(geometry, precision)
    inp = _b_inputs(geometry)
    d = inp.d
    if msg:
        g = _Gpu(inp, precision, cuda)
        actions = torch.full((E, d.xd), SENTINEL, device=cuda)
        chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SENTINEL, device=cuda)
        call = lambda: ops.sample(d, precision, g.packb, g.packf, g.tab, g.T(inp.state.reshape(E, -1)),
                                  x_T=g.T(inp.xT.reshape(E, -1)), noise=g.T(inp.z.reshape(inp.K, E, -1)),
                                  actions=actions, chains=chains)
        _rejected(call, (actions, chains), msg)
        return _hopper_after(cuda, precision)
    g = _Gpu(inp, precision, cuda)
    assert g.plan["kernel"] == (2 if kernel == SPLIT else 0), (g.plan, kernel)
    act, ch = g.sample()
    scale = _k_scale(dims)
    _check(f"B {geometry}-{precision}", precision, _stats(act, ch, *inp.oracle(precision)), scale=scale, plan=g.plan,
           k_scale=scale)


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_in160_has_no_image(cuda, precision):
    """time_dim 64 with SD 64 and XD 32 (160 inputs, 6 in-layer k-steps in 2-byte) passes validate_dims,
    but dppo_pack_actor refuses time_dim > 32 (the row-tile fold), so no image reaches dppo_sample: the
    sampler's widest in-layer is in128's."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd._lib import DppoError
    dims = dict(HOPPER, time_dim=64, obs_dim=32, cond_steps=2, horizon_steps=8, action_dim=4)
    d = _dims(dims)
    assert d.actor_in == 160 and _ksteps(160, "bf16") == 6
    flat = torch.tensor(ops.flatten_params(ops.actor_param_spec(d), make_models(0, dims)[0]), device=cuda)
    with pytest.raises(DppoError, match=re.escape("failed (3): row-tile fold: time_dim 64 > 32")):
        ops.pack_actor(d, flat, precision)


STEP_GEOMETRIES = ["ah128", "ah384", "ah256", "tiny", "k100-h8a4", "in128", "obs3", "narrow"]
STEP_PARAMS = [(g, p, m) for g in STEP_GEOMETRIES for p in ("fp32", "bf16") for m in ("mapped", "unmapped")]


@gpu
@pytest.mark.parametrize("geometry,precision,memory", STEP_PARAMS, ids=["-".join(x) for x in STEP_PARAMS])
def test_sample_step_geometry(cuda, geometry, precision, memory):
    """dppo_sample_step (the rollout's one-call step) at accepted and refused geometries, through its
    mapped path (the kernel reads the observation from mapped host memory) and its unmapped fallback
    (copies around dppo_sample). A refusal comes before the observation's copy is enqueued: the device
    copy of cond, actions, the host actions and chains keep their sentinel. An accepted step equals
    dppo_sample with the same Philox stream bit for bit and matches the oracle."""
    import ctypes
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import ptr, stream_handle
    dims, E, kernel, msg = expected(geometry, precision)
    inp = _b_inputs(geometry)
    d = inp.d
    g = _Gpu(inp, precision, cuda)
    if memory == "mapped":
        mc, ma = ops.MappedArray((E, d.sd), np.float32), ops.MappedArray((E, d.xd), np.float32)
        cond_host, act_host = mc.tensor, ma.tensor
    else:
        cond_host, act_host = torch.empty(E, d.sd), torch.empty(E, d.xd)   # pageable: no device view of it
    cond_host.copy_(torch.from_numpy(inp.state.reshape(E, -1)))
    act_host.fill_(SENTINEL)
    cond = torch.full((E, d.sd), SENTINEL, device=cuda)
    actions = torch.full((E, d.xd), SENTINEL, device=cuda)
    chains = torch.full((E, d.ft_denoising_steps + 1, d.xd), SENTINEL, device=cuda)
    host_ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda: _lib.call("dppo_sample_step", ctypes.byref(d.c()), _lib.PRECISION[precision], ptr(g.packb), ptr(g.packf),
                             ptr(g.tab), host_ptr(cond_host), ptr(cond), E, ctypes.c_uint64(SEED), ctypes.c_uint64(CALL), 0,
                             0, 0.1, 3.0, 0.0, ptr(actions), host_ptr(act_host), ptr(chains), 1, stream_handle(cuda))
    if msg:
        _rejected(call, (cond, actions, chains, act_host), msg)
        return _hopper_after(cuda, precision)
    call()
    torch.cuda.synchronize()
    a_ref, c_ref = g.sample(xT=None, z=None)
    sh = a_ref.shape
    assert np.array_equal(cond.cpu().numpy(), inp.state.reshape(E, -1))
    assert actions.cpu().numpy().tobytes() == a_ref.tobytes() and chains.cpu().numpy().tobytes() == c_ref.tobytes()
    assert act_host.numpy().tobytes() == a_ref.tobytes()
    _check(f"B step {geometry}-{precision}-{memory}", precision,
           _stats(actions.cpu().numpy().reshape(sh), chains.cpu().numpy().reshape(c_ref.shape), *inp.oracle(precision, *inp.philox())))


# ------------------------------------------------------------------------------------------------
# C. kernel paths the plan chooses
# ------------------------------------------------------------------------------------------------
C_SPLIT = [(130, 10, 1), (130, 1, 1), (130, 19, 1), (512, 10, 1), (512, 1, 1), (512, 19, 1), (128, 10, 2)]


@gpu
@pytest.mark.parametrize("E,kf,sets", C_SPLIT, ids=[f"E{e}-kf{k}" for e, k, _ in C_SPLIT])
def test_fp32_split_member_sets(cuda, E, kf, sets):
    """fp32 hopper on the split kernel: 9 and 32 groups run one member set that switches actors
    mid-launch (the resident-fragment reload, at K' = 10, one step before the end and one after the
    start), 8 groups run two sets. Twice on the same inputs, bit-identical."""
    dims = dict(HOPPER, ft_denoising_steps=kf)
    inp = _Inputs(dims, E, seed=1000 * kf + E)
    g = _Gpu(inp, "fp32", cuda)
    assert g.plan["kernel"] == 2 and g.plan["members"] == 8 and g.plan["sets"] == sets, g.plan
    act, ch = g.twice()
    _check(f"C fp32-split-E{E}-kf{kf}", "fp32", _stats(act, ch, *inp.oracle("fp32")), plan=g.plan)


C_STREAM = [("hopper", "bf16", 513), ("hopper", "fp16", 513), ("walker", "fp32", 37)]


@gpu
@pytest.mark.parametrize("kf", [20, 1])
@pytest.mark.parametrize("name,precision,E", C_STREAM, ids=[f"{n}-{p}-E{e}" for n, p, e in C_STREAM])
def test_streaming_kf_edges(cuda, name, precision, E, kf):
    """The streaming kernel at K' = K (chain row 0 = x_T from the draw loop, no actor switch) and
    K' = 1 (the resident set reloaded before the last step): every stored chain row, row 0 bit-equal
    to x_T at K' = K. Twice on the same inputs, bit-identical."""
    dims = dict(A_DIMS[name], ft_denoising_steps=kf)
    inp = _Inputs(dims, E, seed=1000 * kf + E)
    g = _Gpu(inp, precision, cuda)
    assert g.plan["kernel"] == 0, g.plan
    act, ch = g.twice()
    assert ch.shape[1] == kf + 1
    if kf == 20:
        assert ch[:, 0].tobytes() == inp.xT.tobytes()
    _check(f"C stream-{name}-{precision}-E{E}-kf{kf}", precision, _stats(act, ch, *inp.oracle(precision)), plan=g.plan)


@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_ddim_eval_two_byte(cuda, precision):
    """Deterministic DDIM (eta = 0, eval_zero on every row: no row gets noise) on the 2-byte split kernel."""
    inp = _Inputs(HOPPER_DDIM, 37, seed=21, eta=0.0)
    g = _Gpu(inp, precision, cuda)
    assert g.plan["kernel"] == 2, g.plan
    ref = inp.oracle(precision, deterministic=True)
    assert np.array_equal(ref[0], inp.oracle(precision, z=np.zeros_like(inp.z), deterministic=True)[0])
    _assert_moved(f"ddim-eval-{precision}", precision, ref, inp.oracle(precision))
    act, ch = g.twice(deterministic=True)
    _check(f"C ddim-eval-{precision}", precision, _stats(act, ch, *ref), plan=g.plan)


@gpu
def test_ddim_final_clip_fp32(cuda):
    """DDIM (eta = 1) with final_clip = 0.5, fp32."""
    inp = _Inputs(HOPPER_DDIM, 37, seed=21)
    g = _Gpu(inp, "fp32", cuda)
    ref = inp.oracle("fp32", final_clip=0.5)
    _assert_moved("ddim-final-clip", "fp32", ref, inp.oracle("fp32"))
    act, ch = g.twice(final_clip=0.5)
    assert np.abs(act).max() <= 0.5
    _check("C ddim-final-clip-fp32", "fp32", _stats(act, ch, *ref), plan=g.plan)
