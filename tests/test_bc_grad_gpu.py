"""dppo_bc_minibatch (the behaviour-cloning term of the PPO loss and its actor gradient) on the GPU, against
tests/bc_cases.py: every gradient tensor and the metric slot over the row counts, precisions, activations, heads
and schedule records of bc_cases.CASES; the accumulate and overwrite forms; a data-parallel shard; every refusal;
PPODiffusion.c_loss(use_bc_loss=True) and the agent from cfg ft_ppo_diffusion_mlp_bc.

Bounds: per gradient tensor those of the minibatch-gradient cases (fp32 2e-3, 2-byte 1e-2, max |d| / max |ref|);
the metric slot test_bc_loss_matches_oracle's tolerance on the mean times the element count. Every figure is
printed as a JSON line before it is asserted."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import bc_cases as B
from tests.helpers import HOPPER, make_models, to_f64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEFF = 0.1
SENTINEL = -7.25
SLOT = 9


class _Gpu:
    """A bc_cases.Case on the device: the packed actor_ft image, the schedule table (with the case's record) and
    the inputs; run() launches ops.bc_minibatch into sentinel-filled outputs with a tail of 64 beyond the actor."""

    def __init__(self, case, precision, cuda):
        import torch
        from diffusionpolicyoptimization_amd import ops
        from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddim_buffers, ddpm_buffers
        self.case, self.precision, self.dev = case, precision, cuda
        self.d = d = ops.ModelDims(**case.dims)
        K = d.denoising_steps
        buf = ddim_buffers(K * d.time_stride, K, 1.0) if d.time_stride > 1 else ddpm_buffers(K)
        pe = case.sched_kw.get("predict_epsilon", True)
        self.tab = torch.tensor(ops.sched_table(buf, predict_epsilon=pe), device=cuda)
        if case.sched_kw:
            ops.sched_set_params(self.tab, denoised_clip_value=case.sched_kw.get("denoised_clip", 1.0), predict_epsilon=pe)
        self.spec = ops.actor_param_spec(d)
        self.na = ops.spec_count(ops.actor_param_spec(ops.ModelDims(**dict(case.dims, head="residual"))))
        self.pf = torch.tensor(ops.flatten_params(self.spec, case.ft), device=cuda)
        assert self.pf.numel() == self.na
        self.packed = ops.pack_actor(d, self.pf, precision)
        self.cond = torch.tensor(case.state.reshape(case.n, -1).astype(np.float32), device=cuda)
        self.chains = torch.tensor(case.chains.reshape(case.n, case.kf + 1, -1).astype(np.float32), device=cuda)

    def outputs(self):
        import torch
        grads = torch.full((self.na + 64,), SENTINEL, dtype=torch.float32, device=self.dev)
        metrics = torch.full((16,), SENTINEL, dtype=torch.float64, device=self.dev)
        return grads, metrics

    def workspace(self, rows, fill=0xFF):
        import torch
        from diffusionpolicyoptimization_amd import ops
        ws = ops.ppo_workspace(self.d, self.precision, rows, self.dev)
        ws.fill_(fill)
        return ws

    def run(self, grads, metrics, ws=None, sl=slice(None), **kw):
        import torch
        from diffusionpolicyoptimization_amd import ops
        cond, chains = self.cond[sl].contiguous(), self.chains[sl].contiguous()
        ws = self.workspace(cond.shape[0] * self.case.kf) if ws is None else ws
        kw.setdefault("min_logprob_std", self.case.min_logprob_std)
        ops.bc_minibatch(self.d, self.precision, self.packed, self.pf, self.tab, cond, chains, ws, grads, metrics,
                         COEFF, **kw)
        torch.cuda.synchronize()
        return grads.cpu().numpy(), metrics.cpu().numpy()

    def tensors(self, g):
        from diffusionpolicyoptimization_amd import ops
        return ops.unflatten_params(self.spec, g[:self.na])


def _check(label, gpu, g, m, ref, precision, elements, scale=1.0):
    """Every gradient tensor of the oracle (times scale) and the metric slot; the tail of grads and every other
    slot still hold the sentinel."""
    got = gpu.tensors(g)
    errs = {k: B.rel(got[k], r * scale) for k, r in ref["grads"].items()}
    mtol = B.BC_TOL[precision] * max(1.0, abs(ref["clip_sum"]) / elements) * elements
    print(json.dumps({"case": label, "precision": precision, "max_err": max(errs.values()), "errs": errs,
                      "bound": B.GRAD_TOL[precision], "clip_sum": (float(m[SLOT]), ref["clip_sum"]), "clip_sum_bound": mtol}))
    assert np.isfinite(g[:gpu.na]).all()
    bad = {k: v for k, v in errs.items() if not v < B.GRAD_TOL[precision]}
    assert not bad, (label, bad)
    assert abs(m[SLOT] - ref["clip_sum"]) <= mtol, (label, m[SLOT], ref["clip_sum"])
    assert (g[gpu.na:] == SENTINEL).all() and (np.delete(m, SLOT) == SENTINEL).all(), label


def _l2_offset(d):
    """Offset of l2_w in the flat actor layout (the residual spec of the same dims)."""
    import dataclasses
    from diffusionpolicyoptimization_amd import ops
    o = 0
    for n_, s in ops.actor_param_spec(dataclasses.replace(d, head="residual")):
        if n_ == "l2_w":
            return o
        o += int(np.prod(s))


GRID = [(lab, p) for lab, (_, _, precs, _) in B.CASES.items() for p in precs if lab != "tile64"]


@pytest.mark.parametrize("label,precision", GRID, ids=[f"{a}-{b}" for a, b in GRID])
def test_bc_minibatch_matches_oracle(cuda, label, precision):
    """dppo_bc_minibatch without DPPO_BC_ACCUMULATE over a 0xFF workspace into sentinel-filled outputs."""
    from diffusionpolicyoptimization_amd import ops
    case = B.build(label)
    gpu = _Gpu(case, precision, cuda)
    rows = case.n * case.kf
    plan = ops.ppo_plan(gpu.d, precision, rows)
    assert plan["actor_tile_rows"] == 32, plan
    g, m = gpu.run(*gpu.outputs())
    _check(label, gpu, g, m, case.oracle(COEFF, precision), precision, rows * gpu.d.xd)
    if case.dims.get("head") == "plain":   # no l2 layer: its range keeps the zeroing's zeros
        lo, H = _l2_offset(gpu.d), gpu.d.actor_hidden
        assert not g[lo:lo + H * H + H].any()


def test_bc_minibatch_64_row_tile(cuda):
    """The smallest row count ops.ppo_plan reports for the 64-row tile on this device (64 x CU count rows), bf16."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    d = ops.ModelDims(**HOPPER)
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    rows = 64 * cus
    n = -(-rows // d.ft_denoising_steps)
    assert ops.ppo_plan(d, "bf16", n * d.ft_denoising_steps)["actor_tile_rows"] == 64
    assert ops.ppo_plan(d, "bf16", (cus - 1) * 64)["actor_tile_rows"] == 32
    case = B.build("tile64", n=n)
    gpu = _Gpu(case, "bf16", cuda)
    g, m = gpu.run(*gpu.outputs())
    _check("tile64", gpu, g, m, case.oracle(COEFF, "bf16"), "bf16", n * case.kf * d.xd)


def _ppo_part1(gpu, rows, grads, metrics, l2_deferred=False):
    """dppo_ppo_minibatch_part(part = 1) on `rows` rows of a seeded rollout of 20 samples."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    d, dev = gpu.d, gpu.dev
    kf, N = d.ft_denoising_steps, 20
    rng = np.random.default_rng(31)
    T = lambda x: torch.tensor(np.asarray(x, np.float32), device=dev)
    obs, chains = T(rng.uniform(-1, 1, (N, d.sd))), T(rng.standard_normal((N, kf + 1, d.xd)) * 0.5)
    adv, ret = T(rng.normal(size=N)), T(rng.normal(size=N))
    _, lp_old = ops.logprob(d, gpu.precision, gpu.packed, gpu.tab, obs, chains)
    _, _, critic = make_models(0, HOPPER)
    pc = torch.tensor(ops.flatten_params(ops.critic_param_spec(d), critic), device=dev)
    stats = torch.zeros(3, dtype=torch.float64, device=dev)
    ops.ppo_adv_stats(adv, N * kf, kf, 5, 0, 0, rows, stats)
    hp = ops.ppo_hparams(global_rows=rows, l2_deferred=l2_deferred)
    ws = ops.ppo_workspace(d, gpu.precision, rows, dev)
    ops.ppo_minibatch(d, gpu.precision, hp, gpu.packed, ops.pack_critic(d, pc, gpu.precision), gpu.pf, gpu.tab, obs,
                      chains, lp_old.contiguous(), adv, ret, 5, 0, 0, rows, ws, grads, metrics, adv_stats=stats, part=1)
    torch.cuda.synchronize()


def test_accumulate_on_a_ppo_minibatch(cuda):
    """part 1 of a 77-row PPO minibatch, then the term with DPPO_BC_ACCUMULATE, against the two run apart and added
    on the host: per tensor 1e-6 relative l2 (the atomics reorder); the critic's range and metric slots 0..8 are
    bit-equal to the part alone."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    case = B.build("rows150")
    gpu = _Gpu(case, "fp32", cuda)
    nc = ops.spec_count(ops.critic_param_spec(gpu.d))
    mk = lambda: (torch.full((gpu.na + nc,), SENTINEL, dtype=torch.float32, device=cuda),
                  torch.full((16,), SENTINEL, dtype=torch.float64, device=cuda))
    g_ppo, m_ppo = mk()
    _ppo_part1(gpu, 77, g_ppo, m_ppo)
    g_both, m_both = mk()
    _ppo_part1(gpu, 77, g_both, m_both)
    gb, mb = gpu.run(g_both, m_both, accumulate=True)
    g_bc, m_bc = gpu.run(*gpu.outputs())
    gp, mp = g_ppo.cpu().numpy(), m_ppo.cpu().numpy()
    want = gpu.tensors(gp.astype(np.float64)[:gpu.na] + g_bc.astype(np.float64)[:gpu.na])
    errs = {k: B.rel_l2(v, want[k]) for k, v in gpu.tensors(gb).items()}
    print(json.dumps({"case": "accumulate-ppo", "errs": errs, "slot": (float(mb[SLOT]), float(m_bc[SLOT]))}))
    assert max(errs.values()) < 1e-6, errs
    assert np.array_equal(gb[gpu.na:], gp[gpu.na:]) and np.array_equal(mb[:9], mp[:9])
    assert mp[SLOT] == 0.0 and abs(mb[SLOT] - m_bc[SLOT]) <= 1e-6 * abs(m_bc[SLOT])
    assert np.array_equal(mb[10:], mp[10:])


def test_accumulate_chunks_and_l2_deferred(cuda):
    """Three accumulate calls of 5 samples on one workspace against one call of 15 (1e-6 relative l2 per tensor, the
    slot, whose fp32 row sums regroup with the tiles, to 1e-6 too), and DPPO_PPO_L2_DEFERRED followed by dppo_materialize_l2 against the unfactored call."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    case = B.build("rows150")
    gpu = _Gpu(case, "bf16", cuda)
    g1, m1 = gpu.run(*gpu.outputs())
    grads, metrics = gpu.outputs()
    ws = gpu.workspace(5 * case.kf)
    for a in range(0, 15, 5):
        gc, mc = gpu.run(grads, metrics, ws=ws, sl=slice(a, a + 5), accumulate=a > 0, global_samples=15)
    errs = {k: B.rel_l2(v, gpu.tensors(g1)[k]) for k, v in gpu.tensors(gc).items()}
    print(json.dumps({"case": "chunks", "errs": errs, "slot": (float(mc[SLOT]), float(m1[SLOT]))}))
    assert max(errs.values()) < 1e-6, errs
    assert abs(mc[SLOT] - m1[SLOT]) <= 1e-6 * abs(m1[SLOT]) and (gc[gpu.na:] == SENTINEL).all()
    grads, metrics = gpu.outputs()
    ws = gpu.workspace(15 * case.kf)
    gpu.run(grads, metrics, ws=ws, l2_deferred=True)
    H, xd = gpu.d.actor_hidden, gpu.d.xd
    off = _l2_offset(gpu.d)
    fact = grads.cpu().numpy()
    assert not fact[off + H * xd:off + H * H + H].any() and fact[off:off + H * xd].any()
    ops.materialize_l2(gpu.d, "bf16", gpu.packed, grads, ws, 15 * case.kf)
    torch.cuda.synchronize()
    gd = grads.cpu().numpy()
    errs = {k: B.rel_l2(v, gpu.tensors(g1)[k]) for k, v in gpu.tensors(gd).items()}
    print(json.dumps({"case": "l2-deferred", "errs": errs}))
    assert max(errs.values()) < 1e-6, errs


def test_overwrite_and_workspace_reuse(cuda):
    """Without DPPO_BC_ACCUMULATE the outputs are overwritten whatever they held, and a workspace that served a
    larger call (other row padding, stale images) gives the bits of a fresh one up to the atomics' order."""
    case = B.build("rows150")
    gpu = _Gpu(case, "fp32", cuda)
    ws = gpu.workspace(15 * case.kf, fill=0x7F)
    g_big, _ = gpu.run(*gpu.outputs(), ws=ws)
    g_small, m_small = gpu.run(*gpu.outputs(), ws=ws, sl=slice(0, 3))          # 30 rows in the 150-row workspace
    g_ref, m_ref = gpu.run(*gpu.outputs(), sl=slice(0, 3))
    errs = {k: B.rel_l2(v, gpu.tensors(g_ref)[k]) for k, v in gpu.tensors(g_small).items()}
    print(json.dumps({"case": "workspace-reuse", "errs": errs}))
    assert max(errs.values()) < 1e-6 and m_small[SLOT] == m_ref[SLOT]
    assert (g_small[gpu.na:] == SENTINEL).all() and (np.delete(m_small, SLOT) == SENTINEL).all()
    assert B.rel_l2(g_big[:gpu.na], g_small[:gpu.na]) > 0.1


@pytest.mark.parametrize("loss_scale", [0.25, 3.0])
def test_shard(cuda, loss_scale):
    """4 samples of 16 with global_samples = 16: the oracle with D = 16 and the loss scale."""
    case = B.build("rows40")
    for precision in ("fp32", "fp16"):
        gpu = _Gpu(case, precision, cuda)
        g, m = gpu.run(*gpu.outputs(), global_samples=16, loss_scale=loss_scale)
        _check(f"shard-{loss_scale}", gpu, g, m, case.oracle(COEFF, precision, denom=16, loss_scale=loss_scale), precision,
               40 * gpu.d.xd)


def test_refusals(cuda):
    """Every refusal of the header's table: DPPO_EINVAL with its message, nothing enqueued, outputs unchanged."""
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd._lib import DppoError, ptr
    case = B.build("rows40")
    gpu = _Gpu(case, "bf16", cuda)
    grads, metrics = gpu.outputs()
    ws = gpu.workspace(40)
    dims = gpu.d.c()

    def call(**over):
        a = dict(packed=ptr(gpu.packed), params=ptr(gpu.pf), sched=ptr(gpu.tab), cond=ptr(gpu.cond), chains=ptr(gpu.chains),
                 n=4, g=4, std=0.1, coeff=COEFF, ls=1.0, flags=0, ws=ptr(ws), grads=ptr(grads), metrics=ptr(metrics), d=dims)
        a.update(over)
        _lib.call("dppo_bc_minibatch", ctypes.byref(a["d"]), 1, a["packed"], a["params"], a["sched"], a["cond"], a["chains"],
                  a["n"], a["g"], a["std"], a["coeff"], a["ls"], a["flags"], a["ws"], a["grads"], a["metrics"],
                  _lib.stream_handle(cuda))

    cases = [(dict(n=0), 1, "dppo_bc_minibatch: n < 1"), (dict(n=-3), 1, "dppo_bc_minibatch: n < 1"),
             (dict(g=3), 1, "dppo_bc_minibatch: global_samples < n"),
             (dict(coeff=-0.1), 1, "dppo_bc_minibatch: coeff must be >= 0"),
             (dict(coeff=float("nan")), 1, "dppo_bc_minibatch: coeff must be >= 0"),
             (dict(flags=_lib.DPPO_PPO_LEARN_ETA), 1, "dppo_bc_minibatch: DPPO_PPO_LEARN_ETA is not supported"),
             (dict(flags=_lib.DPPO_PPO_ADV_CLIP), 1, "dppo_bc_minibatch: unknown flags 0x8"),
             (dict(flags=32 | _lib.DPPO_BC_ACCUMULATE), 1, "dppo_bc_minibatch: unknown flags 0x30")]
    cases += [({k: None}, 1, "dppo_bc_minibatch: null pointer")
              for k in ("packed", "params", "sched", "cond", "chains", "ws", "grads", "metrics")]
    # the TRAIN tile's own table: no instantiation for this hidden width; more than 64 fine-tuned steps
    cases.append((dict(d=ops.ModelDims(**dict(HOPPER, actor_hidden=384)).c()), 3, "actor: hidden 384"))
    cases.append((dict(d=ops.ModelDims(**dict(HOPPER, denoising_steps=80, ft_denoising_steps=65)).c()), 3,
                  "dppo_bc_minibatch: ft_denoising_steps 65 > 64 unsupported (bucket sums)"))
    for over, code, msg in cases:
        with pytest.raises(DppoError, match=re.escape(f"failed ({code}): {msg}")):
            call(**over)
        torch.cuda.synchronize()
        assert bool((grads == SENTINEL).all()) and bool((metrics == SENTINEL).all()), over
    # the 64-row tile's LDS line: K' = 24 at a minibatch of one round of 64-row tiles
    d24 = ops.ModelDims(**dict(HOPPER, denoising_steps=24, ft_denoising_steps=24))
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    n = -(-64 * cus // 24)
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    keep = (ops.pack_actor(d24, gpu.pf, "bf16"), torch.tensor(ops.sched_table(ddpm_buffers(24)), device=cuda),
            ops.ppo_workspace(d24, "bf16", n * 24, cuda), torch.zeros(n, d24.sd, device=cuda),
            torch.zeros(n, 25, d24.xd, device=cuda))
    big = dict(d=d24.c(), n=n, g=n, packed=ptr(keep[0]), sched=ptr(keep[1]), ws=ptr(keep[2]), cond=ptr(keep[3]),
               chains=ptr(keep[4]))
    with pytest.raises(DppoError, match=re.escape("failed (3): actor row tile needs")):
        call(**big)
    torch.cuda.synchronize()
    assert bool((grads == SENTINEL).all()) and bool((metrics == SENTINEL).all())
    call()   # and the accepted call still runs
    torch.cuda.synchronize()
    assert bool((grads[gpu.na:] == SENTINEL).all()) and float(metrics[SLOT]) != SENTINEL


def _model(cuda, precision="fp32", seed=3):
    from diffusionpolicyoptimization_amd.util.config import instantiate, load_config
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp_bc",
                      [f"model.precision={precision}"])
    return instantiate(cfg.model, device=cuda, seed=seed)


def test_c_loss_with_the_term(cuda):
    """PPODiffusion.c_loss(use_bc_loss=True) at bc_loss_coeff = 0.1 with injected draws: the tuple's bc_loss and
    self.grads against O.c_loss plus bc_cases' oracle on the chains the model drew (the base sampler is pinned by
    test_bc_loss_matches_oracle); at coefficient 0 the gradients are bit-equal to use_bc_loss=False and the
    default coefficient is 0."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    m = _model(cuda)
    assert m.bc_loss_coeff == 0.0
    d, kf, K = m.dims, m.ft_denoising_steps, m.dims.denoising_steps
    b = 24
    rng = np.random.default_rng(17)
    # actor_ft moved off the base so that the clip works
    with torch.no_grad():
        m.train_params[:m.n_actor] += torch.tensor(rng.normal(0, B.PERTURB, m.n_actor).astype(np.float32), device=cuda)
    m.repack()
    state = rng.uniform(-1, 1, (b, d.cond_steps, d.obs_dim)).astype(np.float32)
    xT = torch.tensor(rng.standard_normal((b, d.xd)).astype(np.float32), device=cuda)
    z = torch.tensor(rng.standard_normal((K, b, d.xd)).astype(np.float32), device=cuda)
    sh = (b, d.horizon_steps, d.action_dim)
    j = rng.integers(0, kf, b)
    prev, nxt = (rng.standard_normal(sh) * 0.5).astype(np.float32), (rng.standard_normal(sh) * 0.5).astype(np.float32)
    ret, adv = rng.normal(size=b).astype(np.float32), rng.normal(size=b).astype(np.float32)
    ft = to_f64(ops.unflatten_params(m.actor_spec, m.train_params.cpu().numpy()[:m.n_actor]))
    critic = to_f64(ops.unflatten_params(m.critic_spec, m.train_params.cpu().numpy()[m.n_actor:]))
    sched = O.ddpm_schedule(K)
    drawn = {}
    orig = m._bc_chains

    def inject(st, x_T=None, noise=None):
        drawn["chains"] = orig(st, xT, z)
        return drawn["chains"]
    args = (torch.tensor(state.reshape(b, -1), device=cuda), prev, nxt, j, ret, None, adv)

    def run(coeff, use):
        m.bc_loss_coeff = coeff
        old = _old_logprobs(m, ft, sched, state, prev, nxt, j, kf)
        out = m.c_loss(*args, old, use_bc_loss=use)
        torch.cuda.synchronize()
        return out, m.grads.cpu().numpy().copy()
    m._bc_chains = inject
    out, g = run(COEFF, True)
    ch = drawn["chains"].cpu().numpy().astype(np.float64).reshape(b, kf + 1, d.horizon_steps, d.action_dim)
    _, ga, gc = O.c_loss(ft, critic, sched, state.astype(np.float64), prev.astype(np.float64), nxt.astype(np.float64), j,
                         ret.astype(np.float64), None, adv.astype(np.float64),
                         _old_logprobs(m, ft, sched, state, prev, nxt, j, kf).astype(np.float64), kf)
    ref = B.bc_oracle(ft, sched, state.astype(np.float64), ch, kf, COEFF, min_logprob_std=m.min_logprob_denoising_std)
    got = ops.unflatten_params(m.actor_spec, g[:m.n_actor])
    errs = {k: B.rel(got[k], ga[k] + ref["grads"][k]) for k in ga}
    share = {k: B.rel(ga[k] + ref["grads"][k], ga[k]) for k in ga}
    print(json.dumps({"case": "c_loss", "bc_loss": (out[6], ref["bc_loss"]), "errs": errs, "term_share": share}))
    assert max(errs.values()) < B.GRAD_TOL["fp32"], errs
    assert abs(out[6] - ref["bc_loss"]) <= B.BC_TOL["fp32"] * max(1.0, abs(ref["bc_loss"]))
    assert B.rel(g[m.n_actor:], ops.flatten_params(m.critic_spec, gc)) < B.GRAD_TOL["fp32"]
    assert min(share.values()) > 10 * B.GRAD_TOL["fp32"], share
    (out0, g0), (out_off, g_off) = run(0.0, True), run(0.0, False)
    assert np.array_equal(g0, g_off) and out0[:6] == out_off[:6] and out_off[6] == 0.0 and out0[6] != 0.0


def _old_logprobs(m, ft, sched, state, prev, nxt, j, kf):
    """The clipped row means of the new log-probs themselves (ratio 1), float32 [b]."""
    b = state.shape[0]
    t = kf - 1 - j
    eps, _ = O.diffusion_mlp_forward(ft, prev.astype(np.float64), t, state.astype(np.float64), round_h3=False)
    mu, logvar, _ = O.p_mean_var(sched, eps, prev.astype(np.float64), t)
    std = np.clip(np.exp(0.5 * logvar), m.min_logprob_denoising_std, 1e6)
    lp = O.gaussian_logprob(nxt.astype(np.float64), mu, std)
    return np.clip(lp, -5, 2).mean(axis=(1, 2)).astype(np.float32)


def _agent(tmp_path, *over, name="ft_ppo_diffusion_mlp_bc"):
    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), name,
                      ["train.n_steps=8", "train.batch_size=320", "train.update_epochs=2", f"logdir={tmp_path}",
                       "train.save_checkpoints=false", "train.save_results=false", *over])
    return get_class(cfg._target_)(cfg)


def test_bc_grad_chunks_and_default(cuda):
    """PPODiffusion.bc_grad over 23 observations: the default (ops.bc_chunk: one call here), chunk = 5 (five calls,
    the last of 3 samples) and chunk = 64 (one call in a larger workspace) draw the same chains (the call counter
    set back) and agree per tensor to 1e-6 relative l2, the slot too."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    m = _model(cuda, "bf16")
    rng = np.random.default_rng(2)
    with torch.no_grad():
        m.train_params[:m.n_actor] += torch.tensor(rng.normal(0, B.PERTURB, m.n_actor).astype(np.float32), device=cuda)
    m.repack()
    obs = torch.tensor(rng.uniform(-1, 1, (23, m.dims.sd)).astype(np.float32), device=cuda)
    assert ops.bc_chunk(m.dims, m.precision, 23) == 23
    res = {}
    for chunk in (None, 5, 64):
        m._bc_calls = 7
        loss = m.bc_grad(obs, COEFF, accumulate=False, chunk=chunk)
        torch.cuda.synchronize()
        assert m._bc_calls == 8
        res[chunk] = (ops.unflatten_params(m.actor_spec, m.grads.cpu().numpy()[:m.n_actor].copy()), float(m.metrics[SLOT]),
                      float(loss))
    errs = {str(c): max(B.rel_l2(v, res[None][0][k]) for k, v in res[c][0].items()) for c in (5, 64)}
    print(json.dumps({"case": "bc_grad-chunks", "errs": errs, "slot": [res[c][1] for c in res], "bc_loss": res[None][2]}))
    assert max(errs.values()) < 1e-6, errs
    for c in (5, 64):
        assert abs(res[c][1] - res[None][1]) <= 1e-6 * abs(res[None][1])
    assert abs(res[None][2] + res[None][1] / (23 * m.ft_denoising_steps * m.dims.xd)) <= 1e-9 * abs(res[None][2])


def test_coefficient_zero_makes_no_new_call(cuda, tmp_path, monkeypatch):
    """bc_loss_coeff = 0 with use_bc_loss on: two training iterations never reach dppo_bc_minibatch (a counting
    wrapper over the library's symbols, as the advantage clip's test), the update keeps the split path and the
    report still comes from _bc_loss_report; with the coefficient on the same wrapper counts the calls."""
    from diffusionpolicyoptimization_amd import _lib
    lib, calls = _lib.load(), []

    class Counting:
        def __getattr__(self, name):
            if name == "dppo_bc_minibatch":
                calls.append(name)
            return getattr(lib, name)
    off = _agent(tmp_path, "train.bc_loss_coeff=0")
    on = _agent(tmp_path)
    monkeypatch.setattr(_lib, "_lib", Counting())
    infos = [off.iteration(force_train=True) for _ in range(2)]
    assert off.timing["n_updates"] > 0 and calls == [] and not off.bc_in_loss and not hasattr(off, "_bc_sums")
    assert all(np.isfinite(i["bc_loss"]) and i["bc_loss"] != 0.0 for i in infos)
    on.iteration(force_train=True)
    assert len(calls) == on.timing["n_updates"] > 0


def test_agent_refusals(cuda, tmp_path):
    """The constructor's refusals: a negative coefficient, the coefficient without use_bc_loss, and with learn_eta."""
    for over, name, msg in ((["train.bc_loss_coeff=-0.5"], "ft_ppo_diffusion_mlp_bc", "bc_loss_coeff = -0.5 < 0"),
                            (["train.use_bc_loss=false"], "ft_ppo_diffusion_mlp_bc", "needs train.use_bc_loss"),
                            (["+train.use_bc_loss=true", "+train.bc_loss_coeff=0.1"], "ft_ppo_diffusion_mlp_ddim_learn_eta",
                             "learn_eta")):
        with pytest.raises(ValueError, match=msg):
            _agent(tmp_path, *over, name=name)


def test_agent_applies_the_term(cuda, tmp_path):
    """The agent from cfg ft_ppo_diffusion_mlp_bc, two iterations of 8 steps, one minibatch per epoch: the hooked
    gradients against the same model state's PPO minibatch plus bc_grad re-run with _bc_calls set back (1e-5
    relative l2 per tensor: which observations and which call id the agent uses); info["bc_loss"] is the slot's
    value; with bc_loss_coeff = 0 the term's path is never taken and the parameters agree with use_bc_loss = false to
    the run-to-run difference of the update's atomically ordered sums (below)."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    a = _agent(tmp_path)
    m = a.model
    kf, xd = m.ft_denoising_steps, m.dims.xd
    seen = []

    def hook(epoch, batch, start, rows):
        torch.cuda.synchronize()
        calls = m._bc_calls - 1
        got, slot = m.grads.clone(), float(m.metrics[9])
        total = a.n_steps * a.n_envs * kf
        key = epoch + 1000 * a.itr
        obs_flat = a.obs_traj.view(a.n_steps * a.n_envs, -1)
        adv_flat, ret_flat = a.adv.view(-1), a.ret.view(-1)
        chains_flat = a.chains_traj.view(a.n_steps * a.n_envs, kf + 1, -1)
        stats = torch.zeros(3, dtype=torch.float64, device=cuda)
        ops.ppo_adv_stats(adv_flat, total, kf, a.perm_seed, key, start, rows, stats)
        met = m.metrics.clone()
        m.minibatch(obs_flat, chains_flat, a.lp_old, adv_flat, ret_flat, a.perm_seed, key, start, rows,
                    reward_horizon=a.reward_horizon, adv_stats=stats, old_values=a.values)
        idx = ops.feistel_permute(start, rows, total, a.perm_seed, key, cuda)
        m._bc_calls = calls
        m.bc_grad(obs_flat[idx // kf], a.bc_loss_coeff, accumulate=True)
        torch.cuda.synchronize()
        want = m.grads.cpu().numpy().astype(np.float64)
        na = m.n_actor
        errs = {k: B.rel_l2(v, ops.unflatten_params(m.actor_spec, want[:na])[k])
                for k, v in ops.unflatten_params(m.actor_spec, got.cpu().numpy()[:na]).items()}
        seen.append(dict(errs=errs, slot=slot, slot_again=float(m.metrics[9]), rows=rows,
                         critic=B.rel_l2(got.cpu().numpy()[na:], want[na:])))
        m.grads.copy_(got)
        m.metrics.copy_(met)
    a.minibatch_hook = hook
    infos = [a.iteration(force_train=True) for _ in range(2)]
    print(json.dumps({"case": "agent", "seen": seen, "bc_loss": [i["bc_loss"] for i in infos]}))
    assert len(seen) == 4
    for s in seen:
        assert max(s["errs"].values()) < 1e-5 and s["critic"] < 1e-5, s
        assert abs(s["slot"] - s["slot_again"]) <= 1e-6 * abs(s["slot"])
    for info, s in zip(infos, (seen[1], seen[3])):
        assert abs(info["bc_loss"] - (-s["slot"] / (s["rows"] * kf * xd))) <= 1e-9 * abs(info["bc_loss"]), (info["bc_loss"], s)
    def ran(*over):   # one agent at a time: built, run for two iterations, then the next
        ag = _agent(tmp_path, "train.bc_loss_coeff=0", *over)
        for _ in range(2):
            ag.iteration(force_train=True)
        return ag
    ref = ran("train.use_bc_loss=false")
    off = ran()
    # Bit-equality is not a property two runs of ONE cfg have: the critic's distinct-sample list is in arrival order and
    # the weight-gradient launches add partial tiles with atomics, so fp32 sums accumulate in a run-dependent order
    # (csrc/update.hip, crit_rows_kernel). Two runs of the use_bc_loss=false cfg measured 7.5e-9 apart. Each of the
    # 4 AdamW steps moves a parameter by about lr at most, and a reordered fp32 sum moves a gradient by far less than
    # 1e-3 of itself: 4 lr 1e-3 bounds the difference; the term itself moves the actor by over a hundred times that.
    na = ref.model.n_actor
    diff = lambda x, y: float((x.model.train_params - y.model.train_params).abs().max())
    d_off, d_on = diff(off, ref), float((a.model.train_params[:na] - ref.model.train_params[:na]).abs().max())
    bound = 4 * float(ref.cfg.train.actor_lr) * 1e-3
    print(json.dumps({"case": "agent-off", "off_vs_ref": d_off, "on_vs_ref_actor": d_on, "bound": bound}))
    assert d_off <= bound and d_on > 100 * bound, (d_off, d_on, bound)
    assert not off.bc_in_loss and not hasattr(off, "_bc_sums")   # the term's path was never taken
