"""The pretraining step against the float64 oracle: dppo_pretrain_minibatch (csrc/update.hip; the `pre` prologue
and epilogue of the actor row tile, the dW launch, seg_reduce_kernel, the time-MLP backward) at its edges, and
TrainDiffusionAgent's loop teacher-forced step by step. Cases, inputs and references are in
tests/pretrain_cases.py; tests/test_pretrain_step_cpu.py shows that the inputs are what the cases say and that
each check can fail.

Error measure, per gradient tensor: max |g - ref| / (max |ref| + 1e-12); the loss relative to the oracle's.
Bounds: fp32 2e-3; bf16 and fp16 1e-2 against the oracle rounding at the kernels' rounding points. Every case
prints one JSON line with its figures before it asserts them."""
import json
import os
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import pretrain_cases as C
from tests.helpers import HOPPER_DDIM, adamw_oracle, step_ratios, to_f64
from tests.test_kernels_gpu import _rnd, _setup
from tests.test_update_surface_gpu import SENTINEL, _rejected

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1      # what a DPPO_CHECK returns (include/dppo.h DPPO_EINVAL); the dispatch's refusals are 3

_PROBLEMS = {}


class _Problem:
    """one geometry's device-side constants: dims, parameters, tables and (per precision) the packed image"""

    def __init__(self, cuda, dims):
        import torch
        from diffusionpolicyoptimization_amd import ops
        self.cuda = cuda
        self.d, _, ft, _, self.sched, self.tab, _, self.pf, _ = _setup(dims, cuda)
        self.ft = to_f64(ft)
        self.dims = dims
        self.spec = ops.actor_param_spec(self.d)
        self.na = ops.spec_count(self.spec)
        self._packed = {}
        if self.d.time_stride == 1:
            self.qs = torch.tensor(ops.q_sched_table(self.sched), device=cuda)

    def packed(self, precision):
        from diffusionpolicyoptimization_amd import ops
        if precision not in self._packed:
            self._packed[precision] = ops.pack_actor(self.d, self.pf, precision)
        return self._packed[precision]


def _problem(cuda, K=20):
    if K not in _PROBLEMS:
        _PROBLEMS[K] = _Problem(cuda, C.dims_of(K))
    return _PROBLEMS[K]


def _launch(p, precision, inp, global_rows=None, loss_scale=1.0, ws=None, grads=None, metrics=None):
    """one dppo_pretrain_minibatch on the current stream -> (loss as a device scalar, grads, metrics)"""
    import torch
    from diffusionpolicyoptimization_amd import ops
    T = lambda x: torch.tensor(x, device=p.cuda)
    rows = inp["x0"].shape[0]
    ws = ops.ppo_workspace(p.d, precision, rows, p.cuda) if ws is None else ws
    grads = torch.zeros(p.na, dtype=torch.float32, device=p.cuda) if grads is None else grads
    metrics = torch.zeros(16, dtype=torch.float64, device=p.cuda) if metrics is None else metrics
    loss = ops.pretrain_minibatch(p.d, precision, p.packed(precision), p.pf, p.tab, p.qs, T(inp["x0"]), T(inp["cond"]),
                                  T(inp["t"]), T(inp["noise"]), ws, grads, metrics, global_rows=global_rows,
                                  loss_scale=loss_scale)
    return loss, grads, metrics


def _run(p, precision, inp, **kw):
    import torch
    from diffusionpolicyoptimization_amd import ops
    loss, grads, metrics = _launch(p, precision, inp, **kw)
    torch.cuda.synchronize()
    return float(loss), ops.unflatten_params(p.spec, grads[:p.na].cpu().numpy()), grads, metrics


def _check(case, precision, loss, g, loss_ref, g_ref, only=None):
    bound = C.BOUND[precision]
    errs = C.errors(g, {k: v for k, v in g_ref.items() if only is None or k in only})
    loss_err = abs(loss - loss_ref) / abs(loss_ref)
    finite = bool(np.isfinite(loss)) and all(bool(np.isfinite(v).all()) for v in g.values())
    print(json.dumps({"case": case, "precision": precision, "bound": bound, "loss": loss, "loss_err": loss_err,
                      "finite": finite, "errs": errs}))
    assert finite, case
    bad = {k: v for k, v in errs.items() if not v < bound}
    assert loss_err < bound and not bad, (case, loss_err, bad)


def _compare(case, p, precision, inp, global_rows=None, loss_scale=1.0, **kw):
    loss, g, grads, metrics = _run(p, precision, inp, global_rows=global_rows, loss_scale=loss_scale, **kw)
    loss_ref, g_ref = C.reference(p.ft, p.sched, inp, rnd=_rnd(precision), global_rows=global_rows,
                                  loss_scale=loss_scale, dims=p.dims)
    _check(case, precision, loss, g, loss_ref, g_ref)
    return grads, metrics


def _refused(call, outputs, code, msg):
    """_rejected with the code of the check that fires: a DPPO_CHECK is DPPO_EINVAL, a dispatch refusal 3"""
    import torch
    from diffusionpolicyoptimization_amd._lib import DppoError
    if code == 3:
        return _rejected(call, outputs, msg)
    with pytest.raises(DppoError, match=re.escape(f"failed ({code}): {msg}")):
        call()
    torch.cuda.synchronize()
    for o in outputs:
        assert bool((o == SENTINEL).all()), "a rejected call wrote its outputs"


def _sentinels(p, extra=0):
    import torch
    return (torch.full((p.na + extra,), SENTINEL, dtype=torch.float32, device=p.cuda),
            torch.full((16,), SENTINEL, dtype=torch.float64, device=p.cuda))


# ------------------------------------------------------------------------------------------------
# Part A: dppo_pretrain_minibatch at its edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,precision", C.ROWS_CASES, ids=[f"{r}-{p}" for r, p in C.ROWS_CASES])
def test_rows_around_tile_and_pad_edges(cuda, rows, precision):
    """1, 15, 16, 17, 33, 64, 65 rows (the 16-row MFMA tiles of the 32-row tile, the 64-padded ldm, padded rows
    with segment id -1), t = arange(rows) % 20: loss and every gradient within the bound."""
    from diffusionpolicyoptimization_amd import ops
    p = _problem(cuda)
    assert ops.ppo_plan(p.d, precision, rows, "pretrain")["actor_tile_rows"] == 32
    _compare(f"rows{rows}", p, precision, C.inputs(rows, 20))


@pytest.mark.parametrize("precision", C.POP_PRECISIONS)
@pytest.mark.parametrize("pattern", C.POP_PATTERNS)
def test_t_populations(cuda, pattern, precision):
    """70 rows with one bucket (t = 0, t = K - 1), two ({0, K - 1}) or a single row at t = 7 among rows at t = 3:
    the empty buckets add nothing to the time-MLP gradients and the in-layer bias (the comparison), and every
    gradient is finite (_check)."""
    _compare(f"t-{pattern}", _problem(cuda), precision, C.inputs(C.POP_ROWS, 20, pattern))


@pytest.mark.parametrize("precision", C.PRECISIONS)
@pytest.mark.parametrize("K,rows", C.K_CASES)
def test_k_edges(cuda, K, rows, precision):
    """K = 1 and 2 (17 rows) and K = 64 (70 rows: every bin of seg_reduce_kernel, the int8 segment id 63), on the
    32-row tile, which takes every K <= 64."""
    from diffusionpolicyoptimization_amd import ops
    p = _problem(cuda, K)
    assert ops.ppo_plan(p.d, precision, rows, "pretrain")["actor_tile_rows"] == 32
    _compare(f"K{K}-rows{rows}", p, precision, C.inputs(rows, K))


def test_k65_rejected(cuda):
    """denoising_steps = 65: refused by the entry's own check (DPPO_EINVAL), outputs untouched"""
    p = _problem(cuda, C.K_REJECTED)
    grads, metrics = _sentinels(p)
    _refused(lambda: _launch(p, "bf16", C.inputs(17, C.K_REJECTED), grads=grads, metrics=metrics), (grads, metrics),
             EINVAL, "dppo_pretrain_minibatch: denoising_steps > 64 unsupported (bucket sums)")


def test_time_stride_rejected(cuda):
    """a DDIM table (time_stride 2): refused, outputs untouched"""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    p = _Problem(cuda, HOPPER_DDIM)
    p.qs = torch.tensor(ops.q_sched_table(ddpm_buffers(p.d.denoising_steps)), device=cuda)
    grads, metrics = _sentinels(p)
    _refused(lambda: _launch(p, "bf16", C.inputs(17, p.d.denoising_steps), grads=grads, metrics=metrics),
             (grads, metrics), EINVAL,
             "dppo_pretrain_minibatch: the time-embedding table must be unstrided (time_stride 1)")


def test_global_rows_below_rows_rejected(cuda):
    p = _problem(cuda)
    grads, metrics = _sentinels(p)
    _refused(lambda: _launch(p, "fp32", C.inputs(40, 20), global_rows=39, grads=grads, metrics=metrics),
             (grads, metrics), EINVAL, "dppo_pretrain_minibatch: bad rows / global_rows")


def _tile64_rows(cuda):
    import torch
    return 64 * torch.cuda.get_device_properties(cuda).multi_processor_count


def test_tile64_lds_line_refuses_k24(cuda):
    """bf16, one round of 64-row tiles (64 x CU-count rows): the tile keeps K rows of time embeddings and schedule
    in LDS, 161,616 + 96 K bytes at hopper's geometry, so K = 24 (163,920 B) is refused before any launch, outputs
    untouched; one tile fewer runs the 32-row tile, which takes it (include/dppo.h, "K in pretraining")."""
    from diffusionpolicyoptimization_amd import ops
    K, rows = C.TILE64_K_REFUSED, _tile64_rows(cuda)
    p = _problem(cuda, K)
    assert ops.ppo_plan(p.d, "bf16", rows, "pretrain")["actor_tile_rows"] == 64
    assert ops.ppo_plan(p.d, "bf16", rows - 64, "pretrain")["actor_tile_rows"] == 32
    grads, metrics = _sentinels(p)
    _refused(lambda: _launch(p, "bf16", C.inputs(rows, K), grads=grads, metrics=metrics), (grads, metrics), 3,
             f"actor row tile needs {C.TILE64_LDS(K)} B LDS")


def test_tile64_runs_k23(cuda):
    """K = 23 at the same rows is the last the 64-row tile takes (163,824 B): one launch, the loss and three
    tensors (in_b and time_w1 from the K bucket sums, l1_w from the dW) against the oracle over all the rows (the
    float64 oracle at 64 x 256 rows takes about 2 s on the CPU, so the whole batch is the reference)."""
    from diffusionpolicyoptimization_amd import ops
    K, rows = C.TILE64_K_OK, _tile64_rows(cuda)
    p = _problem(cuda, K)
    assert ops.ppo_plan(p.d, "bf16", rows, "pretrain")["actor_tile_rows"] == 64
    inp = C.inputs(rows, K)
    loss, g, _, _ = _run(p, "bf16", inp)
    loss_ref, g_ref = C.reference(p.ft, p.sched, inp, rnd=_rnd("bf16"), dims=p.dims)
    _check(f"tile64-K{K}-rows{rows}", "bf16", loss, g, loss_ref, g_ref, only=("in_b", "time_w1", "l1_w"))
    assert all(bool(np.isfinite(v).all()) for v in g.values())


@pytest.mark.parametrize("precision", C.PRECISIONS)
@pytest.mark.parametrize("loss_scale", C.SHARD_SCALES)
def test_shard_and_loss_scale(cuda, loss_scale, precision):
    """40 rows of a 160-row global batch with loss_scale 0.25 and 3: O.p_losses(denom = 160 xd) times loss_scale,
    the loss and every gradient; fp16 through round_fp16_rows(160), the row-tied gradient scale of global_rows"""
    _compare(f"shard40of160-ls{loss_scale}", _problem(cuda), precision, C.inputs(C.SHARD_ROWS, 20),
             global_rows=C.SHARD_GLOBAL, loss_scale=loss_scale)


@pytest.mark.parametrize("precision", C.CONTRACT_PRECISIONS)
def test_buffer_contract(cuda, precision):
    """The workspace need not be initialised (every byte 0xFF: NaN in every operand type), grads are overwritten
    and metrics zeroed (both handed in full of a sentinel): the result is finite and within the bound,
    metrics[1:16] are exactly 0, and the tail of a longer grads buffer is untouched."""
    from diffusionpolicyoptimization_amd import ops
    p = _problem(cuda)
    ws = ops.ppo_workspace(p.d, precision, C.CONTRACT_ROWS, cuda)
    ws.fill_(0xFF)
    grads, metrics = _sentinels(p, extra=C.CONTRACT_TAIL)
    _compare(f"dirty-rows{C.CONTRACT_ROWS}", p, precision, C.inputs(C.CONTRACT_ROWS, 20), ws=ws, grads=grads,
             metrics=metrics)
    assert bool((metrics[1:] == 0).all()), metrics.cpu().numpy()
    assert bool((grads[p.na:] == SENTINEL).all()), "the entry wrote past the actor's gradients"


@pytest.mark.parametrize("precision", C.CONTRACT_PRECISIONS)
def test_workspace_reused_by_a_shorter_batch(cuda, precision):
    """DiffusionModel.p_losses' pattern at a ragged last batch: one workspace sized for 256 rows (ldm 256), a
    256-row call, then 100 other rows (ldm 128: another layout over the first call's bytes) with nothing
    cleared between, into the same grads and metrics. The second result meets the bound for its 100 rows."""
    from diffusionpolicyoptimization_amd import ops
    p = _problem(cuda)
    big, small = C.REUSE_ROWS
    ws = ops.ppo_workspace(p.d, precision, big, cuda)
    grads, metrics = _compare(f"reuse-first{big}", p, precision, C.inputs(big, 20), ws=ws)
    _compare(f"reuse-then{small}", p, precision, C.inputs(small, 20, seed=1), ws=ws, grads=grads, metrics=metrics)


@pytest.mark.parametrize("precision", C.PRECISIONS)
def test_callers_stream(cuda, precision):
    """test_pretrain_loss_grads' 150-row call inside torch.cuda.stream(side), inputs, image and buffers produced
    on that stream: the same bound after side.synchronize() (the entry runs on the caller's stream)."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    p = _problem(cuda)
    inp = C.recipe150()
    side = torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        q = _Problem.__new__(_Problem)      # the same problem with its image packed on the side stream
        q.__dict__.update(p.__dict__)
        q._packed = {precision: ops.pack_actor(p.d, p.pf, precision)}
        loss, grads, _ = _launch(q, precision, inp)
    side.synchronize()
    loss_ref, g_ref = C.reference(p.ft, p.sched, inp, rnd=_rnd(precision))
    _check("side-stream-150", precision, float(loss), ops.unflatten_params(p.spec, grads.cpu().numpy()), loss_ref, g_ref)
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows", C.MAG_ROWS)
def test_fp16_at_magnitude(cuda, rows):
    """fp16, 1 and 17 rows, x0 exactly +-1 and noise at 3 N(0, 1) (the oracle's own rounded intermediates stay
    below 65504 there: tests/test_pretrain_step_cpu.py): finite and within the fp16 bound against
    round_fp16_rows."""
    _compare(f"magnitude-rows{rows}", _problem(cuda), "fp16",
             C.inputs(rows, 20, x0_edge=True, noise_scale=C.MAG_NOISE))


# ------------------------------------------------------------------------------------------------
# Part B: the pretraining step, teacher-forced against float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pretrain_steps_follow_the_oracle(cuda, tmp_path, precision):
    """TrainDiffusionAgent.run() over three epochs of two batches (48 rows and a short one of 16), the schedule's
    restart at step 5. p_losses is wrapped to draw its noise itself (the method's own call on the model's
    generator, so the training is the unwrapped one) and record the batch; apply_gradients to snapshot the state
    around the step. Per step i: the gradient and loss against O.p_losses at the GPU's own parameters; the image
    the kernels ran equal to a fresh pack of those parameters (and again after repack_network); p', m', v'
    against helpers.adamw_oracle from the stored state with lr_i restated in float64 at index i - 1, step = i and
    the cfg's weight decay (ratios <= 1). Per epoch: the returned loss is the mean of its batch losses; the EMA
    is a copy before epoch_start_ema and decay ema + (1 - decay) params after (2 fp32 ulps); state_3 and
    ema_state_3 load back to the two vectors."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.agent.dataset.sequence import synthetic_dataset
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    from diffusionpolicyoptimization_amd.util.config import get_class, instantiate, load_config
    data = synthetic_dataset(str(tmp_path / "train.npz"), n_episodes=C.RUN["n_episodes"],
                             episode_len=C.RUN["episode_len"])
    cfg = load_config(os.path.join(ROOT, "cfg/gym/pretrain/hopper-medium-v2"), "pre_diffusion_mlp",
                      [f"train_dataset_path={data}", f"logdir={tmp_path}/log", f"model.precision={precision}"]
                      + C.RUN_OVERRIDES)
    agent = get_class(cfg._target_)(cfg)
    model, opt = agent.model, agent.optimizer
    d, spec = model.pre_dims, model.pre_spec
    tr = cfg.train
    wd_cfg = float(tr.weight_decay)
    sched_args = (float(tr.learning_rate), int(tr.lr_scheduler.first_cycle_steps), float(tr.lr_scheduler.min_lr))
    assert wd_cfg == C.RUN["weight_decay"] and model.precision == precision

    def fresh_image():
        """model.packed with its segments re-derived from the current parameters (the gaps keep their bytes)"""
        img = model.packed.clone()
        ops.pack_actor(d, model.params, precision, out=img)
        return img

    batches, steps, repacks, epochs, emas = [], [], [], [], []
    p_losses, apply_gradients, repack = model.p_losses, opt.apply_gradients, model.repack_network
    train_epoch, step_ema = agent.train_epoch, agent.step_ema

    def w_p_losses(x_start, cond, t, noise=None, **kw):
        assert noise is None and not kw
        B = x_start.shape[0]
        noise = torch.randn(B, d.xd, device=model.device, generator=model._pre_gen)
        image_ok = torch.equal(model.packed, fresh_image())
        loss = p_losses(x_start, cond, t, noise=noise)
        batches.append(dict(x0=x_start.clone(), cond=cond["state"].clone(), t=t.clone(), noise=noise, loss=loss.clone(),
                            image_ok=image_ok))
        return loss

    def w_apply(grads):
        before = [x.clone() for x in (opt.params, opt.m, opt.v, grads)]
        lr = apply_gradients(grads)
        steps.append(dict(before=before, after=[x.clone() for x in (opt.params, opt.m, opt.v)], lr=lr,
                          iterations=opt.iterations))
        return lr

    def w_repack():
        repack()
        repacks.append(torch.equal(model.packed, fresh_image()))

    def w_train_epoch():
        n0 = len(batches)
        loss = train_epoch()
        epochs.append(dict(loss=loss, batches=(n0, len(batches))))
        return loss

    def w_step_ema():
        prev, epoch = agent.ema_params.clone(), agent.epoch
        step_ema()
        emas.append(dict(epoch=epoch, prev=prev, ema=agent.ema_params.clone(), params=model.params.clone()))

    model.p_losses, opt.apply_gradients, model.repack_network = w_p_losses, w_apply, w_repack
    agent.train_epoch, agent.step_ema = w_train_epoch, w_step_ema
    agent.run()
    torch.cuda.synchronize()
    final_image_ok = torch.equal(model.packed, fresh_image())

    n = lambda x: x.detach().cpu().numpy()
    assert [b["x0"].shape[0] for b in batches] == [48, 16] * 3 and len(steps) == len(batches) == 6
    K, bound, rnd = model.denoising_steps, C.BOUND[precision], _rnd(precision)
    sched = O.with_param(ddpm_buffers(K), model.denoised_clip_value, model.predict_epsilon)
    failures = []
    for i, (b, s) in enumerate(zip(batches, steps), start=1):
        B = b["x0"].shape[0]
        P, M, V, G = (n(x) for x in s["before"])
        t = n(b["t"])
        assert t.min() >= 0 and t.max() < K
        loss_ref, g_ref = O.p_losses(to_f64(ops.unflatten_params(spec, P)), sched,
                                     n(b["x0"]).astype(np.float64).reshape(B, d.horizon_steps, d.action_dim),
                                     n(b["cond"]).astype(np.float64).reshape(B, d.cond_steps, d.obs_dim), t,
                                     n(b["noise"]).astype(np.float64).reshape(B, d.horizon_steps, d.action_dim), rnd=rnd,
                                     model=O.Model.from_dims(d))
        errs = C.errors(ops.unflatten_params(spec, G), g_ref)
        loss = float(b["loss"])
        loss_err = abs(loss - loss_ref) / loss_ref
        lr_i = C.lr_at(i - 1, *sched_args)
        hp = C.run_hp(i, *sched_args, wd_cfg)
        ref, bounds = adamw_oracle("keras", P, M, V, G, i, hp)
        ratios = step_ratios([n(x) for x in s["after"]], ref, bounds)
        row = {"case": f"pretrain-run-{precision}", "step": i, "rows": B, "loss": loss, "loss_err": loss_err,
               "grad_errs": errs, "bound": bound, "lr": s["lr"], "lr_ref": lr_i, "adamw_ratios": ratios,
               "image_current_before": b["image_ok"], "image_current_after_repack": repacks[i - 1] if i <= len(repacks) else None}
        print(json.dumps(row))
        if not (loss_err < bound and all(v < bound for v in errs.values())):
            failures.append(("gradient", i, loss_err, {k: v for k, v in errs.items() if not v < bound}))
        if not (s["iterations"] == i and abs(s["lr"] - lr_i) <= 1e-12 * lr_i):
            failures.append(("schedule", i, s["iterations"], s["lr"], lr_i))
        if not max(ratios) <= 1.0:
            failures.append(("adamw", i, ratios))
        if not b["image_ok"]:
            failures.append(("stale image", i))
    assert len(repacks) == len(steps) and all(repacks), repacks
    assert final_image_ok
    assert not failures, failures

    assert len(epochs) == len(emas) == 3
    decay, ema_ref = float(cfg.ema.decay), None
    for e, (ep, em) in enumerate(zip(epochs, emas), start=1):
        lo, hi = ep["batches"]
        mean = float(np.mean([float(b["loss"]) for b in batches[lo:hi]]))
        assert em["epoch"] == e and hi - lo == 2
        ema_ref, tol = C.ema_expected(n(em["prev"]), n(em["params"]), e, int(tr.epoch_start_ema), decay)
        over = np.abs(n(em["ema"]).astype(np.float64) - ema_ref) - tol
        print(json.dumps({"case": f"pretrain-run-{precision}", "epoch": e, "loss": ep["loss"], "mean_of_batches": mean,
                          "ema_excess_max": float(over.max()), "ema_is_copy": bool(torch.equal(em["ema"], em["params"]))}))
        assert abs(ep["loss"] - mean) <= 1e-12 * abs(mean)
        assert (over <= 0).all(), (e, float(over.max()))
        assert torch.equal(em["ema"], em["params"]) == (e < int(tr.epoch_start_ema))
    for name, want in (("state_3", model.params), ("ema_state_3", agent.ema_params)):
        ck = os.path.join(agent.checkpoint_dir, name + ".weights.h5")
        assert os.path.exists(ck), ck
        m2 = instantiate(cfg.model, network_path=ck)
        m2._pretrain_init()
        assert torch.equal(m2.params, want), name
    assert torch.equal(agent.ema_params, emas[-1]["ema"]) and torch.equal(model.params, steps[-1]["after"][0])
