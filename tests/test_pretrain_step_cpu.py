"""The pretraining-step cases (tests/pretrain_cases.py) without a GPU: the inputs are what the case tables say,
the float64 oracle handles every K and rounding the GPU file asks of it, the fp16-at-magnitude inputs keep the
oracle's own rounded intermediates inside fp16, and each check of tests/test_pretrain_step_gpu.py can fail: the
mistake it is there for moves the oracle's result by more than the bound the GPU file asserts. The run of part B
is rolled forward in float64 with NumPy draws of t and noise (the proofs need no device draws)."""
import json
import os

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import pretrain_cases as C
from tests.helpers import adamw_oracle, step_ratios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = max(C.BOUND.values())


def _log(**kw):
    print(json.dumps(kw))


# ------------------------------------------------------------------------------------------------
# Part A
# ------------------------------------------------------------------------------------------------
def test_case_tables():
    """t stays in [0, K) everywhere; `cycle` populates min(rows, K) buckets; the population patterns hold the
    buckets they name; the row counts sit on both sides of the 16 / 32-row tiles and of the 64-row pad."""
    for rows, _ in C.ROWS_CASES:
        t = C.inputs(rows, 20)["t"]
        assert t.dtype == np.int32 and len(np.unique(t)) == min(rows, 20) and t.max() == min(rows, 20) - 1
    assert {r for r, _ in C.ROWS_CASES} == {1, 15, 16, 17, 33, 64, 65}
    assert {r for r, p in C.ROWS_CASES if p == "fp16"} == {1, 17, 65}
    pop = {k: C.inputs(C.POP_ROWS, 20, k)["t"] for k in C.POP_PATTERNS}
    assert set(pop["all0"]) == {0} and set(pop["allK-1"]) == {19} and set(pop["ends"]) == {0, 19}
    assert sorted(np.bincount(pop["single7"], minlength=20).nonzero()[0]) == [3, 7]
    assert int((pop["single7"] == 7).sum()) == 1 and pop["single7"][C.POP_ROWS // 2 + 1] == 7
    for K, rows in C.K_CASES:
        t = C.inputs(rows, K)["t"]
        assert len(np.unique(t)) == min(rows, K) and t.max() == K - 1      # K = 64: all 64 bins, id 63
    assert C.TILE64_LDS(C.TILE64_K_OK) <= 160 * 1024 < C.TILE64_LDS(C.TILE64_K_REFUSED) == 163920
    x0 = C.inputs(17, 20, x0_edge=True, noise_scale=C.MAG_NOISE)["x0"]
    assert set(np.unique(x0)) == {-1.0, 1.0}
    r = C.recipe150()
    rng = np.random.default_rng(21)          # test_pretrain_loss_grads' draws, in its order
    assert np.array_equal(r["x0"], rng.uniform(-1, 1, (150, 12)).astype(np.float32))


@pytest.mark.parametrize("precision", C.PRECISIONS)
@pytest.mark.parametrize("K,rows", [(1, 1), (1, 17), (2, 17), (20, 70), (64, 70)])
def test_oracle_handles_k_edges(K, rows, precision):
    p, sched = C.model(K)
    loss, g = C.reference(p, sched, C.inputs(rows, K), rnd=C.rnd_of(precision), dims=C.dims_of(K))
    assert np.isfinite(loss) and loss > 0 and all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in g.values())
    if precision != "fp32":    # how far the rounding points move the reference (a figure, not a bound)
        loss64, g64 = C.reference(p, sched, C.inputs(rows, K), dims=C.dims_of(K))
        _log(case=f"K{K}-rows{rows}-{precision}", rounded_vs_exact=max(C.errors(g, g64).values()),
             loss=abs(loss - loss64) / loss64)


@pytest.mark.parametrize("K,rows,pattern", [(20, 33, "cycle"), (20, 65, "cycle"), (2, 17, "cycle"), (64, 70, "cycle"),
                                            (20, 70, "ends"), (20, 70, "single7")])
def test_a_lost_bucket_shows(K, rows, pattern):
    """A bucket sum that is lost (the last bucket, tid < nb - 1 in seg_reduce_kernel, or the single row at
    t = 7) moves the in-layer bias or a time-MLP gradient by more than the bound: the oracle over the rows of the
    other buckets, with the same denominator, differs from the full one."""
    p, sched = C.model(K)
    inp = C.inputs(rows, K, pattern)
    lost = 7 if pattern == "single7" else K - 1
    _, g = C.reference(p, sched, inp, dims=C.dims_of(K), global_rows=rows)
    _, g_lost = C.reference(p, sched, C.subset(inp, inp["t"] != lost), dims=C.dims_of(K), global_rows=rows)
    errs = {k: v for k, v in C.errors(g_lost, g).items() if k == "in_b" or k.startswith("time_")}
    _log(case=f"K{K}-rows{rows}-{pattern}", lost_bucket=lost, moved=errs)
    assert max(errs.values()) > 2 * WORST


@pytest.mark.parametrize("rows", [r for r in (15, 16, 17, 33, 64, 65)])
def test_a_lost_last_row_shows(rows):
    """The row on the far side of a tile or pad edge counts: without the last row some tensor moves by more than
    the bound."""
    p, sched = C.model(20)
    inp = C.inputs(rows, 20)
    _, g = C.reference(p, sched, inp, global_rows=rows)
    _, g_lost = C.reference(p, sched, C.subset(inp, np.arange(rows) < rows - 1), global_rows=rows)
    errs = C.errors(g_lost, g)
    _log(case=f"rows{rows}", moved=max(errs.values()))
    assert max(errs.values()) > WORST


def test_shard_and_loss_scale_show():
    """global_rows taken as rows, or loss_scale dropped, moves the loss and every gradient by at least 25
    times the bound."""
    p, sched = C.model(20)
    inp = C.inputs(C.SHARD_ROWS, 20)
    for ls in C.SHARD_SCALES:
        loss, g = C.reference(p, sched, inp, global_rows=C.SHARD_GLOBAL, loss_scale=ls)
        for wrong in (dict(global_rows=C.SHARD_ROWS, loss_scale=ls), dict(global_rows=C.SHARD_GLOBAL, loss_scale=1.0)):
            loss_w, g_w = C.reference(p, sched, inp, **wrong)
            assert abs(loss_w - loss) / loss > 25 * WORST and min(C.errors(g_w, g).values()) > 25 * WORST
    # fp16: the row-tied gradient scale is that of global_rows (128 at 160 rows), not of the shard's 40 (32)
    assert O.fp16_grad_scale(C.SHARD_GLOBAL) == 128.0 and O.fp16_grad_scale(C.SHARD_ROWS) == 32.0


@pytest.mark.parametrize("rows", C.MAG_ROWS)
def test_fp16_magnitude_inputs_stay_in_range(rows):
    """x0 = +-1 with noise at 3 N(0, 1): every value the oracle rounds to fp16 (forward operands; gradient images
    times the row-tied scale) stays below 65504, so the kernel has no excuse for an inf."""
    p, sched = C.model(20)
    inp = C.inputs(rows, 20, x0_edge=True, noise_scale=C.MAG_NOISE)
    rnd, peak = C.recording_fp16(rows)
    loss, g = C.reference(p, sched, inp, rnd=rnd)
    _log(case=f"fp16-magnitude-rows{rows}", peak=peak, loss=loss, noise_max=float(np.abs(inp["noise"]).max()))
    assert 0 < peak["forward"] < C.FP16_MAX and 0 < peak["backward"] < C.FP16_MAX
    assert np.isfinite(loss) and all(np.isfinite(v).all() for v in g.values())
    # the recorder rounds as round_fp16 does under p_losses (which ties the scale to the rows itself)
    loss2, g2 = C.reference(p, sched, inp, rnd=O.round_fp16)
    assert loss2 == loss and all(np.array_equal(g[k], g2[k]) for k in g)


# ------------------------------------------------------------------------------------------------
# Part B: the run, rolled forward in float64
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The GPU file's run in float64: the same cfg, dataset and batches, the network's own seeded initial
    weights, t and noise from NumPy -> (steps, cfg): per 1-based step the batch, the parameters, moments and
    gradient before it, and the parameters after."""
    from diffusionpolicyoptimization_amd.agent.dataset.sequence import StitchedSequenceDataset, synthetic_dataset
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    from diffusionpolicyoptimization_amd.util.config import instantiate, load_config
    tmp = tmp_path_factory.mktemp("pretrain_run")
    data = synthetic_dataset(str(tmp / "train.npz"), n_episodes=C.RUN["n_episodes"], episode_len=C.RUN["episode_len"])
    cfg = load_config(os.path.join(ROOT, "cfg/gym/pretrain/hopper-medium-v2"), "pre_diffusion_mlp",
                      [f"train_dataset_path={data}", f"logdir={tmp}/log"] + C.RUN_OVERRIDES)
    ds = StitchedSequenceDataset(data, horizon_steps=cfg.horizon_steps, cond_steps=cfg.cond_steps, device="cpu")
    K = int(cfg.denoising_steps)
    sched = ddpm_buffers(K)
    p = {k: np.asarray(v, np.float64) for k, v in instantiate(cfg.model.network).init_params(np.random.default_rng(42)).items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    rng = np.random.default_rng(7)
    steps, i = [], 0
    tr = cfg.train
    for _ in range(int(tr.n_epochs)):
        for b in ds.batches(int(tr.batch_size)):
            i += 1
            x0 = b["actions"].numpy().astype(np.float64)
            cond = b["conditions"]["state"].numpy().astype(np.float64)
            B = x0.shape[0]
            t, z = rng.integers(0, K, B), rng.standard_normal(x0.shape)
            loss, g = O.p_losses(p, sched, x0, cond, t, z)
            hp = C.run_hp(i, float(tr.learning_rate), int(tr.lr_scheduler.first_cycle_steps),
                          float(tr.lr_scheduler.min_lr), float(tr.weight_decay))
            rec = dict(i=i, rows=B, batch=(x0, cond, t, z), p=p, m=m, v=v, g=g, loss=loss)
            p, m, v = ({k: adamw_oracle("keras", rec["p"][k], rec["m"][k], rec["v"][k], g[k], i, hp)[0][j] for k in g}
                       for j in range(3))
            steps.append(rec)
    return steps, cfg, sched


def test_run_shape(run):
    """two batches per epoch, the second short; the schedule restarts inside the run"""
    steps, cfg, _ = run
    assert [s["rows"] for s in steps] == [48, 16] * 3
    tr = cfg.train
    lr = [C.lr_at(k, float(tr.learning_rate), int(tr.lr_scheduler.first_cycle_steps), float(tr.lr_scheduler.min_lr))
          for k in range(7)]
    _log(lr=lr)
    assert lr[0] == lr[4] == 1e-3 and lr[1] == lr[5] and lr[0] > lr[1] > lr[2] > lr[3] < lr[4]
    assert float(tr.weight_decay) == C.RUN["weight_decay"]
    from diffusionpolicyoptimization_amd.util.scheduler import CosineDecayRestarts      # the restatement is the schedule
    s = CosineDecayRestarts(float(tr.learning_rate), tr.lr_scheduler.first_cycle_steps, t_mul=1.0, m_mul=1.0,
                            alpha=float(tr.lr_scheduler.min_lr) / float(tr.learning_rate))
    assert all(abs(s(k) - lr[k]) <= 1e-15 for k in range(7))


def test_a_stale_image_shows(run):
    """A missing repack_network(): the kernels would run the previous step's image. At every step >= 2 the
    oracle gradient at the previous step's parameters differs from the one at the current parameters by at
    least 10 times the bound in some tensor (learning_rate 1e-3 is enough; no need to raise it)."""
    steps, _, sched = run
    for prev, cur in zip(steps, steps[1:]):
        x0, cond, t, z = cur["batch"]
        loss_stale, g_stale = O.p_losses(prev["p"], sched, x0, cond, t, z)
        errs = C.errors(g_stale, cur["g"])
        _log(step=cur["i"], stale_moves=max(errs.values()), loss_moves=abs(loss_stale - cur["loss"]) / cur["loss"])
        assert max(errs.values()) >= 10 * WORST


@pytest.mark.parametrize("mistake", ["lr_next", "step_prev", "wd_zero", "wd_default"])
def test_a_wrong_schedule_step_or_decay_shows(run, mistake):
    """lr_{i+1} for lr_i (the schedule read after the counter moved), step i - 1 for i in the bias correction
    (i >= 2), weight decay 0 or AdamW's default 0.004 for the cfg's: each moves p' by more than
    helpers.adamw_oracle's bound in some element at some step."""
    steps, cfg, _ = run
    tr = cfg.train
    args = (float(tr.learning_rate), int(tr.lr_scheduler.first_cycle_steps), float(tr.lr_scheduler.min_lr))
    wd = float(tr.weight_decay)
    worst = {}
    for s in steps:
        i = s["i"]
        hp, step = C.run_hp(i, *args, wd), i
        if mistake == "lr_next":
            hp_w, step_w = C.run_hp(i + 1, *args, wd), i
        elif mistake == "step_prev":
            if i < 2:
                continue
            hp_w, step_w = hp, i - 1
        else:
            hp_w, step_w = C.run_hp(i, *args, 0.0 if mistake == "wd_zero" else 0.004), i
        q = 0.0
        for k in s["g"]:
            ref, bounds = adamw_oracle("keras", s["p"][k], s["m"][k], s["v"][k], s["g"][k], step, hp)
            wrong, _ = adamw_oracle("keras", s["p"][k], s["m"][k], s["v"][k], s["g"][k], step_w, hp_w)
            q = max(q, step_ratios(wrong[:1], ref[:1], bounds[:1])[0])
        worst[i] = q
    _log(mistake=mistake, ratio_by_step=worst)
    assert max(worst.values()) > 1.0
    if mistake != "lr_next":
        assert min(worst.values()) > 1.0       # at every step it applies to
    else:
        assert worst[4] > 1.0                  # step 4 -> 5 is the restart: lr_5 is the initial rate again


def test_ema_expectation_can_fail():
    """an EMA that starts an epoch early is not a copy: it differs from params by more than the zero tolerance"""
    rng = np.random.default_rng(0)
    ema, params = rng.normal(size=100), rng.normal(size=100)
    ref, tol = C.ema_expected(ema, params, 1, 2, 0.995)
    assert np.array_equal(ref, params) and not tol.any()
    early, tol2 = C.ema_expected(ema, params, 2, 2, 0.995)
    assert (np.abs(early - ref) > tol).all() and (tol2 > 0).all() and tol2.max() < 1e-6
