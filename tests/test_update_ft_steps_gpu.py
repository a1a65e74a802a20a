"""dppo_ppo_minibatch at ft_denoising_steps above 16 (K' up to 64) against the float64 oracle.

The actor's dW forms the per-t bucket sums of dh1 (in_b and, through the time-MLP backward, time_w1 /
b1 / w2 / b2) 16 buckets to a wave row of its 256-row tile: K' = 17 puts one bucket in the second wave
row, 33 one in the third, 64 fills all four. The cases are tests/test_update_surface_gpu.py's: 150 rows
of 40 samples from permutation position 37, fp32 'perturbed' at 2e-3, bf16 / fp16 'ratio 1' against the
rounding oracle at 1e-2 (the bounds its ft16 case passes under), per gradient tensor
max|g - ref| / (max|ref| + 1e-12), the metrics at that file's bounds; the learnable-eta derivative in
fp16 at test_update_regimes_gpu's 3e-2. Every figure is printed before it is asserted.
"""
import json

import numpy as np
import pytest

from oracle import dppo_oracle as O
from oracle import philox as PX
from tests.helpers import HOPPER, to_f64
from tests.test_kernels_gpu import _dedup, _rnd
from tests.test_update_regimes_gpu import EPOCH, SEED, START, TOL, _Case, _check_errs, _check_metrics, _tensor_errs
from tests.test_update_surface_gpu import SENTINEL, _rejected

pytestmark = pytest.mark.gpu

ROWS, NSAMP = 150, 40
NAMED = ("time_w1", "time_b1", "time_w2", "time_b2", "in_w", "in_b")


def _dims(K, KF, **kw):
    return dict(HOPPER, denoising_steps=K, ft_denoising_steps=KF, **kw)


# DDIM: 20 sampling rows over K = 100 (time stride 5), all fine-tuned
DDIM20 = _dims(20, 20, time_stride=5)
_CASES = {}


def _case(cuda, precision, dims, N=NSAMP, eta=1.0):
    """One _Case at a time (fp32: perturbed old log-probs, rows on both clip branches; 2-byte: ratio 1)."""
    key = (precision, json.dumps(dims, sort_keys=True), N, eta)
    if key not in _CASES:
        _CASES.clear()
        _CASES[key] = _Case(cuda, precision, dims, N, lp="perturbed" if precision == "fp32" else "ratio1", eta=eta)
    return _CASES[key]


def _rows_of(case, start, rows):
    perm = PX.feistel_permute(np.arange(start, start + rows), case.total, SEED, EPOCH)
    return perm // case.kf, perm % case.kf


def _oracle(case, start, rows, adv_mean_std=None, eta_grad=False):
    """_Case.oracle over permutation rows [start, start + rows)."""
    d = case.d
    bi, di = _rows_of(case, start, rows)
    sh = (rows, d.horizon_steps, d.action_dim)
    return O.c_loss(to_f64(case.ft), to_f64(case.critic), case.sched, case.obs[bi].reshape(rows, 1, -1).astype(np.float64),
                    case.chains[bi, di].reshape(sh).astype(np.float64), case.chains[bi, di + 1].reshape(sh).astype(np.float64),
                    di, case.ret[bi].astype(np.float64), None, case.adv[bi].astype(np.float64), case.lp_old_ref[bi, di],
                    case.kf, rnd=_rnd(case.precision), adv_mean_std=adv_mean_std, denom=rows, critic_dedup=_dedup(bi),
                    eta_grad=eta_grad, model=case.model)


class _Out:
    """The outputs a sequence of launches shares: workspace, gradients, metric sums."""

    def __init__(self, case, rows, fill=0.0):
        import torch
        from diffusionpolicyoptimization_amd import ops
        self.grads = torch.full((case.na + case.nc,), fill, dtype=torch.float32, device=case.cuda)
        self.met = torch.full((16,), fill, dtype=torch.float64, device=case.cuda)
        self.ws = ops.ppo_workspace(case.d, case.precision, rows, case.cuda)

    def read(self):
        import torch
        torch.cuda.synchronize()
        return self.grads.cpu().numpy().astype(np.float64), self.met.cpu().numpy()


def _stats(case, start, rows):
    import torch
    from diffusionpolicyoptimization_amd import ops
    st = torch.zeros(3, dtype=torch.float64, device=case.cuda)
    ops.ppo_adv_stats(case.args[3], case.total, case.kf, SEED, EPOCH, start, rows, st)
    return st


def _launch(case, out, start, rows, part=None, precleared=False, learn_eta=False, stats=None):
    from diffusionpolicyoptimization_amd import _lib, ops
    hp = ops.ppo_hparams(global_rows=rows, learn_eta=learn_eta)
    if precleared:
        hp.flags |= _lib.DPPO_PPO_PRECLEARED
    ops.ppo_minibatch(case.d, case.precision, hp, case.packf, case.packc, case.pf, case.tab, *case.args, SEED, EPOCH,
                      start, rows, out.ws, out.grads, out.met, adv_stats=stats, part=part)


def _check(case, g, m, ref, label, rows=ROWS):
    """Metrics (test_update_surface_gpu's bounds, the ratio mean at pg_loss's form) and every gradient
    tensor at TOL; the bucket-sum tensors by name."""
    met_ref, ga_ref, gc_ref = ref
    rtol, ratio1 = TOL[case.precision], case.precision != "fp32"
    assert np.isfinite(g).all() and np.isfinite(m).all(), label
    if ratio1:
        assert met_ref["clipfrac"] == 0.0
    _check_metrics(m / rows, met_ref, rtol, ratio1, label)
    assert abs(m[4] / rows - met_ref["ratio"]) <= rtol * (abs(met_ref["ratio"]) + 1e-2), (label, m[4] / rows, met_ref["ratio"])
    errs = _tensor_errs(case.d, g, ga_ref, gc_ref)
    assert set(NAMED) <= set(errs) and any(k.startswith("critic.") for k in errs), errs.keys()
    for k in NAMED:
        assert np.abs(ga_ref[k]).max() > 0, k
    _check_errs(errs, rtol, label)
    return errs


GEOMETRIES = {"k20-ft17": _dims(20, 17), "k20-ft20": _dims(20, 20), "k33-ft33": _dims(33, 33), "k64-ft64": _dims(64, 64)}
ORACLE_PARAMS = [("k20-ft17", "fp32"), ("k20-ft17", "bf16"), ("k20-ft20", "fp32"), ("k20-ft20", "bf16"),
                 ("k20-ft20", "fp16"), ("k33-ft33", "bf16"), ("k64-ft64", "fp32"), ("k64-ft64", "bf16")]


@pytest.mark.parametrize("geometry,precision", ORACLE_PARAMS, ids=["-".join(x) for x in ORACLE_PARAMS])
def test_ft_steps_match_oracle(cuda, geometry, precision):
    """One whole minibatch at K' = 17 (bucket 16 alone in the second wave row), 20 (the config users
    run), 33 (bucket 32 alone in the third) and 64 (four full wave rows; chains are random draws, no
    sampler launch). The 150 rows reach every wave row the geometry has (asserted)."""
    case = _case(cuda, precision, GEOMETRIES[geometry])
    _, di = _rows_of(case, START, ROWS)
    t = case.kf - 1 - di
    assert {int(w) for w in np.unique(t // 16)} == set(range(-(-case.kf // 16))), np.unique(t)
    out = _Out(case, ROWS, fill=SENTINEL)
    _launch(case, out, START, ROWS)
    g, m = out.read()
    _check(case, g, m, _oracle(case, START, ROWS), f"{geometry}-{precision}")


def test_ft65_is_refused_before_launch(cuda):
    """K = K' = 65 is refused with the unsupported-configuration error (code 3) naming the bound, the
    sentinel-filled gradients and metrics untouched, and the stream's sample-count scratch unused: the
    same K' = 20 minibatch before and after it gives the same result."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    good = _case(cuda, "fp32", GEOMETRIES["k20-ft20"])
    o0 = _Out(good, ROWS)
    _launch(good, o0, START, ROWS)
    g0, m0 = o0.read()
    d = ops.ModelDims(**_dims(65, 65))
    rng = np.random.default_rng(3)
    T = lambda x: torch.tensor(np.asarray(x, np.float32), device=cuda)
    na, nc = ops.spec_count(ops.actor_param_spec(d)), ops.spec_count(ops.critic_param_spec(d))
    grads = torch.full((na + nc,), SENTINEL, dtype=torch.float32, device=cuda)
    metrics = torch.full((16,), SENTINEL, dtype=torch.float64, device=cuda)
    tab = T(ops.sched_table(ddpm_buffers(65)))
    for precision in ("fp32", "bf16"):
        call = lambda: ops.ppo_minibatch(
            d, precision, ops.ppo_hparams(global_rows=ROWS), ops.pack_actor(d, good.pf, precision),
            ops.pack_critic(d, good.pc, precision), good.pf, tab, T(rng.uniform(-1, 1, (NSAMP, d.sd))),
            T(rng.standard_normal((NSAMP, 66, d.xd)) * 0.5), T(rng.normal(-1, 0.1, (NSAMP, 65))), T(rng.normal(size=NSAMP)),
            T(rng.normal(size=NSAMP)), SEED, EPOCH, START, ROWS, ops.ppo_workspace(d, precision, ROWS, cuda), grads, metrics)
        _rejected(call, (grads, metrics), "dppo_ppo_minibatch: ft_denoising_steps 65 > 64 unsupported (bucket sums)")
    o1 = _Out(good, ROWS)
    _launch(good, o1, START, ROWS)
    g1, m1 = o1.read()
    np.testing.assert_allclose(m1[:5], m0[:5], rtol=1e-6, atol=1e-9)
    assert np.abs(g1 - g0).max() <= 1e-5 * np.abs(g0).max()


def test_tile64_lds_bound_on_ft_steps(cuda):
    """The 64-row actor tile (2-byte operands, at least one round of 64-row tiles) keeps K' rows of
    time embeddings and schedule in LDS beside its activation tiles: hopper's geometry needs
    161,616 + 96 K' bytes, so K' = 23 is the last that fits 160 KiB (163,824 B) and K' = 24 is refused before anything
    is launched, naming the bytes (the 32-row tile of smaller minibatches takes every K' <= 64)."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    good = _case(cuda, "bf16", GEOMETRIES["k20-ft20"])
    rows = 64 * torch.cuda.get_device_properties(cuda).multi_processor_count
    d = ops.ModelDims(**_dims(24, 24))
    assert ops.ppo_plan(d, "bf16", rows)["actor_tile_rows"] == 64
    assert ops.ppo_plan(d, "bf16", rows - 64)["actor_tile_rows"] == 32
    n = -(-(START + rows) // 24)
    rng = np.random.default_rng(3)
    T = lambda x: torch.tensor(np.asarray(x, np.float32), device=cuda)
    grads = torch.full((good.na + good.nc,), SENTINEL, dtype=torch.float32, device=cuda)
    metrics = torch.full((16,), SENTINEL, dtype=torch.float64, device=cuda)
    call = lambda: ops.ppo_minibatch(
        d, "bf16", ops.ppo_hparams(global_rows=rows), ops.pack_actor(d, good.pf, "bf16"), good.packc, good.pf,
        T(ops.sched_table(ddpm_buffers(24))), T(rng.uniform(-1, 1, (n, d.sd))), T(rng.standard_normal((n, 25, d.xd)) * 0.5),
        T(rng.normal(-1, 0.1, (n, 24))), T(rng.normal(size=n)), T(rng.normal(size=n)), SEED, EPOCH, START, rows,
        ops.ppo_workspace(d, "bf16", rows, cuda), grads, metrics)
    _rejected(call, (grads, metrics), "actor row tile needs 163920 B LDS")


@pytest.mark.parametrize("learn_eta", [False, True], ids=["ddim20", "ddim20-learn-eta"])
def test_ft20_ddim_stride_matches_oracle(cuda, learn_eta):
    """DDIM, fp16: 20 sampling rows at time stride 5, all fine-tuned, so the time-MLP backward's
    bucket q sits at t = 5 q for 20 buckets; with DPPO_PPO_LEARN_ETA (eta = 0.6) also the eta
    derivative in metrics[8], at test_update_regimes_gpu's fp16 bound (3e-2)."""
    case = _case(cuda, "fp16", DDIM20, eta=0.6 if learn_eta else 1.0)
    assert case.d.time_stride == 5 and case.kf == 20
    ref = _oracle(case, START, ROWS, eta_grad=learn_eta)
    out = _Out(case, ROWS)
    _launch(case, out, START, ROWS, learn_eta=learn_eta)
    g, m = out.read()
    _check(case, g, m, ref, "ddim20" + ("-learn-eta" if learn_eta else ""))
    if learn_eta:
        want = ref[0]["d_eta"]
        print(json.dumps({"d_eta": float(m[8]), "ref": want}))
        assert abs(want) > 1e-3 and abs(m[8] - want) <= 3e-2 * abs(want), (m[8], want)


def test_ft20_back_to_back_minibatches_zero_every_bucket(cuda):
    """Two different minibatches (rows 37.. and 187..) into the same workspace, gradients and metrics
    at K' = 20: the second equals the oracle's second alone, so the first's bucket sums 16..19 were
    zeroed (the dW adds into them with atomics)."""
    case = _case(cuda, "fp32", GEOMETRIES["k20-ft20"])
    out = _Out(case, ROWS)
    _launch(case, out, START, ROWS)
    g, m = out.read()
    _check(case, g, m, _oracle(case, START, ROWS), "first")
    _launch(case, out, START + ROWS, ROWS)
    g, m = out.read()
    _check(case, g, m, _oracle(case, START + ROWS, ROWS), "second")


def test_ft20_precleared_second_minibatch(cuda):
    """The split update's zeroing at K' = 20: minibatch one as actor and critic halves; each half's
    fused optimizer step (learning rate 0: the parameters and images stay) clears the gradients and
    the half's ops.ClearRanges; minibatch two runs DPPO_PPO_PRECLEARED into the same buffers and must
    equal the oracle's second alone. The ranges come from dppo_ppo_clear_ranges, which must reach
    bucket rows 16..19 of the workspace."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    case = _case(cuda, "fp32", GEOMETRIES["k20-ft20"])
    d, na = case.d, case.na
    out = _Out(case, ROWS)
    pf, pc = case.pf.clone(), case.pc.clone()
    zeros = lambda n: torch.zeros(n, dtype=torch.float32, device=cuda)
    step_a = ops.BoundOptimizerStep(d, "fp32", pf, out.grads[:na], zeros(na), zeros(na), 0.0, 0.9, 0.999, 1e-7, "keras",
                                    pf, case.packf, None, None, defer_sampler_tables=True, fused_pack=True, clear_grads=True)
    step_c = ops.BoundOptimizerStep(d, "fp32", pc, out.grads[na:], zeros(case.nc), zeros(case.nc), 0.0, 0.9, 0.999, 1e-7,
                                    "keras", None, None, pc, case.packc, fused_pack=True, clear_grads=True)
    clear_a, clear_c = (ops.ClearRanges(d, "fp32", ROWS, out.ws, out.met, part) for part in (1, 2))
    st = _stats(case, START, ROWS)
    for part in (1, 2):
        _launch(case, out, START, ROWS, part=part, stats=st)
    g, m = out.read()
    _check(case, g, m, _oracle(case, START, ROWS), "first")
    step_a(1, 0.0, clear=clear_a)
    step_c(1, 0.0, clear=clear_c)
    torch.cuda.synchronize()
    assert torch.equal(pf, case.pf) and torch.equal(pc, case.pc)
    assert int(torch.count_nonzero(out.grads)) == 0 and int(torch.count_nonzero(out.met)) == 0
    st = _stats(case, START + ROWS, ROWS)
    for part in (1, 2):
        _launch(case, out, START + ROWS, ROWS, part=part, precleared=True, stats=st)
    g, m = out.read()
    _check(case, g, m, _oracle(case, START + ROWS, ROWS), "second-precleared")


def test_ft20_multichunk_bucket_sums(cuda):
    """1,600 rows (test_update_regimes_gpu's multi-chunk size) at K' = 20: at least two actor dW
    m-chunks, each adding its partial sums of all 20 buckets from both wave rows."""
    from diffusionpolicyoptimization_amd import ops
    rows = 1600
    case = _case(cuda, "fp32", GEOMETRIES["k20-ft20"], N=170)
    plan = ops.ppo_plan(case.d, "fp32", rows)
    assert plan["dw_chunks_actor"] >= 2, plan
    out = _Out(case, rows)
    _launch(case, out, START, rows)
    g, m = out.read()
    _check(case, g, m, _oracle(case, START, rows), "multichunk-ft20", rows=rows)


def test_ft20_parts_match_whole(cuda):
    """dppo_ppo_minibatch_part as actor row tiles (4), actor dW (5) and critic (2) against the whole
    call at K' = 20, bf16: the parts against the oracle, and against the whole within
    test_split_update_matches_fused's bounds (median 1e-6, max 5e-3 absolute; metrics 1e-3 relative)."""
    case = _case(cuda, "bf16", GEOMETRIES["k20-ft20"])
    whole, parts = _Out(case, ROWS), _Out(case, ROWS)
    _launch(case, whole, START, ROWS)
    gw, mw = whole.read()
    st = _stats(case, START, ROWS)
    for part in (4, 5, 2):
        _launch(case, parts, START, ROWS, part=part, stats=st)
    gp, mp = parts.read()
    _check(case, gp, mp, _oracle(case, START, ROWS), "parts")
    diff = np.abs(gp - gw)
    print(json.dumps({"parts_vs_whole": {"median": float(np.median(diff)), "max": float(diff.max())}}))
    assert np.median(diff) < 1e-6 and diff.max() < 5e-3
    for slot in (0, 1):
        assert abs(mp[slot] - mw[slot]) <= 1e-3 * (abs(mw[slot]) + 1e-3), (slot, mp[slot], mw[slot])
