"""PPODiffusion's advantage clip on the device: the per-minibatch quantile select (csrc/select.hip), the
DPPO_PPO_ADV_CLIP row tiles and the agent, against the oracle's float64 definition (O.quantile, O.bounds) and its
c_loss with adv_clip_quantiles. Every figure is printed before it is asserted.

Bounds. The select: the four fp32 order statistics of every segment exact (bit patterns, +-0 as values); the
fp64 interpolation within 4 ulps of float64, relative (the device evaluates the definition's own operations
with contraction off, so the difference is 0 where it was measured). The flagged minibatch: per gradient tensor
and metric the bounds of the cases it mirrors in tests/test_update_surface_gpu.py (fp32 2e-3, bf16 1e-2).
The agent: tests/test_iteration_gpu.py's. tests/test_adv_clip_cpu.py proves on the same inputs that quantiles
(0.1, 0.9) move the loss and every actor gradient by ten of those bounds."""
import gc
import json
import os

import numpy as np
import pytest

from oracle import dppo_oracle as O
from oracle import philox as PX
from tests import adv_clip_cases as AO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SENTINEL = -7.25


def _segments(adv, kf, seed, epoch0, n_epochs, rows_full, n_batch):
    """The value multiset of every segment, as dppo_ppo_adv_stats_all indexes minibatches."""
    total = adv.size * kf
    out = []
    for e in range(n_epochs):
        for b in range(n_batch):
            s, t = b * rows_full, min((b + 1) * rows_full, total)
            if s >= t:
                out.append(np.zeros(0, np.float32))
                continue
            perm = PX.feistel_permute(np.arange(s, t), total, seed, epoch0 + e)
            out.append(adv[perm // kf])
    return out


def _select(cuda, adv, kf, seed, epoch0, n_epochs, rows_full, n_batch, q_lo, q_hi):
    """ops.ppo_adv_quantiles_all -> (bounds [n_seg, 2], the four selected fp32 values per segment)."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    n_seg = n_epochs * n_batch
    out = torch.full((n_seg, 2), SENTINEL, dtype=torch.float64, device=cuda)
    ws = ops.ppo_adv_quantiles_workspace(n_epochs, n_batch, cuda)
    ops.ppo_adv_quantiles_all(torch.tensor(adv, device=cuda), adv.size * kf, kf, seed, epoch0, n_epochs, rows_full,
                              n_batch, q_lo, q_hi, out, workspace=ws)
    torch.cuda.synchronize()
    state = ws[n_seg * 4096:n_seg * 4096 + n_seg * 72].view(torch.int64).view(n_seg, 9).cpu().numpy()
    keys = state[:, 0:8:2].astype(np.uint32)
    return out.cpu().numpy(), AO.values_of(keys.reshape(-1)).reshape(n_seg, 4), state[:, 8]


def _check_segment(label, vals, q_lo, q_hi, got, sel, worst):
    if vals.size == 0:
        assert got[0] == -np.inf and got[1] == np.inf, (label, got)
        return
    for i, q in enumerate((q_lo, q_hi)):
        n, k, k1, vk, vk1 = O.order_stats(vals, q)
        assert sel[2 * i] == vk and sel[2 * i + 1] == vk1, (label, q, sel, vk, vk1)   # exact order statistics
        ref = O.quantile(vals, q)
        err = abs(got[i] - ref) / max(abs(ref), np.finfo(np.float64).tiny)
        worst[0] = max(worst[0], err / EPS)
        assert err <= 4 * EPS, (label, q, got[i], ref)


@pytest.mark.parametrize("kind", AO.SELECT_KINDS)
def test_select_matches_the_definition(cuda, kind):
    """One segment of n rows (the first n positions of the permutation), n across the wave, workgroup and chunk
    edges up to one row past the count loop's second trip, at every quantile pair of select_quantiles."""
    from diffusionpolicyoptimization_amd import _lib
    worst, calls = [0.0], 0
    for n in AO.select_lengths(_lib.DPPO_ADV_QUANTILES_BLOCK, _lib.DPPO_ADV_QUANTILES_MAX_CHUNKS):
        adv, kf = AO.select_input(kind, n)
        vals = _segments(adv, kf, 7, 3, 1, n, 1)[0]
        assert vals.size == n
        for q_lo, q_hi in AO.select_quantiles(n):
            got, sel, cnt = _select(cuda, adv, kf, 7, 3, 1, n, 1, q_lo, q_hi)
            assert cnt[0] == n
            _check_segment(f"{kind}-n{n}-q{q_lo}-{q_hi}", vals, q_lo, q_hi, got[0], sel[0], worst)
            calls += 1
    print(json.dumps({"case": f"select-{kind}", "calls": calls, "worst_err_ulps": worst[0], "bound_ulps": 4}))


def test_select_segments_ragged_and_empty(cuda):
    """3 epochs x 3 windows of 300 positions over 500 rows (K' = 2): a full window, a ragged one of 200 and an
    empty one per epoch; every segment against the definition, and bit-equal to a call of the entry that ends
    in that segment alone."""
    adv = np.random.default_rng(3).normal(size=250).astype(np.float32)
    kf, seed, e0, q = 2, 11, 5000, (0.05, 0.95)
    segs = _segments(adv, kf, seed, e0, 3, 300, 3)
    assert [s.size for s in segs] == [300, 200, 0] * 3
    got, sel, cnt = _select(cuda, adv, kf, seed, e0, 3, 300, 3, *q)
    worst = [0.0]
    for m, vals in enumerate(segs):
        assert cnt[m] == vals.size
        _check_segment(f"segment{m}", vals, *q, got[m], sel[m], worst)
        e, b = divmod(m, 3)
        alone, _, _ = _select(cuda, adv, kf, seed, e0 + e, 1, 300, b + 1, *q)
        assert np.array_equal(alone[b], got[m]), (m, alone[b], got[m])
    print(json.dumps({"case": "select-3x3", "worst_err_ulps": worst[0], "bound_ulps": 4}))


def test_select_pass_pair_sums_over_two_halves(cuda):
    """The pass-level pair as a data-parallel caller runs it, in one process: each half of the samples counts
    its own rows, the two count tables are added (torch), both halves pick from the sum. The bounds are
    bit-equal to the single-rank entry on the whole, at two epochs."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    adv = np.random.default_rng(8).normal(size=600).astype(np.float32)
    kf, seed, e0, ne, q = 3, 21, 40, 2, (0.05, 0.95)
    whole, _, cnt = _select(cuda, adv, kf, seed, e0, ne, adv.size * kf, 1, *q)
    assert list(cnt) == [1800, 1800]
    halves = [torch.tensor(adv[:300], device=cuda), torch.tensor(adv[300:], device=cuda)]
    st = [ops.ppo_adv_quantiles_state(ne, 1, cuda) for _ in halves]
    outs = [torch.full((ne, 2), SENTINEL, dtype=torch.float64, device=cuda) for _ in halves]
    for p in range(4):
        for h, (counts, state) in zip(halves, st):
            ops.ppo_adv_quantiles_count(h, 900, kf, seed, e0, ne, 900, 1, p, state, counts)
        total = st[0][0] + st[1][0]
        for (counts, state), out in zip(st, outs):
            counts.copy_(total)
            ops.ppo_adv_quantiles_pick(ne, 1, *q, p, state, counts, out=out)
            assert not counts.any()   # every pick leaves the table zero
    torch.cuda.synchronize()
    for out in outs:
        assert np.array_equal(out.cpu().numpy(), whole), (out, whole)
    for m in range(ne):   # and the whole is the definition on all 1800 rows: every sample three times
        ref = O.bounds(np.repeat(adv, kf), *q)
        assert np.allclose(whole[m], ref, rtol=4 * EPS, atol=0), (whole[m], ref)


def test_select_refusals_leave_outputs_untouched(cuda):
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    adv = torch.zeros(64, device=cuda)
    out = torch.full((1, 2), SENTINEL, dtype=torch.float64, device=cuda)
    ws = ops.ppo_adv_quantiles_workspace(1, 1, cuda)
    bad = [dict(q=(0.5, 0.5)), dict(q=(-0.1, 0.9)), dict(q=(0.1, 1.5)), dict(q=(float("nan"), 0.9)), dict(total=0),
           dict(kf=0), dict(rows_full=0), dict(n_epochs=65)]
    for kw in bad:
        q = kw.get("q", (0.05, 0.95))
        rc = _lib.load().dppo_ppo_adv_quantiles_all(
            _lib.ptr(adv), kw.get("total", 64), kw.get("kf", 1), 1, 0, kw.get("n_epochs", 1), kw.get("rows_full", 64), 1,
            q[0], q[1], _lib.ptr(ws), _lib.ptr(out), _lib.stream_handle(cuda))
        assert rc != 0, kw
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    with pytest.raises(ValueError):
        ops.ppo_adv_quantiles_all(adv, 64, 1, 1, 0, 1, 64, 1, 0.9, 0.1, out, workspace=ws)


# ------------------------------------------------------------------------------------------------
# dppo_ppo_minibatch with DPPO_PPO_ADV_CLIP
# ------------------------------------------------------------------------------------------------
class _Run:
    """A grad_problem on the device: the stride-5 table from the moments of the rows' advantages and the select's
    bounds over them, and one minibatch (whole, or parts) through the row_index."""

    def __init__(self, p, cuda):
        import torch
        from diffusionpolicyoptimization_amd import ops
        from tests.test_update_surface_gpu import _Gpu
        self.p, self.cuda, self.g = p, cuda, _Gpu(p, cuda)
        self.rows = int(p.row_index.size)
        self.row_index = torch.tensor(p.row_index, device=cuda)
        rows_adv = p.adv[p.bi]
        a64 = rows_adv.astype(np.float64)
        self.table = torch.tensor([a64.size, a64.sum(), (a64 * a64).sum(), 0.0, 0.0], dtype=torch.float64, device=cuda)
        b = torch.zeros(1, 2, dtype=torch.float64, device=cuda)
        ops.ppo_adv_quantiles_all(torch.tensor(rows_adv, device=cuda), self.rows, 1, 5, 0, 1, self.rows, 1, *AO.GRAD_Q, b)
        self.table[3:] = b[0]
        self.ws = ops.ppo_workspace(p.d, p.precision, self.rows, cuda)

    def minibatch(self, table, adv_clip, norm_adv, part=None, out=None, fill=0.0):
        import torch
        from diffusionpolicyoptimization_amd import ops
        p, g = self.p, self.g
        if out is None:
            out = (torch.full((g.na + g.nc,), fill, dtype=torch.float32, device=self.cuda),
                   torch.full((16,), fill, dtype=torch.float64, device=self.cuda))
        hp = ops.ppo_hparams(global_rows=self.rows, norm_adv=norm_adv, adv_clip=adv_clip)
        ops.ppo_minibatch(p.d, p.precision, hp, g.packf, g.packc, g.pf, g.tab, g.obs, g.chains, g.lp_old, g.T(p.adv),
                          g.T(p.ret), 0, 0, 0, self.rows, self.ws, out[0], out[1], adv_stats=table,
                          row_index=self.row_index, part=part)
        torch.cuda.synchronize()
        return out


_PROBLEMS = {}   # the CPU halves only: nothing of this module holds device memory between tests


def _run(cuda, precision, rows, norm_adv):
    key = (precision, rows, norm_adv)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = AO.grad_problem(precision, rows, norm_adv)
    return _Run(_PROBLEMS[key], cuda)


@pytest.fixture(autouse=True)
def _leave_no_device_memory():
    """Why this file tidies up after itself: tests/test_diffusion_param_gpu.py::test_record_is_erased_with_the_tensor,
    which runs later in the same process, frees a 640-byte table and needs the caching allocator to hand that very
    block back within 256 allocations. It failed once in a full run when this file kept device tensors alive in a
    module-level cache (small live blocks pin allocator segments, and their free remainders are handed out before
    the freed block). So nothing here outlives its test: the cache holds CPU data only, and agents with reference
    cycles are collected before the next test instead of somewhere inside a later file."""
    yield
    gc.collect()


@pytest.fixture(autouse=True, scope="module")
def _return_cached_blocks():
    """The same reason (_leave_no_device_memory): after the file's last test the blocks it freed go back to the
    driver, so the files that follow find no cached fragments of this one's either."""
    yield
    import torch
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


@pytest.mark.parametrize("label,precision,rows,norm_adv", AO.GRAD_CASES, ids=[c[0] for c in AO.GRAD_CASES])
def test_flagged_minibatch_matches_oracle(cuda, label, precision, rows, norm_adv):
    """Quantiles (0.1, 0.9): the bounds from the device select, the clamp in the actor's row tiles, every
    gradient tensor and metric against O.c_loss(adv_clip_quantiles=(0.1, 0.9))."""
    from tests.test_update_surface_gpu import TOL, _compare
    r = _run(cuda, precision, rows, norm_adv)
    p = r.p
    lo_hi = r.table[3:].cpu().numpy()
    ref_b = O.bounds(p.adv[p.bi], *AO.GRAD_Q)
    assert np.allclose(lo_hi, ref_b, rtol=4 * EPS, atol=0), (lo_hi, ref_b)
    ref = p.oracle(norm_adv=norm_adv, adv_clip_quantiles=AO.GRAD_Q)
    grads, metrics = r.minibatch(r.table, True, norm_adv)
    _compare(f"adv-clip-{label}", r.g, metrics.cpu().numpy(), grads.cpu().numpy(), ref, TOL[precision], denom=rows)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_flagged_parts_equal_the_whole(cuda, precision):
    """Parts 2, 4, 5 (and 2, 1) with the flag against the whole minibatch: the same loss metrics, the gradients
    to the dW's summation order."""
    import torch
    r = _run(cuda, precision, 77, True)
    gw, mw = r.minibatch(r.table, True, True)
    for parts in ((2, 4, 5), (2, 1)):
        out = (torch.zeros_like(gw), torch.zeros_like(mw))
        for part in parts:
            r.minibatch(r.table, True, True, part=part, out=out)
        # metric sums: fp32 per-row terms of order 1 (pg_loss's cancel), summed per tile and over tiles and distinct
        # samples in arrival order: 77 terms at 2^-24 each bound the difference by 77 * 6e-8 < 1e-5
        assert torch.allclose(out[1][:5], mw[:5], rtol=0, atol=1e-5), (parts, out[1][:5], mw[:5])
        err = float((out[0] - gw).abs().max() / gw.abs().max())
        print(json.dumps({"case": f"adv-clip-parts-{precision}-{parts}", "grad_rel": err, "bound": 1e-5}))
        assert err <= 1e-5   # fp32 atomic sums in another arrival order


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("norm_adv", [True, False])
def test_infinite_bounds_give_the_unflagged_bits(cuda, precision, norm_adv):
    """(lo, hi) = (-inf, +inf) with the flag set against the flag unset, through the actor's row tiles (part 4,
    the only kernel that reads the bounds): the metric sums and every byte of the workspace (the images the
    weight-gradient kernels read) are bit-equal. 33 rows are two row tiles, so each metric is a sum of two
    terms and does not depend on their arrival order."""
    import torch
    r = _run(cuda, precision, 33, norm_adv) if norm_adv else _Run(AO.grad_problem(precision, 33, False), cuda)
    inf_table = r.table.clone()
    inf_table[3], inf_table[4] = -np.inf, np.inf
    g0, m0 = r.minibatch(r.table[:3].clone(), False, norm_adv, part=4)
    ws0 = r.ws.clone()
    g1, m1 = r.minibatch(inf_table, True, norm_adv, part=4)
    assert m0[0] != 0 and torch.equal(m1, m0), (m1, m0)
    assert torch.equal(r.ws, ws0) and torch.equal(g0, g1)
    g2, m2 = r.minibatch(r.table, True, norm_adv, part=4)   # and the finite bounds do change them
    assert not torch.equal(m2, m0)


def test_flag_without_a_table_is_refused(cuda):
    """DPPO_PPO_ADV_CLIP with adv_stats NULL, whole and every part: DPPO_EINVAL, sentinel outputs untouched."""
    import torch
    from diffusionpolicyoptimization_amd import _lib
    r = _run(cuda, "fp32", 33, True)
    for part in (None, 1, 2, 4, 5):
        g = torch.full((r.g.na + r.g.nc,), SENTINEL, dtype=torch.float32, device=cuda)
        mt = torch.full((16,), SENTINEL, dtype=torch.float64, device=cuda)
        with pytest.raises(_lib.DppoError, match=r"failed \(1\).*needs adv_stats"):   # 1 = DPPO_EINVAL
            r.minibatch(None, True, True, part=part, out=(g, mt))
        torch.cuda.synchronize()
        assert (g == SENTINEL).all() and (mt == SENTINEL).all()


# (label, precision, dims name, rows: a count, "R64" = the 64-row tile's smallest count 64 (C - 1) + 1, "R32" = one
# round of 32-row tiles plus one row 32 C + 1 (C the CU count), tile rows ops.ppo_plan must report, learn-eta)
TILE_CASES = [("relu-fp16-150", "fp16", "relu", 150, 32, False),
              ("tile64-bf16", "bf16", "relu", "R64", 64, False),
              ("tile32-round-plus-one-bf16", "bf16", "relu", "R32", 32, False),
              ("mish-bf16-150", "bf16", "mish", 150, 32, False),
              ("plain-bf16-150", "bf16", "plain", 150, 32, False),
              ("ddim-learn-eta-fp16-150", "fp16", "ddim", 150, 32, True)]


@pytest.mark.parametrize("label,precision,kind,size,tile,learn_eta", TILE_CASES, ids=[c[0] for c in TILE_CASES])
def test_flagged_minibatch_tiles_actors_and_eta(cuda, monkeypatch, label, precision, kind, size, tile, learn_eta):
    """The flag through the other instantiations of the actor's TRAIN tile, on tests/test_update_regimes_gpu.py's
    _Case (permutation rows from START, ratio 1): fp16; the 64-row, 16-wave tile at its smallest row count and the
    32-row tile one row past a round of C tiles (ops.ppo_plan proves which ran; the bounds reach the epilogue
    through thread ROWS and the tile's own LDS slots); a Mish actor; a plain head; the learnable-eta derivative
    under DDIM (metrics[8], eta 0.6, the unflagged cases' 3e-2). Quantiles (0.1, 0.9) from the device select over
    the rows, metrics and every gradient tensor against the oracle with the same quantiles at the mirrored cases' bounds.

    The two large cases are bf16, as every large-minibatch case of the suite is (tests/test_update_regimes_gpu.py
    runs fp32 up to 1,600 rows): there the oracle rounds where the kernels round, so both sides take the same ReLU
    branches. An fp32 run of the 32 C + 1 = 8,193-row case against the unrounded float64 oracle measured l1_w
    7.9e-3 and l1_b 5.3e-3 (bound 2e-3) with every other tensor at 1e-6: the two tensors that sum dh2 over rows
    whose normalised advantages cancel, where one row on the other side of relu(h2) is 1e-2 of a unit's sum. The
    33- and 77-row fp32 cases above pin the same fp32 instantiation (32 rows, 16 waves) at 1.2e-6."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from tests import test_kernels_gpu as KG
    from tests import test_update_regimes_gpu as UR
    from tests.helpers import HOPPER, HOPPER_DDIM
    dims = dict(relu=HOPPER, ddim=HOPPER_DDIM)
    if kind == "mish":
        from tests.variants import HOPPER_MISH, mish_models
        monkeypatch.setattr(KG, "make_models", mish_models)
        dims["mish"] = HOPPER_MISH
    if kind == "plain":
        from tests.variants import HOPPER_PLAIN
        dims["plain"] = HOPPER_PLAIN
    C = UR._cus(cuda)
    rows = {"R64": 64 * (C - 1) + 1, "R32": 32 * C + 1}.get(size, size)
    case = UR._Case(cuda, precision, dims[kind], max(40, -(-(UR.START + rows) // 10) + 50), eta=0.6 if learn_eta else 1.0)
    plan = ops.ppo_plan(case.d, precision, rows)
    assert plan["actor_tile_rows"] == tile, plan
    stats, mean_std = case.adv_stats(rows)
    bi, _ = case.rows_of(rows)
    rows_adv = case.adv[bi]
    table = torch.zeros(5, dtype=torch.float64, device=cuda)
    table[:3] = stats
    ops.ppo_adv_quantiles_all(case.T(rows_adv), rows, 1, 5, 0, 1, rows, 1, *AO.GRAD_Q, table[3:].view(1, 2))
    lo, hi = O.bounds(rows_adv, *AO.GRAD_Q)
    assert np.allclose(table[3:].cpu().numpy(), (lo, hi), rtol=4 * EPS, atol=0)
    assert (rows_adv < lo).mean() >= 0.05 and (rows_adv > hi).mean() >= 0.05   # the clamp has rows to act on
    met_ref, ga_ref, gc_ref = case.oracle(rows, adv_mean_std=mean_std, eta_grad=learn_eta, adv_clip_quantiles=AO.GRAD_Q)
    hp = ops.ppo_hparams(global_rows=rows, learn_eta=learn_eta, adv_clip=True)
    grads = torch.zeros(case.na + case.nc, dtype=torch.float32, device=cuda)
    met = torch.zeros(16, dtype=torch.float64, device=cuda)
    ops.ppo_minibatch(case.d, precision, hp, case.packf, case.packc, case.pf, case.tab, *case.args, UR.SEED, UR.EPOCH,
                      UR.START, rows, ops.ppo_workspace(case.d, precision, rows, cuda), grads, met, adv_stats=table)
    torch.cuda.synchronize()
    g, m = grads.cpu().numpy().astype(np.float64), met.cpu().numpy()
    assert np.isfinite(g).all()
    tol = UR.TOL[precision]
    UR._check_metrics(m / rows, met_ref, tol, True, f"adv-clip-{label}")
    if learn_eta:
        ref = met_ref["d_eta"]
        print(json.dumps({"case": f"adv-clip-{label}", "d_eta": float(m[8]), "ref": ref, "bound_rel": 3e-2}))
        assert abs(ref) > 1e-3 and abs(m[8] - ref) <= 3e-2 * abs(ref), (m[8], ref)
    UR._check_errs(UR._tensor_errs(case.d, g, ga_ref, gc_ref), tol, f"adv-clip-{label}")


def test_pick_takes_the_global_row_count(cuda):
    """n_global: the pick's rank comes from the caller's count, not from the table. With the true count the
    bounds are the entry's; with a count one too small the upper target moves down one order statistic."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    adv = np.sort(np.random.default_rng(2).normal(size=101).astype(np.float32))
    dev = torch.tensor(adv, device=cuda)

    def run(n_global):
        counts, state = ops.ppo_adv_quantiles_state(1, 1, cuda)
        out = torch.zeros(1, 2, dtype=torch.float64, device=cuda)
        for p in range(4):
            ops.ppo_adv_quantiles_count(dev, 101, 1, 9, 0, 1, 101, 1, p, state, counts)
            ops.ppo_adv_quantiles_pick(1, 1, 0.0, 1.0, p, state, counts, out=out, n_global=n_global)
        torch.cuda.synchronize()
        return out.cpu().numpy()[0]
    assert tuple(run(None)) == tuple(run(torch.tensor([101], device=cuda))) == (adv[0], adv[-1])
    assert tuple(run(torch.tensor([100], device=cuda))) == (adv[0], adv[-2])


def test_pass_pair_refusals(cuda):
    """The pass-level entries refuse a pass outside 0..3, null state / counts, quantiles out of order and a last
    pick without bounds: DPPO_EINVAL, nothing enqueued, the tables and the outputs as they were."""
    import torch
    from diffusionpolicyoptimization_amd import _lib
    lib, P, st = _lib.load(), _lib.ptr, _lib.stream_handle(cuda)
    adv = torch.zeros(64, device=cuda)
    counts = torch.full((1, 4, 256), 3, dtype=torch.int32, device=cuda)
    state = torch.full((1, 9), 5, dtype=torch.int64, device=cuda)
    out = torch.full((1, 2), SENTINEL, dtype=torch.float64, device=cuda)
    count = lambda pass_, s, c: lib.dppo_ppo_adv_quantiles_count(P(adv), 64, 1, 1, 0, 1, 64, 1, pass_, s, c, st)
    pick = lambda pass_, s, c, o, q=(0.05, 0.95): lib.dppo_ppo_adv_quantiles_pick(1, 1, q[0], q[1], pass_, None, s, c, o, st)
    rcs = [count(-1, P(state), P(counts)), count(4, P(state), P(counts)), count(0, None, P(counts)),
           count(0, P(state), None), pick(4, P(state), P(counts), P(out)), pick(0, None, P(counts), P(out)),
           pick(0, P(state), None, P(out)), pick(3, P(state), P(counts), None),
           pick(0, P(state), P(counts), P(out), (0.9, 0.1))]
    torch.cuda.synchronize()
    assert rcs == [1] * len(rcs), rcs   # DPPO_EINVAL
    assert (counts == 3).all() and (state == 5).all() and (out == SENTINEL).all()


# ------------------------------------------------------------------------------------------------
# the agent
# ------------------------------------------------------------------------------------------------
def test_advclip_iterations_match_oracle(cuda, tmp_path, monkeypatch):
    """An eval and two training iterations of the fp32 agent from ft_ppo_diffusion_mlp_advclip.yaml (seed 42, the
    shapes and bounds of tests/test_iteration_gpu.py) against oracle/iteration.py with the model's quantiles."""
    from diffusionpolicyoptimization_amd.util import config
    from tests import test_iteration_gpu as IT
    load = config.load_config
    monkeypatch.setattr(config, "load_config", lambda root, nm, ov: load(root, nm + "_advclip", ov))
    a, orc = IT._agent_and_oracle(42, tmp_path)
    m = a.model
    assert (m.clip_advantage_lower_quantile, m.clip_advantage_upper_quantile) == (0.05, 0.95) and m.adv_clip
    assert orc.closs_kw["adv_clip_quantiles"] == (0.05, 0.95)
    errs = IT._run_and_compare(a, orc, n_itr=3)
    print(json.dumps({"case": "adv-clip-iteration", "iterations": errs}))
    assert [e["eval"] for e in errs] == [True, False, False]
    tab = a._adv_clip.cpu().numpy()
    assert tab.shape == (a.update_epochs * 4, 5) and np.isfinite(tab).all() and (tab[:, 3] < tab[:, 4]).all()


def test_default_quantiles_make_no_new_call(cuda, tmp_path, monkeypatch):
    """Quantiles (0, 1): a training iteration never reaches the new entries (a counting wrapper over the
    library's symbols) and allocates none of their buffers."""
    from diffusionpolicyoptimization_amd import _lib
    from tests import test_iteration_gpu as IT
    a, _ = IT._agent_and_oracle(42, tmp_path)
    assert not a.model.adv_clip
    lib, calls = _lib.load(), []

    class Counting:
        def __getattr__(self, name):
            if "adv_quantiles" in name:
                calls.append(name)
            return getattr(lib, name)
    monkeypatch.setattr(_lib, "_lib", Counting())
    a.iteration(force_train=True)
    assert a.timing["n_updates"] > 0 and calls == []
    assert a._adv_clip is None and a._adv_sel is None and a._adv_all.shape[1] == 3


def test_data_parallel_clip_equals_single_rank_on_the_union(cuda, tmp_path):
    """The rig of tests/test_agent_gpu.py::test_data_parallel_update_equals_single_rank_on_the_union (2 ranks over
    gloo on one GPU, reference batch semantics) from the new cfg, at that test's bounds: both ranks hold one
    table; minibatch 0's bounds are the quantiles of the union of the two ranks' rows; the all-reduced gradient
    and metric sums equal ONE rank's flagged minibatch over that union with its own moments and select."""
    import socket
    import subprocess
    import sys

    import torch

    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from dp_equiv import OVERRIDES
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, DPPO_DIST_BACKEND="gloo", DPPO_SINGLE_DEVICE="1", DPPO_EQUIV_DIR=str(tmp_path))
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port),
                          os.path.join(ROOT, "tests", "adv_clip_dp_worker.py")], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    r = [dict(np.load(tmp_path / f"rank{i}.npz")) for i in range(2)]
    assert int(r[0]["world"]) == 2 and int(r[0]["rows"]) == 200
    np.testing.assert_array_equal(r[0]["clip"], r[1]["clip"])          # one table on both ranks
    np.testing.assert_array_equal(r[0]["grads"], r[1]["grads"])
    assert (r[0]["clip"][:, 0] == 400).all() and (r[0]["clip"][:, 3] < r[0]["clip"][:, 4]).all()

    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp_advclip",
                      OVERRIDES + [f"logdir={tmp_path}/single"])
    a = get_class(cfg._target_)(cfg)
    m = a.model
    np.testing.assert_array_equal(m.train_params.cpu().numpy(), r[0]["params"])
    got = {}

    end = [dict(np.load(tmp_path / f"rank{i}_end.npz")) for i in range(2)]
    np.testing.assert_array_equal(end[0]["params"], end[1]["params"])   # replicas after the whole update
    np.testing.assert_array_equal(end[0]["clip"], end[1]["clip"])

    def hook(epoch, batch, start, rows):
        """At the first minibatch (nothing stepped yet) the single rank runs the WHOLE update the two ranks ran:
        per (epoch, batch) one flagged minibatch over the union of the ranks' rows, with its own moments and
        its own select over those rows, and one optimizer step over [actor | critic]."""
        if (epoch, batch) != (0, 0):
            return
        S, E, kf = a.n_steps, a.n_envs, m.ft_denoising_steps
        El, rows_l = int(r[0]["n_envs"]), int(r[0]["rows"])
        adv = np.concatenate([r[0]["adv"], r[1]["adv"]], axis=1)
        np.testing.assert_allclose(adv, a.adv.cpu().numpy(), rtol=0, atol=1e-5 * np.abs(adv).max())
        N = S * E
        adv_flat = a.adv.view(-1)
        opt, ng = a.actor_optimizer, m.grads.numel()
        packs = {"actor": (m.actor_ft_params, m.packed_ft), "critic": (m.critic_params, m.packed_critic)}
        n_batch = (S * El * kf) // rows_l
        tabs = []
        for e in range(a.update_epochs):
            for b in range(n_batch):
                idx = []   # the union of the ranks' rows in the single rank's sample numbering
                for i in range(2):
                    loc = ops.feistel_permute(b * rows_l, rows_l, S * El * kf, int(r[i]["perm_seed"]),
                                              int(r[i]["epoch"]) + e, a.device).cpu().numpy()
                    n_loc, j = loc // kf, loc % kf
                    idx.append(((n_loc // El) * E + i * El + n_loc % El) * kf + j)
                idx = torch.tensor(np.concatenate(idx), device=a.device)
                n = idx.numel()
                rows_adv = adv_flat[idx // kf].contiguous()
                tab = torch.zeros(5, dtype=torch.float64, device=a.device)
                ops.ppo_adv_stats(adv_flat, N * kf, kf, 0, 0, 0, n, tab[:3], row_index=idx)
                ops.ppo_adv_quantiles_all(rows_adv, n, 1, 0, 0, 1, n, 1, 0.05, 0.95, tab[3:].view(1, 2))
                m.minibatch(a.obs_traj.view(N, -1), a.chains_traj.view(N, kf + 1, -1), a.lp_old, adv_flat,
                            a.ret.view(-1), 0, 0, 0, n, global_rows=a.batch_size, row_index=idx, adv_stats=tab)
                torch.cuda.synchronize()
                if (e, b) == (0, 0):
                    got.update(grads=m.grads.cpu().numpy().copy(), metrics=m.metrics[:5].cpu().numpy().copy(),
                               tab=tab.cpu().numpy(), ref=O.bounds(rows_adv.cpu().numpy(), 0.05, 0.95))
                tabs.append(tab.cpu().numpy())
                opt.apply_range(m.grads, 0, ng, opt.begin_step(), m.dims, m.precision, packs=packs)
        torch.cuda.synchronize()
        got.update(tabs=np.stack(tabs), params=m.train_params.cpu().numpy().copy(), steps=opt.iterations)
        raise StopIteration
    a.minibatch_hook = hook
    p0 = m.train_params.cpu().numpy().astype(np.float64)
    with pytest.raises(StopIteration):
        a.iteration(force_train=True)
    scale = np.abs(a.adv.cpu().numpy()).max()
    print(json.dumps({"case": "adv-clip-dp", "dp_bounds": r[0]["clip"][0, 3:].tolist(), "single_bounds": got["tab"][3:].tolist()}))
    assert np.allclose(got["tab"][3:], got["ref"], rtol=4 * EPS, atol=0)
    # every minibatch's bounds; the moments: 400 advantages, each within 1e-5 scale of the single rank's
    assert got["tabs"].shape == end[0]["clip"].shape and got["steps"] == int(end[0]["steps"]) == len(got["tabs"])
    np.testing.assert_allclose(end[0]["clip"][:, 3:], got["tabs"][:, 3:], rtol=0, atol=1e-5 * scale)
    np.testing.assert_allclose(end[0]["clip"][:, :3], got["tabs"][:, :3], rtol=0, atol=400 * 2e-5 * scale * max(1.0, scale))
    g1, g2 = got["grads"], r[0]["grads"]
    err = np.abs(g1 - g2).max() / np.abs(g1).max()
    assert err < 1e-4, err
    np.testing.assert_allclose(got["metrics"], r[0]["metrics"], rtol=1e-4, atol=1e-7)
    # The parameters after the update (10 AdamW steps of lr 1e-4). Both sides are fp32 runs of the same kernels on
    # advantages 1e-5 apart and gradients 1e-4 apart in another summation order, the situation of the fp32 agent
    # against the oracle in tests/test_iteration_gpu.py, whose bounds on the update's parameter change these are
    # (Adam turns gradient elements near zero into +-lr steps on both sides: distribution tight, maximum loose)
    dg, dr = got["params"].astype(np.float64) - p0, end[0]["params"].astype(np.float64) - p0
    diff, sc = np.abs(dg - dr), np.abs(dr).max()
    fig = dict(median=float(np.median(diff) / sc), p99=float(np.quantile(diff, 0.99) / sc), max=float(diff.max() / sc),
               l2=float(np.linalg.norm(dg - dr) / np.linalg.norm(dr)))
    print(json.dumps({"case": "adv-clip-dp-params", **fig, "bounds": dict(median=1e-4, p99=1e-3, max=0.1, l2=5e-3)}))
    assert dr.any() and fig["median"] <= 1e-4 and fig["p99"] <= 1e-3 and fig["l2"] <= 5e-3 and fig["max"] <= 0.1, fig
