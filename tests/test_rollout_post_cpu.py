"""CPU half of the rollout post-processing suite (tests/test_rollout_post_gpu.py): on the GPU cases' own
inputs, (1) a NumPy emulation of the wave scans (per-lane chunk fold, the 6-step shuffle composition with the
kernels' `has` rule, the replay, empty trailing lanes) stays under half of every bound, so a correct kernel
reaches them; (2) fifteen mistakes, applied to the emulations or to the references, each move a compared
quantity of a listed case past ten times its bound, so the inputs bite; (3) the case tables hold what their
comments claim, from host arithmetic. Nothing here calls the library.

GAE stores float32: the bound's first term is exactly that one rounding, which a correct kernel may use up
(the emulation's stored values reach 0.99 of it), so the emulation is held to half of the bound's OTHER term,
the float64 reassociation slack, before the store, and to the whole bound after it. That asks more than half
of the bound."""
import json

import numpy as np
import pytest

from oracle import dppo_oracle as O
from oracle import philox as PX
from tests import rollout_post_cases as C


def _log(name, q, err, bound):
    print(json.dumps({"case": name, "err": err, "bound": bound, "ratio": q}))


# ------------------------------------------------------------------------------------------------
# the case tables, from host arithmetic
# ------------------------------------------------------------------------------------------------
def test_scan_table_geometry():
    """every S named for the scans has the CH, the count of lanes that hold a step and the last lane's chunk
    length SCAN_TABLE claims; the S lists step CH at 64 / 65 and 128 / 129, leave trailing lanes empty and
    give a lane a short chunk"""
    for S, (CH, lanes, last) in C.SCAN_TABLE.items():
        steps = [min(S, (l + 1) * CH) - min(S, l * CH) for l in range(64)]
        assert -(-S // 64) == CH and sum(steps) == S
        assert sum(1 for s in steps if s) == lanes and steps[lanes - 1] == last, S
        assert C.scan_geometry(S) == (CH, lanes, last)
    gae_S, scale_S = {s for s, _ in C.GAE_SIZES}, {s for s, _ in C.SCALE_SIZES}
    assert gae_S == {1, 2, 63, 64, 65, 127, 128, 129, 130, 193} and scale_S == {1, 63, 64, 65, 128, 129, 193}
    assert {e for s, e in C.GAE_SIZES if s > 64} == {1, 3, 4, 5, 9}
    assert [(e - 1) % 4 + 1 for e in (1, 3, 4, 5, 9)] == [1, 3, 4, 1, 1]          # live waves of the last workgroup
    assert {e for _, e in C.SCALE_SIZES} == {1, 3, 5, 64, 65, 130}
    for S in gae_S | scale_S | {257, 300}:
        assert S in C.SCAN_TABLE
    assert any(C.SCAN_TABLE[S][1] < 64 and 1 <= C.SCAN_TABLE[S][2] < C.SCAN_TABLE[S][0] for S in gae_S)
    for E, calls in C.PER_ENV_CASES.values():       # the broadcast rule the oracle applies
        L = E
        for S in calls:
            assert S == L or S == 1 or L == 1
            L = max(S, L)
    assert -(-257 // 256) == 2 and -(-300 // 256) == 2      # col_moments / rms_cols_update: a second workgroup


@pytest.mark.parametrize("S", sorted({s for s, _ in C.GAE_SIZES}))
def test_flag_patterns_sit_on_the_chunk_edges(S):
    CH, lanes, _ = C.SCAN_TABLE[S]
    rng = np.random.default_rng(0)
    f = {p: C.flags(p, S, 2, rng)[:, 0] for p in C.PATTERNS}
    assert f["none"].sum() == 0 and f["all"].sum() == S
    assert list(np.flatnonzero(f["chunk_first"])) == [l * CH for l in range(lanes)]
    assert list(np.flatnonzero(f["chunk_last"])) == [min(S, (l + 1) * CH) - 1 for l in range(lanes)]
    assert list(np.flatnonzero(f["last_only"])) == [S - 1] and list(np.flatnonzero(f["first_only"])) == [0]


def test_episode_layouts_count_what_they_were_designed_for():
    """per env, the layout's designed episode count == the per-env reference's; every layout and every reward
    kind is used; an all-negative column and best rewards exactly on the threshold exist"""
    used, on_threshold = set(), 0
    assert {s for s, _ in C.EP_SIZES} == {1, 30, 31, 32, 33, 63, 64, 65, 97}
    assert {e for _, e in C.EP_SIZES} == {1, 63, 64, 65, 129}
    for S, E in C.EP_SIZES:
        for kind in C.EP_REWARDS:
            firsts, rew, names = C.ep_inputs(S, E, kind)
            thr = C.ep_threshold(kind)
            ref = C.episode_rows_ref(firsts, rew, C.EP_ACT_STEPS, thr)
            for e, name in enumerate(names):
                assert ref[e, 0] == C.ep_designed_count(name, S, firsts[:, e]), (S, E, kind, e, name)
                if ref[e, 0]:
                    used.add(name)
            if kind == "negative":
                assert rew.max() < 0
            if kind == "integer":
                bests = []
                C.emu_episode_rows(firsts, rew, C.EP_ACT_STEPS, thr, bests=bests)
                on_threshold += sum(1 for b in bests if b == thr)
                assert any(b < thr for b in bests) or len(bests) < 4
            assert np.array_equal(C.emu_episode_rows(firsts, rew, C.EP_ACT_STEPS, thr)[:, [0, 3]], ref[:, [0, 3]])
    assert used == {"ends", "ends_plus", "x30_32", "x31_33", "random"}      # the others are designed to count none
    assert on_threshold >= 20
    for name in ("none", "single", "every", "x31_32"):
        assert any(name in C.ep_layout_of(S, E, k) for S, E in C.EP_SIZES for k in C.EP_REWARDS)


def test_feistel_table_steps_at_powers_of_four():
    for n, hb in C.FEISTEL_N.items():
        assert 4 ** hb >= n and (hb == 1 or 4 ** (hb - 1) < n), n
    for k in (2, 4, 6, 8):      # n = 4^k: no cycle walking; n = 4^k + 1: half_bits steps, 3/4 of the domain walks
        assert C.FEISTEL_N[4 ** k] == k and C.FEISTEL_N[4 ** k + 1] == k + 1
        assert 1 - (4 ** k + 1) / 4 ** (k + 1) > 0.73
    assert all(s >= 1 << 32 for s in C.FEISTEL_SEEDS)
    for n in C.FEISTEL_WINDOW_N:
        full = PX.feistel_permute(np.arange(n), n, C.FEISTEL_SEEDS[0], 1)
        assert np.array_equal(np.sort(full), np.arange(n))
        for first, count in C.feistel_windows(n):
            assert first + count <= n and (first, count) != (0, n)
    assert any(f <= 256 < f + c for f, c in C.feistel_windows(257))
    a, b = (PX.feistel_permute(np.arange(257), 257, C.FEISTEL_SEEDS[0], ep) for ep in (0, 1))
    assert not np.array_equal(a, b)


def test_adv_tables_take_the_second_trip():
    N, kf, start, rows = C.ADV_SECOND_TRIP
    assert rows == 512 * 256 + 1 and start + rows <= N * kf
    N, kf, rows_full, n_batch, n_ep = C.ADV_ALL_CASES[-1]
    assert rows_full == 64 * 256 + 1 and n_ep == 3 and 0 < N * kf - (n_batch - 1) * rows_full < rows_full
    assert {(n, k) for n, k, _ in C.ADV_CASES} == {(1, 1), (97, 10), (64, 4), (1025, 17)}
    for N, kf, windows in C.ADV_CASES:
        assert all(s + r <= N * kf for s, r in windows) and any(r == 0 for s, r in windows) or N == 1025
        assert any(s + r == N * kf and 0 < r for s, r in windows)
    ri = C.adv_row_index(970, 300)
    assert (ri == -1).sum() > 5 and (ri == 970).sum() > 5 and (ri == ri[0]).sum() > 10


def test_value_moment_sizes_and_ev_bound():
    """sizes on both sides of the 64-lane and the 1024-thread edge; the explained-variance case's bound is finite
    only without the moments' 1e-12 floor, which allows the whole of Var(y) (it is 1e-12 of sum y^2 / n)"""
    assert set(C.VM_SIZES) == {1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097}
    val, ret = C.vm_inputs(C.VM_EV_N, ev_case=True)
    assert abs(ret.mean() - 1e4) < 1 and 2e-3 < ret.astype(np.float64).std() < 5e-2
    ref, with_floor = C.vm_ref(val, ret)
    _, a_priori = C.vm_ref(val, ret, floor=0.0)
    assert np.isinf(C.ev_bound(ref, with_floor))
    b = C.ev_bound(ref, a_priori)
    ev = O.explained_variance(val.astype(np.float64), ret.astype(np.float64))
    _log("value_moments-ev-reference", abs(C.ev_from_moments(ref) - ev) / b, abs(C.ev_from_moments(ref) - ev), b)
    assert np.isfinite(b) and b < 0.5 and abs(C.ev_from_moments(ref) - ev) <= b
    worst = ref.copy()      # the bound holds for moments at the edge of theirs
    worst[1] += a_priori[1]
    worst[3] -= a_priori[3]
    assert abs(C.ev_from_moments(worst) - ev) <= b


def test_oracle_rets_helper_is_the_oracles_recurrence():
    """every column of oracle_rets == the oracle's own carried state after a call on that prefix"""
    r, first = C.scale_inputs(65, 5, "random", 0)
    prev = np.random.default_rng(1).normal(size=5)
    rets = C.oracle_rets(prev, r.T, first.T.astype(np.float64), 0.99)
    for t in (0, 1, 31, 64):
        orc = O.RunningRewardScalerOracle(5)
        orc.ret = prev
        orc(r.T[:, :t + 1], first.T[:, :t + 1].astype(np.float64))
        assert np.array_equal(orc.ret, rets[:, t])


# ------------------------------------------------------------------------------------------------
# the emulation under half of every bound, on the GPU cases' inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,E", C.GAE_SIZES)
def test_gae_emulation_within_half_the_slack(S, E):
    knobs = [(0.99, 0.95)] + (C.GAE_KNOBS if S == 129 else [])
    for pattern in C.PATTERNS:
        for gamma, lam in knobs:
            inp = C.gae_inputs(S, E, pattern)
            refs = C.gae_ref(inp, gamma, lam)
            for name, emu, ref in zip(("adv", "ret"), C.emu_gae(inp, gamma, lam), refs):
                q, err, b = C.ratio(emu, ref, C.gae_slack(ref))
                qs, _, _ = C.ratio(emu.astype(np.float32), ref, C.gae_bound(ref))
                _log(f"gae-emu-{S}x{E}-{pattern}-{gamma}-{lam}-{name}", q, err, b)
                assert q <= 0.5 and qs <= 1.0, (pattern, name, q, qs)


def _scale_calls(S, E, pattern, knobs=None, mean=0.5, **mistakes):
    """-> per call (emulation, reference)"""
    knobs = knobs or {}
    ref, state, out = C.ScaleRef(E, **knobs), C.scale_state(E), []
    for call in range(C.N_CALLS):
        r, first = C.scale_inputs(S, E, pattern, call, mean)
        out.append((C.emu_scale_call(state, r, first, **knobs, **mistakes), ref(r, first)))
    return out


def _scale_worst(calls):
    return max(C.ratio(emu[k], ref[k], C.scale_bound(ref[k], k))[0] for emu, ref in calls for k in C.SCALE_FIELDS)


@pytest.mark.parametrize("S,E", C.SCALE_SIZES)
def test_scaler_emulation_within_half_the_bound(S, E):
    for pattern in C.SCALE_PATTERNS:
        q = _scale_worst(_scale_calls(S, E, pattern))
        _log(f"scale-emu-{S}x{E}-{pattern}", q, q, 1.0)
        assert q <= 0.5, (pattern, q)


@pytest.mark.parametrize("knob", sorted(C.SCALE_KNOBS))
def test_scaler_knob_moves_the_oracle_and_emulation_follows(knob):
    calls = _scale_calls(65, 5, "random", C.SCALE_KNOBS[knob], mean=0.0)
    default = _scale_calls(65, 5, "random", mean=0.0)
    moved = max(C.ratio(d[1][k], c[1][k], C.scale_bound(c[1][k], k))[0] for c, d in zip(calls, default) for k in C.SCALE_FIELDS)
    assert moved >= 10 and _scale_worst(calls) <= 0.5, (moved, _scale_worst(calls))
    if knob == "cliprew":
        for _, ref in calls:
            assert (ref["out"] == 0.5).mean() >= 0.1 and (ref["out"] == -0.5).mean() >= 0.1


# ------------------------------------------------------------------------------------------------
# the mistakes: each moves a compared quantity of a listed case past ten times its bound
# ------------------------------------------------------------------------------------------------
def _gae_moved(S, E, pattern, **mistake):
    inp = C.gae_inputs(S, E, pattern)
    return max(C.ratio(np.asarray(emu, np.float32), ref, C.gae_bound(ref))[0]
               for emu, ref in zip(C.emu_gae(inp, **mistake), C.gae_ref(inp)))


GAE_MISTAKES = {"carry dropped across a lane boundary at S = 65": (65, 1, "none", dict(drop_carry=True)),
                "values[t + 1] for last_values at t = S - 1": (129, 5, "none", dict(next_value_wrong=True)),
                "nonterm left off the gamma lam factor": (129, 5, "chunk_last", dict(c_without_nonterm=True))}
SCALE_MISTAKES = {"first ignored on a chunk's first step": (65, 65, "chunk_first", dict(ignore_first_on_chunk_start=True)),
                  "ret_state not carried between calls": (63, 5, "none", dict(no_ret_carry=True)),
                  "M2 divided by tot": (64, 64, "random", dict(m2_div_tot=True)),
                  "env moments merged over the first 64 envs": (65, 65, "random", dict(first64_only=True))}


@pytest.mark.parametrize("name", sorted(GAE_MISTAKES))
def test_gae_mistake_is_caught(name):
    S, E, pattern, mistake = GAE_MISTAKES[name]
    assert (S, E) in C.GAE_SIZES
    q = _gae_moved(S, E, pattern, **mistake)
    _log(name, q, q, 1.0)
    assert q >= 10


def test_gae_last_values_masked_only_by_the_last_flag():
    """last_only: the reference must not see last_values at all; first_only: it must"""
    for pattern, seen in (("last_only", False), ("none", True)):
        inp = C.gae_inputs(129, 5, pattern)
        other = dict(inp, lv=inp["lv"] + 1)
        assert (not np.array_equal(C.gae_ref(inp)[0], C.gae_ref(other)[0])) == seen


@pytest.mark.parametrize("name", sorted(SCALE_MISTAKES))
def test_scaler_mistake_is_caught(name):
    S, E, pattern, mistake = SCALE_MISTAKES[name]
    assert (S, E) in C.SCALE_SIZES
    q = _scale_worst(_scale_calls(S, E, pattern, **mistake))
    _log(name, q, q, 1.0)
    assert q >= 10


def test_scaler_carry_pattern_needs_the_carried_ret_per_env():
    """the `carry` sequences: dropping ret_state moves exactly the envs whose first[0] is 0 on calls 2 and 3"""
    good, bad = _scale_calls(129, 130, "carry"), _scale_calls(129, 130, "carry", no_ret_carry=True)
    _, first = C.scale_inputs(129, 130, "carry", 1)
    assert set(first[0]) == {0, 1}
    assert _scale_worst(bad) >= 10 and _scale_worst(good) <= 0.5


EP_MISTAKES = {"a length-1 episode counted": dict(count_len1=True),
               "an episode that spans t = 31 / 32 dropped": dict(drop_chunk_span=True),
               "the flag row t = S ignored": dict(ignore_last_row=True),
               "the running maximum started at 0": dict(max_from_zero=True),
               "> in place of >= at the threshold": dict(strict_threshold=True)}


@pytest.mark.parametrize("name", sorted(EP_MISTAKES))
def test_episode_mistake_is_caught(name):
    """over the GPU cases: a count or a success count differs, or a sum is ten bounds off, in some env"""
    worst, hit_on_edge = 0.0, False
    for S, E in C.EP_SIZES:
        for kind in C.EP_REWARDS:
            firsts, rew, names = C.ep_inputs(S, E, kind)
            thr = C.ep_threshold(kind)
            ref = C.episode_rows_ref(firsts, rew, C.EP_ACT_STEPS, thr)
            good = C.emu_episode_rows(firsts, rew, C.EP_ACT_STEPS, thr)
            assert np.array_equal(good[:, [0, 3]], ref[:, [0, 3]])
            assert C.ratio(good[:, 1:3], ref[:, 1:3], C.ep_bound(rew)[:, None])[0] <= 0.5
            bad = C.emu_episode_rows(firsts, rew, C.EP_ACT_STEPS, thr, **EP_MISTAKES[name])
            exact = not np.array_equal(bad[:, [0, 3]], ref[:, [0, 3]])
            worst = max(worst, np.inf if exact else 0.0, C.ratio(bad[:, 1:3], ref[:, 1:3], C.ep_bound(rew)[:, None])[0])
            for e, layout in enumerate(names):
                if layout in ("x30_32", "x31_33") and not np.array_equal(bad[e], ref[e]):
                    hit_on_edge = True
    assert worst >= 10
    if "31 / 32" in name:
        assert hit_on_edge


ADV_MISTAKES = {"idx % kf in place of idx // kf": dict(mod_kf=True),
                "the invalid row_index entries counted": dict(count_invalid=True),
                "a grid-stride sum stopped after its first trip": dict(trip=512 * 256)}


def _adv_moved(ref, bad, bound):
    q = C.ratio(bad[1:], ref[1:], bound[1:])[0]
    return np.inf if bad[0] != ref[0] else q


@pytest.mark.parametrize("name", sorted(ADV_MISTAKES))
def test_adv_stats_mistake_is_caught(name):
    mistake = ADV_MISTAKES[name]
    if "trip" in mistake:
        N, kf, start, rows = C.ADV_SECOND_TRIP
        args = (C.adv_values(N), N * kf, kf, C.ADV_SEED, C.ADV_EPOCH, start, rows)
        ref, bound = C.adv_ref(*args)
        assert _adv_moved(ref, C.adv_ref(*args, **mistake)[0], bound) >= 10
        N, kf, rows_full, n_batch, n_ep = C.ADV_ALL_CASES[-1]
        args = (C.adv_values(N), N * kf, kf, C.ADV_SEED, C.ADV_EPOCH, n_ep, rows_full, n_batch)
        ref, bound = C.adv_all_ref(*args)
        bad = C.adv_all_ref(*args, trip=64 * 256)[0]
        assert sum(_adv_moved(r, b, bd) >= 10 for r, b, bd in zip(ref, bad, bound)) == 2 * n_ep     # the full minibatches
    elif "mod_kf" in mistake:
        N, kf, windows = C.ADV_CASES[1]
        for start, rows in windows:
            args = (C.adv_values(N), N * kf, kf, C.ADV_SEED, C.ADV_EPOCH, start, rows)
            ref, bound = C.adv_ref(*args)
            assert rows == 0 or C.ratio(C.adv_ref(*args, **mistake)[0][1:], ref[1:], bound[1:])[0] >= 10
    else:
        N, kf = 97, 10
        ri = C.adv_row_index(N * kf, 300)
        args = (C.adv_values(N), N * kf, kf, C.ADV_SEED, C.ADV_EPOCH, 10, 280, ri)
        ref, _ = C.adv_ref(*args)
        assert ref[0] < 280 and C.adv_ref(*args, **mistake)[0][0] == 280
