"""The kernels between the rollout and the update against the float64 oracle at their edges: dppo_gae,
dppo_reward_scale (and its _moments / _apply / _per_env forms), dppo_episode_sums, dppo_value_moments
(csrc/scan.hip), dppo_ppo_adv_stats, dppo_ppo_adv_stats_all and dppo_feistel_permute (csrc/update.hip).
Cases, references and bounds are in tests/rollout_post_cases.py; tests/test_rollout_post_cpu.py shows that a
correct kernel reaches the bounds and that the inputs catch fifteen mistakes. Every case prints one JSON line
{kernel, case, err, bound, ratio}: the error and the bound where err / bound is largest."""
import json

import numpy as np
import pytest

from oracle import dppo_oracle as O
from oracle import philox as PX
from tests import rollout_post_cases as C

pytestmark = pytest.mark.gpu
SENTINEL = -777.25


def _log(kernel, case, q, err, bound):
    print(json.dumps({"kernel": kernel, "case": case, "err": err, "bound": bound, "ratio": q}))


def _check(kernel, case, got, ref, bound):
    q, err, b = C.ratio(got, ref, bound)
    _log(kernel, case, q, err, b)
    assert q <= 1.0, (kernel, case, q, err, b)
    return q


def _dev(x, cuda):
    import torch
    return torch.tensor(np.ascontiguousarray(x), device=cuda)


# ------------------------------------------------------------------------------------------------
# 1. dppo_gae
# ------------------------------------------------------------------------------------------------
def _run_gae(cuda, inp, **kw):
    import torch
    from diffusionpolicyoptimization_amd import ops
    a, r = ops.gae(_dev(inp["r"], cuda), _dev(inp["v"], cuda), _dev(inp["lv"], cuda), _dev(inp["term"], cuda), **kw)
    torch.cuda.synchronize()
    return a.cpu().numpy(), r.cpu().numpy()


@pytest.mark.parametrize("pattern", C.PATTERNS)
@pytest.mark.parametrize("S,E", C.GAE_SIZES)
def test_gae(cuda, S, E, pattern):
    """per element within the one float32 rounding of the store + 1e-12 (1 + max |ref|) of O.gae, advantages and
    returns, with terminations on the first / last step of every lane chunk, on S - 1 alone (last_values
    masked), on 0 alone, everywhere, nowhere and at random"""
    inp = C.gae_inputs(S, E, pattern)
    for name, got, ref in zip(("adv", "ret"), _run_gae(cuda, inp), C.gae_ref(inp)):
        _check("dppo_gae", f"{S}x{E}-{pattern}-{name}", got, ref, C.gae_bound(ref))


@pytest.mark.parametrize("gamma,lam", C.GAE_KNOBS)
def test_gae_knobs(cuda, gamma, lam):
    inp = C.gae_inputs(129, 5, "random")
    refs, default = C.gae_ref(inp, gamma, lam), C.gae_ref(inp)
    assert C.ratio(default[0], refs[0], C.gae_bound(refs[0]))[0] >= 10       # the oracle moved
    for name, got, ref in zip(("adv", "ret"), _run_gae(cuda, inp, gamma=gamma, lam=lam), refs):
        _check("dppo_gae", f"129x5-random-{gamma}-{lam}-{name}", got, ref, C.gae_bound(ref))


@pytest.mark.parametrize("S,E", [(0, 3), (5, 0)])
def test_gae_empty_touches_nothing(cuda, S, E):
    import torch
    from diffusionpolicyoptimization_amd import ops
    adv = torch.full((4, 4), SENTINEL, dtype=torch.float32, device=cuda)
    ret = torch.full((4, 4), SENTINEL, dtype=torch.float32, device=cuda)
    ops.gae(torch.zeros(S, E, dtype=torch.float64, device=cuda), torch.zeros(S, E, dtype=torch.float32, device=cuda),
            torch.zeros(E, dtype=torch.float32, device=cuda), torch.zeros(S, E, dtype=torch.uint8, device=cuda),
            adv=adv, ret=ret)
    torch.cuda.synchronize()
    assert bool((adv == SENTINEL).all()) and bool((ret == SENTINEL).all())
    _log("dppo_gae", f"empty-{S}x{E}", 0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------
# 2. the reward scaler, scalar state
# ------------------------------------------------------------------------------------------------
def _scale_calls(cuda, path, S, E, pattern, knobs=None, mean=0.5):
    """three consecutive calls with the state carried -> the worst ratio; path `fused` = dppo_reward_scale,
    `moments` = dppo_reward_scale_moments + the host merge of util/reward_scaling.py + dppo_reward_scale_apply"""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util import dist as dist_util
    knobs = knobs or {}
    gamma, cliprew, eps = knobs.get("gamma", 0.99), knobs.get("cliprew", 10.0), knobs.get("epsilon", 1e-8)
    orc = C.ScaleRef(E, **knobs)
    ret = torch.zeros(E, dtype=torch.float64, device=cuda)
    rms = torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64, device=cuda)
    ws = ops.reward_scale_workspace(S, E, cuda)
    worst, refs = 0.0, []
    for call in range(C.N_CALLS):
        r, first = C.scale_inputs(S, E, pattern, call, mean)
        ref = orc(r, first)
        rt, ft = _dev(r, cuda), _dev(first, cuda)
        got = {}
        if path == "fused":
            ops.reward_scale(rt, ft, ret, rms, ws, gamma, cliprew, eps)
        else:
            mom = torch.full((3,), SENTINEL, dtype=torch.float64, device=cuda)
            ops.reward_scale_moments(rt, ft, ret, mom, ws, gamma)
            n, m, m2 = dist_util.gather_moments(mom)
            rms.copy_(torch.tensor(dist_util.rms_update(rms.cpu().tolist(), n, m, m2), dtype=torch.float64))
            ops.reward_scale_apply(rt, rms, cliprew, eps)
            got["moments"] = mom.cpu().numpy()
        torch.cuda.synchronize()
        got.update(out=rt.cpu().numpy(), ret=ret.cpu().numpy(), rms=rms.cpu().numpy())
        for k, g in got.items():
            worst = max(worst, _check(f"dppo_reward_scale[{path}]", f"{S}x{E}-{pattern}-call{call}-{k}", g, ref[k],
                                      C.scale_bound(ref[k], k)))
        refs.append(ref)
    return worst, refs


@pytest.mark.parametrize("pattern", C.SCALE_PATTERNS)
@pytest.mark.parametrize("S,E", C.SCALE_SIZES)
@pytest.mark.parametrize("path", ["fused", "moments"])
def test_reward_scale(cuda, path, S, E, pattern):
    """the scaled reward, ret_state, {mean, var, count} (and {n, mean, M2} on the moments path) after each of
    three calls, at the goldens' rtol 1e-12 with atol 1e-12 max(1, max |ref|)"""
    _scale_calls(cuda, path, S, E, pattern)


@pytest.mark.parametrize("knob", sorted(C.SCALE_KNOBS))
@pytest.mark.parametrize("path", ["fused", "moments"])
def test_reward_scale_knobs(cuda, path, knob):
    S, E = 65, 5
    default = C.ScaleRef(E)
    moved = 0.0
    refs = []
    knobbed = C.ScaleRef(E, **C.SCALE_KNOBS[knob])
    for call in range(C.N_CALLS):
        r, first = C.scale_inputs(S, E, "random", call, 0.0)
        a, b = knobbed(r, first), default(r, first)
        refs.append(a)
        moved = max([moved] + [C.ratio(b[k], a[k], C.scale_bound(a[k], k))[0] for k in C.SCALE_FIELDS])
    assert moved >= 10                                                      # the oracle moved
    if knob == "cliprew":
        for ref in refs:                                                    # and really clips, at both signs
            assert (ref["out"] == 0.5).mean() >= 0.1 and (ref["out"] == -0.5).mean() >= 0.1
    _scale_calls(cuda, path, S, E, "random", C.SCALE_KNOBS[knob], mean=0.0)


# ------------------------------------------------------------------------------------------------
# 3. the reward scaler, per_env = True
# ------------------------------------------------------------------------------------------------
def _per_env_inputs(name, E, S, call):
    rng = np.random.default_rng([13, E, S, call, len(name)])
    return rng.normal(0.5, 2.0, size=(S, E)), (rng.random((S, E)) < 0.3).astype(np.uint8)


def _check_per_env(name, call, ref, out, ret, mean, var, count):
    got = dict(out=out, ret=ret, mean=mean, var=var, count=np.float64(count))
    for k, g in got.items():
        r = np.asarray(ref[k], np.float64)
        assert np.shape(g) == r.shape, (k, np.shape(g), r.shape)
        _check("dppo_reward_scale_per_env", f"{name}-call{call}-{k}", g, r, C.scale_bound(r))


@pytest.mark.parametrize("entry", ["raw", "RunningRewardScaler"])
@pytest.mark.parametrize("name", sorted(C.PER_ENV_CASES))
def test_reward_scale_per_env(cuda, name, entry):
    """S == E; E = 1 with S past one workgroup of col_moments_kernel / rms_cols_update_kernel; S = 1 (the output
    broadcasts to [L, E]) followed by S = L"""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util.reward_scaling import RunningRewardScaler
    E, calls = C.PER_ENV_CASES[name]
    orc = C.ScaleRef(E, per_env=True)
    if entry == "raw":
        cap = max(calls + [E])
        L = E
        rin = torch.zeros(1 + 2 * cap, dtype=torch.float64, device=cuda)
        rin[0] = 1e-4
        rin[1 + L:1 + 2 * L] = 1.0
        rout = torch.full((1 + 2 * cap,), SENTINEL, dtype=torch.float64, device=cuda)
        ret = torch.zeros(E, dtype=torch.float64, device=cuda)
    else:
        sc = RunningRewardScaler(E, per_env=True, device=cuda)
    for call, S in enumerate(calls):
        r, first = _per_env_inputs(name, E, S, call)
        ref = orc(r, first)
        if entry == "raw":
            Lo = max(S, L)
            out = torch.full((S if S > 1 or Lo == 1 else Lo, E), SENTINEL, dtype=torch.float64, device=cuda)
            L = ops.reward_scale_per_env(_dev(r, cuda), _dev(first, cuda), ret, rin, L, rout,
                                         ops.reward_scale_workspace(S, E, cuda), out)
            torch.cuda.synchronize()
            assert L == Lo
            st = rout.cpu().numpy()
            _check_per_env(name, call, ref, out.cpu().numpy(), ret.cpu().numpy(), st[1:1 + L], st[1 + L:1 + 2 * L], st[0])
            rin, rout = rout, rin
        else:
            out = sc(reward=r.T, first=first.T)
            st = sc.ret_rms
            _check_per_env(name, call, ref, out.T, sc.ret.cpu().numpy(), st.mean, st.var, st.count)


def test_reward_scale_per_env_rejects_what_the_oracle_rejects(cuda):
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util.reward_scaling import RunningRewardScaler
    E, S = C.PER_ENV_REJECT
    r, first = _per_env_inputs("reject", E, S, 0)
    with pytest.raises(ValueError):
        C.ScaleRef(E, per_env=True)(r, first)
    with pytest.raises(ValueError):
        RunningRewardScaler(E, per_env=True, device=cuda)(reward=r.T, first=first.T)
    rin = torch.tensor([1e-4] + [0.0] * E + [1.0] * E, dtype=torch.float64, device=cuda)
    rout = torch.full((1 + 2 * S,), SENTINEL, dtype=torch.float64, device=cuda)
    out = torch.full((S, E), SENTINEL, dtype=torch.float64, device=cuda)
    with pytest.raises(ValueError):
        ops.reward_scale_per_env(_dev(r, cuda), _dev(first, cuda), torch.zeros(E, dtype=torch.float64, device=cuda), rin,
                                 E, rout, ops.reward_scale_workspace(S, E, cuda), out)
    torch.cuda.synchronize()
    assert bool((rout == SENTINEL).all()) and bool((out == SENTINEL).all())
    _log("dppo_reward_scale_per_env", "reject-4x50", 0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------
# 4. dppo_episode_sums, row by row
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", C.EP_REWARDS)
@pytest.mark.parametrize("S,E", C.EP_SIZES)
def test_episode_sums_rows(cuda, S, E, kind):
    """every env's row against O.episode_stats on that env's column: the episode and success counts exact, the
    two sums within 1e-12 (1 + sum |r| of the env); all E rows written and the guard row after them untouched"""
    import torch
    from diffusionpolicyoptimization_amd import ops
    firsts, rew, _ = C.ep_inputs(S, E, kind)
    thr = C.ep_threshold(kind)
    ref = C.episode_rows_ref(firsts, rew, C.EP_ACT_STEPS, thr)
    buf = torch.full((E + 1, 4), SENTINEL, dtype=torch.float64, device=cuda)
    ops.episode_sums(_dev(rew, cuda), _dev(firsts, cuda), C.EP_ACT_STEPS, thr, buf[:E])
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[E] == SENTINEL).all() and not (got[:E] == SENTINEL).any()
    _check("dppo_episode_sums", f"{S}x{E}-{kind}-sums", got[:E, 1:3], ref[:, 1:3], C.ep_bound(rew)[:, None])
    _check("dppo_episode_sums", f"{S}x{E}-{kind}-counts", got[:E][:, [0, 3]], ref[:, [0, 3]], 0.0)


# ------------------------------------------------------------------------------------------------
# 5. dppo_ppo_adv_stats / _all
# ------------------------------------------------------------------------------------------------
def _adv_one(cuda, case, adv, adv_t, total, kf, start, rows, ri=None):
    import torch
    from diffusionpolicyoptimization_amd import ops
    out = torch.full((4,), SENTINEL, dtype=torch.float64, device=cuda)
    ops.ppo_adv_stats(adv_t, total, kf, C.ADV_SEED, C.ADV_EPOCH, start, rows, out[:3], None if ri is None else _dev(ri, cuda))
    torch.cuda.synchronize()
    ref, bound = C.adv_ref(adv, total, kf, C.ADV_SEED, C.ADV_EPOCH, start, rows, ri)
    got = out.cpu().numpy()
    assert got[3] == SENTINEL
    _check("dppo_ppo_adv_stats", case, got[:3], ref, bound)


@pytest.mark.parametrize("N,kf,windows", C.ADV_CASES + [C.ADV_SECOND_TRIP[:2] + ([C.ADV_SECOND_TRIP[2:]],)],
                         ids=lambda v: str(v) if isinstance(v, int) else "w")
def test_adv_stats(cuda, N, kf, windows):
    """{count, sum, sumsq} of adv[feistel(start + i) // kf]: count exact, the sums within the bound of a float64
    sum in arbitrary order; ragged and empty windows; 131073 rows (the 512 workgroups' second trip)"""
    adv = C.adv_values(N)
    adv_t = _dev(adv, cuda)
    for start, rows in windows:
        _adv_one(cuda, f"{N}x{kf}-{start}+{rows}", adv, adv_t, N * kf, kf, start, rows)


@pytest.mark.parametrize("N,kf", [(97, 10), (1025, 17)])
def test_adv_stats_row_index(cuda, N, kf):
    """the explicit row table: repeats; entries at -1 and at `total` are skipped and count says so"""
    adv = C.adv_values(N)
    ri = C.adv_row_index(N * kf, 300)
    assert ((ri < 0) | (ri >= N * kf)).sum() > 10
    for start, rows in [(0, 300), (10, 280), (299, 1), (3, 0)]:
        _adv_one(cuda, f"{N}x{kf}-row_index-{start}+{rows}", adv, _dev(adv, cuda), N * kf, kf, start, rows, ri)


@pytest.mark.parametrize("N,kf,rows_full,n_batch,n_epochs", C.ADV_ALL_CASES)
def test_adv_stats_all(cuda, N, kf, rows_full, n_batch, n_epochs):
    """every minibatch of every epoch directly against the oracle; rows_full = 16385 (the 64 workgroups'
    second trip) over three epochs with a ragged last minibatch"""
    import torch
    from diffusionpolicyoptimization_amd import ops
    adv = C.adv_values(N)
    out = torch.full((n_epochs * n_batch + 1, 3), SENTINEL, dtype=torch.float64, device=cuda)
    ops.ppo_adv_stats_all(_dev(adv, cuda), N * kf, kf, C.ADV_SEED, C.ADV_EPOCH, n_epochs, rows_full, n_batch, out[:-1])
    torch.cuda.synchronize()
    ref, bound = C.adv_all_ref(adv, N * kf, kf, C.ADV_SEED, C.ADV_EPOCH, n_epochs, rows_full, n_batch)
    got = out.cpu().numpy()
    assert (got[-1] == SENTINEL).all()
    assert len({tuple(r) for r in ref}) > (n_epochs - 1) * (N > 1)            # the epochs' minibatches differ
    _check("dppo_ppo_adv_stats_all", f"{N}x{kf}-{rows_full}x{n_batch}x{n_epochs}", got[:-1], ref, bound)


@pytest.mark.parametrize("n_epochs,rows_full", [(65, 200), (3, 0)])
def test_adv_stats_all_refusals(cuda, n_epochs, rows_full):
    import torch
    from diffusionpolicyoptimization_amd import _lib, ops
    out = torch.full((n_epochs * 2, 3), SENTINEL, dtype=torch.float64, device=cuda)
    with pytest.raises(_lib.DppoError):
        ops.ppo_adv_stats_all(_dev(C.adv_values(97), cuda), 970, 10, C.ADV_SEED, 0, n_epochs, rows_full, 2, out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    _log("dppo_ppo_adv_stats_all", f"refused-{n_epochs}-{rows_full}", 0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------
# 6. dppo_feistel_permute
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(C.FEISTEL_N))
def test_feistel_full_range(cuda, n):
    """bit-exact against PX.feistel_permute and a permutation of range(n), on both sides of every power of
    four up to 4^8, over seeds above 2^32 and several epochs"""
    from diffusionpolicyoptimization_amd import ops
    seen = set()
    for seed in C.FEISTEL_SEEDS:
        for epoch in C.FEISTEL_EPOCHS if n <= 4097 else C.FEISTEL_EPOCHS[:1]:
            got = ops.feistel_permute(0, n, n, seed, epoch, cuda).cpu().numpy()
            assert np.array_equal(got, PX.feistel_permute(np.arange(n), n, seed, epoch)), (n, seed, epoch)
            assert np.array_equal(np.sort(got), np.arange(n))
            seen.add(got.tobytes())
    if n == 257:
        assert len(seen) == len(C.FEISTEL_SEEDS) * len(C.FEISTEL_EPOCHS)     # every (seed, epoch) its own permutation
    _log("dppo_feistel_permute", f"full-{n}", 0.0, 0.0, 0.0)


@pytest.mark.parametrize("n", C.FEISTEL_WINDOW_N)
def test_feistel_windows(cuda, n):
    """first > 0, count < n: a window equals the same slice of the full permutation"""
    import torch
    from diffusionpolicyoptimization_amd import ops
    seed, epoch = C.FEISTEL_SEEDS[1], 7
    full = PX.feistel_permute(np.arange(n), n, seed, epoch)
    for first, count in C.feistel_windows(n):
        got = ops.feistel_permute(first, count, n, seed, epoch, cuda).cpu().numpy()
        assert np.array_equal(got, full[first:first + count]), (n, first, count)
    assert ops.feistel_permute(3, 0, n, seed, epoch, cuda).numel() == 0
    torch.cuda.synchronize()
    _log("dppo_feistel_permute", f"windows-{n}", 0.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------
# 7. dppo_value_moments
# ------------------------------------------------------------------------------------------------
def _value_moments(cuda, val, ret, target):
    import torch
    from diffusionpolicyoptimization_amd import ops
    if target == "mapped":
        out = ops.MappedDoubles(5)
        ops.value_moments(_dev(val, cuda), _dev(ret, cuda), out.address)
        torch.cuda.synchronize()
        return np.array(out.array[:5])
    out = torch.full((6,), SENTINEL, dtype=torch.float64, device=cuda)
    ops.value_moments(_dev(val, cuda), _dev(ret, cuda), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[5] == SENTINEL
    return got[:5]


@pytest.mark.parametrize("target", ["mapped", "device"])
@pytest.mark.parametrize("n", C.VM_SIZES)
def test_value_moments(cuda, n, target):
    """each sum within max(1e-12, 2 n 2^-53) sum |terms|; out[4] == n; into mapped host memory and a device tensor"""
    val, ret = C.vm_inputs(n)
    ref, bound = C.vm_ref(val, ret)
    _check("dppo_value_moments", f"{n}-{target}", _value_moments(cuda, val, ret, target), ref, bound)


def test_value_moments_explained_variance_under_cancellation(cuda):
    """returns with mean 1e4 and spread 1e-2: Var(y) is 1e-12 of sum y^2 / n, so the moments' 1e-12 floor would
    allow a variance of zero (ev_bound is infinite with it; asserted in the CPU suite). The explained variance is
    therefore held to ev_bound of the a-priori part of the moments' bound alone, 2 n 2^-53 sum |terms| (n = 65), and
    the moments of this case to that part as well as to the whole bound."""
    val, ret = C.vm_inputs(C.VM_EV_N, ev_case=True)
    ref, bound = C.vm_ref(val, ret)
    _, a_priori = C.vm_ref(val, ret, floor=0.0)
    got = _value_moments(cuda, val, ret, "mapped")
    _check("dppo_value_moments", "ev-moments", got, ref, bound)
    _check("dppo_value_moments", "ev-moments-a-priori", got, ref, a_priori)
    ev = O.explained_variance(val.astype(np.float64), ret.astype(np.float64))
    _check("dppo_value_moments", "ev", C.ev_from_moments(got), ev, C.ev_bound(ref, a_priori))
