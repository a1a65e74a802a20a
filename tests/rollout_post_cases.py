"""Cases, float64 references, bounds and NumPy emulations for the kernels that run between the rollout and
the update (tests/test_rollout_post_cpu.py, tests/test_rollout_post_gpu.py): dppo_gae, dppo_reward_scale*,
dppo_episode_sums, dppo_value_moments (csrc/scan.hip), dppo_ppo_adv_stats, dppo_ppo_adv_stats_all and
dppo_feistel_permute (csrc/update.hip).

Every reference is oracle/ code (O.gae, O.RunningRewardScalerOracle, O.episode_stats, O.explained_variance,
PX.feistel_permute) or a per-env / per-minibatch helper built from it; none calls the library. The
emulations restate the kernels' own operation order (lane chunks, the 6-step shuffle composition, the replay,
Welford / Chan moments, the LDS chunk walk) and take mistakes as keyword flags, so the CPU tests can show
both that a correct kernel reaches the bounds and that the inputs catch a wrong one."""
import numpy as np

from oracle import dppo_oracle as O
from oracle import philox as PX

U = 2.0 ** -53          # fp64 unit roundoff


def ratio(got, ref, bound):
    """(max |got - ref| / bound, |got - ref| and the bound where that maximum is); a zero bound demands
    equality."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0, 0.0, 0.0
    err = np.abs(got - ref).reshape(-1)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    q = np.where(np.isnan(q), np.inf, q)
    i = int(np.argmax(q))
    return float(q[i]), float(err[i]), float(bound[i])


# ------------------------------------------------------------------------------------------------
# the wave scans' geometry: lane l holds the CH = ceil(S / 64) steps from l * CH
# ------------------------------------------------------------------------------------------------
# S -> (CH, lanes that hold a step, steps of the last such lane)
SCAN_TABLE = {1: (1, 1, 1), 2: (1, 2, 1), 63: (1, 63, 1), 64: (1, 64, 1), 65: (2, 33, 1), 127: (2, 64, 1),
              128: (2, 64, 2), 129: (3, 43, 3), 130: (3, 44, 1), 193: (4, 49, 1), 257: (5, 52, 2), 300: (5, 60, 5)}


def chunk(S):
    return (S + 63) // 64


def scan_geometry(S):
    CH = chunk(S)
    lanes = (S + CH - 1) // CH
    return CH, lanes, S - (lanes - 1) * CH


PATTERNS = ("none", "all", "chunk_first", "chunk_last", "last_only", "first_only", "random")


def flags(pattern, S, E, rng):
    """u8 [S, E] termination / first flags. chunk_first: t = k CH; chunk_last: t = k CH + CH - 1 clipped to
    S - 1; random: p = 0.3."""
    CH, t = chunk(S), np.arange(S)
    if pattern == "random":
        return (rng.random((S, E)) < 0.3).astype(np.uint8)
    col = {"none": t < 0, "all": t >= 0, "chunk_first": t % CH == 0,
           "chunk_last": (t % CH == CH - 1) | (t == S - 1), "last_only": t == S - 1, "first_only": t == 0}[pattern]
    return np.repeat(col.astype(np.uint8)[:, None], E, axis=1)


# ------------------------------------------------------------------------------------------------
# 1. GAE
# ------------------------------------------------------------------------------------------------
# every S of the list; E = 1, 3, 4, 5, 9 (1, 3, 4, 1, 1 live waves in the last workgroup) each with an S > 64
GAE_SIZES = [(1, 5), (2, 3), (63, 4), (64, 9), (65, 1), (127, 3), (128, 4), (129, 5), (130, 9), (193, 5)]
GAE_KNOBS = [(1.0, 1.0), (0.99, 0.0)]     # (gamma, lam) at S = 129


def gae_inputs(S, E, pattern):
    rng = np.random.default_rng([11, S, E, PATTERNS.index(pattern)])
    return dict(r=rng.normal(size=(S, E)), v=rng.normal(size=(S, E)).astype(np.float32),
                lv=rng.normal(size=E).astype(np.float32), term=flags(pattern, S, E, rng))


def gae_ref(inp, gamma=0.99, lam=0.95):
    return O.gae(inp["r"], inp["v"].astype(np.float64), inp["lv"].astype(np.float64), inp["term"].astype(np.float64),
                 gamma=gamma, lam=lam)


def gae_slack(ref):
    """what the scan goldens allow for fp64 reassociation"""
    return 1e-12 * (1 + np.abs(ref).max()) if ref.size else 0.0


def gae_bound(ref):
    """per element: the one float32 rounding of the store + the reassociation slack"""
    return 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + gae_slack(ref)


def _lanes(x, S, fill=0.0):
    """[S, E] -> [64, CH, E], padded with `fill`"""
    CH = chunk(S)
    pad = np.full((64 * CH,) + x.shape[1:], fill, np.float64)
    pad[:S] = x
    return pad.reshape(64, CH, -1)


def _valid(S):
    CH = chunk(S)
    return (np.arange(64 * CH) < S).reshape(64, CH, 1)


def _affine_scan(C, D, forward):
    """affine_scan (csrc/scan.hip) over axis 0 = the 64 lanes"""
    lane = np.arange(64)[:, None]
    for off in (1, 2, 4, 8, 16, 32):
        src = np.clip(lane[:, 0] - off if forward else lane[:, 0] + off, 0, 63)
        oc, od = C[src], D[src]
        has = lane >= off if forward else lane + off < 64
        D = np.where(has, D + C * od, D)
        C = np.where(has, C * oc, C)
    return C, D


def emu_gae(inp, gamma=0.99, lam=0.95, rsc=1.0, drop_carry=False, next_value_wrong=False, c_without_nonterm=False):
    """gae_kernel in float64 NumPy -> (adv, returns) before the float32 store. Mistakes: drop_carry (no carry
    across a lane boundary), next_value_wrong (values[t + 1] of a padded array instead of last_values at
    t = S - 1), c_without_nonterm (gamma lam without the nonterminal factor)."""
    r, v, lv, term = inp["r"], inp["v"].astype(np.float64), inp["lv"].astype(np.float64), inp["term"]
    S, E = r.shape
    CH = chunk(S)
    nonterm = 1.0 - term.astype(np.float64)
    last = np.random.default_rng(5).normal(size=E) if next_value_wrong else lv
    nextv = np.concatenate([v[1:], last[None]], 0)
    dl = _lanes(r * rsc + gamma * nextv * nonterm - v, S)
    c = _lanes(gamma * lam * (1.0 if c_without_nonterm else nonterm) * np.ones_like(r), S)
    ok = _valid(S)
    C, D = np.ones((64, E)), np.zeros((64, E))
    for k in reversed(range(CH)):
        D = np.where(ok[:, k], dl[:, k] + c[:, k] * D, D)
        C = np.where(ok[:, k], c[:, k] * C, C)
    C, D = _affine_scan(C, D, False)
    carry = np.concatenate([D[1:], np.zeros((1, E))], 0)
    if drop_carry:
        carry = np.zeros((64, E))
    adv = np.zeros((64, CH, E))
    for k in reversed(range(CH)):
        carry = np.where(ok[:, k], dl[:, k] + c[:, k] * carry, carry)
        adv[:, k] = carry
    adv = adv.reshape(64 * CH, E)[:S]
    return adv, adv + v


# ------------------------------------------------------------------------------------------------
# 2. / 3. the running reward scaler
# ------------------------------------------------------------------------------------------------
# every S of {1, 63, 64, 65, 128, 129, 193} and every E of {1, 3, 5, 64, 65, 130} (moments_kernel walks envs
# with stride 64: 65 and 130 give a lane a second and a third env)
SCALE_SIZES = [(1, 3), (63, 5), (64, 64), (65, 65), (128, 1), (129, 130), (193, 5)]
SCALE_PATTERNS = PATTERNS + ("carry",)     # carry: on calls 2 and 3 first[0] is 0 for even envs, 1 for odd ones
SCALE_KNOBS = {"gamma": dict(gamma=0.9), "epsilon": dict(epsilon=1e-2), "cliprew": dict(cliprew=0.5)}   # S = 65, E = 5
N_CALLS = 3


def scale_inputs(S, E, pattern, call, mean=0.5):
    rng = np.random.default_rng([12, S, E, SCALE_PATTERNS.index(pattern), call])
    r = rng.normal(mean, 2.0, size=(S, E))
    first = flags("random" if pattern == "carry" else pattern, S, E, rng)
    if pattern == "carry":
        first[0] = (np.arange(E) + (call if E == 1 else 0)) % 2 if call else 0
    return r, first


def oracle_rets(prev, reward_es, first_es, gamma):
    """the discounted running return of O.RunningRewardScalerOracle.__call__ (its first four lines), all
    columns; ScaleRef checks the last column against the oracle's own state"""
    rets = np.zeros_like(reward_es, dtype=np.float64)
    for t in range(reward_es.shape[1]):
        prev = rets[:, t] = reward_es[:, t] + (1 - first_es[:, t]) * gamma * prev
    return rets


def scale_bound(ref, key="out"):
    """the goldens' rtol = 1e-12 with atol = 1e-12 max(1, max |ref|) over the compared array; the entries of
    {mean, var, count} and of {n, mean, M2} are quantities of their own, each with its own atol"""
    ref = np.asarray(ref, np.float64)
    top = np.abs(ref) if key in ("rms", "moments") else float(np.abs(ref).max())
    return 1e-12 * np.maximum(1.0, top) + 1e-12 * np.abs(ref)


class ScaleRef:
    """O.RunningRewardScalerOracle over consecutive calls on time-major inputs -> per call dict(out [S, E] (or
    [L, E], per_env with S == 1), ret [E], rms = [mean, var, count] (per_env: mean [L], var [L], count) and the
    batch moments {n, mean, M2} of the scalar form)."""

    def __init__(self, E, per_env=False, **knobs):
        self.orc = O.RunningRewardScalerOracle(E, per_env=per_env, **knobs)
        self.per_env = per_env

    def __call__(self, r, first):
        orc = self.orc
        rets = oracle_rets(orc.ret, r.T, first.T.astype(np.float64), orc.gamma)
        out = orc(r.T, first.T.astype(np.float64)).T
        assert np.array_equal(rets[:, -1], orc.ret)
        x = rets.reshape(-1)
        res = dict(out=out, ret=orc.ret.copy(), moments=np.array([x.size, x.mean(), x.var() * x.size]))
        if self.per_env:
            res.update(mean=np.array(orc.mean, np.float64).reshape(-1), var=np.array(orc.var, np.float64).reshape(-1),
                       count=float(orc.count))
        else:
            res["rms"] = np.array([orc.mean, orc.var, orc.count], np.float64)
        return res


def _chan(n, mean, m2, nb, meanb, m2b):
    """chan_merge (csrc/scan.hip), elementwise"""
    with np.errstate(divide="ignore", invalid="ignore"):
        tot = n + nb
        delta = meanb - mean
        mean1 = mean + delta * nb / tot
        m21 = m2 + m2b + delta * delta * n * nb / tot
    keep, take = nb == 0, (n == 0) & (nb != 0)
    return (np.where(keep, n, np.where(take, nb, tot)), np.where(keep, mean, np.where(take, meanb, mean1)),
            np.where(keep, m2, np.where(take, m2b, m21)))


def _butterfly(n, mean, m2):
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        n, mean, m2 = _chan(n, mean, m2, n[lane ^ off], mean[lane ^ off], m2[lane ^ off])
    return n[0], mean[0], m2[0]


def emu_rets(r, first, ret_state, gamma, drop_carry=False, ignore_first_on_chunk_start=False):
    """rets_kernel -> (rets [S, E], new ret_state [E], per-env moments [E, 3])"""
    S, E = r.shape
    CH = chunk(S)
    f = first.astype(np.float64)
    g = _lanes((1.0 - f) * gamma, S)
    if ignore_first_on_chunk_start:
        g[:, 0] = gamma
    rr, ok = _lanes(r, S), _valid(S)
    C, D = np.ones((64, E)), np.zeros((64, E))
    for k in range(CH):
        D = np.where(ok[:, k], rr[:, k] + g[:, k] * D, D)
        C = np.where(ok[:, k], g[:, k] * C, C)
    C, D = _affine_scan(C, D, True)
    y0 = np.asarray(ret_state, np.float64)
    carry = np.concatenate([y0[None], D[:-1] + C[:-1] * y0], 0)
    if drop_carry:
        carry = np.repeat(y0[None], 64, 0)
    rets = np.zeros((64, CH, E))
    n, mean, m2 = np.zeros((64, E)), np.zeros((64, E)), np.zeros((64, E))
    for k in range(CH):
        carry = np.where(ok[:, k], rr[:, k] + g[:, k] * carry, carry)
        rets[:, k] = carry
        n1 = n + 1.0
        dlt = carry - mean
        mean1 = mean + dlt / n1
        m21 = m2 + dlt * (carry - mean1)
        n, mean, m2 = np.where(ok[:, k], n1, n), np.where(ok[:, k], mean1, mean), np.where(ok[:, k], m21, m2)
    rets = rets.reshape(64 * CH, E)[:S]
    return rets, rets[S - 1].copy(), np.stack(_butterfly(n, mean, m2), 1)


def emu_moments(env_mom, first64_only=False):
    """moments_kernel: lane `tid` merges envs tid, tid + 64, ... in order, then the butterfly"""
    E = env_mom.shape[0]
    n, mean, m2 = np.zeros(64), np.zeros(64), np.zeros(64)
    for j in range(1 if first64_only else (E + 63) // 64):
        part = np.zeros((64, 3))
        sl = env_mom[64 * j:64 * j + 64]
        part[:sl.shape[0]] = sl
        n, mean, m2 = _chan(n, mean, m2, part[:, 0], part[:, 1], part[:, 2])
    return np.array(_butterfly(n, mean, m2))


def emu_scale_call(state, r, first, gamma=0.99, cliprew=10.0, epsilon=1e-8, no_ret_carry=False, m2_div_tot=False,
                   first64_only=False, **scan_mistakes):
    """dppo_reward_scale on state = dict(ret [E], rms [mean, var, count]) (updated in place) -> the ScaleRef
    fields"""
    y0 = np.zeros_like(state["ret"]) if no_ret_carry else state["ret"]
    rets, state["ret"], env_mom = emu_rets(r, first, y0, gamma, **scan_mistakes)
    n, mean, m2 = emu_moments(env_mom, first64_only)
    rm, rv, rc = state["rms"]
    bv = m2 / n if n > 0 else 0.0
    delta = mean - rm
    tot = rc + n
    M2 = rv * rc + bv * n + delta * delta * rc * n / tot
    state["rms"] = np.array([rm + delta * n / tot, M2 / (tot if m2_div_tot else tot - 1.0), tot])
    out = np.clip(r / np.sqrt(state["rms"][1] + epsilon), -cliprew, cliprew)
    return dict(out=out, ret=state["ret"].copy(), rms=state["rms"].copy(), moments=np.array([n, mean, m2]))


def scale_state(E):
    return dict(ret=np.zeros(E), rms=np.array([0.0, 1.0, 1e-4]))


SCALE_FIELDS = ("out", "ret", "rms", "moments")

# per_env = True: (E, [S of each call]); None = the shape the oracle rejects
PER_ENV_CASES = {"S=E=65": (65, [65, 65, 65]), "E=1,S=257": (1, [257, 257]), "E=1,S=300": (1, [300, 300]),
                 "S=1,E=5": (5, [1, 5, 5])}
PER_ENV_REJECT = (4, 50)


# ------------------------------------------------------------------------------------------------
# 4. episode sums, row by row
# ------------------------------------------------------------------------------------------------
EP_SIZES = [(1, 63), (30, 1), (31, 64), (32, 65), (33, 129), (63, 1), (64, 63), (65, 65), (97, 129), (33, 1), (97, 64)]
EP_REWARDS = ("normal", "negative", "integer")
EP_ACT_STEPS = 4
# name -> (smallest S, flagged rows, episodes it is designed to count)
EP_LAYOUTS = {
    "none": (1, lambda S: [], lambda S: 0),
    "single": (1, lambda S: [S // 2], lambda S: 0),
    "every": (1, lambda S: list(range(S + 1)), lambda S: 0),                 # every episode has length 1
    "ends": (1, lambda S: [0, S], lambda S: int(S > 1)),                     # one episode from 0 to S
    "ends_plus": (1, lambda S: [0, 1, S], lambda S: int(S > 2)),             # a length-1 episode, then 1 to S
    "x31_32": (32, lambda S: [31, 32], lambda S: 0),                         # length 1 across the LDS chunk edge
    "x30_32": (32, lambda S: [30, 32], lambda S: 1),                         # ends on the first row of chunk 1
    "x31_33": (33, lambda S: [31, 33], lambda S: 1),                         # its two rewards straddle the edge
    "random": (1, None, None),                                               # p = 0.2
}


def ep_threshold(kind):
    return 3.0 if kind == "integer" else 0.3


def ep_layout_of(S, E, kind):
    """the layout of every env: the layouts that fit S in turn, rotated by the case so E = 1 sees them all"""
    fit = [k for k, (s_min, _, _) in EP_LAYOUTS.items() if S >= s_min]
    rot = S + EP_REWARDS.index(kind)
    return [fit[(e + rot) % len(fit)] for e in range(E)]


def ep_inputs(S, E, kind):
    """-> (firsts u8 [S + 1, E], rewards [S, E], layout name per env). integer: multiples of act_steps in
    [-2, 3] act_steps with the threshold at 3, so a best reward often equals it exactly."""
    rng = np.random.default_rng([14, S, E, EP_REWARDS.index(kind)])
    if kind == "integer":
        rew = EP_ACT_STEPS * rng.integers(-2, 4, size=(S, E)).astype(np.float64)
    else:
        rew = rng.normal(0, 2, (S, E))
        if kind == "negative":
            rew = -np.abs(rew) - 0.1
    firsts = np.zeros((S + 1, E), np.uint8)
    names = ep_layout_of(S, E, kind)
    for e, name in enumerate(names):
        if name == "random":
            firsts[:, e] = rng.random(S + 1) < 0.2
        else:
            firsts[EP_LAYOUTS[name][1](S), e] = 1
    return firsts, rew, names


def ep_designed_count(name, S, col):
    """episodes an env's layout must count, from host arithmetic (random: gaps > 1 between flagged rows)"""
    if name == "random":
        return int((np.diff(np.flatnonzero(col)) > 1).sum())
    return EP_LAYOUTS[name][2](S)


def episode_rows_ref(firsts, rew, act_steps, thr):
    """O.episode_stats on one env's column at a time -> [E, 4] {episodes, sum of returns, sum of best rewards,
    successes}"""
    E = firsts.shape[1]
    rows = np.zeros((E, 4))
    for e in range(E):
        st = O.episode_stats(firsts[:, e:e + 1], rew[:, e:e + 1], act_steps, thr)
        n = st["num_episode_finished"]
        rows[e] = [n, st["avg_episode_reward"] * n, st["avg_best_reward"] * n, round(st["success_rate"] * n)]
    return rows


def ep_bound(rew):
    """per env, for the two sums"""
    return 1e-12 * (1 + np.abs(rew).sum(axis=0))


def emu_episode_rows(firsts, rew, act_steps, thr, count_len1=False, drop_chunk_span=False, ignore_last_row=False,
                     max_from_zero=False, strict_threshold=False, bests=None):
    """episode_sums_kernel's walk, one env at a time. Mistakes: count_len1, drop_chunk_span (an episode open at a
    32-step chunk edge is forgotten), ignore_last_row (the flag row t = S), max_from_zero, strict_threshold
    (> for >=). bests: a list that receives every counted episode's best reward."""
    S, E = rew.shape
    rows = np.zeros((E, 4))
    for e in range(E):
        start, run, mx = -1, 0.0, 0.0
        for t in range(S + 1):
            if drop_chunk_span and t % 32 == 0:
                start = -1
            if firsts[t, e] and not (ignore_last_row and t == S):
                if start >= 0 and (t - start > 1 or count_len1):
                    b = mx / act_steps
                    rows[e] += [1.0, run, b, float(b > thr if strict_threshold else b >= thr)]
                    if bests is not None:
                        bests.append(b)
                start, run, mx = t, 0.0, 0.0 if max_from_zero else -np.inf
            if t < S:
                run += rew[t, e]
                mx = max(mx, rew[t, e])
    return rows


# ------------------------------------------------------------------------------------------------
# 5. advantage moments of a minibatch
# ------------------------------------------------------------------------------------------------
# (N, kf, [(start, rows)]): whole, a first minibatch, a ragged last one, rows = 0, an inner window
ADV_CASES = [(1, 1, [(0, 1), (0, 0)]),
             (97, 10, [(0, 970), (0, 200), (800, 170), (970, 0), (123, 300)]),
             (64, 4, [(0, 256), (0, 100), (200, 56), (255, 1), (17, 0)]),
             (1025, 17, [(0, 17425), (0, 5000), (15000, 2425), (4999, 257)])]
ADV_SECOND_TRIP = (13108, 10, 3, 131073)        # 512 workgroups x 256 rows + 1
ADV_ALL_CASES = [(97, 10, 200, 5, 3), (64, 4, 100, 3, 2), (1, 1, 1, 1, 1), (1025, 17, 5000, 4, 2),
                 (3287, 10, 16385, 3, 3)]       # (N, kf, rows_full, n_batch, n_epochs); last: 64 x 256 rows + 1
ADV_SEED, ADV_EPOCH = (5 << 32) + 77, 3000


def adv_values(N):
    return np.random.default_rng([15, N]).normal(0.3, 1.0, size=N).astype(np.float32)


def adv_row_index(total, n):
    """an explicit row table: repeats, and entries at -1 and at `total` (skipped)"""
    rng = np.random.default_rng([16, total, n])
    ri = rng.integers(0, total, size=n)
    ri[::7] = ri[0]
    ri[3::11] = -1
    ri[5::13] = total
    return ri.astype(np.int64)


def adv_ref(adv, total, kf, seed, epoch, start, rows, row_index=None, mod_kf=False, count_invalid=False, trip=None):
    """{count, sum, sumsq} of adv[PX.feistel_permute(start + i, total, seed, epoch) // kf], i < rows, in
    float64, and the bound of the two sums. Mistakes: mod_kf (idx % kf), count_invalid (row_index entries
    outside [0, total) counted), trip (only the first `trip` rows: a grid-stride loop that stops after its
    first pass)."""
    n = rows if trip is None else min(rows, trip)
    i = start + np.arange(n, dtype=np.int64)
    invalid = 0
    if row_index is None:
        idx = PX.feistel_permute(i, total, seed, epoch) if n else np.zeros(0, np.int64)
    else:
        idx = row_index[i]
        ok = (idx >= 0) & (idx < total)
        invalid, idx = int((~ok).sum()), idx[ok]
    terms = adv.astype(np.float64)[idx % kf if mod_kf else idx // kf]
    count = terms.size + (invalid if count_invalid else 0)
    f = max(1e-12, 2 * rows * U)
    return (np.array([count, terms.sum(), (terms * terms).sum()]),
            np.array([0.0, f * np.abs(terms).sum(), f * (terms * terms).sum()]))


def adv_all_ref(adv, total, kf, seed, epoch0, n_epochs, rows_full, n_batch, trip=None):
    ref, bound = [], []
    for e in range(n_epochs):
        for b in range(n_batch):
            start = b * rows_full
            rows = max(0, min(rows_full, total - start))
            r, bd = adv_ref(adv, total, kf, seed, epoch0 + e, start if rows else 0, rows, trip=trip)
            ref.append(r)
            bound.append(bd)
    return np.array(ref), np.array(bound)


# ------------------------------------------------------------------------------------------------
# 6. the Feistel permutation
# ------------------------------------------------------------------------------------------------
# n -> half_bits: the domain is 4^half_bits >= n; one past a power of four, 3/4 of the domain walks on
FEISTEL_N = {1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 15: 2, 16: 2, 17: 3, 255: 4, 256: 4, 257: 5, 4095: 6, 4096: 6, 4097: 7,
             65536: 8, 65537: 9}
FEISTEL_WINDOW_N = (17, 257, 65537)
FEISTEL_SEEDS = ((1 << 32) + 1, (0xDEADBEEF << 32) | 0x12345678, (1 << 63) + 5)
FEISTEL_EPOCHS = (0, 1, 3000)


def feistel_windows(n):
    """(first, count): the first 5, the last 5 and a span across index 256 (where n reaches it)"""
    w = [(0, 5), (n - 5, 5)]
    if n > 256:
        w.append((250, min(12, n - 250)))
    return w


# ------------------------------------------------------------------------------------------------
# 7. explained-variance moments
# ------------------------------------------------------------------------------------------------
VM_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)
VM_EV_N = 65


def vm_inputs(n, ev_case=False):
    rng = np.random.default_rng([17, n, int(ev_case)])
    if ev_case:     # returns with mean 1e4 and spread 1e-2
        ret = (1e4 + rng.normal(0, 1e-2, n)).astype(np.float32)
        val = (ret.astype(np.float64) - rng.normal(0, 5e-3, n)).astype(np.float32)
    else:
        val = rng.normal(size=n).astype(np.float32)
        ret = (val + rng.normal(0, 0.3, n)).astype(np.float32)
    return val, ret


def vm_ref(val, ret, floor=1e-12):
    """{sum y, sum y^2, sum d, sum d^2, n} in float64 and each sum's bound max(floor, 2 n 2^-53) sum |terms|
    (the terms themselves are exact: a float32 squared, and a difference of float32s squared, fit in 53 bits)"""
    y = ret.astype(np.float64)
    d = y - val.astype(np.float64)
    n = y.size
    f = max(floor, 2 * n * U)
    return (np.array([y.sum(), (y * y).sum(), d.sum(), (d * d).sum(), n]),
            np.array([f * np.abs(y).sum(), f * (y * y).sum(), f * np.abs(d).sum(), f * (d * d).sum(), 0.0]))


def ev_from_moments(m):
    n = m[4]
    var_y = m[1] / n - (m[0] / n) ** 2
    var_d = m[3] / n - (m[2] / n) ** 2
    return np.nan if var_y == 0 else 1.0 - var_d / var_y


def ev_bound(ref, bound):
    """The error of ev_from_moments(m) when each m[k] is within bound[k] of ref[k]: a variance s2 / n -
    (s1 / n)^2 moves by at most  B2 / n + (2 |s1 / n| + B1 / n) B1 / n  through its moments and by 4 u s2 / n
    through the four float64 roundings of the formula itself (the two terms cancel, so those are relative to
    s2 / n, not to the variance); the quotient then by  dvd / (vy - dvy) + vd dvy / (vy (vy - dvy)). Infinite
    when dvy >= vy: the moments' bounds then allow a variance of zero."""
    n = ref[4]

    def var_and_err(s1, s2, b1, b2):
        return s2 / n - (s1 / n) ** 2, b2 / n + (2 * abs(s1 / n) + b1 / n) * b1 / n + 4 * U * s2 / n
    vy, dvy = var_and_err(ref[0], ref[1], bound[0], bound[1])
    vd, dvd = var_and_err(ref[2], ref[3], bound[2], bound[3])
    if dvy >= vy:
        return np.inf
    return dvd / (vy - dvy) + (vd + dvd) * dvy / (vy * (vy - dvy)) + 4 * U
