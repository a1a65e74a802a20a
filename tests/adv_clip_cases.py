"""The cases of the advantage-clip tests (tests/test_adv_clip_cpu.py, tests/test_adv_clip_gpu.py):
PPODiffusion's clip_advantage_lower_quantile / clip_advantage_upper_quantile.

The float64 definition (quantile, bounds, clip_adv) and the clipped loss are the oracle's
(oracle/dppo_oracle.py; O.c_loss(adv_clip_quantiles=..., adv_clip_bounds=...)). Here: the device's radix select
restated in NumPy, which is no oracle of the reference, and the inputs both test files run."""
import numpy as np

INF = float("inf")


# ------------------------------------------------------------------------------------------------
# the radix select, restated in NumPy: the key transform and the four count / pick passes
# ------------------------------------------------------------------------------------------------
def keys_of(values):
    """Order-preserving uint32 keys of fp32 values: negative -> all bits flipped, else the sign bit set."""
    u = np.asarray(values, np.float32).reshape(-1).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def values_of(keys):
    k = np.asarray(keys, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def radix_select(values, q_lo, q_hi):
    """The device algorithm on one segment: four targets (ranks k, min(k + 1, n - 1) of q_lo and of q_hi), four
    passes of 8 bits; each pass histograms the byte of the keys that match a target's prefix (count) and moves
    the target into the bin that holds its remaining rank (pick). Returns (the four fp32 order statistics, the
    two fp64 bounds)."""
    keys = keys_of(values)
    n = keys.size
    if n == 0:
        return None, (-INF, INF)
    ranks = []
    for q in (q_lo, q_hi):
        k = int(np.floor(q * (n - 1)))
        ranks += [k, min(k + 1, n - 1)]
    prefix = [0, 0, 0, 0]
    for p in range(4):
        shift = 24 - 8 * p
        hi_mask = (0xFFFFFFFF << (32 - 8 * p)) & 0xFFFFFFFF if p else 0
        for t in range(4):
            match = ((keys ^ np.uint32(prefix[t])) & np.uint32(hi_mask)) == 0
            hist = np.bincount((keys[match] >> np.uint32(shift)) & np.uint32(255), minlength=256)
            inc = np.cumsum(hist)
            b = int(np.searchsorted(inc, ranks[t], side="right"))
            ranks[t] -= int(inc[b] - hist[b])
            prefix[t] |= b << shift
    v = values_of(np.array(prefix, np.uint32))
    out = []
    for q, (a, b) in ((q_lo, v[:2]), (q_hi, v[2:])):
        pos = q * (n - 1)
        frac = pos - np.floor(pos)
        a, b = np.float64(a), np.float64(b)
        out.append(a if frac == 0.0 or a == b else a + frac * (b - a))
    return v, tuple(out)


# ------------------------------------------------------------------------------------------------
# the cases both test files run: the select's inputs, the flagged minibatch's problems
# ------------------------------------------------------------------------------------------------
SELECT_KINDS = ("equal", "two-values", "kf4", "negative", "mixed-zeros", "low8", "high8")


def select_lengths(block, max_chunks):
    """1..1025 around the wave, workgroup and chunk edges, and one row past the count loop's second trip."""
    return [1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, 2 * block * max_chunks + 1]


def select_input(kind, n, seed=0):
    """(advantages fp32 [N], K_ft) whose first-n-positions segment has n rows."""
    kf = 4 if kind == "kf4" else 1
    N = -(-n // kf)
    rng = np.random.default_rng([seed, n, SELECT_KINDS.index(kind)])
    if kind == "equal":
        a = np.full(N, 1.25)
    elif kind == "two-values":
        a = rng.choice([-0.5, 2.0], N)
    elif kind == "negative":
        a = -np.abs(rng.normal(size=N)) - 0.1
    elif kind == "mixed-zeros":
        a = rng.normal(size=N)
        a[rng.random(N) < 0.2] = 0.0
        a[rng.random(N) < 0.2] = -0.0
    elif kind == "low8":      # 1.0 <= v < 1.00003: the first three passes see one bin
        a = (np.uint32(0x3F800000) | rng.integers(0, 256, N).astype(np.uint32)).view(np.float32)
    elif kind == "high8":     # sign and the exponent's top seven bits only (exponent <= 254: finite)
        a = ((rng.integers(0, 256, N).astype(np.uint32) << np.uint32(24)) | np.uint32(0x123456)).view(np.float32)
    else:
        a = rng.normal(size=N)
    return np.asarray(a, np.float32), kf


def select_quantiles(n):
    """(q_lo, q_hi) pairs: the ends, the median, 5 % / 95 %, a q whose pos is an exact integer and one just below."""
    qs = [(0.0, 1.0), (0.0, 0.5), (0.5, 1.0), (0.05, 0.95)]
    if n >= 4:
        k = (n - 1) // 2
        q = k / (n - 1)
        if q * (n - 1) == k:
            qs.append((q, 1.0))
        qb = np.nextafter(q, 0.0)
        if np.floor(qb * (n - 1)) == k - 1:
            qs.append((float(qb), 1.0))
    return qs


GRAD_Q = (0.1, 0.9)
# (label, precision, rows through a row_index, norm_adv)
GRAD_CASES = [("fp32-33", "fp32", 33, True), ("fp32-77", "fp32", 77, True), ("fp32-77-nonorm", "fp32", 77, False),
              ("bf16-33", "bf16", 33, True), ("bf16-77-nonorm", "bf16", 77, False)]


def grad_problem(precision, rows, norm_adv):
    """tests/test_update_surface_gpu.py's _Problem (hopper, 100 samples) on `rows` host-chosen rows (a row_index),
    with log-normal advantages (a heavy upper tail) when norm_adv is off."""
    from tests.helpers import HOPPER
    from tests.test_update_surface_gpu import _Problem
    p = _Problem(HOPPER, precision, n_samples=100)
    if not norm_adv:   # a symmetric clip of symmetric advantages leaves their mean, and so pg_loss, nearly alone
        p.adv = np.random.default_rng(5).lognormal(0.0, 1.0, p.N).astype(np.float32)
    rng = np.random.default_rng(rows)   # every row its own sample: no two rows share an advantage
    idx = rng.permutation(p.N)[:rows] * p.kf + rng.integers(0, p.kf, rows)
    p.row_index = idx.astype(np.int64)
    p.bi, p.di = idx // p.kf, idx % p.kf
    p.lp_old_rows = p.lp_old_ref[p.bi, p.di]
    return p
