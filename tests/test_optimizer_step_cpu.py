"""CPU proofs for tests/test_optimizer_step_gpu.py: the bounds of tests/helpers.py adamw_oracle are
neither too tight nor too loose, on the inputs the GPU tests use (step_inputs, STEP_HP, STEP_NUMBERS).

(a) A NumPy float32 emulation of adamw_elem (csrc/optimizer.hip) stays under HALF of every bound, in both
    operation orders (keras, torch), each without and with the multiply-adds the compiler may contract
    (an FMA = the float64 product-sum rounded once to float32).
(b) Each mistake of MUTATIONS moves at least one of p', m', v' past TEN times its bound on at least 1% of
    the elements ("the oracle moves"), at the cases listed with it. Where a mistake is only visible at
    some hyperparameters the reason is written next to the case list.
(c) The virtual l2 gradient read from the stepped W_out instead of the pre-step one misses by more than ten
    times the bound at the learning rates the l2-virtual GPU cases use.
(d) The accept / refuse table of the step against the host arithmetic of dppo_check_dims and the pack.
"""
import math

import numpy as np
import pytest

from tests.helpers import STEP_HP, STEP_NUMBERS, adamw_oracle, step_hp, step_inputs
from tests.test_optimizer_step_gpu import (CLIP_SCALES, FORMS, GEOMETRIES, PRECISIONS, REFUSED, RUNS, STEP_REST, STEP_TABLE,
                                           STEPS3_L2V, step_problem)

F = np.float32
N = 100003


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def emulate_adamw_elem(mode, p, m, v, g, step, raw, fma):
    """adamw_elem in float32, operation for operation, with make_adam_hp's alpha, bc1, bc2 (float64, rounded
    to float32 once); fma: every a * b + c the compiler may contract is one FMA."""
    lr, wd, b1, b2, eps = (F(x) for x in raw)
    bc1d, bc2d = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
    alpha, bc1, bc2 = F(float(lr) * math.sqrt(bc2d) / bc1d), F(bc1d), F(bc2d)
    one = F(1)
    if mode == "keras":
        if fma:
            p1 = _fma(-(p * wd), lr, p)
            m1 = _fma(g - m, one - b1, m)
            v1 = _fma(_fma(g, g, -v), one - b2, v)
        else:
            p1 = p - (p * wd) * lr
            m1 = m + (g - m) * (one - b1)
            v1 = v + (g * g - v) * (one - b2)
        p2 = p1 - (m1 * alpha) / (np.sqrt(v1) + eps)
    else:
        if fma:
            p1 = p * F(_fma(-lr, wd, one))
            m1 = _fma(b1, m, (one - b1) * g)
            v1 = _fma(b2, v, ((one - b2) * g) * g)
        else:
            p1 = p * (one - lr * wd)
            m1 = b1 * m + (one - b1) * g
            v1 = b2 * v + ((one - b2) * g) * g
        p2 = p1 - (lr * (m1 / bc1)) / (np.sqrt(v1 / bc2) + eps)
    assert p2.dtype == m1.dtype == v1.dtype == np.float32
    return p2, m1, v1


def _ratio(got, ref, bound):
    e = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(e == 0, 0.0, e / bound)


@pytest.mark.parametrize("fma", [False, True], ids=["mul-add", "fma"])
@pytest.mark.parametrize("hpname", list(STEP_HP))
@pytest.mark.parametrize("mode", ["keras", "torch"])
def test_emulation_stays_under_half_the_bound(mode, hpname, fma):
    """(a), at every step number of the GPU cases."""
    raw = STEP_HP[hpname]
    p, m, v, g = step_inputs(N, seed=N % 1000)
    worst = {}
    for step in STEP_NUMBERS:
        got = emulate_adamw_elem(mode, p, m, v, g, step, raw, fma)
        ref, bounds = adamw_oracle(mode, p, m, v, g, step, step_hp(*raw))
        worst[step] = [float(_ratio(a, r, b).max()) for a, r, b in zip(got, ref, bounds)]
    print({"case": f"emulation-{mode}-{hpname}-{'fma' if fma else 'mul-add'}", "ratio_p_m_v": worst})
    assert all(max(r) < 0.5 for r in worst.values()), worst


# ------------------------------------------------------------------------------------------------
# (b) the oracle moves
# ------------------------------------------------------------------------------------------------
def _step64(mode, p, m, v, g, step, hp, eps_in_sqrt=False, decay_after=False):
    """The oracle's step restated so that single mistakes can be switched on; with none it IS the oracle
    (asserted in test_restatement_is_the_oracle)."""
    p, m, v, g = (np.asarray(x, np.float64) for x in (p, m, v, g))
    lr, wd, b1, b2, eps = hp["lr"], hp["wd"], hp["beta1"], hp["beta2"], hp["eps"]
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    if mode == "keras":
        m1 = m + (g - m) * (1 - b1)
        v1 = v + (g * g - v) * (1 - b2)
        alpha = lr * math.sqrt(bc2) / bc1
        den = np.sqrt(v1 + eps) if eps_in_sqrt else np.sqrt(v1) + eps
        upd = (m1 * alpha) / den
        if decay_after:
            p1 = p - upd
            return p1 - p1 * wd * lr, m1, v1
        return (p - p * wd * lr) - upd, m1, v1
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + (1 - b2) * g * g
    den = np.sqrt(v1 / bc2 + eps) if eps_in_sqrt else np.sqrt(v1 / bc2) + eps
    upd = lr * (m1 / bc1) / den
    if decay_after:
        return (p - upd) * (1 - lr * wd), m1, v1
    return p * (1 - lr * wd) - upd, m1, v1


def _mut_eps_in_sqrt(mode, s, step, hp, raw):
    return _step64(mode, *s, step, hp, eps_in_sqrt=True)


def _mut_other_mode(mode, s, step, hp, raw):
    return _step64("torch" if mode == "keras" else "keras", *s, step, hp)


def _mut_decay_after(mode, s, step, hp, raw):
    return _step64(mode, *s, step, hp, decay_after=True)


def _mut_previous_step(mode, s, step, hp, raw):
    return _step64(mode, *s, step - 1, hp)


def _mut_beta2_double(mode, s, step, hp, raw):
    return _step64(mode, *s, step, dict(hp, beta2=float(raw[3])))


# name -> (the mistaken step, the (mode, hyperparameter set, step number) cases where it must show)
MUTATIONS = {
    "eps inside the square root": (_mut_eps_in_sqrt, [("keras", "default", 2), ("keras", "off", 2), ("torch", "off", 2)]),
    # eps and decay placement. The decay is the same real number in both modes (p - p wd lr = p (1 - lr wd)); the
    # eps differs by 1 / sqrt(1 - beta2^t), which the default eps = 1e-7 keeps under the bound: eps = 1e-3 shows it
    # while beta2^t is not yet 0 (at step 1000 of "off", 0.9^1000, the two modes are the same function)
    "keras versus torch placement": (_mut_other_mode, [("keras", "off", 2), ("torch", "off", 2), ("keras", "off", 1)]),
    # moves p' by update * wd * lr: 4e-7 |update| at the defaults (under C u), 1e-3 |update| at "off"
    "decay after the Adam update": (_mut_decay_after, [("keras", "off", 2), ("torch", "off", 2), ("keras", "off", 1000)]),
    "bias correction at step t - 1": (_mut_previous_step, [("keras", "default", 2), ("torch", "default", 2),
                                                            ("keras", "off", 2), ("keras", "default", 1000)]),
    # 1 - 0.999f differs from 0.001 by 1.3e-5 relative, v' with it; 0.9f from 0.9 by 2.4e-7 only ("off": nothing to see)
    "beta2 as the double 0.999": (_mut_beta2_double, [("keras", "default", 1), ("keras", "default", 2),
                                                      ("torch", "default", 2), ("keras", "default", 100000)]),
}
MUT_PARAMS = [(name, *case) for name, (_, cases) in MUTATIONS.items() for case in cases]


def _moved_fraction(mut, ref, bounds):
    """Fraction of elements where at least one of (p', m', v') differs by more than ten times its bound."""
    moved = np.zeros(ref[0].shape, bool)
    for a, r, b in zip(mut, ref, bounds):
        moved |= np.abs(a - r) > 10 * b
    return float(moved.mean())


def test_restatement_is_the_oracle():
    p, m, v, g = step_inputs(N, seed=N % 1000)
    for mode in ("keras", "torch"):
        for hpname, raw in STEP_HP.items():
            hp = step_hp(*raw)
            ref, _ = adamw_oracle(mode, p, m, v, g, 3, hp)
            for a, r in zip(_step64(mode, p, m, v, g, 3, hp), ref):
                np.testing.assert_allclose(a, r, rtol=1e-14, atol=0)


@pytest.mark.parametrize("name,mode,hpname,step", MUT_PARAMS, ids=[f"{n}-{m}-{h}-{s}".replace(" ", "_") for n, m, h, s in MUT_PARAMS])
def test_mutation_is_caught(name, mode, hpname, step):
    """(b): the mistake moves >= 1% of the elements past ten times the bound the GPU tests use."""
    raw = STEP_HP[hpname]
    hp = step_hp(*raw)
    s = step_inputs(N, seed=N % 1000)
    ref, bounds = adamw_oracle(mode, *s, step, hp)
    frac = _moved_fraction(MUTATIONS[name][0](mode, s, step, hp, raw), ref, bounds)
    print({"case": f"{name}-{mode}-{hpname}-{step}", "moved_fraction": frac})
    assert frac >= 0.01, frac


@pytest.mark.parametrize("mode", ["keras", "torch"])
def test_clip_after_the_moments_is_caught(mode):
    """(b), the clip scale applied after the moment update instead of before: m', v' from the raw gradient
    and the scale on the update, against the oracle on g * scale with the clipped step's gradient error."""
    raw = STEP_HP["default"]
    hp = step_hp(*raw)
    p, m, v, g = step_inputs(N, seed=N % 1000)
    scale = np.resize(CLIP_SCALES.astype(np.float64), N)      # every hand-written scale, some exactly 1
    ge = g.astype(np.float64) * scale
    ref, bounds = adamw_oracle(mode, p, m, v, ge, 2, hp, g_err=2.0 ** -24 * np.abs(ge))
    raw_step, _ = adamw_oracle(mode, p, m, v, g, 2, hp)
    p64 = p.astype(np.float64)
    mut = (p64 - p64 * hp["wd"] * hp["lr"] - scale * (p64 - p64 * hp["wd"] * hp["lr"] - raw_step[0]), raw_step[1], raw_step[2])
    below = scale < 1
    frac = _moved_fraction([a[below] for a in mut], [r[below] for r in ref], [b[below] for b in bounds])
    same = _moved_fraction([a[~below] for a in mut], [r[~below] for r in ref], [b[~below] for b in bounds])
    print({"case": f"clip-after-moments-{mode}", "moved_fraction_scaled": frac, "moved_fraction_scale1": same})
    assert frac >= 0.5 and same == 0.0 and below.mean() >= 0.01


# ------------------------------------------------------------------------------------------------
# (c) the virtual l2 gradient reads the pre-step W_out
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("geometry", ["hopper", "tiny", "h8a4"])
def test_l2_virtual_reads_the_old_w_out(geometry, precision):
    """At the l2-virtual cases' first (step, lr): the oracle stepped with the l2 gradient formed from the
    STEPPED W_out (a kernel whose W_out pass ran before the l2 elements read the image) differs from the
    oracle in m' or v' of l2_w and of l2_b by more than ten times the bound on >= 1% of their elements."""
    pb = step_problem(geometry, precision)
    sl = pb.range("actor")
    P, M, V, G = pb.P0[sl], pb.M0[sl], pb.V0[sl], pb.G0_l2v[sl]
    stepno, lr = STEPS3_L2V[0]
    hp = step_hp(lr, *STEP_REST)
    ge, gerr = pb.l2_virtual(P, G)
    ref, bounds = adamw_oracle("keras", P, M, V, ge, stepno, hp, g_err=gerr)
    ge2, _ = pb.l2_virtual(ref[0].astype(np.float32), G)
    late, _ = adamw_oracle("keras", P, M, V, ge2, stepno, hp)
    for t in ("actor.l2_w", "actor.l2_b"):
        o, k = pb.off[t]
        cut = slice(o, o + k)
        frac = _moved_fraction([a[cut] for a in late], [r[cut] for r in ref], [b[cut] for b in bounds])
        print({"case": f"l2v-late-w_out-{geometry}-{precision}-{t}", "moved_fraction": frac})
        assert frac >= 0.01, (t, frac)


# ------------------------------------------------------------------------------------------------
# (d) the accept / refuse table
# ------------------------------------------------------------------------------------------------
def _ksteps(width, kg):
    return ((width + kg - 1) // kg + 1) & ~1


def step_accepts(dims, precision):
    """The host arithmetic that decides whether the optimizer step runs (no launch): dppo_check_dims
    (csrc/api.hip), the pack's time tables (add_mlp_jobs) and the row tiles' fold that follows every actor pack
    and fused actor step (dppo_pack_rt_fold, csrc/pack.hip), and the tile step's table sizes (make_tile_step,
    csrc/optimizer.hip). The step kernels themselves take K, N and the k-steps as arguments."""
    xd, sd = dims["horizon_steps"] * dims["action_dim"], dims["cond_steps"] * dims["obs_dim"]
    td, h, hc = dims["time_dim"], dims["actor_hidden"], dims["critic_hidden"]
    ok = 4 <= td <= 64 and td % 2 == 0 and h % 128 == 0 and 128 <= h <= 512 and hc % 128 == 0 and 128 <= hc <= 512
    ok = ok and xd <= 32 and sd <= 64
    ok = ok and td <= 32                                        # row-tile fold: time_dim <= 32
    kg = 16 if precision == "fp32" else 32
    ok = ok and (precision == "fp32" or xd <= _ksteps(xd, kg) * kg // 2)   # rt_tfold_lok
    in_w = 4 * td * td + 3 * td                                 # the time MLP's elements: W_in's offset
    ok = ok and in_w % 4 == 0 and h % 8 == 0                    # 16-B aligned W_in / biases
    n_mats, n_copies, n_jobs = 4, 5, 12                         # TILE_MAXM 4, TILE_MAXC 8, FUSE_MAXJ 12
    return ok and n_mats <= 4 and n_copies <= 8 and n_jobs <= 12


def test_step_table_matches_host_arithmetic():
    for (geometry, precision), outcome in STEP_TABLE.items():
        assert (outcome == RUNS) == step_accepts(GEOMETRIES[geometry], precision), (geometry, precision)
        assert outcome in (RUNS, REFUSED)
    assert set(STEP_TABLE) == {(g, pr) for g in GEOMETRIES for pr in PRECISIONS}
    # the arithmetic can say no: an odd multiple of two for time_dim misaligns W_in, time_dim 64 has no fold
    hopper = GEOMETRIES["hopper"]
    assert not step_accepts(dict(hopper, time_dim=34), "bf16") and not step_accepts(dict(hopper, time_dim=64), "fp32")
    assert not step_accepts(dict(hopper, horizon_steps=11), "fp32")
    # every form's range is one the table's geometries have
    assert {f["net"] for f in FORMS.values()} == {"actor", "critic", "both"}
