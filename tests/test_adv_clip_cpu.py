"""The advantage clip without a GPU: the knobs' refusals, the cfg, the ABI surface, the select's key transform
and its four passes restated in NumPy, and the proof that the GPU gradient cases can fail (the oracle with
quantiles (0.1, 0.9) against (0, 1) on their inputs)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import adv_clip_cases as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dppo_ppo_adv_quantiles_workspace_bytes", "dppo_ppo_adv_quantiles_all", "dppo_ppo_adv_quantiles_count",
               "dppo_ppo_adv_quantiles_pick")


@pytest.mark.parametrize("q", [(0.5, 0.5), (0.9, 0.1), (-0.01, 0.9), (0.1, 1.01), (float("nan"), 0.9), (0.1, float("nan"))])
def test_constructor_refuses_bad_quantiles(q):
    """0 <= q_lo < q_hi <= 1 or ValueError, before anything is built (no device, no other argument is read)."""
    from diffusionpolicyoptimization_amd.model.diffusion.diffusion_ppo import PPODiffusion
    with pytest.raises(ValueError, match="clip_advantage_lower_quantile"):
        PPODiffusion(0.99, 0.01, clip_advantage_lower_quantile=q[0], clip_advantage_upper_quantile=q[1])


def test_ops_refuse_bad_quantiles():
    from diffusionpolicyoptimization_amd import ops
    for q in [(0.5, 0.5), (0.9, 0.1), (-0.01, 0.9), (0.1, 1.01), (float("nan"), 0.9)]:
        with pytest.raises(ValueError):
            ops._check_quantiles(*q)
    ops._check_quantiles(0, 1)
    ops._check_quantiles(0.05, 0.95)


def test_cfg_loads():
    from diffusionpolicyoptimization_amd.util.config import load_config
    root = os.path.join(ROOT, "cfg/gym/finetune/hopper-v2")
    cfg, base = load_config(root, "ft_ppo_diffusion_mlp_advclip", []), load_config(root, "ft_ppo_diffusion_mlp", [])
    assert (cfg.model.clip_advantage_lower_quantile, cfg.model.clip_advantage_upper_quantile) == (0.05, 0.95)
    assert "clip_advantage_lower_quantile" not in base.model
    assert cfg.train.batch_size == base.train.batch_size and cfg.model.actor == base.model.actor


def test_header_declares_and_library_exports_the_new_surface():
    from diffusionpolicyoptimization_amd import _lib
    src = open(os.path.join(ROOT, "include", "dppo.h")).read()
    declared = set(re.findall(r"DPPO_API\s+[\w\s\*]+?\b(dppo_\w+)\s*\(", src))
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(dppo_\w+)\b", nm))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and name in exported, name
    assert declared == set(_lib.EXPORTED_SYMBOLS) == exported
    consts = dict(re.findall(r"\b(DPPO_PPO_ADV_CLIP|DPPO_ADV_QUANTILES_BLOCK|DPPO_ADV_QUANTILES_MAX_CHUNKS) = (\d+)", src))
    assert {k: int(v) for k, v in consts.items()} == {
        "DPPO_PPO_ADV_CLIP": _lib.DPPO_PPO_ADV_CLIP, "DPPO_ADV_QUANTILES_BLOCK": _lib.DPPO_ADV_QUANTILES_BLOCK,
        "DPPO_ADV_QUANTILES_MAX_CHUNKS": _lib.DPPO_ADV_QUANTILES_MAX_CHUNKS}
    # a flag bit of its own, and the struct it travels in is the one ABI 15 had
    others = (_lib.DPPO_PPO_L2_DEFERRED, _lib.DPPO_PPO_LEARN_ETA, _lib.DPPO_PPO_PRECLEARED)
    assert all(_lib.DPPO_PPO_ADV_CLIP & o == 0 for o in others) and lib.dppo_abi_version() == 15
    import ctypes
    assert ctypes.sizeof(_lib.DppoPpoHparams) == 56
    from diffusionpolicyoptimization_amd import ops
    assert ops.ppo_hparams().flags == 0 and ops.ppo_hparams(adv_clip=True).flags == _lib.DPPO_PPO_ADV_CLIP
    assert _lib.query("dppo_ppo_adv_quantiles_workspace_bytes", 5, 6) == 30 * (4096 + 72)
    assert _lib.query("dppo_ppo_adv_quantiles_workspace_bytes", 0, 6) == 0


def test_key_transform_is_monotone():
    """v < w <=> key(v) < key(w) on a sorted table with -inf, -max, negative denormals, -0, +0, denormals, the
    neighbours of 1 and +inf; -0 and +0 (equal as values) get adjacent keys; the inverse restores the bits."""
    f = np.float32
    tiny, big = np.finfo(f).smallest_subnormal, np.finfo(f).max
    table = np.array([-np.inf, -big, -1.0, np.nextafter(f(-1), f(0)), -np.finfo(f).tiny, -2 * tiny, -tiny, -0.0, 0.0, tiny,
                      2 * tiny, np.finfo(f).tiny, np.nextafter(f(1), f(0)), 1.0, np.nextafter(f(1), f(2)), big, np.inf], f)
    assert np.all(np.diff(table.astype(np.float64)) >= 0)
    keys = AO.keys_of(table).astype(np.int64)
    assert np.all(np.diff(keys) > 0), keys
    z = int(np.flatnonzero(np.signbit(table) & (table == 0))[0])
    assert keys[z + 1] - keys[z] == 1 and keys[z] - keys[z - 1] == 1 and keys[z + 2] - keys[z + 1] == 1
    assert np.array_equal(AO.values_of(AO.keys_of(table)).view(np.uint32), table.view(np.uint32))
    rnd = np.random.default_rng(0).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32).view(f)
    rnd = rnd[np.isfinite(rnd)]
    o = np.argsort(AO.keys_of(rnd), kind="stable")
    assert np.all(np.diff(rnd[o].astype(np.float64)) >= 0)


@pytest.mark.parametrize("kind", AO.SELECT_KINDS)
def test_numpy_passes_equal_numpy_quantile(kind):
    """The four count / pick passes in NumPy on the GPU select cases' own inputs: the order statistics are
    np.sort's, the bounds the definition's bit for bit, and np.quantile's. numpy forms the position as
    (n q + (1 - q)) - 1, not q (n - 1), and interpolates from either end, so against it the bound is what one
    rounding of the position and of the product can move: 4 eps (|pos| + 1) |v_k1 - v_k| + 4 eps |Q|."""
    eps = np.finfo(np.float64).eps
    from diffusionpolicyoptimization_amd import _lib
    for n in AO.select_lengths(_lib.DPPO_ADV_QUANTILES_BLOCK, _lib.DPPO_ADV_QUANTILES_MAX_CHUNKS):
        adv, kf = AO.select_input(kind, n)
        vals = np.repeat(adv, kf)[:n]
        for q_lo, q_hi in AO.select_quantiles(n):
            sel, got = AO.radix_select(vals, q_lo, q_hi)
            for i, q in enumerate((q_lo, q_hi)):
                _, k, k1, vk, vk1 = O.order_stats(vals, q)
                assert sel[2 * i] == vk and sel[2 * i + 1] == vk1
                assert got[i] == O.quantile(vals, q) or (q * (n - 1)) % 1 == 0
                ref = np.quantile(vals.astype(np.float64), q)
                assert abs(got[i] - ref) <= 4 * eps * ((q * (n - 1) + 1) * abs(vk1 - vk) + abs(ref)), (kind, n, q, got[i], ref)


@pytest.mark.parametrize("label,precision,rows,norm_adv", AO.GRAD_CASES, ids=[c[0] for c in AO.GRAD_CASES])
def test_the_clip_moves_what_the_gpu_cases_compare(label, precision, rows, norm_adv):
    """On each GPU gradient case's inputs the oracle at quantiles (0.1, 0.9) and at (0, 1) differ in pg_loss and
    in every actor gradient tensor by at least ten times the bound the GPU case asserts; at least a tenth of
    the rows are clamped on each side; no advantage lies within 1e-6 (relative) of a bound, so the fp32 clamp
    and the float64 one pick the same rows. Quantiles (0, 1) are the oracle without the clip."""
    from tests.test_update_surface_gpu import TOL, _assert_moved
    p = AO.grad_problem(precision, rows, norm_adv)
    tol, ratio1 = TOL[precision], p.kind == "ratio1"
    ref0 = p.oracle(norm_adv=norm_adv)
    same = p.oracle(norm_adv=norm_adv, adv_clip_quantiles=(0.0, 1.0))
    assert same[0] == ref0[0] and all(np.array_equal(same[1][k], ref0[1][k]) for k in ref0[1])
    ref = p.oracle(norm_adv=norm_adv, adv_clip_quantiles=AO.GRAD_Q)
    _assert_moved(ref, ref0, ("pg_loss", "actor"), tol, ratio1, label=label)
    assert ref[0]["v_loss"] == ref0[0]["v_loss"] and all(np.array_equal(ref[2][k], ref0[2][k]) for k in ref0[2])
    a = p.adv[p.bi].astype(np.float64)
    lo, hi = O.bounds(a, *AO.GRAD_Q)
    below, above = float((a < lo).mean()), float((a > hi).mean())
    gap = float(min(np.abs(a - lo).min() / abs(lo), np.abs(a - hi).min() / abs(hi)))
    print(json.dumps({"case": label, "clamped_below": below, "clamped_above": above, "nearest_rel_gap": gap,
                      "pg_loss": (ref[0]["pg_loss"], ref0[0]["pg_loss"])}))
    assert below >= 0.1 and above >= 0.1 and gap > 1e-6
