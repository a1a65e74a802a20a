"""The behaviour-cloning term's oracle (tests/bc_cases.py), without a GPU: against finite differences of
coeff * O.bc_loss, the clip's shares on every GPU case's own inputs, how far the oracle moves under the term and
under the two mistakes a kernel could make, and the surface (ABI symbol, enum values, header table, cfg).
Every figure is printed as a JSON line before it is asserted."""
import json
import os
import re

import numpy as np
import pytest

from oracle import dppo_oracle as O
from tests import bc_cases as B
from tests.helpers import HOPPER, make_models, to_f64
from tests.variants import mish_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEFF = 0.1


@pytest.mark.parametrize("head", ["residual", "plain"])
@pytest.mark.parametrize("act", ["ReLU", "Mish"])
def test_oracle_matches_finite_differences(act, head):
    """Central differences of coeff * O.bc_loss along one seeded direction per gradient tensor, float64, the chains
    fixed (O.bc_loss samples them from the base actor, which does not move). h = 1e-7: the loss is piecewise smooth
    (ReLU units, the x_recon clip, the log-prob clip), and a unit that crosses zero inside +-h |x . v| bends the
    difference quotient; at h = 1e-6 a few of the 15,360 hidden units do along in_w's direction (7e-4 off) and at
    1e-7 none does. Cancellation is ~1e-16 |loss| / h = 1e-9 of derivatives of order 0.1, truncation far less, so
    1e-6 of the largest directional derivative holds; the 1e-6 margin of the log-probs to the clip's bounds is
    asserted first."""
    dims = dict(HOPPER, activation=act, head=head)
    model = O.Model.from_dims(dims)
    models = mish_models if act == "Mish" else make_models
    base, ft, _ = models(3, dims, ft_perturb=B.PERTURB)
    base, ft = to_f64(base), to_f64(ft)
    from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
    sched = ddpm_buffers(20)
    rng = np.random.default_rng(5)
    n, kf = 3, 10
    state = rng.uniform(-1, 1, (n, 1, 11))
    xT, z = rng.standard_normal((n, 4, 3)), rng.standard_normal((20, n, 4, 3))
    _, chains = O.sample(base, base, sched, state, xT, z, kf, round_h3=False, model=model)
    ref = B.bc_oracle(ft, sched, state, chains, kf, COEFF, model=model)
    lp = ref["lp"]
    np.testing.assert_array_equal(lp, O.get_logprobs(ft, sched, state, chains, kf, model=model))
    assert abs(ref["bc_loss"] - O.bc_loss(base, ft, sched, state, xT, z, kf, model=model)) < 1e-12
    near = float(np.minimum(np.abs(lp + 5), np.abs(lp - 2)).min())
    outside = float(((lp < -5) | (lp > 2)).mean())
    assert near > 1e-6 and outside > 0.05, (near, outside)
    loss = lambda p: COEFF * O.bc_loss(base, p, sched, state, xT, z, kf, model=model)
    h, out = 1e-7, {}
    for k, g in ref["grads"].items():
        v = rng.standard_normal(g.shape)
        plus, minus = dict(ft), dict(ft)
        plus[k], minus[k] = ft[k] + h * v, ft[k] - h * v
        out[k] = ((loss(plus) - loss(minus)) / (2 * h), float((g * v).sum()))
    scale = max(abs(a) for _, a in out.values())
    print(json.dumps({"case": f"fd-{act}-{head}", "near": near, "outside": outside, "fd_vs_oracle": out}))
    assert set(out) == set(k for k in ft if not (head == "plain" and k.startswith("l2_")))
    bad = {k: v for k, v in out.items() if not abs(v[0] - v[1]) <= 1e-6 * scale}
    assert not bad, bad


@pytest.mark.parametrize("label", list(B.CASES))
def test_inputs_put_the_clip_to_work(label):
    """On each GPU case's own inputs, from the oracle: a tenth to a half of the elements outside [-5, 2]; in fp32 (the
    float64 oracle) none within 1e-3 of either bound, so the mask cannot differ between GPU and oracle; the case at
    min_logprob_denoising_std 0.02 has at least 1 % above 2 (at 0.1 a log-prob cannot exceed -ln 0.1 - ln sqrt(2 pi)
    = 1.38)."""
    c = B.build(label)
    lo, hi, near = c.shares(c.oracle(COEFF)["lp"])
    print(json.dumps({"case": label, "below": lo, "above": hi, "near": near, "rows": c.n * c.kf}))
    assert 0.1 <= lo + hi <= 0.5 and near >= 1e-3, (lo, hi, near)
    if c.min_logprob_std == 0.02:
        assert hi >= 0.01, hi
    else:
        assert hi == 0.0


def test_oracle_moves():
    """coeff = 0.1 moves every actor gradient tensor of a 40-row PPO minibatch (the term over its own 40 rows'
    observations, one chain each) by at least ten times the GPU bound of the cases that check the term on top of a
    PPO minibatch (fp32: the accumulate and c_loss cases, 2e-3); dropping the clip's mask or taking
    [:, :reward_horizon] (2 of 4 steps here) moves the term's own gradient by ten times the largest bound of its
    own cases (1e-2). Measured: 0.08 .. 0.13 for the term, 5.7 .. 11.5 and 0.55 .. 0.89 for the two mistakes.
    The term's movement (0.08 .. 0.13) is under ten times the 2-byte bound (0.1) for most tensors: no 2-byte test
    checks the term ON TOP of a PPO minibatch against an oracle (the 2-byte cases check the term's own gradient,
    and the accumulate case compares two GPU results), so no 2-byte check rests on this sensitivity."""
    c = B.build("rows40", n=40)
    kf, rows = c.kf, 40
    rng = np.random.default_rng(9)
    ft = to_f64(c.ft)
    _, _, critic = make_models(0, HOPPER)
    j = np.arange(rows) % kf
    chains = rng.standard_normal((rows, kf + 1, 4, 3)) * 0.5
    lp = O.get_logprobs(ft, c.sched, c.state, chains, kf).reshape(rows, kf, 4, 3)
    r = np.arange(rows)
    old = np.clip(lp[r, j], -5, 2).mean(axis=(1, 2))
    _, ga, _ = O.c_loss(ft, to_f64(critic), c.sched, c.state, chains[r, j], chains[r, j + 1], j, rng.normal(size=rows),
                        None, rng.normal(size=rows), old, kf)
    full = c.oracle(COEFF)["grads"]
    moved = {k: B.rel(ga[k] + full[k], ga[k]) for k in ga}
    nomask = c.oracle(COEFF, mask=False)["grads"]
    hor = c.oracle(COEFF, horizon=2)["grads"]
    m1 = {k: B.rel(nomask[k], full[k]) for k in full}
    m2 = {k: B.rel(hor[k], full[k]) for k in full}
    print(json.dumps({"case": "oracle-moves", "ppo_plus_bc": moved, "no_mask": m1, "horizon": m2}))
    for name, errs, need in (("ppo+bc", moved, 10 * B.GRAD_TOL["fp32"]), ("no mask", m1, 10 * max(B.GRAD_TOL.values())),
                             ("horizon", m2, 10 * max(B.GRAD_TOL.values()))):
        bad = {k: v for k, v in errs.items() if not v >= need}
        assert not bad, (name, bad)


@pytest.mark.parametrize("precision,limit", [("fp32", 14700), ("bf16", 29000), ("fp16", 29000)])
def test_chunk_choice_at_the_reference_batch(precision, limit):
    """ops.bc_chunk (host arithmetic over dppo_ppo_workspace_bytes) at hopper's geometry: a 50,000-row minibatch
    (the reference's batch_size: 500,000 BC rows, past the entry's 2 GiB workspace limit at about `limit` samples)
    is walked in even chunks whose workspace stays inside the budget; a minibatch that fits runs as one call;
    PPODiffusion.bc_grad and the agent take their chunk from here."""
    import inspect
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.agent.finetune import train_ppo_diffusion_agent as A
    from diffusionpolicyoptimization_amd.model.diffusion.diffusion_ppo import PPODiffusion
    d = ops.ModelDims(**HOPPER)
    kf = d.ft_denoising_steps
    bytes_of = lambda s: ops._workspace_bytes(d, ops._prec(precision), s * kf)
    assert bytes_of(limit) < (1 << 31) <= bytes_of(int(limit * 1.05)), (bytes_of(limit), bytes_of(int(limit * 1.05)))
    out = {}
    for n in (50000, 6250, 49999, 320, 1):
        c = ops.bc_chunk(d, precision, n)
        calls = -(-n // c)
        out[n] = (c, calls, bytes_of(c))
        assert 1 <= c <= n and bytes_of(c) <= ops.BC_WORKSPACE_BYTES < (1 << 31), (n, c)
        assert (c == n) == (bytes_of(n) <= ops.BC_WORKSPACE_BYTES)
        if c < n:   # the fewest calls that fit, evenly shared
            assert c == -(-n // calls) and bytes_of(-(-n // (calls - 1))) > ops.BC_WORKSPACE_BYTES, (n, c, calls)
    print(json.dumps({"case": f"bc-chunk-{precision}", "n -> (chunk, calls, workspace bytes)": out}))
    assert out[50000][1] > 1 and out[320][1] == 1
    small = ops.bc_chunk(d, precision, 50000, budget=bytes_of(100))   # rows pad to 64: a few more samples may fit
    assert 90 <= small <= 106 and bytes_of(small) <= bytes_of(100)
    with pytest.raises(ValueError):
        ops.bc_chunk(d, precision, 50000, budget=1 << 31)
    with pytest.raises(ValueError):
        ops.bc_chunk(d, precision, 10, budget=1024)
    assert "ops.bc_chunk(self.dims, self.precision, n) if chunk is None" in inspect.getsource(PPODiffusion.bc_grad)
    src = inspect.getsource(A.TrainPPODiffusionAgent._enqueue_unsplit)
    assert "ops.bc_chunk(m.dims, m.precision, rows_full)" in src and "chunk=chunk" in src


def test_surface():
    """The ABI symbol with its signature, the enum values on both sides, the header's accept / refuse table, the
    cfg, and the Python entry points."""
    from diffusionpolicyoptimization_amd import _lib, ops
    from diffusionpolicyoptimization_amd.model.diffusion.diffusion_ppo import M_BC, PPODiffusion
    from diffusionpolicyoptimization_amd.util.config import load_config
    assert "dppo_bc_minibatch" in _lib.EXPORTED_SYMBOLS and len(_lib._SIGNATURES["dppo_bc_minibatch"][1]) == 17
    assert _lib.load().dppo_bc_minibatch is not None and _lib.load().dppo_abi_version() == 15
    hdr = open(os.path.join(ROOT, "include", "dppo.h")).read()
    assert re.search(r"enum \{ DPPO_METRIC_BC_LOGPROB = (\d+) \}", hdr).group(1) == str(_lib.DPPO_METRIC_BC_LOGPROB) == "9"
    assert re.search(r"enum \{ DPPO_BC_ACCUMULATE = (\d+) \}", hdr).group(1) == str(_lib.DPPO_BC_ACCUMULATE) == "16"
    assert M_BC == 9
    for row in ("dppo_bc_minibatch: null pointer", "dppo_bc_minibatch: n < 1", "dppo_bc_minibatch: global_samples < n",
                "dppo_bc_minibatch: coeff must be >= 0", "dppo_bc_minibatch: DPPO_PPO_LEARN_ETA is not supported",
                "dppo_bc_minibatch: unknown flags 0x%x", "actor row tile needs %zu B LDS", "DPPO_API int dppo_bc_minibatch("):
        assert row in hdr, row
    assert callable(ops.bc_minibatch) and callable(PPODiffusion.bc_grad)
    # the default coefficient and the constructor's refusals, from the sources (building either needs a device;
    # tests/test_bc_grad_gpu.py builds them)
    import inspect
    from diffusionpolicyoptimization_amd.agent.finetune.train_ppo_diffusion_agent import TrainPPODiffusionAgent
    assert re.search(r"self\.bc_loss_coeff = 0\.0\n", inspect.getsource(PPODiffusion.__init__))
    init = inspect.getsource(TrainPPODiffusionAgent.__init__)
    for cond in ("if self.bc_loss_coeff < 0:", "if self.bc_loss_coeff > 0 and not self.use_bc_loss:",
                 "if self.bc_loss_coeff > 0 and self.learn_eta:"):
        assert cond + "\n            raise ValueError(" in init, cond
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp_bc", [])
    base = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp", [])
    assert cfg.train.use_bc_loss is True and cfg.train.bc_loss_coeff == 0.1
    assert base.train.get("bc_loss_coeff", 0) == 0 and not base.train.get("use_bc_loss", False)
