"""The update's loss hyperparameters and model geometry against the float64 oracle.

The other GPU files run the update at the shipped hopper / walker configs only, where several terms
of the PPO loss multiply by zero or slice nothing and several compiled kernel paths never launch.
Part A moves every hyperparameter of dppo_ppo_hparams (and dppo_gae's) off its default, one per case;
part B runs the four update entries (dppo_logprob, dppo_critic_forward, dppo_ppo_minibatch,
dppo_pretrain_minibatch) at geometries that reach the remaining instantiations, or pins that a
geometry without one is rejected cleanly.

Shapes are test_ppo_minibatch_grads': 40 samples, 150 rows from permutation position 37 (several row
tiles plus a ragged tail), the Feistel permutation of oracle.philox, critic_dedup = _dedup(bi).
K' = 1 needs 200 samples (150 rows from position 37 of 40 would run past the permutation).
Error measure: per gradient tensor max|g - ref| / (max|ref| + 1e-12). Every figure is printed before
it is asserted (pytest -s shows them).

Bounds (test_ppo_minibatch_grads', test_logprob's, test_critic_forward's, test_pretrain_loss_grads'):
fp32 'perturbed' 2e-3; bf16 / fp16 'ratio1' against the oracle rounding at the kernels' rounding
points 1e-2; approx_kl ten times those; clipfrac 0 at ratio 1, else 0.02.

Each part-A case proves on the CPU that it can fail: the oracle at the case's hyperparameters and at
the defaults, on the same inputs, must differ in the quantities the case is meant to move by at
least ten times the bound used against the kernel (_assert_moved).

Accept / reject table of the update entries (read from csrc/rowtile.hip dispatch_actor /
dispatch_critic; validate_dims, csrc/api.hip, is wider). "in" = x + time embedding + conditioning
width; an actor rejection fails dppo_logprob, dppo_pretrain_minibatch and dppo_ppo_minibatch, a critic
rejection dppo_critic_forward and dppo_ppo_minibatch (which reports the actor's first):

  geometry                                   fp32 actor  fp32 critic  2-byte actor  2-byte critic
  ft_denoising_steps 1 / 7 / 16 (K = 20)     runs        runs         runs          runs
  time_dim 32 (in = 55)                      runs        runs         runs          runs
  actor_hidden 256                           REJECTED    runs         runs (NT=2)   runs
  cond_steps 2, hopper (SD 22, in = 50)      runs        runs         runs          runs
  cond_steps 2, walker (SD 34, in = 74)      REJECTED    REJECTED     runs (KSI=4)  runs
  horizon 8 x action 3 (XD 24), r.horizon 4  runs        runs         runs          runs
  horizon 8 x action 4 (XD 32)               runs        runs         runs          runs
  obs 3, action 1 (in = 23)                  REJECTED    runs         runs (KSI=2)  runs
  critic_hidden 128 / 384 / 512              runs        REJECTED     runs          REJECTED
  actor_hidden 128 / 384                     REJECTED    runs         REJECTED      runs

i.e. fp32 actor: hidden 512 and 33..64 inputs; 2-byte actor: hidden 256 or 512 and up to 128 inputs;
critic: hidden 256, conditioning width <= 32 (fp32) or <= 64 (2-byte); K' <= 16; XD <= 32.
"""
import json

import numpy as np
import pytest

from oracle import dppo_oracle as O
from oracle import philox as PX
from tests.helpers import HOPPER, WALKER, make_models, to_f64
from tests.test_kernels_gpu import _dedup, _rnd

pytestmark = pytest.mark.gpu

SEED, EPOCH, START, ROWS, NSAMP = 99, 1, 37, 150, 40
TOL = {"fp32": 2e-3, "bf16": 1e-2, "fp16": 1e-2}
LP_KIND = {"fp32": "perturbed", "bf16": "ratio1", "fp16": "ratio1"}
DEFAULTS = dict(gamma_denoising=0.99, clip_ploss_coef=0.01, clip_ploss_coef_base=0.01, clip_ploss_coef_rate=3.0,
                min_logprob_std=0.1, vf_coef=0.5, norm_adv=True, reward_horizon=4)
METRIC_SLOT = {"pg_loss": 0, "v_loss": 1, "approx_kl": 2, "clipfrac": 3, "ratio": 4}


# ------------------------------------------------------------------------------------------------
# the minibatch problem: CPU half (inputs, oracle) and GPU half (launch, comparison)
# ------------------------------------------------------------------------------------------------
class _Problem:
    """test_ppo_minibatch_grads' inputs for (dims, precision) and the oracle on them; no GPU needed.
    lp_hp: the hyperparameters the old log-probs were taken with (min_logprob_std, reward_horizon), as
    the agent's old-log-prob pass uses the update's. adv: (loc, scale) of the advantages' normal."""

    def __init__(self, dims, precision, n_samples=NSAMP, adv=(0.0, 1.0), lp_hp=None):
        from diffusionpolicyoptimization_amd import ops
        from diffusionpolicyoptimization_amd.model.diffusion.sampling import ddpm_buffers
        self.dims, self.precision, self.N = dims, precision, n_samples
        self.d = d = ops.ModelDims(**dims)
        self.model = O.Model.from_dims(dims)
        self.base, self.ft, self.critic = make_models(0, dims)
        self.sched = ddpm_buffers(d.denoising_steps)
        self.kf = kf = d.ft_denoising_steps
        self.total = n_samples * kf
        assert START + ROWS <= self.total
        rng = np.random.default_rng(12)
        self.obs = rng.uniform(-1, 1, (n_samples, d.sd)).astype(np.float32)
        self.chains = (rng.standard_normal((n_samples, kf + 1, d.xd)) * 0.5).astype(np.float32)
        self.adv = (adv[0] + adv[1] * rng.normal(size=n_samples)).astype(np.float32)
        self.ret = rng.normal(size=n_samples).astype(np.float32)
        self.lp_hp = dict(dict(min_logprob_std=0.1, reward_horizon=4), **(lp_hp or {}))
        self.lp_ref = O.get_logprobs(to_f64(self.ft), self.sched, self.state(self.obs), self.x(self.chains, kf + 1), kf,
                                     min_logprob_std=self.lp_hp["min_logprob_std"], rnd=_rnd(precision), model=self.model)
        H = min(self.lp_hp["reward_horizon"], d.horizon_steps)
        self.lp_ref_mean = np.clip(self.lp_ref, -5, 2)[:, :H].mean(axis=(1, 2)).reshape(n_samples, kf)
        self.kind = LP_KIND[precision]
        if self.kind == "perturbed":
            self.lp_old = (self.lp_ref_mean + rng.normal(0, 0.02, (n_samples, kf))).astype(np.float32)
            self.lp_old_ref = self.lp_old.astype(np.float64)
        else:                 # ratio 1: each side its own policy's log-probs (the GPU's from dppo_logprob)
            self.lp_old = None
            self.lp_old_ref = self.lp_ref_mean
        perm = PX.feistel_permute(np.arange(START, START + ROWS), self.total, SEED, EPOCH)
        self.bi, self.di = perm // kf, perm % kf
        self.lp_old_rows = self.lp_old_ref[self.bi, self.di]
        if kf == 1 and self.kind == "ratio1":
            # K' = 1 has zero clip width (cc = j = 0), so clipfrac counts every ratio that is not exactly 1:
            # the reference's old log-probs must be bit-identical to its new ones, i.e. come from a forward
            # of the minibatch's rows in c_loss's order (the forward over all samples above sums in another
            # BLAS blocking, ~1e-16 away, which made clipfrac of the reference alone 0.07)
            bi = self.bi
            lp = O.get_logprobs(to_f64(self.ft), self.sched, self.state(self.obs[bi]), self.x(self.chains[bi], 2), 1,
                                min_logprob_std=self.lp_hp["min_logprob_std"], rnd=_rnd(precision), model=self.model)
            self.lp_old_rows = np.clip(lp, -5, 2)[:, :H].mean(axis=(1, 2))

    def state(self, obs):
        return obs.reshape(obs.shape[0], self.d.cond_steps, self.d.obs_dim).astype(np.float64)

    def x(self, a, steps=None):
        d = self.d
        sh = (a.shape[0],) + ((steps,) if steps else ()) + (d.horizon_steps, d.action_dim)
        return a.reshape(sh).astype(np.float64)

    def oracle(self, **hp):
        """O.c_loss on the minibatch's rows, for the networks the dims describe; hp: c_loss keywords over DEFAULTS
        (adv_mean_std, denom, adv_clip_quantiles, caches, another model too)."""
        bi, di = self.bi, self.di
        kw = {**DEFAULTS, "model": self.model, **hp}
        return O.c_loss(to_f64(self.ft), to_f64(self.critic), self.sched, self.state(self.obs[bi]),
                        self.x(self.chains[bi, di]), self.x(self.chains[bi, di + 1]), di, self.ret[bi].astype(np.float64),
                        None, self.adv[bi].astype(np.float64), self.lp_old_rows, self.kf, rnd=_rnd(self.precision),
                        critic_dedup=_dedup(bi), **kw)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / (np.abs(np.asarray(b)).max() + 1e-12))


def _metric_bound(key, ref, tol, ratio1):
    """The bound test_ppo_minibatch_grads puts on a metric (the ratio mean: pg_loss's form)."""
    if key == "approx_kl":
        return tol * 10 * (abs(ref) + 1e-4)
    if key == "clipfrac":
        return 0.0 if ratio1 else 0.02
    return tol * (abs(ref) + 1e-2)


def _assert_moved(case, other, moves, tol, ratio1, scale=1.0, label=""):
    """The oracle results `case` and `other` ((metrics, actor grads, critic grads); other's gradients
    times `scale`) differ by >= 10x the kernel's bound in every quantity of `moves`: metric names,
    'actor' / 'critic' (every gradient tensor of the network)."""
    (mc, gac, gcc), (mo, gao, gco) = case, other
    for key in moves:
        if key in ("actor", "critic"):
            gc_, go_ = (gac, gao) if key == "actor" else (gcc, gco)
            diffs = {k: _rel(go_[k] * scale, gc_[k]) for k in gc_}
            assert all(v >= 10 * tol for v in diffs.values()), (label, key, diffs)
        else:
            bound = _metric_bound(key, mc[key], tol, ratio1)
            assert abs(mc[key] - mo[key]) >= 10 * bound and mc[key] != mo[key], (label, key, mc[key], mo[key])


class _Gpu:
    """The device half of a _Problem: images, tensors, the old log-probs of a 'ratio1' case."""

    def __init__(self, p, cuda):
        import torch
        from diffusionpolicyoptimization_amd import ops
        self.p, self.cuda = p, cuda
        d = p.d
        self.T = T = lambda x: torch.tensor(x, device=cuda)
        self.tab = T(ops.sched_table(p.sched))
        self.pf = T(ops.flatten_params(ops.actor_param_spec(d), p.ft))
        self.pc = T(ops.flatten_params(ops.critic_param_spec(d), p.critic))
        self.packf = ops.pack_actor(d, self.pf, p.precision)
        self.packc = ops.pack_critic(d, self.pc, p.precision)
        self.na, self.nc = ops.spec_count(ops.actor_param_spec(d)), ops.spec_count(ops.critic_param_spec(d))
        self.obs, self.chains = T(p.obs), T(p.chains)
        if p.kind == "perturbed":
            self.lp_old = T(p.lp_old)
        else:
            _, self.lp_old = ops.logprob(d, p.precision, self.packf, self.tab, self.obs, self.chains, want_elem=False,
                                         **p.lp_hp)

    def minibatch(self, fill=0.0, adv_stats=None, **hp):
        """One dppo_ppo_minibatch over the problem's rows -> (metric sums, gradient, the two output
        tensors); hp: ops.ppo_hparams keywords (global_rows defaults to the rows)."""
        import torch
        from diffusionpolicyoptimization_amd import ops
        p, d = self.p, self.p.d
        grads = torch.full((self.na + self.nc,), fill, dtype=torch.float32, device=self.cuda)
        metrics = torch.full((16,), fill, dtype=torch.float64, device=self.cuda)
        ws = ops.ppo_workspace(d, p.precision, ROWS, self.cuda)
        hpc = ops.ppo_hparams(**dict(dict(global_rows=ROWS), **hp))
        self.out = (grads, metrics)
        ops.ppo_minibatch(d, p.precision, hpc, self.packf, self.packc, self.pf, self.tab, self.obs, self.chains,
                          self.lp_old, self.T(p.adv), self.T(p.ret), SEED, EPOCH, START, ROWS, ws, grads, metrics,
                          adv_stats=adv_stats)
        torch.cuda.synchronize()
        return metrics.cpu().numpy(), grads.cpu().numpy()

    def split(self, g):
        from diffusionpolicyoptimization_amd import ops
        d = self.p.d
        return (ops.unflatten_params(ops.actor_param_spec(d), g[:self.na]),
                ops.unflatten_params(ops.critic_param_spec(d), g[self.na:]))


def _compare(label, gpu, m_sums, g, ref, tol, denom=ROWS, grad_scale=1.0):
    """test_ppo_minibatch_grads' assertions plus the ratio mean: metric sums / denom and every gradient
    tensor against the oracle's (its gradients times grad_scale). Returns the per-tensor errors."""
    mref, ga_ref, gc_ref = ref
    ratio1 = gpu.p.kind == "ratio1"
    m = m_sums / denom
    ga, gc = gpu.split(g)
    errs = {k: _rel(ga[k], r * grad_scale) for k, r in ga_ref.items()}
    errs.update({"critic." + k: _rel(gc[k], r * grad_scale) for k, r in gc_ref.items()})
    mets = {k: (float(m[s]), float(mref[k])) for k, s in METRIC_SLOT.items()}
    print(json.dumps({"case": label, "metrics": mets, "max_err": max(errs.values()), "errs": errs}))
    for k, (got, want) in mets.items():
        assert abs(got - want) <= _metric_bound(k, want, tol, ratio1), (label, k, got, want)
    bad = {k: v for k, v in errs.items() if not v < tol}
    assert not bad, (label, bad, errs)
    return errs


# ------------------------------------------------------------------------------------------------
# A. hyperparameter cases (hopper dims)
# ------------------------------------------------------------------------------------------------
# name -> (hyperparameters, what the oracle must move against the defaults, _Problem keywords)
BOTH = ("fp32", "bf16")
HP_CASES = {
    # clip width per denoising step j: base + (coef - base) (exp(rate j / 9) - 1) / (exp(rate) - 1); the
    # old-log-prob noise N(0, 0.02) puts |ratio - 1| on both sides of it across j. fp32 only: at ratio 1
    # (the 2-byte cases) every row is inside any clip width and nothing can move
    "clip-rate3": (dict(clip_ploss_coef=0.1, clip_ploss_coef_base=0.001, clip_ploss_coef_rate=3.0),
                   ("pg_loss", "clipfrac", "actor"), {}, ("fp32",)),
    "clip-rate1": (dict(clip_ploss_coef=0.1, clip_ploss_coef_base=0.001, clip_ploss_coef_rate=1.0),
                   ("pg_loss", "clipfrac", "actor"), {}, ("fp32",)),
    "reward-horizon1": (dict(reward_horizon=1), ("actor",), dict(lp_hp=dict(reward_horizon=1)), BOTH),
    "reward-horizon2": (dict(reward_horizon=2), ("actor",), dict(lp_hp=dict(reward_horizon=2)), BOTH),
    # 8 > horizon_steps clamps to the row: the reference equals the defaults' by construction (nothing to
    # move); a kernel that did not clamp would average over 24 of a row's 12 elements
    "reward-horizon8": (dict(reward_horizon=8), (), dict(lp_hp=dict(reward_horizon=8)), BOTH),
    "no-norm-adv": (dict(norm_adv=False), ("pg_loss", "actor"), dict(adv=(0.7, 2.5)), BOTH),
    # fp32 only: against 0.99 a row's discount moves by at most 1 - 0.99^9 = 8.6%, the gradients by ~5%,
    # under ten times the bf16 bound (10%) whatever the inputs; 0.8 covers bf16
    "gamma1.0": (dict(gamma_denoising=1.0), ("actor",), {}, ("fp32",)),
    "gamma0.8": (dict(gamma_denoising=0.8), ("pg_loss", "actor"), {}, BOTH),
    "vf0.25": (dict(vf_coef=0.25), ("critic",), {}, BOTH),
    "vf1.0": (dict(vf_coef=1.0), ("critic",), {}, BOTH),
    "minstd0.01": (dict(min_logprob_std=0.01), ("actor",), dict(lp_hp=dict(min_logprob_std=0.01)), BOTH),
    "minstd0.3": (dict(min_logprob_std=0.3), ("actor",), dict(lp_hp=dict(min_logprob_std=0.3)), BOTH),
}
HP_PARAMS = [(n, pr) for n, c in HP_CASES.items() for pr in c[3]]


def hp_reference(name, precision):
    """The CPU half of an HP case: (problem, oracle at the case, oracle at the defaults), with the
    case's discriminating power asserted. Callable without a GPU."""
    hp, moves, pkw, _ = HP_CASES[name]
    p = _Problem(HOPPER, precision, **pkw)
    tol, ratio1 = TOL[precision], p.kind == "ratio1"
    ref, ref0 = p.oracle(**hp), p.oracle()
    _assert_moved(ref, ref0, moves, tol, ratio1, label=name)
    if name.startswith("clip-rate"):   # the rate itself: the other rate's reference must differ too
        other = dict(hp, clip_ploss_coef_rate=4.0 - hp["clip_ploss_coef_rate"])
        _assert_moved(ref, p.oracle(**other), ("pg_loss", "actor"), tol, ratio1, label=name + " vs the other rate")
    if name.startswith("vf"):          # the actor's gradient and v_loss do not depend on vf_coef
        assert ref[0]["v_loss"] == ref0[0]["v_loss"] and all(np.array_equal(ref[1][k], ref0[1][k]) for k in ref[1])
        s = hp["vf_coef"] / 0.5
        assert all(np.allclose(ref[2][k], ref0[2][k] * s, rtol=1e-12, atol=0) for k in ref[2])
    if name.startswith("minstd"):      # the clamp must hold for some of the K' steps and not for others
        std = np.exp(0.5 * np.asarray(p.sched["ddpm_logvar_clipped"], np.float64)[:p.kf])
        assert (std < hp["min_logprob_std"]).any() and (std > hp["min_logprob_std"]).any(), std
    if name == "reward-horizon8":
        assert all(np.array_equal(ref[1][k], ref0[1][k]) for k in ref[1])
    return p, ref, ref0


@pytest.mark.parametrize("name,precision", HP_PARAMS, ids=[f"{n}-{p}" for n, p in HP_PARAMS])
def test_ppo_hparams_off_default(cuda, name, precision):
    """dppo_ppo_minibatch with one loss hyperparameter off its default (HP_CASES) against O.c_loss at
    the same value: pg_loss, v_loss, approx_kl, clipfrac, the ratio mean and every gradient tensor.
    fp32 'perturbed' (rows on both clip branches), bf16 'ratio1' against the rounding oracle.
    reward_horizon < horizon_steps also pins the gradient mask: in fp32 the out-layer bias gradient is
    exactly 0.0 for every element q >= reward_horizon * action_dim."""
    p, ref, _ = hp_reference(name, precision)
    hp = HP_CASES[name][0]
    gpu = _Gpu(p, cuda)
    m, g = gpu.minibatch(**hp)
    _compare(f"{name}-{precision}", gpu, m, g, ref, TOL[precision])
    if name.startswith("reward-horizon") and precision == "fp32":
        nh = min(hp["reward_horizon"], p.d.horizon_steps) * p.d.action_dim
        out_b = gpu.split(g)[0]["out_b"]
        assert np.all(out_b[nh:] == 0.0), out_b
        assert np.all(out_b[:nh] != 0.0), out_b


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("rh", [1, 2, 8])
def test_logprob_reward_horizon(cuda, precision, rh):
    """dppo_logprob's per-row mean over [:, :reward_horizon] (8 > horizon_steps = 4 clamps to the row)
    against np.clip(lp, -5, 2)[:, :H].mean; test_logprob's bounds (10x the element tolerance)."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    tol = {"fp32": 1e-3, "bf16": 2e-3}[precision]
    p = _Problem(HOPPER, precision, lp_hp=dict(reward_horizon=rh))
    full = np.clip(p.lp_ref, -5, 2).mean(axis=(1, 2)).reshape(p.N, p.kf)
    if rh < 4:   # the slice moves the mean by more than 10x the bound
        assert np.abs(p.lp_ref_mean - full).max() >= 10 * tol * 10
    else:
        assert np.array_equal(p.lp_ref_mean, full)
    gpu = _Gpu(p, cuda)
    _, lpm = ops.logprob(p.d, precision, gpu.packf, gpu.tab, gpu.obs, gpu.chains, want_elem=False, reward_horizon=rh)
    torch.cuda.synchronize()
    err = float(np.abs(lpm.cpu().numpy() - p.lp_ref_mean).max())
    print(json.dumps({"case": f"logprob-rh{rh}-{precision}", "max_abs_err": err, "bound": tol * 10}))
    assert err < tol * 10


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ppo_data_parallel_shard(cuda, precision):
    """One shard of a data-parallel minibatch: global_rows = 4 x rows, loss_scale = 0.25 and the
    advantage moments {count, sum, sumsq} of a larger population (mean 0.4, std 1.7; the shard's own
    are ~0 and ~1), against O.c_loss(adv_mean_std = the population's, denom = global_rows) x loss_scale."""
    import torch
    p = _Problem(HOPPER, precision)
    tol = TOL[precision]
    grows, ls = 4 * ROWS, 0.25
    pop = np.random.default_rng(5).normal(0.4, 1.7, grows)
    st = np.array([grows, pop.sum(), (pop * pop).sum()])
    mean = st[1] / st[0]
    std = np.sqrt(max(st[2] / st[0] - mean * mean, 0.0))
    own = p.adv[p.bi].astype(np.float64)
    assert abs(mean - own.mean()) > 0.2 and abs(std - own.std()) > 0.3
    ref = p.oracle(adv_mean_std=(mean, std), denom=grows)
    ref0 = p.oracle()
    # against the defaults (own moments, denom = rows, scale 1), and against each hook alone
    _assert_moved(ref, ref0, ("pg_loss", "v_loss", "actor", "critic"), tol, p.kind == "ratio1", scale=1.0 / ls)
    _assert_moved(ref, p.oracle(denom=grows), ("pg_loss", "actor"), tol, p.kind == "ratio1")
    _assert_moved(ref, p.oracle(adv_mean_std=(mean, std)), ("pg_loss", "v_loss", "actor", "critic"), tol,
                  p.kind == "ratio1")
    gpu = _Gpu(p, cuda)
    m, g = gpu.minibatch(global_rows=grows, loss_scale=ls, adv_stats=torch.tensor(st, dtype=torch.float64, device=cuda))
    _compare(f"shard-{precision}", gpu, m, g, ref, tol, denom=grows, grad_scale=ls)


@pytest.mark.parametrize("gamma,lam,rsc", [(0.9, 0.8, 0.1), (1.0, 1.0, 1.0), (0.99, 0.0, 2.0)])
@pytest.mark.parametrize("S,E", [(7, 3), (50, 4)])
def test_gae_off_default(cuda, S, E, gamma, lam, rsc):
    """dppo_gae off (gamma, lam, reward_scale_const) = (0.99, 0.95, 1) against O.gae; column 0 is
    terminated at every step, column 1 never; test_gae's tolerances."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    rng = np.random.default_rng(S * 100 + E)
    r = rng.normal(size=(S, E))
    v = rng.normal(size=(S, E)).astype(np.float32)
    lv = rng.normal(size=E).astype(np.float32)
    term = (rng.uniform(size=(S, E)) < 0.05).astype(np.uint8)
    term[:, 0], term[:, 1] = 1, 0
    args = (r, v.astype(np.float64), lv.astype(np.float64), term.astype(np.float64))
    ref_a, ref_r = O.gae(*args, gamma=gamma, lam=lam, reward_scale_const=rsc)
    def_a, _ = O.gae(*args)
    assert np.abs(ref_a[:, 1:] - def_a[:, 1:]).max() >= 10 * (1e-5 + 1e-6 * np.abs(ref_a).max())
    a, ret = ops.gae(torch.tensor(r, device=cuda), torch.tensor(v, device=cuda), torch.tensor(lv, device=cuda),
                     torch.tensor(term, device=cuda), gamma=gamma, lam=lam, reward_scale_const=rsc)
    torch.cuda.synchronize()
    print(json.dumps({"case": f"gae-{S}x{E}-{gamma}-{lam}-{rsc}", "max_abs_err": float(np.abs(a.cpu().numpy() - ref_a).max())}))
    np.testing.assert_allclose(a.cpu().numpy(), ref_a, rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(ret.cpu().numpy(), ref_r, rtol=1e-6, atol=1e-5)


# ------------------------------------------------------------------------------------------------
# B. geometry cases (default hyperparameters)
# ------------------------------------------------------------------------------------------------
def _ksteps(width, precision):
    """packed_ksteps (csrc/dppo_layout.h): k-steps of a layer of `width` inputs, rounded up to even."""
    kg = 16 if precision == "fp32" else 32
    return ((width + kg - 1) // kg + 1) & ~1


def _actor_msg(dims, precision):
    xd = dims["horizon_steps"] * dims["action_dim"]
    ind = xd + dims["time_dim"] + dims["cond_steps"] * dims["obs_dim"]
    return (f"actor: hidden {dims['actor_hidden']} / chunk {xd} / in-layer k-steps {_ksteps(ind, precision)} "
            "not instantiated")


def _critic_hidden_msg(dims, precision):
    return f"critic: hidden {dims['critic_hidden']} not instantiated"


def _critic_layout_msg(dims, precision):
    return "critic row tile: layout does not match the instantiation"


RUNS = None
ALL_RUN = dict(fp32=(RUNS, RUNS), two_byte=(RUNS, RUNS))
# name -> (dims, {fp32 | two_byte: (actor, critic)} each RUNS or the rejection's message, what it reaches)
GEOMETRIES = {
    "ft1": (dict(HOPPER, ft_denoising_steps=1), ALL_RUN,
            "the reference's K' = 1 quirk cc = j: every row at zero clip width; one time-MLP bucket"),
    "ft7": (dict(HOPPER, ft_denoising_steps=7), ALL_RUN, "7 time-MLP buckets (neither 10 nor a power of two)"),
    "ft16": (dict(HOPPER, ft_denoising_steps=16), ALL_RUN, "16 buckets: the bound of dppo_ppo_minibatch"),
    "td32": (dict(HOPPER, time_dim=32), ALL_RUN,
             "the generic dtemb loop of time_bwd_body (backward_tail.hip: not TD == 16 && H == 512)"),
    "ah256": (dict(HOPPER, actor_hidden=256), dict(fp32=(_actor_msg, RUNS), two_byte=(RUNS, RUNS)),
              "dispatch_actor's 2-byte NT = 2 on 8 waves, and time_bwd_body's generic dtemb loop (H != 512)"),
    "cond2-hopper": (dict(HOPPER, cond_steps=2), ALL_RUN, "more than one conditioning step (SD 22, 50 inputs)"),
    "cond2-walker": (dict(WALKER, cond_steps=2), dict(fp32=(_actor_msg, _critic_layout_msg), two_byte=(RUNS, RUNS)),
                     "dispatch_actor's 2-byte KSI = 4 cases (74 inputs)"),
    "h8a3": (dict(HOPPER, horizon_steps=8), ALL_RUN, "reward_horizon 4 of 8 predicted steps on the 32-row tile (XD 24)"),
    "h8a4": (dict(HOPPER, horizon_steps=8, action_dim=4), ALL_RUN, "XD = 32: the bound of validate_dims"),
    "tiny": (dict(HOPPER, obs_dim=3, action_dim=1), dict(fp32=(_actor_msg, RUNS), two_byte=(RUNS, RUNS)),
             "23 inputs: 2-byte KSI = 2 with a mostly empty in-layer"),
    "ch128": (dict(HOPPER, critic_hidden=128), dict(fp32=(RUNS, _critic_hidden_msg), two_byte=(RUNS, _critic_hidden_msg)), ""),
    "ch384": (dict(HOPPER, critic_hidden=384), dict(fp32=(RUNS, _critic_hidden_msg), two_byte=(RUNS, _critic_hidden_msg)), ""),
    "ch512": (dict(HOPPER, critic_hidden=512), dict(fp32=(RUNS, _critic_hidden_msg), two_byte=(RUNS, _critic_hidden_msg)), ""),
    "ah128": (dict(HOPPER, actor_hidden=128), dict(fp32=(_actor_msg, RUNS), two_byte=(_actor_msg, RUNS)), ""),
    "ah384": (dict(HOPPER, actor_hidden=384), dict(fp32=(_actor_msg, RUNS), two_byte=(_actor_msg, RUNS)), ""),
}
ENTRIES = ("logprob", "critic_forward", "ppo_minibatch", "pretrain_minibatch")
GEO_PARAMS = [(g, pr, e) for g in GEOMETRIES for pr in ("fp32", "bf16", "fp16") for e in ENTRIES]
SENTINEL = -7.25


def expected_rejection(geometry, precision, entry):
    """None where the table says the entry runs, else the message it must fail with."""
    dims, table, _ = GEOMETRIES[geometry]
    actor, critic = table["fp32" if precision == "fp32" else "two_byte"]
    first = {"logprob": (actor,), "pretrain_minibatch": (actor,), "critic_forward": (critic,),
             "ppo_minibatch": (actor, critic)}[entry]
    for f in first:
        if f is not RUNS:
            return f(dims, precision)
    return None


def test_geometry_table_matches_host_arithmetic():
    """The table against the layout's k-steps and ops.ppo_plan (host arithmetic; no launch): the fp32
    actor has H = 512 with 4 in-layer k-steps only, the 2-byte actor H / 128 in {2, 4} column tiles per
    wave with 2 or 4, the critic HC = 256 with 2; every case runs the 32-row actor tile."""
    from diffusionpolicyoptimization_amd import ops
    for name, (dims, table, _) in GEOMETRIES.items():
        d = ops.ModelDims(**dims)
        for precision in ("fp32", "bf16", "fp16"):
            actor, critic = table["fp32" if precision == "fp32" else "two_byte"]
            ks_a, ks_c = _ksteps(d.actor_in, precision), _ksteps(d.sd, precision)
            if precision == "fp32":
                a_ok = d.actor_hidden == 512 and ks_a == 4
            else:
                a_ok = d.actor_hidden in (256, 512) and ks_a in (2, 4)
            c_ok = d.critic_hidden == 256 and ks_c == 2
            assert (actor is RUNS) == a_ok and (critic is RUNS) == c_ok, (name, precision, ks_a, ks_c)
            plan = ops.ppo_plan(d, precision, ROWS)
            assert plan["actor_tile_rows"] == 32 and plan["actor_waves"] == (16 if precision == "fp32" else 8), (name, plan)
    assert _ksteps(74, "bf16") == 4 and _ksteps(23, "bf16") == 2 and _ksteps(74, "fp32") == 6 and _ksteps(23, "fp32") == 2


_PROBLEMS = {}


def _geo_problem(geometry, precision):
    key = (geometry, precision)
    if key not in _PROBLEMS:
        _PROBLEMS.clear()       # one at a time: the parametrisation visits a key's entries in a row
        dims = GEOMETRIES[geometry][0]
        _PROBLEMS[key] = _Problem(dims, precision, n_samples=200 if dims["ft_denoising_steps"] == 1 else NSAMP)
    return _PROBLEMS[key]


def _rejected(call, outputs, msg):
    """call() raises the library's unsupported-configuration error (code 3) with the dispatch's message
    and leaves the sentinel-filled outputs untouched."""
    import re
    import torch
    from diffusionpolicyoptimization_amd._lib import DppoError
    with pytest.raises(DppoError, match=re.escape(f"failed (3): {msg}")):
        call()
    torch.cuda.synchronize()
    for o in outputs:
        assert bool((o == SENTINEL).all()), "a rejected call wrote its outputs"


@pytest.mark.parametrize("geometry,precision,entry", GEO_PARAMS, ids=["-".join(x) for x in GEO_PARAMS])
def test_geometry(cuda, geometry, precision, entry):
    """One update entry at one geometry of GEOMETRIES (its third field names the branch it reaches:
    td32 and ah256 the generic dtemb loop of time_bwd_body, ah256 the 2-byte NT = 2 on 8 waves
    instantiations of dispatch_actor, cond2-walker its 2-byte KSI = 4 ones) against the oracle at the
    entry's existing tolerance — or, where the table says REJECTED, the unsupported-configuration error
    with the dispatch's message and untouched outputs. Shapes: logprob 37 samples, critic_forward 77,
    ppo_minibatch 150 rows of 40 samples (200 at K' = 1), pretrain_minibatch 150 rows."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    p = _geo_problem(geometry, precision)
    d, rnd = p.d, _rnd(precision)
    msg = expected_rejection(geometry, precision, entry)
    gpu = _Gpu(p, cuda) if entry == "ppo_minibatch" and msg is None else None
    T = lambda x: torch.tensor(x, device=cuda)
    full = lambda *shape, dtype=torch.float32: torch.full(shape, SENTINEL, dtype=dtype, device=cuda)
    label = f"{geometry}-{precision}-{entry}"
    rh = min(4, d.horizon_steps)
    if entry != "ppo_minibatch" or msg is not None:
        pf = T(ops.flatten_params(ops.actor_param_spec(d), p.ft))
        pc = T(ops.flatten_params(ops.critic_param_spec(d), p.critic))
        tab = T(ops.sched_table(p.sched))
    if entry == "logprob":
        n, kf = 37, p.kf
        rng = np.random.default_rng(4)
        state = rng.uniform(-1, 1, (n, d.sd)).astype(np.float32)
        chains = (rng.standard_normal((n, kf + 1, d.xd)) * 0.5).astype(np.float32)
        lpe, lpm = full(n * kf, d.xd), full(n, kf)
        call = lambda: ops.logprob(d, precision, ops.pack_actor(d, pf, precision), tab, T(state), T(chains),
                                   reward_horizon=rh, lp_elem=lpe, lp_mean=lpm)
        if msg:
            return _rejected(call, (lpe, lpm), msg)
        call()
        torch.cuda.synchronize()
        tol = {"fp32": 1e-3, "bf16": 2e-3, "fp16": 2e-3}[precision]
        ref = O.get_logprobs(to_f64(p.ft), p.sched, p.state(state), p.x(chains, kf + 1), kf, rnd=rnd)
        ref_mean = np.clip(ref, -5, 2)[:, :rh].mean(axis=(1, 2)).reshape(n, kf)
        rel = np.abs(lpe.cpu().numpy().reshape(ref.shape) - ref) / (1 + np.abs(ref))
        q99, em = float(np.quantile(rel, 0.99)), float(np.abs(lpm.cpu().numpy() - ref_mean).max())
        print(json.dumps({"case": label, "q99_rel": q99, "bound": tol, "mean_abs": em, "mean_bound": tol * 10}))
        assert q99 < tol and em < tol * 10
    elif entry == "critic_forward":
        n = 77
        state = np.random.default_rng(5).uniform(-1, 1, (n, d.sd)).astype(np.float32)
        v = full(n)
        call = lambda: ops.critic_forward(d, precision, ops.pack_critic(d, pc, precision), T(state), values=v)
        if msg:
            return _rejected(call, (v,), msg)
        call()
        torch.cuda.synchronize()
        tol = {"fp32": 1e-4, "bf16": 1e-3, "fp16": 1e-3}[precision]
        ref, _ = O.critic_forward(to_f64(p.critic), p.state(state), rnd=rnd)
        err = float(np.abs(v.cpu().numpy() - ref[:, 0]).max() / (1 + np.abs(ref).max()))
        print(json.dumps({"case": label, "err": err, "bound": tol}))
        assert err < tol
    elif entry == "ppo_minibatch":
        if msg:
            na, nc = ops.spec_count(ops.actor_param_spec(d)), ops.spec_count(ops.critic_param_spec(d))
            grads, metrics = full(na + nc), full(16, dtype=torch.float64)
            lp_old = T(p.lp_ref_mean.astype(np.float32))
            call = lambda: ops.ppo_minibatch(
                d, precision, ops.ppo_hparams(global_rows=ROWS), ops.pack_actor(d, pf, precision),
                ops.pack_critic(d, pc, precision), pf, tab, T(p.obs), T(p.chains), lp_old, T(p.adv), T(p.ret), SEED, EPOCH,
                START, ROWS, ops.ppo_workspace(d, precision, ROWS, cuda), grads, metrics)
            return _rejected(call, (grads, metrics), msg)
        ref = p.oracle(reward_horizon=rh)
        if geometry == "ft1":   # cc = j = 0: a row counts as clipped as soon as its ratio is not exactly 1
            assert ref[0]["clipfrac"] == (0.0 if p.kind == "ratio1" else 1.0)
        m, g = gpu.minibatch(fill=SENTINEL, reward_horizon=rh)
        _compare(label, gpu, m, g, ref, TOL[precision])
    else:
        rows, K = 150, d.denoising_steps
        rng = np.random.default_rng(21)
        x0 = rng.uniform(-1, 1, (rows, d.xd)).astype(np.float32)
        cond = rng.uniform(-1, 1, (rows, d.sd)).astype(np.float32)
        t = rng.integers(0, K, rows).astype(np.int32)
        noise = rng.standard_normal((rows, d.xd)).astype(np.float32)
        na = ops.spec_count(ops.actor_param_spec(d))
        grads, metrics = full(na), full(16, dtype=torch.float64)
        call = lambda: ops.pretrain_minibatch(d, precision, ops.pack_actor(d, pf, precision), pf, tab,
                                              T(ops.q_sched_table(p.sched)), T(x0), T(cond), T(t), T(noise),
                                              ops.ppo_workspace(d, precision, rows, cuda), grads, metrics)
        if msg:
            return _rejected(call, (grads, metrics), msg)
        loss = call()
        torch.cuda.synchronize()
        tol = TOL[precision]
        loss_ref, g_ref = O.p_losses(to_f64(p.ft), p.sched, p.x(x0), p.state(cond), t, p.x(noise), rnd=rnd)
        ga = ops.unflatten_params(ops.actor_param_spec(d), grads.cpu().numpy())
        errs = {k: _rel(ga[k], r) for k, r in g_ref.items()}
        print(json.dumps({"case": label, "loss": [float(loss), loss_ref], "max_err": max(errs.values()), "errs": errs}))
        assert abs(float(loss) - loss_ref) < tol * loss_ref
        bad = {k: v for k, v in errs.items() if not v < tol}
        assert not bad, (bad, errs)


def test_rejected_minibatch_leaves_the_stream_usable(cuda):
    """A minibatch rejected for its critic (critic_hidden = 128) is refused before its first launch: the
    stream's per-sample count scratch (zeroed by the critic's last launch) holds no stale counts, so
    the same supported minibatch before and after it gives the same critic gradient and v_loss."""
    import torch
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd._lib import DppoError
    good = _Gpu(_Problem(HOPPER, "fp32"), cuda)
    m0, g0 = good.minibatch()
    bad = _Problem(dict(HOPPER, critic_hidden=128), "fp32")
    d = bad.d
    T = good.T
    pf = T(ops.flatten_params(ops.actor_param_spec(d), bad.ft))
    pc = T(ops.flatten_params(ops.critic_param_spec(d), bad.critic))
    na, nc = ops.spec_count(ops.actor_param_spec(d)), ops.spec_count(ops.critic_param_spec(d))
    with pytest.raises(DppoError, match="critic: hidden 128 not instantiated"):
        ops.ppo_minibatch(d, "fp32", ops.ppo_hparams(global_rows=ROWS), ops.pack_actor(d, pf, "fp32"),
                          ops.pack_critic(d, pc, "fp32"), pf, good.tab, T(bad.obs), T(bad.chains), T(bad.lp_old), T(bad.adv),
                          T(bad.ret), SEED, EPOCH, START, ROWS, ops.ppo_workspace(d, "fp32", ROWS, cuda),
                          torch.zeros(na + nc, device=cuda), torch.zeros(16, dtype=torch.float64, device=cuda))
    m1, g1 = good.minibatch()
    np.testing.assert_allclose(m1[:5], m0[:5], rtol=1e-6, atol=1e-9)
    assert np.abs(g1 - g0).max() <= 1e-5 * np.abs(g0).max()
