"""Whole-iteration parity: the fp32 agent on the GPU against the oracle's composition of the
reference loop (oracle/iteration.py; reference agent/finetune/train_ppo_diffusion_agent.py:58-377).

Three iterations per seed (eval, train, train) on the synthetic env with 10-chunk episodes, so
every iteration completes episodes and the ±5 % returns metric (the north star's acceptance
quantity) is exercised. Per iteration the test compares sampled chains and actions, `firsts`,
rewards, episode returns; per train iteration the value / old-log-prob passes, advantages and
returns (reward scaler state carried over iterations), the last minibatch's loss metrics, the
number of applied minibatches and the parameters after the update.

Tolerances (fp32 kernels vs the float64 oracle; measured maxima in DESIGN.md §5):
  chains / actions 2e-5 abs; rewards and episode returns 1e-5 relative (the north star's
  "sampled actions / episode returns match on fixed seeds"); values / log-probs 1e-4 abs;
  advantages / returns 1e-4 relative to their scale; parameter change of the update phase
  (about 20 AdamW steps of lr 1e-4): median 1e-4 and 99th percentile 1e-3 of its largest
  element, 5e-3 in L2 norm (max 0.1: Adam's per-element normalisation turns gradient elements
  that are near zero, |g| ~ their fp32 error, into noise in both implementations).
"""
import json
import os

import numpy as np
import pytest

from oracle import dppo_oracle as O
from oracle.iteration import PPODiffusionLoopOracle, SyntheticVecEnvOracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _agent_and_oracle(seed, tmp_path, extra=(), precision="fp32", env_oracle=None, as_shipped=False):
    from diffusionpolicyoptimization_amd import ops
    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    base = ([] if as_shipped else
            [f"model.precision={precision}", "train.n_steps=24", "train.batch_size=240", "train.val_freq=3",
             "env.max_episode_steps=40"])
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp",
                      [*base, "train.n_train_itr=3", f"seed={seed}", f"logdir={tmp_path}", "train.save_checkpoints=false",
                       *extra])
    a = get_class(cfg._target_)(cfg)
    m = a.model
    na = m.n_actor
    base = ops.unflatten_params(m.actor_spec, m.base_params.cpu().numpy())
    tp = m.train_params.cpu().numpy()
    ft = ops.unflatten_params(m.actor_spec, tp[:na])
    critic = ops.unflatten_params(m.critic_spec, tp[na:])
    seeds = [a.seed + a.env_offset + i for i in range(a.n_envs)]
    if env_oracle is not None:
        env = env_oracle(a, cfg, seeds)
    else:
        env = SyntheticVecEnvOracle(seeds, cfg.obs_dim, cfg.action_dim, cfg.act_steps, cfg.env.max_episode_steps,
                                    cfg.env.get("family_seed", 0))
    assert a.actor_lr_scheduler(1) == a.actor_lr_scheduler(50) == cfg.train.actor_lr   # constant at this cfg
    # the variant is the agent's model's: its networks, its diffusion parameterisation, its advantage quantiles
    sched = O.with_param(O.ddpm_schedule(cfg.denoising_steps), m.denoised_clip_value, m.predict_epsilon)
    quantiles = (m.clip_advantage_lower_quantile, m.clip_advantage_upper_quantile) if m.adv_clip else None
    orc = PPODiffusionLoopOracle(
        base, ft, critic, m.actor_spec, m.critic_spec, sched, env, model=O.Model.from_dims(m.dims),
        adv_clip_quantiles=quantiles,
        seed=m.seed, perm_seed=a.perm_seed, n_steps=a.n_steps, ft_steps=m.ft_denoising_steps,
        act_steps=a.act_steps, horizon_steps=a.horizon_steps, action_dim=a.action_dim, val_freq=a.val_freq,
        batch_size=a.batch_size, update_epochs=a.update_epochs, target_kl=a.target_kl, gamma=a.gamma,
        gae_lambda=a.gae_lambda, reward_scale_running=a.reward_scale_running,
        reward_scale_const=a.reward_scale_const, reset_at_iteration=a.reset_at_iteration,
        lr=cfg.train.actor_lr, weight_decay=a.actor_optimizer.weight_decay,
        min_sampling_std=m.min_sampling_denoising_std, randn_clip=m.randn_clip_value,
        min_logprob_std=m.min_logprob_denoising_std, gamma_denoising=m.gamma_denoising,
        clip_ploss_coef=m.clip_ploss_coef, clip_ploss_coef_base=m.clip_ploss_coef_base,
        clip_ploss_coef_rate=m.clip_ploss_coef_rate, vf_coef=a.vf_coef,
        success_threshold=a.best_reward_threshold_for_success, env_offset=a.env_offset,
        n_critic_warmup_itr=a.n_critic_warmup_itr,
        ft_denoising_steps_d=m.ft_denoising_steps_d, ft_denoising_steps_t=m.ft_denoising_steps_t)
    return a, orc


def _rel(x, ref):
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / (np.abs(ref).max() + 1e-12))


def _run_and_compare_bf16(a, orc, n_itr=3):
    """The bf16 agent against the float64 oracle (no rounding emulation): the trajectories drift
    apart by the bf16 rounding of every denoiser layer, compounded through the env, so the bound
    that matters is the north star's own, episode returns within +-5 %; chains, rewards and the
    loss metrics are recorded and bounded at a few times their measured drift."""
    errs = []
    for it in range(n_itr):
        res = a.iteration()
        ref = orc.iteration()
        e = {"itr": it, "eval": bool(res["eval"])}
        assert res["eval"] == ref["eval"]
        np.testing.assert_array_equal(a.firsts, ref["firsts"])
        ch = a.chains_traj.cpu().numpy().reshape(ref["chains"].shape)
        e["chains_abs"] = float(np.abs(ch - ref["chains"]).max())
        e["rewards_rel"] = _rel(a.reward_pin.numpy(), ref["rewards"])
        ep_ref = ref["episodes"]
        assert res["num_episode_finished"] == ep_ref["num_episode_finished"] > 0
        e["return_rel"] = abs(res["avg_episode_reward"] - ep_ref["avg_episode_reward"]) / abs(ep_ref["avg_episode_reward"])
        if not res["eval"]:
            last = ref["metrics"][-1]
            for k in ("pg_loss", "v_loss", "approx_kl"):
                e[k] = (float(res[k]), float(last[k]))
        errs.append(e)
        assert e["return_rel"] <= 0.05, e                  # north star: returns within +-5 %
        assert e["chains_abs"] <= 0.3 and e["rewards_rel"] <= 0.05, e   # measured <= 0.13 / 0.0096
        if not res["eval"]:
            assert abs(res["v_loss"] - last["v_loss"]) <= 0.05 * abs(last["v_loss"]), e
    return errs


def _run_and_compare(a, orc, n_itr=3, need_episodes=True, chains_tol=2e-5):
    errs = []
    for it in range(n_itr):
        p0 = a.model.train_params.cpu().numpy().astype(np.float64)
        th0 = orc.theta.copy()
        n0 = a.timing["n_updates"]
        res = a.iteration()
        ref = orc.iteration()
        e = {"itr": it, "eval": bool(res["eval"])}
        assert res["eval"] == ref["eval"]
        np.testing.assert_array_equal(a.firsts, ref["firsts"])
        S, E = a.n_steps, a.n_envs
        ch = a.chains_traj.cpu().numpy().reshape(ref["chains"].shape)
        e["chains_abs"] = float(np.abs(ch - ref["chains"]).max())
        e["rewards_rel"] = _rel(a.reward_pin.numpy(), ref["rewards"])
        np.testing.assert_array_equal(a.obs_traj.cpu().numpy().shape, (S, E, ref["obs"].shape[-1]))
        e["obs_abs"] = float(np.abs(a.obs_traj.cpu().numpy() - ref["obs"]).max())
        ep_ref = ref["episodes"]
        assert res["num_episode_finished"] == ep_ref["num_episode_finished"]
        if need_episodes or ep_ref["num_episode_finished"] > 0:
            assert ep_ref["num_episode_finished"] > 0
            e["return_rel"] = (abs(res["avg_episode_reward"] - ep_ref["avg_episode_reward"]) /
                               abs(ep_ref["avg_episode_reward"]))
        else:
            e["return_rel"] = 0.0
        assert e["chains_abs"] <= chains_tol, e
        assert e["rewards_rel"] <= 1e-5 and e["return_rel"] <= 1e-5, e
        if not res["eval"]:
            e["values_abs"] = float(np.abs(a.values.cpu().numpy().reshape(S, E) - ref["values"]).max())
            e["lp_old_abs"] = float(np.abs(a.lp_old.cpu().numpy() - ref["lp_old"]).max())
            e["adv_rel"] = _rel(a.adv.cpu().numpy(), ref["adv"])
            e["ret_rel"] = _rel(a.ret.cpu().numpy(), ref["ret"])
            n_upd = a.timing["n_updates"] - n0
            assert n_upd == len(ref["metrics"]), (n_upd, len(ref["metrics"]))
            last = ref["metrics"][-1]
            for k in ("pg_loss", "v_loss", "approx_kl"):
                e[k] = (float(res[k]), float(last[k]))
            assert abs(res["v_loss"] - last["v_loss"]) <= 1e-3 * abs(last["v_loss"]) + 1e-7, e
            assert abs(res["pg_loss"] - last["pg_loss"]) <= 1e-3 * abs(last["pg_loss"]) + 1e-6, e
            dg = a.model.train_params.cpu().numpy().astype(np.float64) - p0
            dr = orc.theta - th0
            diff = np.abs(dg - dr)
            stepped = bool(dr.any())   # False inside the critic warm-up: the oracle applied no step (:348-356)
            if stepped:
                scale = np.abs(dr).max()
                e["param_delta_max_rel"] = float(diff.max() / scale)
                e["param_delta_p99_rel"] = float(np.quantile(diff, 0.99) / scale)
                e["param_delta_p999_rel"] = float(np.quantile(diff, 0.999) / scale)
                e["param_delta_l2_rel"] = float(np.linalg.norm(dg - dr) / np.linalg.norm(dr))
                e["param_delta_median_rel"] = float(np.median(diff) / scale)
            e["explained_var"] = (float(res["explained_var"]), float(ref["explained_var"]))
            # explained variance (agent :373-377) of the pre-update values and the returns
            assert abs(e["explained_var"][0] - e["explained_var"][1]) <= 1e-3 * max(1.0, abs(e["explained_var"][1])), e
            assert e["values_abs"] <= 1e-4 and e["lp_old_abs"] <= 1e-4, e
            assert e["adv_rel"] <= 1e-4 and e["ret_rel"] <= 1e-4, e
            # Adam divides each gradient by its own running norm: where a gradient element is near
            # zero (|g| ~ its fp32 error) the step direction is fp-noise in BOTH implementations, so
            # the bound is on the distribution: median and 99.9th percentile tight, the max loose
            if stepped:
                assert e["param_delta_median_rel"] <= 1e-4 and e["param_delta_p99_rel"] <= 1e-3, e
                assert e["param_delta_l2_rel"] <= 5e-3, e
                assert e["param_delta_max_rel"] <= 0.1, e
            else:   # no reference change to be relative to (0 / 0): the agent's must be exactly none
                assert not dg.any(), e
        errs.append(e)
    return errs


def _record(name, errs):
    out = os.environ.get("DPPO_PARITY_LOG")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps({"case": name, "iterations": errs}) + "\n")


@pytest.mark.parametrize("seed", [42, 43, 44])
def test_iterations_match_oracle(cuda, seed, tmp_path):
    a, orc = _agent_and_oracle(seed, tmp_path)
    errs = _run_and_compare(a, orc)
    _record(f"seed{seed}", errs)
    assert [e["eval"] for e in errs] == [True, False, False]


@pytest.mark.parametrize("seed", [42, 43, 44])
def test_iterations_bf16_returns_match_oracle(cuda, seed, tmp_path):
    """The BASELINE config-2 operand policy (bf16 denoiser) over the same three iterations:
    episode returns within the north star's +-5 % of the float64 oracle on each seed."""
    a, orc = _agent_and_oracle(seed, tmp_path, precision="bf16")
    errs = _run_and_compare_bf16(a, orc)
    _record(f"bf16_seed{seed}", errs)
    assert [e["eval"] for e in errs] == [True, False, False]


def test_iterations_match_oracle_kl_stop(cuda, tmp_path):
    """target_kl = -1: every minibatch trips the stop, so each epoch applies exactly its first
    minibatch (reference :366-368 leaves the batch loop only)."""
    a, orc = _agent_and_oracle(42, tmp_path, ["train.target_kl=-1.0"])
    errs = _run_and_compare(a, orc)
    _record("kl_stop", errs)
    assert orc.n_updates == 2 * a.update_epochs


@pytest.mark.parametrize("split", ["1", "0"], ids=["split", "unsplit"])
def test_iterations_match_oracle_critic_warmup(cuda, tmp_path, monkeypatch, split):
    """train.n_critic_warmup_itr = 2 (agent :348-356, oracle/iteration.py `if self.itr >=
    self.n_critic_warmup_itr`): the three iterations are an eval, a train iteration inside the warm-up
    (every minibatch computed and counted, no optimizer step: the metrics leave by a plain copy and an
    event, nothing is pre-cleared) and a train iteration whose steps are applied; through the split and
    the unsplit update."""
    import torch
    monkeypatch.setenv("DPPO_SPLIT_UPDATE", split)
    a, orc = _agent_and_oracle(42, tmp_path, ["train.n_critic_warmup_itr=2"])
    assert a.n_critic_warmup_itr == orc.n_critic_warmup_itr == 2
    errs = _run_and_compare(a, orc, n_itr=1)
    before = a.model.train_params.clone()
    errs += _run_and_compare(a, orc, n_itr=1)
    assert torch.equal(a.model.train_params, before)
    assert a.actor_optimizer.iterations == 0
    in_warmup = orc.n_updates          # warm-up minibatches count as updates though none is applied
    errs += _run_and_compare(a, orc, n_itr=1)
    _record(f"critic_warmup_split{split}", errs)
    assert [e["eval"] for e in errs] == [True, False, False]
    assert orc.opt_steps == orc.n_updates - in_warmup > 0     # the last iteration's minibatches alone
    assert a.actor_optimizer.iterations == orc.opt_steps


def test_iterations_match_oracle_with_annealing(cuda, tmp_path):
    """ft_denoising_steps annealing (model.step(), diffusion_vpg.py:114-142) with d = t = 1: K'
    drops 10 -> 9 -> 8 over the three iterations and the base actor becomes a copy of actor_ft
    each time; the rollout buffers follow K' (the reference re-sizes chains_trajs every
    iteration, agent :87-95). Compared with the oracle loop extended by the same anneal."""
    a, orc = _agent_and_oracle(42, tmp_path, ["model.ft_denoising_steps_d=1", "model.ft_denoising_steps_t=1"])
    kfs = []
    errs = []
    for _ in range(3):
        kfs.append(a.model.ft_denoising_steps)
        errs += _run_and_compare(a, orc, n_itr=1)
        assert a.model.ft_denoising_steps == orc.kf
    _record("anneal", errs)
    assert kfs == [10, 9, 8] and a.chains_traj.shape[2] == 9 and a.lp_old.shape[1] == 8


def test_config1_as_shipped_matches_oracle(cuda, tmp_path):
    """BASELINE config 1 exactly as ft_ppo_diffusion_mlp.yaml ships it — 4 envs x 50 chunks, fp32,
    batch_size 50,000, val_freq 10 — for three iterations (eval, train, train). S E K' = 2,000 rows <
    b, so each epoch takes ONE partial minibatch of all 2,000 rows: the reference's past-the-end
    slice inds_k[0:50000] (agent :288-292, num_batch = max(1, total // b)). The agent runs it on the
    50,000-row workspace with rows = 2,000 (update.hip / the actor step take the partial layout) and
    must match the oracle loop at the fp32 tolerances of _run_and_compare. With 1,000-step episodes
    (250 chunks) no episode completes inside 50 chunks, as in the reference: the
    episode counts must agree (zero)."""
    a, orc = _agent_and_oracle(42, tmp_path, as_shipped=True)
    assert (a.n_envs, a.n_steps, a.batch_size, a.val_freq, a.model.precision) == (4, 50, 50000, 10, "fp32")
    # chains 1e-4 abs here, not 2e-5: without an episode end in 100 chunks (itr 1 continues itr 0's
    # envs, quirk 4) the fp32 action error is carried through 400 sub-steps of the env's dynamics
    # (obs differ by ~3e-5 at itr 2) instead of 40
    errs = _run_and_compare(a, orc, need_episodes=False, chains_tol=1e-4)
    _record("config1_as_shipped", errs)
    assert [e["eval"] for e in errs] == [True, False, False]
    assert orc.n_updates == 2 * a.update_epochs       # one (partial) minibatch per epoch, both train itrs


@pytest.mark.parametrize("threads", [1, 4])
def test_iterations_match_oracle_lowdim_env(cuda, tmp_path, threads):
    """The agent on the reference's wrapper stack (env.synthetic = lowdim: MultiStep +
    MujocoLocomotionLowdimWrapper batched in C over the C reference simulator, normalised by the
    reference's own hopper normalization.npz; env/lowdim.py) against the loop oracle over the
    per-env NumPy restatement of the same wrappers (oracle/envstack.py): the pipelined host path
    (the gated tagged step of csrc/envwrap.c on 1 or 4 host threads) with terminal states as well
    as truncations."""
    from oracle.envstack import LinearSimOracle, LowdimVecEnvOracle
    norm_path = os.path.join(ROOT, "tests", "golden", "hopper_medium_v2_normalization.npz")

    def env_oracle(a, cfg, seeds):
        sim = a.venv.sim
        nm = a.venv.norm
        sims = [LinearSimOracle(sim.A, sim.B, sim.c, sim.goal, sim.center, sim.scale, sim.bound, s) for s in seeds]
        return LowdimVecEnvOracle(sims, nm, cfg.obs_dim, cfg.action_dim, cfg.act_steps, cfg.env.max_episode_steps)

    a, orc = _agent_and_oracle(42, tmp_path, ["env.synthetic=lowdim", f"+env.num_threads={threads}",
                                              f"+env.wrappers.mujoco_locomotion_lowdim.normalization_path={norm_path}"],
                               env_oracle=env_oracle)
    from diffusionpolicyoptimization_amd.env.lowdim import LowdimVecEnv
    assert isinstance(a.venv, LowdimVecEnv) and a.venv.norm is not None and a.venv.num_threads == threads
    assert a.pipe is not None and a.venv.native is not None       # the gated (pipelined) host step runs
    errs = _run_and_compare(a, orc)
    _record(f"lowdim_env_t{threads}", errs)
