"""Data-parallel worker of tests/test_adv_clip_gpu.py::test_data_parallel_clip_equals_single_rank_on_the_union
(torch.distributed.run, 2 ranks): tools/dp_equiv.py's run from ft_ppo_diffusion_mlp_advclip.yaml. Each rank runs
one train iteration of the reference-batch DP agent and, at minibatch 0 of epoch 0, saves its rollout shard, its
row selection keys, the all-reduced gradient + metric sums and the update's table {count, sum, sumsq, lo, hi}
to $DPPO_EQUIV_DIR/rank<r>.npz."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import numpy as np
    import torch
    import torch.distributed as dist
    from dp_equiv import OVERRIDES

    from diffusionpolicyoptimization_amd.util.config import get_class, load_config
    out_dir = os.environ["DPPO_EQUIV_DIR"]
    rank = int(os.environ.get("RANK", "0"))
    cfg = load_config(os.path.join(ROOT, "cfg/gym/finetune/hopper-v2"), "ft_ppo_diffusion_mlp_advclip",
                      OVERRIDES + [f"logdir={out_dir}/log{rank}"])
    a = get_class(cfg._target_)(cfg)

    def hook(epoch, batch, start, rows):
        if (epoch, batch) != (0, 0):
            return
        torch.cuda.synchronize()
        m = a.model
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), obs=a.obs_traj.cpu().numpy(),
                 chains=a.chains_traj.cpu().numpy(), adv=a.adv.cpu().numpy(), grads=m.grads.cpu().numpy(),
                 metrics=m.metrics[:5].cpu().numpy(), clip=a._adv_clip.cpu().numpy(),
                 perm_seed=np.uint64(a.perm_seed), epoch=np.int64(1000 * a.itr), rows=np.int64(rows),
                 n_envs=np.int64(a.n_envs), world=np.int64(a.world_size), params=m.train_params.cpu().numpy())
    a.minibatch_hook = hook
    a.iteration(force_train=True)
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, f"rank{rank}_end.npz"), params=a.model.train_params.cpu().numpy(),
             steps=np.int64(a.actor_optimizer.iterations), clip=a._adv_clip.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
