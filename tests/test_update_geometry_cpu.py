"""minibatch_geometry (agent/finetune/train_ppo_diffusion_agent.py): the minibatches of an epoch and a
rank's rows of a full one. One rank against the reference's own arithmetic as the loop oracle states
it (oracle/iteration.py `_update`: total = N * kf, num_batch = max(1, total // batch_size), slices of
batch_size rows); eight ranks against pairs worked out by hand from
    eff_batch = batch_size * (world if dp_scale_batch else 1)
    num_batch = max(1, total_local * world // eff_batch)
    rows_local_full = eff_batch // world
No device, no library."""
import pytest

from diffusionpolicyoptimization_amd.agent.finetune.train_ppo_diffusion_agent import minibatch_geometry


@pytest.mark.parametrize("total, batch_size", [
    (5760, 240),        # tests/test_iteration_gpu.py's small config: a multiple
    (5000, 240),        # not a multiple of batch_size: the 200-row remainder is dropped (:288-292)
    (320000, 50000),    # the 64-env benchmark: 6 minibatches, 20,000 rows left over
    (2000, 50000),      # config 1 as shipped: fewer rows than one minibatch, one partial minibatch
    (239, 240), (240, 240), (241, 240),
])
def test_one_rank_is_the_reference_arithmetic(total, batch_size):
    num_batch = max(1, total // batch_size)                  # oracle/iteration.py, agent :288
    for scale in (False, True):                              # one rank: dp_scale_batch changes nothing
        assert minibatch_geometry(total, batch_size, 1, scale) == (num_batch, batch_size)


def test_config1_as_shipped_is_one_minibatch():
    assert minibatch_geometry(4 * 50 * 10, 50000, 1, False)[0] == 1


@pytest.mark.parametrize("total_local, batch_size, scale, expect", [
    # the benchmark's rank of 8: 320,000 rows per rank, 2,560,000 in all
    (320000, 50000, False, (51, 6250)),     # 2,560,000 // 50,000 = 51 minibatches of 50,000 / 8 rows per rank
    (320000, 50000, True, (6, 50000)),      # 2,560,000 // 400,000 = 6 of 400,000 / 8 = batch_size rows per rank
    # a total that is no multiple of the minibatch
    (5000, 240, False, (166, 30)),          # 40,000 // 240 = 166 (160 rows left), 240 / 8 = 30
    (5000, 240, True, (20, 240)),           # 40,000 // 1,920 = 20 (1,600 rows left)
    # fewer rows in all than one minibatch
    (2000, 50000, False, (1, 6250)),        # 16,000 // 50,000 = 0 -> 1
    (2000, 50000, True, (1, 50000)),
    # a batch_size that 8 does not divide: the rank's share rounds down
    (1000, 100, False, (80, 12)),           # 8,000 // 100 = 80, 100 // 8 = 12
])
def test_eight_ranks(total_local, batch_size, scale, expect):
    assert minibatch_geometry(total_local, batch_size, 8, scale) == expect
