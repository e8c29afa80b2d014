"""Gradient accumulation on the data-parallel paths (Trainer.step_many with distributed=True), in the two-rank gloo pattern of
tests/test_dp_gpu.py (both ranks on cuda:0): two ranks x 2 micro-batches must equal one process x 4 micro-batches at that
file's tolerances, with the collectives of a step WITHOUT accumulation -- the micro-batches ahead of the last meet none."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import util
from fira_icse_amd import data
from fira_icse_amd.config import FiraConfig

pytestmark = pytest.mark.gpu


def _run(rank, world, port, out, zero1=False):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, util.REPO)
    from fira_icse_amd.model import TransModel, DeviceBatch, reference_init_state_dict
    from fira_icse_amd.train import Trainer
    from fira_icse_amd.parallel import shard_indices
    from run_model import micro_batches
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = FiraConfig()
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = data.split_index(*util.GOLDEN_SPLIT, seed=0)["train"]
    torch.manual_seed(0)
    model = TransModel(cfg, init=False)
    model.load_state_dict(util.perturb_state_dict(reference_init_state_dict(cfg), seed=1))
    model.eval()                                        # dropout off: the comparison must be deterministic
    K = 4 // world                                      # 1 process x 4 micro-batches, 2 ranks x 2
    trainer = Trainer(model, distributed=world > 1, zero1=zero1, accum_steps=K)
    count = {"n": 0}
    for name in ("all_reduce", "reduce_scatter", "reduce_scatter_tensor", "all_gather", "all_gather_into_tensor", "broadcast"):
        real = getattr(dist, name)

        def counted(*a, _real=real, **k):
            count["n"] += 1
            return _real(*a, **k)
        setattr(dist, name, counted)
    losses, per_step, shapes = [], [], []
    for step in range(4):
        # steps 0 / 1: four commits -- every micro-batch holds one.  Step 2: THREE commits -- with two ranks, rank 1's shard is one
        # commit and its second micro-batch is empty.  Step 3: the plain step (no accumulation) on four commits, for its count
        gidx = idx[4 * step:4 * step + 4] if step != 2 else idx[8:11]
        mine = shard_indices(gidx, rank, world)
        n0 = count["n"]
        if step < 3:
            micro = micro_batches(mine, K)
            shapes.append([len(mb) for mb in micro])
            trainer.step_many([DeviceBatch(store.batch(mb), cfg) if mb else None for mb in micro])
        else:
            trainer.step(DeviceBatch(store.batch(mine), cfg))
        per_step.append(count["n"] - n0)
        losses.append(trainer.last_loss())
    assert trainer.t == 4
    if world > 1:
        assert shapes[2] == ([1, 1], [1, 0])[rank]       # the empty second micro-batch of rank 1
    else:
        assert shapes[2] == [1, 1, 1, 0]
    torch.cuda.synchronize()
    opt = trainer.state_dict()                              # collective with zero1
    if rank == 0:
        torch.save({"flat": model.flat.data.cpu(), "losses": losses, "m": opt["m"].cpu(), "v": opt["v"].cpu(),
                    "collectives": per_step}, out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("zero1", [False, True])
def test_two_ranks_of_two_micro_batches_equal_one_process_of_four(tmp_path, zero1):
    port = 29300 + (os.getpid() % 150) + (160 if zero1 else 0)
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    mp.spawn(_run, args=(1, port, one), nprocs=1, join=True)
    mp.spawn(_run, args=(2, port + 1, two, zero1), nprocs=2, join=True)
    a, b = torch.load(one, weights_only=False), torch.load(two, weights_only=False)
    for x, y in zip(a["losses"], b["losses"]):
        assert abs(x - y) / x < 1e-5, (a["losses"], b["losses"])        # the ACCUMULATED global mean token loss on every rank
    # tests/test_dp_gpu.py::test_two_rank_training_equals_single_process: the parameter change, element-wise
    cfg = FiraConfig()
    diff = (a["flat"] - b["flat"]).abs()
    assert float((diff > 0.05 * cfg.lr).float().mean()) < 2e-4, float(diff.max())
    assert float(diff.mean()) < 1e-3 * cfg.lr
    # collectives per step: the accumulated steps (the one with the empty micro-batch included) make as many as the plain step
    c = b["collectives"]
    assert c[3] > 0 and c[0] == c[1] == c[2] == c[3], c
    assert a["collectives"] == [0, 0, 0, 0]
