"""The multi-process training path on a real GPU: two ranks (both on cuda:0, gloo transport so that one device is
enough) run the sharded step -- fused fwd+bwd with the mid-event, two-bucket all-reduce on a side stream, global token
normaliser, fused Adam -- and must end with the same parameters as one process stepping on the whole global batch."""
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


def _run(rank, world, port, out, zero1=False, backend="gloo", wire="f32"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, util.REPO)
    if backend == "nccl":                                   # RCCL: one rank per device
        torch.cuda.set_device(rank)
    from fira_icse_amd.model import TransModel, DeviceBatch, reference_init_state_dict
    from fira_icse_amd.train import Trainer
    from fira_icse_amd.parallel import shard_indices
    if world > 1:
        dist.init_process_group(backend, rank=rank, world_size=world)
    cfg = FiraConfig()
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = data.split_index(*util.GOLDEN_SPLIT, seed=0)["train"]
    torch.manual_seed(0)
    model = TransModel(cfg, init=False)
    model.load_state_dict(util.perturb_state_dict(reference_init_state_dict(cfg), seed=1))
    model.eval()                                        # dropout off: the comparison must be deterministic
    trainer = Trainer(model, distributed=world > 1, zero1=zero1, grad_wire=wire)
    if world > 1 and not zero1:
        assert trainer.fused_dp                         # (round 6) fira_train_step_begin / _end with the collectives in between
    losses = []
    m_first = None
    for step in range(3):
        # the last global batch holds ONE commit: with two ranks, rank 1's shard is empty (DataParallel.scatter chunking)
        # and it must still join the collectives and apply the same Adam update (deadlock / divergence)
        gidx = idx[4 * step:4 * step + 4] if step < 2 else idx[8:9]
        mine = shard_indices(gidx, rank, world)
        trainer.step(DeviceBatch(store.batch(mine), cfg) if mine else None)
        losses.append(trainer.last_loss())
        if step == 0 and (zero1 or world == 1):
            m_first = trainer.state_dict()["m"].cpu()           # (collective with zero1) first moment after the FIRST update
    torch.cuda.synchronize()
    opt = trainer.state_dict()                              # collective with zero1 (shards gathered onto every rank)
    if rank == 0:
        torch.save({"flat": model.flat.data.cpu(), "losses": losses, "m": opt["m"].cpu(), "v": opt["v"].cpu(), "m_first": m_first}, out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_rank_training_equals_single_process(tmp_path):
    port = 29800 + (os.getpid() % 150)
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    mp.spawn(_run, args=(1, port, one), nprocs=1, join=True)
    mp.spawn(_run, args=(2, port + 1, two), nprocs=2, join=True)
    a, b = torch.load(one, weights_only=False), torch.load(two, weights_only=False)
    for x, y in zip(a["losses"], b["losses"]):
        assert abs(x - y) / x < 1e-5, (a["losses"], b["losses"])        # GLOBAL mean token loss on every rank
    # Adam normalises the update magnitude to ~lr, so compare the parameter *change* over the three steps
    cfg = FiraConfig()
    # (element-wise; the attention fc_k.bias entries are excluded by the quantile: their true gradient is zero, both
    # runs hold rounding noise there and Adam turns noise of either sign into a +-lr step)
    diff = (a["flat"] - b["flat"]).abs()
    assert float((diff > 0.05 * cfg.lr).float().mean()) < 2e-4, float(diff.max())
    assert float(diff.mean()) < 1e-3 * cfg.lr


def test_two_ranks_with_bf16_gradient_wire_track_single_process(tmp_path):
    """Trainer(grad_wire="bf16"): the two buckets travel as bf16 (cast -> all-reduce -> widen; BASELINE configs[2]).  The update
    is no longer bit-comparable -- every gradient carries a 2^-9 relative rounding -- but three steps must stay on the
    single-process trajectory: global losses within 1e-3, parameters within a fraction of the Adam step."""
    port = 29350 + (os.getpid() % 150)
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    mp.spawn(_run, args=(1, port, one), nprocs=1, join=True)
    mp.spawn(_run, args=(2, port + 1, two, False, "gloo", "bf16"), nprocs=2, join=True)
    a, b = torch.load(one, weights_only=False), torch.load(two, weights_only=False)
    assert abs(a["losses"][0] - b["losses"][0]) / a["losses"][0] < 1e-5        # (the first loss precedes any update)
    for x, y in zip(a["losses"], b["losses"]):
        assert abs(x - y) / x < 1e-3, (a["losses"], b["losses"])
    cfg = FiraConfig()
    diff = (a["flat"] - b["flat"]).abs()
    assert float(diff.mean()) < 0.05 * cfg.lr, float(diff.mean())
    d = (a["m"] - b["m"]).norm() / a["m"].norm()
    assert 1e-6 < float(d) < 1e-2, float(d)                                    # (the wire really was bf16; first moments agree)


def test_two_rank_zero1_equals_single_process(tmp_path):
    """reduce-scatter + Adam on the owned shard + all-gather (Trainer(zero1=True)): same parameters, and the gathered Adam
    moments equal the single-process moments (checkpoints are interchangeable between the modes)."""
    port = 29500 + (os.getpid() % 150)
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    mp.spawn(_run, args=(1, port, one), nprocs=1, join=True)
    mp.spawn(_run, args=(2, port + 1, two, True), nprocs=2, join=True)
    a, b = torch.load(one, weights_only=False), torch.load(two, weights_only=False)
    for x, y in zip(a["losses"], b["losses"]):
        assert abs(x - y) / x < 1e-5, (a["losses"], b["losses"])
    cfg = FiraConfig()
    diff = (a["flat"] - b["flat"]).abs()
    assert float((diff > 0.05 * cfg.lr).float().mean()) < 2e-4, float(diff.max())
    assert float(diff.mean()) < 1e-3 * cfg.lr
    _check_moments(a, b)


def _check_moments(a, b):
    """Moments: the same accumulation up to the reduction order.  The first update is compared tightly (the forward pass of
    step 0 is bit-identical between the runs).  From the second step on the runs' parameters differ by the rounding noise
    of the float atomics, and on this batch one hidden unit of decoder layer 3 (feed_forward fc1, unit 693) sits at a ReLU tie in
    step 1: its pre-activation is +-1e-9, so either run may take either side -- the loss does not see it (relu(h) ~ 0 both ways),
    but the mask does: row 693 of that weight's gradient changes wholesale and everything below it by ~5e-4
    (scripts/probes/nondet_probe.py finds the same two outcomes between two SINGLE-process runs; profiles/r6_probes.md).  A flip
    moves |dm| / |m| to 9.5e-4, so the three-step moments get 3e-3; v (squares: the small gradients hardly count) stays tight."""
    d1 = (a["m_first"] - b["m_first"]).norm() / a["m_first"].norm()
    assert float(d1) < 1e-5, float(d1)
    dm = (a["m"] - b["m"]).norm() / a["m"].norm()
    assert float(dm) < 3e-3, float(dm)
    dv = (a["v"] - b["v"]).norm() / a["v"].norm()
    assert float(dv) < 1e-4, float(dv)


needs_two_gpus = pytest.mark.skipif(torch.cuda.device_count() < 2,
                                    reason="RCCL between two devices needs >= 2 visible GPUs (one-GPU box: gloo tests above)")


@needs_two_gpus
@pytest.mark.parametrize("zero1", [False, True])
def test_two_ranks_over_rccl_equal_single_process(tmp_path, zero1):
    """The same comparison with backend "nccl" (= RCCL over xGMI), one rank per device -- the transport the reference's
    multi-GPU mode implies (run_model.py:392-394) and the one bench.py --gpus N uses.  zero1: the native
    reduce_scatter_tensor / all_gather_into_tensor branch of parallel.ShardedOptimizerComm, which gloo cannot reach.
    SKIPPED on the one-GPU boxes of the build pool; runs wherever two devices are visible."""
    port = 29650 + (os.getpid() % 150) + (7 if zero1 else 0)
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    mp.spawn(_run, args=(1, port, one), nprocs=1, join=True)
    mp.spawn(_run, args=(2, port + 1, two, zero1, "nccl"), nprocs=2, join=True)
    a, b = torch.load(one, weights_only=False), torch.load(two, weights_only=False)
    for x, y in zip(a["losses"], b["losses"]):
        assert abs(x - y) / x < 1e-5, (a["losses"], b["losses"])
    cfg = FiraConfig()
    diff = (a["flat"] - b["flat"]).abs()
    assert float((diff > 0.05 * cfg.lr).float().mean()) < 2e-4, float(diff.max())
    assert float(diff.mean()) < 1e-3 * cfg.lr
    if zero1:
        _check_moments(a, b)
    else:
        for k, tol in (("m", 3e-3), ("v", 1e-4)):          # (m: see _check_moments -- a ReLU tie in step 1)
            d = (a[k] - b[k]).norm() / a[k].norm()
            assert float(d) < tol, (k, float(d))


@needs_two_gpus
def test_bench_two_gpus_over_rccl():
    """`python bench.py --gpus 2` with one rank per device: the line must say backend nccl and carry the collective timings."""
    import json
    import subprocess
    cmd = [sys.executable, os.path.join(util.REPO, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full",
           "--no-decode", "--no-cpu-baseline", "--no-extras"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["process_group"]["backend"] == "nccl" and line["value"] > 0


def test_bench_self_launches_under_torchrun():
    """`python bench.py --gpus 2` (what the driver runs) re-launches itself with one process per rank and prints exactly
    one JSON line; on a one-GPU box both ranks share cuda:0 over gloo."""
    import json
    import subprocess
    cmd = [sys.executable, os.path.join(util.REPO, "bench.py"), "--gpus", "2", "--dp-same-device", "--steps", "3",
           "--warmup", "1", "--full", "--no-decode", "--no-cpu-baseline", "--no-extras"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["process_group"]["rccl_world_size"] == 2
    assert line["config"]["global_batch"] == 64 and line["value"] > 0
