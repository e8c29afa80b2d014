"""Gradient accumulation on the device (Trainer.step_many; include/fira_hip.h: fira_accum_stats, fira_train_accum_micro,
fira_train_accum_last): one optimizer step over several micro-batches must be the step of their concatenation.

The golden batch (util.GOLDEN_B commits) with dropout off, split into micro-batches.  The training step is not bit-reproducible
run to run (atomic column sums, the ReLU tie of the golden batch), so gradients are compared at the project's
gradient gate (rel-L2 1e-4) and trainers at the floors tests/test_adam_rows_gpu.py uses for its rows-vs-dense comparison."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import util
from fira_icse_amd import data, synth
from fira_icse_amd.config import FiraConfig

pytestmark = pytest.mark.gpu

GRAD_GATE = 1e-4                                                  # rel-L2 the project gates gradients at
# tests/test_adam_rows_gpu.py:184-185 (test_rows_trainer_equals_dense_trainer): dist < 6 * noise + floor, noise = two runs of the
# SAME trainer against each other
FLOORS = {"params": 1e-4, "m": 1e-2, "v": 1e-3}
# bf16 (that file has no bf16 floors): the distance of the bf16 big-batch step against itself, the largest over three steps and
# the six pairs of four runs measured on an MI355X (scripts/accum_probe.py --noise); the test allows twice that
BF16_SELF = {"params": 4.92e-6, "m": 6.56e-3, "v": 8.13e-4}


def dist(x, y):
    return float((x.double() - y.double()).norm() / y.double().norm())


@pytest.fixture(scope="module")
def gold():
    from fira_icse_amd.model import reference_init_state_dict
    cfg = FiraConfig()
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = list(data.split_index(*util.GOLDEN_SPLIT, seed=0)["train"][:util.GOLDEN_B])
    torch.manual_seed(0)
    sd = util.perturb_state_dict(reference_init_state_dict(cfg), seed=1)
    return cfg, store, idx, sd


def make_model(gold, dtype="f32"):
    from fira_icse_amd.model import TransModel
    cfg, _, _, sd = gold
    model = TransModel(cfg, init=False)
    model.load_state_dict(sd)
    model.compute_dtype = dtype
    model.eval()                                                  # dropout off
    return model


def batches(gold, sizes):
    from fira_icse_amd.model import DeviceBatch
    cfg, store, idx, _ = gold
    out, lo = [], 0
    for n in sizes:
        out.append(DeviceBatch(store.batch(idx[lo:lo + n]), cfg))
        lo += n
    assert lo == len(idx)
    return out


def snapshot(tr):
    tr.sync()
    live = tr.model.layout.live
    return {"params": tr.model.flat.data[:live].clone(), "m": tr.m[:live].clone(), "v": tr.v[:live].clone()}


# ------------------------------------------------------------------------------------------------ 1. the stats kernel
def test_stats_kernel_is_the_numpy_loop_bit_for_bit():
    """fira_accum_stats over a sequence of (loss_sum, n_tok, first) against a numpy float32 / int32 loop: first = 1 on a dirty
    buffer (a nan and a stale total), n_tok = 0, and a total above 2^24 -- odd, so float(total) rounds while the int32 holds
    it exactly -- then first = 1 again."""
    from fira_icse_amd import ops
    dev = "cuda"
    stats = torch.tensor([float("nan"), 123.0], dtype=torch.float32, device=dev)
    total = torch.tensor([77], dtype=torch.int32, device=dev)
    seq = [(3.25, 17, 1), (1e-3, 0, 0), (12345.678, 9_000_000, 0), (0.1, 9_000_001, 0), (7.0, 1, 0), (2.5, 3, 1), (0.0, 0, 0)]
    ref_l, ref_n = np.float32(0), np.int32(0)
    for loss, n, first in seq:
        ls = torch.tensor([loss], dtype=torch.float32, device=dev)
        nt = torch.tensor([n], dtype=torch.int32, device=dev)
        ops.accum_stats(ls, nt, stats, total, bool(first))
        ref_l = np.float32((np.float32(0) if first else ref_l) + np.float32(loss))
        ref_n = np.int32((np.int32(0) if first else ref_n) + np.int32(n))
        got = stats.cpu().numpy()
        assert got[0] == ref_l and got[1] == np.float32(ref_n), (loss, n, first, got, ref_l, ref_n)
        assert int(total.item()) == int(ref_n)
        assert float(ls.item()) == float(np.float32(loss)) and int(nt.item()) == n          # the inputs are read only
        if (loss, n) == (7.0, 1):                                # 18 000 019: above 2^24 and odd -- no float holds it
            assert int(ref_n) == 18_000_019 > 2 ** 24 and float(got[1]) != 18_000_019.0
    assert int(total.item()) == 3
    # the same in one call, first = 1 over a dirty pair
    stats.fill_(5.0); total.fill_(9)
    ops.accum_stats(torch.tensor([1.0], device=dev), torch.tensor([18_000_001], dtype=torch.int32, device=dev), stats, total, True)
    assert int(total.item()) == 18_000_001 and float(stats[1].item()) == float(np.float32(18_000_001)) != 18_000_001.0


# ------------------------------------------------------------------------------------------------ 2. the gradient is the sum
@pytest.mark.parametrize("sizes", [(2, 2), (3, 1)])
def test_accumulated_gradient_is_the_sum_of_the_micro_batch_gradients(gold, sizes, monkeypatch):
    """gbuf after step_many([a, b]) against gbuf_a + gbuf_b of two train_fwd_bwd(zero_grad=True) calls, rel-L2 < 1e-4 (the
    engine's gradient is not bit-reproducible: atomic column sums).  Seen on an MI355X: 2 + 2: 1.43e-7, 3 + 1:
    1.41e-7; two runs of the SAME separate calls against each other: 1.37e-7 / 1.36e-7.  n_tok: the exact sum.  loss_sum: the fp32 sum
    of the two values this run's micro-batches produced, to the rounding of that one addition (2^-24 relative), and within
    the project's loss gate (1e-5) of the separate calls' values."""
    from fira_icse_amd import ops
    from fira_icse_amd.train import Trainer
    model = make_model(gold)
    live = model.layout.live
    a, b = batches(gold, sizes)
    sep, again = [], []
    for db in (a, b):
        l, n = model.train_fwd_bwd(db, zero_grad=True)
        sep.append((model.gbuf[:live].clone(), float(l.item()), int(n.item())))
        model.train_fwd_bwd(db, zero_grad=True)
        again.append(model.gbuf[:live].clone())
    want = sep[0][0] + sep[1][0]
    seen = []
    real = ops.accum_stats

    def spy(loss_sum, n_tok, *rest):
        seen.append((float(loss_sum.item()), int(n_tok.item())))
        return real(loss_sum, n_tok, *rest)
    monkeypatch.setattr(ops, "accum_stats", spy)
    tr = Trainer(model)
    tr.step_many([a, b])
    torch.cuda.synchronize()
    got = model.gbuf[:live]
    d, noise = dist(got, want), dist(again[0] + again[1], want)
    print("accumulated gradient %s: rel-L2 %.3g, two separate runs %.3g" % (sizes, d, noise))
    assert d < GRAD_GATE, (d, noise)
    assert float(got.abs().max()) > 0
    # the stats: micro-batch 1 through ops.accum_stats (seen), the last one inside the library (model.loss_sum holds it)
    assert len(seen) == 1
    la, na = seen[0]
    lb, nb = float(model.loss_sum.item()), int(model.n_tok.item())
    assert (na, nb) == (sep[0][2], sep[1][2])
    assert int(tr.n_tok_total.item()) == na + nb and float(tr.stats[1].item()) == float(na + nb)
    s = float(tr.stats[0].item())
    assert s == float(np.float32(np.float32(la) + np.float32(lb)))
    assert abs(s - (la + lb)) <= 2.0 ** -24 * (la + lb)
    assert abs(s - (sep[0][1] + sep[1][1])) <= 1e-5 * s
    assert abs(tr.last_loss() - s / (na + nb)) <= 1e-6 * tr.last_loss()


# ------------------------------------------------------------------------------------------------ 3. the big batch
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_equivalence_with_the_big_batch(gold, dtype):
    """step on the 4 golden commits against step_many on their 2 + 2 split, same weights, zero moments, three consecutive
    steps, parameters / m / v after sync().  fp32: dist < 6 * noise + floor with the floors and the form of
    tests/test_adam_rows_gpu.py:184-185, noise = a second big-batch run against the first.  bf16 (no floors there): twice the
    distance of the bf16 big-batch step against itself as measured on an MI355X (largest of three steps, six pairs of runs:
    params 4.92e-6, m 6.56e-3, v 8.13e-4 = BF16_SELF; the same measurement in fp32: 3.6e-8 / 6.9e-7 / 6.3e-7).  Seen for
    step_many against step: fp32 params 2.4e-8 / m 9.1e-7 / v 8.2e-7 (two big-batch runs: 2.8e-8 / 6.3e-7 / 5.4e-7); bf16
    params 5.5e-6 / m 6.2e-3 (step 2; two big-batch runs in the same test: 3.7e-6 / 6.4e-3)."""
    from fira_icse_amd.train import Trainer
    (big,), (a, b) = batches(gold, (4,)), batches(gold, (2, 2))
    runs = {}
    for name in ("big", "big2", "accum"):
        model = make_model(gold, dtype)
        tr = Trainer(model)
        snaps = []
        for _ in range(3):
            if name == "accum":
                tr.step_many([a, b])
            else:
                tr.step(big)
            snaps.append(snapshot(tr))
        assert tr.t == 3
        runs[name] = snaps
    for step in range(3):
        for key in ("params", "m", "v"):
            d = dist(runs["accum"][step][key], runs["big"][step][key])
            noise = dist(runs["big2"][step][key], runs["big"][step][key])
            print("big batch vs 2 + 2, %s step %d %s: %.3g (two big-batch runs %.3g)" % (dtype, step + 1, key, d, noise))
            bound = 6 * noise + FLOORS[key] if dtype == "f32" else 2 * BF16_SELF[key]
            assert d < bound, (dtype, step, key, d, noise)


# ------------------------------------------------------------------------------------------------ 4. rows == dense
def test_row_sparse_equals_dense_under_accumulation():
    """Four step_many calls of two micro-batches (four synthetic commits each) whose touched word rows differ, row-sparse against
    FIRA_ADAM_ROWS=0 (switched as tests/test_adam_rows_gpu.py switches it): after sync() tables, moments and row_step agree at
    that file's floors (noise = a second dense run).  Before the sync, every encoder-table row that only the FIRST micro-batch
    of a step touched carries that step's stamp: the update saw the union of the micro-batches' rows."""
    from fira_icse_amd.model import DeviceBatch, TransModel
    from fira_icse_amd.train import Trainer
    cfg = FiraConfig()
    store = data.process_raw(cfg, synth.generate_dataset(32, seed=11))
    V = cfg.vocab_size
    hbs = [store.batch(list(range(4 * i, 4 * i + 4))) for i in range(8)]

    def enc_ids(hb):
        ids = set(np.asarray(hb.sou).reshape(-1).tolist()) | set(np.asarray(hb.sub_token).reshape(-1).tolist())
        return {i for i in ids if 0 < i < V}
    out = {}
    for run, rows in (("rows", "1"), ("dense", "0"), ("dense2", "0")):
        os.environ["FIRA_ADAM_ROWS"] = rows
        try:
            torch.manual_seed(0)
            model = TransModel(cfg, device="cuda")
            model.eval()
            tr = Trainer(model, accum_steps=2)
        finally:
            os.environ.pop("FIRA_ADAM_ROWS", None)
        assert (tr.row_step is not None) == (rows == "1") and tr.accum_steps == 2
        dbs = [DeviceBatch(hb, cfg, model.device_) for hb in hbs]
        for i in range(4):
            ia, ib = enc_ids(hbs[2 * i]), enc_ids(hbs[2 * i + 1])
            assert not ia <= ib and not ib <= ia                 # neither micro-batch's rows contain the other's
            tr.step_many([dbs[2 * i], dbs[2 * i + 1]])
            if rows == "1":
                stamps = tr.row_step[V:].cpu().numpy()           # (decoder table first)
                first_only = sorted(ia - ib)
                assert first_only and (stamps[first_only] == i + 1).all(), (i, stamps[first_only])
                assert (stamps[sorted(ib)] == i + 1).all()
                assert int(tr.row_step.min()) < i + 1            # ... and rows nobody touched still lag
        assert tr.t == 4
        snap = snapshot(tr)
        sd = model.state_dict()
        snap["encoder.embedding"], snap["decoder.embedding"] = sd["encoder.embedding.weight"].clone(), sd["decoder.embedding.weight"].clone()
        if rows == "1":
            assert int(tr.row_step.min()) == int(tr.row_step.max()) == 4
        out[run] = snap
    for key in ("params", "m", "v", "encoder.embedding", "decoder.embedding"):
        d, noise = dist(out["rows"][key], out["dense"][key]), dist(out["dense2"][key], out["dense"][key])
        print("rows vs dense under accumulation, %s: %.3g (two dense runs %.3g)" % (key, d, noise))
        assert d < 6 * noise + FLOORS.get(key, 1e-4), (key, d, noise)


# ------------------------------------------------------------------------------------------------ 5. bookkeeping
def test_one_step_of_bookkeeping_for_three_micro_batches(gold):
    """step_many of K = 3 (2 + 1 + 1 commits): t, the inv-sqrt rate of step t, exactly one EMA update (the numpy float32
    expression on the synced weights), and the clip state: the norm of the ACCUMULATED gradient over the TOTAL token count.
    fira_grad_sqsum's header bound is (D + 1) * 2^-24 relative on each bucket's sum of squares (D = 19 for the live
    parameters); the square root halves a relative error and the sum of the two buckets, the root and the product with
    1 / count add three roundings, so the norm is held to the same (D + 1) * 2^-24."""
    from fira_icse_amd import ops
    from fira_icse_amd.train import Trainer
    model = make_model(gold)
    live = model.layout.live
    sched = {"kind": "inv-sqrt", "base_lr": 2e-4, "warmup_steps": 4}
    tr = Trainer(model, lr_schedule=sched, ema_decay=0.9, ema_every=1, clip_grad_norm=1e-3)
    e0 = tr.ema.cpu().numpy().copy()
    tr.step_many(batches(gold, (2, 1, 1)))
    assert tr.t == 1
    want_lr = ops.lr_at(ops.LrSchedule.make(sched), 1)
    assert tr.last_lr() == want_lr and abs(want_lr - 2e-4 / 4) < 1e-9
    assert tr.ema_updates == 1
    ema = tr.ema.cpu().numpy()                                  # (taken before the sync: the rows entry reads lazily)
    tr.sync()
    p = model.flat.data.cpu().numpy()
    w = np.float32(ops.ema_weight(0.9, 1))
    assert np.array_equal(ema, (e0 + w * (p - e0).astype(np.float32)).astype(np.float32))
    assert not np.array_equal(ema, e0)
    norm, coef, n_clipped, n_nonfinite = tr.last_grad_norm()
    n_tok = int(tr.n_tok_total.item())
    assert n_tok == int(tr.stats[1].item()) > int(model.n_tok.item()) > 0          # the total, not the last micro-batch's
    ref = float(torch.linalg.norm(model.gbuf[:live].double())) / n_tok
    D = max(ops.grad_sqsum_depth(model.layout.split), ops.grad_sqsum_depth(live - model.layout.split), ops.grad_sqsum_depth(live))
    print("accumulated clip norm %.9g, reference %.9g, rel %.3g (bound %.3g)" % (norm, ref, abs(norm - ref) / ref, (D + 1) * 2.0 ** -24))
    assert abs(norm - ref) <= (D + 1) * 2.0 ** -24 * ref, (norm, ref)
    assert norm > 1e-3 and n_clipped == 1 and n_nonfinite == 0
    assert abs(coef - 1e-3 / (norm + 1e-6)) <= 1e-6 * coef
    assert abs(tr.last_loss() - float(tr.stats[0].item()) / n_tok) < 1e-6


# ------------------------------------------------------------------------------------------------ 6. None entries
def test_none_entries_are_skipped(gold):
    """step_many([None, db, None]) == step_many([db]) at test 3's floors (both are step(db): the noise is two runs of it);
    step_many([None, None]) on one device changes nothing."""
    from fira_icse_amd.train import Trainer
    (big,) = batches(gold, (4,))
    runs = {}
    for name, dbs in (("plain", [big]), ("plain2", [big]), ("holes", [None, big, None])):
        tr = Trainer(make_model(gold))
        tr.step_many(dbs)
        assert tr.t == 1
        runs[name] = snapshot(tr)
    for key in ("params", "m", "v"):
        d, noise = dist(runs["holes"][key], runs["plain"][key]), dist(runs["plain2"][key], runs["plain"][key])
        assert d < 6 * noise + FLOORS[key], (key, d, noise)
    tr = Trainer(make_model(gold))
    tr.step(big)
    before = (tr.t, tr.model.flat.data.clone(), tr.m.clone(), tr.v.clone())
    tr.step_many([None, None])
    torch.cuda.synchronize()
    assert tr.t == before[0] == 1
    assert torch.equal(tr.model.flat.data, before[1]) and torch.equal(tr.m, before[2]) and torch.equal(tr.v, before[3])
    with pytest.raises(ValueError):
        tr.step_many([])


# ------------------------------------------------------------------------------------------------ 7. option off
class RecordingLib:
    """_lib.lib() with the name of every call kept in order (tests/test_ensemble_gpu.py: CountingLib)."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def recorded(*args):
            self.calls.append(name)
            return fn(*args)
        return recorded


@pytest.mark.parametrize("clip", [None, 1.0])
def test_one_micro_batch_makes_the_library_calls_of_step(gold, monkeypatch, clip):
    from fira_icse_amd import _lib
    from fira_icse_amd.train import Trainer
    (big,), (a, b) = batches(gold, (4,)), batches(gold, (2, 2))
    tr = Trainer(make_model(gold), clip_grad_norm=clip)
    tr.step(big)                                                  # (workspaces, streams and the first sync are behind us --
    tr.step_many([a, b])                                          #  for the micro-batches' shape too: fira_workspace_bytes)
    seqs = []
    for run in (lambda: tr.step(big), lambda: tr.step_many([big]), lambda: tr.step_many([a, b])):
        lib = RecordingLib(_lib.lib())
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "_lib", lib)
            run()
        torch.cuda.synchronize()
        seqs.append(lib.calls)
    assert seqs[0] == seqs[1] and len(seqs[0]) >= 1
    assert not any("accum" in name for name in seqs[0])
    assert seqs[2] == ["fira_train_accum_micro", "fira_accum_stats", "fira_train_accum_last"]


# ------------------------------------------------------------------------------------------------ 8. the command line
def test_cli_accum_steps_two_epochs(tmp_path):
    """run_model.py train --accum-steps 2 --batch-size 4 --no-dropout for two epochs on the golden synthetic DataSet (16 train
    commits: 4 optimizer steps per epoch): one --loss-log line per optimizer step, each with micro = 2 and the positions of the
    whole global batch; the first line's loss equals the big-batch run's to 1e-5 (the project's loss gate)."""
    recs = {}
    for name, extra in (("accum", ["--accum-steps", "2"]), ("plain", ["--max-steps", "1"])):
        root = str(tmp_path / name)
        os.makedirs(root)
        synth.write_dataset(root, util.load_golden_raw())
        log = os.path.join(root, "loss.jsonl")
        env = dict(os.environ, PYTHONPATH=util.REPO)
        r = subprocess.run([sys.executable, os.path.join(util.REPO, "run_model.py"), "train", "--splits", "16,4,4", "--batch-size",
                            "4", "--dev-from-epoch", "99", "--epochs", "2", "--no-dropout", "--loss-log", log] + extra, cwd=root,
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        with open(log) as f:
            recs[name] = [json.loads(l) for l in f.read().splitlines()]
    acc, plain = recs["accum"], recs["plain"]
    assert len(acc) == 2 * 4 and len(plain) == 1
    assert all(r["micro"] == 2 and len(r["index"]) == 4 for r in acc)
    assert "micro" not in plain[0]
    assert [r["epoch"] for r in acc] == [0] * 4 + [1] * 4 and [r["batch"] for r in acc] == [0, 1, 2, 3] * 2
    assert acc[0]["index"] == plain[0]["index"]
    assert abs(acc[0]["loss"] - plain[0]["loss"]) <= 1e-5 * plain[0]["loss"], (acc[0], plain[0])
    assert all(np.isfinite(r["loss"]) and r["loss"] > 0 for r in acc)
