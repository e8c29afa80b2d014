"""Dev-set model selection on the device: the BLEU kernel against its string oracle (exact), the device pass against the
host pass (== totals, identical lines), sharding, the resident set, and ``run_model.py train --dev-on-device``."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import util
import dev_bleu_ref as R
from fira_icse_amd import _lib, devset, ops, synth

pytestmark = pytest.mark.gpu

SHAPE = (30, 12, 7, 5)                      # T, V, L, S


def run_kernel(ids, sou, sub, tar, V):
    dev = lambda a: torch.from_numpy(a).cuda()
    hyp, stats = ops.dev_bleu_stats(dev(ids), dev(sou), dev(sub), dev(tar), V)
    return stats.cpu().numpy(), hyp.cpu().numpy()


def reference(ids, sou, sub, tar, V, L, S):
    rows = [R.stats_ref(ids[b], sou[b], sub[b], tar[b], V, L, S) for b in range(ids.shape[0])]
    return np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows], dtype=np.int32)


@pytest.fixture(scope="module")
def cases():
    T, V, L, S = SHAPE
    c = R.kernel_cases(37, T, V, L, S, seed=0)
    return c, reference(*c, V, L, S)


def test_kernel_is_exactly_the_string_oracle(cases):
    T, V, L, S = SHAPE
    (ids, sou, sub, tar), (want_stats, want_hyp) = cases
    cov = R.coverage(ids, sou, sub, tar, V, L, S)
    assert all(cov.values()), cov                                   # every edge case of the list is among the rows
    stats, hyp = run_kernel(ids, sou, sub, tar, V)
    assert np.array_equal(stats, want_stats), np.argwhere(stats != want_stats)[:5]
    assert np.array_equal(hyp, want_hyp), np.argwhere(hyp != want_hyp)[:5]
    # B = 1 (a workgroup with one live wave)
    for b in (3, 36):
        stats1, hyp1 = run_kernel(ids[b:b + 1], sou[b:b + 1], sub[b:b + 1], tar[b:b + 1], V)
        assert np.array_equal(stats1, want_stats[b:b + 1]) and np.array_equal(hyp1, want_hyp[b:b + 1])


def test_kernel_with_no_commits_writes_nothing(cases):
    T, V, L, S = SHAPE
    (ids, sou, sub, tar), _ = cases
    dev = lambda a: torch.from_numpy(a).cuda()
    hyp = torch.full((2, T), 77, dtype=torch.int32, device="cuda")
    stats = torch.full((2, 12), 77, dtype=torch.int32, device="cuda")
    rc = _lib.lib().fira_dev_bleu_stats(_lib.cur_stream(), 0, T, V, L, S, _lib.ptr(dev(ids)), _lib.ptr(dev(sou)), _lib.ptr(dev(sub)),
                                        _lib.ptr(dev(tar)), _lib.ptr(hyp), _lib.ptr(stats))
    torch.cuda.synchronize()
    assert rc == 0 and bool((hyp == 77).all()) and bool((stats == 77).all())
    e = torch.empty((0, T), dtype=torch.int32, device="cuda")
    h0, s0 = ops.dev_bleu_stats(e, torch.empty((0, L), dtype=torch.int32, device="cuda"),
                                torch.empty((0, S), dtype=torch.int32, device="cuda"), e.clone(), V)
    assert tuple(h0.shape) == (0, T) and tuple(s0.shape) == (0, 12)
    # arguments the kernel cannot serve are refused with a message, not launched
    lib = _lib.lib()
    assert lib.fira_dev_bleu_stats(_lib.cur_stream(), 1, 65, V, L, S, None, None, None, None, None, None) != 0
    assert b"T = 65" in lib.fira_last_error()
    assert lib.fira_dev_bleu_stats(_lib.cur_stream(), 1, T, V, L, S, None, None, None, None, None, None) != 0
    assert b"null" in lib.fira_last_error()
    assert lib.fira_dev_bleu_stats(_lib.cur_stream(), -1, T, V, L, S, None, None, None, None, None, None) != 0


def test_kernel_rows_do_not_depend_on_their_neighbours(cases):
    T, V, L, S = SHAPE
    (ids, sou, sub, tar), _ = cases
    stats, hyp = run_kernel(ids, sou, sub, tar, V)
    for b in range(ids.shape[0]):
        s1, h1 = run_kernel(ids[b:b + 1], sou[b:b + 1], sub[b:b + 1], tar[b:b + 1], V)
        assert np.array_equal(s1[0], stats[b]) and np.array_equal(h1[0], hyp[b]), b


def test_kernel_at_the_widest_row():
    """T = 64: every lane holds a position, the full-width masks and the reads past lane 63 are in play."""
    T, V, L, S = 64, 12, 7, 5
    c = R.kernel_cases(9, T, V, L, S, seed=3)
    want_stats, want_hyp = reference(*c, V, L, S)
    stats, hyp = run_kernel(*c, V)
    assert np.array_equal(stats, want_stats) and np.array_equal(hyp, want_hyp)
    assert int(want_stats[:, 8].max()) == 64


@pytest.fixture(scope="module")
def valid():
    """23 synthetic valid commits at batch 8 (tail batch of 7), a model with seeded weights, injected ids."""
    from fira_icse_amd.model import TransModel
    cfg, store, r_vocab, var_maps, valid_index = R.synthetic_valid(23, 8)
    torch.manual_seed(0)
    model = TransModel(cfg)
    model.eval()
    table = R.label_ids_table(store, cfg, seed=0)
    return dict(cfg=cfg, store=store, args=(r_vocab, var_maps, valid_index), model=model, table=table)


def evaluator(v, injected, rank=0, world=1):
    return devset.DevEvaluator(v["model"], v["store"], v["cfg"], *v["args"], rank=rank, world=world,
                               ids_fn=R.table_ids_fn(v["table"]) if injected else None)


@pytest.mark.parametrize("injected", [False, True], ids=["forward_dev", "injected_ids"])
def test_device_pass_equals_host_pass(valid, injected):
    ev = evaluator(valid, injected)
    assert [db_len for db_len in (len(ev.mine[lo:lo + ev.bs]) for lo in range(0, 23, ev.bs))] == [8, 8, 7]
    h_total, h_lines = ev.host_pass()
    h_scores = list(ev.last_scores)
    d_total, d_lines = ev.device_pass()
    print("total host %r device %r, non-zero commits %d of 23" % (h_total, d_total, sum(s > 0 for s in h_scores)))
    assert d_total == h_total
    assert ev.last_scores == h_scores
    assert "\n".join(d_lines()) == "\n".join(h_lines())
    assert len(d_lines()) == 23
    if injected:
        assert h_total / 23 > 0 and sum(s > 0 for s in h_scores) >= 12
    assert [db.B for db in ev._batches] == [8, 8, 7] and ev.resident_bytes > 23 * 10000


def test_sharded_evaluators_add_up_to_one(valid):
    one = evaluator(valid, True)
    total, _ = one.device_pass()
    scores, lines = list(one.last_scores), one.device_pass()[1]()
    parts, part_scores, part_lines = [], [], []
    for rank in (0, 1):
        ev = evaluator(valid, True, rank, 2)
        t, l = ev.device_pass()
        assert ev.bs == 4 and len(ev.mine) == (12 if rank == 0 else 11)
        parts.append(t)
        part_scores += ev.last_scores
        part_lines += l()
    assert part_scores == scores and part_lines == lines
    assert abs(sum(parts) - total) <= 1e-12 * max(1.0, total)       # (two partial sums: the association differs)


def test_resident_set_is_built_once(valid, monkeypatch):
    ev = evaluator(valid, True)
    calls = []
    real = valid["store"].batch
    monkeypatch.setattr(valid["store"], "batch", lambda idx: (calls.append(len(idx)), real(idx))[1])
    first_total, first_lines = ev.device_pass()
    first_lines = first_lines()
    assert calls == [8, 8, 7]
    del calls[:]
    # later collates (a training step's, a host pass) must not disturb the resident batches
    ev.host_pass()
    assert calls == [8, 8, 7]
    del calls[:]
    again_total, again_lines = ev.device_pass()
    assert calls == []
    assert again_total == first_total and again_lines() == first_lines


def test_cli_train_with_dev_on_device(tmp_path):
    root = str(tmp_path)
    synth.write_dataset(root, util.load_golden_raw())
    env = dict(os.environ, PYTHONPATH=util.REPO)
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "run_model.py"), "train", "--splits", "16,4,4", "--batch-size", "4",
                        "--epochs", "3", "--dev-from-epoch", "1", "--dev-every", "2", "--dev-on-device"], cwd=root, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    proc = open(os.path.join(root, "OUTPUT", "train_process")).read().strip().split("\n")
    assert len(proc) == 4                                            # epochs 1, 2 x batches 0, 2
    for line, (epoch, batch) in zip(proc, ((1, 0), (1, 2), (2, 0), (2, 2))):
        assert line.startswith("epoch: %d batch: %d dev bleu: " % (epoch, batch)), line
        assert line.endswith("is better: True") or line.endswith("is better: False"), line
    assert proc[0].endswith("is better: True")
    out = open(os.path.join(root, "OUTPUT", "dev_output")).read()
    assert out.endswith("\n") and len(out.strip().split("\n")) == 4
    # dev_output is written with the last better pass: its per-commit scores, summed in file order, are that pass's mean.
    # (best_model.pt holds the weights of that same pass -- dev() runs and saves before the step -- but scoring it again in
    #  another process would lean on run-to-run bit equality of forward_dev, which is not promised: left out.)
    best = [float(l.split("dev bleu: ")[1].split(" is better")[0]) for l in proc if l.endswith("True")][-1]
    total = 0.0
    for l in out.strip("\n").split("\n"):
        total += float(l.rsplit(",", 1)[1])
    assert total / 4 == best
    assert os.path.exists(os.path.join(root, "best_model.pt"))
