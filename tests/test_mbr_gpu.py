"""MBR selection by expected sentence BLEU on the device: the all-pairs kernel against its Counter oracle (exact), rows that do
not depend on their neighbours or on what lies behind a length, the empty batch and the refusals, ``Searcher.mbr`` on sampled
candidates against the string scorer (``==``), and ``run_model.py test --sample N --rerank mbr_bleu``."""
import json
import math
import os

import numpy as np
import pytest
import torch

import util
import mbr_ref as R
from search_kit import golden_search, run_cli, spread_state_dict
from fira_icse_amd import _lib, metrics, ops, synth
from fira_icse_amd.config import FiraConfig

pytestmark = pytest.mark.gpu


def run_kernel(tokens, length):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return ops.mbr_bleu_stats(dev(tokens), dev(length)).cpu().numpy()


@pytest.fixture(scope="module")
def case_list():
    """The case sets with their oracle rows, computed once and left unchanged."""
    out = []
    for tokens, length in R.all_cases():
        out.append((tokens, length, R.stats_ref_all(tokens, length)))
    return out


@pytest.mark.parametrize("k", range(len(R.SHAPES)), ids=["B%d_n%d_T%d" % s for s in R.SHAPES])
def test_kernel_is_exactly_the_counter_oracle(case_list, k):
    tokens, length, want = case_list[k]
    assert tokens.shape == R.SHAPES[k]
    stats = run_kernel(tokens, length)
    assert stats.shape == want.shape and stats.dtype == np.int32
    assert np.array_equal(stats, want), np.argwhere(stats != want)[:5]
    diag = stats[:, np.arange(tokens.shape[1]), np.arange(tokens.shape[1])]
    assert np.array_equal(diag[:, :, 0:4], diag[:, :, 4:8]) and np.array_equal(diag[:, :, 8], diag[:, :, 9])


def test_kernel_rows_do_not_depend_on_their_neighbours(case_list):
    for tokens, length, want in case_list[:1] + case_list[3:5]:
        stats = run_kernel(tokens, length)
        for b in range(tokens.shape[0]):
            assert np.array_equal(run_kernel(tokens[b:b + 1], length[b:b + 1])[0], stats[b]), b


def test_kernel_ignores_what_lies_behind_a_length(case_list):
    for tokens, length, want in case_list:
        other = R.regarbage(tokens, length, seed=99)
        T = tokens.shape[2]
        behind = np.arange(T)[None, None, :] >= length[:, :, None]
        assert np.array_equal(other[~behind], tokens[~behind])
        if behind.any():
            assert (other[behind] != tokens[behind]).any()
        assert np.array_equal(run_kernel(other, length), want)


def test_kernel_with_no_commits_writes_nothing(case_list):
    tokens, length, _ = case_list[0]
    _, n, T = tokens.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t, l = dev(tokens), dev(length)
    stats = torch.full((2, n, n, 12), 77, dtype=torch.int32, device="cuda")
    rc = _lib.lib().fira_mbr_bleu_stats(_lib.cur_stream(), 0, n, T, _lib.ptr(t), _lib.ptr(l), _lib.ptr(stats))
    torch.cuda.synchronize()
    assert rc == 0 and bool((stats == 77).all())
    assert _lib.lib().fira_mbr_bleu_stats(_lib.cur_stream(), 0, n, T, None, None, None) == 0
    s0 = ops.mbr_bleu_stats(torch.empty((0, n, T), dtype=torch.int32, device="cuda"),
                            torch.empty((0, n), dtype=torch.int32, device="cuda"))
    assert tuple(s0.shape) == (0, n, n, 12)


def test_kernel_refuses_what_it_cannot_serve(case_list):
    tokens, length, _ = case_list[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t, l = dev(tokens), dev(length)
    stats = torch.full((5, 8, 8, 12), 77, dtype=torch.int32, device="cuda")
    lib, s = _lib.lib(), _lib.cur_stream()
    p = _lib.ptr
    for args, word in (((1, 33, 30, p(t), p(l), p(stats)), b"n = 33"), ((1, 0, 30, p(t), p(l), p(stats)), b"n = 0"),
                       ((1, 8, 65, p(t), p(l), p(stats)), b"T = 65"), ((1, 8, 0, p(t), p(l), p(stats)), b"T = 0"),
                       ((-1, 8, 30, p(t), p(l), p(stats)), b"B = -1"), ((1, 8, 30, None, p(l), p(stats)), b"null pointer"),
                       ((1, 8, 30, p(t), None, p(stats)), b"null pointer"), ((1, 8, 30, p(t), p(l), None), b"null pointer")):
        assert lib.fira_mbr_bleu_stats(s, *args) != 0, args
        assert word in lib.fira_last_error(), (word, lib.fira_last_error())
    torch.cuda.synchronize()
    assert bool((stats == 77).all())
    with pytest.raises(_lib.FiraError, match="n = 33"):
        ops.mbr_bleu_stats(torch.zeros((1, 33, 30), dtype=torch.int32, device="cuda"),
                           torch.zeros((1, 33), dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------------------------ Searcher.mbr
@pytest.fixture(scope="module")
def sampled():
    g = golden_search(weights="spread")
    search, db = g.searchers[0], g.db
    draws = [search.sample(db, 4, temperature=1.3, top_k=30, seed=seed) for seed in (5, 6)]
    return search, draws


def check_mbr(search, toks, lens, logp):
    pick, util_ = search.mbr(toks, lens, logp)
    B, n, _ = toks.shape
    want = R.utilities_ref(toks.cpu().numpy(), lens.cpu().numpy())
    assert util_.dtype == torch.float64 and tuple(util_.shape) == (B, n) and not util_.is_cuda
    assert util_.tolist() == want
    assert pick == R.pick_ref(want, logp.tolist())
    assert search.mbr(toks, lens)[0] == R.pick_ref(want)
    return pick, want


def test_searcher_mbr_on_sampled_candidates(sampled):
    search, draws = sampled
    (toks, lens, _, logp), (toks2, lens2, _, logp2) = draws
    B = toks.shape[0]
    msgs = [[tuple(R.words(toks[b, i].tolist(), int(lens[b, i]))) for i in range(4)] for b in range(B)]
    assert all(len(set(m)) >= 2 for m in msgs), "the temperature should give candidates that differ"
    pick, want = check_mbr(search, toks, lens, logp)
    print("utilities", want, "pick", pick, "arg-max logp", logp.argmax(1).tolist())
    assert any(u > 0 for row in want for u in row)
    # two draws pooled along n
    pooled = (torch.cat([toks, toks2], 1), torch.cat([lens, lens2], 1), torch.cat([logp, logp2], 1))
    assert pooled[0].shape[1] == 8
    check_mbr(search, *pooled)
    # one candidate: utility 0, pick 0
    p1, u1 = search.mbr(toks[:, :1], lens[:, :1], logp[:, :1])
    assert p1 == [0] * B and u1.tolist() == [[0.0]] * B
    # int32 inputs and CPU inputs are the same thing
    assert search.mbr(toks.int().cpu(), lens.int().cpu(), logp.cpu())[0] == pick


def test_searcher_mbr_refuses_bad_arguments(sampled, monkeypatch):
    search, draws = sampled
    toks, lens, _, logp = draws[0]
    launched = []
    monkeypatch.setattr(ops, "mbr_bleu_stats", lambda *a, **k: launched.append(1))
    for args in ((toks[0], lens[0]), (toks, lens[:, :3]), (toks.repeat(1, 9, 1), lens.repeat(1, 9)),
                 (torch.cat([toks, toks, toks], 2), lens), (toks[:, :, :0], lens), (toks.float(), lens),
                 (toks, lens.float()), (toks + (1 << 40), lens), (toks, lens, logp[:, :2])):
        with pytest.raises(ValueError):
            search.mbr(*args)
    assert not launched


# ------------------------------------------------------------------------------------------------ command line
def test_cli_rerank_mbr_bleu(tmp_path):
    """The ``mbr_bleu`` values are compared with the string scorer on the WORDS of the written candidates: no variable map of
    the synthetic root maps a placeholder back to a vocabulary word (asserted below), so ids and words are interchangeable."""
    root = str(tmp_path)
    raw = util.load_golden_raw()
    for var_map in raw["variable"]:
        back = {v: k for k, v in var_map.items()}
        assert len(back) == len(var_map) and not any(orig in raw["word_vocab"] for orig in back.values())
    synth.write_dataset(root, raw)
    torch.save(spread_state_dict(FiraConfig()), os.path.join(root, "best_model.pt"))
    base = ["test", "--splits", "16,4,4", "--test-batch-size", "3"]
    opts = ["--sample", "4", "--temperature", "1.2", "--top-k", "30", "--sample-seed", "5"]
    out_f, samp_f = os.path.join(root, "OUTPUT", "output_fira"), os.path.join(root, "OUTPUT", "output_fira_samples")
    run_cli(base + opts + ["--rerank", "mbr_bleu"], root)
    lines, recs = open(out_f).read().split("\n"), [json.loads(l) for l in open(samp_f).read().strip().split("\n")]
    assert len(lines) == 5 and lines[-1] == "" and len(recs) == 4
    differ = 0
    for line, rec in zip(lines, recs):
        assert sorted(rec) == ["candidates", "logp", "mbr_bleu"] and len(rec["candidates"]) == len(rec["mbr_bleu"]) == 4
        ws = [c.split() for c in rec["candidates"]]
        want = [math.fsum(metrics.sentence_bleu_method2([ws[j]], ws[i]) for j in range(4) if j != i) / 3 for i in range(4)]
        assert rec["mbr_bleu"] == want
        pick = R.pick_ref([rec["mbr_bleu"]], [rec["logp"]])[0]
        assert line == rec["candidates"][pick]
        differ += pick != int(np.argmax(rec["logp"]))
    print("commits whose pick differs from the arg-max of logp: %d of 4" % differ)
    # the same command without --rerank, run afterwards: the same candidates, the pick and the fields of before
    run_cli(base + opts, root)
    lines0, recs0 = open(out_f).read().split("\n"), [json.loads(l) for l in open(samp_f).read().strip().split("\n")]
    assert len(lines0) == 5 and lines0[-1] == "" and len(recs0) == 4
    for line, rec0, rec in zip(lines0, recs0, recs):
        assert sorted(rec0) == ["candidates", "logp"]
        assert rec0["candidates"] == rec["candidates"] and rec0["logp"] == rec["logp"]
        assert line == rec0["candidates"][int(np.argmax(rec0["logp"]))]
