"""MBR selection by expected sentence BLEU, the parts that need no GPU: the inputs of the kernel test hold every edge case, its
Counter oracle agrees with the string scorer, utilities and tie-breaking on the host, the command line, and the ABI."""
import argparse
import math
import os
import re

import numpy as np
import pytest

import util
import mbr_ref as R
from fira_icse_amd import _lib, metrics
from run_model import RERANK_KEYS, check_score_args, parse_args


@pytest.fixture(scope="module")
def case_list():
    return R.all_cases()


def test_case_list_holds_every_edge_case(case_list):
    assert [c[0].shape for c in case_list] == [(5, 8, 30), (3, 1, 30), (1, 2, 30), (2, 32, 30), (3, 5, 64), (7, 3, 1)]
    cov = R.coverage(case_list)
    assert len(cov) == 14 and all(cov.values()), cov
    # the first shape alone holds them too (it carries all eight hand-made candidates)
    cov = R.coverage(case_list[:1])
    assert all(cov.values()), cov
    for tokens, length in case_list:
        assert tokens.dtype == np.int32 and length.dtype == np.int32 and int(tokens.min()) >= 0 and int(tokens.max()) < R.V + 40


def test_stats_oracle_agrees_with_the_string_scorer(case_list):
    n_pos = n_zero = 0
    for tokens, length in case_list:
        B, n, _ = tokens.shape
        for b in range(B):
            ws = [R.as_text(R.words(tokens[b, i], length[b, i])) for i in range(n)]
            for i in range(n):
                for j in range(n):
                    st = R.stats_ref(tokens[b, i], length[b, i], tokens[b, j], length[b, j])
                    want = metrics.sentence_bleu_method2([ws[j]], ws[i])
                    assert metrics.bleu_method2_from_stats(st[0:4], st[4:8], st[8], st[9]) == want, (b, i, j)
                    assert st[8] == len(ws[i]) and st[9] == len(ws[j]) and st[10:] == [0, 0]
                    if i == j:
                        assert st[0:4] == st[4:8]
                    n_pos += want > 0
                    n_zero += want == 0
    assert n_pos > 500 and n_zero > 100


def test_utilities_from_oracle_stats_are_the_string_scorers(case_list):
    for tokens, length in case_list:
        assert metrics.mbr_utilities(R.stats_ref_all(tokens, length)) == R.utilities_ref(tokens, length)


def test_utilities_on_a_hand_made_array():
    def row(num, cnt, hl, rl):
        return list(num) + list(cnt) + [hl, rl, 0, 0]

    full = row([3, 2, 1, 0], [3, 2, 1, 0], 3, 3)                      # a 3-word hypothesis against itself
    half = row([2, 1, 0, 0], [3, 2, 1, 0], 3, 4)
    none = row([0, 0, 0, 0], [3, 2, 1, 0], 3, 2)
    empty = row([0, 0, 0, 0], [0, 0, 0, 0], 0, 3)
    stats = [[[full, half, none], [half, full, half], [empty, empty, empty]]]
    s_full = metrics.bleu_method2_from_stats([3, 2, 1, 0], [3, 2, 1, 0], 3, 3)
    s_half = metrics.bleu_method2_from_stats([2, 1, 0, 0], [3, 2, 1, 0], 3, 4)
    assert 0 < s_half < s_full
    u = metrics.mbr_utilities(stats)
    # the diagonal never counts; a pair without a common unigram and an empty hypothesis score 0
    assert u == [[math.fsum([s_half, 0.0]) / 2, math.fsum([s_half, s_half]) / 2, 0.0]]
    assert metrics.mbr_utilities(np.array(stats, dtype=np.int32)) == u
    assert metrics.mbr_utilities([[[full]], [[empty]]]) == [[0.0], [0.0]]            # n = 1
    assert metrics.mbr_utilities([]) == []
    assert metrics.mbr_pick(u) == [1]


def test_pick_breaks_ties_by_logp_then_by_index():
    assert metrics.mbr_pick([[0.1, 0.5, 0.2]]) == [1]
    assert metrics.mbr_pick([[0.5, 0.5, 0.2]]) == [0]
    assert metrics.mbr_pick([[0.5, 0.5, 0.2]], [[-3.0, -1.0, -0.1]]) == [1]           # equal utilities: the larger logp
    assert metrics.mbr_pick([[0.5, 0.5, 0.5]], [[-1.0, -2.0, -1.0]]) == [0]           # equal both: the lower index
    assert metrics.mbr_pick([[0.0, 0.0, 0.0, 0.0]], [[-4.0, -2.0, -2.0, -9.0]]) == [1]   # disjoint candidates all score 0
    assert metrics.mbr_pick([[0.3, 0.9]], [[-0.1, -50.0]]) == [1]                      # logp only decides ties
    assert metrics.mbr_pick([[0.0]]) == [0] and metrics.mbr_pick([[0.0]], [[-7.0]]) == [0]      # n = 1
    assert metrics.mbr_pick([[0.2, 0.4], [0.4, 0.2]], np.zeros((2, 2))) == [1, 0]
    assert metrics.mbr_pick([]) == []
    rows = [[0.25, 0.5, 0.5, 0.125], [0.0, 0.0, 0.0, 0.0]]
    lp = [[-1.0, -3.0, -2.0, -0.5], [-2.0, -1.0, -1.0, -3.0]]
    assert metrics.mbr_pick(rows, lp) == R.pick_ref(rows, lp) == [2, 1]
    with pytest.raises(ValueError):
        metrics.mbr_pick([[0.1, 0.2]], [[-1.0]])


def test_command_line():
    assert RERANK_KEYS == ("logp_word", "mean_logp_word", "mbr_bleu")
    a = parse_args(["test", "--sample", "4", "--rerank", "mbr_bleu"])
    assert (a.sample, a.rerank, a.beam, a.score) == (4, "mbr_bleu", 1, None)
    a = parse_args(["test", "--sample", "1", "--rerank", "mbr_bleu"])
    assert (a.sample, a.rerank) == (1, "mbr_bleu")
    for argv in (["test", "--rerank", "mbr_bleu"], ["test", "--score", "refs", "--rerank", "mbr_bleu"],
                 ["test", "--sample", "4", "--rerank", "mbr_bleu", "--beam", "3"],
                 ["test", "--sample", "4", "--rerank", "mbr_bleu", "--score", "refs"]):
        with pytest.raises(SystemExit):
            parse_args(argv)
    ns = dict(stage="test", score=None, rerank="mbr_bleu", sample=None, beam=None)
    with pytest.raises(ValueError, match="--sample"):
        check_score_args(argparse.Namespace(**ns))
    with pytest.raises(ValueError, match="--sample"):
        check_score_args(argparse.Namespace(**dict(ns, score="refs")))
    with pytest.raises(ValueError, match="--sample"):
        check_score_args(argparse.Namespace(**dict(ns, score="refs", sample=4)))
    check_score_args(argparse.Namespace(**dict(ns, sample=4)))


def test_entry_is_declared_exported_and_bound(lib):
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+fira_mbr_bleu_stats\s*\(", code)
    assert hasattr(lib, "fira_mbr_bleu_stats")
    assert "fira_mbr_bleu_stats" in _lib.SIGNATURES and len(_lib.SIGNATURES["fira_mbr_bleu_stats"][1]) == 7
    assert lib.fira_abi_version() == int(re.search(r"#define FIRA_ABI_VERSION (\d+)", header).group(1)) == 11
