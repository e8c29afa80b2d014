"""ROUGE-L, the parts that need no GPU: the definition on the host (one-division form against the two-division form, word lists,
symmetry, empty sides, the corpus figure), the bit-vector recurrence of the kernel against the DP table, the case sets of the
kernel test, utilities on the host, the host dev pass, and the ABI."""
import math
import os
import random
import re

import numpy as np
import pytest

import util
import dev_bleu_ref
import rouge_ref as R
from fira_icse_amd import _lib, devset, metrics

WORDS = ["a", "b", "c", "d", "e", "f"]


def word_pairs():
    rnd = random.Random(414)
    out = [([], []), ([], ["a"]), (["a"], []), (["a"], ["a"]), (["a"], ["b"]), (["a", "b", "c"], ["c", "b", "a"]),
           (["a", "b", "c", "d"], ["b", "d"]), (["a"] * 30, ["a", "b", "a"])]
    for _ in range(600):
        alpha = WORDS[:rnd.randint(1, 6)]
        out.append(([rnd.choice(alpha) for _ in range(rnd.randint(0, 30))], [rnd.choice(alpha) for _ in range(rnd.randint(0, 30))]))
    return out


def test_one_division_form_is_within_one_ulp_of_the_two_division_form():
    """Every (lcs <= h, r <= 64): the value is the Python expression ``2.0 * lcs / (h + r)`` and lies within 1 ulp of
    ``2PR / (P + R)`` with ``P = lcs / h``, ``R = lcs / r``.  The two-division form is evaluated in RATIONAL arithmetic: written
    in floats it carries five roundings of its own (P, R, the product, the sum, the quotient) and is itself up to 2.5 ulp off
    its true value -- against that float evaluation the correctly rounded one-division value differs by more than 1 ulp on 636
    of the 89 440 triples with lcs >= 1 (at most 3 ulp, e.g. (3, 5, 21): 0.23076923076923078 against 0.23076923076923073),
    which says nothing about the function.  Measured here: at most 0.496 ulp from the exact value.  Both figures are printed."""
    from fractions import Fraction
    worst = worst_float = 0.0
    n_float_off = 0
    for h in range(0, 65):
        for r in range(0, 65):
            for lcs in range(0, min(h, r) + 1):
                got = metrics.rouge_l_from_stats(lcs, h, r)
                if lcs == 0:
                    assert got == 0.0
                    continue
                assert got == 2.0 * lcs / (h + r)
                p, rec = Fraction(lcs, h), Fraction(lcs, r)
                want = 2 * p * rec / (p + rec)
                dist = abs(Fraction(got) - want) / Fraction(math.ulp(got))
                worst = max(worst, float(dist))
                assert dist <= 1, (lcs, h, r, got, float(want))
                assert 0.0 < got <= 1.0
                pf, rf = lcs / h, lcs / r
                dist_f = abs(got - 2 * pf * rf / (pf + rf)) / math.ulp(got)
                worst_float, n_float_off = max(worst_float, dist_f), n_float_off + (dist_f > 1)
    print("largest distance from 2PR / (P + R): %.3f ulp (exact), %.1f ulp from its float evaluation (%d triples above 1 ulp)"
          % (worst, worst_float, n_float_off))


def test_rouge_l_on_word_lists():
    n_pos = n_zero = 0
    for hyp, ref in word_pairs():
        lcs = R.lcs_dp(hyp, ref)
        assert metrics.lcs_length(hyp, ref) == lcs == metrics.lcs_length(ref, hyp)
        got = metrics.rouge_l(ref, hyp)
        assert got == metrics.rouge_l_from_stats(lcs, len(hyp), len(ref))
        assert got == metrics.rouge_l(hyp, ref)                                       # symmetric (beta = 1)
        assert metrics.rouge_l(hyp, hyp) == (1.0 if hyp else 0.0)
        n_pos += got > 0
        n_zero += got == 0
    assert n_pos > 400 and n_zero >= 5
    assert metrics.rouge_l([], []) == 0.0 and metrics.rouge_l(["a"], []) == 0.0 and metrics.rouge_l([], ["a"]) == 0.0
    assert metrics.rouge_l(["a", "b", "c", "d"], ["b", "d"]) == 2.0 * 2 / 6
    assert metrics.rouge_l(["a", "b", "c"], ["c", "b", "a"]) == 2.0 * 1 / 6           # bag overlap 3, in-order overlap 1


def test_corpus_figure():
    refs = ["fix the bug", "add  a test\n", "", "x"]
    preds = ["fix bug", "a test added", "something", ""]
    want = 100.0 * math.fsum([2.0 * 2 / 5, 2.0 * 2 / 6, 0.0, 0.0]) / 4
    assert metrics.rouge_l_corpus(refs, preds) == want
    assert metrics.rouge_l_corpus(iter(refs), iter(preds)) == want
    assert metrics.rouge_l_corpus(["a b"], ["a b"]) == 100.0
    with pytest.raises(ValueError, match="2 references and 1 predictions"):
        metrics.rouge_l_corpus(["a", "b"], ["a"])


def bit_vector_lcs(a, b):
    """The recurrence csrc/rouge.hip runs, on Python ints cut to 64 bits: the positions of ``a`` are the bits."""
    mask = (1 << 64) - 1
    x = mask
    for c in b:
        m = sum(1 << p for p, w in enumerate(a) if w == c)
        u = x & m
        x = ((x + u) | (x - u)) & mask
    return len(a) - bin(x & ((1 << len(a)) - 1)).count("1")


def test_bit_vector_recurrence_is_the_dp():
    rnd = random.Random(7)
    pairs = [([7] * 64, [7] * 64), ([7] * 63, [7] * 63), (list(range(64)), list(range(64))), ([], []), ([1], []), ([], [1]),
             (list(range(62)) + [99], [99] + list(range(200, 240)))]
    for _ in range(3000):
        alpha = rnd.choice((1, 2, 3, 40))
        pairs.append(([rnd.randrange(alpha) for _ in range(rnd.choice((0, 1, 2, 63, 64, rnd.randint(0, 64))))],
                      [rnd.randrange(alpha) for _ in range(rnd.choice((0, 1, 2, 63, 64, rnd.randint(0, 64))))]))
    for a, b in pairs:
        assert bit_vector_lcs(a, b) == R.lcs_dp(a, b), (a, b)
    # bits at or above len(a) may hold anything: what lanes past the message ballot cannot reach the count
    for a, b in pairs[:400]:
        mask, x, junk = (1 << 64) - 1, (1 << 64) - 1, rnd.getrandbits(64) & ~((1 << len(a)) - 1)
        for c in b:
            u = x & (sum(1 << p for p, w in enumerate(a) if w == c) | junk)
            x = ((x + u) | (x - u)) & mask
        assert len(a) - bin(x & ((1 << len(a)) - 1)).count("1") == R.lcs_dp(a, b)


@pytest.fixture(scope="module")
def case_list():
    return R.all_cases()


def test_case_list_holds_every_property(case_list):
    cov = R.check_cases(case_list)
    assert len(cov) == 21
    for tokens, length in case_list:
        assert tokens.dtype == np.int32 and length.dtype == np.int32


def test_utilities_are_a_direct_loop(case_list):
    for tokens, length in case_list:
        stats = R.stats_ref_all(tokens, length)
        B, n, _ = tokens.shape
        want = [[math.fsum(metrics.rouge_l_from_stats(*[int(v) for v in stats[b, i, j, :3]]) for j in range(n) if j != i) / (n - 1)
                 if n > 1 else 0.0 for i in range(n)] for b in range(B)]
        assert metrics.mbr_utilities(stats, "rouge_l") == want == R.utilities_ref(tokens, length)
        assert metrics.mbr_utilities(stats.tolist(), utility="rouge_l") == want
        diag = stats[:, np.arange(n), np.arange(n)]
        assert np.array_equal(diag[:, :, 0], diag[:, :, 1]) and np.array_equal(diag[:, :, 1], diag[:, :, 2])
        assert np.array_equal(stats[..., 0], stats[..., 0].transpose(0, 2, 1)) and not stats[..., 3].any()
    assert metrics.mbr_utilities([[[[0, 0, 0, 0]]]], "rouge_l") == [[0.0]]
    assert metrics.mbr_utilities([], "rouge_l") == []


def test_unknown_utility_is_refused():
    for bad in ("rouge", "ROUGE_L", "meteor", None, 1):
        with pytest.raises(ValueError, match="utility"):
            metrics.mbr_utilities([[[[0, 0, 0, 0]]]], bad)
    row = [3, 2, 1, 0, 3, 2, 1, 0, 3, 3, 0, 0]
    assert metrics.mbr_utilities([[[row, row], [row, row]]]) == metrics.mbr_utilities([[[row, row], [row, row]]], "bleu")


def test_host_pass_fills_rouge_l_and_changes_nothing_else():
    cfg, store, r_vocab, var_maps, valid_index = dev_bleu_ref.synthetic_valid()
    table = dev_bleu_ref.label_ids_table(store, cfg, seed=0)
    make = lambda **kw: devset.DevEvaluator(None, store, cfg, r_vocab, var_maps, valid_index,
                                            ids_fn=dev_bleu_ref.table_ids_fn(table), device="cpu", **kw)
    plain, with_rouge = make(), make(rouge_l=True)
    total, lines = plain.host_pass()
    total_r, lines_r = with_rouge.host_pass()
    assert total_r == total and lines_r() == lines() and with_rouge.last_scores == plain.last_scores
    assert plain.last_rouge_l == [] and len(with_rouge.last_rouge_l) == len(store) == 23
    V, L, S = cfg.vocab_size, cfg.sou_len, cfg.sub_token_len
    want = [metrics.rouge_l_from_stats(*R.dev_stats_ref(table[i], store.sou[i], store.sub_token[i], store.tar[i], V, L, S, r_vocab)[:3])
            for i in range(len(store))]
    assert with_rouge.last_rouge_l == want and sum(v > 0 for v in want) >= 12


def test_entries_are_declared_exported_and_bound(lib):
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("fira_mbr_rouge_l_stats", 7), ("fira_dev_rouge_l_stats", 11)):
        proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert proto and len(proto.group(1).split(",")) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
        assert hasattr(lib, name)
    assert lib.fira_abi_version() == int(re.search(r"#define FIRA_ABI_VERSION (\d+)", header).group(1)) == 11
