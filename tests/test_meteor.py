"""METEOR with exact (and caller-supplied class) matches, the parts that need no GPU: the ranked alignment of
``metrics.meteor_alignment`` against the literal two-loop oracle, the hand-derived cases, symmetry, the score's expression, the
corpus figure, utilities on the host, the host dev pass, and the ABI."""
import math
import os
import random
import re

import numpy as np
import pytest

import util
import dev_bleu_ref
import meteor_ref as R
from fira_icse_amd import _lib, devset, metrics

WORDS = ["a", "b", "c", "d", "e", "f"]
MERGE = {"a": 0, "b": 0, "c": 1, "d": 1, "e": 2}                          # "f" has no class


def word_pairs():
    rnd = random.Random(515)
    out = [([], []), ([], ["a"]), (["a"], []), (["a"] * 64, ["a"] * 64), (["a"] * 64, ["b", "a", "a", "c", "a"]),
           (WORDS * 10 + WORDS[:4], WORDS[::-1] * 10 + WORDS[:4])]
    for _ in range(500):
        alpha = WORDS[:rnd.randint(1, 6)]
        out.append(([rnd.choice(alpha) for _ in range(rnd.randint(0, 64))], [rnd.choice(alpha) for _ in range(rnd.randint(0, 64))]))
    return out


@pytest.fixture(scope="module")
def pairs():
    return word_pairs()


def test_alignment_is_the_literal_two_loop_oracle(pairs):
    assert max(len(h) for h, _ in pairs) == 64 and min(len(r) for _, r in pairs) == 0
    n_multi = 0
    for hyp, ref in pairs:
        want = R.align_ref(hyp, ref)
        assert metrics.meteor_alignment(ref, hyp) == want, (hyp, ref)
        assert 0 <= want[0] <= min(len(hyp), len(ref)) and (want[1] >= 1) == (want[0] >= 1) and want[1] <= want[0]
        assert want[0] == sum(min(hyp.count(w), ref.count(w)) for w in set(hyp))      # stage 1 matches the whole bag overlap
        n_multi += want[1] > 1
    assert n_multi > 300


def test_alignment_with_a_class_table_that_merges_words(pairs):
    more = 0
    for hyp, ref in pairs:
        want = R.align_ref(hyp, ref, MERGE.get)
        assert metrics.meteor_alignment(ref, hyp, MERGE) == want, (hyp, ref)
        assert metrics.meteor_alignment(ref, hyp, MERGE.get) == want                  # a callable
        more += want[0] > R.align_ref(hyp, ref)[0]
    assert more > 100                                                                 # the second stage does match
    # an integer table indexed by integer words; words outside it have no class
    rnd = random.Random(3)
    table = [0, 0, 1, 1, 2, 5]
    for _ in range(300):
        hyp = [rnd.choice([0, 1, 2, 3, 4, 5, -1, 6, 1 << 40]) for _ in range(rnd.randint(0, 40))]
        ref = [rnd.choice([0, 1, 2, 3, 4, 5, -1, 6, 1 << 40]) for _ in range(rnd.randint(0, 40))]
        want = R.align_ref(hyp, ref, R.table_key(table))
        assert metrics.meteor_alignment(ref, hyp, table) == want
        assert metrics.meteor_alignment(ref, hyp, np.asarray(table, dtype=np.int32)) == want
    assert metrics.meteor_alignment([6], [-1], table) == (0, 0) and metrics.meteor_alignment([0], [1], table) == (1, 1)


def test_hand_derived_cases():
    for n in (1, 2, 5, 27, 64):
        ws = ["w%d" % i for i in range(n)]
        assert metrics.meteor_alignment(ws, ws) == (n, 1)
        assert metrics.meteor_exact(ws, ws) == 1 - 0.5 / n ** 3
        assert metrics.meteor_alignment(["x"] * n, ["x"] * n) == (n, 1)
    hyp, ref = "on the mat sat the cat".split(), "the cat sat on the mat".split()
    assert metrics.meteor_alignment(ref, hyp) == (6, 6) == R.align_ref(hyp, ref)
    assert metrics.meteor_exact(ref, hyp) == 0.5
    assert metrics.meteor_exact(["a", "b"], ["c", "d"]) == 0.0 == metrics.meteor_exact([], ["a"]) == metrics.meteor_exact(["a"], [])
    assert metrics.meteor_exact([], []) == 0.0
    # counts 3 against 2 of one word: the LAST two occurrences pair -- hypothesis x at 0, 2, 4 and reference x at 0, 1: (2, 0)
    # and (4, 1), which no chunk joins; were the FIRST two paired, (0, 0) alone would stand at the start
    hyp, ref = ["x", "p", "x", "q", "x"], ["x", "x", "r"]
    assert metrics.meteor_alignment(ref, hyp) == (2, 2) == R.align_ref(hyp, ref)
    hyp, ref = ["x", "x", "p", "x"], ["q", "x", "x"]                                # (3, 2) and (1, 1); hypothesis 0 stays free
    assert metrics.meteor_alignment(ref, hyp) == (2, 2)
    hyp, ref = ["x", "p", "x", "x"], ["q", "x", "x"]                                # (2, 1) and (3, 2): one chunk
    assert metrics.meteor_alignment(ref, hyp) == (2, 1)


def walk_alignment(a, b, key=None):
    """The form csrc/meteor.hip runs, on Python ints as the 64-bit masks: ``b`` is walked from its last position to its first,
    each free position takes the HIGHEST free position of ``a`` with an equal key; the partner of a position of ``a`` is kept,
    and a match continues a chunk iff the next position's partner is its own plus one."""
    a_free, b_free = (1 << len(a)) - 1, (1 << len(b)) - 1
    partner = [-1] * 64

    def step(a_keys, j, b_key, a_ok):
        nonlocal a_free, b_free
        cand = sum(1 << i for i, k in enumerate(a_keys) if k == b_key) & a_free & a_ok
        if cand:
            i = cand.bit_length() - 1
            a_free &= ~(1 << i)
            b_free &= ~(1 << j)
            partner[i] = j

    for j in range(len(b) - 1, -1, -1):
        step(a, j, b[j], ~0)
    if key is not None:
        ka, kb = [key(w) for w in a], [key(w) for w in b]
        a_has = sum(1 << i for i, k in enumerate(ka) if k is not None)
        for j in range(len(b) - 1, -1, -1):
            if b_free >> j & 1 and kb[j] is not None:
                step(ka, j, kb[j], a_has)
    m = sum(p >= 0 for p in partner)
    nxt = partner[1:] + partner[-1:]                                    # lane 63 reads itself
    return m, m - sum(p >= 0 and q == p + 1 for p, q in zip(partner, nxt))


def test_walking_either_side_is_the_two_loop_oracle(pairs):
    for hyp, ref in pairs:
        for key in (None, MERGE.get):
            want = R.align_ref(hyp, ref, key)
            assert walk_alignment(hyp, ref, key) == want == walk_alignment(ref, hyp, key), (hyp, ref)


def test_score_is_the_stated_expression():
    for m, chunks, h, r in ((1, 1, 1, 1), (3, 2, 5, 4), (6, 6, 6, 6), (10, 1, 27, 10), (64, 64, 64, 64), (2, 1, 64, 3)):
        p, rec = m / h, m / r
        assert metrics.meteor_exact_from_stats(m, chunks, h, r) == (1 - 0.5 * (chunks / m) ** 3) * (p * rec / (0.9 * p + 0.1 * rec))
    assert metrics.meteor_exact_from_stats(0, 0, 5, 7) == 0.0 == metrics.meteor_exact_from_stats(0, 0, 0, 0)
    # recall-weighted: a short hypothesis inside a long reference scores below a long hypothesis that covers a short reference
    assert metrics.meteor_exact_from_stats(3, 1, 3, 9) < metrics.meteor_exact_from_stats(3, 1, 9, 3)


def test_alignment_is_symmetric_and_none_is_the_identity_table(pairs):
    ident = {w: w for w in WORDS}
    for hyp, ref in pairs:
        assert metrics.meteor_alignment(ref, hyp) == metrics.meteor_alignment(hyp, ref)
        assert R.align_ref(hyp, ref) == R.align_ref(ref, hyp)
        assert metrics.meteor_alignment(ref, hyp, MERGE) == metrics.meteor_alignment(hyp, ref, MERGE)
        assert metrics.meteor_alignment(ref, hyp, ident) == metrics.meteor_alignment(ref, hyp)
        assert metrics.meteor_exact(ref, hyp, ident) == metrics.meteor_exact(ref, hyp, None)


def test_corpus_figure_and_its_errors():
    refs = ["fix the bug", "add  a test\n", "", "x"]
    preds = ["fix bug", "a test added", "something", ""]
    want = 100.0 * math.fsum([metrics.meteor_exact(r.split(), p.split()) for r, p in zip(refs, preds)]) / 4
    assert want > 0 and metrics.meteor_exact_corpus(refs, preds) == want == metrics.meteor_exact_corpus(iter(refs), iter(preds))
    assert metrics.meteor_exact(["fix", "the", "bug"], ["fix", "bug"]) == metrics.meteor_exact_from_stats(2, 2, 2, 3)
    assert metrics.meteor_exact_corpus(["a b"], ["a b"]) == 100.0 * (1 - 0.5 / 8)
    assert metrics.meteor_exact_corpus(["a"], ["b"], {"a": 1, "b": 1}) == 100.0 * 0.5
    for fn, name in ((metrics.meteor_exact_corpus, "meteor_exact_corpus"), (metrics.rouge_l_corpus, "rouge_l_corpus")):
        with pytest.raises(ValueError, match="%s: 2 references and 1 predictions" % name):
            fn(["a", "b"], ["a"])
        with pytest.raises(ValueError, match="%s: no lines" % name):
            fn([], [])


@pytest.fixture(scope="module")
def pair_cases():
    return R.all_pair_cases()[:4]


def test_utilities_are_a_direct_loop(pair_cases):
    assert "meteor_exact" in metrics.MBR_UTILITIES
    for tokens, length in pair_cases:
        B, n, _ = tokens.shape
        for classes in (None, R.merging_table(R.PAIR_V)):
            stats = R.stats_ref_all(tokens, length, classes)
            table = None if classes is None else classes.tolist()
            want = []
            for b in range(B):
                ws = [R.words(tokens[b, i], length[b, i]) for i in range(n)]
                want.append([math.fsum(metrics.meteor_exact(ws[j], ws[i], table) for j in range(n) if j != i) / (n - 1)
                             if n > 1 else 0.0 for i in range(n)])
            assert metrics.mbr_utilities(stats, "meteor_exact") == want
            assert metrics.mbr_utilities(stats.tolist(), utility="meteor_exact") == want
            # the two facts the kernel uses: m and chunks do not depend on the roles; the diagonal needs no alignment
            assert np.array_equal(stats[..., :2], stats[..., :2].transpose(0, 2, 1, 3))
            assert np.array_equal(stats[..., 2], stats[..., 3].transpose(0, 2, 1))
            d = stats[:, np.arange(n), np.arange(n)]
            assert np.array_equal(d[..., 0], d[..., 2]) and np.array_equal(d[..., 2], d[..., 3])
            assert np.array_equal(d[..., 1], (d[..., 0] > 0).astype(np.int32))
    assert metrics.mbr_utilities([[[[0, 0, 0, 0]]]], "meteor_exact") == [[0.0]]
    assert metrics.mbr_utilities([], "meteor_exact") == []
    for bad in ("meteor", "METEOR_EXACT", "meteor-exact"):
        with pytest.raises(ValueError, match="utility"):
            metrics.mbr_utilities([[[[0, 0, 0, 0]]]], bad)


def test_pair_cases_hold_what_the_kernel_test_needs():
    cases = R.all_pair_cases()
    assert [c[0].shape for c in cases] == R.PAIR_SHAPES
    tokens, length = cases[3]
    ws = [R.words(tokens[0, i], length[0, i]) for i in range(8)]
    assert ws[0] == [7] * 63 and ws[1].count(7) == 3 and ws[2] == []
    assert R.align_ref(ws[0], ws[1]) == (3, 3) and R.align_ref(ws[3], ws[4])[0] == 5
    assert any(w < 0 for w in ws[5]) and any(w > 1 << 30 for w in ws[5])
    table = R.merging_table(R.PAIR_V)
    assert len(set(table.tolist())) < R.PAIR_V and any(c < 0 for c in table.tolist())
    more = sum(int((R.stats_ref_all(t, l, table)[..., 0] > R.stats_ref_all(t, l)[..., 0]).sum()) for t, l in cases[:4])
    assert more > 20


def test_host_pass_fills_meteor_exact_and_changes_nothing_else():
    cfg, store, r_vocab, var_maps, valid_index = dev_bleu_ref.synthetic_valid()
    table = dev_bleu_ref.label_ids_table(store, cfg, seed=0)
    make = lambda **kw: devset.DevEvaluator(None, store, cfg, r_vocab, var_maps, valid_index,
                                            ids_fn=dev_bleu_ref.table_ids_fn(table), device="cpu", **kw)
    V, L, S = cfg.vocab_size, cfg.sou_len, cfg.sub_token_len
    classes = R.merging_table(V, seed=1, n_classes=5)
    plain, both, with_cls = make(rouge_l=True), make(rouge_l=True, meteor_exact=True), make(meteor_exact=True, meteor_classes=classes)
    total, lines = plain.host_pass()
    for ev, table_ in ((both, None), (with_cls, classes)):
        total_m, lines_m = ev.host_pass()
        assert total_m == total and lines_m() == lines() and ev.last_scores == plain.last_scores
        rows = [R.dev_stats_ref(table[i], store.sou[i], store.sub_token[i], store.tar[i], V, L, S, table_, r_vocab)
                for i in range(len(store))]
        want = [metrics.meteor_exact_from_stats(*row) for row in rows]
        assert ev.last_meteor_exact == want and len(want) == 23 and sum(v > 0 for v in want) >= 12
    assert both.last_rouge_l == plain.last_rouge_l and with_cls.last_rouge_l == [] and plain.last_meteor_exact == []
    assert with_cls.last_meteor_exact != both.last_meteor_exact
    for kw in (dict(meteor_classes=classes), dict(meteor_exact=True, meteor_classes=classes[:-1]),
               dict(meteor_exact=True, meteor_classes=classes.astype(np.float32)),
               dict(meteor_exact=True, meteor_classes=classes.astype(np.int64) + (1 << 40))):
        with pytest.raises(ValueError, match="meteor_classes"):
            make(**kw)


def test_entries_are_declared_exported_and_bound(lib):
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("fira_mbr_meteor_stats", 9), ("fira_dev_meteor_stats", 12)):
        proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert proto and len(proto.group(1).split(",")) == n_args, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
        assert hasattr(lib, name)
    assert lib.fira_abi_version() == int(re.search(r"#define FIRA_ABI_VERSION (\d+)", header).group(1)) == 11
