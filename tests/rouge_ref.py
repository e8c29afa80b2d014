"""Oracle and inputs shared by tests/test_rouge.py (CPU) and tests/test_rouge_gpu.py.

* ``lcs_dp``: the textbook (m + 1) x (n + 1) table -- nothing of the kernel's bit-vector recurrence, nor of the one-row form in
  ``metrics.lcs_length``.
* ``stats_ref`` / ``stats_ref_all``: what ``fira_mbr_rouge_l_stats`` must write (lcs, hyp_len, ref_len, 0); the message of a
  candidate is ``mbr_ref.words``.  ``dev_stats_ref``: what ``fira_dev_rouge_l_stats`` must write for one commit, on the word
  STRINGS ``dev_bleu_ref.strings_ref`` builds (so a hypothesis <unkm>, written as the emoji, matches nothing).
* ``utilities_ref``: expected ROUGE-L through ``metrics.rouge_l`` on word strings.
* ``cases`` / ``all_cases``: seeded candidate sets, one per shape, with the hand-made candidates in commit 0 where the shape has
  room; ``coverage`` says from the data alone which properties a list of case sets holds, ``check_cases`` asserts them all.
"""
import math

import numpy as np

import dev_bleu_ref
import mbr_ref
from mbr_ref import as_text, pick_ref, regarbage, words            # noqa: F401  (one rule for the message, re-exported)
from fira_icse_amd import metrics
from fira_icse_amd.config import EOS, PAD, START

# (B, n, T); the seed is the position
SHAPES = [
    (1, 1, 30),       # one candidate
    (3, 2, 30),
    (5, 5, 30),       # n not a multiple of any wave count, B not of any commits-per-workgroup
    (2, 32, 64),      # the limits
    (1, 8, 1),        # nothing but <start>
    (2, 3, 2),        # one word
    (4, 8, 64),
]
ALPHABETS = (1, 2, 3, 40)             # words a commit's candidates draw from
BIG = (1 << 30) + 12345               # ids that are ordinary words
NEG = -7


def lcs_dp(a, b):
    table = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            table[i][j] = table[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(table[i - 1][j], table[i][j - 1])
    return table[len(a)][len(b)]


def stats_ref(tokens_row_i, len_i, tokens_row_j, len_j):
    hyp, ref = words(tokens_row_i, len_i), words(tokens_row_j, len_j)
    return [lcs_dp(hyp, ref), len(hyp), len(ref), 0]


def stats_ref_all(tokens, length):
    """[B, n, n, 4] int32: ``stats_ref`` of every ordered pair of every commit."""
    B, n, _ = tokens.shape
    out = np.zeros((B, n, n, 4), dtype=np.int32)
    for b in range(B):
        ws = [words(tokens[b, i], length[b, i]) for i in range(n)]
        for i in range(n):
            for j in range(n):
                out[b, i, j] = [lcs_dp(ws[i], ws[j]), len(ws[i]), len(ws[j]), 0]
    return out


def utilities_ref(tokens, length):
    """u[b][i]: the mean over j != i of ``metrics.rouge_l(words_j, words_i)`` on word STRINGS (0.0 for n == 1)."""
    B, n, _ = tokens.shape
    out = []
    for b in range(B):
        ws = [as_text(words(tokens[b, i], length[b, i])) for i in range(n)]
        out.append([math.fsum(metrics.rouge_l(ws[j], ws[i]) for j in range(n) if j != i) / (n - 1) if n > 1 else 0.0
                    for i in range(n)])
    return out


def dev_stats_ref(ids, sou, sub, tar, V, L, S, r_vocab=None):
    """The stats row (lcs, hyp_len, ref_len, 0) of one commit of the dev pass."""
    hyp, ref = dev_bleu_ref.strings_ref(ids, sou, sub, tar, V, L, S, r_vocab)
    return [lcs_dp(hyp, ref), len(hyp), len(ref), 0]


# ------------------------------------------------------------------------------------------------ inputs
def _message(ws, T, eos=True):
    ids = ([START] + [int(w) for w in ws] + ([EOS] if eos else []))[:T]
    return ids, len(ids)


def hand_made(T):
    """The edge-case candidates of commit 0, (ids, length) each; used where T == 64 and n >= 8."""
    far = [20 + i for i in range(62)] + [9]                           # word 9 at hypothesis position 62 ...
    near = [9] + [100 + i for i in range(40)]                         # ... and at reference position 0: their only match
    return [
        _message([7] * 63, T, eos=False),                             # 63 x one word: the carry runs through every bit
        _message([7] * 63, T, eos=False),                             # ... against itself
        _message(far, T, eos=False),
        _message(near, T),
        _message([5, PAD, 6, START, EOS, 8, 5], T),                   # <pad> / <start> / <eos> inside: dropped where they stand
        _message([NEG, BIG, 5, NEG, BIG + 1], T),                     # negative and > 2^30 ids are words
        _message([BIG, NEG, 6, BIG + 1], T),
        _message([5, 6], T),                                          # two words
    ]


def cases(B, n, T, seed):
    """(tokens [B, n, T], length [B, n]) int32; every position at or past ``length`` holds a random non-zero id.  Commit b
    draws from an alphabet of ALPHABETS[(b + seed) % 4] words, so that LCS and bag overlap differ."""
    rng = np.random.default_rng(1000 + seed)
    tokens = np.zeros((B, n, T), dtype=np.int64)
    length = np.zeros((B, n), dtype=np.int64)
    for b in range(B):
        alpha = ALPHABETS[(b + seed) % len(ALPHABETS)]
        draw = lambda k: [int(w) for w in rng.integers(4, 4 + alpha, size=k)]
        base = draw(int(rng.integers(0, T)))
        for i in range(n):
            r = rng.random()
            if r < 0.5:                                               # near the commit's message: words dropped and replaced
                ws = [w if rng.random() < 0.85 else draw(1)[0] for w in base if rng.random() < 0.9]
            elif r < 0.6 and i > 0:
                tokens[b, i], length[b, i] = tokens[b, i - 1], length[b, i - 1]
                continue
            else:
                ws = draw(int(rng.integers(0, T)))
            ws = [int(rng.choice([PAD, START, EOS])) if rng.random() < 0.03 else w for w in ws]
            ids, ln = _message(ws, T, eos=rng.random() < 0.8)
            tokens[b, i, :ln], length[b, i] = ids, ln
            if ln == T and rng.random() < 0.4:
                length[b, i] = T + 1 + int(rng.integers(0, 5))        # a length past the row counts as T
    if T == 64 and n >= 8:
        for i, (ids, ln) in enumerate(hand_made(T)):
            tokens[0, i], length[0, i] = 0, ln
            tokens[0, i, :ln] = ids
        if n >= 12:                                                   # the short lengths next to the long ones
            for i, k in ((8, 0), (9, 1), (10, 2), (11, 63)):
                ids, ln = _message([7] * k, T, eos=False)
                tokens[0, i], length[0, i] = 0, ln
                tokens[0, i, :ln] = ids
            length[0, 11] = T + 3
    pos = np.arange(T)[None, None, :]
    garbage = rng.integers(1, 50, size=(B, n, T))
    tokens = np.where(pos >= length[:, :, None], garbage, tokens)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return i32(tokens), i32(length)


def all_cases():
    return [cases(B, n, T, seed) for seed, (B, n, T) in enumerate(SHAPES)]


def coverage(case_list):
    """Which properties the candidates and pairs of a list of (tokens, length) hold (name -> bool), from the data alone."""
    names = ["len_0", "len_1", "len_2", "len_63", "length_past_T", "alphabet_1", "alphabet_2", "alphabet_3", "alphabet_large",
             "lcs_below_bag_overlap", "one_word_63_times_twice", "only_match_at_62_and_0", "inner_pad", "inner_eos",
             "inner_start", "negative_word", "word_above_2_30", "garbage_behind_every_length", "hyp_longer", "hyp_shorter",
             "no_common_word"]
    hit = {k: 0 for k in names}
    for tokens, length in case_list:
        B, n, T = tokens.shape
        pos = np.arange(T)[None, None, :]
        hit["garbage_behind_every_length"] += bool((tokens[pos >= length[:, :, None]] != 0).all())
        for b in range(B):
            rows = [[int(t) for t in tokens[b, i]] for i in range(n)]
            lens = [int(l) for l in length[b]]
            ws = [words(rows[i], lens[i]) for i in range(n)]
            used = set(w for x in ws for w in x)
            hit["alphabet_1"] += len(used) == 1 and n > 1
            hit["alphabet_2"] += len(used) == 2 and n > 1
            hit["alphabet_3"] += len(used) == 3 and n > 1
            hit["alphabet_large"] += len(used) >= 30
            for i in range(n):
                inside = rows[i][1:min(lens[i], T)]
                for k in (0, 1, 2, 63):
                    hit["len_%d" % k] += len(ws[i]) == k
                hit["length_past_T"] += lens[i] > T
                hit["inner_pad"] += PAD in inside[:-1] and len(ws[i]) > 0
                hit["inner_eos"] += EOS in inside[:-1] and len(ws[i]) > 0
                hit["inner_start"] += START in inside[:-1] and len(ws[i]) > 0
                hit["negative_word"] += any(w < 0 for w in ws[i])
                hit["word_above_2_30"] += any(w > 1 << 30 for w in ws[i])
                for j in range(n):
                    if i == j:
                        continue
                    common = set(ws[i]) & set(ws[j])
                    hit["one_word_63_times_twice"] += len(ws[i]) == len(ws[j]) == 63 and len(set(ws[i])) == 1 and ws[i] == ws[j]
                    hit["only_match_at_62_and_0"] += (len(ws[i]) > 62 and len(common) == 1 and ws[i][62] == ws[j][0]
                                                      and ws[i].count(ws[j][0]) == 1 and ws[j].count(ws[j][0]) == 1)
                    hit["hyp_longer"] += len(ws[i]) > len(ws[j]) > 0
                    hit["hyp_shorter"] += 0 < len(ws[i]) < len(ws[j])
                    hit["no_common_word"] += len(ws[i]) > 0 and len(ws[j]) > 0 and not common
                    if common and not hit["lcs_below_bag_overlap"]:
                        bag = sum(min(ws[i].count(w), ws[j].count(w)) for w in common)
                        hit["lcs_below_bag_overlap"] += lcs_dp(ws[i], ws[j]) < bag
    hit["garbage_behind_every_length"] = hit["garbage_behind_every_length"] == len(case_list)
    return {k: bool(v) for k, v in hit.items()}


def check_cases(case_list):
    """Asserts that the case sets have the shapes of SHAPES and hold every property ``coverage`` knows, a message of 64 - 1
    words with a length of 64 included (T = 64 leaves 63 positions behind <start>: 63 words is the longest message)."""
    assert [c[0].shape for c in case_list] == SHAPES
    cov = coverage(case_list)
    assert all(cov.values()), {k: v for k, v in cov.items() if not v}
    assert any(int(l) == 64 for _, length in case_list for l in length.reshape(-1))
    return cov
