"""Oracle and inputs shared by tests/test_mbr.py (CPU) and tests/test_mbr_gpu.py.

* ``words`` / ``stats_ref``: the message of a candidate and what ``fira_mbr_bleu_stats`` must write for one ordered pair, with
  plain ``Counter``s on word lists -- nothing of the kernel's equality-mask formulation.
* ``cases``: seeded candidate sets over a 12-word vocabulary (so that n-grams repeat), garbage behind every length, the
  hand-made edge cases in commit 0 where the shape has room for them.
* ``coverage``: which of the edge cases a list of case sets hits, from the data alone.
* ``utilities_ref`` / ``pick_ref``: expected-BLEU utilities and the pick through the STRING scorer.
"""
import math
from collections import Counter

import numpy as np

from fira_icse_amd import metrics
from fira_icse_amd.config import EOS, PAD, START, UNK

V = 12
SHAPES = [(5, 8, 30), (3, 1, 30), (1, 2, 30), (2, 32, 30), (3, 5, 64), (7, 3, 1)]      # (B, n, T); the seed is the position
DROPPED = (PAD, EOS, START)


def words(row, length):
    """The message of a candidate: ids at positions 1 .. min(length, T) - 1 without <pad> / <eos> / <start>."""
    row = [int(t) for t in row]
    return [t for t in row[1:max(min(int(length), len(row)), 0)] if t not in DROPPED]


def stats_ref(tokens_row_i, len_i, tokens_row_j, len_j):
    """The stats row of the pair (hypothesis i, reference j): num[4], cnt[4], hyp_len, ref_len, 0, 0."""
    hyp, ref = words(tokens_row_i, len_i), words(tokens_row_j, len_j)
    num, cnt = [], []
    for n in range(1, 5):
        hc = Counter(tuple(hyp[i:i + n]) for i in range(len(hyp) - n + 1))
        rc = Counter(tuple(ref[i:i + n]) for i in range(len(ref) - n + 1))
        num.append(sum(min(c, rc[g]) for g, c in hc.items()))
        cnt.append(sum(hc.values()))
    return num + cnt + [len(hyp), len(ref), 0, 0]


def stats_ref_all(tokens, length):
    """[B, n, n, 12] int32: ``stats_ref`` of every ordered pair of every commit."""
    B, n, _ = tokens.shape
    out = np.zeros((B, n, n, 12), dtype=np.int32)
    for b in range(B):
        for i in range(n):
            for j in range(n):
                out[b, i, j] = stats_ref(tokens[b, i], length[b, i], tokens[b, j], length[b, j])
    return out


def as_text(ws):
    return ["w%d" % t for t in ws]


def utilities_ref(tokens, length):
    """u[b][i]: the mean over j != i of ``sentence_bleu_method2([words_j], words_i)`` on word STRINGS (0.0 for n == 1)."""
    B, n, _ = tokens.shape
    out = []
    for b in range(B):
        ws = [as_text(words(tokens[b, i], length[b, i])) for i in range(n)]
        out.append([math.fsum(metrics.sentence_bleu_method2([ws[j]], ws[i]) for j in range(n) if j != i) / (n - 1)
                    if n > 1 else 0.0 for i in range(n)])
    return out


def pick_ref(utilities, logp=None):
    """The arg-max per commit, ties to the larger logp, then to the lower index -- written as a scan, not as a key."""
    out = []
    for b, row in enumerate(utilities):
        best = 0
        for i in range(1, len(row)):
            if row[i] > row[best] or (row[i] == row[best] and logp is not None and logp[b][i] > logp[b][best]):
                best = i
        out.append(best)
    return out


def _message(ws, T, eos=True):
    """<start> + words (+ <eos>) cut to T positions; its length."""
    ids = ([START] + [int(w) for w in ws] + ([EOS] if eos else []))[:T]
    return ids, len(ids)


def hand_made(T):
    """The edge-case candidates of commit 0: (ids, length) each.  Words 8..11 and words 3..7 never meet."""
    full = [8 + (i % 4) for i in range(T - 1)]                       # every position used, no <eos>
    return [
        ([START], 1),                                                # empty: length 1
        ([START, EOS], 2),                                           # empty: <start> <eos>
        _message(full, T, eos=False),
        _message([5, PAD, 6, UNK], T),                               # inner id 0; three words
        _message([5, START, 6, UNK, 7], T),                          # inner id 2
        _message([5, START, 6, UNK, 7], T),                          # the same candidate again
        _message([7, 7, 7, 5], T),                                   # clipping against the next one (7 three times / once)
        _message([7, 5, 9, 10, 11, 4], T),
    ]


def cases(B, n, T, seed):
    """(tokens [B, n, T], length [B, n]) int32.  Every position at or past ``length`` holds a random non-zero id."""
    rng = np.random.default_rng(seed)
    tokens = np.zeros((B, n, T), dtype=np.int64)
    length = np.zeros((B, n), dtype=np.int64)
    for b in range(B):
        base = rng.integers(3, V, size=int(rng.integers(0, T)))      # the commit's "true" message: candidates stay near it
        for i in range(n):
            r = rng.random()
            if r < 0.6:
                ws = [w if rng.random() < 0.8 else int(rng.integers(3, V)) for w in base][:int(rng.integers(0, T))]
            elif r < 0.7 and i > 0:
                ws = None                                            # a copy of the candidate before it
            else:
                ws = list(rng.integers(3, V, size=int(rng.integers(0, T))))
            if ws is None:
                tokens[b, i], length[b, i] = tokens[b, i - 1], length[b, i - 1]
                continue
            ws = [int(rng.choice([PAD, START])) if rng.random() < 0.03 else w for w in ws]     # a special id drawn mid-message
            ids, ln = _message(ws, T, eos=rng.random() < 0.9)
            tokens[b, i, :ln], length[b, i] = ids, ln
            if ln == T and rng.random() < 0.3:
                length[b, i] = T + 1                                 # a length past the row counts as T
    if T >= 8:
        for i, (ids, ln) in enumerate(hand_made(T)[:n]):
            tokens[0, i], length[0, i] = 0, ln
            tokens[0, i, :ln] = ids
    pos = np.arange(T)[None, None, :]
    garbage = rng.integers(1, V, size=(B, n, T))
    tokens = np.where(pos >= length[:, :, None], garbage, tokens)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return i32(tokens), i32(length)


def regarbage(tokens, length, seed):
    """The same candidates with other random non-zero ids at every position at or past ``length``."""
    rng = np.random.default_rng(seed)
    pos = np.arange(tokens.shape[2])[None, None, :]
    out = np.where(pos >= length[:, :, None], rng.integers(1, V + 40, size=tokens.shape), tokens)
    return np.ascontiguousarray(out, dtype=np.int32)


def all_cases():
    return [cases(B, n, T, seed) for seed, (B, n, T) in enumerate(SHAPES)]


def coverage(case_list):
    """Which edge cases the candidates and pairs of a list of (tokens, length) hit (name -> bool), from the data alone."""
    hit = Counter({k: 0 for k in (
        "empty_from_length_1", "empty_from_start_eos", "fills_all_positions_without_eos", "inner_pad", "inner_start",
        "identical_candidates", "hyp_shorter_than_4", "clipping_active", "no_common_unigram", "hyp_longer", "hyp_shorter",
        "equal_lengths", "unk_on_both_sides", "garbage_behind_every_length")})
    for tokens, length in case_list:
        B, n, T = tokens.shape
        pos = np.arange(T)[None, None, :]
        hit["garbage_behind_every_length"] += bool((tokens[pos >= length[:, :, None]] != 0).all())
        for b in range(B):
            rows = [[int(t) for t in tokens[b, i]] for i in range(n)]
            lens = [int(l) for l in length[b]]
            ws = [words(rows[i], lens[i]) for i in range(n)]
            for i in range(n):
                inside = rows[i][1:min(lens[i], T)]
                hit["empty_from_length_1"] += lens[i] == 1
                hit["empty_from_start_eos"] += lens[i] == 2 and rows[i][:2] == [START, EOS]
                hit["fills_all_positions_without_eos"] += T > 1 and lens[i] >= T and EOS not in rows[i] and len(ws[i]) == T - 1
                hit["inner_pad"] += PAD in inside[:-1] and len(ws[i]) > 0
                hit["inner_start"] += START in inside[:-1] and len(ws[i]) > 0
                hit["hyp_shorter_than_4"] += 1 <= len(ws[i]) < 4 and n > 1
                for j in range(n):
                    if i == j:
                        continue
                    hc, rc = Counter(ws[i]), Counter(ws[j])
                    hit["identical_candidates"] += len(ws[i]) > 0 and rows[i][:lens[i]] == rows[j][:lens[j]]
                    hit["clipping_active"] += any(0 < rc[g] < c for g, c in hc.items())
                    hit["no_common_unigram"] += len(ws[i]) > 0 and len(ws[j]) > 0 and not (set(ws[i]) & set(ws[j]))
                    hit["hyp_longer"] += len(ws[i]) > len(ws[j]) > 0
                    hit["hyp_shorter"] += 0 < len(ws[i]) < len(ws[j])
                    hit["equal_lengths"] += len(ws[i]) == len(ws[j]) > 0 and ws[i] != ws[j]
                    hit["unk_on_both_sides"] += UNK in ws[i] and UNK in ws[j]
    hit["garbage_behind_every_length"] = hit["garbage_behind_every_length"] == len(case_list)
    return {k: bool(v) for k, v in hit.items()}
