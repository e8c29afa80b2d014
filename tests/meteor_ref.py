"""Oracle and inputs shared by tests/test_meteor.py (CPU) and tests/test_meteor_gpu.py.

* ``align_ref``: NLTK's ``_match_enums`` stated literally -- two nested loops from the last position to the first over the
  positions still unmatched, pop both and break on the first equal key -- once per stage, and ``_count_chunks`` as a walk over
  the matches sorted by hypothesis position.  Deliberately NOT the ranked form of ``metrics.meteor_alignment`` nor the
  walk-one-side form of csrc/meteor.hip, so that the three check each other.
* ``stats_ref_all``: what ``fira_mbr_meteor_stats`` must write (m, chunks, hyp_len, ref_len); the message of a candidate is
  ``mbr_ref.words``.  ``dev_stats_ref``: what ``fira_dev_meteor_stats`` must write for one commit, on the word STRINGS
  ``dev_bleu_ref.strings_ref`` builds (so a hypothesis <unkm>, written as the emoji, matches nothing and has no class).
* ``pair_cases`` / ``dev_rows``: the seeded inputs of the two kernels with the hand-made rows the issue names.
"""
import numpy as np

import dev_bleu_ref
from mbr_ref import pick_ref, words                                # noqa: F401  (one rule for the message, re-exported)
from fira_icse_amd.config import EOS, PAD, START, UNK

BIG = (1 << 30) + 12345               # ids that are ordinary words without a class
NEG = -7


def table_key(classes):
    """word -> class (None: no class) for an integer table indexed by the word, or None."""
    if classes is None:
        return None
    return lambda w: int(classes[w]) if isinstance(w, (int, np.integer)) and 0 <= w < len(classes) else None


def align_ref(hyp, ref, key=None):
    """(m, chunks) of hypothesis and reference word lists; ``key``: word -> class or None for stage 2 (None: no stage 2)."""
    h, r = list(enumerate(hyp)), list(enumerate(ref))
    matches = []

    def stage(kh, kr):                                               # keys of the positions still in h / r, in step with them
        for i in range(len(h))[::-1]:
            for j in range(len(r))[::-1]:
                if kh[i] is not None and kh[i] == kr[j]:
                    matches.append((h[i][0], r[j][0]))
                    h.pop(i), kh.pop(i), r.pop(j), kr.pop(j)
                    break

    stage([("word", w) for _, w in h], [("word", w) for _, w in r])
    if key is not None:
        stage([key(w) for _, w in h], [key(w) for _, w in r])
    matches.sort()
    if not matches:
        return 0, 0
    chunks = 1
    for k in range(len(matches) - 1):
        if not (matches[k + 1][0] == matches[k][0] + 1 and matches[k + 1][1] == matches[k][1] + 1):
            chunks += 1
    return len(matches), chunks


def stats_ref_all(tokens, length, classes=None):
    """[B, n, n, 4] int32: (m, chunks, hyp_len, ref_len) of every ordered pair (hypothesis i, reference j) of every commit."""
    B, n, _ = tokens.shape
    key = table_key(classes)
    out = np.zeros((B, n, n, 4), dtype=np.int32)
    for b in range(B):
        ws = [words(tokens[b, i], length[b, i]) for i in range(n)]
        for i in range(n):
            for j in range(n):
                out[b, i, j] = list(align_ref(ws[i], ws[j], key)) + [len(ws[i]), len(ws[j])]
    return out


def dev_stats_ref(ids, sou, sub, tar, V, L, S, classes=None, r_vocab=None):
    """The stats row (m, chunks, hyp_len, ref_len) of one commit of the dev pass."""
    r_vocab = r_vocab or dev_bleu_ref.toy_r_vocab(V)
    hyp, ref = dev_bleu_ref.strings_ref(ids, sou, sub, tar, V, L, S, r_vocab)
    key = None
    if classes is not None:
        word_class = {r_vocab[i]: int(c) for i, c in enumerate(classes)}
        key = word_class.get
    return list(align_ref(hyp, ref, key)) + [len(hyp), len(ref)]


def merging_table(V, seed=0, n_classes=None):
    """A class table over [0, V) that merges words: V / 3 classes unless told, arbitrary int32 values (negative ones included)."""
    rng = np.random.default_rng(seed)
    names = rng.integers(-(1 << 31), 1 << 31, size=n_classes or max(1, V // 3), dtype=np.int64)
    return np.ascontiguousarray(names[rng.integers(0, len(names), size=V)], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ all-pairs inputs
PAIR_V = 12                           # vocabulary of the class table of the all-pairs cases
# (B, n, T): n covers one candidate, odd and even round-robin, the distance n / 2 pair, and the limit
PAIR_SHAPES = [(3, 1, 30), (3, 2, 30), (3, 3, 64), (3, 8, 64), (3, 31, 30), (3, 32, 30)]


def _message(ws, T, eos=True):
    ids = ([START] + [int(w) for w in ws] + ([EOS] if eos else []))[:T]
    return ids, len(ids)


def hand_made(T):
    """The edge-case candidates of commit 0, (ids, length) each; used where T == 64 and n >= 8."""
    return [
        _message([7] * 63, T, eos=False),                             # one word in every position a message has ...
        _message([4, 7, 5, 7, 6, 7], T),                              # ... against 3 occurrences of it
        _message([], T),                                              # empty
        _message([9, 4, 5, 6, 9, 7, 8, 9], T),                    # counts 3 against 2: the LAST two occurrences pair
        _message([5, 9, 4, 9, 6], T),
        _message([NEG, BIG, 5, NEG, 10], T),                          # words outside [0, V): matched by id, never by class
        _message([BIG, NEG, 11, BIG + 1, 4], T),
        _message([5, PAD, 6, START, EOS, 8, 5], T),                   # <pad> / <start> / <eos> inside: dropped where they stand
    ]


def pair_cases(B, n, T, seed):
    """(tokens [B, n, T], length [B, n]) int32 over a 6-word alphabet (ids 4..9), so that repeats are frequent; lengths of
    0 .. T - 1 words, a random non-zero id at every position at or past ``length``."""
    rng = np.random.default_rng(2000 + seed)
    tokens = np.zeros((B, n, T), dtype=np.int64)
    length = np.zeros((B, n), dtype=np.int64)
    for b in range(B):
        base = rng.integers(4, 10, size=int(rng.integers(0, T)))
        for i in range(n):
            if rng.random() < 0.5:                                    # near the commit's message: dropped, replaced, moved
                ws = [int(w) if rng.random() < 0.85 else int(rng.integers(4, 12)) for w in base if rng.random() < 0.9]
                if len(ws) > 3 and rng.random() < 0.5:
                    cut = int(rng.integers(1, len(ws)))
                    ws = ws[cut:] + ws[:cut]
            else:
                ws = [int(w) for w in rng.integers(4, 10, size=int(rng.integers(0, T)))]
            ids, ln = _message(ws, T, eos=rng.random() < 0.8)
            tokens[b, i, :ln], length[b, i] = ids, ln
            if ln == T and rng.random() < 0.4:
                length[b, i] = T + 1 + int(rng.integers(0, 5))        # a length past the row counts as T
    if T == 64 and n >= 8:
        for i, (ids, ln) in enumerate(hand_made(T)):
            tokens[0, i], length[0, i] = 0, ln
            tokens[0, i, :ln] = ids
    pos = np.arange(T)[None, None, :]
    tokens = np.where(pos >= length[:, :, None], rng.integers(1, 50, size=(B, n, T)), tokens)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return i32(tokens), i32(length)


def all_pair_cases():
    return [pair_cases(B, n, T, seed) for seed, (B, n, T) in enumerate(PAIR_SHAPES)]


# ------------------------------------------------------------------------------------------------ dev-pass inputs
DEV_B = 13                            # rows of a dev case set: 3 workgroups of 4 commits and one more


def dev_rows(T, V, L, S, seed):
    """(ids [13, T] in [0, V + L + S), sou [13, L], sub [13, S], tar [13, T]) int32: the hand-made rows first (each cut or
    padded to T), seeded rows near their reference behind them.  What the hand-made rows are is asserted by the test from the
    oracle's output, not taken from here."""
    rng = np.random.default_rng(3000 + seed)
    B = DEV_B
    sou = rng.integers(4, V, size=(B, L))
    sub = rng.integers(4, V, size=(B, S))
    ids = np.zeros((B, T), dtype=np.int64)
    tar = np.zeros((B, T), dtype=np.int64)
    fit = lambda row: (list(row) + [PAD] * T)[:T]
    sou[4, :3], sub[4, :2] = [6, 7, UNK], [8, 5]
    hand = [
        ([4 + (i % 7) for i in range(T)], [START] + [4 + ((3 * i) % 7) for i in range(T - 1)]),      # all T positions are words
        ([EOS, 5, 6], [START, 5, 6, EOS]),                                                           # empty hypothesis
        ([5, 6, EOS], [START, EOS]),                                                                 # empty reference
        ([7] * T, [START, 4, 7, 5, 7, 6, 7, EOS]),                                                   # T x one word against 3
        ([V, 5, V + 1, V + L, V + L + 1, V + 2, EOS], [START, 6, 5, 7, 8, 5, UNK, EOS]),             # copies; one resolves to <unkm>
        ([UNK, 5, UNK, 6, EOS], [START, UNK, 5, UNK, 6, EOS]),                                       # <unkm> on both sides
        ([9, 4, 5, 6, 9, 7, 8, 9, EOS], [START, 5, 9, 4, 9, 6, EOS]),                                # counts 3 against 2
        ([5, PAD, 6, 7, EOS], [START, 7, 6, 5, EOS]),                                                # all matched, all out of order
    ]
    for b in range(B):
        if b < len(hand):
            ids[b], tar[b] = fit(hand[b][0]), fit(hand[b][1])
            continue
        n_ref = int(rng.integers(0, max(T - 1, 1)))
        ref = rng.integers(3, V, size=n_ref)                          # (3 = <unkm> included)
        tar[b] = fit([START] + list(ref) + [EOS])
        out = []
        for w in ref:
            r = rng.random()
            hit_l, hit_s = np.nonzero(sou[b] == w)[0], np.nonzero(sub[b] == w)[0]
            if r < 0.1:
                continue                                              # dropped
            if r < 0.3:
                w = rng.integers(3, V)                                # replaced
            elif r < 0.45 and hit_l.size:
                w = V + hit_l[0]                                      # copied from the source
            elif r < 0.6 and hit_s.size:
                w = V + L + hit_s[0]
            out.append(int(w))
        if len(out) > 3 and rng.random() < 0.5:
            cut = int(rng.integers(1, len(out)))
            out = out[cut:] + out[:cut]
        out = (out + [EOS])[:T]
        ids[b, :len(out)] = out
        ids[b, len(out):] = rng.integers(0, V + L + S, size=T - len(out))         # what a model writes behind <eos>: anything
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return i32(ids), i32(sou), i32(sub), i32(tar)
