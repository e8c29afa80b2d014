"""Text scorers of the reference's evaluation protocol, re-implemented without nltk / sumeval.

* ``bnorm_bleu`` / ``penalty_bleu``: the corpus scores the paper reports (reference Metrics/Bleu-B-Norm.py:26-129,
  171-185 and Metrics/Bleu-Penalty.py:160-186): NIST-mteval style tokenisation, per-sentence BLEU-4 with add-one
  smoothing on the 2..4-gram precisions, brevity penalty ``min(0, 1 - (r+1)/(c+1))`` in log space; B-Norm is the plain
  mean x 100, Penalty-BLEU the reference-length-weighted mean.  On the reference's shipped ``OUTPUT/`` files they give
  17.666 / 0.13299 (checked in tests/test_metrics.py when the reference tree is present).
* ``sentence_bleu_method2``: what ``dev()`` uses for checkpoint selection (reference run_model.py:22,171):
  NLTK ``sentence_bleu`` with ``SmoothingFunction().method2``.
* ``rouge_l`` / ``rouge_l_corpus``: sentence-level ROUGE-L as Lin (2004) defines it -- the F-measure (beta = 1) of the longest
  common subsequence of two word lists.  The reference computes its ROUGE column by calling the ``sumeval`` command-line tool
  (Metrics/Rouge.py); that tool is not available here, so identity with ``sumeval r-nl`` has NOT been checked (its tokenisation
  and stop-word handling may differ) and no claim against the paper's 21.58 is made.
* ``meteor_exact`` / ``meteor_exact_corpus``: the alignment and the score of NLTK's ``meteor_score`` (alpha = 0.9, beta = 3,
  gamma = 0.5), which the reference calls (Metrics/Meteor.py), WITHOUT its Porter-stem and WordNet-synonym stages: words match
  when they are equal, and then, only if the caller supplies ``classes``, when they have the same class.  The project ships no
  stemmer and no synonym table.  No figure is comparable with the paper's METEOR column, and identity with NLTK has NOT been
  checked (NLTK is absent).
"""
from __future__ import annotations

import math
import re
import sys
from collections import Counter
from typing import Iterable, List, Sequence
from xml.sax.saxutils import unescape

_TINY = sys.float_info.min
_SPLIT = re.compile(r"\w+|[^\s\w]")
# punctuation that is always set off by spaces: every ASCII punctuation mark (and the blank) except ' , - .
_ALWAYS = re.compile("([" + re.escape("{|}~[\\]^_` !\"#$%&()*+:;<=>?@/") + "])")
_AFTER_NONDIGIT = re.compile(r"([^0-9])([.,])")
_BEFORE_NONDIGIT = re.compile(r"([.,])([^0-9])")
_DIGIT_DASH = re.compile(r"([0-9])(-)")


def split_punct(line: str) -> str:
    return " ".join(_SPLIT.findall(line))


def mteval_tokens(s: str) -> List[str]:
    s = s.replace("<skipped>", "").replace("-\n", "").replace("\n", " ")
    s = unescape(s, {"&quot;": '"'})
    s = (" %s " % s).lower()
    s = _ALWAYS.sub(r" \1 ", s)
    s = _AFTER_NONDIGIT.sub(r"\1 \2 ", s)
    s = _BEFORE_NONDIGIT.sub(r" \1 \2", s)
    s = _DIGIT_DASH.sub(r"\1 \2 ", s)
    return s.split()


def _ngrams(words: Sequence[str], n: int = 4) -> Counter:
    c = Counter()
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            c[tuple(words[i:i + k])] += 1
    return c


def smoothed_sentence_bleu(refs: Sequence[str], hyp: str, n: int = 4):
    """(BLEU in [0,1], effective reference length) of one segment; refs/hyp are raw strings."""
    ref_tok = [mteval_tokens(r) for r in refs]
    hyp_tok = mteval_tokens(hyp)
    max_ref = Counter()
    for r in ref_tok:
        for g, c in _ngrams(r, n).items():
            max_ref[g] = max(max_ref[g], c)
    ref_len = min(len(r) for r in ref_tok)
    guess = [max(len(hyp_tok) - k + 1, 0) for k in range(1, n + 1)]
    correct = [0] * n
    for g, c in _ngrams(hyp_tok, n).items():
        correct[len(g) - 1] += min(max_ref.get(g, 0), c)
    log_b = 0.0
    for k in range(n):
        add = 1 if k > 0 else 0
        log_b += math.log(correct[k] + add + _TINY) - math.log(guess[k] + add + _TINY)
    log_b /= n
    log_b += min(0.0, 1.0 - float(ref_len + 1) / (len(hyp_tok) + 1))
    return math.exp(log_b), ref_len


def _pairs(references: Iterable[str], predictions: Iterable[str]):
    """Pair lines by running index exactly as the reference scripts do: blank reference lines are dropped BEFORE
    numbering, predictions keep their line numbers, and a blank prediction is an error."""
    refs = [r.strip() for r in references if r.strip()]
    preds = list(predictions)
    for i, p in enumerate(preds):
        if not p.strip():
            raise ValueError("prediction %d is empty (the reference scorer raises here too)" % i)
    for i, r in enumerate(refs):
        if i < len(preds):
            yield split_punct(r.lower()), split_punct(preds[i].strip().lower())


def bnorm_bleu(references: Iterable[str], predictions: Iterable[str]) -> float:
    scores = [smoothed_sentence_bleu([r], p)[0] for r, p in _pairs(references, predictions)]
    return 100.0 * sum(scores) / len(scores)


def penalty_bleu(references: Iterable[str], predictions: Iterable[str]) -> float:
    res = [smoothed_sentence_bleu([r], p) for r, p in _pairs(references, predictions)]
    total = float(sum(l for _, l in res))
    return sum(l / total * s for s, l in res)


def sentence_bleu_method2(references: Sequence[Sequence[str]], hypothesis: Sequence[str]) -> float:
    """NLTK ``sentence_bleu(references, hypothesis, smoothing_function=SmoothingFunction().method2)`` on token lists:
    uniform 4-gram weights, clipped precisions with +1/+1 smoothing on orders 2..4, closest-reference-length
    brevity penalty, 0 when no unigram matches or the hypothesis is empty."""
    hyp = list(hypothesis)
    if not hyp:
        return 0.0
    nums, cnts = [], []
    for n in range(1, 5):
        counts = Counter(tuple(hyp[i:i + n]) for i in range(len(hyp) - n + 1))
        max_ref = Counter()
        for ref in references:
            rc = Counter(tuple(ref[i:i + n]) for i in range(len(ref) - n + 1))
            for g in counts:
                max_ref[g] = max(max_ref[g], rc[g])
        nums.append(sum(min(c, max_ref[g]) for g, c in counts.items()))
        cnts.append(sum(counts.values()))
    if nums[0] == 0:
        return 0.0
    hyp_len = len(hyp)
    ref_len = min((abs(len(r) - hyp_len), len(r)) for r in references)[1]
    return bleu_method2_from_stats(nums, cnts, hyp_len, ref_len)


def bleu_method2_from_stats(num: Sequence[int], cnt: Sequence[int], hyp_len: int, ref_len: int) -> float:
    """``sentence_bleu_method2`` from its integer statistics (Python ints): for n = 1..4 ``cnt[n-1]`` hypothesis n-grams, of
    which ``num[n-1]`` are matched after clipping; the hypothesis and the (closest) reference length.  These are the twelve
    numbers ``fira_dev_bleu_stats`` writes per commit, and the expressions -- ``max(1, cnt)``, ``math.log``, ``math.fsum``,
    ``math.exp``, in this order -- are the ones the string scorer has always used, so the value is ``==`` its value."""
    if hyp_len == 0:
        return 0.0
    dens = [max(1, c) for c in cnt]
    if num[0] == 0:
        return 0.0
    bp = 1.0 if hyp_len > ref_len else math.exp(1 - ref_len / hyp_len)
    logs = [math.log(num[0] / dens[0])] + [math.log((num[i] + 1) / (dens[i] + 1)) for i in range(1, 4)]
    return bp * math.exp(math.fsum(0.25 * x for x in logs))


def lcs_length(a: Sequence, b: Sequence) -> int:
    """Length of the longest common subsequence of two sequences: the plain O(mn) DP, one row kept."""
    row = [0] * (len(b) + 1)
    for x in a:
        diag = 0
        for j, y in enumerate(b):
            diag, row[j + 1] = row[j + 1], (diag + 1 if x == y else max(row[j + 1], row[j]))
    return row[len(b)]


def rouge_l_from_stats(lcs: int, hyp_len: int, ref_len: int) -> float:
    """Sentence-level ROUGE-L (Lin 2004, F-measure with beta = 1) from its three integers: ``2PR / (P + R)`` with
    ``P = lcs / hyp_len`` and ``R = lcs / ref_len``, reduced to ``2 lcs / (hyp_len + ref_len)`` so that the value has one
    rounding.  0.0 when ``lcs == 0`` (which covers either side empty).  These are the numbers ``fira_dev_rouge_l_stats`` /
    ``fira_mbr_rouge_l_stats`` write.  The standard definition; identity with the reference's ``sumeval r-nl`` has NOT been
    checked (the tool is absent)."""
    if lcs == 0:
        return 0.0
    return 2.0 * lcs / (hyp_len + ref_len)


def rouge_l(reference: Sequence[str], hypothesis: Sequence[str]) -> float:
    """``rouge_l_from_stats`` of two word lists."""
    return rouge_l_from_stats(lcs_length(hypothesis, reference), len(hypothesis), len(reference))


def rouge_l_corpus(references: Iterable[str], predictions: Iterable[str]) -> float:
    """100 x the mean sentence-level ROUGE-L of the lines, both sides tokenised by ``str.split()``.  Raises ValueError when the
    two sides differ in length (or are empty).  Not checked against ``sumeval`` -- see the module docstring."""
    refs, preds = list(references), list(predictions)
    if len(refs) != len(preds):
        raise ValueError("rouge_l_corpus: %d references and %d predictions" % (len(refs), len(preds)))
    if not refs:
        raise ValueError("rouge_l_corpus: no lines")
    return 100.0 * math.fsum(rouge_l(r.split(), p.split()) for r, p in zip(refs, preds)) / len(refs)


def meteor_exact_from_stats(m: int, chunks: int, hyp_len: int, ref_len: int) -> float:
    """NLTK's METEOR score (alpha = 0.9, beta = 3, gamma = 0.5) from the four integers of an alignment: ``m`` matched word
    pairs in ``chunks`` chunks, the two lengths.  ``(1 - pen) * fmean`` with ``P = m / hyp_len``, ``R = m / ref_len``,
    ``fmean = P * R / (0.9 * P + 0.1 * R)`` and ``pen = 0.5 * (chunks / m) ** 3``, the operations written once and in this
    order on Python ints and floats; 0.0 when ``m == 0``.  These are the numbers ``fira_dev_meteor_stats`` /
    ``fira_mbr_meteor_stats`` write, so a value from the device is ``==`` the value from the words."""
    if m == 0:
        return 0.0
    p = m / hyp_len
    r = m / ref_len
    fmean = p * r / (0.9 * p + 0.1 * r)
    pen = 0.5 * (chunks / m) ** 3
    return (1 - pen) * fmean


def _class_of(classes):
    """word -> class or None (no class) for a mapping, a callable or a table indexed by integer words."""
    if hasattr(classes, "get"):
        return classes.get
    if callable(classes):
        return classes
    size = len(classes)

    def lookup(w):
        if isinstance(w, bool) or not hasattr(w, "__index__"):
            return None
        k = w.__index__()
        return classes[k] if 0 <= k < size else None
    return lookup


def meteor_alignment(reference: Sequence, hypothesis: Sequence, classes=None):
    """(m, chunks) of NLTK's METEOR alignment (``_match_enums`` and ``_count_chunks``) of two word lists, without NLTK's stem and
    WordNet stages.  Stage 1 pairs equal words.  Stage 2 runs only with ``classes`` -- a mapping (``.get``), a callable, or a
    table indexed by integer words -- and pairs the words still free that have the same class; a word whose class is None, that
    the mapping lacks or that lies outside the table has no class and matches nothing.  A caller with NLTK passes Porter stems
    or synonym sets through it; the project ships neither.

    Within a stage NLTK walks the hypothesis from its last word to its first and gives each the last free reference word of
    equal key.  Words of different keys never compete, and for one key that loop pairs the k-th last free occurrence in the
    hypothesis with the k-th last in the reference: this function pairs by that rank (DESIGN.md 6j-3 has the proof,
    tests/meteor_ref.py the literal loops).  ``chunks`` is m minus the matches (i, j) for which (i + 1, j + 1) is a match too."""
    hyp, ref = list(hypothesis), list(reference)
    partner = {}                                         # hypothesis position -> reference position
    taken = set()                                        # reference positions

    def stage(key):
        by_key = {}
        for j, w in enumerate(ref):
            if j not in taken:
                k = key(w)
                if k is not None:
                    by_key.setdefault(k, []).append(j)
        for i in range(len(hyp) - 1, -1, -1):            # the k-th last free hypothesis occurrence pops the k-th last reference one
            if i not in partner:
                k = key(hyp[i])
                js = by_key.get(k) if k is not None else None
                if js:
                    partner[i] = js.pop()
                    taken.add(partner[i])

    stage(lambda w: ("word", w))
    if classes is not None:
        stage(_class_of(classes))
    m = len(partner)
    return m, m - sum(1 for i, j in partner.items() if partner.get(i + 1) == j + 1)


def meteor_exact(reference: Sequence, hypothesis: Sequence, classes=None) -> float:
    """``meteor_exact_from_stats`` of two word lists: NLTK's alignment and score with exact matches (and the caller's
    ``classes`` as a second stage), NOT NLTK's ``meteor_score`` with its stemmer and WordNet -- not comparable with the paper's
    METEOR column, and identity with NLTK has not been checked (NLTK is absent)."""
    m, chunks = meteor_alignment(reference, hypothesis, classes)
    return meteor_exact_from_stats(m, chunks, len(hypothesis), len(reference))


def meteor_exact_corpus(references: Iterable[str], predictions: Iterable[str], classes=None) -> float:
    """100 x the mean ``meteor_exact`` of the lines, both sides tokenised by ``str.split()``.  Raises ValueError when the two
    sides differ in length (or are empty).  Not NLTK's METEOR -- see ``meteor_exact``."""
    refs, preds = list(references), list(predictions)
    if len(refs) != len(preds):
        raise ValueError("meteor_exact_corpus: %d references and %d predictions" % (len(refs), len(preds)))
    if not refs:
        raise ValueError("meteor_exact_corpus: no lines")
    return 100.0 * math.fsum(meteor_exact(r.split(), p.split(), classes) for r, p in zip(refs, preds)) / len(refs)


MBR_UTILITIES = ("bleu", "rouge_l", "meteor_exact")


def mbr_utilities(stats, utility: str = "bleu") -> List[List[float]]:
    """Expected-utility values from the all-pairs statistics of one commit's candidates: ``stats`` is [B][n][n][k] integers
    (nested lists, a numpy array or a CPU tensor), row [b][i][j] the statistics of candidate i scored against candidate j.

    ``"bleu"``: the twelve integers of ``fira_mbr_bleu_stats``; ``u[b][i]`` is the mean over j != i of
    ``bleu_method2_from_stats`` of pair (i, j) -- Python ints in, ``math.fsum`` for the mean -- so it is ``==`` the same mean of
    ``sentence_bleu_method2`` on the candidates' word lists.  ``"rouge_l"``: the four integers (lcs, hyp_len, ref_len, 0) of
    ``fira_mbr_rouge_l_stats`` and ``rouge_l_from_stats`` in the same mean, ``==`` that of ``rouge_l``.  ``"meteor_exact"``:
    the four integers (m, chunks, hyp_len, ref_len) of ``fira_mbr_meteor_stats`` and ``meteor_exact_from_stats`` in the same
    mean, ``==`` that of ``meteor_exact``.  0.0 for n == 1."""
    if utility not in MBR_UTILITIES:
        raise ValueError("mbr_utilities: utility %r is not one of %s" % (utility, ", ".join(MBR_UTILITIES)))
    if hasattr(stats, "tolist"):
        stats = stats.tolist()
    if utility == "bleu":
        score = lambda st: bleu_method2_from_stats(st[0:4], st[4:8], st[8], st[9])
    elif utility == "rouge_l":
        score = lambda st: rouge_l_from_stats(st[0], st[1], st[2])
    else:
        score = lambda st: meteor_exact_from_stats(st[0], st[1], st[2], st[3])
    out = []
    for commit in stats:
        n = len(commit)
        row = []
        for i in range(n):
            scores = [score(st) for j, st in enumerate(commit[i]) if j != i]
            row.append(math.fsum(scores) / (n - 1) if n > 1 else 0.0)
        out.append(row)
    return out


def mbr_pick(utilities, logp=None) -> List[int]:
    """Index of the candidate of highest utility per commit; ties go to the larger ``logp[b][i]`` when given, then to the
    lower index (candidates that share no word with any other all have utility 0)."""
    if hasattr(utilities, "tolist"):
        utilities = utilities.tolist()
    if logp is not None and hasattr(logp, "tolist"):
        logp = logp.tolist()
    pick = []
    for b, row in enumerate(utilities):
        if not row:
            raise ValueError("mbr_pick: commit %d has no candidates" % b)
        if logp is not None and len(logp[b]) != len(row):
            raise ValueError("mbr_pick: commit %d has %d utilities and %d log-probabilities" % (b, len(row), len(logp[b])))
        key = (lambda i: (row[i], logp[b][i], -i)) if logp is not None else (lambda i: (row[i], -i))
        pick.append(max(range(len(row)), key=key))
    return pick
