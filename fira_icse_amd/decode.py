"""Test-time search of the reference (run_model.py:202-340) on the HIP engine.

The reference re-runs the whole 6-layer decoder, the 24 650-way generator and the copy head over all 30 positions for
every beam at every step, and moves hypotheses through python lists with a host<->device round trip per step and beam.
Here the encoder, the cross-attention K/V of all layers and ``LinearSource(memory)`` are computed once per batch
(``fira_decode_begin``); every step is one KV-cached pass over the (commit, beam) rows (``fira_decode_step``), and the
hypothesis bookkeeping (probability products, -1 for finished rows, carried finished beams, descending sort, copy-id
resolution) stays on the device with the reference's exact semantics.  ``beam = 1`` is the reference's "greedy".

Every search (``greedy`` / ``greedy_many``, ``sample``, ``score``, ``beam``, ``contrastive``) is the same chunked step loop,
driven by ``_Loop``: static buffers per ``Searcher._ws`` key, the steps captured once into hipGraphs of ``chunk`` steps, replayed chunk by chunk with
at most one device value read back between chunks.  A search supplies its state, its reset, its ``steps(lo, hi)`` (the library
calls of those steps), its stop test and how its results are read out -- nothing else.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import gc
import numbers
import types
from typing import List, Optional, Tuple

import torch

from . import _lib
from .config import EOS, PAD, START, UNK
from .model import DeviceBatch, TransModel


def concurrent_streams(n: int, device, pool: int = 12):
    """``n`` HIP streams that really run side by side.  HIP multiplexes streams onto a few hardware queues (4 by default,
    assigned round-robin in creation order over everything the process has created so far): two streams that land on the same
    queue serialise, and which ones do depends on the process's history.  So: create ``pool`` candidate streams, time a short
    spin kernel on pairs of them, and keep a set whose members overlap with each other (measured: 4 lanes on 4 distinct queues
    run 4 batches of 64 in 17 ms, on 2 queues in 32 ms -- DESIGN.md section 6).  Costs a few milliseconds, once per Searcher."""
    import time
    cands = [torch.cuda.Stream(device=device) for _ in range(max(pool, n))]
    if n <= 1:
        return cands[:1]
    spin = 400_000                                         # cycles of torch.cuda._sleep: ~0.2 ms

    def run(streams):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for st in streams:
            with torch.cuda.stream(st):
                torch.cuda._sleep(spin)
        torch.cuda.synchronize(device)
        return time.perf_counter() - t0

    run(cands[:2])                                         # warm-up
    one = min(run(cands[:1]) for _ in range(3))
    chosen = [cands[0]]
    for c in cands[1:]:
        if len(chosen) == n:
            break
        if all(min(run([c, o]) for _ in range(2)) < 1.5 * one for o in chosen):
            chosen.append(c)
    for c in cands:                                        # fewer distinct queues than lanes: fill up with the rest
        if len(chosen) == n:
            break
        if c not in chosen:
            chosen.append(c)
    return chosen


@dataclasses.dataclass(frozen=True)
class Constraints:
    """What a search must not emit (``fira_constrain_dist``).  A constraint blocks a WORD: its generator id and
    every copy slot of the commit that carries it, so the copy head cannot route around it.

    ``no_repeat_ngram`` n >= 1: no n-gram of words occurs twice in a message (1: no word twice); 0 = off.
    ``min_length`` M: no <eos> before M words (a hypothesis that runs to tar_len ends without one, as always); 0 = off.
    ``banned``: up to 32 vocabulary ids in [UNK, vocab) = [3, vocab) -- <pad>, <eos> and <start> (0..2) cannot be banned,
    <unkm> (3) can; stored sorted and without duplicates, so equal sets compare and hash equal.

    Values are checked here (``ValueError`` with the reason); what depends on the model (n and M against tar_len, ids against
    the vocabulary) is checked by ``check`` when a ``Searcher`` takes the value."""
    no_repeat_ngram: int = 0
    min_length: int = 0
    banned: Tuple[int, ...] = ()

    MAX_BANNED = 32

    def __post_init__(self):
        for name in ("no_repeat_ngram", "min_length"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError("Constraints: %s = %r is not an integer" % (name, v))
            if v < 0:
                raise ValueError("Constraints: %s = %d is negative" % (name, v))
        try:
            ids = list(self.banned)
        except TypeError:
            raise ValueError("Constraints: banned = %r is not a sequence of vocabulary ids" % (self.banned,)) from None
        for w in ids:
            if isinstance(w, bool) or not isinstance(w, int):
                raise ValueError("Constraints: banned id %r is not an integer" % (w,))
            if w < UNK:
                raise ValueError("Constraints: banned id %d is below %d (<pad>, <eos> and <start> cannot be banned)" % (w, UNK))
        ids = tuple(sorted(set(ids)))
        if len(ids) > self.MAX_BANNED:
            raise ValueError("Constraints: %d banned ids, more than %d" % (len(ids), self.MAX_BANNED))
        object.__setattr__(self, "banned", ids)

    @property
    def active(self) -> bool:
        return bool(self.no_repeat_ngram or self.min_length or self.banned)

    def check(self, cfg) -> "Constraints":
        """Against a model's geometry (the kernel's own argument checks, with the names of this class)."""
        if self.no_repeat_ngram > cfg.tar_len:
            raise ValueError("Constraints: no_repeat_ngram = %d exceeds tar_len = %d" % (self.no_repeat_ngram, cfg.tar_len))
        if self.min_length > cfg.tar_len - 2:
            raise ValueError("Constraints: min_length = %d exceeds tar_len - 2 = %d" % (self.min_length, cfg.tar_len - 2))
        for w in self.banned:
            if w >= cfg.vocab_size:
                raise ValueError("Constraints: banned id %d outside the vocabulary [%d, %d)" % (w, UNK, cfg.vocab_size))
        return self


@dataclasses.dataclass(frozen=True)
class BeamScoring:
    """How a beam search ranks its hypotheses (``fira_beam_select_scored``).

    ``length_alpha`` a: hypotheses are ranked by ln(prob) / ((5 + m) / 6)^a, m = words emitted (GNMT's length penalty; 0 = the
    raw probability, under which a hypothesis that ends early wins).
    ``groups`` G and ``diversity`` l: the beam is G groups of beam / G slots; a group ranks a continuation l lower for every
    earlier group that has just appended the same WORD (generator or copied) for the commit, so the groups spell different
    messages (diverse beam search, Hamming diversity).  Both or neither: a penalty needs groups, groups without a penalty
    would search the same thing G times.

    Values are checked here (``ValueError`` with the reason); ``check`` holds the value against a beam size."""
    length_alpha: float = 0.0
    groups: int = 1
    diversity: float = 0.0

    MAX_ALPHA, MAX_GROUPS, MAX_DIVERSITY = 4.0, 8, 1024.0

    def __post_init__(self):
        for name, hi in (("length_alpha", self.MAX_ALPHA), ("diversity", self.MAX_DIVERSITY)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError("BeamScoring: %s = %r is not a number" % (name, v))
            if not 0 <= v <= hi:                              # (also refuses nan)
                raise ValueError("BeamScoring: %s = %r outside [0, %g]" % (name, v, hi))
            object.__setattr__(self, name, float(v))
        g = self.groups
        if isinstance(g, bool) or not isinstance(g, int):
            raise ValueError("BeamScoring: groups = %r is not an integer" % (g,))
        if not 1 <= g <= self.MAX_GROUPS:
            raise ValueError("BeamScoring: groups = %d outside 1..%d" % (g, self.MAX_GROUPS))
        if self.diversity > 0 and g == 1:
            raise ValueError("BeamScoring: diversity = %g needs groups > 1 (the penalty acts between groups)" % self.diversity)
        if g > 1 and self.diversity == 0:
            raise ValueError("BeamScoring: groups = %d needs diversity > 0 (else every group searches the same)" % g)

    def active(self) -> bool:
        return bool(self.length_alpha or self.groups > 1)

    def check(self, beam: int) -> "BeamScoring":
        if beam < 2:
            raise ValueError("BeamScoring: a beam of %d has nothing to rank (beam >= 2)" % beam)
        if beam % self.groups:
            raise ValueError("BeamScoring: groups = %d does not divide the beam of %d" % (self.groups, beam))
        return self

    def inv_lp(self, tar_len: int) -> List[float]:
        """inv_lp[m] = 1 / ((5 + m) / 6)^length_alpha for m = 0 .. tar_len, in float64 (the device buffer rounds it to fp32)."""
        return [1.0 / ((5.0 + m) / 6.0) ** self.length_alpha for m in range(tar_len + 1)]


@dataclasses.dataclass(frozen=True)
class Penalties:
    """Soft word penalties and biases of a search (``fira_penalise_dist``).  Where ``Constraints`` forbids a
    word, this makes it less or more likely: the entries of the WORD -- its generator id and every copy slot of the commit that
    carries it -- are multiplied by a factor; nothing is renormalised.

    ``presence`` a and ``frequency`` f, each in [0, 10] (the OpenAI / vLLM meaning): a word the message holds c >= 1 times is
    multiplied by exp(-(a + f c)) -- the table ``table(tar_len)``: t[c] = float32(exp(-(float64(a) + float64(f) * c))), t[0] = 1.
    A factor that underflows to 0 bans the repeated word.
    ``bias``: None, one mapping {vocabulary id: b} used for every commit, or a sequence of one mapping (or None) per commit
    (the OpenAI ``logit_bias``).  b in [-30, 30]; the word is multiplied by float32(exp(float64(b))) at every step.  At most 16 ids
    per commit, each <eos> (1) or in [UNK, vocab) = [3, vocab): <pad> and <start> are refused.  Stored as sorted (id, b) pairs.

    Values are checked here (``ValueError`` with the reason); what depends on the model and the batch is checked by ``check``
    when a ``Searcher`` takes the value.  The value a search returns under an active ``Penalties`` is the product of the EDITED
    entries taken: a score, not a probability (``Searcher.score`` gives the model's probability of a message)."""
    presence: float = 0.0
    frequency: float = 0.0
    bias: object = None

    MAX_PENALTY, MAX_BIAS, MAX_BIASED = 10.0, 30.0, 16
    MAX_LOG_SCORE = 87.0                             # ln FLT_MAX = 88.72...

    def __post_init__(self):
        for name in ("presence", "frequency"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, numbers.Real):
                raise ValueError("Penalties: %s = %r is not a number" % (name, v))
            if not 0 <= v <= self.MAX_PENALTY:                # (also refuses nan)
                raise ValueError("Penalties: %s = %r outside [0, %g]" % (name, v, self.MAX_PENALTY))
            object.__setattr__(self, name, float(v))
        bias = self.bias
        shared = bias is None or hasattr(bias, "items")
        if shared:
            rows = [bias]
        else:
            try:
                rows = list(bias)
            except TypeError:
                raise ValueError("Penalties: bias = %r is neither a mapping {id: b} nor a sequence of them" % (bias,)) from None
        out = []
        for k, row in enumerate(rows):
            where = "bias" if shared else "bias of commit %d" % k
            if row is None:
                out.append(())
                continue
            if not hasattr(row, "items"):
                raise ValueError("Penalties: %s = %r is not a mapping {id: b}" % (where, row))
            pairs = list(row.items())
            for w, b in pairs:
                if isinstance(w, bool) or not isinstance(w, numbers.Integral):
                    raise ValueError("Penalties: %s: id %r is not an integer" % (where, w))
                if w != EOS and w < UNK:
                    raise ValueError("Penalties: %s: id %d is neither <eos> (%d) nor at least %d (<pad> and <start> cannot be "
                                     "biased)" % (where, w, EOS, UNK))
                if isinstance(b, bool) or not isinstance(b, numbers.Real):
                    raise ValueError("Penalties: %s: the bias %r of id %d is not a number" % (where, b, w))
                if not -self.MAX_BIAS <= b <= self.MAX_BIAS:  # (also refuses nan)
                    raise ValueError("Penalties: %s: the bias %r of id %d is outside [-%g, %g]" % (where, b, w, self.MAX_BIAS,
                                                                                                  self.MAX_BIAS))
            if len(pairs) > self.MAX_BIASED:                  # (a mapping's keys are distinct: so are the ids)
                raise ValueError("Penalties: %s: %d ids, more than %d" % (where, len(pairs), self.MAX_BIASED))
            out.append(tuple(sorted((int(w), float(b)) for w, b in pairs)))
        object.__setattr__(self, "bias", None if bias is None else out[0] if shared else tuple(out))
        object.__setattr__(self, "_shared", shared)

    @property
    def active(self) -> bool:
        return bool(self.presence or self.frequency or any(b for row in self._rows(1) for _, b in row))

    def _rows(self, B: int):
        """The (id, b) pairs of each of B commits (a per-commit value: of the commits it was given for)."""
        if self.bias is None:
            return [()] * B
        return [self.bias] * B if self._shared else list(self.bias)

    def check(self, cfg, B: int) -> "Penalties":
        """Against a model's geometry and a batch of B commits: the number of mappings, the ids against the vocabulary, and the
        overflow bound max(b, 0) * (tar_len - 1) <= 87 -- a message's score is a product of at most tar_len - 1 edited values,
        each at most exp(max b), and ln FLT_MAX = 88.7."""
        if not self._shared and len(self.bias) != B:
            raise ValueError("Penalties: %d bias mappings for a batch of %d commits" % (len(self.bias), B))
        for k, row in enumerate(self._rows(B)):
            for w, b in row:
                if w >= cfg.vocab_size:
                    raise ValueError("Penalties: commit %d: id %d outside the vocabulary [%d, %d)" % (k, w, UNK, cfg.vocab_size))
                if max(b, 0.0) * (cfg.tar_len - 1) > self.MAX_LOG_SCORE:
                    raise ValueError("Penalties: commit %d: the bias %g of id %d times tar_len - 1 = %d exceeds %g (a message's "
                                     "score could overflow fp32): at most %g" % (k, b, w, cfg.tar_len - 1, self.MAX_LOG_SCORE,
                                                                                 self.MAX_LOG_SCORE / (cfg.tar_len - 1)))
        return self

    def table(self, tar_len: int):
        """count_factor [tar_len] float32: the exponent formed in float64, the factor cast once -- the kernel's work is then one
        fp32 multiplication, which numpy repeats bit for bit."""
        import numpy as np
        c = np.arange(tar_len, dtype=np.float64)
        t = np.exp(-(np.float64(self.presence) + np.float64(self.frequency) * c)).astype(np.float32)
        t[0] = np.float32(1.0)
        return t

    def bias_arrays(self, B: int):
        """(bias_id [B, 16] int32, bias_factor [B, 16] float32 = float32(exp(float64(b))), n_bias [B] int32) of B commits;
        unused pairs hold id 0 and factor 1."""
        import numpy as np
        ids = np.zeros((B, self.MAX_BIASED), dtype=np.int32)
        fac = np.ones((B, self.MAX_BIASED), dtype=np.float32)
        n = np.zeros(B, dtype=np.int32)
        for k, row in enumerate(self._rows(B)):
            n[k] = len(row)
            for q, (w, b) in enumerate(row):
                ids[k, q] = w
                fac[k, q] = np.float32(np.exp(np.float64(b)))
        return ids, fac, n


@dataclasses.dataclass(frozen=True)
class Phrases:
    """Word SEQUENCES in the hard search controls: what a message must not contain and what it must
    contain, where ``Constraints.banned`` and ``beam(require=)`` speak of single words.

    ``banned``: phrases of 2..4 vocabulary ids in [UNK, vocab) -- one list of phrases used for every commit, or a sequence of one
    list per commit; at most 8 per commit.  ``fira_ban_phrases_dist`` blocks the word that would complete a listed phrase: its
    generator id and every copy slot of the commit that carries it, as ``no_repeat_ngram`` blocks the word that would complete
    an n-gram the hypothesis already holds.  Taken by ``greedy``, ``greedy_many``, ``beam`` and ``sample_search``.
    ``required``: one list of ITEMS per commit, an item being 1..4 ids in (UNK, vocab) that the message must hold contiguously;
    at most 4 items per commit whose lengths sum to at most 4 (the selection keeps five banks); an empty list means no
    requirement for that commit.  ``fira_beam_select_phrases`` divides the beam into banks by ``progress`` (the words of the
    completed items plus the longest phrase start the hypothesis ends in).  Taken by ``beam`` only.

    Values are checked here (``ValueError`` with the reason); what depends on the model, the batch and the other options is
    checked when a ``Searcher`` takes the value.  Stored as tuples, so equal values compare and hash equal."""
    banned: object = ()
    required: object = ()

    MAX_BANNED, MAX_WORDS, MAX_ITEMS, MAX_REQUIRED_WORDS = 8, 4, 4, 4

    @staticmethod
    def _ids(seq, what, lowest):
        out = []
        for w in seq:
            if isinstance(w, bool) or not isinstance(w, numbers.Integral):
                raise ValueError("Phrases: %s: id %r is not an integer" % (what, w))
            if w < lowest:
                raise ValueError("Phrases: %s: id %d is below %d" % (what, w, lowest))
            out.append(int(w))
        return tuple(out)

    @staticmethod
    def _seq(x):
        return not isinstance(x, (str, bytes)) and hasattr(x, "__iter__")

    def __post_init__(self):
        seq = self._seq
        banned = self.banned
        if banned is None:
            banned = ()
        if not seq(banned):
            raise ValueError("Phrases: banned = %r is not a sequence of phrases" % (banned,))
        banned = [list(p) if seq(p) else p for p in banned]
        if any(not seq(p) for p in banned):
            raise ValueError("Phrases: banned = %r is neither a list of phrases nor one list of phrases per commit" % (self.banned,))
        # one list for every commit: every element is a non-empty sequence of ids; else one list (possibly empty) per commit
        shared = all(len(p) > 0 and not any(seq(w) for w in p) for p in banned)
        rows = [banned] if shared else banned
        out = []
        for k, row in enumerate(rows):
            where = "banned" if shared else "banned phrases of commit %d" % k
            phrases = []
            for ph in row:
                if not seq(ph):
                    raise ValueError("Phrases: %s: %r is not a phrase (a sequence of ids)" % (where, ph))
                ph = self._ids(ph, where, UNK)
                if len(ph) == 1:
                    raise ValueError("Phrases: %s: (%d,) is one word; a single word is banned with Constraints.banned" % (where, ph[0]))
                if not 2 <= len(ph) <= self.MAX_WORDS:
                    raise ValueError("Phrases: %s: a phrase of %d words, outside 2..%d" % (where, len(ph), self.MAX_WORDS))
                if ph in phrases:
                    raise ValueError("Phrases: %s: the phrase %r is listed twice" % (where, ph))
                phrases.append(ph)
            if len(phrases) > self.MAX_BANNED:
                raise ValueError("Phrases: %s: %d phrases, more than %d" % (where, len(phrases), self.MAX_BANNED))
            out.append(tuple(phrases))
        required = self.required
        if required is None:
            required = ()
        if not seq(required) or any(not seq(row) for row in required):
            raise ValueError("Phrases: required = %r is not one list of items per commit" % (required,))
        req = []
        for k, row in enumerate(required):
            where = "required items of commit %d" % k
            items = []
            for item in row:
                if not seq(item):
                    raise ValueError("Phrases: %s: %r is not an item (a sequence of 1..%d ids)" % (where, item, self.MAX_WORDS))
                item = self._ids(item, where, UNK + 1)
                if not 1 <= len(item) <= self.MAX_WORDS:
                    raise ValueError("Phrases: %s: an item of %d words, outside 1..%d" % (where, len(item), self.MAX_WORDS))
                items.append(item)
            if len(items) > self.MAX_ITEMS:
                raise ValueError("Phrases: %s: %d items, more than %d" % (where, len(items), self.MAX_ITEMS))
            if sum(len(i) for i in items) > self.MAX_REQUIRED_WORDS:
                raise ValueError("Phrases: %s: %d words in all, more than %d (one bank per word)"
                                 % (where, sum(len(i) for i in items), self.MAX_REQUIRED_WORDS))
            for a, x in enumerate(items):
                for c, y in enumerate(items):
                    if a != c and len(x) <= len(y) and any(y[o:o + len(x)] == x for o in range(len(y) - len(x) + 1)) \
                            and (len(x) < len(y) or a > c):
                        raise ValueError("Phrases: %s: the item %r %s %r" % (where, x, "duplicates" if x == y else "is part of", y))
            req.append(tuple(items))
        object.__setattr__(self, "banned", out[0] if shared else tuple(out))
        object.__setattr__(self, "required", tuple(req))
        object.__setattr__(self, "_shared", shared)

    @property
    def ban_active(self) -> bool:
        return any(self.banned_rows(1)) if self._shared else any(self.banned)

    @property
    def require_active(self) -> bool:
        return any(self.required)

    @property
    def active(self) -> bool:
        return self.ban_active or self.require_active

    def banned_rows(self, B: int):
        """The banned phrases of each of B commits (a per-commit value: of the commits it was given for)."""
        return [self.banned] * B if self._shared else list(self.banned)

    def check(self, cfg, B: int) -> "Phrases":
        """Against a model's geometry and a batch of B commits: the counts of lists and the ids against the vocabulary."""
        if not self._shared and self.banned and len(self.banned) != B:
            raise ValueError("Phrases: %d lists of banned phrases for a batch of %d commits" % (len(self.banned), B))
        if self.required and len(self.required) != B:
            raise ValueError("Phrases: %d lists of required items for a batch of %d commits" % (len(self.required), B))
        for what, rows in (("banned", self.banned_rows(B)), ("required", self.required)):
            for k, row in enumerate(rows):
                for ph in row:
                    for w in ph:
                        if w >= cfg.vocab_size:
                            raise ValueError("Phrases: commit %d: %s id %d outside the vocabulary (below %d)"
                                             % (k, what, w, cfg.vocab_size))
        return self

    def banned_arrays(self, B: int):
        """(phrase [B, 8, 4] int32, phrase_len [B, 8] int32, n_phrases [B] int32) of B commits; unused places hold 0."""
        import numpy as np
        words = np.zeros((B, self.MAX_BANNED, self.MAX_WORDS), dtype=np.int32)
        lens = np.zeros((B, self.MAX_BANNED), dtype=np.int32)
        n = np.zeros(B, dtype=np.int32)
        for k, row in enumerate(self.banned_rows(B)):
            n[k] = len(row)
            for q, ph in enumerate(row):
                words[k, q, :len(ph)] = ph
                lens[k, q] = len(ph)
        return words, lens, n

    def required_arrays(self, B: int):
        """(words [B, 4] int32: the items' words concatenated, item_len [B, 4] int32, n_items [B] int32) of B commits."""
        import numpy as np
        words = np.zeros((B, self.MAX_REQUIRED_WORDS), dtype=np.int32)
        lens = np.zeros((B, self.MAX_ITEMS), dtype=np.int32)
        n = np.zeros(B, dtype=np.int32)
        for k, row in enumerate(self.required or [()] * B):
            flat = [w for item in row for w in item]
            words[k, :len(flat)] = flat
            lens[k, :len(row)] = [len(item) for item in row]
            n[k] = len(row)
        return words, lens, n


def contains_phrase(words, phrase) -> bool:
    """``phrase`` occurs contiguously in ``words``."""
    words, phrase = list(words), list(phrase)
    return any(words[o:o + len(phrase)] == phrase for o in range(len(words) - len(phrase) + 1))


@dataclasses.dataclass(frozen=True)
class Template:
    """A TEMPLATE in the hard search controls: a deterministic automaton over word classes that every
    message must be accepted by -- the general form of ``Constraints.banned``, ``prefix=`` and ``Phrases(banned=)``, each of which
    is a regular language over words.  ``fira_template_dist`` blocks, at every step, the words after which no accepted message
    fits into the buffer any more, and <eos> wherever the automaton does not accept.  ``Template.sequence`` builds one from a
    list of (word set, at least, at most) items.

    ``word_class``: the class 0 .. C-1 of the vocabulary ids -- a ``{id: class}`` mapping (every id not named has class 0) or a
    full sequence of ``vocab_size`` classes.  <pad>, <start> and <unkm> are ordinary ids; <eos> is no word: a mapping must not
    name it, and its place in a full sequence is never used.
    ``next``: S rows of C targets: the state after a word of that class, or -1 for "no such word here"; S, C <= 32.
    ``accept``: the states in which a message may end.
    ``start``: the start state -- one for every commit, or a sequence of one per commit, so that one union automaton serves a
    batch whose commits follow different rules.

    The default value has no state: it is inactive, and a search that is given it is the plain search.  Values are checked here
    (``ValueError`` with the reason); what depends on the model and the batch is checked by ``check`` when a ``Searcher`` takes
    the value.  Stored as tuples, so equal values compare and hash equal."""
    word_class: object = ()
    next: object = ()
    accept: object = ()
    start: object = 0

    MAX_STATES, MAX_CLASSES, NEVER = 32, 32, 1 << 20

    @staticmethod
    def _int(v, what):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError("Template: %s %r is not an integer" % (what, v))
        return int(v)

    def __post_init__(self):
        seq = Phrases._seq
        if not seq(self.next) or any(not seq(row) for row in self.next):
            raise ValueError("Template: next = %r is not a sequence of rows of target states" % (self.next,))
        nxt = tuple(tuple(self._int(t, "next: target") for t in row) for row in self.next)
        S = len(nxt)
        if S > self.MAX_STATES:
            raise ValueError("Template: %d states, more than %d states" % (S, self.MAX_STATES))
        C_ = len(nxt[0]) if S else 0
        if any(len(row) != C_ for row in nxt):
            raise ValueError("Template: next: the rows have different numbers of classes")
        if C_ > self.MAX_CLASSES:
            raise ValueError("Template: %d classes, more than %d classes" % (C_, self.MAX_CLASSES))
        if S and C_ == 0:
            raise ValueError("Template: next: no class (class 0, every word not named, always exists)")
        for s, row in enumerate(nxt):
            for c, t in enumerate(row):
                if not -1 <= t < S:
                    raise ValueError("Template: next[%d][%d] = %d is a target outside -1..%d" % (s, c, t, S - 1))
        if not seq(self.accept):
            raise ValueError("Template: accept = %r is not a sequence of states" % (self.accept,))
        accept = tuple(sorted(set(self._int(s, "accept: state") for s in self.accept)))
        for s in accept:
            if not 0 <= s < S:
                raise ValueError("Template: accept: state %d outside 0..%d" % (s, S - 1))
        shared = not seq(self.start)
        start = (self._int(self.start, "start: state"),) if shared else tuple(self._int(s, "start: state") for s in self.start)
        for s in start:
            if S and not 0 <= s < S:
                raise ValueError("Template: start: state %d outside 0..%d (wrong range)" % (s, S - 1))
        wc = self.word_class
        full = not isinstance(wc, dict)
        if full and not seq(wc):
            raise ValueError("Template: word_class = %r is neither an {id: class} mapping nor a sequence of classes" % (wc,))
        pairs = list(enumerate(wc)) if full else sorted((self._int(w, "word_class: id"), c) for w, c in wc.items())
        classes = []
        for w, c in pairs:
            c = self._int(c, "word_class: class of id %d:" % w)
            if w < 0:
                raise ValueError("Template: word_class: id %d is negative" % w)
            if not 0 <= c < max(C_, 1):
                raise ValueError("Template: word_class: id %d has class %d outside 0..%d" % (w, c, max(C_, 1) - 1))
            classes.append(c)
        # need[s]: the fewest words from s to an accepting state (breadth first, backwards from the accepting states)
        need = [0 if s in accept else self.NEVER for s in range(S)]
        frontier = list(accept)
        while frontier:
            reached = []
            for s in range(S):
                if need[s] == self.NEVER and any(t in frontier for t in nxt[s]):
                    need[s] = need[frontier[0]] + 1
                    reached.append(s)
            frontier = reached
        object.__setattr__(self, "next", nxt)
        object.__setattr__(self, "accept", accept)
        object.__setattr__(self, "start", start[0] if shared else start)
        object.__setattr__(self, "word_class", tuple(classes) if full else tuple((w, c) for (w, _), c in zip(pairs, classes)))
        object.__setattr__(self, "_full", full)
        object.__setattr__(self, "_class_of", None if full else dict(self.word_class))
        object.__setattr__(self, "need", tuple(need))

    @property
    def n_states(self) -> int:
        return len(self.next)

    @property
    def n_classes(self) -> int:
        return len(self.next[0]) if self.next else 0

    @property
    def active(self) -> bool:
        return self.n_states > 0

    def class_of(self, w: int) -> int:
        """The class of the word ``w``; an id that is not named, or outside the vocabulary, has class 0."""
        if self._full:
            return self.word_class[w] if 0 <= w < len(self.word_class) else 0
        return self._class_of.get(w, 0)

    def start_rows(self, B: int):
        """The start state of each of B commits."""
        return [self.start] * B if isinstance(self.start, int) else list(self.start)

    def walk(self, words, state: int) -> int:
        """The state after ``words`` from ``state``; -1 once there is no transition."""
        for w in words:
            if state < 0:
                break
            state = self.next[state][self.class_of(int(w))]
        return state

    def accepts(self, ids, commit: int = 0) -> bool:
        """The automaton of commit ``commit`` accepts the message ``ids``: the words after <start>, with or without the <eos>
        that ends them (a message that filled the buffer has none).  The inactive value accepts everything."""
        words = [int(w) for w in ids]
        if words and words[-1] == EOS:
            words.pop()
        if not self.active:
            return True
        if EOS in words:
            return False
        return self.walk(words, self.start_rows(commit + 1)[commit]) in self.accept

    def longest_fits(self, state: int, least: int, most: int) -> bool:
        """From ``state`` some accepted message has between ``least`` and ``most`` words (a dynamic program over (state, words))."""
        reach = {state} if state >= 0 else set()
        for n in range(most + 1):
            if n >= least and reach & set(self.accept):
                return True
            reach = {t for s in reach for t in self.next[s] if t >= 0}
        return False

    def check(self, cfg, B: int) -> "Template":
        """Against a model's geometry and a batch of B commits."""
        V, T = cfg.vocab_size, cfg.tar_len
        if self._full:
            if len(self.word_class) != V:
                raise ValueError("Template: word_class: %d classes for a vocabulary of %d ids" % (len(self.word_class), V))
        else:
            for w, _ in self.word_class:
                if w >= V:
                    raise ValueError("Template: word_class: id %d outside the vocabulary [0, %d)" % (w, V))
                if w == EOS:
                    raise ValueError("Template: word_class: <eos> (id %d) is named; it is no word, accept says where a message "
                                     "may end" % EOS)
        if not isinstance(self.start, int) and len(self.start) != B:
            raise ValueError("Template: start: %d states for a batch of %d commits (wrong length)" % (len(self.start), B))
        for b, s in enumerate(self.start_rows(B)):
            if self.need[s] > T - 1:
                raise ValueError("Template: commit %d: no accepted message within tar_len - 1 = %d words from state %d"
                                 % (b, T - 1, s))
        return self

    def arrays(self, B: int, vocab_size: Optional[int] = None):
        """The device tables of B commits as numpy arrays: (word_class [V] uint8, next [32 * 32] int8 with pitch 32, need [32]
        int32, start [B] int32).  Rows of states that do not exist hold -1 (need: ``NEVER``); the columns of classes that do
        not exist repeat class 0's, so a state that takes every word allows all 32 classes and the kernel returns early."""
        import numpy as np
        V = len(self.word_class) if self._full else vocab_size
        if V is None:
            raise ValueError("Template: arrays needs vocab_size for an {id: class} mapping")
        wc = np.zeros(V, dtype=np.uint8)
        if self._full:
            wc[:] = self.word_class
        else:
            for w, c in self.word_class:
                wc[w] = c
        S, C_ = self.n_states, self.n_classes
        nxt = np.full((self.MAX_STATES, self.MAX_CLASSES), -1, dtype=np.int8)
        need = np.full(self.MAX_STATES, self.NEVER, dtype=np.int32)
        if S:
            nxt[:S, :C_] = self.next
            nxt[:S, C_:] = nxt[:S, :1]
            need[:S] = self.need
        return wc, nxt.reshape(-1), need, np.array(self.start_rows(B), dtype=np.int32)

    @classmethod
    def sequence(cls, items, vocab_size: int, start=0) -> "Template":
        """The template "``items`` in this order": every item is (ids or None, lo, hi) -- a word from this set of vocabulary ids,
        or any word for None, between ``lo`` and ``hi`` times, ``hi=None`` meaning unbounded.  The classes are the distinct
        membership signatures of the ids in the sets (class 0: in no set), the states come from the subset construction, so
        adjacent sets may overlap ("any word, 0 to 3 times" followed by ":").  More than 32 of either is a ``ValueError``."""
        V = cls._int(vocab_size, "sequence: vocab_size")
        sets, units = [], []                               # units: (set index or None, optional); loops: node -> set index
        loops = {}
        for k, item in enumerate(items):
            try:
                ids, lo, hi = item
            except (TypeError, ValueError):
                raise ValueError("Template.sequence: item %d: %r is not (ids or None, lo, hi)" % (k, item)) from None
            lo = cls._int(lo, "sequence: item %d: lo" % k)
            hi = None if hi is None else cls._int(hi, "sequence: item %d: hi" % k)
            if lo < 0 or (hi is not None and hi < lo):
                raise ValueError("Template.sequence: item %d: counts %d..%r are not 0 <= lo <= hi" % (k, lo, hi))
            if ids is not None:
                if not Phrases._seq(ids):
                    raise ValueError("Template.sequence: item %d: %r is neither a set of ids nor None" % (k, ids))
                ids = frozenset(cls._int(w, "sequence: item %d: id" % k) for w in ids)
                for w in sorted(ids):
                    if not 0 <= w < V:
                        raise ValueError("Template.sequence: item %d: id %d outside the vocabulary [0, %d)" % (k, w, V))
                    if w == EOS:
                        raise ValueError("Template.sequence: item %d: <eos> (id %d) is named; it is no word" % (k, EOS))
                if not ids:
                    raise ValueError("Template.sequence: item %d: an empty set of ids" % k)
            if lo > cls.MAX_STATES or (hi is not None and hi - lo > cls.MAX_STATES):
                raise ValueError("Template.sequence: item %d: counting %d..%r words takes more than %d states"
                                 % (k, lo, hi, cls.MAX_STATES))
            if ids is not None and ids not in sets:
                sets.append(ids)
            j = None if ids is None else sets.index(ids)
            units += [(j, False)] * lo + [(j, True)] * (0 if hi is None else hi - lo)
            if hi is None:
                loops.setdefault(len(units), []).append(j)
        # classes: the membership signature of every id; class 0 is "in no set"
        sig_class = {(False,) * len(sets): 0}
        word_class = {}
        for w in sorted(set().union(*sets) if sets else ()):
            c = sig_class.setdefault(tuple(w in s for s in sets), len(sig_class))
            word_class[w] = c
        if len(sig_class) > cls.MAX_CLASSES:
            too_many_classes = len(sig_class)
        else:
            too_many_classes = 0
        takes = lambda j, sig: j is None or sig[j]         # a unit or a loop over set j (None: any word) takes a word of sig
        final = len(units)

        def closure(nodes):
            out = set()
            for n in nodes:
                out.add(n)
                while n < final and units[n][1]:           # an optional unit may be skipped
                    n += 1
                    out.add(n)
            return frozenset(out)

        sigs = sorted(sig_class, key=sig_class.get)
        states = {closure({0}): 0}
        order = [closure({0})]
        nxt = []
        for sub in order:                                  # (grows while it is walked)
            row = []
            for sig in sigs:
                to = set()
                for n in sub:
                    if n < final and takes(units[n][0], sig):
                        to.add(n + 1)
                    if any(takes(j, sig) for j in loops.get(n, ())):
                        to.add(n)
                if not to:
                    row.append(-1)
                    continue
                to = closure(to)
                if to not in states:
                    states[to] = len(order)
                    order.append(to)
                    if len(order) > cls.MAX_STATES:
                        raise ValueError("Template.sequence: the items take more than %d states" % cls.MAX_STATES)
                row.append(states[to])
            nxt.append(row)
        if too_many_classes:
            raise ValueError("Template.sequence: the sets divide the vocabulary into %d classes, more than %d classes"
                             % (too_many_classes, cls.MAX_CLASSES))
        return cls(word_class, nxt, [k for k, sub in enumerate(order) if final in sub], start)


def looks_like_an_identifier(word: str) -> bool:
    """The default predicate of ``WordSets.grounded``: the word contains a digit, ``_``, ``.``, ``/`` or an inner capital (a
    capital letter after the first character) -- the shape of identifiers, file names and ticket-like tokens."""
    return any(ch.isdigit() or ch in "_./" for ch in word) or any(ch.isupper() for ch in word[1:])


@dataclasses.dataclass(frozen=True)
class WordSets:
    """Per-commit WORD SETS in the search controls (``fira_wordset_dist``): the hard and the soft word
    controls at the scale of the vocabulary, where ``Constraints.banned`` takes 32 ids and ``Penalties.bias`` 16.  A set speaks of
    WORDS: the generator id and every copy slot of the commit that carries it.

    ``allow``: only these ids (and <eos>, always) may be written.  ``deny``: these ids may not.  ``boost``: these ids are
    multiplied by float32(exp(float64(``boost_bias``))) at every step.  Each is None, one iterable of vocabulary ids used for
    every commit, or a list of one iterable per commit.  ``boost_bias`` b in [-30, 30]: one number, or a list of one per commit.
    ``ground``: one iterable of ids for every commit (a property of the vocabulary): such an id may be written only if a valid
    copy slot of the commit carries it -- "identifier-like words only if the diff has them" (``WordSets.grounded``).

    The default value holds nothing: it is inactive, and a search that is given it is the plain search.  A given ``allow`` is
    active whatever it holds; ``deny`` and ``ground`` are active if they hold an id; ``boost`` if it holds an id and some bias is
    not 0.  Values are checked here (``ValueError`` with the reason); what depends on the model and the batch is checked by
    ``check`` when a ``Searcher`` takes the value.  Stored as sorted tuples, so equal values compare and hash equal.  Under an
    active ``boost`` the value a search returns is the product of the EDITED entries taken: a score, not a probability
    (``Searcher.score`` gives the model's probability of a message)."""
    allow: object = None
    deny: object = None
    boost: object = None
    boost_bias: object = 0.0
    ground: object = None

    MAX_BIAS, MAX_LOG_SCORE = Penalties.MAX_BIAS, Penalties.MAX_LOG_SCORE

    @staticmethod
    def _ids(ids, where):
        out = []
        for w in ids:
            if isinstance(w, bool) or not isinstance(w, numbers.Integral):
                raise ValueError("WordSets: %s: id %r is not an integer" % (where, w))
            out.append(int(w))
        return tuple(sorted(set(out)))

    def __post_init__(self):
        seq = Phrases._seq
        shared = {}
        for name in ("allow", "deny", "boost"):
            v = getattr(self, name)
            if v is None:
                shared[name] = True
                continue
            if not seq(v):
                raise ValueError("WordSets: %s = %r is neither an iterable of vocabulary ids nor a list of one per commit" % (name, v))
            v = list(v)
            per_commit = bool(v) and all(x is None or seq(x) for x in v)
            if per_commit:
                value = tuple(self._ids(() if x is None else x, "%s of commit %d" % (name, k)) for k, x in enumerate(v))
            else:
                value = self._ids(v, name)
            shared[name] = not per_commit
            object.__setattr__(self, name, value)
        if self.ground is not None:
            if not seq(self.ground):
                raise ValueError("WordSets: ground = %r is not an iterable of vocabulary ids" % (self.ground,))
            g = list(self.ground)
            if any(seq(x) for x in g):
                raise ValueError("WordSets: ground is one set for every commit (a property of the vocabulary), not one per commit")
            object.__setattr__(self, "ground", self._ids(g, "ground"))
        bias = self.boost_bias
        bias_shared = not seq(bias)
        values = []
        for k, b in enumerate([bias] if bias_shared else list(bias)):
            where = "boost_bias" if bias_shared else "boost_bias of commit %d" % k
            if isinstance(b, bool) or not isinstance(b, numbers.Real):
                raise ValueError("WordSets: %s = %r is not a number" % (where, b))
            if not -self.MAX_BIAS <= b <= self.MAX_BIAS:      # (also refuses nan)
                raise ValueError("WordSets: %s = %r is outside [-%g, %g]" % (where, b, self.MAX_BIAS, self.MAX_BIAS))
            values.append(float(b))
        object.__setattr__(self, "boost_bias", values[0] if bias_shared else tuple(values))
        object.__setattr__(self, "_shared", dict(shared, boost_bias=bias_shared))

    def _rows(self, name: str, B: int):
        """The ids of set ``name`` for each of B commits, or None for a set that is not given."""
        v = getattr(self, name)
        if v is None:
            return None
        return [v] * B if name == "ground" or self._shared[name] else list(v)

    def bias_rows(self, B: int):
        return [self.boost_bias] * B if self._shared["boost_bias"] else list(self.boost_bias)

    @property
    def given(self):
        """Which sets a launch gets, as the tuple of their names in the order allow, deny, boost, ground."""
        out = []
        if self.allow is not None:
            out.append("allow")
        if any(self._rows("deny", 1) or ()):
            out.append("deny")
        if any(self._rows("boost", 1) or ()) and any(self.bias_rows(1)):
            out.append("boost")
        if self.ground:
            out.append("ground")
        return tuple(out)

    @property
    def active(self) -> bool:
        return bool(self.given)

    def check(self, cfg, B: int) -> "WordSets":
        """Against a model's geometry and a batch of B commits: the list lengths, every id against the vocabulary and the special
        ids, an ``allow`` that holds nothing, and the overflow bound max(b, 0) * (tar_len - 1) <= 87 of ``Penalties``."""
        V, T = cfg.vocab_size, cfg.tar_len
        for name in ("allow", "deny", "boost", "boost_bias"):
            if not self._shared[name] and len(getattr(self, name)) != B:
                raise ValueError("WordSets: %s: %d lists for a batch of %d commits" % (name, len(getattr(self, name)), B)
                                 if name != "boost_bias" else
                                 "WordSets: boost_bias: %d values for a batch of %d commits" % (len(self.boost_bias), B))
        for name in ("allow", "deny", "boost", "ground"):
            for k, row in enumerate(self._rows(name, B) or ()):
                where = name if name == "ground" or self._shared[name] else "%s of commit %d" % (name, k)
                for w in row:
                    if not 0 <= w < V:
                        raise ValueError("WordSets: %s: id %d outside the vocabulary [0, %d)" % (where, w, V))
                    if w in (PAD, START):
                        raise ValueError("WordSets: %s: id %d is <pad> or <start>, which no set may hold" % (where, w))
                    if w == EOS and name in ("deny", "ground"):
                        raise ValueError("WordSets: %s: <eos> (id %d) cannot be in %s (Constraints.min_length holds a message "
                                         "open)" % (where, EOS, name))
                if name == "allow" and not row:
                    raise ValueError("WordSets: %s: commit %d is allowed no word at all" % (where, k))
                if name == "ground" or self._shared[name]:
                    break                                      # (one set for every commit: checked once)
        for k, b in enumerate(self.bias_rows(B)):
            if max(b, 0.0) * (T - 1) > self.MAX_LOG_SCORE:
                raise ValueError("WordSets: commit %d: boost_bias = %g times tar_len - 1 = %d exceeds %g (a message's score could "
                                 "overflow fp32): at most %g" % (k, b, T - 1, self.MAX_LOG_SCORE, self.MAX_LOG_SCORE / (T - 1)))
        return self

    def blocks(self, w: int, commit: int, B: int) -> bool:
        """``allow`` or ``deny`` blocks the word ``w`` for commit ``commit`` of B (``ground`` depends on the batch: not here)."""
        allow, deny = self._rows("allow", B), self._rows("deny", B)
        return (allow is not None and w != EOS and w not in allow[commit]) or (deny is not None and w in deny[commit])

    @staticmethod
    def pack(rows, vocab_size: int):
        """[len(rows), ceil(vocab_size / 32)] uint32: bit w % 32 of word w / 32 set for every id w of the row."""
        import numpy as np
        out = np.zeros((len(rows), (vocab_size + 31) // 32), dtype=np.uint32)
        cache = {}
        for k, row in enumerate(rows):
            if id(row) not in cache:
                ids = np.asarray(row, dtype=np.int64).reshape(-1)
                words = np.zeros(out.shape[1], dtype=np.uint32)
                np.bitwise_or.at(words, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
                cache[id(row)] = words
            out[k] = cache[id(row)]
        return out

    def arrays(self, B: int, vocab_size: int):
        """The device buffers of B commits as numpy arrays: a dict with "allow" / "deny" / "boost" / "ground", each
        [B, ceil(vocab_size / 32)] uint32 for a set in ``given`` and None otherwise, and "boost_factor" [B] float32 =
        float32(exp(float64(b))).  No bit at or past ``vocab_size`` is set."""
        import numpy as np
        given = self.given
        out = {name: self.pack(self._rows(name, B), vocab_size) if name in given else None
               for name in ("allow", "deny", "boost", "ground")}
        out["boost_factor"] = np.exp(np.asarray(self.bias_rows(B), dtype=np.float64)).astype(np.float32)
        return out

    @classmethod
    def grounded(cls, words, is_identifier=looks_like_an_identifier, **sets) -> "WordSets":
        """The value whose ``ground`` holds every id of the vocabulary list ``words`` (id = position) from UNK + 1 on whose word
        ``is_identifier`` accepts: such a word can then be written only where the commit's diff carries it.  ``sets``: the other
        fields."""
        return cls(ground=[w for w, word in enumerate(words) if w > UNK and is_identifier(word)], **sets)


class Scores(dict):
    """Result of ``Searcher.score``: a dict whose keys also read as attributes."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


MAX_MODELS = 8                                   # fira_mix_dist: 2 <= n_members <= 8
MAX_REQUIRED = 4                                 # fira_beam_select_required: required[B, 4]


def ensemble_weights(weights, n_models: int):
    """The mixing weights of an ensemble of ``n_models`` models as a float32 numpy array, the primary first.  None: uniform,
    np.float32(1) / np.float32(M).  Given weights are normalised in float64 to sum 1, then cast to float32.  ``ValueError`` on a
    wrong count, a negative or non-finite weight, or weights that sum to 0."""
    import numpy as np
    if weights is None:
        return np.full(n_models, np.float32(1) / np.float32(n_models), dtype=np.float32)
    try:
        w = np.array([float(x) for x in weights], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("weights: %r is not a sequence of numbers" % (weights,)) from None
    if w.shape != (n_models,):
        raise ValueError("weights: %d values for %d models (one per model, the primary first)" % (w.size, n_models))
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weights: %s holds a negative or non-finite value" % (w.tolist(),))
    if not w.sum() > 0:
        raise ValueError("weights: %s sum to 0" % (w.tolist(),))
    return (w / w.sum()).astype(np.float32)


class _Members:
    """What ``Searcher._begin`` hands to ``Searcher._step`` for an ensemble in place of the one decode workspace: the decode
    workspace and the [R, out_len] distribution buffer of every member, and the host arrays ``fira_mix_dist`` reads at launch."""

    def __init__(self, ws, dist, weights):
        self.ws, self.dist = ws, dist
        self.ptrs = (C.c_void_p * len(dist))(*[t.data_ptr() for t in dist])
        self.weights = (C.c_float * len(dist))(*[float(x) for x in weights])


def neighbour_coef(sim, lam: float, min_sim: float = 0.0):
    """The mixing coefficients of ``fira_mix_neighbour`` as a float32 numpy array [B, 2]: with c = lam * sim[b], formed in
    float64, (a, b) = (float32(1 / (1 + c)), float32(c / (1 + c))); a commit with sim < min_sim gets (1, 0)."""
    import numpy as np
    sim = np.asarray(sim, dtype=np.float64).reshape(-1)
    c = float(lam) * sim
    out = np.stack([1.0 / (1.0 + c), c / (1.0 + c)], axis=1)
    out[sim < float(min_sim)] = (1.0, 0.0)
    return out.astype(np.float32)


@dataclasses.dataclass(frozen=True, eq=False)
class Neighbour:
    """The retrieved neighbours of a batch: ``db`` is a ``DeviceBatch`` of the same B whose row b is the
    training commit nearest to commit b, ``sim`` [B] their similarities in [0, 1] (``retrieve.Datastore.query``).  At every
    step the distribution the model predicts for the neighbour on the same tokens, folded into words, is mixed into the
    input's with weight c = ``lam`` * sim[b]: p <- (p + c q) / (1 + c), so the row stays normalised.  A commit with
    sim < ``min_sim`` is searched as if it had no neighbour.  Values are checked here (``ValueError`` with the reason);
    ``check`` holds the value against a batch."""
    db: DeviceBatch
    sim: object
    lam: float = 1.0
    min_sim: float = 0.0

    MAX_LAMBDA = 1024.0

    def __post_init__(self):
        import numpy as np
        if not hasattr(self.db, "B") or not hasattr(self.db, "struct"):
            raise ValueError("Neighbour: db = %r is not a DeviceBatch" % (self.db,))
        for name, hi in (("lam", self.MAX_LAMBDA), ("min_sim", float("inf"))):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError("Neighbour: %s = %r is not a number" % (name, v))
            if not 0 <= v <= hi:                              # (also refuses nan)
                raise ValueError("Neighbour: %s = %r outside [0, %g]" % (name, v, hi))
            object.__setattr__(self, name, float(v))
        sim = self.sim
        if torch.is_tensor(sim):
            sim = sim.detach().cpu().tolist()
        try:
            sim = np.array([float(x) for x in sim], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("Neighbour: sim = %r is not a sequence of numbers" % (self.sim,)) from None
        if sim.shape != (self.db.B,):
            raise ValueError("Neighbour: %d similarities for a neighbour batch of %d commits" % (sim.size, self.db.B))
        if not (np.isfinite(sim).all() and (sim >= 0).all() and (sim <= 1).all()):
            raise ValueError("Neighbour: sim = %s holds a value outside [0, 1]" % (sim.tolist(),))
        object.__setattr__(self, "sim", sim)

    def check(self, B: int) -> "Neighbour":
        if self.db.B != B:
            raise ValueError("Neighbour: a neighbour batch of %d commits for a batch of %d" % (self.db.B, B))
        return self

    def coef(self):
        return neighbour_coef(self.sim, self.lam, self.min_sim)


class _NeighbourWs:
    """What ``Searcher._begin`` hands to ``Searcher._step`` for a search with a neighbour in place of the one decode workspace:
    the input's workspace, the neighbour batch's, the [R, out_len] buffer of the neighbour's distribution, the device
    coefficients and the neighbour's id rows (static buffers, filled on every call: one capture serves every batch)."""

    def __init__(self, ws, ws_n, R, B, cfg, dev):
        self.ws, self.ws_n = ws, ws_n
        self.q = torch.zeros((R, cfg.out_len), dtype=torch.float32, device=dev)
        self.coef = torch.zeros((B, 2), dtype=torch.float32, device=dev)
        self.sou = torch.zeros((B, cfg.sou_len), dtype=torch.int32, device=dev)
        self.sub = torch.zeros((B, max(cfg.sub_token_len, 1)), dtype=torch.int32, device=dev)


@dataclasses.dataclass(frozen=True, eq=False)
class KnnMT:
    """Token-level retrieval (kNN-MT): ``store`` is a ``retrieve.TokenStore``.  At every step the row's
    last hidden state (``fira_decode_hidden``) is looked up among the stored keys (``fira_knn_search``: the ``k`` nearest by
    squared distance, ties to the lower row), and the words that followed there are mixed into the row's distribution
    (``fira_mix_knn``): p <- (1 - ``lam``) p, then p[value_k] += ``lam`` w_k with w = softmax(-d2 / ``temperature``) over the
    slots found.  ``exclude``: per commit of the batch an owner (commit index of the store) whose rows are left out, e.g. the
    commit itself when it is in the store; None or -1: nothing.  ``check`` refuses a wrong value before anything is launched;
    ``lam == 0`` is the search without the option."""
    store: object
    k: int = 8
    lam: float = 0.3
    temperature: float = 10.0
    exclude: object = None

    MAX_K = 16                                   # fira_knn_search: 1 <= K <= 16
    WIDTH = 256

    @property
    def active(self) -> bool:
        return self.lam != 0

    def check(self, B: Optional[int] = None) -> "KnnMT":
        if isinstance(self.k, bool) or not isinstance(self.k, numbers.Integral) or not 1 <= self.k <= self.MAX_K:
            raise ValueError("KnnMT: k = %r outside 1..%d" % (self.k, self.MAX_K))
        for name in ("lam", "temperature"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError("KnnMT: %s = %r is not a number" % (name, v))
        if not 0 <= self.lam <= 1:                            # (also refuses nan)
            raise ValueError("KnnMT: lam = %r outside [0, 1]" % (self.lam,))
        if not 0 < self.temperature < float("inf"):
            raise ValueError("KnnMT: temperature = %r must be finite and > 0" % (self.temperature,))
        keys = getattr(self.store, "keys", None)
        if keys is None or not all(hasattr(self.store, f) for f in ("key_sq", "values", "owner", "N")):
            raise ValueError("KnnMT: store = %r is not a retrieve.TokenStore" % (self.store,))
        if self.store.N < 1 or keys.shape[0] < 1:
            raise ValueError("KnnMT: the store is empty")
        if keys.dim() != 2 or keys.shape[1] != self.WIDTH:
            raise ValueError("KnnMT: the store's keys are %s, expected [N, %d]" % (tuple(keys.shape), self.WIDTH))
        if self.exclude is not None:
            ex = self.exclude_rows()
            if B is not None and len(ex) != B:
                raise ValueError("KnnMT: %d exclude values for a batch of %d commits" % (len(ex), B))
        return self

    def exclude_rows(self) -> List[int]:
        try:
            ex = self.exclude.tolist() if hasattr(self.exclude, "tolist") else list(self.exclude)
            return [-1 if e is None else int(e) for e in ex]
        except (TypeError, ValueError):
            raise ValueError("KnnMT: exclude = %r is not a sequence of commit indices" % (self.exclude,)) from None

    def coef(self):
        """(lam, 1 / temperature) as the float32 pair ``fira_mix_knn`` reads from the device."""
        import numpy as np
        return np.array([self.lam, 1.0 / float(self.temperature)], dtype=np.float64).astype(np.float32)


class _KnnWs:
    """What ``Searcher._begin`` hands to ``Searcher._step`` for a search with ``knn=`` in place of the one decode workspace:
    the workspace, the store, and the static buffers of the three extra launches -- the hidden rows [R, 256], the slots found
    idx / d2 [R, K], the search's scratch, and the device values filled on every call (coef [2], exclude [R]: one capture serves
    every lam, temperature and exclude list)."""

    def __init__(self, ws, store, R, K, dev):
        self.ws, self.store, self.K = ws, store, K
        self.hidden = torch.zeros((R, KnnMT.WIDTH), dtype=torch.float32, device=dev)
        self.idx = torch.full((R, K), -1, dtype=torch.int32, device=dev)
        self.d2 = torch.full((R, K), float("inf"), dtype=torch.float32, device=dev)
        self.coef = torch.zeros(2, dtype=torch.float32, device=dev)
        self.exclude = torch.full((R,), -1, dtype=torch.int32, device=dev)
        need = _lib.lib().fira_knn_search_scratch_bytes(R, store.N, K)
        if need == 0:
            raise ValueError("knn: fira_knn_search takes no store of %d rows with K = %d" % (store.N, K))
        self.scratch = torch.empty(need, dtype=torch.uint8, device=dev)


def rank_values(scores, by: str) -> torch.Tensor:
    """The [B, n] values ``Searcher.rank`` orders candidates by (larger is better)."""
    if by == "mean_logp_word":
        return scores["logp_word"] / (scores["length"] - 1).clamp(min=1).to(scores["logp_word"].dtype)
    return scores[by]


# ---------------------------------------------------------------------- the options of a search: refusing, checking, resolving
# The class of every option a search takes by keyword, and what a search that does not take it says (``_refuse``).
_OPTION = {"constraints": Constraints, "penalties": Penalties, "phrases": Phrases, "template": Template, "wordsets": WordSets,
           "neighbour": Neighbour, "knn": KnnMT}
_REFUSAL = {"penalties": "%s does not take penalties (%s); greedy, greedy_many, beam and sample_search do",
            "phrases": "%s does not take phrases (greedy, greedy_many, beam and sample_search take banned phrases, beam "
                       "required ones)",
            "template": "%s does not take a template (greedy, greedy_many, beam and sample_search do)",
            "wordsets": "%s does not take word sets (greedy, greedy_many, beam and sample_search do)",
            "neighbour": "%s does not combine with a neighbour (greedy, greedy_many and beam do)",
            "knn": "%s does not combine with knn= (greedy, greedy_many, beam and sample_search do)"}


def _given(option: str, value, check=None, check_first: bool = False):
    """What every option checker begins with: None for "off" -- no value, or an inactive one: today's launches, buffers and
    graphs -- else the value, held against ``check`` (the arguments of its ``.check``) when that is given.  A value of another
    type is a ``ValueError``.  ``check_first``: ``.check`` runs before ``active`` is read (``knn``: a wrong value is refused
    even where ``lam == 0`` would switch it off)."""
    if value is None:
        return None
    if not isinstance(value, _OPTION[option]):
        raise ValueError("%s: expected decode.%s or None, got %r" % (option, _OPTION[option].__name__, value))
    if check_first:
        value.check(*check)
    if not getattr(value, "active", True):
        return None
    return value if check is None or check_first else value.check(*check)


def _refuse(what: str, option: str, value, why: Optional[str] = None):
    """For the search ``what``, which does not take ``option``: None and an inactive value pass, an active one and a value of
    the wrong type are refused with the option's text (``why``: the reason it names, for ``penalties``).  A neighbour has no
    inactive value; ``knn`` names a wrong type as its checker does and is checked before ``active`` is read."""
    if option == "knn":
        value = _given(option, value, (), check_first=True)
    if value is not None and (not isinstance(value, _OPTION[option]) or getattr(value, "active", True)):
        raise ValueError(_REFUSAL[option] % ((what,) if why is None else (what, why)))


def _refuse_each(what: str, why: Optional[str], **values):
    """``_refuse`` for every ``option=value`` given, in that order; ``why`` is the reason a refusal of ``penalties`` names."""
    for option, value in values.items():
        _refuse(what, option, value, why if option == "penalties" else None)


def _refuses(*options, why: Optional[str] = None):
    """For a search whose published signature stays as it is: each keyword named here is taken for one purpose only, to refuse
    it (``_refuse_each``), in the order given, before the search itself is entered; it is not handed on."""
    def wrap(search):
        @functools.wraps(search)
        def refusing(self, *args, **kwargs):
            _refuse_each(search.__name__, why, **{option: kwargs.pop(option, None) for option in options})
            return search(self, *args, **kwargs)
        return refusing
    return wrap


@dataclasses.dataclass(frozen=True)
class _Part:
    """One row of ``_PARTS``: what one option of a search adds to its key, its state and its launches.

    ``on``: the resolved value of an ``_Options`` record that turns the part on (None or False: off).  ``key``: value -> the
    part's components of the state key (default: its name in the table, a marker).  ``flag``: value -> what the state holds
    under the part's name (None: no such entry, or one of ``entries``).  ``entries``: (name, dtype, shape(q, value)) of every
    device buffer the part owns in a state, q having ``cfg``, ``B`` and ``R`` -- or value -> such a tuple.  ``arrays``:
    (options, value, batch) -> the host values of the leading entries, in their order, copied in on every call (one capture
    serves every value).  ``call``: for a link of the edit chain, its library entry; it gets the stream, the dims, R, the rows
    per commit, ``gen`` / ``length`` (``rows``), sou, sub, then ``args(st)`` (default: the entries' pointers in their order),
    the distribution and the best pair."""
    on: object
    key: object = None
    flag: object = None
    entries: object = ()
    arrays: object = None
    call: Optional[str] = None
    args: object = None
    rows: bool = True

    def entries_of(self, value):
        return self.entries(value) if callable(self.entries) else self.entries


_I32, _F32 = torch.int32, torch.float32
_PER_COMMIT = lambda q, v: (q.B,)
_PER_ROW = lambda q, v: (q.R,)
_MARK = lambda v: True
_WST = ("allow", "deny", "boost", "ground", "slot_valid", "boost_factor")      # fira_wordset_dist's pointers, in its order


def _padded(rows, width: int):
    """(ids [len(rows), width] int32 zero-padded, lengths [len(rows)] int32) of checked id lists, on the host."""
    host = torch.zeros((len(rows), width), dtype=torch.int32)
    for b, row in enumerate(rows):
        host[b, :len(row)] = torch.tensor(row, dtype=torch.int32)
    return host, torch.tensor([len(row) for row in rows], dtype=torch.int32)


def _slot_words(cfg) -> int:
    return max((cfg.sou_len + cfg.sub_token_len + 31) // 32, 1)


def _wordset_entries(wst: WordSets):
    """One [B, ceil(vocab / 32)] bit set for each set the value gives, the valid slots [B, ceil(slots / 32)] with ``ground`` and
    the factors [B] with ``boost``."""
    shape = {"slot_valid": lambda q, v: (q.B, _slot_words(q.cfg)), "boost_factor": _PER_COMMIT}
    need = wst.given + (("slot_valid",) if "ground" in wst.given else ()) + (("boost_factor",) if "boost" in wst.given else ())
    return tuple(("wst_" + name, _F32 if name == "boost_factor" else _I32,
                  shape.get(name, lambda q, v: (q.B, (q.cfg.vocab_size + 31) // 32))) for name in _WST if name in need)


def _wordset_arrays(o, wst: WordSets, db: DeviceBatch):
    """The checked sets, and the valid copy slots of the batch: slot j is valid iff its source id is not <pad> (0) -- the rule
    by which ``fira_decode_begin`` forms the copy head's mask (mem_valid), so a slot is valid here exactly where the step can
    give it mass."""
    a = wst.arrays(db.B, o.cfg.vocab_size)
    if "ground" in wst.given:
        ids = torch.cat([db.sou, db.sub_token], 1) if o.cfg.sub_token_len else db.sou
        n = _slot_words(o.cfg) * 32
        valid = torch.zeros((db.B, n), dtype=torch.int64, device=ids.device)
        valid[:, :ids.shape[1]] = ids != PAD
        words = (valid.view(db.B, n // 32, 32) << torch.arange(32, device=ids.device)).sum(-1)
        a["slot_valid"] = torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)
    return [a[name[len("wst_"):]] for name, _, _ in _wordset_entries(wst)]


# Every part of a search that an option switches on.  First the links of the edit chain, IN THE ORDER ``Searcher._edit`` issues
# them (its docstring says why the order is what it is); then the parts that are no edit: the selections of ``beam`` (required
# words, required items, a scoring) and the second distribution mixed in by ``Searcher._step`` (a neighbour, knn=).
_PARTS = {
    "merge": _Part(lambda o: o.merge, flag=_MARK, call="fira_merge_dist", rows=False),
    "prefix": _Part(lambda o: o.rows, entries=(("prefix", _I32, lambda q, v: (q.B, q.cfg.tar_len)), ("prefix_len", _I32, _PER_COMMIT)),
                    arrays=lambda o, rows, db: _padded(rows, o.cfg.tar_len), call="fira_force_dist"),
    "con": _Part(lambda o: o.con, key=lambda c: (c,), entries=(("banned", _I32, lambda q, c: (max(len(c.banned), 1),)),),
                 arrays=lambda o, c, db: (torch.tensor(list(c.banned) or [0], dtype=torch.int32),), call="fira_constrain_dist",
                 args=lambda st: (st["con"].no_repeat_ngram, st["con"].min_length, _lib.ptr(st["banned"]), len(st["con"].banned))),
    "ban-phrases": _Part(lambda o: o.ban, flag=_MARK, call="fira_ban_phrases_dist",
                         entries=(("ban_phrase", _I32, lambda q, v: (q.B, Phrases.MAX_BANNED, Phrases.MAX_WORDS)),
                                  ("ban_phrase_len", _I32, lambda q, v: (q.B, Phrases.MAX_BANNED)), ("n_ban_phrases", _I32, _PER_COMMIT)),
                         arrays=lambda o, ban, db: ban.banned_arrays(db.B)),
    "template": _Part(lambda o: o.tpl, flag=_MARK, call="fira_template_dist",
                      entries=(("tpl_word_class", torch.uint8, lambda q, v: (q.cfg.vocab_size,)),
                               ("tpl_next", torch.int8, lambda q, v: (Template.MAX_STATES * Template.MAX_CLASSES,)),
                               ("tpl_need", _I32, lambda q, v: (Template.MAX_STATES,)), ("tpl_start", _I32, _PER_COMMIT)),
                      arrays=lambda o, tpl, db: tpl.arrays(db.B, o.cfg.vocab_size)),
    "wordsets": _Part(lambda o: o.wst, key=lambda wst: (("wordsets", tuple(wst.given)),), flag=lambda wst: wst.given,
                      entries=_wordset_entries, arrays=_wordset_arrays, call="fira_wordset_dist",
                      args=lambda st: [_lib.ptr(st["wst_" + name]) if "wst_" + name in st else None for name in _WST]),
    "penalties": _Part(lambda o: o.pen, flag=_MARK, call="fira_penalise_dist",
                       entries=(("count_factor", _F32, lambda q, v: (q.cfg.tar_len,)),
                                ("bias_id", _I32, lambda q, v: (q.B, Penalties.MAX_BIASED)),
                                ("bias_factor", _F32, lambda q, v: (q.B, Penalties.MAX_BIASED)), ("n_bias", _I32, _PER_COMMIT)),
                       arrays=lambda o, pen, db: (pen.table(o.cfg.tar_len),) + tuple(pen.bias_arrays(db.B))),
    "require": _Part(lambda o: o.words, entries=(("required", _I32, lambda q, v: (q.B, MAX_REQUIRED)),
                                                 ("n_required", _I32, _PER_COMMIT), ("met", _I32, _PER_ROW)),
                     arrays=lambda o, words, db: _padded(words, MAX_REQUIRED)),
    "require-phrases": _Part(lambda o: o.items, flag=_MARK,
                             entries=(("item_words", _I32, lambda q, v: (q.B, Phrases.MAX_REQUIRED_WORDS)),
                                      ("item_len", _I32, lambda q, v: (q.B, Phrases.MAX_ITEMS)), ("n_items", _I32, _PER_COMMIT),
                                      ("met", _I32, _PER_ROW)),
                             arrays=lambda o, items, db: items.required_arrays(db.B)),
    "scoring": _Part(lambda o: o.scoring, key=lambda sc: (sc,), flag=lambda sc: sc,
                     entries=(("inv_lp", _F32, lambda q, v: (q.cfg.tar_len + 1,)), ("key", _F32, _PER_ROW)),
                     arrays=lambda o, sc, db: (torch.tensor(sc.inv_lp(o.cfg.tar_len), dtype=torch.float64).to(torch.float32),)),
    "neighbour": _Part(lambda o: o.nb),
    "knn": _Part(lambda o: o.kn, key=lambda kn: (("knn", kn.k, id(kn.store)),)),
}
_CHAIN = tuple((name, part) for name, part in _PARTS.items() if part.call is not None)
# The order of the key's components -- the order in which the options came to the searches, which the states in use are keyed
# by -- and of the fills.
_KEY_ORDER = ("merge", "prefix", "require", "neighbour", "knn", "penalties", "ban-phrases", "require-phrases", "template",
              "wordsets", "con", "scoring")
assert sorted(_KEY_ORDER) == sorted(_PARTS)


def _state_key(base, on):
    """``base`` and, in ``_KEY_ORDER``, the key components of every part that ``on`` (name -> value; None or False: off) has
    on: see ``Searcher._key``."""
    return base + tuple(c for name in _KEY_ORDER if on.get(name) is not None and on[name] is not False
                        for c in ((name,) if _PARTS[name].key is None else _PARTS[name].key(on[name])))


@dataclasses.dataclass(frozen=True, eq=False)
class _Options:
    """The resolved options of one search over one batch (``Searcher._options``): the checked values, each None (``merge``:
    False) where the option is off -- no value, an inactive one, an all-empty prefix.  It launches nothing and allocates
    nothing until ``state`` / ``fill`` are called; what it answers, it reads from ``_PARTS``."""
    search: "Searcher"
    con: Optional[Constraints] = None
    merge: bool = False
    rows: Optional[list] = None                  # the checked prefix
    words: Optional[list] = None                 # the checked required words
    nb: Optional[Neighbour] = None
    kn: Optional[KnnMT] = None
    pen: Optional[Penalties] = None
    ban: Optional[Phrases] = None                # the Phrases value, where it bans phrases
    items: Optional[Phrases] = None              # the Phrases value, where it requires items
    tpl: Optional[Template] = None
    wst: Optional[WordSets] = None
    scoring: Optional[BeamScoring] = None

    cfg = property(lambda self: self.search.cfg)

    def on(self, names=_KEY_ORDER):
        """(name, part, value) of every part that is on, in the order of ``names``."""
        parts = [(name, _PARTS[name], _PARTS[name].on(self)) for name in names]
        return [(name, part, value) for name, part, value in parts if value is not None and value is not False]

    @property
    def mixer(self):
        """The ``Neighbour``, the ``KnnMT`` or None: what ``Searcher._begin`` / ``_step`` mix a second distribution in from."""
        return self.nb if self.kn is None else self.kn

    @property
    def edits(self) -> bool:
        """Whether any link of the edit chain is on: the state then owns the distribution the chain edits."""
        return bool(self.on([name for name, _ in _CHAIN]))

    def key(self, base):
        """The state key of the search (``Searcher._key``)."""
        return _state_key(base, {name: value for name, _, value in self.on()})

    def state(self, i32, f32, R: int, B: int, dist: bool = False):
        """What the options own in a state of R rows over B commits: ``con`` always (None: no constraint), the flag and the
        entries of every part that is on, and the [R, out_len] distribution with any link of the edit chain (``dist=True``: in
        any case -- the beam family and the samplers, whose selection reads it, and a search that mixes a second one in)."""
        q = types.SimpleNamespace(cfg=self.cfg, B=B, R=R)
        st = dict(con=self.con)
        for name, part, value in self.on():
            if part.flag is not None:
                st[name] = part.flag(value)
            for entry, dtype, shape in part.entries_of(value):
                if dtype in (_I32, _F32):
                    st[entry] = (i32 if dtype is _I32 else f32)(*shape(q, value))
                else:
                    st[entry] = torch.zeros(shape(q, value), dtype=dtype, device=self.search.model.device_)
        if dist or self.edits:
            st["dist"] = f32(R, self.cfg.out_len)
        return st

    def fill(self, st, db: DeviceBatch):
        """The checked values into the state's device buffers -- on every call, the way ``Searcher._state`` fills sou / sub."""
        for _, part, value in self.on():
            if part.arrays is not None:
                for (entry, _, _), a in zip(part.entries_of(value), part.arrays(self, value, db)):
                    st[entry].copy_(a if torch.is_tensor(a) else torch.from_numpy(a.view("int32") if a.dtype == "uint32" else a))


class _Loop:
    """The chunked step loop of one search over one batch, on the current stream.

    Creating it runs the encoder pass (``Searcher._begin``) and finds or builds the search's static state under ``key`` (see
    ``Searcher._state``); the search then fills in its own inputs and calls ``start`` with its ``steps(lo, hi)``, its
    ``reset()`` and, if it can end early, its ``stop(hi)`` (evaluated on the host after the chunk that ended at step ``hi``:
    the one read-back between chunks).  ``n_steps`` is the number of steps the loop needs when the host knows it (default: all
    tar_len - 1): chunks that begin at or after it are not run, and eager launches trim the last chunk to it (a captured chunk
    is replayed whole).  ``launch`` / ``done`` are one turn of the loop, so a caller can keep several loops in flight; ``run``
    is all turns of one.

    The graphs live in the state (``st["graphs"]``: None before capture, then one object with ``.replay()`` per chunk) beside
    the ``chunk`` and the ``bounds`` they were captured with: a graph call with another ``chunk`` is refused, since the captured
    chunks would not match its bounds.  Eager calls take any ``chunk``."""

    def __init__(self, search: "Searcher", db: DeviceBatch, rows: int, key, make, chunk: int, use_graphs: bool, mixer=None):
        st = search._ws.get(key)
        if use_graphs and st is not None and st["graphs"] is not None and st["chunk"] != chunk:
            raise ValueError("chunk = %d, but the graphs of %r were captured with chunk = %d (use_graphs=False takes any chunk)"
                             % (chunk, key, st["chunk"]))
        self.T, self.chunk, self.use_graphs = search.cfg.tar_len, chunk, use_graphs
        self.ws = search._begin(db, rows) if mixer is None else search._begin(db, rows, mixer)
        self.st = search._state(key, db, make)

    def start(self, steps, reset, stop=None, n_steps: Optional[int] = None):
        st, T = self.st, self.T
        self.steps, self.stop = steps, stop
        self.n_steps = T - 1 if n_steps is None else n_steps
        reset()
        if self.use_graphs and st["graphs"] is not None:
            self.bounds = st["bounds"]
        else:
            self.bounds = [(lo, min(lo + self.chunk, T - 1)) for lo in range(0, T - 1, self.chunk)]
            if self.use_graphs:
                # warm-up outside capture (lazy initialisation inside the library / torch), then capture every chunk
                steps(0, 1)
                torch.cuda.synchronize()
                # No destructor of a device object may run inside a capture: destroying a captured graph or freeing its memory
                # there makes the runtime abort the process.  Reference counting frees nothing of that kind in ``steps``, but
                # the cyclic collector may start at any allocation and free a dead cycle that owns graphs and buffers (torch
                # no longer collects when a capture begins).  So: collect now, and keep the collector off while capturing.
                gc.collect()
                gc_was_on = gc.isenabled()
                gc.disable()
                graphs = []
                try:
                    for lo, hi in self.bounds:
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            steps(lo, hi)
                        graphs.append(g)
                finally:
                    if gc_was_on:
                        gc.enable()
                st.update(graphs=graphs, chunk=self.chunk, bounds=self.bounds)
                reset()
        self.n = sum(lo < self.n_steps for lo, _ in self.bounds)      # chunks this loop runs at most
        self.i = self.hi = 0                                           # next chunk; end of the last step run
        return self

    def launch(self):
        """Enqueue the next chunk of steps: one hipGraph replay, or the eager calls."""
        lo, hi = self.bounds[self.i]
        if self.use_graphs:
            self.st["graphs"][self.i].replay()
        else:
            hi = min(hi, self.n_steps)
            self.steps(lo, hi)
        self.hi = hi

    def done(self) -> bool:
        """After the chunk launched last: advance, and only if chunks remain evaluate the stop test (which synchronises with
        that chunk); nothing is read back after the final chunk."""
        self.i += 1
        return self.i >= self.n or (self.stop is not None and self.stop(self.hi))

    def run(self):
        done = self.n == 0
        while not done:
            self.launch()
            done = self.done()
        return self.st


class Searcher:
    """The searches over one model (or an ensemble).  ``greedy`` / ``greedy_many``, ``beam`` and ``sample_search`` take seven options
    that edit the step's distribution before a word is chosen (``sample_distinct`` takes the first two); ``_options`` resolves
    them into one ``_Options`` record, ``_PARTS`` says what each adds to the key, the state and the launches, and ``_edit`` issues
    their kernels, in the order merge, prefix, constraints, banned phrases, template, word sets, penalties.  Each is off by
    default, and off -- None, False, an inactive value, an all-empty prefix -- means the calls, keys, buffers and graphs of a
    search without it.

    ``constraints``: a ``Constraints`` value.  ``fira_constrain_dist`` zeroes the blocked words' entries of every row between
    the step and the selection; nothing is renormalised (greedy: probability = the product of the UNnormalised entries taken).
    The value joins the state key: its scalars are baked into the captured launches.

    ``merge_copies``: search over WORDS instead of entries.  ``fira_merge_dist`` folds every copy entry into the generator entry
    of the word it resolves to, so a word is one candidate however many entries carry it: greedy takes the most probable word,
    not the largest single entry, and the beam's slots of positive probability hold pairwise distinct word sequences.  The
    returned probability is then the probability of the WORD SEQUENCE: the sum over every entry path that spells it -- exact,
    because the next step depends on the resolved ids only -- and no longer the product of the entries taken.  "merge" joins the
    state key (``_key``), so merged and unmerged searches own separate buffers and graphs.

    ``prefix``: how every message begins -- a sequence of B sequences of vocabulary ids in [UNK, vocab), without <start>, at most
    tar_len - 2 long; an empty one means no prefix for that commit.  While a hypothesis (every running row of every beam group)
    is inside its commit's prefix, ``fira_force_dist`` zeroes every entry of the step's distribution that does not resolve to the
    prefix word, so the search can only take that word -- through its generator entry or a copy slot -- and then continues
    freely: each hypothesis of positive probability starts with the prefix.  The returned probability is the JOINT probability
    of prefix and continuation (nothing is divided out; the ranking within a commit is unaffected).  ``merge_copies`` is
    recommended with a prefix: without it the forced word's mass stays split over its entries; greedy takes the largest one
    and the beam may spend slots on several of them, exactly as it does on unforced steps.  The state is keyed by a "prefix"
    marker, not by the values (device buffers read when the kernels run: one capture serves every prefix).  A ``ValueError``
    before anything is launched on a wrong count, a non-integer id, an id outside [UNK, vocab), a prefix that is too long, or --
    with ``constraints`` -- one that holds a banned id or itself repeats an n-gram.

    ``penalties``: a ``Penalties`` value -- presence and frequency penalties on the words a hypothesis already holds (prefix words
    count as emitted) and a per-word bias.  ``fira_penalise_dist`` multiplies the words' entries by their factors, last in the
    chain: a finite non-negative factor commutes bit for bit with the zeroing links, and after a merge a word's mass sits on its
    generator entry.  The value a search then returns is the product of the EDITED entries taken: a score, not a probability
    (``score`` gives the model's probability of a message).  The state is keyed by a "penalties" marker, not by the values (the
    table and the bias lists are device buffers, filled on every call: one capture serves every value).  ``sample``, ``score``,
    ``sample_distinct`` and ``contrastive`` refuse an active value with a ``ValueError`` before anything is launched.

    ``phrases``: a ``Phrases`` value.  Its banned phrases are the chain's fourth link: ``fira_ban_phrases_dist`` zeroes the entries of
    the word that would complete a listed phrase.  Its required items are no edit but a selection (``fira_beam_select_phrases``), and
    ``beam`` alone takes them.  The state is keyed by the markers "ban-phrases" / "require-phrases" (the lists are device buffers,
    filled on every call).  ``sample``, ``score``, ``sample_distinct`` and ``contrastive`` refuse an active value.

    ``template``: a ``Template`` value, the chain's fifth link: ``fira_template_dist`` zeroes the entries of every word after which
    the automaton accepts no message that still fits, and <eos> where it does not accept, so a message of positive probability
    is one the automaton accepts.  The state is keyed by a "template" marker (the four tables are device buffers, filled on every
    call).  It does not combine with required words or items; ``sample``, ``score``, ``sample_distinct`` and ``contrastive``
    refuse an active value.

    ``wordsets``: a ``WordSets`` value, the chain's sixth link: ``fira_wordset_dist`` zeroes the entries of every word its
    ``allow``, ``deny`` and ``ground`` sets block for the row's commit and multiplies the entries of the ``boost`` words.  The state
    is keyed by a ("wordsets", names of the given sets) marker (the sets are device buffers, filled on every call; which of them
    a launch gets is part of a captured graph).  ``sample``, ``score``, ``sample_distinct`` and ``contrastive`` refuse an active
    value."""

    def __init__(self, model: TransModel, kv_bf16: bool = False, members=(), weights=None):
        """``kv_bf16``: stream a bf16 copy of the cross-attention K|V in the step loop (FIRA_DECODE_KV_BF16: half of the
        bytes a step moves; ids no longer bit-identical to the fp32 search -- off by default).

        ``members``: further ``TransModel`` instances of the same geometry on the same device.  ``greedy`` / ``greedy_many`` /
        ``beam`` then search under the linear mix of the models' step distributions (``fira_mix_dist``):
        p = w_0 p_0 + w_1 p_1 + ..., ``model`` being member 0.  ``weights``: one value per model, the primary first (default
        uniform; given weights are normalised to sum 1: ``ensemble_weights``).  With ``members == ()`` nothing changes."""
        self.model = model
        self.cfg = model.cfg
        self.flags = 1 if kv_bf16 else 0
        self._ws = {}
        self.members = tuple(members)
        models = (model,) + self.members
        if len(models) > MAX_MODELS:
            raise ValueError("members: %d models in all, more than %d" % (len(models), MAX_MODELS))
        for k, m in enumerate(self.members, 1):
            if not isinstance(m, TransModel):
                raise ValueError("members: member %d is %r, not a TransModel" % (k, type(m).__name__))
            for name, _ in _lib.Dims._fields_:
                if getattr(m.dims, name) != getattr(model.dims, name):
                    raise ValueError("members: member %d has %s = %d, the primary %d (every member has the primary's geometry)"
                                     % (k, name, getattr(m.dims, name), getattr(model.dims, name)))
            if m.device_ != model.device_:
                raise ValueError("members: member %d is on %s, the primary on %s" % (k, m.device_, model.device_))
        if not self.members and weights is not None:
            ensemble_weights(weights, 1)                      # (one model: only the count and the values can be wrong)
        self.weights = ensemble_weights(weights, len(models)) if self.members else None

    def _lane(self) -> "Searcher":
        """A second Searcher over the same models (its own workspaces, states and graphs) for a lane of ``greedy_many``."""
        lane = Searcher(self.model, kv_bf16=bool(self.flags), members=self.members)
        lane.weights = self.weights                           # the very float32 values: normalising twice may move a bit
        return lane

    def _edit_state(self, i32, f32, R, B, con, merge, rows, dist=False, pen=None, ban=None, tpl=None, wst=None):
        """``_Options.state`` for checked values given one by one (the searches hold a record and ask it)."""
        return _Options(self, con=con, merge=bool(merge), rows=rows, pen=pen, ban=ban, tpl=tpl, wst=wst).state(i32, f32, R, B, dist)

    def _no_ensemble(self, what: str):
        if self.members:
            raise ValueError("%s does not combine with an ensemble (its fused step has no distribution hand-off)" % what)

    def _workspace(self, B, beam, model=None, key=None):
        model = self.model if model is None else model
        key = (B, beam) if key is None else key
        if key not in self._ws:
            n = _lib.lib().fira_decode_workspace_bytes_ex(C.byref(model.dims), B, beam, self.flags)
            if n == 0:
                _lib.check(1, "fira_decode_workspace_bytes")
            self._ws[key] = torch.empty(n, dtype=torch.uint8, device=model.device_)
        return self._ws[key]

    def _begin_model(self, model, ws, db, beam):
        _lib.check(_lib.lib().fira_decode_begin_ex(_lib.cur_stream(), C.byref(model.dims), C.byref(db.struct),
                                                   _lib.ptr(model.flat.data), _lib.ptr(ws), ws.numel(), beam,
                                                   self.flags), "fira_decode_begin")

    def _begin(self, db, beam, neighbour=None):
        ws = self._workspace(db.B, beam)
        self.model.sync_params()
        db.wait_ready()
        self._begin_model(self.model, ws, db, beam)
        if isinstance(neighbour, KnnMT):
            # knn= (never with members or a neighbour): the static buffers of the three extra launches, keyed by the store
            # and K, and the per-call values into the device buffers the captured launches read
            kn, R = neighbour, db.B * beam
            key = ("knn", db.B, beam, kn.k, id(kn.store))
            if key not in self._ws:
                self._ws[key] = _KnnWs(ws, kn.store, R, kn.k, self.model.device_)
            kw = self._ws[key]
            kw.coef.copy_(torch.from_numpy(kn.coef()))
            ex = [-1] * db.B if kn.exclude is None else kn.exclude_rows()
            kw.exclude.copy_(torch.tensor(ex, dtype=torch.int32).repeat_interleave(beam))
            return kw
        if neighbour is not None:
            # a neighbour (never with members): a second workspace of the one model for the neighbour batch, its encoder pass on
            # the current stream, and the per-batch values into the static buffers the captured launches read
            key = ("neighbours", db.B, beam)
            if key not in self._ws:
                self._ws[key] = _NeighbourWs(ws, self._workspace(db.B, beam, key=("neighbour", db.B, beam)), db.B * beam, db.B,
                                             self.cfg, self.model.device_)
            nb = self._ws[key]
            neighbour.db.wait_ready()
            self._begin_model(self.model, nb.ws_n, neighbour.db, beam)
            nb.coef.copy_(torch.from_numpy(neighbour.coef()))
            nb.sou.copy_(neighbour.db.sou)
            if self.cfg.sub_token_len:
                nb.sub.copy_(neighbour.db.sub_token)
            return nb
        if not self.members:
            return ws
        # an ensemble: one workspace (the primary's under today's key) and one distribution buffer per member; the encoder pass
        # of every member on the current stream, in member order, all of them reading the one ``db``
        key = ("members", db.B, beam)
        if key not in self._ws:
            wss = [ws] + [self._workspace(db.B, beam, m, ("member", k, db.B, beam)) for k, m in enumerate(self.members, 1)]
            dist = [torch.zeros((db.B * beam, self.cfg.out_len), dtype=torch.float32, device=self.model.device_) for _ in wss]
            self._ws[key] = _Members(wss, dist, self.weights)
        mem = self._ws[key]
        for model, w in zip(self.members, mem.ws[1:]):
            model.sync_params()
            self._begin_model(model, w, db, beam)
        return mem

    def _step_model(self, model, ws, B, beam, step, tokens, parent, dist, best_id, best_p):
        _lib.check(_lib.lib().fira_decode_step_ex(_lib.cur_stream(), C.byref(model.dims),
                                                  _lib.ptr(model.flat.data), _lib.ptr(ws), ws.numel(), B, beam, step,
                                                  _lib.ptr(tokens), _lib.ptr(parent), _lib.ptr(dist), _lib.ptr(best_id),
                                                  _lib.ptr(best_p), self.flags), "fira_decode_step")

    def _step(self, ws, B, beam, step, tokens, parent, dist, best_id, best_p):
        if isinstance(ws, _KnnWs):
            # knn= (``ws`` is the _KnnWs of ``_begin``): the model's step into the search's ``dist``, the rows' hidden states,
            # their K nearest stored rows, then the mix in place over ``dist`` -- which also delivers best_id / best_p
            lib, s, dims, st, R = _lib.lib(), _lib.cur_stream(), C.byref(self.model.dims), ws.store, B * beam
            self._step_model(self.model, ws.ws, B, beam, step, tokens, parent, dist, None, None)
            _lib.check(lib.fira_decode_hidden(s, dims, _lib.ptr(ws.ws), ws.ws.numel(), B, beam, self.flags, _lib.ptr(ws.hidden)),
                       "fira_decode_hidden")
            _lib.check(lib.fira_knn_search(s, _lib.ptr(ws.hidden), R, _lib.ptr(st.keys), _lib.ptr(st.key_sq), _lib.ptr(st.owner),
                                           _lib.ptr(ws.exclude), st.N, ws.K, _lib.ptr(ws.idx), _lib.ptr(ws.d2),
                                           _lib.ptr(ws.scratch), ws.scratch.numel()), "fira_knn_search")
            return _lib.check(lib.fira_mix_knn(s, dims, R, _lib.ptr(ws.idx), _lib.ptr(ws.d2), _lib.ptr(st.values), st.N, ws.K,
                                               _lib.ptr(ws.coef), _lib.ptr(dist), _lib.ptr(best_id), _lib.ptr(best_p)),
                              "fira_mix_knn")
        if isinstance(ws, _NeighbourWs):
            # a neighbour (``ws`` is the _NeighbourWs of ``_begin``): the input's step into the search's ``dist``, the same
            # model's step over the neighbour batch with the same tokens and parents into ``ws.q``, the neighbour's row folded
            # into words with the NEIGHBOUR's ids, then the mix in place over ``dist`` -- which also delivers best_id / best_p
            lib, s, dims = _lib.lib(), _lib.cur_stream(), C.byref(self.model.dims)
            self._step_model(self.model, ws.ws, B, beam, step, tokens, parent, dist, None, None)
            self._step_model(self.model, ws.ws_n, B, beam, step, tokens, parent, ws.q, None, None)
            _lib.check(lib.fira_merge_dist(s, dims, B * beam, beam, _lib.ptr(ws.sou), _lib.ptr(ws.sub), _lib.ptr(ws.q), None, None),
                       "fira_merge_dist")
            return _lib.check(lib.fira_mix_neighbour(s, dims, B * beam, beam, _lib.ptr(ws.coef), _lib.ptr(ws.q), _lib.ptr(dist),
                                                     _lib.ptr(best_id), _lib.ptr(best_p)), "fira_mix_neighbour")
        if not self.members:
            return self._step_model(self.model, ws, B, beam, step, tokens, parent, dist, best_id, best_p)
        # an ensemble (``ws`` is the _Members of ``_begin``): every member's step with the same tokens and parents into its own
        # buffer, then one fira_mix_dist into the caller's ``dist`` -- or, for a search that asks for the arg-max only, in place
        # over member 0's buffer -- which also delivers best_id / best_p
        for model, w, d in zip((self.model,) + self.members, ws.ws, ws.dist):
            self._step_model(model, w, B, beam, step, tokens, parent, d, None, None)
        out = ws.dist[0] if dist is None else dist
        _lib.check(_lib.lib().fira_mix_dist(_lib.cur_stream(), B * beam, self.cfg.out_len, len(ws.dist), ws.ptrs, ws.weights,
                                            _lib.ptr(out), _lib.ptr(best_id), _lib.ptr(best_p)), "fira_mix_dist")

    def _active(self, constraints: Optional[Constraints]) -> Optional[Constraints]:
        """None for "no constraint" (None or an inactive value: today's launches, buffers and graphs), else the checked value."""
        return _given("constraints", constraints, (self.cfg,))

    def _penalties(self, penalties, B: int) -> Optional[Penalties]:
        """None for "no penalties" (None or an inactive value: today's launches, buffers and graphs), else the value checked
        against the model and the batch; raises before any launch."""
        return _given("penalties", penalties, (self.cfg, B))

    def _phrases(self, phrases, B: int, con: Optional[Constraints], what: str, prefix_rows=None, beam: Optional[int] = None,
                 require=None, scoring=None):
        """(ban, req) of a search: each None for "none" (no value, or nothing in it: today's launches, buffers and graphs), else the
        ``Phrases`` value checked against the model, the batch and the search's other options.  ``beam`` None: a search that has
        no banks and refuses required items.  Raises ``ValueError`` naming the reason; nothing is launched before."""
        phrases = _given("phrases", phrases, (self.cfg, B))
        if phrases is None:
            return None, None
        cfg = self.cfg
        ban = phrases if phrases.ban_active else None
        req = phrases if phrases.require_active else None
        banned = phrases.banned_rows(B)
        if ban is not None and prefix_rows is not None:
            for b, row in enumerate(prefix_rows):
                for ph in banned[b]:
                    if contains_phrase(row, ph):
                        raise ValueError("phrases: commit %d: the prefix contains the banned phrase %r" % (b, ph))
        if req is None:
            return ban, None
        if beam is None:
            raise ValueError("phrases: %s does not take required items (banks need a beam; beam does)" % what)
        if require is not None:
            raise ValueError("phrases: required items do not combine with require= (a one-word item is a required word)")
        if scoring is not None:
            raise ValueError("phrases: required items do not combine with an active scoring (the banks rank by raw probability)")
        if beam < 2:
            raise ValueError("phrases: beam = %d, but required items need a beam of at least 2" % beam)
        for b, row in enumerate(phrases.required):
            total = sum(len(item) for item in row)
            if beam < total + 1:
                raise ValueError("phrases: commit %d: %d required words need a beam of at least %d (one bank per word of "
                                 "progress), beam = %d" % (b, total, total + 1, beam))
            if total > cfg.tar_len - 2:
                raise ValueError("phrases: commit %d: %d required words, more than tar_len - 2 = %d" % (b, total, cfg.tar_len - 2))
            for item in row:
                if con is not None:
                    hit = sorted(set(item) & set(con.banned))
                    if hit:
                        raise ValueError("phrases: commit %d: the required item %r holds id %d, which the constraints ban"
                                         % (b, item, hit[0]))
                    n = con.no_repeat_ngram
                    grams = [item[i:i + n] for i in range(len(item) - n + 1)] if n >= 1 else []
                    if len(set(grams)) != len(grams):
                        raise ValueError("phrases: commit %d: the required item %r itself repeats a %d-gram, which "
                                         "no_repeat_ngram = %d forbids" % (b, item, n, n))
                for ph in banned[b]:
                    if contains_phrase(item, ph):
                        raise ValueError("phrases: commit %d: the required item %r contains the banned phrase %r" % (b, item, ph))
        return ban, req

    def _template(self, template, B: int, con: Optional[Constraints], prefix_rows=None, require=None, items=None):
        """None for "no template" (None or the inactive value: today's launches, buffers and graphs), else the ``Template`` value
        checked against the model, the batch and the search's other options: ``prefix_rows`` (the checked prefix), ``con``,
        ``require`` (the checked required words) and ``items`` (a ``Phrases`` value with required items).  Raises ``ValueError``
        naming the reason; nothing is launched before.  What cannot be seen in advance -- a state that admits only words another
        control blocks at that step -- gives the hypothesis probability 0: a zero simply loses."""
        template = _given("template", template, (self.cfg, B))
        if template is None:
            return None
        T = self.cfg.tar_len
        if require is not None or items is not None:
            raise ValueError("template: does not combine with require= or Phrases(required=) (their <eos> rule and the "
                             "template's can leave a row with nothing, and the banks would need the automaton)")
        starts = template.start_rows(B)
        for b, row in enumerate(prefix_rows or ()):
            s = template.walk(row, starts[b])
            if s < 0:
                raise ValueError("template: commit %d: the prefix is not a path of the automaton from state %d" % (b, starts[b]))
            if template.need[s] > T - 1 - len(row):
                raise ValueError("template: commit %d: after the prefix of %d words no accepted message fits into the "
                                 "remaining %d words" % (b, len(row), T - 1 - len(row)))
        if con is not None and con.min_length:
            for b, s in enumerate(starts):
                if not template.longest_fits(s, con.min_length, T - 1):
                    raise ValueError("template: commit %d: no accepted message has at least min_length = %d words within "
                                     "tar_len - 1 = %d" % (b, con.min_length, T - 1))
        return template

    def _wordsets(self, wordsets, B: int, prefix_rows=None, require=None, items=None):
        """None for "no word sets" (None or an inactive value: today's launches, buffers and graphs), else the ``WordSets`` value
        checked against the model, the batch and the search's other options: no word of ``prefix_rows`` (the checked prefix),
        of ``require`` (the checked required words) or of ``items`` (a ``Phrases`` value with required items) may be one that
        ``allow`` or ``deny`` blocks.  Raises ``ValueError`` naming the reason; nothing is launched before.  What the host cannot
        see -- a forced or required word that ``ground`` blocks because the commit does not carry it, a ``Template`` state
        reachable only through blocked words -- leaves the hypothesis probability 0."""
        wordsets = _given("wordsets", wordsets, (self.cfg, B))
        if wordsets is None:
            return None
        item_rows = None if items is None else [[w for item in row for w in item] for row in items.required]
        for what, rows in (("prefix", prefix_rows), ("required", require), ("required phrase", item_rows)):
            for b, row in enumerate(rows or ()):
                for w in row:
                    if wordsets.blocks(w, b, B):
                        raise ValueError("wordsets: commit %d: the %s word %d is blocked by allow or deny" % (b, what, w))
        return wordsets

    def _neighbour(self, neighbour, B: int):
        """None for "no neighbour" (today's launches, buffers and graphs), else the checked value; raises before any launch."""
        if _given("neighbour", neighbour) is None:
            return None
        if self.members:
            raise ValueError("neighbour: does not combine with an ensemble (members)")
        return neighbour.check(B)

    def _knn(self, knn, B: int, neighbour=None):
        """None for "no retrieval" (None, or ``lam == 0``: today's launches, buffers and graphs), else the checked value; raises
        before any launch."""
        knn = _given("knn", knn, (B,), check_first=True)
        if knn is None:
            return None
        if self.members:
            raise ValueError("knn: does not combine with an ensemble (members)")
        if neighbour is not None:
            raise ValueError("knn: does not combine with a neighbour")
        have, want = knn.store.keys.device, torch.device(self.model.device_)
        if have.type != want.type or (have.index is not None and want.index is not None and have.index != want.index):
            raise ValueError("knn: the store is on %s, the model on %s" % (knn.store.keys.device, self.model.device_))
        return knn

    def _edit(self, st, R, rows_per_commit, gen, length, best):
        """The edit chain: the kernels that edit the step's distribution st["dist"] ([R, out_len], ``rows_per_commit`` rows per
        commit) between the decoder step and the selection, for whatever the state ``st`` carries: the links of ``_PARTS`` that
        the state has on, in the table's order.  Each link reads its buffers from the state when its kernel runs (``_Part``).
        Why the order is what it is:

        merge: ``fira_merge_dist`` folds every copy entry into the generator entry of the word it resolves to (DESIGN.md
        section 6l).  Words first: a blocked word's mass then sits on its generator entry.
        force: ``fira_force_dist`` leaves the rows still inside their commit's prefix the entries of the prefix word only
        (section 6q); ``gen`` / ``length`` say where a row is.
        constrain: ``fira_constrain_dist`` zeroes the blocked words' entries (section 6k); nothing is renormalised.  Its scalars
        are baked into a captured graph.
        ban phrases: ``fira_ban_phrases_dist`` zeroes the entries of the word that would complete a banned phrase (section 6zb).
        template: ``fira_template_dist`` zeroes the entries of the words the automaton does not admit after the row's hypothesis,
        and <eos> where it does not accept (section 6zc).
        word sets: ``fira_wordset_dist`` zeroes the entries of the words the commit's allow / deny / ground sets block and
        multiplies the entries of its boost set (section 6zd).  After the other hard edits, before the soft one: its one
        multiplication is the last of its own edits.  It gets the sets the state owns and NULL for the rest.
        penalise: ``fira_penalise_dist`` multiplies the entries of the words a row already holds, and of the commit's biased
        words, by their factors (section 6za).  Last: a finite non-negative factor commutes bit for bit with the zeroing links,
        and after a merge a word's mass sits on its generator entry.

        ``best``: (best_id, best_p) or None.  The last kernel that edits the distribution takes the arg-max of what is left: a
        pair goes to the last call the chain makes, every other call gets NULL for both (greedy); None: NULL for all (the beam
        family, whose selection reads the distribution itself).  This is the one place that knows that rule."""
        lib, s, dims = _lib.lib(), _lib.cur_stream(), C.byref(self.model.dims)
        sou, sub, dist = _lib.ptr(st["sou"]), _lib.ptr(st["sub"]), _lib.ptr(st["dist"])
        chain = [part for name, part in _CHAIN if st.get(name) is not None]
        for part in chain:
            where = (_lib.ptr(gen), _lib.ptr(length)) if part.rows else ()
            args = [_lib.ptr(st[entry]) for entry, _, _ in part.entries] if part.args is None else part.args(st)
            last = (_lib.ptr(best[0]), _lib.ptr(best[1])) if best is not None and part is chain[-1] else (None, None)
            _lib.check(getattr(lib, part.call)(s, dims, R, rows_per_commit, *where, sou, sub, *args, dist, *last), part.call)

    def _prefix_rows(self, prefix, B: int, con: Optional[Constraints]):
        """None for "no prefix" (None, or every sequence empty: today's launches, buffers and graphs), else the checked prefix as
        B lists of vocabulary ids.  Raises ``ValueError`` naming the commit and the reason; nothing is launched before."""
        if prefix is None:
            return None
        cfg = self.cfg
        try:
            rows = [list(p) for p in prefix]
        except TypeError:
            raise ValueError("prefix: expected one sequence of vocabulary ids per commit, got %r" % (prefix,)) from None
        if len(rows) != B:
            raise ValueError("prefix: %d sequences for a batch of %d commits" % (len(rows), B))
        for b, row in enumerate(rows):
            for w in row:
                if isinstance(w, bool) or not isinstance(w, numbers.Integral):
                    raise ValueError("prefix: commit %d: id %r is not an integer" % (b, w))
                if not UNK <= w < cfg.vocab_size:
                    raise ValueError("prefix: commit %d: id %d outside [%d, %d) (<pad>, <eos> and <start> cannot be forced)"
                                     % (b, w, UNK, cfg.vocab_size))
            rows[b] = row = [int(w) for w in row]
            if len(row) > cfg.tar_len - 2:
                raise ValueError("prefix: commit %d: %d words, more than tar_len - 2 = %d" % (b, len(row), cfg.tar_len - 2))
            if con is not None:                               # the constraint kernel would zero the forced word: an all-zero row
                hit = sorted(set(row) & set(con.banned))
                if hit:
                    raise ValueError("prefix: commit %d: id %d is banned by the constraints" % (b, hit[0]))
                n = con.no_repeat_ngram
                grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)] if n >= 1 else []
                if len(set(grams)) != len(grams):
                    raise ValueError("prefix: commit %d: the prefix itself repeats a %d-gram, which no_repeat_ngram = %d forbids"
                                     % (b, n, n))
        return rows if any(rows) else None

    @staticmethod
    def _key(base, merge: bool, con, scoring=None, forced: bool = False, *, require: bool = False, neighbour: bool = False,
             penalties: bool = False, ban_phrases: bool = False, require_phrases: bool = False, template: bool = False,
             wordsets=(), knn=None):
        """The state key of a search, from flags (the searches themselves ask their ``_Options`` record: ``_Options.key``; both
        read ``_state_key``): ``base``, then the component of every part that is on, in ``_KEY_ORDER`` -- "merge" (merged and
        unmerged searches own separate buffers and graphs), "prefix", "require", "neighbour", ("knn", K, the store), "penalties",
        "ban-phrases", "require-phrases", "template", ("wordsets", the names of the sets given), the ``Constraints`` value, the
        ``BeamScoring`` value.  A marker stands for values that live in device buffers, filled on every call: one capture
        serves all of them.  What a captured launch bakes in is in the key itself: the scalars of the constraints and of the
        scoring, K, N and the store's pointers of ``knn=`` (lam, the temperature and the exclude list are device values), and
        which set pointers a word-set launch gets.  Off -- False, None, () -- adds nothing: today's key."""
        given = types.SimpleNamespace(given=wordsets) if wordsets else None
        return _state_key(base, {"merge": merge, "prefix": forced, "require": require, "neighbour": neighbour, "knn": knn,
                                 "penalties": penalties, "ban-phrases": ban_phrases, "require-phrases": require_phrases,
                                 "template": template, "wordsets": given, "con": con, "scoring": scoring})

    def _options(self, what: str, db_or_B, *, beam: Optional[int] = None, scoring=None, constraints=None,
                 merge_copies: bool = False, prefix=None, require=None, neighbour=None, penalties=None, phrases=None,
                 template=None, wordsets=None, knn=None) -> _Options:
        """The options of the search ``what`` over a batch (or its size), checked against the model, the batch and one another
        in the one order every search has had -- constraints, scoring, prefix, required words, neighbour, knn, penalties,
        phrases, template, word sets -- and resolved into a record.  ``beam``: None for a search without one, which takes
        neither a scoring nor required words or items.  Raises ``ValueError`` naming the reason; nothing is launched or
        allocated here."""
        B = db_or_B if isinstance(db_or_B, int) else db_or_B.B
        con = self._active(constraints)
        if scoring is not None:
            if not isinstance(scoring, BeamScoring):
                raise ValueError("scoring: expected decode.BeamScoring or None, got %r" % (scoring,))
            scoring = scoring.check(beam) if scoring.active() or beam < 2 else None
        rows = self._prefix_rows(prefix, B, con)
        words = self._required_rows(require, B, beam, con, scoring)
        nb = self._neighbour(neighbour, B)
        kn = self._knn(knn, B, nb)
        pen = self._penalties(penalties, B)
        ban, items = self._phrases(phrases, B, con, what, rows, beam, words, scoring)
        tpl = self._template(template, B, con, rows, words, items)
        wst = self._wordsets(wordsets, B, rows, words, items)
        return _Options(self, con, bool(merge_copies), rows, words, nb, kn, pen, ban, items, tpl, wst, scoring)

    def _required_rows(self, require, B: int, beam: int, con: Optional[Constraints], scoring):
        """None for "no required words" (None, or every sequence empty: today's launches, buffers and graphs), else the checked
        words as B lists of vocabulary ids.  Raises ``ValueError`` naming the commit and the reason; nothing is launched before."""
        if require is None:
            return None
        cfg = self.cfg
        try:
            rows = [list(p) for p in require]
        except TypeError:
            raise ValueError("require: expected one sequence of vocabulary ids per commit, got %r" % (require,)) from None
        if len(rows) != B:
            raise ValueError("require: %d sequences for a batch of %d commits" % (len(rows), B))
        for b, row in enumerate(rows):
            for w in row:
                if isinstance(w, bool) or not isinstance(w, numbers.Integral):
                    raise ValueError("require: commit %d: id %r is not an integer" % (b, w))
                if not UNK < w < cfg.vocab_size:
                    raise ValueError("require: commit %d: id %d outside (%d, %d) (<pad>, <eos>, <start> and <unkm> cannot be "
                                     "required)" % (b, w, UNK, cfg.vocab_size))
            rows[b] = row = [int(w) for w in row]
            if len(set(row)) != len(row):
                raise ValueError("require: commit %d: id %d is listed twice" % (b, next(w for w in row if row.count(w) > 1)))
            if len(row) > MAX_REQUIRED:
                raise ValueError("require: commit %d: %d words, more than %d" % (b, len(row), MAX_REQUIRED))
        if not any(rows):
            return None
        if beam < 2:
            raise ValueError("require: beam = %d, but required words need a beam of at least 2" % beam)
        for b, row in enumerate(rows):
            if beam < len(row) + 1:
                raise ValueError("require: commit %d: %d words need a beam of at least %d (one bank per count of words met), "
                                 "beam = %d" % (b, len(row), len(row) + 1, beam))
            if len(row) > cfg.tar_len - 2:
                raise ValueError("require: commit %d: %d words, more than tar_len - 2 = %d" % (b, len(row), cfg.tar_len - 2))
            if con is not None:
                hit = sorted(set(row) & set(con.banned))
                if hit:
                    raise ValueError("require: commit %d: id %d is banned by the constraints" % (b, hit[0]))
        if scoring is not None:
            raise ValueError("require: required words do not combine with an active scoring (the banks rank by raw probability)")
        return rows

    @staticmethod
    def _sbs_key(B: int, n: int, merge: bool, con, temperature: float):
        """The state key of ``sample_distinct``: fixed positions (the merge flag and the Constraints value or None as they are),
        and the temperature last -- it is baked into the captured launches."""
        return ("sbs", B, n, merge, con, temperature)

    def _state(self, key, db: DeviceBatch, make):
        """The static device buffers of one search loop (its captured hipGraphs live beside them), built on first use as
        ``make(i32, f32)`` (zero-filled int32 / float32 allocators) plus what every search has: the commits' ``sou`` /
        ``sub`` id rows, which are filled from ``db`` here, and ``graphs`` = None until ``_Loop`` captures."""
        st = self._ws.get(key)
        if st is None:
            cfg, dev = self.cfg, self.model.device_
            i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
            f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
            # (a geometry without sub-token slots: one zero column, so that the kernels never get a null pointer -- no entry of
            #  the distribution resolves to a sub-token then, and the row stride they use is the geometry's, 0)
            st = self._ws[key] = dict(make(i32, f32), sou=i32(db.B, cfg.sou_len), sub=i32(db.B, max(cfg.sub_token_len, 1)),
                                      graphs=None)
        st["sou"].copy_(db.sou)
        if self.cfg.sub_token_len:
            st["sub"].copy_(db.sub_token)
        return st

    def _hypothesis_rows(self, i32, f32, R):
        """The per-row state of ``fira_greedy_advance`` / ``fira_sample_advance`` over R rows."""
        return dict(out=i32(R, self.cfg.tar_len), length=i32(R), prob=f32(R), alive=i32(R), tok=i32(R),
                    n_alive=i32(self.cfg.tar_len), best_id=i32(R), best_p=f32(R))

    def _beam_rows(self, i32, f32, R):
        """The per-row state of ``fira_beam_prepare`` and the selections over R rows; ``gen`` / ``length`` are ping-pong pairs."""
        T = self.cfg.tar_len
        return dict(gen=[i32(R, T), i32(R, T)], length=[i32(R), i32(R)], tok=i32(R), parent=i32(R), fin=i32(R), active=i32(9),
                    done=i32(1))

    def _noise(self, keys, seed, B: int):
        """The noise inputs of ``sample`` / ``sample_distinct``: checks ``keys`` (default: the commit's row in the batch) now, before
        anything is launched; returns (the state's entries for ``make``, ``fill(st)`` that writes keys and seed into them)."""
        keys = torch.arange(B) if keys is None else torch.as_tensor(keys)
        if keys.numel() != B:
            raise ValueError("keys: %d values for a batch of %d commits" % (keys.numel(), B))

        def fill(st):
            st["key"].copy_(keys.reshape(B).to(torch.int32))
            bits = int(seed) & 0xFFFFFFFFFFFFFFFF
            st["seed"].fill_(bits - (1 << 64) if bits >= 1 << 63 else bits)     # the uint64 bits in an int64 tensor
        rows = lambda i32: dict(key=i32(B), seed=torch.zeros(1, dtype=torch.int64, device=self.model.device_))
        return rows, fill

    # ------------------------------------------------------------------ greedy (beam 1): no sort, no dist tensor
    def _greedy_reset(self, st):
        st["out"].zero_()
        st["out"][:, 0] = START
        st["length"].fill_(1)
        st["prob"].fill_(1.0)
        st["alive"].fill_(1)
        st["tok"].fill_(START)
        st["n_alive"].zero_()

    def _greedy_steps(self, st, ws, B, lo, hi):
        """Steps lo..hi-1 of run_model.py:225-340 at beam 1: two library calls per step (KV-cached decoder step with the
        arg-max of the output distribution, then the hypothesis bookkeeping), no torch op, no host round trip.  A state with
        edits (it owns ``dist``): the step writes the distribution instead and the edit chain reports the arg-max."""
        lib, s = _lib.lib(), _lib.cur_stream()
        for step in range(lo, hi):
            if "dist" not in st:
                self._step(ws, B, 1, step, st["tok"], None, None, st["best_id"], st["best_p"])
            elif st.get("mix_best", False):                   # a neighbour and an empty edit chain: the mix takes the arg-max
                self._step(ws, B, 1, step, st["tok"], None, st["dist"], st["best_id"], st["best_p"])
            else:
                self._step(ws, B, 1, step, st["tok"], None, st["dist"], None, None)
                self._edit(st, B, 1, st["out"], st["length"], (st["best_id"], st["best_p"]))
            _lib.check(lib.fira_greedy_advance(s, C.byref(self.model.dims), B, step, _lib.ptr(st["best_id"]),
                                               _lib.ptr(st["best_p"]), _lib.ptr(st["sou"]), _lib.ptr(st["sub"]),
                                               _lib.ptr(st["out"]), _lib.ptr(st["length"]), _lib.ptr(st["prob"]),
                                               _lib.ptr(st["alive"]), _lib.ptr(st["tok"]), _lib.ptr(st["n_alive"])),
                       "fira_greedy_advance")

    def _greedy_loop(self, db: DeviceBatch, chunk: int, use_graphs: bool, opts: _Options) -> _Loop:
        """Encoder pass + reset of the hypothesis state for one batch on the CURRENT stream; returns the started loop.  The
        options that are on join the key (``_key``, over the base ("greedy", B)), and so own their graphs, and add what
        ``_Options.state`` lists to the state -- the [B, out_len] distribution with any link of the edit chain, and always with a
        neighbour or knn=, whose mix takes the arg-max itself ("mix_best") where the chain is empty."""
        B = db.B
        mixed = opts.mixer is not None
        make = lambda i32, f32: dict(self._hypothesis_rows(i32, f32, B), **({"mix_best": True} if mixed and not opts.edits else {}),
                                     **opts.state(i32, f32, B, B, dist=mixed))
        loop = _Loop(self, db, 1, opts.key(("greedy", B)), make, chunk, use_graphs, opts.mixer)
        st, ws = loop.st, loop.ws
        opts.fill(st, db)
        return loop.start(lambda lo, hi: self._greedy_steps(st, ws, B, lo, hi), lambda: self._greedy_reset(st),
                          lambda hi: self._none_alive(st, hi))

    @staticmethod
    def _none_alive(st, hi) -> bool:
        """Stop test of greedy and sample: every hypothesis has emitted <eos> by step hi - 1 (run_model.py:276-279)."""
        return int(st["n_alive"][hi - 1].item()) == 0

    @staticmethod
    def _greedy_result(st):
        return st["out"].long(), st["length"].long(), st["prob"].clone()

    @torch.no_grad()
    def greedy(self, db: DeviceBatch, chunk: int = 5, use_graphs: bool = True, constraints: Optional[Constraints] = None,
               merge_copies: bool = False, prefix=None, neighbour: Optional[Neighbour] = None,
               penalties: Optional[Penalties] = None, phrases: Optional[Phrases] = None,
               template: Optional[Template] = None, wordsets: Optional[WordSets] = None, knn: Optional[KnnMT] = None):
        """Returns (tokens [B,T] int64 starting with <start>, lengths [B], probability [B]).  ``constraints``, ``merge_copies``,
        ``prefix`` and ``penalties`` are the class's options: with any of them the step writes its distribution instead of taking
        its fused arg-max, and the last kernel of the edit chain (``_edit``) takes the arg-max of what is left.  With active
        ``penalties`` the third tensor is the product of the edited entries taken -- a score, not a probability (``score`` gives
        the model's probability of a message).  ``phrases``: a ``Phrases`` value with banned phrases (a link of the edit chain
        after the constraints; "ban-phrases" joins the state key); required items are refused, they need a beam's banks.
        ``template``: a ``Template`` value, a link of the edit chain after the banned phrases ("template"
        joins the state key; the tables are device buffers, one capture for every template).  A message of positive probability
        is then accepted by the automaton.  A ``ValueError`` before anything is launched on what ``Template.check`` and
        ``_template`` refuse: a prefix that is no path of the automaton or leaves no room, a ``min_length`` no accepted message
        reaches.  A state that admits only words another control blocks leaves the hypothesis probability 0.
        ``wordsets``: a ``WordSets`` value, a link of the edit chain after the template (("wordsets",
        names of the given sets) joins the state key; the sets are device buffers, one capture for every value that gives the
        same sets).  No word its ``allow``, ``deny`` or ``ground`` blocks is then written by a message of positive probability.
        With an active ``boost`` the third tensor is a score, as under ``penalties``.  A ``ValueError`` before anything is launched
        on what ``WordSets.check`` and ``_wordsets`` refuse, a prefix word that ``allow`` or ``deny`` blocks among them; a word
        ``ground`` blocks because the commit does not carry it leaves probability 0.

        ``neighbour``: a ``Neighbour`` value.  Every step then also runs the model over the neighbour
        batch on the same tokens (a second workspace), folds that row into words with the neighbour's ids and mixes it into the
        input's row (``fira_mix_neighbour``) ahead of the edit chain; the returned probability is the product of the mixed
        entries taken.  It combines with the three options above; the state gains a "neighbour" key component and always owns
        a distribution.  A ``ValueError`` before anything is launched on a wrong value or an ensemble.

        ``knn``: a ``KnnMT`` value.  Every step then also takes the rows' last hidden states
        (``fira_decode_hidden``), finds their K nearest rows in the token store (``fira_knn_search``) and mixes the words that
        followed there into the step's distribution (``fira_mix_knn``) ahead of the edit chain; the returned probability is the
        product of the mixed entries taken.  ("knn", K, the store) joins the state key; lam, the temperature and the exclude
        list are device values.  None or ``lam == 0``: the search without it.  A ``ValueError`` before anything is launched on
        what ``KnnMT.check`` refuses, an ensemble or a neighbour.

        The step loop is launch-bound (~58 small kernels per generated token), so it is captured once per batch size
        into hipGraphs of ``chunk`` steps each and replayed; between chunks one counter is read back to stop as soon
        as every hypothesis has emitted <eos> (run_model.py:276-279)."""
        opts = self._options("greedy", db, constraints=constraints, merge_copies=merge_copies, prefix=prefix,
                             neighbour=neighbour, penalties=penalties, phrases=phrases, template=template, wordsets=wordsets,
                             knn=knn)                       # raises before anything is launched
        return self._greedy_result(self._greedy_loop(db, chunk, use_graphs, opts).run())

    @staticmethod
    def _per_batch(name: str, value, n: int, expected: str, one=None, unit: str = "values"):
        """An argument of ``greedy_many`` as a list of one value per batch: None -- or, for an option with a class ``one``, a
        single value -- stands for every batch; otherwise a sequence as long as the batches."""
        if value is None or (one is not None and isinstance(value, one)):
            return [value] * n
        try:
            value = list(value)
        except TypeError:
            raise ValueError("%s: expected %s, got %r" % (name, expected, value)) from None
        if len(value) != n:
            raise ValueError("%s: %d %s for %d batches" % (name, len(value), unit, n))
        return value

    @torch.no_grad()
    def greedy_many(self, dbs, in_flight: int = 4, chunk: int = 5, constraints: Optional[Constraints] = None,
                    merge_copies: bool = False, prefix=None, neighbour=None, penalties: Optional[Penalties] = None,
                    phrases: Optional[Phrases] = None, template: Optional[Template] = None, wordsets=None, knn=None):
        """Greedy search over a sequence of batches with ``in_flight`` of them on the GPU at once, each on its own stream
        (its own workspace, hypothesis state and captured graphs); results are returned in the order of ``dbs``.

        One decode step is ~58 dependent launches of 16-48 workgroups each: a single batch of 64 keeps a fraction of the 256
        CUs busy and the loop is bound by the launch chain, not by the chip.  The reference walks the test set batch after
        batch (run_model.py:225); nothing couples two batches, so independent chains share the chip.  HIP multiplexes the
        lanes' streams onto GPU_MAX_HW_QUEUES hardware queues: on the default 4, three lanes gave x1.7 step-tokens/s and four fell
        BELOW one lane (x0.8) once the process had created more streams (a trainer's) -- two lanes on one queue run one after
        the other.  On 8 queues (run_model.py / bench.py / this package set GPU_MAX_HW_QUEUES=8 before HIP initialises) three
        lanes give x2.06 and four x2.35 in a process that trained first; six collapse again (profiles/r6_probes.md).
        Same arithmetic, same ids as ``greedy`` batch by batch, ``constraints`` and ``merge_copies`` included (with
        ``merge_copies`` the probability is that of the word sequence, summed over every entry path that spells it).
        ``prefix``: one prefix argument of ``greedy`` per batch (a sequence as long as ``dbs``; an entry may be None); the
        returned probability is then the joint probability of prefix and continuation.
        ``neighbour``: one ``Neighbour`` (or None) per batch, a sequence as long as ``dbs``.
        ``penalties``: one ``Penalties`` value for every batch (a per-commit bias list then needs batches of one size); the
        returned value is then a score, as for ``greedy``.
        ``phrases``: one ``Phrases`` value with banned phrases for every batch (per-commit lists then need batches of one
        size), as for ``greedy``.
        ``template``: one ``Template`` value for every batch (per-commit start states then need batches of one size), as for
        ``greedy``.
        ``wordsets``: one ``WordSets`` value for every batch, or a sequence of one value (or None) per batch, as for ``greedy``.
        ``knn``: one ``KnnMT`` value for every batch (an exclude list then needs batches of one size), or a sequence of one value
        (or None) per batch, as for ``greedy``."""
        dbs = list(dbs)
        self._active(constraints)                            # (even for no batch at all)
        knn = self._per_batch("knn", knn, len(dbs), "decode.KnnMT, None or one of them per batch", KnnMT)
        wordsets = self._per_batch("wordsets", wordsets, len(dbs), "decode.WordSets, None or one of them per batch", WordSets)
        neighbour = self._per_batch("neighbour", neighbour, len(dbs), "one Neighbour per batch")
        prefix = self._per_batch("prefix", prefix, len(dbs), "one prefix argument per batch", unit="prefix arguments")
        # every batch's options, resolved before a lane starts: every refusal comes before the first device call
        opts = [self._options("greedy_many", db, constraints=constraints, merge_copies=merge_copies, prefix=p, neighbour=nb,
                              penalties=penalties, phrases=phrases, template=template, wordsets=w, knn=kn)
                for db, p, nb, w, kn in zip(dbs, prefix, neighbour, wordsets, knn)]
        n_lane = max(1, min(in_flight, len(dbs)))
        if not hasattr(self, "_lanes") or len(self._lanes) < n_lane:
            streams = concurrent_streams(n_lane, self.model.device_)
            old = getattr(self, "_lanes", [])
            # (lane 0 is this Searcher, kept as None: a reference to itself would make it a cycle that only the cyclic
            # collector frees, graphs and buffers included)
            self._lanes = [(old[k][0] if k < len(old) else (self._lane() if k else None),
                            streams[k]) for k in range(n_lane)]
        main = torch.cuda.current_stream()
        results = [None] * len(dbs)
        active = [None] * n_lane                                # per lane: (batch index, loop)
        nxt = 0
        for lane, stream in self._lanes[:n_lane]:
            stream.wait_stream(main)
        while True:
            busy = False
            for k in range(n_lane):
                lane, stream = self._lanes[k]
                lane = self if lane is None else lane
                with torch.cuda.stream(stream):
                    if active[k] is not None:
                        j, loop = active[k]
                        if loop.done():                         # (synchronises with this lane's last chunk only)
                            results[j] = self._greedy_result(loop.st)
                            for r_ in results[j]:
                                r_.record_stream(main)          # allocated on the lane's stream, consumed on the caller's
                            active[k] = None
                        else:
                            loop.launch()
                    if active[k] is None and nxt < len(dbs):
                        loop = lane._greedy_loop(dbs[nxt], chunk, True, opts[nxt])
                        loop.launch()
                        active[k] = (nxt, loop)
                        nxt += 1
                busy = busy or active[k] is not None
            if not busy:
                break
        for lane, stream in self._lanes[:n_lane]:
            main.wait_stream(stream)
        return results

    # ------------------------------------------------------------------ sampling: temperature / top-k / top-p, n per commit
    def _sample_reset(self, st):
        self._greedy_reset(st)
        st["logp"].zero_()

    CUTS_OFF = (0.0, 0.0, 0.0, 1.0)                           # (min_p, epsilon, eta, typical_p)

    @staticmethod
    def _check_cuts(top_p, min_p, epsilon, eta, typical_p):
        """The four truncation cuts of ``sample`` as the floats the library receives; raises ValueError naming the argument
        on a value outside its range (nan included) or a combination the library refuses."""
        f32 = lambda v: C.c_float(float(v)).value
        cuts = tuple(f32(v) for v in (min_p, epsilon, eta, typical_p))
        for name, v in zip(("min_p", "epsilon", "eta"), cuts):
            if not 0 <= v < 1:
                raise ValueError("%s %r: must be in [0, 1) (0 = off)" % (name, v))
        if not 0 < cuts[3] <= 1:
            raise ValueError("typical_p %r: must be in (0, 1] (1 = off)" % cuts[3])
        if cuts[3] < 1:
            for name, v, off in (("top_p", f32(top_p), 1.0), ("min_p", cuts[0], 0.0), ("epsilon", cuts[1], 0.0),
                                 ("eta", cuts[2], 0.0)):
                if v != off:
                    raise ValueError("typical_p %r keeps a band of the distribution, not its head: it does not combine "
                                     "with %s %r" % (cuts[3], name, v))
        return cuts

    def _sample_steps(self, st, ws, B, n, lo, hi, temperature, top_k, top_p, cuts=CUTS_OFF):
        """Steps lo..hi-1: the KV-cached decoder step with the sampling kernel in place of the arg-max, then the bookkeeping
        of greedy search over the B * n rows (plus the log-probability sum); no torch op, no host round trip."""
        lib, s = _lib.lib(), _lib.cur_stream()
        for step in range(lo, hi):
            if cuts == self.CUTS_OFF:
                _lib.check(lib.fira_decode_step_sample(s, C.byref(self.model.dims), _lib.ptr(self.model.flat.data), _lib.ptr(ws),
                                                       ws.numel(), B, n, step, _lib.ptr(st["tok"]), _lib.ptr(st["key"]),
                                                       _lib.ptr(st["seed"]), float(temperature), int(top_k), float(top_p), None,
                                                       _lib.ptr(st["best_id"]), _lib.ptr(st["best_p"]), self.flags),
                           "fira_decode_step_sample")
            else:
                _lib.check(lib.fira_decode_step_sample_cut(s, C.byref(self.model.dims), _lib.ptr(self.model.flat.data),
                                                           _lib.ptr(ws), ws.numel(), B, n, step, _lib.ptr(st["tok"]),
                                                           _lib.ptr(st["key"]), _lib.ptr(st["seed"]), float(temperature),
                                                           int(top_k), float(top_p), *cuts, None, _lib.ptr(st["best_id"]),
                                                           _lib.ptr(st["best_p"]), self.flags),
                           "fira_decode_step_sample_cut")
            _lib.check(lib.fira_sample_advance(s, C.byref(self.model.dims), B, n, step, _lib.ptr(st["best_id"]),
                                               _lib.ptr(st["best_p"]), _lib.ptr(st["sou"]), _lib.ptr(st["sub"]),
                                               _lib.ptr(st["out"]), _lib.ptr(st["length"]), _lib.ptr(st["prob"]),
                                               _lib.ptr(st["logp"]), _lib.ptr(st["alive"]), _lib.ptr(st["tok"]),
                                               _lib.ptr(st["n_alive"])), "fira_sample_advance")

    @_refuses("knn", "wordsets")
    @torch.no_grad()
    def sample(self, db: DeviceBatch, n: int, *, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
               keys=None, chunk: int = 5, use_graphs: bool = True, neighbour=None, min_p: float = 0.0, epsilon: float = 0.0,
               eta: float = 0.0, typical_p: float = 1.0, penalties=None, phrases=None, template=None):
        """``n`` sampled messages per commit.  Returns (tokens [B,n,T] int64 starting with <start>, lengths [B,n],
        probability [B,n], log-probability [B,n]); the probabilities are the model's (untempered, unfiltered) ones of the
        emitted ids.

        Truncation cuts on top of the filters, on q = the tempered distribution renormalised over what top-k and top-p kept
        (``fira_decode_step_sample_cut``): ``min_p`` keeps q >= min_p * max q, ``epsilon`` keeps q >= epsilon, ``eta`` keeps
        q >= min(eta, sqrt(eta) * exp(-H)) with H the entropy of q (each in [0, 1), ``0`` = off), ``typical_p`` keeps the
        entries whose surprise is nearest H until they hold that share of the mass (in (0, 1], ``1`` = off; with temperature
        and top-k only).  Every cut keeps the row's maximum.  With all four off this is the call and the state of the plain
        sampler; otherwise the four values join the state's key, since they too are fixed in the captured launches.

        Filters in the order of HF ``generate``: temperature, then top-k (``0`` = off), then top-p (``1`` = off); the draw is a
        Gumbel-max over the kept entries with counter-hash noise of (``seed``, ``keys[b]``, sample, step, entry), so a commit's
        samples depend on its key (default: its row in the batch), not on the batch it lands in.  The step loop is captured
        into hipGraphs by the loop driver of ``greedy`` (``_Loop``), with the same early stop between chunks.  The filters are
        fixed in the captured launches, so they are part of the state's key; the seed is a device scalar read at run time: one
        capture serves every seed."""
        self._no_ensemble("sample")                           # raises before anything is launched
        _refuse_each("sample", "its fused step hands no distribution over; sample_search does", neighbour=neighbour,
                     penalties=penalties, phrases=phrases, template=template)
        cuts = self._check_cuts(top_p, min_p, epsilon, eta, typical_p)
        B, T = db.B, self.cfg.tar_len
        R = B * n
        noise_rows, fill_noise = self._noise(keys, seed, B)   # raises before anything is launched
        make = lambda i32, f32: dict(self._hypothesis_rows(i32, f32, R), logp=f32(R), **noise_rows(i32))
        key = ("sample", B, n, float(temperature), int(top_k), float(top_p))
        loop = _Loop(self, db, n, key if cuts == self.CUTS_OFF else key + cuts, make, chunk, use_graphs)
        st, ws = loop.st, loop.ws
        fill_noise(st)
        loop.start(lambda lo, hi: self._sample_steps(st, ws, B, n, lo, hi, temperature, top_k, top_p, cuts),
                   lambda: self._sample_reset(st), lambda hi: self._none_alive(st, hi)).run()
        return (st["out"].view(B, n, T).long(), st["length"].view(B, n).long(), st["prob"].view(B, n).clone(),
                st["logp"].view(B, n).clone())

    def _sample_search_steps(self, st, ws, B, n, lo, hi, temperature, top_k, top_p, cuts):
        """Steps lo..hi-1 of ``sample_search``: the step (every member's and the mix, or the neighbour's and the mix) into the
        state's distribution, the edit chain without an arg-max, the draw from the rows as they then stand, the bookkeeping of
        ``sample``; no torch op, no host round trip."""
        lib, s, dims = _lib.lib(), _lib.cur_stream(), C.byref(self.model.dims)
        R = B * n
        for step in range(lo, hi):
            self._step(ws, B, n, step, st["tok"], None, st["dist"], None, None)
            self._edit(st, R, n, st["out"], st["length"], None)
            _lib.check(lib.fira_sample_dist(s, dims, R, n, step, _lib.ptr(st["dist"]), _lib.ptr(st["key"]), _lib.ptr(st["seed"]),
                                            float(temperature), int(top_k), float(top_p), *cuts, _lib.ptr(st["best_id"]),
                                            _lib.ptr(st["best_p"])), "fira_sample_dist")
            _lib.check(lib.fira_sample_advance(s, dims, B, n, step, _lib.ptr(st["best_id"]), _lib.ptr(st["best_p"]),
                                               _lib.ptr(st["sou"]), _lib.ptr(st["sub"]), _lib.ptr(st["out"]),
                                               _lib.ptr(st["length"]), _lib.ptr(st["prob"]), _lib.ptr(st["logp"]),
                                               _lib.ptr(st["alive"]), _lib.ptr(st["tok"]), _lib.ptr(st["n_alive"])),
                       "fira_sample_advance")

    @torch.no_grad()
    def sample_search(self, db: DeviceBatch, n: int, *, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                      min_p: float = 0.0, epsilon: float = 0.0, eta: float = 0.0, typical_p: float = 1.0, seed: int = 0, keys=None,
                      constraints: Optional[Constraints] = None, merge_copies: bool = False, prefix=None,
                      neighbour: Optional[Neighbour] = None, chunk: int = 5, use_graphs: bool = True,
                      penalties: Optional[Penalties] = None, phrases: Optional[Phrases] = None,
                      template: Optional[Template] = None, wordsets: Optional[WordSets] = None, knn: Optional[KnnMT] = None):
        """``n`` sampled messages per commit, drawn from the search's EDITED distribution: what ``sample`` returns (tokens
        [B,n,T], lengths [B,n], probability [B,n], log-probability [B,n]), with every option of the searches -- ``constraints``,
        ``merge_copies``, ``prefix``, ``penalties`` (the class's options), an ensemble (``members=``) and a ``neighbour`` -- and
        every filter and cut of ``sample``.  With active ``penalties`` the returned values are scores (products and log-sums of
        the penalised entries), not probabilities.  Per step: the decoder step writes its distribution (every member's and ``fira_mix_dist``, or the
        neighbour's and ``fira_mix_neighbour``), the edit chain (``_edit``) edits it, ``fira_sample_dist`` applies the filters, the
        cuts and the Gumbel-max draw to the rows as they then stand, ``fira_sample_advance`` appends.  The rows are not
        renormalised; the filters work relative to each row's own sums, an entry with probability 0 is never drawn, and the
        returned probabilities are the edited (untempered, unfiltered) values of the entries taken: a word's probability after
        a merge, the mixed probability after a mix, the joint probability of prefix and continuation with a prefix.  A row the
        edits left without a positive entry takes entry 0 with probability 0 (log-probability -inf).

        What holds exactly:
          * no option and no members: ``sample``'s result, bit for bit, for the same filters, cuts, seed and keys;
          * ``top_k=1``: ``greedy(...)`` with the same options, wherever every step's maximum is unique;
          * members with weights (1, 0, ...): the single model's result;
          * a neighbour with ``lam = 0``: the plain result.

        The filters and cuts are fixed in the captured launches and join the state's key with the options (``_key``); the
        prefix, the seed, the keys and the neighbour's coefficients are device values, so one capture serves all of them.
        ``template``: a ``Template`` value, as for ``greedy``.
        ``wordsets``: a ``WordSets`` value, as for ``greedy``; with an active ``boost`` the returned values are scores.
        ``knn``: a ``KnnMT`` value, as for ``greedy``: the returned probabilities are the mixed values of the entries taken.
        ``phrases``: banned phrases, as for ``greedy``.  There is no ``require=`` and no required item: banks need a beam.  A ``ValueError`` before anything is launched on a value outside its
        range, ``n`` outside 1..8, or whatever the options' own checks refuse (a neighbour with members among them)."""
        cuts = self._check_cuts(top_p, min_p, epsilon, eta, typical_p)     # every refusal: before anything is launched
        if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 1 <= n <= 8:
            raise ValueError("n = %r: samples per commit outside 1..8" % (n,))
        temperature, top_p = C.c_float(float(temperature)).value, C.c_float(float(top_p)).value
        if not 0 < temperature < float("inf"):
            raise ValueError("temperature %r: must be finite and > 0" % temperature)
        if isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral) or not 0 <= top_k <= self.cfg.out_len:
            raise ValueError("top_k %r: must be an integer in 0..%d (0 = off)" % (top_k, self.cfg.out_len))
        if not 0 < top_p <= 1:
            raise ValueError("top_p %r: must be in (0, 1] (1 = off)" % top_p)
        n, top_k = int(n), int(top_k)
        B, T = db.B, self.cfg.tar_len
        R = B * n
        opts = self._options("sample_search", db, constraints=constraints, merge_copies=merge_copies, prefix=prefix,
                             neighbour=neighbour, penalties=penalties, phrases=phrases, template=template, wordsets=wordsets,
                             knn=knn)
        noise_rows, fill_noise = self._noise(keys, seed, B)
        make = lambda i32, f32: dict(self._hypothesis_rows(i32, f32, R), logp=f32(R), **noise_rows(i32),
                                     **opts.state(i32, f32, R, B, dist=True))
        loop = _Loop(self, db, n, opts.key(("sample_search", B, n, temperature, top_k, top_p) + cuts), make, chunk, use_graphs,
                     opts.mixer)
        st, ws = loop.st, loop.ws
        fill_noise(st)
        opts.fill(st, db)
        loop.start(lambda lo, hi: self._sample_search_steps(st, ws, B, n, lo, hi, temperature, top_k, top_p, cuts),
                   lambda: self._sample_reset(st), lambda hi: self._none_alive(st, hi)).run()
        return (st["out"].view(B, n, T).long(), st["length"].view(B, n).long(), st["prob"].view(B, n).clone(),
                st["logp"].view(B, n).clone())

    def best_sample(self, tokens, lengths, logp) -> List[List[int]]:
        """The highest-log-probability sample per commit, first on ties."""
        return self.best(tokens, lengths, logp)

    # ------------------------------------------------------------------ minimum-Bayes-risk pick by expected sentence BLEU
    MBR_MAX_N, MBR_MAX_T = 32, 64

    def mbr(self, tokens, lengths, logp=None, utility="bleu", classes=None):
        """Minimum-Bayes-risk selection among candidate messages: the candidates of a commit are taken as draws from the model
        and the one with the highest mean sentence BLEU (method 2) against the others wins.  ``tokens`` [B, n, T] vocabulary
        ids and ``lengths`` [B, n] as ``sample`` returns them (or several ``sample`` calls concatenated along n), 1 <= n <= 32,
        1 <= T <= 64; the message of a candidate is its ids at positions 1 .. length - 1 without <pad> / <eos> / <start>, which
        is its text (``text.detokenize``).  ``logp`` [B, n] (optional) breaks ties, then the lower index.

        Returns (pick: the winner's index per commit, utilities [B, n] float64 CPU tensor).  One launch
        (``fira_mbr_bleu_stats``: all n x n pairs, exact integers), one copy back, the scores formed on the host by
        ``metrics.mbr_utilities`` / ``mbr_pick`` -- ``==`` the string scorer on the same words.  Raises ValueError before
        anything is launched on a wrong shape, an id outside int32 or n / T outside the limits.

        ``utility="rouge_l"`` takes sentence-level ROUGE-L (``metrics.rouge_l``: in-order overlap at any distance) in place of
        BLEU: the same messages, the same checks, ``fira_mbr_rouge_l_stats`` as the one launch (4 integers per pair), the
        utilities ``==`` the mean of ``metrics.rouge_l`` on the words.

        ``utility="meteor_exact"`` takes ``metrics.meteor_exact`` -- NLTK's METEOR alignment and score (alpha 0.9, beta 3,
        gamma 0.5: recall-weighted unigram matches with a fragmentation penalty) WITHOUT its stem and WordNet stages, so not
        the paper's METEOR and not checked against NLTK -- through ``fira_mbr_meteor_stats`` as the one launch (4 integers per
        pair).  ``classes`` (this utility only): an integer tensor or sequence of length ``cfg.vocab_size``; ids of equal class
        match in a second stage after the equal ids (the caller's stems or synonym sets; the project ships none).  A wrong
        length, a non-integer dtype or ``classes`` with another utility is a ValueError before anything is launched.  Any other
        ``utility`` is a ValueError."""
        from . import metrics, ops
        if utility not in metrics.MBR_UTILITIES:
            raise ValueError("utility: %r is not one of %s" % (utility, ", ".join(metrics.MBR_UTILITIES)))
        if classes is not None:
            if utility != "meteor_exact":
                raise ValueError("classes: only utility=\"meteor_exact\" takes a class table, not %r" % (utility,))
            classes = torch.as_tensor(classes)
            if classes.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
                raise ValueError("classes: expected integers, got %s" % classes.dtype)
            if tuple(classes.shape) != (self.cfg.vocab_size,):
                raise ValueError("classes: shape %s, expected (%d,) -- one class per vocabulary id"
                                 % (tuple(classes.shape), self.cfg.vocab_size))
            if classes.dtype == torch.int64 and classes.numel():
                lo, hi = torch.aminmax(classes)
                if int(lo) < -(1 << 31) or int(hi) >= 1 << 31:
                    raise ValueError("classes: class outside the int32 range")
        if not (torch.is_tensor(tokens) and torch.is_tensor(lengths)):
            tokens, lengths = torch.as_tensor(tokens), torch.as_tensor(lengths)
        if tokens.dim() != 3:
            raise ValueError("tokens: expected [B, n, T] token ids, got shape %s" % (tuple(tokens.shape),))
        B, n, T = tokens.shape
        if not 1 <= n <= self.MBR_MAX_N:
            raise ValueError("tokens: n = %d candidates per commit, outside 1..%d" % (n, self.MBR_MAX_N))
        if not 1 <= T <= self.MBR_MAX_T:
            raise ValueError("tokens: T = %d positions, outside 1..%d" % (T, self.MBR_MAX_T))
        if tuple(lengths.shape) != (B, n):
            raise ValueError("lengths: shape %s, expected %s" % (tuple(lengths.shape), (B, n)))
        int_types = (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64)
        if tokens.dtype not in int_types or lengths.dtype not in int_types:
            raise ValueError("tokens / lengths: expected integer tensors, got %s / %s" % (tokens.dtype, lengths.dtype))
        if logp is not None:
            logp = torch.as_tensor(logp)
            if tuple(logp.shape) != (B, n):
                raise ValueError("logp: shape %s, expected %s" % (tuple(logp.shape), (B, n)))
        if B == 0:
            return [], torch.zeros((0, n), dtype=torch.float64)
        dev = self.model.device_
        tokens, lengths = tokens.to(dev), lengths.to(dev)
        if tokens.dtype == torch.int64:                       # (the one range check: a single read-back, before the launch)
            lo, hi = torch.aminmax(tokens)
            if int(lo) < -(1 << 31) or int(hi) >= 1 << 31:
                raise ValueError("tokens: id outside the int32 range")
        lengths = lengths.clamp(min=0, max=T)                 # (the message ends at min(length, T) anyway)
        tokens, lengths = tokens.to(torch.int32).contiguous(), lengths.to(torch.int32).contiguous()
        if utility == "meteor_exact":
            stats = ops.mbr_meteor_stats(tokens, lengths, None if classes is None else classes.to(dev, torch.int32).contiguous())
        else:
            stats = (ops.mbr_bleu_stats if utility == "bleu" else ops.mbr_rouge_l_stats)(tokens, lengths)
        util = metrics.mbr_utilities(stats.cpu(), utility)
        pick = metrics.mbr_pick(util, None if logp is None else logp.detach().cpu())
        return pick, torch.tensor(util, dtype=torch.float64).reshape(B, n)

    # ------------------------------------------------------------------ scoring given messages (teacher-forced)
    SCORE_TOKEN_KEYS = ("p_word", "p_entry", "entry", "copy_share", "top_id", "p_label")
    RANK_KEYS = ("logp_entry", "logp_word", "mean_logp_word")

    def _score_reset(self, st):
        for k in ("p_word", "p_entry", "copy_share", "p_label", "logp_word", "logp_entry", "logp_label"):
            st[k].zero_()
        st["entry"].fill_(-1)
        st["top_id"].fill_(-1)

    def _score_steps(self, st, ws, B, n, lo, hi, dist=None):
        """Steps lo..hi-1: one library call per step -- the KV-cached decoder step fed with the candidates' own tokens and the
        scoring kernel in place of the arg-max; no bookkeeping launch, no torch op, no host round trip."""
        lib, s = _lib.lib(), _lib.cur_stream()
        lab = st["labelled"]
        for step in range(lo, hi):
            _lib.check(lib.fira_decode_step_score(
                s, C.byref(self.model.dims), _lib.ptr(self.model.flat.data), _lib.ptr(ws), ws.numel(), B, n, step,
                _lib.ptr(st["cand"][step]), _lib.ptr(st["cand"][step + 1]), _lib.ptr(st["label"][step + 1]) if lab else None,
                _lib.ptr(st["sou"]), _lib.ptr(st["sub"]), _lib.ptr(dist[step]) if dist is not None else None,
                _lib.ptr(st["p_word"][step]), _lib.ptr(st["p_entry"][step]), _lib.ptr(st["entry"][step]),
                _lib.ptr(st["copy_share"][step]), _lib.ptr(st["p_label"][step]) if lab else None,
                _lib.ptr(st["top_id"][step]), _lib.ptr(st["logp_word"]), _lib.ptr(st["logp_entry"]),
                _lib.ptr(st["logp_label"]) if lab else None, self.flags), "fira_decode_step_score")

    def check_candidates(self, cand, lengths=None, labels=None, B=None):
        """Validates candidate messages on the host (nothing is launched) and returns them as int32 CPU tensors
        (cand [B, n, tar_len] zero-padded, length [B, n], labels [B, n, tar_len] with -1 past the message, or None).
        Raises ValueError on anything the scoring kernel's contract excludes."""
        cfg = self.cfg
        T, V = cfg.tar_len, cfg.vocab_size
        cand = torch.as_tensor(cand).detach().cpu().long()
        if cand.dim() == 2:
            cand = cand[:, None, :]
        if cand.dim() != 3:
            raise ValueError("cand: expected [B, n, T] or [B, T] token ids, got shape %s" % (tuple(cand.shape),))
        Bc, n, Tc = cand.shape
        if B is not None and Bc != B:
            raise ValueError("cand: %d commits for a batch of %d" % (Bc, B))
        if not 1 <= n <= 8:
            raise ValueError("cand: %d candidates per commit, outside 1..8" % n)
        if not 1 <= Tc <= T:
            raise ValueError("cand: %d positions, outside 1..tar_len = %d" % (Tc, T))
        if Tc < T:
            cand = torch.cat([cand, cand.new_zeros(Bc, n, T - Tc)], 2)
        pos = torch.arange(T)[None, None, :]
        if lengths is None:
            length = (cand != PAD).long().cumprod(2).sum(2)                # the leading run of non-zero ids
        else:
            length = torch.as_tensor(lengths).detach().cpu().long().reshape(Bc, n)
            if int(length.min()) < 1 or int(length.max()) > Tc:
                raise ValueError("lengths: outside 1..%d" % Tc)
            cand = torch.where(pos < length[:, :, None], cand, torch.zeros_like(cand))
        inside = pos < length[:, :, None]
        if bool(((cand == PAD) != ~inside).any()):
            raise ValueError("cand: id 0 (<pad>) inside a message (only the padding after it may be 0)")
        if int(cand.min()) < 0 or int(cand.max()) >= V:
            raise ValueError("cand: token id outside the vocabulary [0, %d)" % V)
        if bool((cand[:, :, 0] != START).any()):
            raise ValueError("cand: every message starts with <start> (id %d)" % START)
        if bool(((cand == EOS) & (pos != length[:, :, None] - 1)).any()):
            raise ValueError("cand: <eos> before the end of a message")
        if labels is not None:
            labels = torch.as_tensor(labels).detach().cpu().long()
            if labels.dim() == 2:
                labels = labels[:, None, :]
            if labels.shape[:2] != (Bc, n) or labels.shape[2] > T:
                raise ValueError("labels: shape %s does not match the candidates' %s" % (tuple(labels.shape), (Bc, n, Tc)))
            if labels.shape[2] < T:
                labels = torch.cat([labels, labels.new_zeros(Bc, n, T - labels.shape[2])], 2)
            if int(labels.max()) >= cfg.out_len:
                raise ValueError("labels: entry index outside [0, %d)" % cfg.out_len)
            labels = torch.where(inside & (labels >= 0), labels, torch.full_like(labels, -1)).to(torch.int32)
        return cand.to(torch.int32), length.to(torch.int32), labels

    @_refuses("knn", "wordsets")
    @torch.no_grad()
    def score(self, db: DeviceBatch, cand, lengths=None, labels=None, chunk: int = 5, use_graphs: bool = True, dist=None,
              neighbour=None, penalties=None, phrases=None, template=None):
        """Teacher-forced probability of given messages.  ``cand`` [B, n, T] (or [B, T]) vocabulary ids, each message starting
        with <start> and ending with <eos> unless truncated, zero-padded; 1 <= n <= 8 candidates per commit share the
        commit's encoder pass and memory (``fira_decode_begin`` with n rows per commit).  ``labels`` (same shape, optional):
        the output entry credited at every position, as ``tar_label`` (-1 = none).

        Returns a ``Scores`` dict: per token [B, n, tar_len - 1] (index t scores the id at position t + 1) ``p_word`` (the
        word's probability over every entry that resolves to it), ``p_entry`` / ``entry`` (its largest single entry),
        ``copy_share``, ``top_id`` (the model's arg-max entry, -1 where nothing is scored) and ``p_label``; per candidate
        [B, n] ``logp_word``, ``logp_entry``, ``logp_label`` (float64 sums of log max(p, 1e-10)) and ``length`` (ids including
        <start>; ``length - 1`` tokens are scored).  The step loop is captured into hipGraphs per (B, n, labels given) by the
        loop driver of ``greedy`` (``_Loop``); how many chunks to replay follows from the longest candidate, so nothing is read
        back between chunks.  Candidates, labels and per-token outputs are step-major in the state ([T, B * n]), so step t's
        inputs and outputs are plain rows of them.
        ``dist`` (tests): a [tar_len - 1, B * n, out_len] tensor that receives every step's distribution (eager only)."""
        self._no_ensemble("score")                            # raises before anything is launched
        _refuse_each("score", "its fused step hands no distribution over, and it reports the model's probability",
                     neighbour=neighbour, penalties=penalties, phrases=phrases, template=template)
        cfg = self.cfg
        B, T = db.B, cfg.tar_len
        cand, length, labels = self.check_candidates(cand, lengths, labels, B)        # raises before anything is launched
        n = cand.shape[1]
        R = B * n
        make = lambda i32, f32: dict(cand=i32(T, R), label=i32(T, R), p_word=f32(T - 1, R), p_entry=f32(T - 1, R),
                                     entry=i32(T - 1, R), copy_share=f32(T - 1, R), p_label=f32(T - 1, R), top_id=i32(T - 1, R),
                                     logp_word=f32(R), logp_entry=f32(R), logp_label=f32(R), labelled=labels is not None)
        loop = _Loop(self, db, n, ("score", B, n, labels is not None), make, chunk, use_graphs and dist is None)
        st, ws = loop.st, loop.ws
        st["cand"].copy_(cand.reshape(R, T).t())
        if labels is not None:
            st["label"].copy_(labels.reshape(R, T).t())
        # step t scores position t + 1 <= length - 1: the loop needs max(length) - 1 steps and no stop test
        loop.start(lambda lo, hi: self._score_steps(st, ws, B, n, lo, hi, dist), lambda: self._score_reset(st),
                   n_steps=max(int(length.max()) - 1, 0)).run()
        res = Scores()
        scored = (st["cand"][1:] != PAD).t().reshape(B, n, T - 1)
        for k in self.SCORE_TOKEN_KEYS:
            if k == "p_label" and labels is None:
                continue
            res[k] = st[k].t().reshape(B, n, T - 1).clone()
        res["top_id"] = torch.where(scored, res["top_id"], torch.full_like(res["top_id"], -1)).long()
        res["entry"] = res["entry"].long()
        # The per-candidate sums are re-formed here in float64 from the per-token values (exact fp32 inputs, one small torch
        # expression).  The kernel's own fp32 running sums (the C ABI's logp_*) round once per step at the magnitude of the
        # sum: measured 4.3e-6 relative on exp(logp) at logp = -32, above the T * 2^-23 a product of T factors stays within.
        floor = lambda p: torch.log(p.double().clamp(min=1e-10))
        res["logp_word"] = torch.where(scored, floor(res["p_word"]), 0.0).sum(2)
        res["logp_entry"] = torch.where(scored, floor(res["p_entry"]), 0.0).sum(2)
        if labels is not None:
            labelled = scored & (st["label"][1:] >= 0).t().reshape(B, n, T - 1)
            res["logp_label"] = torch.where(labelled, floor(res["p_label"]), 0.0).sum(2)
        res["length"] = length.to(self.model.device_).long()
        return res

    def rank(self, scores, by: str = "logp_word") -> List[int]:
        """Index of the best candidate per commit under ``by``: ``logp_entry`` (what ``best_sample`` ranks by: the largest
        single entry per token), ``logp_word`` (the word marginal) or ``mean_logp_word`` (per scored token); first on ties."""
        if by not in self.RANK_KEYS:
            raise ValueError("rank: by=%r, expected one of %s" % (by, ", ".join(self.RANK_KEYS)))
        return torch.argmax(rank_values(scores, by), dim=1).tolist()

    # ------------------------------------------------------------------ beam search with the reference's semantics
    def _family_reset(self, st, values, void):
        """The reset of the beam family (``beam``, ``sample_distinct``): both ping-pong buffers of ``gen`` / ``length`` empty, then
        <start> at length 1 in the first, the per-slot ``values`` at ``void`` and ``done`` clear; the caller seeds its live slots."""
        for k in ("gen", "length"):
            st[k][0].zero_()
            st[k][1].zero_()
        st["gen"][0][:, 0] = START
        st["length"][0].fill_(1)
        for k in values:
            st[k][0].fill_(void)
            st[k][1].fill_(void)
        st["done"].zero_()

    def _family_steps(self, st, ws, B, beam, lo, hi, select):
        """Steps lo..hi-1 of the beam family: prepare -> KV-cached decoder step (the members' steps and the mix, for an
        ensemble) -> edit chain -> ``select(lib, s, step, cur, nxt)``, the caller's selection call from the ``cur`` ping-pong
        buffers into the ``nxt`` ones; all on the device."""
        lib, s, T = _lib.lib(), _lib.cur_stream(), self.cfg.tar_len
        for step in range(lo, hi):
            cur, nxt = step & 1, (step + 1) & 1
            _lib.check(lib.fira_beam_prepare(s, B, beam, T, step, _lib.ptr(st["gen"][cur]), _lib.ptr(st["length"][cur]),
                                             _lib.ptr(st["tok"]), _lib.ptr(st["fin"]), _lib.ptr(st["active"]),
                                             _lib.ptr(st["done"])), "fira_beam_prepare")
            self._step(ws, B, beam, step, st["tok"], st["parent"] if step > 0 else None, st["dist"], None, None)
            self._edit(st, B * beam, beam, st["gen"][cur], st["length"][cur], None)
            select(lib, s, step, cur, nxt)

    def _family_result(self, loop, B, beam, values):
        """(hypotheses [B,beam,T] int64, lengths [B,beam], the per-slot ``values`` [B,beam]) of a finished beam-family loop."""
        st, cur = loop.st, loop.hi & 1                       # the ping-pong buffer the last step run wrote
        return (st["gen"][cur].view(B, beam, self.cfg.tar_len).long(), st["length"][cur].view(B, beam).long()) + tuple(
            st[k][cur].view(B, beam).clone() for k in values)

    def _beam_reset(self, st, B, beam):
        self._family_reset(st, ("prob",), 0.0)
        sc = st.get("scoring")                               # the first slot of the beam, or of every group
        st["prob"][0].view(B, beam)[:, ::beam if sc is None else beam // sc.groups] = 1.0

    def _beam_steps(self, st, ws, B, beam, lo, hi):
        """Steps lo..hi-1 of run_model.py:225-340 (``_family_steps``) with fira_beam_select, under a BeamScoring
        fira_beam_select_scored, with required words fira_beam_select_required, or with required items
        fira_beam_select_phrases, as the selection."""
        sc, dims, req, items = st.get("scoring"), C.byref(self.model.dims), "required" in st, "require-phrases" in st

        def select(lib, s, step, cur, nxt):
            state = (_lib.ptr(st["dist"]), _lib.ptr(st["fin"]), _lib.ptr(st["active"]), _lib.ptr(st["done"]),
                     _lib.ptr(st["sou"]), _lib.ptr(st["sub"]), _lib.ptr(st["gen"][cur]), _lib.ptr(st["length"][cur]),
                     _lib.ptr(st["prob"][cur]), _lib.ptr(st["gen"][nxt]), _lib.ptr(st["length"][nxt]),
                     _lib.ptr(st["prob"][nxt]), _lib.ptr(st["parent"]))
            if items:
                _lib.check(lib.fira_beam_select_phrases(s, dims, B, beam, *state, _lib.ptr(st["item_words"]),
                                                        _lib.ptr(st["item_len"]), _lib.ptr(st["n_items"]), _lib.ptr(st["met"])),
                           "fira_beam_select_phrases")
            elif req:
                _lib.check(lib.fira_beam_select_required(s, dims, B, beam, *state, _lib.ptr(st["required"]),
                                                         _lib.ptr(st["n_required"]), _lib.ptr(st["met"])),
                           "fira_beam_select_required")
            elif sc is None:
                _lib.check(lib.fira_beam_select(s, dims, B, beam, *state), "fira_beam_select")
            else:
                _lib.check(lib.fira_beam_select_scored(s, dims, B, beam, *state, _lib.ptr(st["inv_lp"]), sc.groups,
                                                       sc.diversity, _lib.ptr(st["key"])), "fira_beam_select_scored")
        self._family_steps(st, ws, B, beam, lo, hi, select)

    @torch.no_grad()
    def beam(self, db: DeviceBatch, beam: int, chunk: int = 4, use_graphs: bool = True,
             constraints: Optional[Constraints] = None, merge_copies: bool = False,
             scoring: Optional[BeamScoring] = None, prefix=None, require=None, neighbour: Optional[Neighbour] = None,
             penalties: Optional[Penalties] = None, phrases: Optional[Phrases] = None,
             template: Optional[Template] = None, wordsets: Optional[WordSets] = None, knn: Optional[KnnMT] = None):
        """Returns (hypotheses [B,beam,T] int64, lengths [B,beam], probabilities [B,beam]).  ``constraints``, ``merge_copies``,
        ``prefix`` and ``penalties`` are the class's options, one library call per step each, between the step and the selection
        (``_edit``); the state is keyed ("beam", B, beam[, "merge"][, "prefix"][, "require"][, "neighbour"][, "penalties"]
        [, constraints][, scoring]) (``_key``).  ``penalties`` combines with everything below (the selections read the edited row);
        the third tensor is then the product of the edited entries taken -- a score, not a probability.

        ``scoring``: a ``BeamScoring`` value.  ``fira_beam_select_scored`` then takes the place of ``fira_beam_select`` (after
        the edit chain): hypotheses are ranked by the length-normalised key ln(prob) / ((5 + m) / 6)^alpha instead of
        the raw probability, within ``groups`` beam groups that a ``diversity`` penalty per repeated word keeps apart.  The
        call then returns FOUR tensors, (hypotheses, lengths, probabilities, keys [B,beam]) -- the raw probability and the
        unpenalised key of every slot, -inf where the probability is 0 -- and ``best(gen, length, key)`` picks by key.  The
        value joins the state key (the scalars are baked into captured graphs); the state owns the inv_lp table and the key
        buffer, and its reset seeds the first slot of every group.  None or an inactive value: today's key, buffers,
        launches, graphs and three tensors.  A beam of 1 with ``scoring`` given is a ``ValueError``.

        ``require``: the words every message must contain -- B sequences of at most 4 distinct vocabulary ids in (UNK, vocab);
        an empty one means none for that commit.  ``fira_beam_select_required`` then takes the place of ``fira_beam_select``
        (DESIGN.md section 6v): lexically constrained decoding with dynamic beam allocation.  The beam is divided into banks by
        the number of required words a hypothesis holds, every bank keeps slots, and no message ends before it holds all its
        words.  A word counts through its generator entry or a copy slot that carries it; prefix words count as met;
        ``merge_copies`` is recommended.  The call then returns FOUR tensors, (hypotheses, lengths, probabilities,
        met [B,beam]) -- met is the number of required words a slot's hypothesis holds -- and ``best_required`` picks the
        message.  The state is keyed by a "require" marker, not by the words (device buffers, filled on every call: one capture
        serves every word list).  A commit without words gets the plain ``beam`` result bit for bit.  None or every sequence
        empty: today's key, buffers, launches, graphs and three tensors.  A ``ValueError`` before anything is launched on a
        wrong count, a non-integer id, an id outside (UNK, vocab), a duplicate, more than 4 words, ``beam < 2``,
        ``beam < len(words) + 1`` (a bank per count), more than tar_len - 2 words, a word the ``constraints`` ban, or an
        active ``scoring``.

        ``phrases``: a ``Phrases`` value.  Its banned phrases are a link of the edit chain, after the
        constraints ("ban-phrases" joins the state key).  Its required items take ``require=``'s place with word sequences:
        ``fira_beam_select_phrases`` is the selection, the banks count ``progress`` -- the words of the items a hypothesis holds
        contiguously plus the longest item start it ends in, a credit it loses when it breaks the phrase off -- no message ends
        before every item is complete, and the call returns (hypotheses, lengths, probabilities, met [B,beam]) with met = the
        progress of every slot; ``best_required`` picks the message ("require-phrases" joins the state key; device buffers, one
        capture for every list).  A ``ValueError`` before anything is launched on what ``Phrases`` and ``_phrases`` refuse:
        required items together with ``require=`` or an active ``scoring``, ``beam < 2``, ``beam`` below the number of required
        words + 1, an item that holds a banned word or phrase or repeats an n-gram, a prefix that contains a banned phrase.

        ``template``: a ``Template`` value, a link of the edit chain after the banned phrases ("template"
        joins the state key; device buffers, one capture for every template): every hypothesis of positive probability is then
        accepted by the automaton.  It does not combine with ``require=`` or required items (a ``ValueError``, like a prefix
        that is no path of the automaton and a ``min_length`` no accepted message reaches).

        ``wordsets``: a ``WordSets`` value, a link of the edit chain after the template (("wordsets",
        names of the given sets) joins the state key; device buffers, one capture for every value that gives the same sets): no
        hypothesis of positive probability then holds a word that ``allow``, ``deny`` or ``ground`` blocks for its commit.  With an
        active ``boost`` the returned values are scores, as under ``penalties``.  A prefix word, a ``require=`` word or a word of
        a required item that ``allow`` or ``deny`` blocks is a ``ValueError``; one that ``ground`` blocks leaves probability 0.

        ``neighbour``: a ``Neighbour`` value, as for ``greedy``: the neighbour batch's step over the same tokens and parents (its
        caches follow the beam's reordering), its row folded into words, ``fira_mix_neighbour`` into the beam's distribution, then
        the edit chain and the selection as ever.  It combines with every option above; "neighbour" joins the state key.

        ``knn``: a ``KnnMT`` value, as for ``greedy``: every (commit, slot) row's hidden state is looked up (a commit's exclude
        value holds for all its rows), ``fira_mix_knn`` over the beam's distribution, then the edit chain and the selection as
        ever.  It combines with every option above but a neighbour; ("knn", K, the store) joins the state key.

        Per step, with every option off: fira_beam_prepare, fira_decode_step, fira_beam_select (csrc/beam.hip) -- three library
        calls, no torch op and no host round trip; the loop is captured into hipGraphs of ``chunk`` steps per (batch, beam)
        shape, and the ``done`` latch is read back between chunks (run_model.py:276-279)."""
        B, T = db.B, self.cfg.tar_len
        BR = B * beam
        opts = self._options("beam", db, beam=beam, scoring=scoring, constraints=constraints, merge_copies=merge_copies,
                             prefix=prefix, require=require, neighbour=neighbour, penalties=penalties, phrases=phrases,
                             template=template, wordsets=wordsets, knn=knn)         # raises before anything is launched
        make = lambda i32, f32: dict(self._beam_rows(i32, f32, BR), prob=[f32(BR), f32(BR)],
                                     **opts.state(i32, f32, BR, B, dist=True))
        # (a captured graph bakes the constraint scalars, the merge launch and the scoring scalars: they are part of the key)
        loop = _Loop(self, db, beam, opts.key(("beam", B, beam)), make, chunk, use_graphs, opts.mixer)
        st, ws = loop.st, loop.ws
        opts.fill(st, db)
        loop.start(lambda lo, hi: self._beam_steps(st, ws, B, beam, lo, hi), lambda: self._beam_reset(st, B, beam),
                   lambda hi: bool(st["done"].item())).run()
        res = self._family_result(loop, B, beam, ("prob",))
        if opts.words is not None or opts.items is not None:
            return res + (st["met"].view(B, beam).long(),)
        return res if opts.scoring is None else res + (st["key"].view(B, beam).clone(),)

    # ------------------------------------------------------------------ stochastic beam search: n samples without replacement
    def _sbs_reset(self, st, B, n):
        self._family_reset(st, ("phi", "G", "logp"), float("-inf"))
        for k in ("phi", "G", "logp"):
            st[k][0].view(B, n)[:, 0] = 0.0                   # slot 0 of every commit is the empty message; the others are void

    def _sbs_steps(self, st, ws, B, n, lo, hi, temperature):
        """Steps lo..hi-1 of the beam's loop (``_family_steps``) with fira_beam_select_gumbel as the selection."""
        def select(lib, s, step, cur, nxt):
            _lib.check(lib.fira_beam_select_gumbel(
                s, C.byref(self.model.dims), B, n, step, float(temperature), _lib.ptr(st["dist"]), _lib.ptr(st["fin"]),
                _lib.ptr(st["done"]), _lib.ptr(st["sou"]), _lib.ptr(st["sub"]), _lib.ptr(st["key"]), _lib.ptr(st["seed"]),
                _lib.ptr(st["gen"][cur]), _lib.ptr(st["length"][cur]), _lib.ptr(st["phi"][cur]), _lib.ptr(st["G"][cur]),
                _lib.ptr(st["logp"][cur]), _lib.ptr(st["gen"][nxt]), _lib.ptr(st["length"][nxt]), _lib.ptr(st["phi"][nxt]),
                _lib.ptr(st["G"][nxt]), _lib.ptr(st["logp"][nxt]), _lib.ptr(st["parent"])), "fira_beam_select_gumbel")
        self._family_steps(st, ws, B, n, lo, hi, select)

    @_refuses("knn", "wordsets")
    @torch.no_grad()
    def sample_distinct(self, db: DeviceBatch, n: int, *, temperature: float = 1.0, seed: int = 0, keys=None,
                        merge_copies: bool = True, constraints: Optional[Constraints] = None, chunk: int = 4,
                        use_graphs: bool = True, neighbour=None, penalties=None, phrases=None, template=None):
        """``n`` messages per commit sampled WITHOUT replacement: stochastic beam search (Kool, van Hoof and Welling 2019;
        ``fira_beam_select_gumbel``).  A beam search whose ranking key is the Gumbel-perturbed
        log-probability of the hypothesis, a child's key conditioned on its parent's; the n hypotheses it ends with are an exact
        sample without replacement from the model's distribution over messages, and slot 0 is an ordinary ancestral sample.

        Returns (tokens [B,n,T] int64 starting with <start>, lengths [B,n], logp [B,n], phi [B,n], key [B,n]); slots are in key
        order, best first.  ``logp`` is the untempered sum of the log-probabilities of the entries taken (comparable with
        ``sample``'s), ``phi`` the log-probability under the sampling model q ~ p^(1/temperature), renormalised over the
        positive entries of every step's row as merge and constraints leave it.  A commit with fewer than n possible
        messages leaves VOID slots: length 1, <start> alone, logp = phi = key = -inf.

        The noise is the sampler's counter hash of (``seed``, ``keys[b]``, slot, step, entry): a commit's result depends on its
        key (default: its row in the batch), not on the batch it lands in; with n = 1 and ``merge_copies=False`` the result is
        ``sample(db, 1, ...)``'s, bit for bit.  ``merge_copies`` (default on): sample WORDS -- the hypotheses of finite key are
        then pairwise distinct word sequences.  Off, they are distinct ENTRY paths, and one message may appear twice (spelled
        once through the generator and once through a copy slot).  ``constraints`` as for ``beam``; an ensemble (``members=``)
        samples from the mix.  The loop is the beam's (``_family_steps``): prepare, step, edit chain, selection, captured into
        hipGraphs of ``chunk`` steps; the state is keyed ("sbs", B, n, merge, constraints, temperature) -- the temperature
        is baked into the captured launches; the seed and the keys are device values: one capture serves them all."""
        B = db.B
        _refuse_each("sample_distinct", "its hypotheses are an exact sample from the model's distribution",
                     neighbour=neighbour, penalties=penalties, phrases=phrases, template=template)        # before any launch
        opts = self._options("sample_distinct", db, constraints=constraints, merge_copies=merge_copies)
        noise_rows, fill_noise = self._noise(keys, seed, B)   # raises before anything is launched
        temperature = float(temperature)
        # the kernel's own limits, before the encoder pass or any other launch
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= 8:
            raise ValueError("sample_distinct: n = %r outside 1..8" % (n,))
        if not 0.0 < temperature < float("inf"):              # (also refuses nan)
            raise ValueError("sample_distinct: temperature = %r must be finite and > 0" % (temperature,))
        BR = B * n
        make = lambda i32, f32: dict(self._beam_rows(i32, f32, BR), phi=[f32(BR), f32(BR)], G=[f32(BR), f32(BR)],
                                     logp=[f32(BR), f32(BR)], **noise_rows(i32),
                                     **opts.state(i32, f32, BR, B, dist=True))
        loop = _Loop(self, db, n, self._sbs_key(B, n, opts.merge, opts.con, temperature), make, chunk, use_graphs)
        st, ws = loop.st, loop.ws
        fill_noise(st)
        opts.fill(st, db)
        loop.start(lambda lo, hi: self._sbs_steps(st, ws, B, n, lo, hi, temperature), lambda: self._sbs_reset(st, B, n),
                   lambda hi: bool(st["done"].item())).run()
        return self._family_result(loop, B, n, ("logp", "phi", "G"))

    # ------------------------------------------------------------------ contrastive search: top-k look-ahead, degeneration penalty
    @staticmethod
    def _check_contrastive(members, k, alpha) -> float:
        """The refusals of ``contrastive``, before anything is launched; returns alpha as a float."""
        if members:
            raise ValueError("contrastive does not combine with an ensemble (the hidden state it compares is one model's)")
        if isinstance(k, bool) or not isinstance(k, int) or not 2 <= k <= 8:
            raise ValueError("contrastive: k = %r outside 2..8" % (k,))
        if isinstance(alpha, bool) or not isinstance(alpha, numbers.Real) or not 0.0 <= alpha <= 1.0:     # (also refuses nan)
            raise ValueError("contrastive: alpha = %r must be a finite number in [0, 1]" % (alpha,))
        return float(alpha)

    def _contrastive_reset(self, st, B, k):
        self._family_reset(st, ("p",), -1.0)
        st["p"][0].view(B, k)[:, 0] = 1.0                     # slot 0 holds <start> with confidence 1; the others are void
        for q in (0, 1):
            st["prob"][q].fill_(1.0)
        st["ended"].zero_()                                   # (hist needs no reset: step t reads the rows below t only)

    def _contrastive_steps(self, st, ws, B, k, lo, hi, alpha):
        """Steps lo..hi-1 of the beam's loop (``_family_steps``) with fira_decode_hidden + fira_contrastive_select as the
        selection.  Neither call changes the step's ``dist`` and ``hidden`` nor the ``cur`` buffers, so after an eager step
        the state still holds everything the selection saw."""
        dims = C.byref(self.model.dims)

        def select(lib, s, step, cur, nxt):
            _lib.check(lib.fira_decode_hidden(s, dims, _lib.ptr(ws), ws.numel(), B, k, self.flags, _lib.ptr(st["hidden"])),
                       "fira_decode_hidden")
            _lib.check(lib.fira_contrastive_select(
                s, dims, B, k, step, alpha, _lib.ptr(st["dist"]), _lib.ptr(st["hidden"]), _lib.ptr(st["fin"]), _lib.ptr(st["sou"]),
                _lib.ptr(st["sub"]), _lib.ptr(st["gen"][cur]), _lib.ptr(st["length"][cur]), _lib.ptr(st["p"][cur]),
                _lib.ptr(st["prob"][cur]), _lib.ptr(st["hist"]), _lib.ptr(st["ended"]), _lib.ptr(st["gen"][nxt]),
                _lib.ptr(st["length"][nxt]), _lib.ptr(st["p"][nxt]), _lib.ptr(st["prob"][nxt]), _lib.ptr(st["parent"]),
                _lib.ptr(st["pick"]), _lib.ptr(st["sim"]), _lib.ptr(st["score"])), "fira_contrastive_select")
        self._family_steps(st, ws, B, k, lo, hi, select)

    def _contrastive_loop(self, db: DeviceBatch, k: int, alpha: float, chunk: int, use_graphs: bool,
                          constraints: Optional[Constraints] = None, prefix=None) -> _Loop:
        """Encoder pass + reset of the state for one batch; returns the started loop (``contrastive`` runs it and reads the
        result with ``_contrastive_result``)."""
        alpha = self._check_contrastive(self.members, k, alpha)          # raises before anything is launched
        B, T = db.B, self.cfg.tar_len
        BR = B * k
        opts = self._options("contrastive", db, constraints=constraints, merge_copies=True, prefix=prefix)      # likewise
        make = lambda i32, f32: dict(self._beam_rows(i32, f32, BR), p=[f32(BR), f32(BR)], prob=[f32(B), f32(B)],
                                     hist=f32(B, T, 256), hidden=f32(BR, 256), ended=i32(B), pick=i32(B), sim=f32(BR),
                                     score=f32(BR), **opts.state(i32, f32, BR, B, dist=True))
        loop = _Loop(self, db, k, opts.key(("contrastive", B, k, alpha)), make, chunk, use_graphs)
        st, ws = loop.st, loop.ws
        opts.fill(st, db)
        return loop.start(lambda lo, hi: self._contrastive_steps(st, ws, B, k, lo, hi, alpha),
                          lambda: self._contrastive_reset(st, B, k), lambda hi: bool(st["done"].item()))

    def _contrastive_result(self, loop, B, k):
        st, T, cur = loop.st, self.cfg.tar_len, loop.hi & 1   # the ping-pong buffer the last step run wrote
        gen, length = st["gen"][cur].view(B, k, T)[:, 0], st["length"][cur].view(B, k)[:, 0]
        # a commit still running at tar_len takes slot 0, its most probable candidate (the candidates are in value order)
        last = st["p"][cur].view(B, k)[:, 0]
        running = (st["ended"] == 0) & (last > 0)
        return gen.long(), length.long(), torch.where(running, st["prob"][cur] * last, st["prob"][cur])

    @_refuses("knn", "wordsets", "template", "phrases", "penalties", why="it already penalises degeneration")
    @torch.no_grad()
    def contrastive(self, db: DeviceBatch, k: int, alpha: float = 0.6, chunk: int = 4, use_graphs: bool = True,
                    constraints: Optional[Constraints] = None, prefix=None):
        """Contrastive search (Su et al., NeurIPS 2022; ``fira_contrastive_select``): the deterministic
        search that looks one word ahead.  Returns (tokens [B,T] int64 starting with <start>, lengths [B], probability [B]),
        the message's raw model probability as ``greedy`` returns it.

        The ``k`` slots of a commit hold the chosen prefix and one of the k most probable next WORDS each; a step runs the
        decoder on all of them and keeps the candidate with the largest (1 - ``alpha``) * p - ``alpha`` * sim, sim being the
        largest cosine between the candidate's last decoder state and the states of the positions chosen before: a word
        that would lead the message back to where it has been is passed over.  ``alpha = 0`` is ``greedy(merge_copies=True)``.
        A message that reaches tar_len without <eos> takes its most probable last word (nothing is left to look ahead to).

        The loop is the beam's (``_family_steps``): prepare, step, edit chain, then ``fira_decode_hidden`` and the selection,
        captured into hipGraphs of ``chunk`` steps; the edit chain always merges copy entries into words (else the k
        candidates could be k entries of one word), and ``constraints`` / ``prefix`` pass through it unchanged.  The state
        is keyed ("contrastive", B, k, alpha, "merge"[, "prefix"][, constraints]): alpha is baked into the captured launches.
        It owns the history [B, tar_len, 256], the hidden rows, the per-slot confidences and the per-commit probability and
        ``ended`` flag; after a call ``pick`` / ``sim`` / ``score`` hold the last step's choice.  A ``ValueError`` before
        anything is launched on an ensemble, ``k`` outside 2..8 or ``alpha`` outside [0, 1] or not finite."""
        loop = self._contrastive_loop(db, k, alpha, chunk, use_graphs, constraints, prefix)
        loop.run()
        return self._contrastive_result(loop, db.B, k)

    def best(self, gen, length, prob) -> List[List[int]]:
        """argmax-probability hypothesis per item, first on ties (run_model.py:351-352)."""
        if gen.dim() == 2:
            return [row[:n] for row, n in zip(gen.tolist(), length.tolist())]
        j = torch.argmax(prob, dim=1)        # first maximal index, like np.argmax
        g = gen[torch.arange(gen.shape[0], device=gen.device), j].tolist()
        n = length[torch.arange(gen.shape[0], device=gen.device), j].tolist()
        return [row[:k] for row, k in zip(g, n)]

    def best_required(self, gen, length, prob, met) -> List[List[int]]:
        """The message of a search with required words, per commit: positive probability first, then the most words met, then
        the highest probability, then the lowest slot."""
        out = []
        for g, n, p, m in zip(gen.tolist(), length.tolist(), prob.tolist(), met.tolist()):
            j = min(range(len(p)), key=lambda q: (not p[q] > 0, -m[q], -p[q], q))
            out.append(g[j][:n[j]])
        return out


# ``_refuse`` under one name per option, ``Searcher._no_<option>(what[, why], value)``: the stand-in searchers of the tests bind
# these names when they are imported.
for _option in _REFUSAL:
    setattr(Searcher, "_no_" + _option, staticmethod(
        lambda what, *why_value, _option=_option: _refuse(what, _option, why_value[-1], *why_value[:-1])))
