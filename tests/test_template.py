"""Template-constrained search, the parts that need no GPU: the ABI, ``decode.Template`` and ``Template.sequence`` against
Python's ``re``, ``need`` against brute force, every refusal of the value and of the searches ahead of any device work, the state
keys, and the numpy statement (template_ref.py) on rows written out by hand."""
import itertools
import os
import re
import types

import numpy as np
import pytest

import template_ref as TR
import util
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, START, FiraConfig
from fira_icse_amd.decode import Constraints, Phrases, Searcher, Template

# the automaton of the hand-written rows and of the kernel tests: 5 states, 4 classes
#   class 1: a type word (4, 5); class 2: the colon (6); class 3: a word no message may hold (7); class 0: every other word
#   0 -type-> 1 -any word but the colon-> 2 (scope: further class-0 words stay in 2) -colon-> 3 -any word but 7-> 4 (accepts, loops);
#   1 -colon-> 3
HAND_CLASS = {4: 1, 5: 1, 6: 2, 7: 3}
HAND_NEXT = [[-1, 1, -1, -1], [2, 2, 3, 2], [2, -1, 3, -1], [4, 4, 4, -1], [4, 4, 4, -1]]
HAND_ACCEPT = [4]
HAND_NEED = [3, 2, 2, 1, 0]


def hand_template(start=0):
    return Template(HAND_CLASS, HAND_NEXT, HAND_ACCEPT, start)


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_library_exports_and_the_binding_matches():
    name, kinds = "fira_template_dist", "PPII" + "P" * 11
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    assert "#define FIRA_ABI_VERSION 11" in header
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, "%s is not declared" % name
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert "".join("P" if "*" in p else "I" for p in params) == kinds
    res, args = _lib.SIGNATURES[name]
    assert res is _lib._I and len(args) == len(kinds) and args[1] is _lib._DP
    assert all(t in ((_lib._P, _lib._DP) if k == "P" else (_lib._I,)) for t, k in zip(args, kinds))
    lib = _lib.lib()
    assert lib.fira_abi_version() == 11 and hasattr(lib, name)
    assert '"template.hip"' in open(os.path.join(util.REPO, "fira_icse_amd", "build.py")).read()


# ------------------------------------------------------------------------------------------------ Template.sequence against re
ALPHABET = (4, 5, 6, 7)                                        # four ids, the letters a b c d
LETTER = dict(zip(ALPHABET, "abcd"))
ITEM_LISTS = {
    "conventional": [({4, 5}, 1, 1), (None, 0, 1), ({6}, 1, 1), (None, 1, 3)],              # "any word, 0..1 times" overlaps ":"
    "overlap": [(None, 0, 3), ({6}, 1, 1)],
    "unbounded": [({4}, 1, None), ({4, 5}, 0, None), ({6}, 2, 2)],
    "lo0": [({4}, 0, 1), ({5}, 0, 2), ({4, 6}, 0, None)],
    "tail": [({7}, 2, 3), (None, 0, None)],
    "empty": [],
    "shared-sets": [({4, 5}, 1, 2), ({5, 6}, 1, 2), ({4, 5}, 0, 1)],
}


def pattern_of(items):
    out = ""
    for ids, lo, hi in items:
        letters = "".join(LETTER[w] for w in (ALPHABET if ids is None else sorted(ids)))
        out += "[%s]{%d,%s}" % (letters, lo, "" if hi is None else hi)
    return re.compile(out)


def strings(up_to=5):
    for n in range(up_to + 1):
        yield from itertools.product(ALPHABET, repeat=n)


@pytest.mark.parametrize("name", sorted(ITEM_LISTS))
def test_sequence_accepts_what_the_regular_expression_matches(name):
    items = ITEM_LISTS[name]
    t, pat = Template.sequence(items, 12), pattern_of(items)
    assert t.active and t.n_states <= 32 and t.n_classes <= 32
    n_yes = 0
    for ids in strings():
        want = pat.fullmatch("".join(LETTER[w] for w in ids)) is not None
        assert t.accepts(ids) == want, (name, ids)
        assert t.accepts(list(ids) + [EOS]) == want            # with or without the <eos> that ends it
        n_yes += want
    assert 0 < n_yes < 1365                                    # neither everything nor nothing
    # class 0 is "in no set": an id the items do not name behaves as any other such id
    assert t.class_of(11) == 0 and t.class_of(0) == 0 and t.class_of(10 ** 6) == 0


@pytest.mark.parametrize("name", sorted(ITEM_LISTS))
def test_need_is_the_fewest_words_to_acceptance(name):
    t = Template.sequence(ITEM_LISTS[name], 12)
    for s in range(t.n_states):
        brute = min((len(u) for u in strings() if t.walk(u, s) in t.accept), default=None)
        if brute is None:
            assert t.need[s] > 5, (name, s)
        else:
            assert t.need[s] == brute, (name, s)
    # the device form and the numpy statement agree with it
    wc, nxt, need, start = t.arrays(3, 12)
    assert wc.dtype == np.uint8 and wc.shape == (12,) and nxt.dtype == np.int8 and nxt.shape == (1024,)
    assert need.dtype == np.int32 and start.tolist() == [0, 0, 0]
    assert need.tolist() == TR.need_of(nxt, t.accept).tolist()
    for u in strings(4):
        assert TR.walk(u, wc, nxt, 0) == t.walk(u, 0)


def test_template_value():
    off = Template()
    assert not off.active and off.accepts([5, 6, 7]) and off.n_states == 0
    t = hand_template()
    assert t.active and t.need == tuple(HAND_NEED) and t.n_states == 5 and t.n_classes == 4
    assert t == Template({7: 3, 6: 2, 5: 1, 4: 1}, [tuple(r) for r in HAND_NEXT], (4, 4), np.int64(0)) and hash(t) == hash(hand_template())
    with pytest.raises(Exception):
        t.accept = ()                                          # frozen
    assert t.accepts([4, 6, 9]) and t.accepts([5, 9, 9, 6, 8, 8, EOS]) and not t.accepts([4, 6]) and not t.accepts([4, 6, 7])
    assert not t.accepts([4, 6, EOS, 9]) and not t.accepts([])
    both = hand_template(start=[0, 3])
    assert not both.accepts([9], 0) and both.accepts([9], 1)   # one union automaton, two rules
    full = Template([HAND_CLASS.get(w, 0) for w in range(10)], HAND_NEXT, HAND_ACCEPT)
    assert [full.class_of(w) for w in range(-1, 11)] == [t.class_of(w) for w in range(-1, 11)]
    wc, nxt, need, start = both.arrays(2, 10)
    assert wc.tolist() == [0, 0, 0, 0, 1, 1, 2, 3, 0, 0] and start.tolist() == [0, 3]
    table = nxt.reshape(32, 32)
    assert table[:5, :4].tolist() == HAND_NEXT and (table[5:] == -1).all()
    assert (table[:5, 4:] == table[:5, :1]).all()              # the columns of classes that do not exist repeat class 0's
    assert need[:5].tolist() == HAND_NEED and (need[5:] == Template.NEVER).all()
    # the accept-everything template allows all 32 classes in its one state
    every = Template({}, [[0]], [0])
    assert (every.arrays(1, 10)[1].reshape(32, 32)[0] == 0).all() and every.accepts([9, 9, 7])
    assert t.longest_fits(0, 3, 3) and not t.longest_fits(0, 0, 2) and t.longest_fits(0, 20, 25)
    assert not Template({}, [[1], [-1]], [1]).longest_fits(0, 2, 29)       # exactly one word, never two


def test_the_value_refuses_what_it_cannot_hold():
    cfg = FiraConfig()
    V, T = cfg.vocab_size, cfg.tar_len
    for kwargs, msg in ((dict(next=[[0]] * 33), "more than 32 states"), (dict(next=[[0] * 33]), "more than 32 classes"),
                        (dict(next=[[1], [2]]), r"next\[1\]\[0\] = 2 is a target outside -1..1"),
                        (dict(next=[[-2]]), "target outside -1..0"), (dict(next=[[0, 0], [0]]), "different numbers of classes"),
                        (dict(next=[[0]], accept=[1]), "accept: state 1 outside 0..0"),
                        (dict(next=[[0]], start=1), "start: state 1 outside 0..0"),
                        (dict(next=[[0]], start=[0, -1]), "start: state -1 outside"),
                        (dict(next=[[0]], word_class={5: 1}), "id 5 has class 1 outside 0..0"),
                        (dict(next=[[0]], word_class={-5: 0}), "id -5 is negative"),
                        (dict(next=[[0]], word_class={5: 0.5}), "not an integer"),
                        (dict(next=[[0.5]]), "not an integer"), (dict(next=7), "not a sequence of rows"),
                        (dict(next=[[0]], word_class=7), "neither an")):
        with pytest.raises(ValueError, match=msg):
            Template(**dict(dict(word_class={}, accept=[0]), **kwargs))
    ok = Template({}, [[0]], [0])
    assert ok.check(cfg, 4) is ok
    for t, B, msg in ((Template({V: 0}, [[0]], [0]), 2, "id %d outside the vocabulary" % V),
                      (Template({EOS: 0}, [[0]], [0]), 2, "<eos> .* is named"),
                      (Template([0] * (V - 1), [[0]], [0]), 2, "%d classes for a vocabulary of %d" % (V - 1, V)),
                      (Template({}, [[0]], [0], start=[0, 0, 0]), 2, "3 states for a batch of 2 commits"),
                      (Template({}, [[0]], []), 2, "commit 0: no accepted message within tar_len - 1 = %d words" % (T - 1)),
                      (Template({}, [[s + 1] for s in range(T)] + [[-1]], [T], start=[1, 0]), 2,
                       "commit 1: no accepted message within")):
        with pytest.raises(ValueError, match=msg):
            t.check(cfg, B)
    Template({}, [[s + 1] for s in range(T)] + [[-1]], [T], start=1).check(cfg, 2)      # exactly tar_len - 1 words: fits
    Template([0] * V, [[0]], [0]).check(cfg, 2)                # a full sequence has an entry for <eos>; it is never used


def test_sequence_refuses_what_it_cannot_build():
    with pytest.raises(ValueError, match="more than 32 states"):
        Template.sequence([({10 + k}, 1, 1) for k in range(33)], 100)      # 33 distinct single words in a row: the smallest
    Template.sequence([({10}, 1, 1) for k in range(31)], 100)              # 32 states
    with pytest.raises(ValueError, match="more than 32 states"):
        Template.sequence([({10}, 1, 1) for k in range(32)], 100)
    with pytest.raises(ValueError, match="more than 32 states"):
        Template.sequence([(None, 0, 10 ** 9)], 100)
    six = [({w for w in range(10, 74) if (w - 10) >> k & 1}, 0, 1) for k in range(6)]       # 64 membership signatures
    with pytest.raises(ValueError, match="64 classes, more than 32 classes"):
        Template.sequence(six, 100)
    assert Template.sequence(six[:5], 100).n_classes == 32
    for items, msg in (([({EOS}, 1, 1)], "<eos> .* is named"), ([({100}, 1, 1)], "id 100 outside the vocabulary"),
                       ([({5}, 2, 1)], "not 0 <= lo <= hi"), ([({5}, -1, 1)], "not 0 <= lo <= hi"), ([(set(), 1, 1)], "empty set"),
                       ([({5}, 1)], "is not \\(ids or None, lo, hi\\)"), ([(5, 1, 1)], "neither a set of ids nor None"),
                       ([({5}, 1.5, 2)], "not an integer")):
        with pytest.raises(ValueError, match=msg):
            Template.sequence(items, 100)


# ------------------------------------------------------------------------------------------------ the searches' refusals
def no_launch(members=()):
    """A Searcher whose every device path raises: a refusal must come before any of them."""
    class NoLaunch(Searcher):
        def __init__(self, members=()):
            self.members = members
            self.cfg = FiraConfig()
            self._ws = {}

        def _begin(self, *a, **k):
            raise AssertionError("device work before the refusal")
        _state = _workspace = _begin
    return NoLaunch()


def host_refusals(s, db, reaches_device):
    """Every refusal of the searches for ``template=``, on a Searcher ``s`` and a batch of two commits.  ``reaches_device(run)``
    is asked to show that an accepted value gets past the checks."""
    T = s.cfg.tar_len
    t = hand_template()
    takers = (lambda **k: s.greedy(db, **k), lambda **k: s.greedy_many([db, db], **k), lambda **k: s.beam(db, 5, **k),
              lambda **k: s.sample_search(db, 2, **k))
    for run in takers:
        with pytest.raises(ValueError, match="expected decode.Template"):
            run(template=HAND_NEXT)
        with pytest.raises(ValueError, match="3 states for a batch of 2 commits"):
            run(template=hand_template(start=[0, 0, 3]))
        with pytest.raises(ValueError, match="<eos> .* is named"):
            run(template=Template({EOS: 1}, HAND_NEXT, HAND_ACCEPT))
        with pytest.raises(ValueError, match="no accepted message has at least min_length = %d words" % (T - 2)):
            run(template=Template({}, [[1], [-1]], [1]), constraints=Constraints(min_length=T - 2))
        if run is not takers[1]:                               # (greedy_many sets up its lanes first)
            reaches_device(lambda: run(template=t))
            reaches_device(lambda: run(template=t, constraints=Constraints(min_length=T - 2)))
    # a prefix that is no path of the automaton, and one after which nothing fits (greedy_many: one prefix argument per batch)
    for bad, msg in (([[4, 6, 9], [6]], "commit 1: the prefix is not a path of the automaton from state 0"),
                     ([[4] + [9] * (T - 3), []], "commit 0: after the prefix of %d words no accepted message fits" % (T - 2))):
        for run, prefix in ((takers[0], bad), (takers[1], [None, bad]), (takers[2], bad), (takers[3], bad)):
            with pytest.raises(ValueError, match=msg):
                run(template=t, prefix=prefix)
    for run in (takers[0], takers[2], takers[3]):
        reaches_device(lambda: run(template=t, prefix=[[4, 6, 9], [5]]))
        reaches_device(lambda: run(template=t, prefix=[[4] + [9] * (T - 5) + [6], []]))     # room for the last word
    # required words and required items: their <eos> rule and the template's do not combine
    for kw in (dict(require=[[10], []]), dict(phrases=Phrases(required=[[(10, 11)], []]))):
        with pytest.raises(ValueError, match="template: does not combine with require= or Phrases\\(required=\\)"):
            s.beam(db, 5, template=t, **kw)
    # the searches that refuse the option, whatever is in it (the inactive value passes)
    cand = np.full((2, 1, 3), START)
    for v in (t, "template"):
        for name, run in (("sample", lambda: s.sample(db, 2, template=v)), ("score", lambda: s.score(db, cand, template=v)),
                          ("sample_distinct", lambda: s.sample_distinct(db, 2, template=v)),
                          ("contrastive", lambda: s.contrastive(db, 2, template=v))):
            with pytest.raises(ValueError, match="^%s does not take a template" % name):
                run()
    Searcher._no_template("sample", None)
    Searcher._no_template("sample", Template())


def test_every_search_refuses_a_wrong_value_before_any_device_work(monkeypatch):
    def no_library():
        raise AssertionError("a library call before the refusal")
    monkeypatch.setattr(_lib, "lib", no_library)
    s = no_launch()

    def reaches_device(run):
        with pytest.raises(AssertionError, match="device work"):
            run()
    host_refusals(s, types.SimpleNamespace(B=2), reaches_device)
    assert s._ws == {}


def test_an_inactive_value_leaves_the_keys_alone():
    key = Searcher._key
    base = ("beam", 4, 3)
    assert key(base, False, None) == base and key(base, False, None, template=False) == base
    assert key(base, False, None, template=True) == base + ("template",)
    con = Constraints(min_length=2)
    assert key(base, True, con, forced=True, penalties=True, ban_phrases=True, template=True) == \
        base + ("merge", "prefix", "penalties", "ban-phrases", "template", con)
    s = no_launch()
    assert s._template(None, 2, None) is None and s._template(Template(), 2, None) is None
    t = hand_template()
    assert s._template(t, 2, None, [[4, 6], []]) is t


# ------------------------------------------------------------------------------------------------ the numpy statement by hand
DIMS, T_HAND = (10, 3, 2), 8
SOU, SUB = [4, 6, EOS], [7, 9]                                 # entries 10..12 and 13..14


def hand_mask(row, start=0, T=T_HAND):
    wc, nxt, need, st = hand_template(start).arrays(1, DIMS[0])
    gen = np.zeros(T, dtype=np.int32)
    gen[:len(row)] = row
    return TR.template_mask(gen, len(row), SOU, SUB, DIMS, wc, nxt, need, st[0])


def test_the_reference_mask_on_rows_written_out_by_hand():
    every = set(range(15))
    # <start> alone, state 0: a type word or nothing -- generator 4 and 5, and the diff slot that carries 4
    assert set(np.flatnonzero(~hand_mask([START]))) == {4, 5, 10}
    # after "type :", state 3 with room: every word but 7, and no <eos> yet -- generator 1 and 7, the diff slot with <eos>, the
    # sub-token slot with 7
    assert set(np.flatnonzero(hand_mask([START, 4, 6]))) == {1, 7, 12, 13}
    # tar_len 4, after "type": two places are left and state 2 needs two words after it, so only the colon (state 3 needs one) stays
    assert set(np.flatnonzero(~hand_mask([START, 4], T=4))) == {6, 11}
    # the same row with room: everything but <eos>
    assert set(np.flatnonzero(hand_mask([START, 4]))) == {1, 12}
    # a hypothesis that left the language: the whole row
    assert set(np.flatnonzero(hand_mask([START, 6]))) == every
    # finished: untouched
    assert not hand_mask([START, 4, 6, 9, EOS]).any()
    # an accepting state with room: <eos> is free, 7 is not
    assert set(np.flatnonzero(hand_mask([START, 4, 6, 9]))) == {7, 13}
    # the last step (len = tar_len - 1): from state 3 every transition enters the accepting state, from state 2 none does
    assert set(np.flatnonzero(hand_mask([START, 4, 9, 9, 9, 9, 6]))) == {1, 7, 12, 13}
    assert set(np.flatnonzero(hand_mask([START, 4, 9, 9, 9, 9, 9]))) == every
    # another start state: the same words from state 3
    assert set(np.flatnonzero(hand_mask([START], start=3))) == {1, 7, 12, 13}
