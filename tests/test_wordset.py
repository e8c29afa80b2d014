"""Per-commit word sets, the parts that need no GPU: the ABI, ``decode.WordSets`` (every refusal with its message, the packing of
the bit sets, the ``grounded`` builder), the searches' refusals ahead of any device work, the state keys, and the numpy statement
(wordset_ref.py) on rows written out by hand."""
import os
import re
import types

import numpy as np
import pytest

import util
import wordset_ref as WR
from test_template import no_launch
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, PAD, START, FiraConfig
from fira_icse_amd.decode import Constraints, Phrases, Searcher, WordSets, looks_like_an_identifier


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_library_exports_and_the_binding_matches():
    name, kinds = "fira_wordset_dist", "PPII" + "P" * 13
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
    assert '"wordset.hip"' in open(os.path.join(util.REPO, "fira_icse_amd", "build.py")).read()


# ------------------------------------------------------------------------------------------------ the value
def test_wordsets_value():
    off = WordSets()
    assert not off.active and off.given == ()
    assert not WordSets(deny=[], boost=[5], boost_bias=0.0, ground=[]).active       # nothing that edits anything
    assert not WordSets(boost=[], boost_bias=2.0).active
    assert WordSets(allow=[5]).given == ("allow",) and WordSets(allow=range(4, 9)).active     # a given allow is active
    v = WordSets(allow=[7, 5, 5], deny=[[9], []], boost={8}, boost_bias=[0.0, 1.5], ground=(6, 4))
    assert v.given == ("allow", "deny", "boost", "ground")
    assert v.allow == (5, 7) and v.deny == ((9,), ()) and v.boost == (8,) and v.ground == (4, 6) and v.boost_bias == (0.0, 1.5)
    assert v == WordSets(allow=(5, 7), deny=[(9,), None], boost=[np.int64(8)], boost_bias=(0, 1.5), ground=[4, 6])
    assert hash(v) == hash(WordSets(allow=(5, 7), deny=[(9,), ()], boost=[8], boost_bias=(0, 1.5), ground=[4, 6]))
    with pytest.raises(Exception):
        v.allow = ()                                           # frozen
    assert v.blocks(9, 0, 2) and v.blocks(9, 1, 2)             # denied for commit 0, and allowed for neither
    assert not v.blocks(5, 1, 2) and not v.blocks(EOS, 0, 2) and v.blocks(6, 0, 2)
    cfg = FiraConfig()
    assert v.check(cfg, 2) is v


def test_the_value_refuses_what_it_cannot_hold():
    cfg = FiraConfig()
    V, T = cfg.vocab_size, cfg.tar_len
    for kwargs, msg in ((dict(allow=5), "allow = 5 is neither an iterable"), (dict(deny=[1.5]), "deny: id 1.5 is not an integer"),
                        (dict(boost=[[4], [True]]), "boost of commit 1: id True is not an integer"),
                        (dict(ground=[[4], [5]]), "ground is one set for every commit"), (dict(ground=7), "ground = 7 is not an iterable"),
                        (dict(boost_bias="2"), "boost_bias = '2' is not a number"), (dict(boost_bias=30.5), "boost_bias = 30.5 is outside"),
                        (dict(boost_bias=[0.0, -31]), "boost_bias of commit 1 = -31 is outside"),
                        (dict(boost_bias=float("nan")), "is outside")):
        with pytest.raises(ValueError, match=msg):
            WordSets(**kwargs)
    big = 87.0 / (T - 1)
    for v, B, msg in ((WordSets(allow=[V]), 2, "allow: id %d outside the vocabulary \\[0, %d\\)" % (V, V)),
                      (WordSets(deny=[[5], [-1]]), 2, "deny of commit 1: id -1 outside the vocabulary"),
                      (WordSets(boost=[V + 7], boost_bias=1.0), 2, "boost: id %d outside" % (V + 7)),
                      (WordSets(ground=[V]), 2, "ground: id %d outside" % V),
                      (WordSets(allow=[PAD, 5]), 2, "allow: id 0 is <pad> or <start>"),
                      (WordSets(deny=[START]), 2, "deny: id 2 is <pad> or <start>"),
                      (WordSets(boost=[START], boost_bias=1.0), 2, "boost: id 2 is <pad> or <start>"),
                      (WordSets(ground=[PAD]), 2, "ground: id 0 is <pad> or <start>"),
                      (WordSets(deny=[EOS]), 2, "deny: <eos> \\(id 1\\) cannot be in deny"),
                      (WordSets(ground=[5, EOS]), 2, "ground: <eos> \\(id 1\\) cannot be in ground"),
                      (WordSets(allow=[]), 2, "allow: commit 0 is allowed no word at all"),
                      (WordSets(allow=[[5], []]), 2, "allow of commit 1: commit 1 is allowed no word at all"),
                      (WordSets(allow=[[5], [6], [7]]), 2, "allow: 3 lists for a batch of 2 commits"),
                      (WordSets(deny=[[5]]), 2, "deny: 1 lists for a batch of 2 commits"),
                      (WordSets(boost=[[5], [6], [7]], boost_bias=1.0), 2, "boost: 3 lists for a batch of 2"),
                      (WordSets(boost=[5], boost_bias=[1.0]), 2, "boost_bias: 1 values for a batch of 2 commits"),
                      (WordSets(boost=[5], boost_bias=big + 0.01), 2, "commit 0: boost_bias = .* times tar_len - 1 = %d exceeds 87" % (T - 1)),
                      (WordSets(boost=[5], boost_bias=[0.0, big + 0.01]), 2, "commit 1: boost_bias")):
        with pytest.raises(ValueError, match=msg):
            v.check(cfg, B)
    WordSets(boost=[5], boost_bias=big).check(cfg, 2)          # the bound itself
    WordSets(boost=[5], boost_bias=-30.0).check(cfg, 2)        # a negative bias cannot overflow
    WordSets(allow=[EOS], boost=[EOS], boost_bias=1.0).check(cfg, 2)       # <eos> may be allowed and boosted


# ------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("V", [33, 64, 70, 24650])
def test_packing(V):
    ids = sorted({w for w in (4, 31, 32, 63, V - 1) if w < V})
    packed = WordSets.pack([ids, [], ids[:1]], V)
    n = (V + 31) // 32
    assert packed.dtype == np.uint32 and packed.shape == (3, n)
    for w in range(V):
        assert WR.in_set(packed[0], w, V) == (w in ids), w
    assert not packed[1].any() and int(packed[2].astype(np.int64).sum()) == 1 << 4
    assert int(packed[0, (V - 1) >> 5]) >> ((V - 1) & 31) == 1                   # vocab - 1 is the highest bit set: no tail bit
    every = WordSets.pack([range(3, V)], V)[0]
    assert int(every[0]) == 0xFFFFFFF8 and all(int(x) == 0xFFFFFFFF for x in every[1:-1])
    tail = V - 32 * (n - 1)
    assert int(every[-1]) == (1 << tail) - 1 if n > 1 else True
    # bit 0 is bit 0: <pad> packs where the kernel looks for it (the value refuses it; the packing is the format)
    assert int(WordSets.pack([[0, 31, 32]], V)[0, 0]) == 0x80000001 and int(WordSets.pack([[0, 31, 32]], V)[0, 1]) & 1
    # the reference ignores tail bits: a word with every tail bit set adds no id
    dirty = packed[0].copy()
    dirty[-1] |= np.uint32((0xFFFFFFFF << tail) & 0xFFFFFFFF) if tail < 32 else np.uint32(0)
    assert [w for w in range(V + 40) if WR.in_set(dirty, w, V)] == ids


def test_arrays():
    v = WordSets(allow=[[5, 40], [6]], deny=[7], boost=[[8], []], boost_bias=[1.0, -2.0], ground=[9, 69])
    a = v.arrays(2, 70)
    assert set(a) == {"allow", "deny", "boost", "ground", "boost_factor"}
    assert a["allow"].shape == (2, 3) and a["allow"].tolist() == [[1 << 5, 1 << 8, 0], [1 << 6, 0, 0]]
    assert a["deny"].tolist() == [[1 << 7, 0, 0]] * 2 and a["boost"].tolist() == [[1 << 8, 0, 0], [0, 0, 0]]
    assert a["ground"].tolist() == [[1 << 9, 0, 1 << 5]] * 2
    assert a["boost_factor"].dtype == np.float32
    assert a["boost_factor"].tolist() == [np.float32(np.exp(np.float64(1.0))), np.float32(np.exp(np.float64(-2.0)))]
    only = WordSets(deny=[7]).arrays(3, 70)
    assert only["allow"] is None and only["boost"] is None and only["ground"] is None and only["deny"].shape == (3, 3)
    assert only["boost_factor"].tolist() == [1.0, 1.0, 1.0]


def test_the_grounded_builder_on_a_ten_word_vocabulary():
    words = ["<pad>", "<eos>", "<start>", "<unkm>", "fix", "parseArgs", "v2", "read_file", "src/main.c", "Add"]
    assert [looks_like_an_identifier(w) for w in words[4:]] == [False, True, True, True, True, False]
    v = WordSets.grounded(words)
    assert v.ground == (5, 6, 7, 8) and v.given == ("ground",) and v.allow is None
    assert WordSets.grounded(words, lambda w: w.islower(), deny=[9]).ground == (4, 6, 7, 8)
    assert WordSets.grounded(words, lambda w: True).ground == (4, 5, 6, 7, 8, 9)      # never a special id, whatever the predicate
    assert not WordSets.grounded(words[:5]).active


# ------------------------------------------------------------------------------------------------ the searches' refusals
def host_refusals(s, db, reaches_device):
    """Every refusal of the searches for ``wordsets=``, on a Searcher ``s`` and a batch of two commits."""
    V = s.cfg.vocab_size
    ok = WordSets(allow=range(3, 200), deny=[[50], [60]])
    takers = (lambda **k: s.greedy(db, **k), lambda **k: s.greedy_many([db, db], **k), lambda **k: s.beam(db, 5, **k),
              lambda **k: s.sample_search(db, 2, **k))
    for run in takers:
        with pytest.raises(ValueError, match="expected decode.WordSets"):
            run(wordsets={5, 6})
        with pytest.raises(ValueError, match="deny: 3 lists for a batch of 2 commits"):
            run(wordsets=WordSets(deny=[[5], [6], [7]]))
        with pytest.raises(ValueError, match="allow: id %d outside the vocabulary" % V):
            run(wordsets=WordSets(allow=[V]))
        with pytest.raises(ValueError, match="<eos> .* cannot be in ground"):
            run(wordsets=WordSets(ground=[EOS]))
        if run is not takers[1]:                               # (greedy_many sets up its lanes first)
            reaches_device(lambda: run(wordsets=ok))
    with pytest.raises(ValueError, match="wordsets: 3 values for 2 batches"):
        s.greedy_many([db, db], wordsets=[ok, None, ok])
    with pytest.raises(ValueError, match="expected decode.WordSets"):
        s.greedy_many([db, db], wordsets=[ok, 5])
    # a forced or required word that allow or deny blocks (ground cannot be seen here)
    for run, prefix in ((takers[0], [[70], [60]]), (takers[1], [None, [[70], [60]]]), (takers[2], [[70], [60]]),
                        (takers[3], [[70], [60]])):
        with pytest.raises(ValueError, match="wordsets: commit 1: the prefix word 60 is blocked by allow or deny"):
            run(wordsets=ok, prefix=prefix)
    with pytest.raises(ValueError, match="commit 0: the prefix word 300 is blocked"):
        s.greedy(db, wordsets=ok, prefix=[[300], []])
    with pytest.raises(ValueError, match="commit 0: the required word 50 is blocked"):
        s.beam(db, 5, wordsets=ok, require=[[50], [50]])
    with pytest.raises(ValueError, match="commit 1: the required phrase word 60 is blocked"):
        s.beam(db, 5, wordsets=ok, phrases=Phrases(required=[[], [(70, 60)]]))
    reaches_device(lambda: s.beam(db, 5, wordsets=ok, require=[[60], [50]]))
    reaches_device(lambda: s.greedy(db, wordsets=WordSets(ground=range(4, 300)), prefix=[[70], [71]]))    # ground: probability 0
    # the searches that refuse the option, whatever is in it (the inactive value passes)
    cand = np.full((2, 1, 3), START)
    for v in (ok, "wordsets"):
        for name, run in (("sample", lambda: s.sample(db, 2, wordsets=v)), ("score", lambda: s.score(db, cand, wordsets=v)),
                          ("sample_distinct", lambda: s.sample_distinct(db, 2, wordsets=v)),
                          ("contrastive", lambda: s.contrastive(db, 2, wordsets=v))):
            with pytest.raises(ValueError, match="^%s does not take word sets" % name):
                run()
    Searcher._no_wordsets("sample", None)
    Searcher._no_wordsets("sample", WordSets())
    for run in (lambda: s.sample(db, 2, wordsets=WordSets()), lambda: s.sample_distinct(db, 2, wordsets=None)):
        reaches_device(run)                                    # the inactive value is not handed on


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
    assert key(base, False, None) == base and key(base, False, None, wordsets=()) == base
    assert key(base, False, None, wordsets=("allow", "ground")) == base + (("wordsets", ("allow", "ground")),)
    con = Constraints(min_length=2)
    assert key(base, True, con, forced=True, penalties=True, template=True, wordsets=("deny",)) == \
        base + ("merge", "prefix", "penalties", "template", ("wordsets", ("deny",)), con)
    s = no_launch()
    assert s._wordsets(None, 2) is None and s._wordsets(WordSets(), 2) is None and s._wordsets(WordSets(deny=[]), 2) is None
    v = WordSets(deny=[9])
    assert s._wordsets(v, 2, [[4, 6], []]) is v


# ------------------------------------------------------------------------------------------------ the numpy statement by hand
DIMS, T_HAND = (10, 3, 2), 6
SOU, SUB = [4, 6, EOS], [7, 12]                                # entries 10..12 and 13..14; 12 is outside the vocabulary
VALID = np.array([0b10111], dtype=np.uint32)                   # the sub-token slot that carries 7 is not valid


def hand(row, dist=None, **sets):
    gen = np.zeros(T_HAND, dtype=np.int32)
    gen[:len(row)] = row
    packed = {k: WordSets.pack([v], DIMS[0])[0] for k, v in sets.items() if k != "factor"}
    dist = np.full(15, 0.5, dtype=np.float32) if dist is None else dist
    return WR.wordset_row(dist, gen, len(row), SOU, SUB, DIMS, slot_valid=VALID, factor=sets.get("factor"), **packed)


def test_the_reference_on_rows_written_out_by_hand():
    out, blk, up = hand([START], allow=[4, 5])
    # <eos> stays under allow (generator 1 and the diff slot that carries it); the slot with id 12 is in no set: blocked
    assert set(np.flatnonzero(~blk)) == {1, 4, 5, 10, 12} and not up.any() and out[blk].tolist() == [0.0] * 10
    out, blk, up = hand([START], deny=[6, 7])
    assert set(np.flatnonzero(blk)) == {6, 7, 11, 13}          # a denied word goes with its slots, valid or not; 12 is untouched
    out, blk, up = hand([START], ground=[4, 7, 8])
    # 4 is carried by a valid slot: kept, everywhere; 7 only by the invalid slot: blocked, that slot included; 8 by none
    assert set(np.flatnonzero(blk)) == {7, 8, 13}
    out, blk, up = hand([START], boost=[4, 6, 9], deny=[6], factor=np.float32(3.0))
    assert set(np.flatnonzero(up)) == {4, 9, 10} and set(np.flatnonzero(blk)) == {6, 11}
    assert out[4] == np.float32(1.5) and out[10] == np.float32(1.5) and out[6] == 0 and out[5] == np.float32(0.5)
    out, blk, up = hand([START, 5, EOS], allow=[4], deny=[5], ground=[6], boost=[4], factor=np.float32(2.0))
    assert not blk.any() and not up.any() and (out == np.float32(0.5)).all()       # finished: untouched
    nan = np.full(15, 0.5, dtype=np.float32)
    nan[[4, 6]] = np.nan
    out, blk, up = hand([START], dist=nan, deny=[6])
    assert out[6] == 0 and np.isnan(out[4]) and WR.argmax_ref(np.nan_to_num(out, nan=-np.inf))[0] == 0
