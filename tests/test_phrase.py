"""Phrases in the hard search controls, the parts that need no GPU: the ABI, ``decode.Phrases`` and every refusal of the searches
ahead of any device work, the inactive value and the state keys, and the numpy statement (phrase_ref.py) against a brute-force
substring search and against require_ref.py."""
import os
import re
import types

import numpy as np
import pytest

import phrase_ref as P
import require_ref as R
import util
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, START, UNK, FiraConfig
from fira_icse_amd.decode import BeamScoring, Constraints, Phrases, Searcher

A, B_, C_, D, E = 10, 11, 12, 13, 14          # five ordinary words


# ------------------------------------------------------------------------------------------------ ABI
@pytest.mark.parametrize("name, kinds, source", [("fira_ban_phrases_dist", "PPIIPPPPPPPPPP", "phrase.hip"),
                                                 ("fira_beam_select_phrases", "PPII" + "P" * 17, "beam_phrase.hip")])
def test_header_declares_library_exports_and_the_binding_matches(name, kinds, source):
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
    assert '"%s"' % source in open(os.path.join(util.REPO, "fira_icse_amd", "build.py")).read()


# ------------------------------------------------------------------------------------------------ decode.Phrases
def test_phrases_value():
    p = Phrases()
    assert p.banned == () and p.required == () and not p.active
    assert not Phrases(banned=[[], []]).active and not Phrases(required=[[], []]).active
    assert Phrases(banned=[(A, B_)]).ban_active and not Phrases(banned=[(A, B_)]).require_active
    assert Phrases(required=[[], [(A,)]]).require_active and not Phrases(required=[[], [(A,)]]).ban_active
    assert Phrases(banned=[[A, B_], (C_, D, E, A)]).banned == ((A, B_), (C_, D, E, A))
    assert Phrases(banned=[[], [(A, B_)]]).banned == ((), ((A, B_),))                        # one list per commit
    assert Phrases(banned=[[(UNK, A)]] * 2).banned_rows(2) == [((UNK, A),), ((UNK, A),)]    # <unkm> can be banned
    assert Phrases(banned=[(A, B_)]).banned_rows(3) == [((A, B_),)] * 3
    assert Phrases(banned=[(np.int64(A), np.int32(B_))]) == Phrases(banned=[(A, B_)])
    assert hash(Phrases(required=[[[A, B_]]])) == hash(Phrases(required=[[(A, B_)]]))
    assert Phrases(banned=[(UNK + q, A) for q in range(8)]).ban_active                       # eight phrases
    assert Phrases(required=[[(A,), (B_,), (C_,), (D,)], [(A, B_, C_, D)], [(A, B_), (B_, C_)]]).require_active
    with pytest.raises(Exception):
        p.banned = ()                                                                        # frozen
    words, lens, n = Phrases(banned=[[], [(A, B_), (C_, D, E)]]).banned_arrays(2)
    assert words.shape == (2, 8, 4) and words.dtype == np.int32 and n.tolist() == [0, 2]
    assert words[1, 0].tolist() == [A, B_, 0, 0] and words[1, 1].tolist() == [C_, D, E, 0] and lens[1].tolist() == [2, 3] + [0] * 6
    words, lens, n = Phrases(required=[[(A, B_, C_), (D,)], []]).required_arrays(2)
    assert words.tolist() == [[A, B_, C_, D], [0] * 4] and lens.tolist() == [[3, 1, 0, 0], [0] * 4] and n.tolist() == [2, 0]


@pytest.mark.parametrize("kw, word", [
    (dict(banned=5), "not a sequence"), (dict(banned=[5]), "neither a list of phrases"),
    (dict(banned=[(A,)]), "one word.*Constraints.banned"), (dict(banned=[[(A, B_)], [(C_,)]]), "commit 1.*Constraints.banned"),
    (dict(banned=[(A, B_, C_, D, E)]), "5 words, outside 2..4"), (dict(banned=[(A, 2.5)]), "not an integer"),
    (dict(banned=[(A, True)]), "not an integer"), (dict(banned=[(A, START)]), "id 2 is below 3"), (dict(banned=[(EOS, A)]), "below"),
    (dict(banned=[(A, B_), (A, B_)]), "listed twice"), (dict(banned=[[], [(A, B_), [A, B_]]]), "commit 1.*listed twice"),
    (dict(banned=[(UNK + q, A) for q in range(9)]), "9 phrases, more than 8"),
    (dict(required=5), "one list of items per commit"), (dict(required=[5]), "one list of items per commit"),
    (dict(required=[[A]]), "not an item"), (dict(required=[[()]]), "0 words, outside 1..4"),
    (dict(required=[[(A, B_, C_, D, E)]]), "5 words, outside 1..4"), (dict(required=[[(A, "b")]]), "not an integer"),
    (dict(required=[[(UNK,)]]), "id 3 is below 4"), (dict(required=[[], [(A,), (B_,), (C_,), (D,), (E,)]]), "commit 1: 5 items"),
    (dict(required=[[(A, B_, C_), (D, E)]]), "5 words in all, more than 4"),
    (dict(required=[[(A, B_), (A, B_)]]), "duplicates"), (dict(required=[[(A, B_, C_), (B_,)]]), r"\(11,\) is part of"),
    (dict(required=[[(C_,), (B_, C_)]]), r"\(12,\) is part of \(11, 12\)"),
])
def test_phrases_refuses_bad_values(kw, word):
    with pytest.raises(ValueError, match=word):
        Phrases(**kw)


def no_launch():
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


@pytest.fixture
def searcher(monkeypatch):
    def no_library():
        raise AssertionError("a library call before the refusal")
    monkeypatch.setattr(_lib, "lib", no_library)
    return no_launch(), types.SimpleNamespace(B=2)


def test_every_search_refuses_a_wrong_value_before_any_device_work(searcher):
    s, db = searcher
    V = s.cfg.vocab_size
    takers = (lambda **k: s.greedy(db, **k), lambda **k: s.greedy_many([db, db], **k), lambda **k: s.beam(db, 5, **k),
              lambda **k: s.sample_search(db, 2, **k))
    for run in takers:
        with pytest.raises(ValueError, match="expected decode.Phrases"):
            run(phrases=[(A, B_)])
        with pytest.raises(ValueError, match="3 lists of banned phrases for a batch of 2"):
            run(phrases=Phrases(banned=[[(A, B_)], [], []]))
        with pytest.raises(ValueError, match="commit 1: banned id %d outside the vocabulary" % V):
            run(phrases=Phrases(banned=[[], [(A, V)]]))
        if run is not takers[1]:                                           # (greedy_many sets up its lanes first)
            with pytest.raises(AssertionError, match="device work"):      # an accepted value reaches the device
                run(phrases=Phrases(banned=[(A, B_)]))
    # a prefix that contains a banned phrase (greedy_many: one prefix argument per batch)
    bad = [[C_, A, B_], []]
    for run, prefix in ((takers[0], bad), (takers[1], [None, bad]), (takers[2], bad), (takers[3], bad)):
        with pytest.raises(ValueError, match=r"commit 0: the prefix contains the banned phrase \(10, 11\)"):
            run(phrases=Phrases(banned=[(A, B_)]), prefix=prefix)
        if run is not takers[1]:
            with pytest.raises(AssertionError, match="device work"):      # the words apart are no phrase
                run(phrases=Phrases(banned=[(A, B_)]), prefix=[[A, C_, B_], []])
    # required items: the beam alone
    req = Phrases(required=[[(A, B_)], []])
    for run, name in zip((takers[0], takers[1], takers[3]), ("greedy", "greedy_many", "sample_search")):
        with pytest.raises(ValueError, match="%s does not take required items" % name):
            run(phrases=req)
    # the searches that refuse the option, whatever is in it (an inactive value passes, as an inactive Penalties does)
    cand = np.full((2, 1, 3), START)
    for p in (Phrases(banned=[(A, B_)]), req, "phrases"):
        for name, run in (("sample", lambda: s.sample(db, 2, phrases=p)), ("score", lambda: s.score(db, cand, phrases=p)),
                          ("sample_distinct", lambda: s.sample_distinct(db, 2, phrases=p)),
                          ("contrastive", lambda: s.contrastive(db, 2, phrases=p))):
            with pytest.raises(ValueError, match="^%s does not take phrases" % name):
                run()
    Searcher._no_phrases("sample", None)
    Searcher._no_phrases("sample", Phrases())
    Searcher._no_phrases("sample", Phrases(banned=[[], []], required=[[], []]))
    assert s._ws == {}


def test_the_beam_refuses_required_items_it_cannot_serve(searcher):
    s, db = searcher
    T = s.cfg.tar_len
    beam = lambda k=5, **kw: s.beam(db, k, **kw)
    item3 = Phrases(required=[[(A, B_, C_)], []])
    with pytest.raises(ValueError, match="3 lists of required items for a batch of 2"):
        beam(phrases=Phrases(required=[[(A,)], [], []]))
    with pytest.raises(ValueError, match="required id %d outside the vocabulary" % s.cfg.vocab_size):
        beam(phrases=Phrases(required=[[(A, s.cfg.vocab_size)], []]))
    with pytest.raises(ValueError, match="commit 0: 3 required words need a beam of at least 4 .*beam = 3"):
        beam(3, phrases=item3)
    with pytest.raises(ValueError, match="commit 1: 4 required words need a beam of at least 5"):
        beam(4, phrases=Phrases(required=[[(A,)], [(A, B_), (C_, D)]]))
    with pytest.raises(ValueError, match="beam = 1, but required items need a beam of at least 2"):
        beam(1, phrases=Phrases(required=[[(A,)], []]))
    with pytest.raises(ValueError, match="do not combine with require="):
        beam(phrases=item3, require=[[D], []])
    with pytest.raises(ValueError, match="do not combine with an active scoring"):
        beam(6, phrases=item3, scoring=BeamScoring(length_alpha=0.6))
    with pytest.raises(ValueError, match=r"the required item \(10, 11, 12\) holds id 11, which the constraints ban"):
        beam(phrases=item3, constraints=Constraints(banned=(B_,)))
    with pytest.raises(ValueError, match=r"the required item \(10, 11, 12\) contains the banned phrase \(11, 12\)"):
        beam(phrases=Phrases(banned=[(B_, C_)], required=item3.required))
    with pytest.raises(ValueError, match=r"commit 1: the required item \(10, 11\) contains the banned phrase"):
        beam(phrases=Phrases(banned=[[], [(A, B_)]], required=[[(A, B_)], [(A, B_)]]))
    with pytest.raises(ValueError, match="itself repeats a 1-gram"):
        beam(phrases=Phrases(required=[[(A, B_, A)], []]), constraints=Constraints(no_repeat_ngram=1))
    with pytest.raises(ValueError, match="itself repeats a 2-gram"):
        beam(phrases=Phrases(required=[[(A, A, A)], []]), constraints=Constraints(no_repeat_ngram=2))
    short = no_launch()
    short.cfg = FiraConfig(tar_len=5)
    with pytest.raises(ValueError, match="4 required words, more than tar_len - 2 = 3"):
        short.beam(db, 5, phrases=Phrases(required=[[(A, B_, C_, D)], []]))
    assert s._ws == {} and short._ws == {}
    # what is allowed reaches the device: require= with every list empty, an inactive scoring, a banned phrase beside the item
    for kw in (dict(require=[[], []]), dict(scoring=BeamScoring()), dict(constraints=Constraints(no_repeat_ngram=2)),
               dict(prefix=[[A, B_], []])):
        with pytest.raises(AssertionError, match="device work"):
            beam(phrases=Phrases(banned=[(C_, A)], required=item3.required), **kw)
    assert T == 30


def test_an_inactive_value_leaves_the_keys_alone():
    key = Searcher._key
    base = ("beam", 4, 3)
    assert key(base, False, None) == base
    assert key(base, False, None, ban_phrases=True) == base + ("ban-phrases",)
    assert key(base, True, Constraints(min_length=2), None, True, require=False, penalties=True, ban_phrases=True,
               require_phrases=True) == base + ("merge", "prefix", "penalties", "ban-phrases", "require-phrases",
                                                Constraints(min_length=2))
    s = no_launch()
    for p in (None, Phrases(), Phrases(banned=[[], []], required=[[], []])):
        assert s._phrases(p, 2, None, "beam", None, 3) == (None, None)
    ban, req = s._phrases(Phrases(banned=[(A, B_)]), 2, None, "beam", None, 3)
    assert ban is not None and req is None
    st = s._edit_state(lambda *a: a, lambda *a: a, 6, 2, None, False, None)
    assert set(st) == {"con"}                                                                # today's state
    st = s._edit_state(lambda *a: a, lambda *a: a, 6, 2, None, False, None, ban=ban)
    assert set(st) == {"con", "dist", "ban-phrases", "ban_phrase", "ban_phrase_len", "n_ban_phrases"}
    assert st["ban_phrase"] == (2, 8, 4) and st["ban_phrase_len"] == (2, 8) and st["n_ban_phrases"] == (2,)


# ------------------------------------------------------------------------------------------------ the reference itself
def brute_progress(h, items):
    """progress by string search: a hypothesis and an item as strings over one character per id."""
    s = "".join(chr(65 + w) for w in h)
    pats = ["".join(chr(65 + w) for w in item) for item in items]
    done = [s.find(p) >= 0 for p in pats]
    partial = max([q for p, d in zip(pats, done) if not d for q in range(1, len(p)) if s.endswith(p[:q])] + [0])
    return sum(len(p) for p, d in zip(pats, done) if d) + partial


ITEM_SETS = [[], [[1, 2]], [[1, 1, 2], [3]], [[1, 2], [2, 3]], [[1], [2], [3], [4]], [[1, 1, 1, 2]], [[1, 2, 1], [0]], [[0, 0], [0, 1]]]


def test_progress_equals_a_brute_force_substring_search():
    rng = np.random.RandomState(0)
    seen = set()
    for items in ITEM_SETS:
        total = sum(len(i) for i in items)
        for _ in range(400):
            h = rng.randint(0, 5, size=rng.randint(0, 9)).tolist()           # five ids: overlaps happen, partial matches restart
            got = P.progress(h, items)
            assert got == brute_progress(h, items), (h, items)
            assert 0 <= got <= total
            seen.add((ITEM_SETS.index(items), got))
    assert {(2, q) for q in range(5)} <= seen and {(5, q) for q in range(5)} <= seen      # every bank is reached


def test_progress_by_hand():
    assert P.progress([1, 1], [[1, 1, 2]]) == 2 and P.progress([1, 1, 1], [[1, 1, 2]]) == 2     # a partial match restarts
    assert P.progress([1, 1, 3], [[1, 1, 2]]) == 0 and P.progress([1, 1, 2, 3], [[1, 1, 2]]) == 3  # broken off; done stays
    assert P.progress([1, 2], [[1, 2], [2, 3]]) == 3 and P.progress([1, 2, 3], [[1, 2], [2, 3]]) == 4   # a shared word
    assert P.progress([3, 1], [[1, 2], [1, 2, 3]][:1]) == 1
    assert P.blocked_by_phrases([5, 6], [[6, 7], [5, 6, 8], [5, 9], [4, 5, 6, 3]]) == {7, 8}
    assert P.blocked_by_phrases([], [[6, 7]]) == set() and P.blocked_by_phrases([6], [[6, 7], [5, 6, 8]]) == {7}


def test_progress_of_one_word_items_is_the_met_count():
    rng = np.random.RandomState(1)
    for _ in range(300):
        req = rng.permutation(np.arange(4, 10))[:rng.randint(0, 5)].tolist()
        gen = np.concatenate([[START], rng.randint(4, 10, size=7)])
        length = rng.randint(1, 9)
        assert P.progress(P.hyp(gen, length), [[w] for w in req]) == len(R.met_set(gen, length, req)) \
            == R.count_met(gen[:length], req)


# ------------------------------------------------------------------------------------------------ scripts/phrase_probe.py
def probe():
    import importlib.util
    spec = importlib.util.spec_from_file_location("phrase_probe", os.path.join(util.REPO, "scripts", "phrase_probe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_probe_options_parse_and_phrases_are_tokenised_mapped_and_dropped(capsys, tmp_path):
    pp = probe()
    a = pp.parse_args(["--root", "x"])
    assert (a.beam, a.ban_phrases, a.require_phrases, a.require_phrase_file, a.reps) == (3, None, None, None, 20)
    assert pp.parse_phrases("minor changes, fix bug ,,abc-123") == [["minor", "changes"], ["fix", "bug"], ["abc", "-", "123"]]
    assert pp.parse_phrases(None) == [] and pp.parse_phrases("Foo.bar") == [["Foo", ".", "bar"]]
    vocab = {"<pad>": 0, "<eos>": EOS, "<start>": START, "<unkm>": UNK, "fix": 4, "bug": 5, "minor": 6, "changes": 7, "abc": 8,
             "-": 9, "123": 10, "VAR0": 11, "revert": 12}
    maps = [{}, {"fooBar": "VAR0"}]                                         # commit 1 knows the identifier fooBar
    assert pp.phrase_ids(["fix", "fooBar"], vocab, maps[0]) is None and pp.phrase_ids(["fix", "fooBar"], vocab, maps[1]) == (4, 11)
    assert pp.phrase_ids(["abc", "-", "123"], vocab, {}) == (8, 9, 10)
    assert pp.phrase_ids(["fix", "\U0001F605"], vocab, {}) is None          # the emoji of <unkm> is no vocabulary word
    a = pp.parse_args(["--root", "x", "--beam", "5", "--ban-phrases", "minor changes,fix fooBar,fix,nosuch word,minor  changes",
                       "--require-phrases", "abc-123,revert"])
    p, dropped = pp.phrases_from_args(a, vocab, maps)
    assert p.banned == (((6, 7),), ((6, 7), (4, 11)))                       # per commit; the repeated phrase once
    assert p.required == (((8, 9, 10), (12,)),) * 2
    assert dropped == 1 + 2 + 2                                             # "fix fooBar" for commit 0; "fix", "nosuch word" for both
    p.check(FiraConfig(), 2)
    path = str(tmp_path / "items")
    with open(path, "w") as f:
        f.write("revert\n\n")
    a = pp.parse_args(["--root", "x", "--require-phrase-file", path])
    p, dropped = pp.phrases_from_args(a, vocab, maps)
    assert p.required == (((12,),), ()) and p.banned == () and dropped == 0
    with pytest.raises(ValueError, match="2 lines for 3 test commits"):
        pp.phrases_from_args(a, vocab, maps + [{}])
    assert not pp.phrases_from_args(pp.parse_args(["--root", "x"]), vocab, maps)[0].active
    assert pp.holds_all([4, 8, 9, 10, 12], [(8, 9, 10), (12,)]) and not pp.holds_all([8, 9, 4, 10, 12], [(8, 9, 10), (12,)])
    for argv, word in ((["--beam", "0"], "1..8"), (["--beam", "9"], "1..8"), (["--reps", "2"], "--reps"),
                       (["--require-phrases", "a", "--require-phrase-file", path], "mutually exclusive"),
                       (["--require-phrase-file", path + ".no"], "no such file"), (["--beam", "1", "--require-phrases", "a"], "banks"),
                       (["--ban-phrases", " , "], "no phrase given"), (["--require-phrases", "abc-123"], "need --beam 4"),
                       (["--beam", "8", "--require-phrases", "a b c d e"], "outside 1..4"),
                       (["--beam", "8", "--require-phrases", "a b c,d e"], "5 words in all"),
                       (["--ban-phrases", "a b c d e"], "outside 2..4"),
                       (["--ban-phrases", ",".join("w%d x" % k for k in range(9))], "9 phrases, more than 8")):
        with pytest.raises(SystemExit) as e:
            pp.parse_args(["--root", "x"] + argv)
        assert e.value.code == 2
        assert word in capsys.readouterr().err.strip().split("\n")[-1], (argv, word)
