"""Required words in the beam search, the parts that need no GPU: the numpy statement (require_ref.py) on hand-made steps, every
``ValueError`` of ``Searcher.beam(require=)`` (raised before anything is launched: the Searcher here has no model and no device),
the state keys, the library's own refusals, and the command line."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import util
from search_kit import device_dims as dims
import require_ref as R
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, PAD, START, UNK, FiraConfig
from fira_icse_amd.decode import MAX_REQUIRED, BeamScoring, Constraints, Searcher
from run_model import check_require_args, nbest_record, parse_args, read_require_lines, required_from_args, required_summary

A, B_, C_, D, E = 10, 11, 12, 13, 14       # five ordinary words


# ------------------------------------------------------------------------------------------------ the reference on hand-made steps
V, L, S, T = 9, 2, 1, 6                    # W = 12


def hand_step(beam, rows, prob, hyps, sou=(5, 6), sub=(7,), fin=None):
    """dist [beam, W] from {slot: {entry: value}}, hypotheses from word lists (a trailing EOS finishes one)."""
    dist = np.zeros((beam, V + L + S), dtype=np.float32)
    for j, row in rows.items():
        for i, v in row.items():
            dist[j, i] = v
    gen = np.zeros((beam, T), dtype=np.int64)
    length = np.zeros(beam, dtype=np.int64)
    for j, h in enumerate(hyps):
        gen[j, 0] = START
        gen[j, 1:1 + len(h)] = h
        length[j] = 1 + len(h)
    fin = np.array([len(h) > 0 and h[-1] == EOS for h in hyps]) if fin is None else np.asarray(fin)
    active = np.ones(beam, dtype=np.int64)
    return dict(dist=dist, fin=fin, active=active, prob=np.asarray(prob, dtype=np.float32), length=length, gen=gen,
                words=R.words_of(sou, sub, V))


def picks_of(st, req):
    return R.select(st["dist"], st["fin"], st["active"], st["prob"], st["length"], st["gen"], st["words"], req)


def test_even_share_with_overflow():
    """Beam 5, two required words (5 and 8): bank 2 has one candidate, bank 1 three, bank 0 many.  Round robin: 2, 1, 0, then
    bank 2 is dry and its share goes on: 1, 0."""
    rows = {0: {8: 0.01, 2: 0.5, 3: 0.4, 4: 0.3},            # h_0 holds 5: entry 8 completes the pair (bank 2); the rest bank 1
            1: {2: 0.9, 3: 0.8, 4: 0.7, 6: 0.6, 8: 0.05}}    # h_1 holds nothing: entry 8 is bank 1, the rest bank 0
    st = hand_step(5, rows, [0.5, 1.0, 0, 0, 0], [[5], [4], [], [], []])
    st["active"][2:] = 0
    picks = picks_of(st, [5, 8])
    got = [(p["bank"], p["src"], p["entry"], p["phase"]) for p in picks]
    # picks in pick order: (2: 0/8) (1: 0/2 = .25) (0: 1/2 = .9) (1: 0/3 = .2) (0: 1/3 = .8); written bank descending, p descending
    assert got == [(2, 0, 8, 1), (1, 0, 2, 1), (1, 0, 3, 1), (0, 1, 2, 1), (0, 1, 3, 1)]
    f = np.float32
    assert [p["p"] for p in picks] == [f(0.01) * f(0.5), f(0.5) * f(0.5), f(0.4) * f(0.5), f(0.9), f(0.8)]
    g, l, p, parent, met = R.apply(picks, st["gen"], st["length"])
    assert met.tolist() == [2, 1, 1, 0, 0] and parent.tolist() == [0, 0, 0, 1, 1]
    assert g[0, :3].tolist() == [START, 5, 8] and l.tolist() == [3, 3, 3, 3, 3]
    assert [R.count_met(g[o, :l[o]], [5, 8]) for o in range(5)] == met.tolist()


def test_a_copy_slot_promotes_like_the_generator_entry():
    """Word 5 is required and sou[0] carries it: entry V + 0 is in bank 1 beside generator entry 5."""
    st = hand_step(2, {0: {2: 0.6, 5: 0.1, V: 0.2, V + 1: 0.05}}, [1.0, 0.0], [[], []])
    picks = picks_of(st, [5])
    assert [(p["bank"], p["entry"], p["word"]) for p in picks] == [(1, V, 5), (0, 2, 2)]
    st = hand_step(3, {0: {2: 0.6, 5: 0.1, V: 0.2, V + 1: 0.05}}, [1.0, 0.0, 0.0], [[], [], []])
    assert [(p["bank"], p["entry"]) for p in picks_of(st, [5])] == [(1, V), (1, 5), (0, 2)]


def test_no_required_word_is_a_plain_top_k():
    rng = np.random.RandomState(0)
    st = hand_step(4, {}, [0.7, 0.2, 0.0, 0.5], [[2], [3, EOS], [4], [6, 2]])
    st["dist"][:] = rng.uniform(0.01, 1.0, size=st["dist"].shape).astype(np.float32)
    st["dist"][0, 3] = st["dist"][0, 7]                                         # a tie: the index decides
    flat = []
    for k, j in enumerate([0, 1, 2, 3]):
        flat += [(-1.0 if st["fin"][j] else float(np.float32(st["dist"][j, i]) * np.float32(st["prob"][j])), k * 12 + i)
                 for i in range(12)]
    flat += [(float(st["prob"][1]), 4 * 12 + 0)] + [(-1.0, 4 * 12 + q) for q in (1, 2, 3)]
    want = sorted(flat, key=lambda c: (-c[0], c[1]))[:4]
    picks = picks_of(st, [])
    assert [p["index"] for p in picks] == [i for _, i in want]
    assert [float(p["p"]) for p in picks] == [v for v, _ in want]
    assert all(p["bank"] == 0 for p in picks)


def test_eos_is_blocked_below_the_count():
    """<eos> through the generator (entry 1) and through a copy slot that carries id 1, while a word is missing."""
    rows = {0: {EOS: 0.9, V + 1: 0.8, 2: 0.1, 5: 0.001}, 1: {EOS: 0.7, 2: 0.2}}
    st = hand_step(2, rows, [1.0, 1.0], [[3], [5]], sou=(5, EOS))
    picks = picks_of(st, [5])
    # h_0 lacks the word: both its <eos> entries are void; h_1 holds it and may end
    assert [(p["bank"], p["src"], p["word"]) for p in picks] == [(1, 1, EOS), (0, 0, 2)]
    c = R.candidates(st["dist"], st["fin"], st["active"], st["prob"], st["length"], st["gen"], st["words"], [5])
    assert np.flatnonzero(c["void"]).tolist() == [EOS, V + 1, 24, 25]            # and the carried list's padding
    assert [(p["src"], p["word"]) for p in picks_of(st, [])] == [(0, EOS), (0, EOS)]          # without words nothing is blocked


def test_zero_probability_slots_never_take_a_bank_slot():
    """Step 0: slot 0 alone is alive.  The rows of the other slots hold the required word (bank 1) at probability 0: phase 1
    passes them over, and phase 2 fills by index (entry 1 is <eos>, void while the word is missing)."""
    row = {2: 0.5, 3: 0.3, 5: 0.0}
    st = hand_step(4, {0: row, 1: {5: 0.9}, 2: {5: 0.9}, 3: {5: 0.9}}, [1.0, 0.0, 0.0, 0.0], [[], [], [], []])
    picks = picks_of(st, [5])
    assert [(p["phase"], p["bank"], p["src"], p["entry"]) for p in picks] == [(1, 0, 0, 2), (1, 0, 0, 3), (2, 0, 0, 0), (2, 0, 0, 4)]
    assert [p["p"] for p in picks] == [np.float32(0.5), np.float32(0.3), 0.0, 0.0]


def test_finished_hypotheses_are_carried_in_their_bank():
    st = hand_step(3, {0: {2: 0.5, 5: 0.01}}, [0.4, 0.3, 0.25], [[3], [5, EOS], [4, EOS]])
    picks = picks_of(st, [5])
    assert [(p["carry"], p["bank"], p["src"]) for p in picks] == [(True, 1, 1), (False, 1, 0), (True, 0, 2)]
    g, l, p, parent, met = R.apply(picks, st["gen"], st["length"])
    assert l.tolist() == [3, 3, 3] and list(p) == [np.float32(0.3), np.float32(0.01) * np.float32(0.4), np.float32(0.25)]
    assert R.required_of([5, 8, 0, 0], 9) == [5, 8, 0, 0] and R.required_of([5, 8, 0, 0], -2) == []       # the clamp


# ------------------------------------------------------------------------------------------------ ABI and the library's refusals
def test_header_declares_and_library_exports_the_entry():
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    assert re.search(r"\bint\s+fira_beam_select_required\s*\(", header)
    assert "#define FIRA_ABI_VERSION 11" in header
    lib = _lib.lib()
    assert lib.fira_abi_version() == 11 and hasattr(lib, "fira_beam_select_required")
    assert len(_lib.SIGNATURES["fira_beam_select_required"][1]) == len(_lib.SIGNATURES["fira_beam_select"][1]) + 3


BAD_CALLS = {
    "beam 1": (dict(beam=1), "n_beam"),
    "beam 9": (dict(beam=9), "n_beam"),
    "tar_len 65": (dict(d=dims(tar_len=65)), "tar_len"),
    "vocabulary 8": (dict(d=dims(vocab=8)), "vocabulary"),
    "vocabulary 25601": (dict(d=dims(vocab=25601)), "vocabulary"),
    "too many memory slots": (dict(d=dims(sou_len=900, sub_len=125)), "memory slots"),
    "no commit": (dict(B=0), "B = 0"),
    "null required": (dict(null=17), "null pointer"),
    "null n_required": (dict(null=18), "null pointer"),
    "null dist": (dict(null=4), "null pointer"),
}


@pytest.mark.parametrize("name", sorted(BAD_CALLS))
def test_argument_checks_fire_before_any_launch(name):
    """Pointers that are never dereferenced: every case fails a check."""
    kw, word = BAD_CALLS[name]
    args = [None, C.byref(kw.get("d", dims())), kw.get("B", 2), kw.get("beam", 3)] + [C.c_void_p(16)] * 16
    if "null" in kw:
        args[kw["null"]] = None
    assert _lib.lib().fira_beam_select_required(*args) != 0
    msg = _lib.lib().fira_last_error().decode()
    assert "fira_beam_select_required" in msg and word in msg, msg


# ------------------------------------------------------------------------------------------------ Searcher: the ValueErrors
def bare_searcher(**cfg):
    """A Searcher with a geometry and nothing else: any launch, workspace or model access raises AttributeError, so a
    ValueError from it was raised before anything was launched."""
    s = Searcher.__new__(Searcher)
    s.cfg = FiraConfig(**cfg)
    s._ws = {}
    s.members = ()
    return s


CFG = FiraConfig()
BAD_REQUIRE = {
    "too few sequences": (dict(require=[[A]]), "1 sequences for a batch of 2"),
    "too many sequences": (dict(require=[[A], [], [B_]]), "3 sequences for a batch of 2"),
    "not a sequence of sequences": (dict(require=[A, B_]), "sequence"),
    "a float id": (dict(require=[[A], [B_, 4.0]]), "commit 1.*not an integer"),
    "a string id": (dict(require=[["fix"], []]), "commit 0.*not an integer"),
    "a bool id": (dict(require=[[True], []]), "commit 0.*not an integer"),
    "<unkm>": (dict(require=[[A, UNK], []]), "commit 0.*cannot be required"),
    "<eos>": (dict(require=[[], [EOS]]), "commit 1.*cannot be required"),
    "<start>": (dict(require=[[START], []]), "commit 0.*cannot be required"),
    "<pad>": (dict(require=[[PAD], []]), "commit 0.*cannot be required"),
    "negative id": (dict(require=[[], [-1]]), "commit 1.*outside"),
    "id at the vocabulary size": (dict(require=[[CFG.vocab_size], []]), "commit 0.*outside"),
    "a duplicate": (dict(require=[[], [A, B_, A]]), "commit 1.*%d is listed twice" % A),
    "five words": (dict(require=[[A, B_, C_, D, E], []], beam=8), "commit 0.*5 words, more than 4"),
    "beam 1": (dict(require=[[A], []], beam=1), "beam of at least 2"),
    "beam below words + 1": (dict(require=[[A], [A, B_, C_]], beam=3), "commit 1.*3 words need a beam of at least 4"),
    "a banned word": (dict(require=[[A, B_], []], constraints=Constraints(banned=(B_,))), "commit 0.*%d is banned" % B_),
    "an active scoring": (dict(require=[[A], []], beam=4, scoring=BeamScoring(1.0, 2, 0.5)), "scoring"),
}


@pytest.mark.parametrize("name", sorted(BAD_REQUIRE))
def test_beam_refuses_bad_required_words_before_anything_is_launched(name):
    kw, word = BAD_REQUIRE[name]
    kw = dict(kw)
    s, db = bare_searcher(), types.SimpleNamespace(B=2)
    with pytest.raises(ValueError, match=word):
        s.beam(db, kw.pop("beam", 3), **kw)


def test_more_words_than_the_message_has_room_for():
    s, db = bare_searcher(tar_len=5), types.SimpleNamespace(B=1)
    with pytest.raises(ValueError, match="commit 0.*4 words, more than tar_len - 2 = 3"):
        s.beam(db, 5, require=[[A, B_, C_, D]])


def test_what_the_checks_let_through_and_the_keys():
    s = bare_searcher()
    assert s._required_rows(None, 2, 3, None, None) is None
    assert s._required_rows([[], ()], 2, 3, None, None) is None                  # all empty: inactive
    assert s._required_rows([[], []], 2, 1, None, BeamScoring(1.0)) is None      # ... whatever else is given
    got = s._required_rows([np.array([A, B_]), [np.int32(C_)]], 2, 3, Constraints(banned=(D,)), None)
    assert got == [[A, B_], [C_]] and all(type(w) is int for row in got for w in row)
    assert s._required_rows([[UNK + 1, CFG.vocab_size - 1, A, B_], []], 2, 5, None, None)[0][:2] == [UNK + 1, CFG.vocab_size - 1]
    assert MAX_REQUIRED == 4
    # the state key: a marker, not the words; without it today's key, and the positional arguments as they were
    c = Constraints(1)
    assert Searcher._key(("beam", 2, 3), False, None, require=True) == ("beam", 2, 3, "require")
    assert Searcher._key(("beam", 2, 3), True, c, None, True, require=True) == ("beam", 2, 3, "merge", "prefix", "require", c)
    assert Searcher._key(("beam", 2, 3), True, c, None, True) == ("beam", 2, 3, "merge", "prefix", c)
    assert Searcher._key(("beam", 2, 3), False, None) == ("beam", 2, 3) == Searcher._key(("beam", 2, 3), False, None, require=False)
    with pytest.raises(TypeError):
        Searcher._key(("beam", 2, 3), False, None, None, False, True)            # the marker is a keyword, never positional


def test_the_other_searches_do_not_take_the_argument():
    s, db = bare_searcher(), types.SimpleNamespace(B=2)
    for call in (lambda: s.greedy(db, require=[[A], []]), lambda: s.greedy_many([db], require=[[[A], []]]),
                 lambda: s.sample(db, 2, require=[[A], []]), lambda: s.sample_distinct(db, 2, require=[[A], []]),
                 lambda: s.score(db, [[START, A, EOS]] * 2, require=[[A], []])):
        with pytest.raises(TypeError):
            call()


def test_best_required_ranks_by_positive_then_met_then_probability_then_slot():
    import torch
    s = bare_searcher()
    gen = torch.arange(2 * 4 * 5).view(2, 4, 5)
    length = torch.tensor([[2, 3, 4, 5], [5, 4, 3, 2]])
    prob = torch.tensor([[0.0, 0.5, 0.1, 0.1], [0.0, 0.0, 0.0, 0.0]])
    met = torch.tensor([[3, 1, 2, 2], [0, 1, 1, 0]])
    got = s.best_required(gen, length, prob, met)
    assert got == [gen[0, 2, :4].tolist(), gen[1, 1, :4].tolist()]


# ------------------------------------------------------------------------------------------------ command line
VOCAB = {"<pad>": PAD, "<eos>": EOS, "<start>": START, "<unkm>": UNK, "fix": 4, "the": 5, "update": 6, "VAR0": 7, "bug": 8, "a": 9}


def test_cli_options_parse_and_the_options_off_namespace_is_unchanged(tmp_path):
    off = vars(parse_args(["test"]))
    assert off.pop("require_words") is None and off.pop("require_file") is None
    on = vars(parse_args(["test", "--require-words", "fix,the"]))
    assert on.pop("require_words") == "fix,the" and on.pop("require_file") is None
    assert on == off and off["beam"] == 3 and off["prefix"] is None          # nothing else moves, in either direction
    assert required_from_args(parse_args(["test"]), VOCAB, [{}, {}], 30) == (None, 0)
    path = tmp_path / "words"
    path.write_text("fix\n\nupdate the\n")
    a = parse_args(["test", "--require-file", str(path), "--beam", "5", "--merge-copies", "--no-repeat-ngram", "2", "--nbest",
                    "--min-length", "2", "--ban-words", "the", "--prefix", "fix"])
    assert a.require_file == str(path) and a.require_words is None and a.beam == 5


def test_cli_words_become_ids_through_the_commits_variable_map(tmp_path):
    maps = [{}, {"counter": "VAR0"}, {}]
    a = parse_args(["test", "--require-words", "fix,counter,nosuchword,fix", "--beam", "4"])
    ids, n_dropped = required_from_args(a, VOCAB, maps, 30)
    assert ids == [[4], [4, 7], [4]]                           # counter exists for commit 1 alone; the second fix collapses
    assert n_dropped == 2 + 1 + 2
    path = tmp_path / "words"
    path.write_text("fix the\n\n  update   counter the update <eos>\n")
    ids, n_dropped = required_from_args(parse_args(["test", "--require-file", str(path), "--beam", "4"]), VOCAB, maps, 30)
    assert ids == [[4, 5], [], [6, 5]] and n_dropped == 2      # counter is unknown for commit 2; <eos> cannot be required
    assert read_require_lines(str(path), 3) == ["fix the", "", "  update   counter the update <eos>"]
    assert required_summary([[START, 4, 5, EOS], [START, 9], [START, 5, EOS]], ids) == (2, 1)


def test_cli_wrong_line_count_too_many_words_and_too_small_a_beam_are_named(tmp_path):
    path = tmp_path / "words"
    path.write_text("fix\nthe\n")
    a = parse_args(["test", "--require-file", str(path)])
    with pytest.raises(ValueError, match="2 lines for 3 test commits"):
        required_from_args(a, VOCAB, [{}, {}, {}], 30)
    path.write_text("fix\nfix the update bug a\n\n")
    with pytest.raises(ValueError, match="line 2.*5 words, more than 4"):
        required_from_args(parse_args(["test", "--require-file", str(path), "--beam", "8"]), VOCAB, [{}, {}, {}], 30)
    path.write_text("fix\nfix the fix update the bug\n\n")             # six words, four after collapsing
    b8 = parse_args(["test", "--require-file", str(path), "--beam", "8"])
    assert required_from_args(b8, VOCAB, [{}, {}, {}], 30)[0] == [[4], [4, 5, 6, 8], []]
    with pytest.raises(ValueError, match="line 2.*4 words, more than tar_len - 2 = 3"):
        required_from_args(b8, VOCAB, [{}, {}, {}], 5)
    with pytest.raises(ValueError, match="line 2.*4 words need --beam 5 or more.*not --beam 3"):
        required_from_args(a, VOCAB, [{}, {}, {}], 30)
    # the same through --require-words: the beam that is needed is named; a word the vocabulary lacks needs no bank
    with pytest.raises(ValueError, match="--require-words: 3 words need --beam 4 or more.*not --beam 3"):
        required_from_args(parse_args(["test", "--require-words", "fix,the,bug"]), VOCAB, [{}], 30)
    with pytest.raises(ValueError, match="--require-words: 2 words need --beam 3 or more.*not --beam 2"):
        required_from_args(parse_args(["test", "--require-words", "fix,the", "--beam", "2"]), VOCAB, [{}], 30)
    with pytest.raises(ValueError, match="--require-words: 5 words, more than 4"):
        required_from_args(parse_args(["test", "--require-words", "fix,the,bug,a,update", "--beam", "8"]), VOCAB, [{}], 30)
    assert required_from_args(parse_args(["test", "--require-words", "fix,the,nosuchword"]), VOCAB, [{}], 30) == ([[4, 5]], 1)


@pytest.mark.parametrize("argv, words", [
    (["--require-words", "fix", "--sample", "3"], ("--require-words", "does not combine with --sample")),
    (["--require-words", "fix", "--score", "refs"], ("--require-words", "does not combine with --score")),
    (["--require-file", "FILE", "--sample", "3"], ("--require-file", "does not combine with --sample")),
    (["--require-file", "FILE", "--score", "refs"], ("--require-file", "does not combine with --score")),
    (["--require-words", "fix", "--beam", "1"], ("--require-words", "does not combine with --beam 1")),
    (["--require-file", "FILE", "--beam", "1"], ("--require-file", "does not combine with --beam 1")),
    (["--require-words", "fix", "--length-penalty", "1"], ("--require-words", "does not combine with --length-penalty")),
    (["--require-words", "fix", "--beam", "4", "--beam-groups", "2", "--diversity-penalty", "0.5"],
     ("--require-words", "does not combine with --beam-groups")),
    (["--require-file", "FILE", "--diversity-penalty", "0"], ("--require-file", "does not combine with --diversity-penalty")),
    (["--require-words", "fix", "--require-file", "FILE"], ("--require-words", "--require-file", "mutually exclusive")),
    (["--require-words", " , "], ("--require-words", "no word given")),
    (["--require-words", "fix the"], ("--require-words", "a phrase is not one word")),
    (["--require-file", "no/such/file"], ("--require-file", "no such file")),
])
def test_cli_conflicts_are_refused_in_one_line(argv, words, capsys, tmp_path):
    path = tmp_path / "words"
    path.write_text("fix\n")
    with pytest.raises(SystemExit) as e:
        parse_args(["test"] + [str(path) if x == "FILE" else x for x in argv])
    assert e.value.code == 2
    last = capsys.readouterr().err.strip().split("\n")[-1]
    assert "error" in last and all(w in last for w in words), last


def test_cli_refuses_the_options_at_train_time(capsys):
    with pytest.raises(SystemExit):
        parse_args(["train", "--require-words", "fix"])
    assert "test stage" in capsys.readouterr().err
    ns = types.SimpleNamespace(stage="train", sample=None, score=None)             # a namespace without the options
    assert check_require_args(ns) is ns


def test_nbest_lines_carry_met_and_lead_with_the_most_words():
    import json
    rec = json.loads(nbest_record(["a", "b", "c", "d"], [0.5, 0.0, 0.1, 0.2], None, [0, 2, 2, 1]))
    assert rec == {"messages": ["c", "d", "a"], "prob": [0.1, 0.2, 0.5], "met": [2, 1, 0]}
    assert "met" not in json.loads(nbest_record(["a", "b"], [0.5, 0.1]))
