"""Prefix-forced search, the parts that need no GPU: the ABI and the argument checks of ``fira_force_dist``, every ``ValueError`` of
``Searcher.greedy`` / ``greedy_many`` / ``beam`` (raised before anything is launched: the Searcher here has no model and no
device), the command line, and the numpy statement (prefix_ref.py) on hand-written rows."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import util
from search_kit import device_dims as dims
import prefix_ref as P
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, PAD, START, UNK, FiraConfig
from fira_icse_amd.decode import BeamScoring, Constraints, Searcher
from run_model import check_prefix_args, parse_args, prefixes_from_args, read_prefix_lines

A, B_, C_, D = 10, 11, 12, 13          # four ordinary words


# ------------------------------------------------------------------------------------------------ ABI and argument checks
def test_header_declares_and_library_exports_the_entry():
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    assert re.search(r"\bint\s+fira_force_dist\s*\(", header)
    assert "#define FIRA_ABI_VERSION 11" in header
    lib = _lib.lib()
    assert lib.fira_abi_version() == 11 and hasattr(lib, "fira_force_dist") and "fira_force_dist" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["fira_force_dist"][1]) == 13


def call(d=None, R_=6, rpc=3, gen=16, length=16, sou=16, sub=16, prefix=16, prefix_len=16, dist=16, best_id=16, best_p=16):
    """fira_force_dist with pointers that are never dereferenced (every case here fails a check, or R = 0)."""
    p = lambda v: None if v is None else C.c_void_p(v)
    d = d if d is not None else dims()
    return _lib.lib().fira_force_dist(None, C.byref(d), R_, rpc, p(gen), p(length), p(sou), p(sub), p(prefix), p(prefix_len),
                                      p(dist), p(best_id), p(best_p))


BAD_CALLS = {
    "negative R": (dict(R_=-1, rpc=1), "R = -1"),
    "rows_per_commit 0": (dict(rpc=0), "rows_per_commit"),
    "rows_per_commit does not divide R": (dict(R_=7, rpc=3), "rows_per_commit"),
    "tar_len 65": (dict(d=dims(tar_len=65)), "tar_len"),
    "vocabulary too wide": (dict(d=dims(vocab=25601)), "vocabulary"),
    "vocabulary too narrow": (dict(d=dims(vocab=3)), "vocabulary"),
    "too many memory slots": (dict(d=dims(sou_len=900, sub_len=125)), "memory slots"),
    "best_id without best_p": (dict(best_p=None), "best_id and best_p"),
    "best_p without best_id": (dict(best_id=None), "best_id and best_p"),
    "null gen": (dict(gen=None), "null pointer"),
    "null length": (dict(length=None), "null pointer"),
    "null sou": (dict(sou=None), "null pointer"),
    "null sub_token": (dict(sub=None), "null pointer"),
    "null dist": (dict(dist=None), "null pointer"),
    "null prefix": (dict(prefix=None), "null pointer"),
    "null prefix_len": (dict(prefix_len=None), "null pointer"),
}


@pytest.mark.parametrize("name", sorted(BAD_CALLS))
def test_argument_checks_fire_before_any_launch(name):
    kw, word = BAD_CALLS[name]
    assert call(**kw) != 0
    msg = _lib.lib().fira_last_error().decode()
    assert "fira_force_dist" in msg and word in msg, msg


def test_empty_call_is_a_no_op():
    assert call(R_=0) == 0
    assert call(R_=0, gen=None, length=None, sou=None, sub=None, prefix=None, prefix_len=None, dist=None, best_id=None,
                best_p=None) == 0
    assert call(R_=0, d=dims(tar_len=64, vocab=25600, sou_len=512, sub_len=512)) == 0      # the limits themselves pass


# ------------------------------------------------------------------------------------------------ Searcher: the ValueErrors
def bare_searcher():
    """A Searcher with a geometry and nothing else: any launch, workspace or model access raises AttributeError, so a
    ValueError from it was raised before anything was launched."""
    s = Searcher.__new__(Searcher)
    s.cfg = FiraConfig()
    s._ws = {}
    s.members = ()
    return s


CFG = FiraConfig()
BAD_PREFIXES = {
    "too few sequences": ([[A]], None, "1 sequences for a batch of 2"),
    "too many sequences": ([[A], [], [B_]], None, "3 sequences for a batch of 2"),
    "not a sequence of sequences": ([A, B_], None, "sequence"),
    "not a sequence": (5, None, "sequence"),
    "a float id": ([[A], [B_, 4.0]], None, "commit 1.*not an integer"),
    "a string id": ([["fix"], []], None, "commit 0.*not an integer"),
    "a bool id": ([[True], []], None, "commit 0.*not an integer"),
    "<pad>": ([[A, PAD], []], None, "commit 0.*cannot be forced"),
    "<eos>": ([[], [EOS]], None, "commit 1.*cannot be forced"),
    "<start>": ([[START], []], None, "commit 0.*cannot be forced"),
    "negative id": ([[], [-1]], None, "commit 1.*outside"),
    "id at the vocabulary size": ([[CFG.vocab_size], []], None, "commit 0.*outside"),
    "too long": ([[], [A] * (CFG.tar_len - 1)], None, "commit 1.*tar_len - 2"),
    "a banned id": ([[A, B_], []], Constraints(banned=(B_,)), "commit 0.*%d is banned" % B_),
    "a repeated word under n = 1": ([[], [A, B_, A]], Constraints(no_repeat_ngram=1), "commit 1.*repeats a 1-gram"),
    "a repeated bigram under n = 2": ([[A, B_, C_, A, B_], []], Constraints(no_repeat_ngram=2), "commit 0.*repeats a 2-gram"),
}


@pytest.mark.parametrize("name", sorted(BAD_PREFIXES))
def test_every_search_refuses_a_bad_prefix_before_anything_is_launched(name):
    prefix, con, word = BAD_PREFIXES[name]
    s, db = bare_searcher(), types.SimpleNamespace(B=2)
    with pytest.raises(ValueError, match=word):
        s.greedy(db, prefix=prefix, constraints=con)
    with pytest.raises(ValueError, match=word):
        s.beam(db, 3, prefix=prefix, constraints=con)
    with pytest.raises(ValueError, match=word):
        s.beam(db, 4, prefix=prefix, constraints=con, merge_copies=True, scoring=BeamScoring(1.0, 2, 0.5))
    with pytest.raises(ValueError, match=word):
        s.greedy_many([db, db], prefix=[[[], []], prefix], constraints=con)       # the SECOND batch's: before a lane starts


def test_greedy_many_wants_one_prefix_argument_per_batch():
    s, db = bare_searcher(), types.SimpleNamespace(B=2)
    with pytest.raises(ValueError, match="1 prefix arguments for 2 batches"):
        s.greedy_many([db, db], prefix=[[[A], []]])
    with pytest.raises(ValueError, match="per batch"):
        s.greedy_many([db, db], prefix=7)


def test_what_the_checks_let_through():
    s = bare_searcher()
    T, V = s.cfg.tar_len, s.cfg.vocab_size
    assert s._prefix_rows(None, 2, None) is None
    assert s._prefix_rows([[], []], 2, None) is None and s._prefix_rows([(), ()], 2, Constraints(1)) is None      # all empty: inactive
    assert s._prefix_rows([[UNK], []], 2, None) == [[UNK], []]                       # <unkm> can be forced
    assert s._prefix_rows([[V - 1] * (T - 2), (A,)], 2, None) == [[V - 1] * (T - 2), [A]]
    got = s._prefix_rows([np.array([A, B_]), [np.int32(C_)]], 2, None)               # numpy integers are integers
    assert got == [[A, B_], [C_]] and all(type(w) is int for row in got for w in row)
    # a repeat that the constraint in force does not forbid; ids the constraint does not ban
    assert s._prefix_rows([[A, B_, A], []], 2, Constraints(no_repeat_ngram=2, banned=(C_,))) == [[A, B_, A], []]
    assert s._prefix_rows([[A, A], []], 2, Constraints(min_length=3)) == [[A, A], []]
    # the state key: a marker, not the values
    assert Searcher._key(("greedy", 2), False, None, forced=True) == ("greedy", 2, "prefix")
    c = Constraints(1)
    assert Searcher._key(("beam", 2, 3), True, c, None, True) == ("beam", 2, 3, "merge", "prefix", c)
    assert Searcher._key(("beam", 2, 3), True, c) == ("beam", 2, 3, "merge", c)       # off: today's key


def test_sample_and_score_do_not_take_the_argument():
    s, db = bare_searcher(), types.SimpleNamespace(B=2)
    with pytest.raises(TypeError):
        s.sample(db, 2, prefix=[[A], []])
    with pytest.raises(TypeError):
        s.score(db, [[START, A, EOS]] * 2, prefix=[[A], []])


# ------------------------------------------------------------------------------------------------ command line
VOCAB = {"<pad>": PAD, "<eos>": EOS, "<start>": START, "<unkm>": UNK, "fix": 4, "the": 5, "update": 6, "VAR0": 7}


def test_cli_options_parse_and_the_options_off_namespace_is_unchanged(tmp_path):
    off = vars(parse_args(["test"]))
    assert off.pop("prefix") is None and off.pop("prefix_file") is None
    on = vars(parse_args(["test", "--prefix", "fix the"]))
    assert on.pop("prefix") == "fix the" and on.pop("prefix_file") is None
    assert on == off and off["beam"] == 3                      # nothing else moves, in either direction
    assert prefixes_from_args(parse_args(["test"]), VOCAB, [{}, {}], 30) == (None, 0)
    path = tmp_path / "starts"
    path.write_text("fix\n\nupdate the\n")
    a = parse_args(["test", "--prefix-file", str(path), "--beam", "1", "--merge-copies", "--no-repeat-ngram", "2",
                    "--min-length", "2", "--ban-words", "the"])
    assert a.prefix_file == str(path) and a.prefix is None and a.beam == 1
    a = parse_args(["test", "--prefix", "fix", "--beam", "4", "--nbest", "--length-penalty", "1", "--beam-groups", "2",
                    "--diversity-penalty", "0.5"])
    assert a.prefix == "fix" and a.beam == 4


def test_cli_words_become_ids_through_the_commits_variable_map(tmp_path):
    maps = [{}, {"counter": "VAR0"}, {}]
    a = parse_args(["test", "--prefix", "fix counter nosuchword " + "\U0001F605"])
    ids, n_unk = prefixes_from_args(a, VOCAB, maps, 30)
    assert ids == [[4, UNK, UNK, UNK], [4, 7, UNK, UNK], [4, UNK, UNK, UNK]]
    assert n_unk == 2 + 1 + 2                                  # words the vocabulary lacks; the <unkm> emoji is not one of them
    path = tmp_path / "starts"
    path.write_text("fix the\n\n  update   counter\n")
    ids, n_unk = prefixes_from_args(parse_args(["test", "--prefix-file", str(path)]), VOCAB, maps, 30)
    assert ids == [[4, 5], [], [6, UNK]] and n_unk == 1
    assert read_prefix_lines(str(path), 3) == ["fix the", "", "  update   counter"]


def test_cli_wrong_line_count_and_too_long_a_line_are_named(tmp_path):
    path = tmp_path / "starts"
    path.write_text("fix\nthe\n")
    a = parse_args(["test", "--prefix-file", str(path)])
    with pytest.raises(ValueError, match="2 lines for 3 test commits"):
        prefixes_from_args(a, VOCAB, [{}, {}, {}], 30)
    path.write_text("fix\n" + "the " * 7 + "\n\n")
    with pytest.raises(ValueError, match="line 2.*7 words.*tar_len - 2 = 6"):
        prefixes_from_args(a, VOCAB, [{}, {}, {}], 8)
    path.write_text("fix\n" + "the " * 6 + "\n\n")
    assert prefixes_from_args(a, VOCAB, [{}, {}, {}], 8)[0] == [[4], [5] * 6, []]          # tar_len - 2 words: allowed
    with pytest.raises(ValueError, match="--prefix: 3 words"):
        prefixes_from_args(parse_args(["test", "--prefix", "fix the the"]), VOCAB, [{}], 4)


@pytest.mark.parametrize("argv, words", [
    (["--prefix", "fix", "--sample", "3"], ("--prefix", "do not combine with --sample")),
    (["--prefix", "fix", "--score", "refs"], ("--prefix", "do not combine with --score")),
    (["--prefix-file", "FILE", "--sample", "3"], ("--prefix-file", "do not combine with --sample")),
    (["--prefix-file", "FILE", "--score", "refs"], ("--prefix-file", "do not combine with --score")),
    (["--prefix", "fix", "--prefix-file", "FILE"], ("--prefix", "--prefix-file", "mutually exclusive")),
    (["--prefix", "  "], ("--prefix", "no word given")),
    (["--prefix-file", "no/such/file"], ("--prefix-file", "no such file")),
])
def test_cli_conflicts_are_refused_in_one_line(argv, words, capsys, tmp_path):
    path = tmp_path / "starts"
    path.write_text("fix\n")
    with pytest.raises(SystemExit) as e:
        parse_args(["test"] + [str(path) if x == "FILE" else x for x in argv])
    assert e.value.code == 2
    last = capsys.readouterr().err.strip().split("\n")[-1]
    assert "error" in last and all(w in last for w in words), last


def test_cli_refuses_the_options_at_train_time(capsys):
    with pytest.raises(SystemExit):
        parse_args(["train", "--prefix", "fix"])
    assert "test stage" in capsys.readouterr().err
    ns = types.SimpleNamespace(stage="train", sample=None, score=None)             # a namespace without the options
    assert check_prefix_args(ns) is ns


# ------------------------------------------------------------------------------------------------ the numpy statement
DIMS = (20, 4, 3)
SOU, SUB = [A, 5, A, EOS], [6, A, 7]


def row_of(words, T=6, tail=0):
    g = np.full(T, tail, dtype=np.int32)
    g[0] = START
    g[1:1 + len(words)] = words
    return g, 1 + len(words)


def test_a_forced_row_keeps_exactly_the_words_entries():
    V, L, S = DIMS
    prefix = np.array([A, 5, 9, 0, 0, 0], dtype=np.int32)
    g, n = row_of([])
    keep = ~P.forced_mask(g, n, SOU, SUB, DIMS, prefix, 3)
    assert np.flatnonzero(keep).tolist() == [A, V + 0, V + 2, V + L + 1]            # generator, two diff slots, one sub-token slot
    g, n = row_of([A])
    assert np.flatnonzero(~P.forced_mask(g, n, SOU, SUB, DIMS, prefix, 3)).tolist() == [5, V + 1]
    g, n = row_of([A, 5])
    assert np.flatnonzero(~P.forced_mask(g, n, SOU, SUB, DIMS, prefix, 3)).tolist() == [9]      # no slot carries the word
    dist = np.linspace(0.1, 0.9, V + L + S).astype(np.float32)
    out = P.edited(dist, P.forced_mask(g, n, SOU, SUB, DIMS, prefix, 3))
    assert out[9] == dist[9] and np.count_nonzero(out) == 1 and not np.signbit(out).any()
    assert P.argmax_ref(out) == (9, dist[9])
    assert P.forced_word(g, n, prefix, 3, 6) == 9
    # a word outside the generator's range matches slots only
    far = np.array([EOS + 1000], dtype=np.int32)
    assert not (~P.forced_mask(row_of([])[0], 1, SOU, SUB, DIMS, far, 1)).any()
    assert np.flatnonzero(~P.forced_mask(row_of([])[0], 1, [1001, 5, A, 1001], SUB, DIMS, far, 1)).tolist() == [V, V + 3]


def test_finished_rows_and_rows_past_the_prefix_are_untouched():
    prefix = np.array([A, 5, 9, 0, 0, 0], dtype=np.int32)
    g, n = row_of([A, 5, 9])                                   # m == prefix_len
    assert not P.forced_mask(g, n, SOU, SUB, DIMS, prefix, 3).any() and P.forced_word(g, n, prefix, 3, 6) is None
    g, n = row_of([A, 5, 9, 6])                                # m above it
    assert not P.forced_mask(g, n, SOU, SUB, DIMS, prefix, 3).any()
    g, n = row_of([A, EOS])                                    # finished inside the prefix
    assert not P.forced_mask(g, n, SOU, SUB, DIMS, prefix, 3).any()
    g2, n2 = row_of([A], tail=EOS)                             # the same ids one position shorter: junk past the length is ignored
    assert P.forced_mask(g2, n2, SOU, SUB, DIMS, prefix, 3).any()
    for plen in (0, -4):                                       # no prefix; a negative length counts as 0
        assert not P.forced_mask(row_of([])[0], 1, SOU, SUB, DIMS, prefix, plen).any()
    # a length above tar_len counts as tar_len: the last position of a full row is still forced
    full = np.arange(6, dtype=np.int32) + A
    g, n = row_of([A, 5, 9, 6])
    assert P.forced_word(g, n, full, 99, 6) == int(full[4])
    pre, plen = P.prefix_arrays([[A, 5], [], [9]], 6)
    assert pre.tolist() == [[A, 5, 0, 0, 0, 0], [0] * 6, [9, 0, 0, 0, 0, 0]] and plen.tolist() == [2, 0, 1]
