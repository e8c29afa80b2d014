"""Search constraints (no-repeat n-gram, minimum length, banned words), the parts that need no GPU: the reference statement on
hand-written cases, ``decode.Constraints``, the ABI and every argument check of ``fira_constrain_dist``, the command line."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

import util
from search_kit import device_dims as dims
import constrain_ref as R
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, PAD, START, UNK, FiraConfig
from fira_icse_amd.decode import Constraints
from run_model import check_constraint_args, constraints_from_args, parse_args

A, B_, C_, D = 10, 11, 12, 13          # four ordinary words


# ------------------------------------------------------------------------------------------------ the reference statement
def test_ngram_tail_does_not_match_itself():
    # n = 2, hypothesis A B: the tail is (B); the only completed bigram is A B, whose predecessor A != B -> nothing.  The tail's
    # own position (j = m) would need h_{m+1}: excluded by j + n - 1 <= m
    assert R.blocked_words([A, B_], 2, 0, ()) == set()
    # A B A: tail (A); A at position 1 is followed by B -> B is blocked; A at position 3 is the tail itself
    assert R.blocked_words([A, B_, A], 2, 0, ()) == {B_}
    # A A: tail (A), bigram A A at j = 1 completes with A; the tail at j = 2 does not match itself
    assert R.blocked_words([A, A], 2, 0, ()) == {A}
    assert R.blocked_words([A], 2, 0, ()) == set()
    # n = 3, A B C A B: tail (A B) occurred at 1..2, followed by C
    assert R.blocked_words([A, B_, C_, A, B_], 3, 0, ()) == {C_}
    assert R.blocked_words([A, B_, C_, B_, A], 3, 0, ()) == set()
    # two earlier occurrences with different continuations
    assert R.blocked_words([A, B_, A, C_, A], 2, 0, ()) == {B_, C_}


def test_unigram_blocks_every_emitted_word():
    assert R.blocked_words([], 1, 0, ()) == set()
    assert R.blocked_words([A], 1, 0, ()) == {A}
    assert R.blocked_words([A, B_, A, D], 1, 0, ()) == {A, B_, D}


def test_n_larger_than_the_hypothesis_blocks_nothing():
    for m in range(0, 4):
        assert R.blocked_words([A] * m, 4, 0, ()) == set(), m        # m < n: no completed 4-gram
    assert R.blocked_words([A] * 4, 4, 0, ()) == {A}
    assert R.blocked_words([A, A], 0, 0, ()) == set()                # off


def test_min_length_boundary():
    M = 3
    assert R.blocked_words([A, B_], 0, M, ()) == {EOS}               # m = M - 1
    assert R.blocked_words([A, B_, C_], 0, M, ()) == set()           # m = M
    assert R.blocked_words([], 0, 1, ()) == {EOS}
    assert R.blocked_words([], 0, 0, ()) == set()


def test_union_of_the_three_rules():
    assert R.blocked_words([A, B_, A], 2, 5, (UNK, D)) == {B_, EOS, UNK, D}


def test_a_word_is_blocked_through_generator_diff_and_sub_token_entries_at_once():
    V, L, S = dims = (20, 4, 3)
    sou, sub = [A, 5, A, EOS], [6, A, 7]
    gen = np.array([START, A, 0, 0, 0, 0], dtype=np.int32)
    mask = R.blocked_mask(gen, 2, sou, sub, dims, Constraints(no_repeat_ngram=1))
    assert mask.shape == (V + L + S,)
    assert np.flatnonzero(mask).tolist() == [A, V + 0, V + 2, V + L + 1]
    # min length: <eos> through its generator id and the diff slot that carries it
    mask = R.blocked_mask(gen, 2, sou, sub, dims, Constraints(min_length=2))
    assert np.flatnonzero(mask).tolist() == [EOS, V + 3]
    # ids past length are not part of the hypothesis
    gen2 = np.array([START, A, 5, 6, 7, 5], dtype=np.int32)
    assert np.array_equal(R.blocked_mask(gen2, 2, sou, sub, dims, Constraints(no_repeat_ngram=1)),
                          R.blocked_mask(gen, 2, sou, sub, dims, Constraints(no_repeat_ngram=1)))


def test_a_finished_row_is_left_alone():
    dims = (20, 4, 3)
    sou, sub = [A, 5, A, EOS], [6, A, 7]
    gen = np.array([START, A, EOS, A, A, A], dtype=np.int32)
    c = Constraints(no_repeat_ngram=1, min_length=4, banned=(UNK, A))
    assert not R.blocked_mask(gen, 3, sou, sub, dims, c).any()
    assert R.blocked_mask(gen, 2, sou, sub, dims, c).any()           # the same ids one position shorter: not finished
    row = np.array([0.25, 0.5, 0.5, 0.125], dtype=np.float32)
    assert R.argmax_ref(row) == (1, np.float32(0.5))                 # lowest index among equals
    assert R.has_repeated_ngram([1, 2, 1, 2], 2) and not R.has_repeated_ngram([1, 2, 2, 1], 2)


# ------------------------------------------------------------------------------------------------ decode.Constraints
def test_constraints_value():
    c = Constraints()
    assert (c.no_repeat_ngram, c.min_length, c.banned) == (0, 0, ()) and not c.active
    assert Constraints(no_repeat_ngram=2).active and Constraints(min_length=1).active and Constraints(banned=(UNK,)).active
    a, b = Constraints(2, 3, [7, UNK, 7]), Constraints(2, 3, (UNK, 7))
    assert a == b and hash(a) == hash(b) and a.banned == (UNK, 7) and len({a, b, Constraints(2, 3)}) == 2
    with pytest.raises(Exception):
        a.min_length = 4                                             # frozen
    cfg = FiraConfig()
    assert Constraints(cfg.tar_len, cfg.tar_len - 2, (cfg.vocab_size - 1,)).check(cfg) is not None


@pytest.mark.parametrize("kw, word", [
    (dict(no_repeat_ngram=-1), "no_repeat_ngram"), (dict(min_length=-2), "min_length"), (dict(no_repeat_ngram=1.5), "integer"),
    (dict(min_length="3"), "integer"), (dict(banned=(PAD,)), "banned"), (dict(banned=(EOS,)), "banned"),
    (dict(banned=(START,)), "banned"), (dict(banned=(-1,)), "banned"), (dict(banned=(4.0,)), "integer"),
    (dict(banned=tuple(range(UNK, UNK + 33))), "33"), (dict(banned=5), "sequence"),
])
def test_constraints_refuses_bad_values(kw, word):
    with pytest.raises(ValueError, match=word):
        Constraints(**kw)


def test_constraints_against_the_model():
    cfg = FiraConfig()
    for c in (Constraints(no_repeat_ngram=cfg.tar_len + 1), Constraints(min_length=cfg.tar_len - 1),
              Constraints(banned=(cfg.vocab_size,))):
        with pytest.raises(ValueError):
            c.check(cfg)


# ------------------------------------------------------------------------------------------------ ABI and argument checks
def test_header_declares_and_library_exports_the_entry():
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    assert re.search(r"\bint\s+fira_constrain_dist\s*\(", header)
    assert "#define FIRA_ABI_VERSION 11" in header
    lib = _lib.lib()
    assert lib.fira_abi_version() == 11 and hasattr(lib, "fira_constrain_dist") and "fira_constrain_dist" in _lib.SIGNATURES


def call(d=None, R_=6, rpc=3, n=2, M=3, n_banned=1, gen=16, length=16, sou=16, sub=16, banned=16, dist=16, best_id=16, best_p=16):
    """fira_constrain_dist with pointers that are never dereferenced (every case here fails a check, or R = 0)."""
    p = lambda v: None if v is None else C.c_void_p(v)
    d = d if d is not None else dims()
    return _lib.lib().fira_constrain_dist(None, C.byref(d), R_, rpc, p(gen), p(length), p(sou), p(sub), n, M, p(banned), n_banned,
                                          p(dist), p(best_id), p(best_p))


BAD_CALLS = {
    "negative R": (dict(R_=-1, rpc=1), "R = -1"),
    "rows_per_commit 0": (dict(rpc=0), "rows_per_commit"),
    "rows_per_commit does not divide R": (dict(R_=7, rpc=3), "rows_per_commit"),
    "tar_len 65": (dict(d=dims(tar_len=65)), "tar_len"),
    "vocabulary too wide": (dict(d=dims(vocab=25601)), "vocabulary"),
    "too many memory slots": (dict(d=dims(sou_len=900, sub_len=125)), "memory slots"),
    "negative n": (dict(n=-1), "no_repeat_ngram"),
    "n above tar_len": (dict(n=31), "no_repeat_ngram"),
    "negative min_length": (dict(M=-1), "min_length"),
    "min_length above tar_len - 2": (dict(M=29), "min_length"),
    "negative n_banned": (dict(n_banned=-1), "n_banned"),
    "33 banned": (dict(n_banned=33), "n_banned"),
    "banned missing": (dict(n_banned=2, banned=None), "banned"),
    "best_id without best_p": (dict(best_p=None), "best_id and best_p"),
    "best_p without best_id": (dict(best_id=None), "best_id and best_p"),
    "null gen": (dict(gen=None), "null pointer"),
    "null length": (dict(length=None), "null pointer"),
    "null sou": (dict(sou=None), "null pointer"),
    "null sub_token": (dict(sub=None), "null pointer"),
    "null dist": (dict(dist=None), "null pointer"),
}


@pytest.mark.parametrize("name", sorted(BAD_CALLS))
def test_argument_checks_fire_before_any_launch(name):
    kw, word = BAD_CALLS[name]
    assert call(**kw) != 0
    msg = _lib.lib().fira_last_error().decode()
    assert "fira_constrain_dist" in msg and word in msg, msg


def test_empty_call_is_a_no_op():
    assert call(R_=0) == 0
    assert call(R_=0, gen=None, length=None, sou=None, sub=None, dist=None, best_id=None, best_p=None, n_banned=0, banned=None) == 0
    # the limits themselves pass the checks (R = 0: nothing is launched)
    assert call(R_=0, d=dims(tar_len=64, vocab=25600, sou_len=512, sub_len=512), n=64, M=62, n_banned=32) == 0
    assert call(R_=0, n=0, M=0, n_banned=0, banned=None, best_id=None, best_p=None) == 0


# ------------------------------------------------------------------------------------------------ command line
VOCAB = {"<pad>": PAD, "<eos>": EOS, "<start>": START, "<unkm>": UNK, "fix": 4, "the": 5, "update": 6}


def test_cli_options_parse():
    a = parse_args(["test"])
    assert a.no_repeat_ngram is None and a.min_length is None and a.ban_words is None and a.beam == 3
    assert constraints_from_args(a, VOCAB) is None
    a = parse_args(["test", "--no-repeat-ngram", "3", "--min-length", "2", "--ban-words", "<unkm>,the"])
    assert (a.no_repeat_ngram, a.min_length, a.ban_words, a.beam) == (3, 2, "<unkm>,the", 3)
    assert constraints_from_args(a, VOCAB, FiraConfig()) == Constraints(3, 2, (UNK, 5))
    for beam in ("1", "5"):
        a = parse_args(["test", "--beam", beam, "--min-length", "4"])
        assert a.beam == int(beam) and constraints_from_args(a, VOCAB) == Constraints(min_length=4)
    assert constraints_from_args(parse_args(["test", "--ban-words", "fix"]), VOCAB) == Constraints(banned=(4,))


@pytest.mark.parametrize("argv, word", [
    (["--sample", "3", "--no-repeat-ngram", "2"], "--sample"),
    (["--sample", "3", "--min-length", "2"], "--sample"),
    (["--sample", "3", "--ban-words", "fix"], "--sample"),
    (["--score", "refs", "--no-repeat-ngram", "2"], "--score"),
    (["--score", "refs", "--min-length", "2"], "--score"),
    (["--score", "refs", "--ban-words", "fix"], "--score"),
])
def test_cli_conflicts_are_refused_in_one_line(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(["test"] + argv)
    assert e.value.code == 2
    last = capsys.readouterr().err.strip().split("\n")[-1]
    assert "error" in last and argv[2] in last and "do not combine with " + word in last, last


@pytest.mark.parametrize("argv", [["--no-repeat-ngram", "-1"], ["--min-length", "-1"], ["--ban-words", ","]])
def test_cli_out_of_range_values_are_refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(["test"] + argv)
    assert e.value.code == 2
    last = capsys.readouterr().err.strip().split("\n")[-1]
    assert "error" in last and argv[0] in last, last


def test_cli_refuses_the_options_at_train_time(capsys):
    with pytest.raises(SystemExit):
        parse_args(["train", "--min-length", "2"])
    assert "test stage" in capsys.readouterr().err


def test_cli_unknown_or_unbannable_word_is_named():
    a = parse_args(["test", "--ban-words", "fix,nosuchword"])
    with pytest.raises(ValueError, match="nosuchword"):
        constraints_from_args(a, VOCAB)
    with pytest.raises(ValueError, match="<eos>"):
        constraints_from_args(parse_args(["test", "--ban-words", "<eos>"]), VOCAB)
    with pytest.raises(ValueError, match="min_length"):
        constraints_from_args(parse_args(["test", "--min-length", "29"]), VOCAB, FiraConfig())
    ns = argparse.Namespace(stage="test", sample=None, score=None, no_repeat_ngram=None, min_length=None, ban_words=None)
    assert check_constraint_args(ns) is ns
