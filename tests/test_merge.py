"""Search over words (copy entries folded into their word, n-best output), the parts that need no GPU: the reference statement
on hand-made rows, the ABI and every argument check of ``fira_merge_dist``, the command line."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import util
from search_kit import device_dims as dims
import merge_ref as M
from fira_icse_amd import _lib
from run_model import check_merge_args, nbest_record, parse_args

f32 = np.float32
DIMS = V, L, S = (20, 4, 3)
A = 10                                  # an ordinary word


def hand_row(seed=0):
    rng = np.random.RandomState(seed)
    return rng.uniform(1e-3, 1.0, size=V + L + S).astype(f32)


# ------------------------------------------------------------------------------------------------ the reference statement
def test_a_word_on_four_entries_ends_on_its_generator_entry_in_the_stated_order():
    sou, sub = [A, 5, A, 6], [7, A, 8]                       # A: diff slots 0 and 2, sub-token slot 1 (slot index L + 1)
    row = hand_row()
    # values whose sum depends on the order of the additions
    row[A], row[V + 0], row[V + 2], row[V + L + 1] = f32(1.0), f32(3e-8), f32(3e-8), f32(5e-8)
    out = M.merged(row, sou, sub, DIMS)
    want = f32(f32(f32(row[V + 0] + row[V + 2]) + row[V + L + 1]) + row[A])
    assert out[A].tobytes() == want.tobytes()
    assert want != f32(f32(f32(row[A] + row[V + 0]) + row[V + 2]) + row[V + L + 1])        # (the order is observable here)
    assert out[V + 0] == 0 and out[V + 2] == 0 and out[V + L + 1] == 0
    # the other words: one slot each, folded into their own generator entries
    for s, w in ((1, 5), (3, 6), (L + 0, 7), (L + 2, 8)):
        assert out[w].tobytes() == f32(row[V + s] + row[w]).tobytes() and out[V + s] == 0
    untouched = [i for i in range(V) if i not in (A, 5, 6, 7, 8)]
    assert out[untouched].tobytes() == row[untouched].tobytes()


@pytest.mark.parametrize("bad", [V, -1, V + 5, -7])
def test_a_slot_whose_id_is_outside_the_vocabulary_is_left_alone(bad):
    sou, sub = [A, bad, A, 6], [bad, A, 8]
    row = hand_row(1)
    out = M.merged(row, sou, sub, DIMS)
    assert out[V + 1].tobytes() == row[V + 1].tobytes() and out[V + L].tobytes() == row[V + L].tobytes()
    assert out[V + 0] == 0 and out[A] == f32(f32(f32(row[V] + row[V + 2]) + row[V + L + 1]) + row[A])
    keep = [i for i in range(V) if i not in (A, 6, 8)]
    assert out[keep].tobytes() == row[keep].tobytes()


def test_a_zero_probability_padded_slot_with_id_0_changes_nothing_bit_for_bit():
    sou, sub = [0, 0, 0, 0], [0, 0, 0]                       # every slot padded: id 0, p == 0.0f exactly
    row = hand_row(2)
    row[V:] = f32(0.0)
    assert M.merged(row, sou, sub, DIMS).tobytes() == row.tobytes()
    # a padded slot among live ones: the live word folds, word 0 keeps its bits
    sou = [A, 0, A, 0]
    row = hand_row(3)
    row[V + 1] = row[V + 3] = f32(0.0)
    row[V + L:] = f32(0.0)
    out = M.merged(row, sou, sub, DIMS)
    assert out[0].tobytes() == row[0].tobytes() and out[A] == f32(f32(row[V] + row[V + 2]) + row[A])


def test_the_mass_of_the_row_is_conserved():
    rng = np.random.RandomState(4)
    dims = (37, 30, 20)
    for trial in range(20):
        sou, sub = rng.choice([3, 5, 6, 9, 37, -1], size=dims[1]), rng.choice([3, 5, 6, 9, 37, -1], size=dims[2])
        row = rng.uniform(1e-6, 1.0, size=sum(dims)).astype(f32)
        out = M.merged(row, sou, sub, dims)
        before, after = float(row.astype(np.float64).sum()), float(out.astype(np.float64).sum())
        assert abs(after - before) <= (dims[1] + dims[2]) * 2.0 ** -24 * before


def test_rows_per_commit_selects_the_commits_sources():
    rng = np.random.RandomState(5)
    sou, sub = rng.randint(0, V, size=(2, L)), rng.randint(0, V, size=(2, S))
    dist = rng.uniform(0.1, 1.0, size=(6, V + L + S)).astype(f32)
    out = M.merged_rows(dist, sou, sub, DIMS, 3)
    for r in range(6):
        assert out[r].tobytes() == M.merged(dist[r], sou[r // 3], sub[r // 3], DIMS).tobytes()


# ------------------------------------------------------------------------------------------------ ABI and argument checks
def test_header_declares_and_library_exports_the_entry():
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    assert re.search(r"\bint\s+fira_merge_dist\s*\(", header)
    assert "#define FIRA_ABI_VERSION 11" in header
    lib = _lib.lib()
    assert lib.fira_abi_version() == 11 and hasattr(lib, "fira_merge_dist") and "fira_merge_dist" in _lib.SIGNATURES


def call(d=None, R_=6, rpc=3, sou=16, sub=16, dist=16, best_id=16, best_p=16):
    """fira_merge_dist with pointers that are never dereferenced (every case here fails a check, or R = 0)."""
    p = lambda v: None if v is None else C.c_void_p(v)
    d = d if d is not None else dims()
    return _lib.lib().fira_merge_dist(None, C.byref(d), R_, rpc, p(sou), p(sub), p(dist), p(best_id), p(best_p))


BAD_CALLS = {
    "negative R": (dict(R_=-1, rpc=1), "R = -1"),
    "rows_per_commit 0": (dict(rpc=0), "rows_per_commit"),
    "rows_per_commit does not divide R": (dict(R_=7, rpc=3), "rows_per_commit"),
    "vocabulary too wide": (dict(d=dims(vocab=25601)), "vocabulary"),
    "vocabulary too narrow": (dict(d=dims(vocab=3)), "vocabulary"),
    "too many memory slots": (dict(d=dims(sou_len=900, sub_len=125)), "memory slots"),
    "best_id without best_p": (dict(best_p=None), "best_id and best_p"),
    "best_p without best_id": (dict(best_id=None), "best_id and best_p"),
    "null sou": (dict(sou=None), "null pointer"),
    "null sub_token": (dict(sub=None), "null pointer"),
    "null dist": (dict(dist=None), "null pointer"),
}


@pytest.mark.parametrize("name", sorted(BAD_CALLS))
def test_argument_checks_fire_before_any_launch(name):
    kw, word = BAD_CALLS[name]
    assert call(**kw) != 0
    msg = _lib.lib().fira_last_error().decode()
    assert "fira_merge_dist" in msg and word in msg, msg


def test_empty_call_is_a_no_op():
    assert call(R_=0) == 0
    assert call(R_=0, sou=None, sub=None, dist=None, best_id=None, best_p=None) == 0
    # the limits themselves pass the checks (R = 0: nothing is launched)
    assert call(R_=0, d=dims(vocab=25600, sou_len=512, sub_len=512)) == 0
    assert call(R_=0, d=dims(vocab=4, sou_len=0, sub_len=0), best_id=None, best_p=None) == 0


# ------------------------------------------------------------------------------------------------ command line
def test_cli_options_parse():
    a = parse_args(["test"])
    assert a.merge_copies is False and a.nbest is False and a.beam == 3
    a = parse_args(["test", "--merge-copies", "--nbest"])
    assert a.merge_copies and a.nbest and a.beam == 3
    a = parse_args(["test", "--merge-copies", "--beam", "1"])
    assert a.merge_copies and not a.nbest and a.beam == 1
    a = parse_args(["test", "--nbest", "--beam", "5", "--merge-copies", "--no-repeat-ngram", "2", "--min-length", "3",
                    "--ban-words", "<unkm>"])
    assert a.merge_copies and a.nbest and (a.beam, a.no_repeat_ngram, a.min_length, a.ban_words) == (5, 2, 3, "<unkm>")
    assert parse_args(["test", "--nbest"]).nbest                     # without --merge-copies: allowed, may repeat a message
    assert check_merge_args(a) is a


@pytest.mark.parametrize("argv, flag, word", [
    (["--sample", "3", "--merge-copies"], "--merge-copies", "not combine with --sample"),
    (["--sample", "3", "--nbest"], "--nbest", "not combine with --sample"),
    (["--score", "refs", "--merge-copies"], "--merge-copies", "not combine with --score"),
    (["--score", "refs", "--nbest"], "--nbest", "not combine with --score"),
    (["--nbest", "--beam", "1"], "--nbest", "not combine with --beam 1"),
    (["--merge-copies", "--nbest", "--beam", "1"], "--nbest", "not combine with --beam 1"),
])
def test_cli_conflicts_are_refused_in_one_line(argv, flag, word, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(["test"] + argv)
    assert e.value.code == 2
    last = capsys.readouterr().err.strip().split("\n")[-1]
    assert "error" in last and flag in last and word in last, last


@pytest.mark.parametrize("argv", [["--merge-copies"], ["--nbest"], ["--merge-copies", "--nbest"]])
def test_cli_refuses_the_options_at_train_time(argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(["train"] + argv)
    assert e.value.code == 2
    last = capsys.readouterr().err.strip().split("\n")[-1]
    assert "test stage" in last and all(f in last for f in argv), last


def test_nbest_record_orders_by_probability_then_slot_and_drops_what_is_not_positive():
    rec = json.loads(nbest_record(["a", "b", "c", "d", "e"], [0.25, 0.5, -1.0, 0.5, 0.0]))
    assert rec == {"messages": ["b", "d", "a"], "prob": [0.5, 0.5, 0.25]}
    assert json.loads(nbest_record(["a", "b"], [-1.0, 0.0])) == {"messages": [], "prob": []}
