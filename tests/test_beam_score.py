"""Length-normalised ranking and diverse beam groups, the parts that need no GPU: the reference statement (beamscore_ref.py) on
hand-worked cases, ``decode.BeamScoring``, the ABI and every argument check of ``fira_beam_select_scored``, the command line."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import util
from search_kit import device_dims as dims
import beamscore_ref as R
from fira_icse_amd import _lib
from fira_icse_amd.decode import BeamScoring
from run_model import check_scoring_args, nbest_record, parse_args, scoring_from_args

V, L, S, T = 12, 3, 2, 16                       # W = 17
W = V + L + S
EOS = 1


def rows(beam, fill=1e-30):
    return np.full((beam, W), fill, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ the reference statement
def test_inv_lp_is_gnmt():
    t = R.inv_lp_table(1.0, T)
    assert t.dtype == np.float32 and len(t) == T + 1
    assert t[1] == np.float32(1.0) and t[7] == np.float32(0.5) and t[10] == np.float32(0.4)
    assert (R.inv_lp_table(0.0, T) == 1).all()
    assert R.key64(np.float32(0.0), 1.0) == -np.inf


@pytest.mark.parametrize("alpha, winner", [(0.0, "finished"), (1.0, "continuation")])
def test_length_penalty_lets_a_long_continuation_beat_a_short_finished_one(alpha, winner):
    """Slot 0: <start> w <eos>, finished, two words, p = 0.05.  Slot 1: nine words so far, p = 0.1, and one entry of 0.1: a
    ten-word continuation of p = 0.01.  alpha = 0: ln 0.05 = -3.00 > ln 0.01 = -4.61.  alpha = 1: -3.00 * 6/7 = -2.57 against
    -4.61 * 6/15 = -1.84."""
    dist = rows(2)
    dist[1, 7] = 0.1
    words = R.words_of([4, 5, 6], [8, 9], V)
    inv = R.inv_lp_table(alpha, T)
    picks = R.select(dist, fin=[1, 0], active=[0, 1], prob=np.float32([0.05, 0.1]), length=[3, 10], words=words, inv_lp=inv,
                     groups=1, lam=0.0)
    first, second = picks
    if winner == "finished":
        assert first["carry"] and first["src"] == 0 and first["p"] == np.float32(0.05)
        assert not second["carry"] and (second["src"], second["entry"], second["word"]) == (1, 7, 7)
        assert first["key"] == pytest.approx(math.log(0.05), abs=1e-6) and second["key"] == pytest.approx(math.log(0.01), abs=1e-6)
    else:
        assert not first["carry"] and (first["src"], first["entry"]) == (1, 7) and second["carry"]
        assert first["key"] == pytest.approx(math.log(0.01) * 0.4, abs=1e-6)
        assert second["key"] == pytest.approx(math.log(0.05) * 6 / 7, abs=1e-6)


def two_group_case():
    """beam 2 in two groups at step 0 (both slots hold <start> at probability 1, same row).  Entries: generator 7 = 0.5,
    generator 4 = 0.3, copy slot V + 1 (sou id 5) = 0.1."""
    dist = rows(2)
    dist[:, 7], dist[:, 4], dist[:, V + 1] = 0.5, 0.3, 0.1
    return dist


def test_a_word_taken_through_a_copy_slot_is_penalised():
    """Group 0's best entry is copy slot V + 0 (sou id 7, p = 0.6): it appends WORD 7.  Group 1's best entry is generator 7
    (0.5) and the same slot (0.6), both word 7: penalised by lam = 1 they have ln 0.6 - 1 = -1.51 and ln 0.5 - 1 = -1.69, below
    ln 0.3 = -1.20, so group 1 appends word 4; with lam = 0.4 the slot still wins at ln 0.6 - 0.4 = -0.91."""
    dist = two_group_case()
    dist[:, V + 0] = 0.6
    words = R.words_of([7, 5, 6], [8, 9], V)
    kw = dict(fin=[0, 0], active=[1, 1], prob=np.float32([1, 1]), length=[1, 1], words=words, inv_lp=R.inv_lp_table(0.0, T), groups=2)
    g0, g1 = R.select(dist, lam=1.0, **kw)
    assert (g0["entry"], g0["word"], g0["pkey"]) == (V + 0, 7, pytest.approx(math.log(0.6), abs=1e-6))
    assert (g1["src"], g1["entry"], g1["word"]) == (1, 4, 4) and g1["pkey"] == g1["key"] == pytest.approx(math.log(0.3), abs=1e-6)
    g0, g1 = R.select(dist, lam=0.4, **kw)
    assert (g1["entry"], g1["word"]) == (V + 0, 7) and g1["pkey"] == pytest.approx(math.log(0.6) - 0.4, abs=1e-6)
    assert g1["key"] == pytest.approx(math.log(0.6), abs=1e-6) and g1["p"] == np.float32(0.6)      # reported unpenalised


def test_a_carried_pick_adds_no_count():
    """Group 0's slot is finished: <start> 7 <eos>, carried.  Its hypothesis holds word 7, but a carried pick counts for nothing:
    group 1 takes generator 7 unpenalised."""
    dist = two_group_case()
    words = R.words_of([4, 5, 6], [8, 9], V)
    g0, g1 = R.select(dist, fin=[1, 0], active=[0, 1], prob=np.float32([0.2, 1]), length=[3, 1], words=words,
                      inv_lp=R.inv_lp_table(0.0, T), groups=2, lam=5.0)
    assert g0["carry"] and g0["src"] == 0 and g0["word"] is None
    assert (g1["entry"], g1["word"]) == (7, 7) and g1["pkey"] == g1["key"] == pytest.approx(math.log(0.5), abs=1e-6)


def test_multiplicity_is_counted():
    """beam 3 in three groups, lam = 0.3.  Group 0 appends 7 (ln 0.5 = -0.69).  Group 1: 7 at -0.69 - 0.3 = -0.99 still beats 4
    at ln 0.3 = -1.20: 7 again.  Group 2: 7 at -0.69 - 0.6 = -1.29 now loses to 4 at -1.20 -- one count would not do."""
    dist = rows(3)
    dist[:, 7], dist[:, 4] = 0.5, 0.3
    words = R.words_of([4 + 100, 5, 6], [8, 9], V)
    picks = R.select(dist, fin=[0, 0, 0], active=[1, 1, 1], prob=np.float32([1, 1, 1]), length=[1, 1, 1], words=words,
                     inv_lp=R.inv_lp_table(0.0, T), groups=3, lam=0.3)
    assert [p["word"] for p in picks] == [7, 7, 4]
    assert picks[1]["pkey"] == pytest.approx(math.log(0.5) - 0.3, abs=1e-6)
    assert [p["src"] for p in picks] == [0, 1, 2]


def test_one_group_alpha_zero_is_value_then_index():
    rng = np.random.RandomState(0)
    dist = rng.choice(np.float32([0.0, 0.125, 0.25, 0.5]), size=(3, W)).astype(np.float32)
    prob = np.float32([0.5, 0.25, 0.5])
    words = R.words_of([4, 5, 6], [8, 9], V)
    picks = R.select(dist, fin=[0, 1, 0], active=[1, 1, 1], prob=prob, length=[2, 3, 2], words=words, inv_lp=R.inv_lp_table(0.0, T),
                     groups=1, lam=0.0)
    flat = np.concatenate([dist[0] * prob[0], np.full(W, -1, np.float32), dist[2] * prob[2], [prob[1]], [-1, -1]])
    order = np.lexsort((np.arange(len(flat)), -flat))[:3]
    assert [float(p["p"]) for p in picks] == [float(flat[n]) for n in order]
    got_idx = [(3 * W if p["carry"] else p["src"] * W + p["entry"]) for p in picks]
    assert got_idx == order.tolist()


def test_apply_builds_the_state():
    dist = two_group_case()
    words = R.words_of([4, 5, 6], [8, 9], V)
    inv = R.inv_lp_table(1.0, T)
    gen = np.zeros((2, T), dtype=np.int64)
    gen[:, 0] = 2
    picks = R.select(dist, fin=[0, 0], active=[1, 1], prob=np.float32([1, 1]), length=[1, 1], words=words, inv_lp=inv, groups=2, lam=1.0)
    g, l, p, parent, key = R.apply(picks, gen, np.array([1, 1]), inv)
    assert g[:, :2].tolist() == [[2, 7], [2, 4]] and l.tolist() == [2, 2] and parent.tolist() == [0, 1]
    assert key[0] == pytest.approx(math.log(0.5)) and key[1] == pytest.approx(math.log(0.3), abs=1e-6)     # inv_lp[1] = 1


# ------------------------------------------------------------------------------------------------ decode.BeamScoring
def test_beam_scoring_values():
    d = BeamScoring()
    assert (d.length_alpha, d.groups, d.diversity) == (0.0, 1, 0.0) and not d.active()
    assert BeamScoring(length_alpha=0.6).active() and BeamScoring(groups=2, diversity=0.5).active()
    assert BeamScoring(1, 2, 1) == BeamScoring(1.0, 2, 1.0) and hash(BeamScoring(1, 2, 1)) == hash(BeamScoring(1.0, 2, 1.0))
    assert len({BeamScoring(0.6), BeamScoring(0.6), BeamScoring(0.7)}) == 2
    with pytest.raises(Exception):
        d.groups = 2                                           # frozen
    assert BeamScoring(4.0, 8, 1024.0).check(8).groups == 8
    assert BeamScoring(1.0).inv_lp(3) == [1.2, 1.0, 6 / 7, 0.75]


@pytest.mark.parametrize("kw, word", [
    (dict(length_alpha=-0.1), "length_alpha"), (dict(length_alpha=4.5), "length_alpha"), (dict(length_alpha=float("nan")), "length_alpha"),
    (dict(length_alpha="1"), "length_alpha"), (dict(groups=0, diversity=1.0), "groups"), (dict(groups=9, diversity=1.0), "groups"),
    (dict(groups=2.0, diversity=1.0), "groups"), (dict(groups=True, diversity=1.0), "groups"),
    (dict(groups=2, diversity=-1.0), "diversity"), (dict(groups=2, diversity=1025.0), "diversity"),
    (dict(groups=2, diversity=float("inf")), "diversity"), (dict(diversity=0.5), "groups > 1"), (dict(groups=2), "diversity > 0"),
])
def test_beam_scoring_refuses(kw, word):
    with pytest.raises(ValueError, match=re.escape(word)):
        BeamScoring(**kw)


def test_beam_scoring_check_against_the_beam():
    with pytest.raises(ValueError, match="beam"):
        BeamScoring(1.0).check(1)
    with pytest.raises(ValueError, match="divide"):
        BeamScoring(0.0, 2, 1.0).check(3)
    with pytest.raises(ValueError, match="divide"):
        BeamScoring(0.0, 8, 1.0).check(4)
    assert BeamScoring(0.0, 3, 1.0).check(6)


# ------------------------------------------------------------------------------------------------ ABI and argument checks
def test_header_declares_and_library_exports_the_entry():
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    assert re.search(r"\bint\s+fira_beam_select_scored\s*\(", header)
    assert "#define FIRA_ABI_VERSION 11" in header
    lib = _lib.lib()
    assert lib.fira_abi_version() == 11 and hasattr(lib, "fira_beam_select_scored") and "fira_beam_select_scored" in _lib.SIGNATURES


def call(d=None, B=2, beam=4, groups=2, diversity=0.5, inv_lp=16, key_out=16, dist=16):
    """fira_beam_select_scored with pointers that are never dereferenced (every case here fails a check)."""
    p = lambda v: None if v is None else C.c_void_p(v)
    d = d if d is not None else dims()
    q = p(16)
    return _lib.lib().fira_beam_select_scored(None, C.byref(d), B, beam, p(dist), q, q, q, q, q, q, q, q, q, q, q, q, p(inv_lp), groups,
                                              diversity, p(key_out))


BAD_CALLS = {
    "beam 1": (dict(beam=1, groups=1), "n_beam = 1"),
    "beam 9": (dict(beam=9, groups=3), "n_beam = 9"),
    "groups do not divide": (dict(beam=4, groups=3), "n_groups = 3"),
    "groups 0": (dict(groups=0), "n_groups = 0"),
    "negative diversity": (dict(diversity=-0.5), "diversity"),
    "infinite diversity": (dict(diversity=float("inf")), "diversity"),
    "nan diversity": (dict(diversity=float("nan")), "diversity"),
    "tar_len 65": (dict(d=dims(tar_len=65)), "tar_len = 65"),
    "too many memory slots": (dict(d=dims(sou_len=900, sub_len=125)), "memory slots"),
    "no commits": (dict(B=0), "B = 0"),
    "null inv_lp": (dict(inv_lp=None), "null pointer"),
    "null dist": (dict(dist=None), "null pointer"),
}


@pytest.mark.parametrize("name", sorted(BAD_CALLS))
def test_argument_checks_fire_before_any_launch(name):
    kw, word = BAD_CALLS[name]
    assert call(**kw) != 0
    msg = _lib.lib().fira_last_error().decode()
    assert "fira_beam_select_scored" in msg and word in msg, msg


# ------------------------------------------------------------------------------------------------ command line
def test_cli_options_parse():
    a = parse_args(["test"])
    assert (a.length_penalty, a.beam_groups, a.diversity_penalty) == (None, None, None) and a.beam == 3
    assert scoring_from_args(a) is None
    a = parse_args(["test", "--length-penalty", "0.6"])
    assert scoring_from_args(a) == BeamScoring(0.6) and a.beam == 3
    a = parse_args(["test", "--beam", "4", "--beam-groups", "2", "--diversity-penalty", "0.5", "--length-penalty", "1", "--nbest",
                    "--merge-copies", "--no-repeat-ngram", "2", "--min-length", "3", "--ban-words", "<unkm>"])
    assert scoring_from_args(a) == BeamScoring(1.0, 2, 0.5) and a.nbest and a.merge_copies
    assert check_scoring_args(a) is a
    # every option at its off value: today's search
    assert scoring_from_args(parse_args(["test", "--length-penalty", "0", "--beam-groups", "1", "--diversity-penalty", "0"])) is None
    assert scoring_from_args(parse_args(["test", "--beam-groups", "3", "--diversity-penalty", "2"])) == BeamScoring(0.0, 3, 2.0)


@pytest.mark.parametrize("argv, flag, word", [
    (["--sample", "3", "--length-penalty", "1"], "--length-penalty", "not combine with --sample"),
    (["--sample", "3", "--beam-groups", "1"], "--beam-groups", "not combine with --sample"),
    (["--sample", "3", "--diversity-penalty", "0"], "--diversity-penalty", "not combine with --sample"),
    (["--score", "refs", "--length-penalty", "1"], "--length-penalty", "not combine with --score"),
    (["--score", "refs", "--beam-groups", "2", "--diversity-penalty", "1"], "--beam-groups", "not combine with --score"),
    (["--beam", "1", "--length-penalty", "1"], "--length-penalty", "not combine with --beam 1"),
    (["--beam", "1", "--beam-groups", "1"], "--beam-groups", "not combine with --beam 1"),
    (["--length-penalty", "-0.5"], "--length-penalty", "[0, 4]"),
    (["--length-penalty", "4.5"], "--length-penalty", "[0, 4]"),
    (["--length-penalty", "nan"], "--length-penalty", "[0, 4]"),
    (["--beam", "4", "--beam-groups", "0", "--diversity-penalty", "1"], "--beam-groups", "1..8"),
    (["--beam", "8", "--beam-groups", "9", "--diversity-penalty", "1"], "--beam-groups", "1..8"),
    (["--beam", "4", "--beam-groups", "2", "--diversity-penalty", "-1"], "--diversity-penalty", "[0, 1024]"),
    (["--beam", "4", "--beam-groups", "2", "--diversity-penalty", "2000"], "--diversity-penalty", "[0, 1024]"),
    (["--beam", "4", "--beam-groups", "2", "--diversity-penalty", "inf"], "--diversity-penalty", "[0, 1024]"),
    (["--diversity-penalty", "0.5"], "--diversity-penalty", "needs --beam-groups"),
    (["--beam", "4", "--beam-groups", "2"], "--beam-groups", "needs --diversity-penalty"),
    (["--beam", "4", "--beam-groups", "2", "--diversity-penalty", "0"], "--beam-groups", "needs --diversity-penalty"),
    (["--beam-groups", "2", "--diversity-penalty", "1"], "--beam-groups", "does not divide --beam 3"),
    (["--beam", "4", "--beam-groups", "3", "--diversity-penalty", "1"], "--beam-groups", "does not divide --beam 4"),
])
def test_cli_conflicts_are_refused_in_one_line(argv, flag, word, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(["test"] + argv)
    assert e.value.code == 2
    last = capsys.readouterr().err.strip().split("\n")[-1]
    assert "error" in last and flag in last and word in last, last


@pytest.mark.parametrize("argv", [["--length-penalty", "1"], ["--beam-groups", "1"], ["--diversity-penalty", "0"]])
def test_cli_refuses_the_options_at_train_time(argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(["train"] + argv)
    assert e.value.code == 2
    last = capsys.readouterr().err.strip().split("\n")[-1]
    assert "test stage" in last and argv[0] in last, last


def test_nbest_record_with_keys_orders_by_key_and_without_is_unchanged():
    rec = json.loads(nbest_record(["a", "b", "c", "d"], [0.25, 0.5, 0.0, 0.125], [-0.5, -0.7, float("-inf"), -0.5]))
    assert rec == {"messages": ["a", "d", "b"], "prob": [0.25, 0.125, 0.5], "key": [-0.5, -0.5, -0.7]}
    assert nbest_record(["a", "b"], [0.25, 0.5]) == json.dumps({"messages": ["b", "a"], "prob": [0.5, 0.25]})
