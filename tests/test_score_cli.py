"""Scoring given messages without a GPU: the numpy statement of the kernel's row outputs on hand-made rows, the inverse of
detokenize on every golden message, and the command-line validation of --score / --rerank."""
import argparse

import numpy as np
import pytest

import score_ref
import util
from fira_icse_amd import data, text
from fira_icse_amd.config import EOS, START, UNK, FiraConfig
from run_model import check_score_args, parse_args, read_score_lines

V = 8
#       slot:  0  1  2  3  4  5
SRC = np.array([5, 6, 5, 7, 9, 0])            # word 9 is outside the generator's vocabulary; slot 5 is padding (id 0)
VALID = np.array([1, 1, 1, 0, 1, 0])          # word 7 sits in a masked slot only


def row(gen, copy):
    return np.array(gen + copy, dtype=np.float32)


GEN = [0.0, 0.05, 0.05, 0.1, 0.1, 0.125, 0.0, 0.05]
COPY = [0.125, 0.1, 0.0625, 0.03, 0.2, 0.0075]


def test_word_in_the_generator_only():
    r = score_ref.score_row(row(GEN, COPY), SRC, VALID, V, 4, label=4)
    assert (r["entry"], r["k"], r["copy_share"]) == (4, 1, 0.0)
    assert r["p_word"] == r["p_entry"] == r["p_label"] == float(np.float32(0.1))


def test_word_in_diff_positions_only():
    r = score_ref.score_row(row(GEN, COPY), SRC, VALID, V, 9, label=V + 4)
    assert (r["entry"], r["k"], r["copy_share"]) == (V + 4, 1, 1.0)
    assert r["p_word"] == r["p_label"] == float(np.float32(0.2))


def test_word_in_both_sums_every_entry_and_reports_the_largest():
    d = row(GEN, COPY)
    r = score_ref.score_row(d, SRC, VALID, V, 5, label=V + 2)
    assert r["k"] == 3 and r["entry"] == 5                         # tie between generator entry 5 and slot 0: lowest index
    assert r["p_word"] == float(d[5]) + float(d[V]) + float(d[V + 2])
    assert r["p_entry"] == 0.125 and r["p_label"] == 0.0625
    assert r["copy_share"] == pytest.approx(0.1875 / 0.3125)
    d[5] = 0.12                                                    # now the copy entry is strictly larger
    r = score_ref.score_row(d, SRC, VALID, V, 5)
    assert r["entry"] == V and r["p_entry"] == 0.125 and r["p_label"] == 0.0


def test_tie_between_two_copy_slots_takes_the_first():
    d = row(GEN, COPY)
    d[5], d[V + 2] = 0.0, 0.125
    assert score_ref.score_row(d, SRC, VALID, V, 5)["entry"] == V


def test_masked_slot_does_not_count():
    r = score_ref.score_row(row(GEN, COPY), SRC, VALID, V, 7)
    assert r["k"] == 1 and r["entry"] == 7 and r["p_word"] == float(np.float32(0.05)) and r["copy_share"] == 0.0
    src = SRC.copy()
    src[3] = 9                                                     # a masked slot that carries a copy-only word
    r = score_ref.score_row(row(GEN, COPY), src, VALID, V, 9)
    assert r["k"] == 1 and r["entry"] == V + 4


def test_word_nowhere_and_target_zero():
    r = score_ref.score_row(row(GEN, COPY), SRC, VALID, V, 11)     # not in the vocabulary, in no slot
    assert (r["p_word"], r["p_entry"], r["entry"], r["copy_share"], r["k"]) == (0.0, 0.0, -1, 0.0, 0)
    r = score_ref.score_row(row(GEN, COPY), SRC, VALID, V, 0, label=3)      # padding: id 0 never matches the padded slot
    assert (r["p_word"], r["p_entry"], r["entry"], r["copy_share"], r["p_label"]) == (0.0, 0.0, -1, 0.0, 0.0)
    assert r["top_id"] == V + 4
    assert score_ref.message_logp([0.5, 0.0]) == pytest.approx(np.log(0.5) + np.log(1e-10))


# ------------------------------------------------------------------------------------------------ tokenize_message
def test_tokenize_message_inverts_detokenize_on_all_golden_messages():
    cfg = FiraConfig()
    raw = util.load_golden_raw()
    store = data.process_raw(cfg, raw)
    vocab = raw["word_vocab"]
    r_vocab = {v: k for k, v in vocab.items()}
    assert len(store) == util.GOLDEN_N == 24
    n_unk = n_copy = 0
    for i in range(util.GOLDEN_N):
        ids = store.tar[i].tolist()
        ids = ids[:ids.index(EOS) + 1]                              # none of the golden messages is truncated
        var_map = raw["variable"][i]
        line = text.detokenize(ids, r_vocab, var_map)
        assert text.tokenize_message(line, vocab, var_map, cfg.tar_len) == ids, (i, line)
        n_unk += UNK in ids
        n_copy += bool((store.tar_label[i] >= cfg.vocab_size).any())
    assert (n_unk, n_copy) == (11, 23)


def test_tokenize_message_unknown_words_identifiers_and_truncation():
    vocab = {"<pad>": 0, "<eos>": 1, "<start>": 2, "<unkm>": 3, "fix": 4, "VAR0": 5, "bug": 6}
    var_map = {"fooBar": "VAR0"}
    assert text.tokenize_message("fix fooBar \U0001F605 zzz bug", vocab, var_map) == [START, 4, 5, UNK, UNK, 6, EOS]
    assert text.tokenize_message("", vocab, var_map) == [START, EOS]
    long = text.tokenize_message(" ".join(["fix"] * 40), vocab, var_map, tar_len=30)
    assert len(long) == 30 and long[0] == START and EOS not in long          # cut like data._fit cuts a target


# ------------------------------------------------------------------------------------------------ command line
def test_score_and_rerank_defaults():
    a = parse_args(["test"])
    assert a.score is None and a.rerank is None and a.beam == 3
    a = parse_args(["test", "--score", "refs"])
    assert a.score == "refs" and a.beam == 1 and a.sample is None
    assert parse_args(["test", "--score", "refs", "--beam", "1"]).beam == 1
    a = parse_args(["test", "--sample", "4", "--rerank", "mean_logp_word"])
    assert (a.sample, a.rerank, a.beam) == (4, "mean_logp_word", 1)


@pytest.mark.parametrize("argv,names", [
    (["test", "--score", "refs", "--sample", "3"], ["--score", "--sample"]),
    (["test", "--score", "refs", "--beam", "3"], ["--score", "--beam"]),
    (["test", "--rerank", "logp_word"], ["--rerank", "--sample"]),
    (["test", "--score", "refs", "--rerank", "logp_word"], ["--rerank", "--sample"]),
    (["test", "--sample", "2", "--rerank", "logp_entry"], ["--rerank"]),
    (["test", "--score", "/no/such/file"], ["--score"]),
    (["train", "--score", "refs"], ["--score"]),
])
def test_conflicts_exit_with_status_2_and_name_the_option(argv, names, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "error" in err
    for n in names:
        assert n in err


def test_check_score_args_raises_value_error():
    ns = dict(stage="test", score=None, rerank=None, sample=None, beam=None)
    check_score_args(argparse.Namespace(**ns))
    with pytest.raises(ValueError):
        check_score_args(argparse.Namespace(**dict(ns, rerank="logp_word")))
    with pytest.raises(ValueError):
        check_score_args(argparse.Namespace(**dict(ns, score="refs", sample=2)))


def test_score_file_is_checked_without_a_model(tmp_path):
    p = tmp_path / "cands"
    p.write_text('fix the bug\n{"candidates": ["a b", "c"], "logp": [-1, -2]}\n{not json\n\n')
    got = read_score_lines(str(p), 4)
    assert got == [(["fix the bug"], False), (["a b", "c"], True), (["{not json"], False), ([""], False)]
    with pytest.raises(ValueError, match="4 lines for 5 test commits"):
        read_score_lines(str(p), 5)
    p.write_text('{"candidates": []}\n')
    with pytest.raises(ValueError, match="candidates"):
        read_score_lines(str(p), 1)
    p.write_text(__import__("json").dumps({"candidates": ["x"] * 9}) + "\n")
    with pytest.raises(ValueError, match="candidates"):
        read_score_lines(str(p), 1)
