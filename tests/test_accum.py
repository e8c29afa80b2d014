"""The host side of gradient accumulation (--accum-steps): argument validation of the helper and of the command line, the cut
of a rank's shard into micro-batches as a pure function, and the shape of a --loss-log line.  No GPU, no DataSet."""
import argparse
import json

import pytest

import util  # noqa: F401
from fira_icse_amd import ops
from run_model import check_accum_args, loss_log_record, micro_batches, parse_args


def test_default_is_off_and_values_are_parsed():
    assert parse_args(["train"]).accum_steps is None
    assert parse_args(["test"]).accum_steps is None
    assert parse_args(["train", "--accum-steps", "1"]).accum_steps == 1
    a = parse_args(["train", "--accum-steps", "64", "--batch-size", "680", "--zero1"])
    assert (a.accum_steps, a.batch_size) == (64, 680)           # --batch-size stays the global batch


@pytest.mark.parametrize("argv,msg", [
    (["train", "--accum-steps", "0"], "[1, 64]"),
    (["train", "--accum-steps", "-2"], "[1, 64]"),
    (["train", "--accum-steps", "65"], "[1, 64]"),
    (["test", "--accum-steps", "2"], "only applies to the train stage"),
    (["test", "--accum-steps", "0"], "only applies to the train stage"),
])
def test_parser_refuses_out_of_range_values_and_the_test_stage(argv, msg, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "error" in err and msg in err


def test_validation_function_raises_value_error():
    check_accum_args(argparse.Namespace(stage="test", accum_steps=None))
    assert check_accum_args(argparse.Namespace(stage="train", accum_steps=8)).accum_steps == 8
    for stage, k in (("train", 0), ("train", 65), ("train", -1), ("test", 2), ("test", 1)):
        with pytest.raises(ValueError):
            check_accum_args(argparse.Namespace(stage=stage, accum_steps=k))


@pytest.mark.parametrize("k", [0, 65, -3, 1.5, True, "2"])
def test_helper_refuses_what_is_no_count_in_range(k):
    with pytest.raises(ValueError):
        ops.accum_check(k)


def test_helper_returns_a_plain_int_and_none_is_one():
    assert ops.accum_check(None) == 1 and ops.accum_check(1) == 1 and ops.accum_check(64) == 64
    assert type(ops.accum_check(7)) is int and ops.ACCUM_MAX == 64


@pytest.mark.parametrize("n,k,sizes", [
    (8, 2, [4, 4]), (8, 1, [8]), (7, 2, [4, 3]), (7, 3, [3, 3, 1]), (170, 4, [43, 43, 43, 41]), (9, 4, [3, 3, 3, 0]),
    (5, 4, [2, 2, 1, 0]), (2, 5, [1, 1, 0, 0, 0]), (1, 3, [1, 0, 0]), (0, 3, [0, 0, 0]), (64, 64, [1] * 64),
])
def test_split_sizes_order_and_empty_tails(n, k, sizes):
    mine = [100 + 3 * i for i in range(n)]                      # positions, not 0..n-1: the cut must keep the VALUES in order
    parts = micro_batches(mine, k)
    assert len(parts) == k and [len(p) for p in parts] == sizes
    assert [x for p in parts for x in p] == mine                # every commit once, in order
    size = -(-n // k)
    assert all(len(p) <= size for p in parts)
    assert all(len(p) == size for p in parts[:n // size if size else 0])      # full micro-batches first
    # an empty micro-batch is never followed by a non-empty one (a short tail leaves the LAST ones empty)
    seen_empty = False
    for p in parts:
        assert not (seen_empty and p)
        seen_empty = seen_empty or not p


def test_split_ranges_of_a_shard_inside_the_global_batch():
    assert ops.accum_split(10, 17, 3) == [(10, 13), (13, 16), (16, 17)]
    assert ops.accum_split(4, 4, 2) == [(4, 4), (4, 4)]
    assert ops.accum_split(0, 3, 8) == [(0, 1), (1, 2), (2, 3)] + [(3, 3)] * 5
    with pytest.raises(ValueError):
        ops.accum_split(0, 4, 0)


def test_loss_log_line_shape():
    import numpy as np
    plain = loss_log_record(2, 5, np.array([7, 3, 9]), 1.25)
    assert plain == {"epoch": 2, "batch": 5, "index": [7, 3, 9], "loss": 1.25}         # the option off: today's line, no new key
    assert list(plain) == ["epoch", "batch", "index", "loss"]
    rec = loss_log_record(0, 1, [4, 5, 6, 7], 0.5, micro=2)
    assert rec == {"epoch": 0, "batch": 1, "index": [4, 5, 6, 7], "loss": 0.5, "micro": 2}
    full = loss_log_record(0, 1, [4], 0.5, micro=3, grad=(2.0, 0.5), lr=1e-4)
    assert list(full) == ["epoch", "batch", "index", "loss", "grad_norm", "clip_coef", "lr", "micro"]
    line = json.loads(json.dumps(full))
    assert line["micro"] == 3 and line["index"] == [4] and line["grad_norm"] == 2.0 and line["clip_coef"] == 0.5
    assert all(type(i) is int for i in rec["index"])
