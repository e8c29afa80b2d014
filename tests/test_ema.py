"""The host side of the weight average (--ema-decay): the update weight, argument validation of the helpers and of the command
line.  No GPU, no DataSet."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

import util
from fira_icse_amd import ops
from run_model import check_ema_args, parse_args


@pytest.mark.parametrize("decay,every", [(0.999, 1), (0.999, 32), (0.5, 4)])
def test_weight_is_the_double_expression_rounded_once(decay, every):
    w = ops.ema_weight(decay, every)
    assert isinstance(w, float)
    assert np.float32(w) == np.float32(1.0 - decay ** every) and float(np.float32(w)) == w      # exactly representable in fp32
    assert 0.0 < w < 1.0


def test_weight_of_one_step_and_of_a_cadence_agree_with_the_closed_form():
    assert ops.ema_weight(0.5, 4) == 0.9375                     # 1 - 2^-4, exact
    assert ops.ema_weight(0.5) == 0.5                           # K defaults to 1
    # K updates with decay D shrink (e - p) by D^K when p stands still: the cadence form does it in one update
    assert abs((1.0 - ops.ema_weight(0.999, 32)) - 0.999 ** 32) < 1e-7


@pytest.mark.parametrize("decay,every", [(0.0, 1), (1.0, 1), (-0.1, 1), (1.5, 4), (float("nan"), 1), (None, 1), ("x", 1),
                                         (0.9, 0), (0.9, -3), (0.9, 1.5), (0.9, True)])
def test_helpers_refuse_what_is_out_of_range(decay, every):
    with pytest.raises(ValueError):
        ops.ema_check(decay, every)
    with pytest.raises(ValueError):
        ops.ema_weight(decay, every)


def test_check_returns_plain_numbers():
    assert ops.ema_check(0.9, 4) == (0.9, 4)
    d, k = ops.ema_check(np.float32(0.5), 32)
    assert type(d) is float and type(k) is int


def test_default_is_off_and_values_are_parsed():
    a = parse_args(["train"])
    assert a.ema_decay is None and a.ema_every is None
    a = parse_args(["train", "--ema-decay", "0.999"])
    assert a.ema_decay == 0.999 and a.ema_every == 32          # the every-row cadence of the row-sparse Adam
    a = parse_args(["train", "--ema-decay", "0.5", "--ema-every", "1", "--zero1"])
    assert (a.ema_decay, a.ema_every) == (0.5, 1)


@pytest.mark.parametrize("argv,msg", [
    (["train", "--ema-every", "4"], "--ema-every needs --ema-decay"),
    (["train", "--ema-decay", "0"], "(0, 1)"),
    (["train", "--ema-decay", "1"], "(0, 1)"),
    (["train", "--ema-decay", "1.5"], "(0, 1)"),
    (["train", "--ema-decay", "-0.5"], "(0, 1)"),
    (["train", "--ema-decay", "nan"], "(0, 1)"),
    (["train", "--ema-decay", "0.9", "--ema-every", "0"], ">= 1"),
    (["train", "--ema-decay", "0.9", "--ema-every", "-2"], ">= 1"),
    (["test", "--ema-decay", "0.9"], "only applies to the train stage"),
])
def test_parser_refuses_conflicts_and_out_of_range_values(argv, msg, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "error" in err and msg in err


def test_validation_function_raises_value_error():
    check_ema_args(argparse.Namespace(stage="test", ema_decay=None, ema_every=None))
    assert check_ema_args(argparse.Namespace(stage="train", ema_decay=0.99, ema_every=None)).ema_every == 32
    for stage, d, k in (("train", None, 4), ("train", 0.0, None), ("train", 1.0, 1), ("train", 0.9, 0), ("test", 0.9, None)):
        with pytest.raises(ValueError):
            check_ema_args(argparse.Namespace(stage=stage, ema_decay=d, ema_every=k))


def test_the_driver_exits_before_anything_touches_the_gpu(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "run_model.py"), "train", "--ema-every", "8"], capture_output=True,
                       text=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 2
    assert "--ema-every needs --ema-decay" in r.stderr.splitlines()[-1] and "Traceback" not in r.stderr
