"""Command-line validation of --clip-grad-norm (run_model.py train --clip-grad-norm C): no GPU, no DataSet."""
import math
import os
import subprocess
import sys

import pytest

import util
from run_model import check_clip_args, parse_args


def test_default_is_off_and_values_are_parsed():
    assert parse_args(["train"]).clip_grad_norm is None
    assert parse_args(["train", "--clip-grad-norm", "1.0"]).clip_grad_norm == 1.0
    assert parse_args(["train", "--clip-grad-norm", "0.25", "--zero1"]).clip_grad_norm == 0.25
    assert math.isinf(parse_args(["train", "--clip-grad-norm", "inf"]).clip_grad_norm)        # observe and guard only


@pytest.mark.parametrize("argv,msg", [
    (["train", "--clip-grad-norm", "0"], "must be > 0"),
    (["train", "--clip-grad-norm", "-1"], "must be > 0"),
    (["train", "--clip-grad-norm", "nan"], "must be > 0"),
    (["test", "--clip-grad-norm", "1.0"], "only applies to the train stage"),
])
def test_out_of_range_values_and_the_test_stage_are_refused(argv, msg, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "error" in err and msg in err


def test_validation_function_raises_value_error():
    import argparse
    check_clip_args(argparse.Namespace(stage="test", clip_grad_norm=None))
    check_clip_args(argparse.Namespace(stage="train", clip_grad_norm=float("inf")))
    for stage, c in (("train", 0.0), ("train", float("nan")), ("train", -2.0), ("test", 1.0)):
        with pytest.raises(ValueError):
            check_clip_args(argparse.Namespace(stage=stage, clip_grad_norm=c))


@pytest.mark.parametrize("argv", [["train", "--clip-grad-norm", "0"], ["train", "--clip-grad-norm", "nan"],
                                  ["test", "--clip-grad-norm", "1"]])
def test_the_driver_exits_before_anything_touches_the_gpu(argv, tmp_path):
    """The whole program: a one-line error and exit status 2 from an empty directory (no DataSet, no model, no device needed)."""
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "run_model.py")] + argv, capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=300)
    assert r.returncode == 2
    assert "--clip-grad-norm" in r.stderr.splitlines()[-1] and "Traceback" not in r.stderr


def test_help_names_the_option():
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "run_model.py"), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "--clip-grad-norm" in r.stdout
