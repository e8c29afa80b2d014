"""Command-line validation of the sampling options (run_model.py test --sample ...): no GPU, no DataSet."""
import pytest

import util  # noqa: F401
from run_model import check_sample_args, parse_args


def test_defaults_without_sample_are_the_search():
    a = parse_args(["test"])
    assert a.sample is None and a.beam == 3 and a.temperature is None and a.top_k is None and a.top_p is None
    assert parse_args(["test", "--beam", "1"]).beam == 1


def test_sample_fills_defaults_and_beam_one():
    a = parse_args(["test", "--sample", "3"])
    assert (a.sample, a.beam, a.temperature, a.top_k, a.top_p, a.sample_seed) == (3, 1, 1.0, 0, 1.0, 0)
    a = parse_args(["test", "--sample", "8", "--temperature", "0.7", "--top-k", "50", "--top-p", "0.95", "--sample-seed", "9",
                    "--beam", "1"])
    assert (a.sample, a.beam, a.temperature, a.top_k, a.top_p, a.sample_seed) == (8, 1, 0.7, 50, 0.95, 9)


@pytest.mark.parametrize("argv", [
    ["--sample", "3", "--beam", "3"],
    ["--sample", "0"], ["--sample", "9"],
    ["--sample", "2", "--temperature", "0"], ["--sample", "2", "--temperature", "-1"], ["--sample", "2", "--temperature", "inf"],
    ["--sample", "2", "--temperature", "nan"],
    ["--sample", "2", "--top-k", "-1"],
    ["--sample", "2", "--top-p", "0"], ["--sample", "2", "--top-p", "1.5"], ["--sample", "2", "--top-p", "nan"],
    ["--sample", "2", "--sample-seed", "-1"],
    ["--temperature", "0.5"], ["--top-k", "5"], ["--top-p", "0.9"], ["--sample-seed", "3"],
])
def test_conflicts_and_out_of_range_values_are_refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(["test"] + argv)
    assert e.value.code == 2
    assert "error" in capsys.readouterr().err


def test_validation_function_raises_value_error_and_checks_top_k_against_the_vocabulary():
    import argparse
    a = argparse.Namespace(sample=2, beam=None, temperature=None, top_k=30000, top_p=None, sample_seed=None)
    check_sample_args(argparse.Namespace(**vars(a)))                    # no vocabulary known: only k >= 0
    with pytest.raises(ValueError):
        check_sample_args(argparse.Namespace(**vars(a)), vocab_size=25020)
    with pytest.raises(ValueError):
        check_sample_args(argparse.Namespace(sample=None, beam=None, temperature=None, top_k=None, top_p=0.5,
                                             sample_seed=None))
