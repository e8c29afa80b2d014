"""The truncation cuts of the sampler without a GPU: the command line (--min-p, --epsilon-cutoff, --eta-cutoff,
--typical-p), the argument check of Searcher.sample, and the numpy twin's own properties (cut_ref.py)."""
import re

import numpy as np
import pytest

import cut_ref
import sample_ref
import util  # noqa: F401
from run_model import check_cut_args, parse_args

CUT_KEYS = ("min_p", "epsilon_cutoff", "eta_cutoff", "typical_p")
# the options-off namespace before the cuts existed (a later option adds its keys here)
BEFORE = {'stage': 'test', 'root': '.', 'splits': None, 'batch_size': None, 'test_batch_size': 20, 'epochs': 150, 'beam': 3,
          'lr': 0.0001, 'dev_from_epoch': 15, 'dev_every': 10, 'dev_on_device': False, 'max_steps': 0, 'no_dropout': False,
          'seed': 0, 'loss_log': None, 'save_optimizer': False, 'resume': False, 'dtype': 'f32', 'grad_wire': 'auto',
          'zero1': False, 'sample': None, 'temperature': None, 'top_k': None, 'top_p': None, 'sample_seed': None,
          'without_replacement': False, 'score': None, 'rerank': None, 'no_repeat_ngram': None, 'min_length': None,
          'ban_words': None, 'merge_copies': False, 'nbest': False, 'length_penalty': None, 'beam_groups': None,
          'diversity_penalty': None, 'ensemble': None, 'ensemble_weights': None, 'prefix': None, 'prefix_file': None,
          'require_words': None, 'require_file': None, 'retrieve': False, 'retrieve_lambda': None, 'retrieve_min_sim': None,
          'retrieve_store': None, 'retrieve_only': False, 'clip_grad_norm': None, 'lr_schedule': None, 'warmup_steps': None,
          'lr_decay_steps': None, 'lr_min': None, 'ema_decay': None, 'ema_every': None, 'accum_steps': None}


def test_flags_parse_and_the_options_off_namespace_gains_only_the_four_keys():
    off = vars(parse_args(["test"]))
    for k in CUT_KEYS:
        assert off.pop(k) is None
    assert off == BEFORE
    a = parse_args(["test", "--sample", "4", "--min-p", "0.1", "--epsilon-cutoff", "0.02", "--eta-cutoff", "0.003", "--top-k", "50",
                    "--top-p", "0.9", "--rerank", "mbr_bleu"])
    assert (a.min_p, a.epsilon_cutoff, a.eta_cutoff, a.typical_p, a.rerank) == (0.1, 0.02, 0.003, None, "mbr_bleu")
    a = parse_args(["test", "--sample", "2", "--typical-p", "0.9", "--top-k", "40", "--temperature", "0.8"])
    assert (a.typical_p, a.min_p, a.top_k, a.top_p, a.beam) == (0.9, None, 40, 1.0, 1)
    a = parse_args(["test", "--sample", "2"])                    # --sample alone: the cuts stay off
    assert all(getattr(a, k) is None for k in CUT_KEYS)
    assert parse_args(["test", "--sample", "2", "--typical-p", "1", "--min-p", "0.2"]).min_p == 0.2     # 1 = off


@pytest.mark.parametrize("argv, word", [
    (["test", "--min-p", "0.1"], "--min-p only apply with --sample"),
    (["test", "--epsilon-cutoff", "0.1"], "--epsilon-cutoff only apply with --sample"),
    (["test", "--eta-cutoff", "0.1"], "--eta-cutoff only apply with --sample"),
    (["test", "--typical-p", "0.9"], "--typical-p only apply with --sample"),
    (["train", "--epsilon-cutoff", "0.1"], "--epsilon-cutoff only apply to the test stage"),
    (["train", "--min-p", "0.1"], "--min-p"), (["train", "--eta-cutoff", "0.1"], "--eta-cutoff"),
    (["train", "--typical-p", "0.5"], "--typical-p"),
    (["test", "--sample", "2", "--without-replacement", "--epsilon-cutoff", "0.1"], "does not combine with --epsilon-cutoff"),
    (["test", "--sample", "2", "--without-replacement", "--min-p", "0.1"], "does not combine with --min-p"),
    (["test", "--sample", "2", "--without-replacement", "--eta-cutoff", "0.1"], "does not combine with --eta-cutoff"),
    (["test", "--sample", "2", "--without-replacement", "--typical-p", "0.5"], "does not combine with --typical-p"),
    (["test", "--sample", "2", "--typical-p", "0.9", "--top-p", "0.9"], "--typical-p .* does not combine with --top-p"),
    (["test", "--sample", "2", "--typical-p", "0.9", "--min-p", "0.1"], "--typical-p .* does not combine with --min-p"),
    (["test", "--sample", "2", "--typical-p", "0.9", "--epsilon-cutoff", "0.1"], "--typical-p .* does not combine with --epsilon-cutoff"),
    (["test", "--sample", "2", "--typical-p", "0.9", "--eta-cutoff", "0.1"], "--typical-p .* does not combine with --eta-cutoff"),
    (["test", "--sample", "2", "--min-p", "1"], "--min-p 1: must be in \\[0, 1\\)"),
    (["test", "--sample", "2", "--min-p", "-0.1"], "--min-p"), (["test", "--sample", "2", "--min-p", "nan"], "--min-p"),
    (["test", "--sample", "2", "--epsilon-cutoff", "1.5"], "--epsilon-cutoff"),
    (["test", "--sample", "2", "--epsilon-cutoff", "inf"], "--epsilon-cutoff"),
    (["test", "--sample", "2", "--eta-cutoff", "-1"], "--eta-cutoff"), (["test", "--sample", "2", "--eta-cutoff", "nan"], "--eta-cutoff"),
    (["test", "--sample", "2", "--typical-p", "0"], "--typical-p 0: must be in \\(0, 1\\]"),
    (["test", "--sample", "2", "--typical-p", "1.01"], "--typical-p"), (["test", "--sample", "2", "--typical-p", "nan"], "--typical-p"),
    # everything --sample itself refuses still refuses it with a cut given
    (["test", "--sample", "2", "--beam", "3", "--epsilon-cutoff", "0.1"], "--beam"),
    (["test", "--sample", "2", "--score", "refs", "--epsilon-cutoff", "0.1"], "--score"),
    (["test", "--sample", "2", "--retrieve", "--epsilon-cutoff", "0.1"], "--sample"),
    (["test", "--sample", "2", "--min-length", "3", "--min-p", "0.1"], "--sample"),
    (["test", "--sample", "2", "--prefix", "fix", "--typical-p", "0.5"], "--sample"),
])
def test_conflicts_exit_with_code_2_and_name_the_flag(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    assert re.search(word, capsys.readouterr().err)


def test_check_raises_value_error_leaves_old_namespaces_alone_and_help_lists_the_flags(capsys):
    import argparse
    old = argparse.Namespace(stage="test", sample=2, top_p=1.0)      # a namespace from before the cuts: nothing to check
    assert check_cut_args(old) is old
    with pytest.raises(ValueError, match="--min-p"):
        check_cut_args(argparse.Namespace(stage="test", sample=2, top_p=1.0, min_p=2.0, typical_p=None))
    with pytest.raises(SystemExit):
        parse_args(["--help"])
    out = capsys.readouterr().out
    for flag in ("--min-p", "--epsilon-cutoff", "--eta-cutoff", "--typical-p"):
        assert flag in out


def test_searcher_refuses_bad_cuts_with_value_error_before_any_launch():
    from fira_icse_amd.decode import Searcher
    chk = Searcher._check_cuts
    assert chk(1.0, 0, 0, 0, 1) == Searcher.CUTS_OFF == (0.0, 0.0, 0.0, 1.0)
    got = chk(0.9, 0.1, 0.02, 0.003, 1.0)
    assert got == tuple(float(np.float32(v)) for v in (0.1, 0.02, 0.003, 1.0))
    for name, bad in (("min_p", dict(min_p=1.0)), ("min_p", dict(min_p=-0.5)), ("min_p", dict(min_p=float("nan"))),
                      ("epsilon", dict(epsilon=1.0)), ("epsilon", dict(epsilon=float("inf"))), ("eta", dict(eta=-1e-3)),
                      ("eta", dict(eta=float("nan"))), ("typical_p", dict(typical_p=0.0)), ("typical_p", dict(typical_p=1.5)),
                      ("typical_p", dict(typical_p=float("nan"))), ("typical_p", dict(typical_p=1e-60))):
        kw = dict(top_p=1.0, min_p=0.0, epsilon=0.0, eta=0.0, typical_p=1.0)
        kw.update(bad)
        with pytest.raises(ValueError, match=name):
            chk(**kw)
    for partner in (dict(top_p=0.9), dict(min_p=0.1), dict(epsilon=0.1), dict(eta=0.1)):
        kw = dict(top_p=1.0, min_p=0.0, epsilon=0.0, eta=0.0, typical_p=0.9)
        kw.update(partner)
        with pytest.raises(ValueError, match="typical_p .* does not combine with %s" % list(partner)[0]):
            chk(**kw)

    class NoLaunch(Searcher):                                      # sample() itself raises ahead of any device work
        def __init__(self):
            self.members = ()
    with pytest.raises(ValueError, match="epsilon"):
        NoLaunch().sample(None, 2, epsilon=1.0)
    with pytest.raises(ValueError, match="typical_p .* top_p"):
        NoLaunch().sample(None, 2, typical_p=0.5, top_p=0.9)


# ------------------------------------------------------------------------------------------------ the numpy twin
def random_row(rng, n=300, peaked=1.0):
    p = np.exp(peaked * rng.standard_normal(n) * 3.0)
    p[rng.integers(0, n, 5)] = 0.0
    return (p / p.sum()).astype(np.float32).astype(np.float64)


SETTINGS = [dict(min_p=0.05), dict(min_p=0.5), dict(epsilon=0.001), dict(epsilon=0.05), dict(eta=0.0003), dict(eta=0.2),
            dict(typical_p=0.2), dict(typical_p=0.95), dict(top_k=40, epsilon=0.01), dict(top_p=0.9, min_p=0.02, eta=0.01),
            dict(top_k=30, typical_p=0.8), dict(temperature=1.7, epsilon=0.002), dict(temperature=0.7, typical_p=0.5)]


@pytest.mark.parametrize("kw", SETTINGS)
def test_strict_set_is_inside_the_relaxed_set_and_never_empty(kw):
    rng = np.random.default_rng(11)
    for trial in range(20):
        p = random_row(rng, peaked=0.3 + 0.1 * trial)
        strict, relaxed = cut_ref.kept_sets(p, **kw)
        assert strict.any() and strict[int(np.argmax(p))] and not strict[p == 0].any() and not relaxed[p == 0].any()
        assert not (strict & ~relaxed).any()
        # a cut only removes entries: inside the set of the filters alone
        base = sample_ref.kept_mask(p, kw.get("temperature", 1.0), kw.get("top_k", 0), kw.get("top_p", 1.0))
        assert not (strict & ~base).any()
        q, s2, _ = cut_ref.cut_q(p, **kw)
        assert np.array_equal(s2, strict) and abs(q.sum() - 1) < 1e-12 and (q[~strict] == 0).all()


def test_cuts_off_is_the_filters_own_set_and_the_definitions_hold_on_a_small_row():
    p = np.array([0.4, 0.3, 0.15, 0.1, 0.05, 0.0])
    strict, relaxed = cut_ref.kept_sets(p, top_k=4)
    assert np.array_equal(strict, sample_ref.kept_mask(p, 1.0, 4, 1.0)) and np.array_equal(strict, relaxed)
    assert cut_ref.kept_sets(p, min_p=0.3)[0].tolist() == [True, True, True, False, False, False]      # >= 0.12
    assert cut_ref.kept_sets(p, epsilon=0.1)[0].tolist() == [True, True, True, True, False, False]     # ties kept
    assert cut_ref.kept_sets(p, epsilon=0.999)[0].tolist() == [True] + [False] * 5                     # the maximum stays
    # top-k first: q is renormalised over the two kept entries (4/7, 3/7), so epsilon = 0.43 removes the second
    assert cut_ref.kept_sets(p, top_k=2, epsilon=0.43)[0].tolist() == [True, False, False, False, False, False]
    # typical: H = 1.391; surprises 0.916 1.204 1.897 2.303 2.996 -> distances .475 .187 .506 .912 1.605
    assert cut_ref.kept_sets(p, typical_p=1e-9)[0].tolist() == [True, True, False, False, False, False]  # nearest + maximum
    assert cut_ref.kept_sets(p, typical_p=0.5)[0].tolist() == [True, True, False, False, False, False]
    assert cut_ref.kept_sets(p, typical_p=0.75)[0].tolist() == [True, True, True, False, False, False]
    with pytest.raises(ValueError):
        cut_ref.kept_sets(p, typical_p=0.5, top_p=0.9)


def test_eta_threshold_is_eta_on_a_peaked_row_and_the_entropy_term_on_a_flat_one():
    """min(eta, sqrt(eta) e^-H): the entropy term is the smaller one exactly when H >= -ln sqrt(eta), i.e. on a row at least
    as flat as 1 / sqrt(eta) equal entries; on a peaked row (H near 0) sqrt(eta) > eta and eta itself decides."""
    n, eta = 100, 0.0009
    flat = np.full(n, 1.0 / n)
    H = cut_ref.entropy(flat)
    assert abs(H - np.log(n)) < 1e-12
    assert cut_ref.eta_threshold(eta, H) == pytest.approx(np.sqrt(eta) / n)          # 0.03 / 100 = 0.0003 < eta
    few = np.full(4, 0.25)                                                          # flat, but fewer than 1 / 0.03 entries
    assert cut_ref.eta_threshold(eta, cut_ref.entropy(few)) == eta
    peaked = np.array([0.97] + [0.03 / (n - 1)] * (n - 1))
    Hp = cut_ref.entropy(peaked)
    assert np.sqrt(eta) * np.exp(-Hp) > eta and cut_ref.eta_threshold(eta, Hp) == eta
    assert cut_ref.lower_threshold(peaked, eta=eta) == eta
    assert cut_ref.kept_sets(peaked, eta=eta)[0].sum() == 1                 # 0.03 / 99 < eta: the tail goes
    assert cut_ref.kept_sets(flat, eta=eta)[0].all()                        # 0.01 >= 0.0003: a flat row stays whole
