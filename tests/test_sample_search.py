"""Sampling from the search's edited distribution without a GPU: the ABI of fira_sample_dist, every refusal of
Searcher.sample_search ahead of any device work, the argument parser of scripts/sample_search_probe.py, and the numpy
statement's own properties on rows with zeros (sample_search_ref.py)."""
import importlib.util
import inspect
import os
import re
import types

import numpy as np
import pytest

import sample_search_ref as ref
import util
from fira_icse_amd import _lib
from fira_icse_amd.config import FiraConfig


def test_header_declares_the_entry_and_the_binding_matches_it():
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    assert "#define FIRA_ABI_VERSION 11" in header
    m = re.search(r"\bint\s+fira_sample_dist\s*\(([^;]*)\)\s*;", header)
    assert m, "fira_sample_dist is not declared"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    kinds = ["P" if "*" in p else "F" if p.startswith("float") else "I" for p in params]
    assert "".join(kinds) == "PPIIIPPPFIFFFFFPP"
    res, args = _lib.SIGNATURES["fira_sample_dist"]
    assert res is _lib._I
    want = {"P": (_lib._P, _lib._DP), "I": (_lib._I,), "F": (_lib._F,)}
    assert len(args) == len(kinds) and all(t in want[k] for t, k in zip(args, kinds))
    assert args[1] is _lib._DP
    lib = _lib.host_lib()
    if lib is not None:                                            # (a box without hipcc: the header and the table still agree)
        assert lib.fira_abi_version() == 11 and hasattr(lib, "fira_sample_dist")
    build = open(os.path.join(util.REPO, "fira_icse_amd", "build.py")).read()
    assert '"sample_row.hip"' in build


def no_launch():
    """A Searcher whose every device path raises: a refusal must come before any of them."""
    from fira_icse_amd.decode import Searcher

    class NoLaunch(Searcher):
        def __init__(self, members=()):
            self.members = members
            self.cfg = FiraConfig()
            self._ws = {}

        def _begin(self, *a, **k):
            raise AssertionError("device work before the refusal")
        _state = _workspace = _begin
    return NoLaunch


def test_every_refusal_of_sample_search_comes_before_any_launch():
    from fira_icse_amd.decode import Constraints, Neighbour, Searcher
    NoLaunch = no_launch()
    cfg = FiraConfig()
    db = types.SimpleNamespace(B=4)
    s = NoLaunch()
    bad = [("min_p", dict(min_p=1.0)), ("min_p", dict(min_p=float("nan"))), ("epsilon", dict(epsilon=-1e-3)),
           ("epsilon", dict(epsilon=float("inf"))), ("eta", dict(eta=1.5)), ("typical_p", dict(typical_p=0.0)),
           ("typical_p", dict(typical_p=1.5)), ("typical_p .* top_p", dict(typical_p=0.5, top_p=0.9)),
           ("typical_p .* min_p", dict(typical_p=0.5, min_p=0.1)), ("typical_p .* epsilon", dict(typical_p=0.5, epsilon=0.1)),
           ("typical_p .* eta", dict(typical_p=0.5, eta=0.1)),
           ("temperature", dict(temperature=0.0)), ("temperature", dict(temperature=-1.0)),
           ("temperature", dict(temperature=float("inf"))), ("temperature", dict(temperature=float("nan"))),
           ("top_k", dict(top_k=-1)), ("top_k", dict(top_k=cfg.out_len + 1)), ("top_k", dict(top_k=2.5)),
           ("top_p", dict(top_p=0.0)), ("top_p", dict(top_p=1.5)), ("top_p", dict(top_p=float("nan"))),
           ("constraints: expected decode.Constraints", dict(constraints=(2, 3))),
           ("no_repeat_ngram = %d exceeds tar_len" % (cfg.tar_len + 1), dict(constraints=Constraints(no_repeat_ngram=cfg.tar_len + 1))),
           ("banned id %d outside" % cfg.vocab_size, dict(constraints=Constraints(banned=(cfg.vocab_size,)))),
           ("prefix: 3 sequences for a batch of 4", dict(prefix=[[5], [5], [5]])),
           ("prefix: commit 1: id 2 outside", dict(prefix=[[5], [2], [], []])),
           ("prefix: commit 0: id 7 is banned", dict(prefix=[[7], [], [], []], constraints=Constraints(banned=(7,)))),
           ("prefix: commit 2: .* words, more than", dict(prefix=[[], [], [5] * (cfg.tar_len - 1), []])),
           ("neighbour: expected decode.Neighbour", dict(neighbour=object())),
           ("a neighbour batch of 2 commits for a batch of 4", dict(neighbour=Neighbour(types.SimpleNamespace(B=2, struct=None), [0.5, 0.5]))),
           ("keys: 3 values for a batch of 4", dict(keys=[1, 2, 3]))]
    for word, kw in bad:
        with pytest.raises(ValueError, match=word):
            s.sample_search(db, 2, **kw)
    for n in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match="n = "):
            s.sample_search(db, n)
    nb = Neighbour(types.SimpleNamespace(B=4, struct=None), [0.5] * 4)
    with pytest.raises(ValueError, match="does not combine with an ensemble"):
        NoLaunch(members=(object(),)).sample_search(db, 2, neighbour=nb)
    assert s._ws == {}
    # an accepted call reaches the device path (and only then)
    with pytest.raises(AssertionError, match="device work"):
        s.sample_search(db, 2, top_k=5, epsilon=0.01, constraints=Constraints(min_length=2), prefix=[[5], [], [], []])
    # there is no require=, and sample itself keeps its signature and its refusals
    assert "require" not in inspect.signature(Searcher.sample_search).parameters
    assert list(inspect.signature(Searcher.sample_search).parameters)[:3] == ["self", "db", "n"]
    with pytest.raises(ValueError, match="sample does not combine with an ensemble"):
        NoLaunch(members=(object(),)).sample(db, 2)
    with pytest.raises(ValueError, match="sample does not combine with a neighbour"):
        s.sample(db, 2, neighbour=nb)


def test_state_key_carries_filters_cuts_and_option_markers():
    from fira_icse_amd.decode import Constraints, Searcher
    cuts = Searcher._check_cuts(1.0, 0.0, 0.02, 0.0, 1.0)
    base = ("sample_search", 4, 3, 1.5, 40, 1.0) + cuts
    con = Constraints(min_length=2)
    assert Searcher._key(base, False, None) == base
    assert Searcher._key(base, True, con, forced=True, neighbour=True) == base + ("merge", "prefix", "neighbour", con)


# ------------------------------------------------------------------------------------------------ the probe's parser
def probe():
    spec = importlib.util.spec_from_file_location("sample_search_probe", os.path.join(util.REPO, "scripts", "sample_search_probe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_probe_parser_accepts_the_search_options_next_to_sample(tmp_path):
    p = probe()
    a = p.parse_args(["--root", "x", "--sample", "4"])
    assert (a.sample, a.temperature, a.top_k, a.top_p, a.sample_seed) == (4, 1.0, 0, 1.0, 0)
    assert (a.min_p, a.epsilon_cutoff, a.eta_cutoff, a.typical_p, a.rerank, a.ensemble) == (None,) * 6
    assert not p.options_given(a) and a.reps == 20
    ck = tmp_path / "other.pt"
    ck.write_bytes(b"")
    a = p.parse_args(["--root", "x", "--sample", "8", "--temperature", "1.3", "--top-k", "50", "--top-p", "0.9", "--min-p", "0.05",
                      "--epsilon-cutoff", "0.01", "--eta-cutoff", "0.003", "--ban-words", "fix,bug", "--no-repeat-ngram", "2",
                      "--min-length", "3", "--merge-copies", "--prefix", "fix :", "--ensemble", str(ck), "--ensemble-weights", "3,1",
                      "--rerank", "mbr_bleu", "--sample-seed", "7", "--reps", "0"])
    assert (a.sample, a.top_k, a.min_p, a.no_repeat_ngram, a.min_length, a.merge_copies, a.prefix, a.rerank, a.reps) == \
        (8, 50, 0.05, 2, 3, True, "fix :", "mbr_bleu", 0)
    assert a.ensemble == [str(ck)] and a.ensemble_weights == [3.0, 1.0] and p.options_given(a)
    assert p.parse_args(["--root", "x", "--sample", "2", "--typical-p", "0.9", "--top-k", "40", "--no-repeat-ngram", "2"]).typical_p == 0.9


@pytest.mark.parametrize("argv, word", [
    (["--sample", "2"], "--root"), (["--root", "x"], "--sample"),
    (["--root", "x", "--sample", "9"], "--sample 9"), (["--root", "x", "--sample", "0"], "--sample 0"),
    (["--root", "x", "--sample", "2", "--temperature", "0"], "--temperature"),
    (["--root", "x", "--sample", "2", "--top-k", "-1"], "--top-k"), (["--root", "x", "--sample", "2", "--top-p", "1.5"], "--top-p"),
    (["--root", "x", "--sample", "2", "--min-p", "1"], "--min-p 1: must be in \\[0, 1\\)"),
    (["--root", "x", "--sample", "2", "--epsilon-cutoff", "nan"], "--epsilon-cutoff"),
    (["--root", "x", "--sample", "2", "--typical-p", "0.9", "--top-p", "0.9"], "--typical-p .* does not combine with --top-p"),
    (["--root", "x", "--sample", "2", "--typical-p", "0.9", "--eta-cutoff", "0.1"], "--typical-p .* does not combine with --eta-cutoff"),
    (["--root", "x", "--sample", "2", "--no-repeat-ngram", "-1"], "--no-repeat-ngram -1"),
    (["--root", "x", "--sample", "2", "--min-length", "-2"], "--min-length -2"),
    (["--root", "x", "--sample", "2", "--ban-words", " , "], "--ban-words: no word given"),
    (["--root", "x", "--sample", "2", "--prefix", "  "], "--prefix: no word given"),
    (["--root", "x", "--sample", "2", "--prefix", "fix", "--prefix-file", "p"], "mutually exclusive"),
    (["--root", "x", "--sample", "2", "--prefix-file", "/nonexistent/prefixes"], "no such file"),
    (["--root", "x", "--sample", "2", "--ensemble", "/nonexistent/model.pt"], "--ensemble: no such file"),
    (["--root", "x", "--sample", "2", "--ensemble-weights", "1,2"], "--ensemble-weights only applies with --ensemble"),
    (["--root", "x", "--sample", "2", "--rerank", "logp_word"], "--rerank"),
    (["--root", "x", "--sample", "2", "--reps", "2"], "--reps 2"),
    (["--root", "x", "--sample", "2", "--require-words", "fix"], "unrecognized arguments"),
    (["--root", "x", "--sample", "2", "--beam", "3"], "unrecognized arguments"),
])
def test_probe_parser_refuses_with_code_2_and_names_the_flag(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        probe().parse_args(argv)
    assert e.value.code == 2
    assert re.search(word, capsys.readouterr().err)


# ------------------------------------------------------------------------------------------------ the numpy statement
def edited_row(rng, n=300, zeros=0.6, total=0.4):
    """A row as an edit chain leaves it: unnormalised (sum ``total``), with ``zeros`` of the entries 0 -- the former maximum too."""
    p = np.exp(rng.standard_normal(n) * 2.5)
    gone = rng.random(n) < zeros
    gone[int(np.argmax(p))] = True
    p[gone] = 0.0
    return (p * (total / p.sum())).astype(np.float32).astype(np.float64)


SETTINGS = [dict(), dict(temperature=1.7), dict(top_k=5, temperature=1.3), dict(top_k=50), dict(top_p=0.5), dict(top_p=0.9, temperature=0.8),
            dict(top_k=50, top_p=0.9, temperature=1.5), dict(min_p=0.05), dict(epsilon=0.01), dict(eta=0.003), dict(typical_p=0.8),
            dict(top_k=40, typical_p=0.5, temperature=0.7), dict(top_p=0.9, min_p=0.02, epsilon=0.001, eta=0.003, temperature=1.3)]


@pytest.mark.parametrize("kw", SETTINGS, ids=lambda kw: ",".join("%s=%g" % it for it in kw.items()) or "plain")
def test_a_zero_is_never_kept_and_the_kept_set_is_never_empty_on_a_row_with_mass(kw):
    rng = np.random.default_rng(3)
    for trial in range(10):
        p = edited_row(rng)
        strict, relaxed = ref.kept(p, **kw)
        assert strict.any() and strict[int(np.argmax(p))]
        assert not strict[p == 0].any() and not relaxed[p == 0].any() and not (strict & ~relaxed).any()
        i, gap, clear = ref.draw(p, key=trial, seed=99, j=1, tar_len=30, step=4, **kw)
        assert strict[i] and p[i] > 0 and gap >= 0
    none, none_r = ref.kept(np.zeros(17), **kw)
    assert not none.any() and not none_r.any()
    assert ref.draw(np.zeros(17), 1, 2, 0, 30, 0, **kw) == (0, float("inf"), True) and ref.EMPTY == (0, 0.0)


def test_fewer_positive_entries_than_top_k_cut_nothing():
    rng = np.random.default_rng(4)
    p = edited_row(rng, zeros=0.9)
    n_pos = int((p > 0).sum())
    assert 5 < n_pos < 60
    for k in (n_pos, n_pos + 1, 2 * n_pos, len(p)):
        strict, relaxed = ref.kept(p, top_k=k)
        assert np.array_equal(strict, p > 0) and np.array_equal(relaxed, p > 0)
    assert ref.kept(p, top_k=n_pos - 1)[0].sum() == n_pos - 1
    one = np.zeros(64)                                             # (at least as long as the largest top_k of SETTINGS)
    one[23] = 0.125
    for kw in SETTINGS:
        assert ref.kept(one, **kw)[0].tolist() == (one > 0).tolist()
        assert ref.draw(one, 5, 6, 2, 30, 7, **kw)[0] == 23


@pytest.mark.parametrize("kw", SETTINGS, ids=lambda kw: ",".join("%s=%g" % it for it in kw.items()) or "plain")
def test_scaling_a_row_by_a_power_of_two_changes_neither_the_kept_set_nor_the_draw(kw):
    """Every quantity is relative to the row's own maximum and sums, and a power of two scales float values exactly."""
    rng = np.random.default_rng(5)
    same = 0
    for trial in range(10):
        p = edited_row(rng)
        a = ref.kept(p, **kw)
        i, gap, _ = ref.draw(p, trial, 7, 0, 30, 2, **kw)
        for scale in (2.0 ** -20, 0.25, 8.0):
            b = ref.kept(p * scale, **kw)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            j, _, _ = ref.draw(p * scale, trial, 7, 0, 30, 2, **kw)
            if gap > 1e-9:                                         # (log(2^k p) is log p + k ln 2 only up to float64 rounding)
                assert i == j
                same += 1
    assert same >= 27
