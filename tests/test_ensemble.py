"""Ensemble decoding, the parts that need no GPU: the numpy statement of the mix, the inputs of the kernel tests (both traps
exist and do what is said), the weight normalisation, the ABI and every argument check of ``fira_mix_dist``, the constructor
errors of ``Searcher(model, members=...)`` and the command line."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import util
import ensemble_ref as E
from fira_icse_amd import _lib
from fira_icse_amd.config import FiraConfig
from fira_icse_amd.decode import MAX_MODELS, ensemble_weights
from run_model import check_ensemble_args, parse_args

f32 = np.float32


# ------------------------------------------------------------------------------------------------ the numpy statement
def normal_rows(seed, shape=(5, 97)):
    """Normal floats only: magnitudes in [2^-100, 2^100], both signs."""
    rng = np.random.RandomState(seed)
    return (rng.uniform(1.0, 2.0, size=shape) * 2.0 ** rng.randint(-100, 100, size=shape) * rng.choice([-1, 1], size=shape)).astype(f32)


def test_half_and_half_of_one_row_is_the_row_bit_for_bit():
    p = normal_rows(0)
    assert np.isfinite(p).all() and (np.abs(p) >= np.finfo(f32).tiny * 4).all()
    assert E.mix([p, p], [0.5, 0.5]).tobytes() == p.tobytes()
    assert E.mix([p, p], ensemble_weights(None, 2)).tobytes() == p.tobytes()


def test_weights_one_and_zero_return_the_first_member_bit_for_bit():
    p, q = normal_rows(1), normal_rows(2)
    assert E.mix([p, q], [1.0, 0.0]).tobytes() == (p + f32(0.0)).tobytes() == p.tobytes()
    rng = np.random.RandomState(3)
    d = rng.uniform(0.0, 1.0, size=(4, 50)).astype(f32)          # what a search mixes: values >= 0, exact zeros included
    d[0, :5] = 0
    assert E.mix([d, normal_rows(4, d.shape)], ensemble_weights((1, 0), 2)).tobytes() == d.tobytes()


def test_the_mix_is_the_member_ordered_sum_with_every_operation_rounded():
    rng = np.random.RandomState(5)
    d = [rng.uniform(1e-6, 1.0, size=(3, 11)).astype(f32) for _ in range(3)]
    w = ensemble_weights((0.5, 0.3, 0.2), 3)
    got = E.mix(d, w)
    contracted = 0
    for r in range(3):
        for i in range(11):
            want = f32(f32(f32(w[0] * d[0][r, i]) + f32(w[1] * d[1][r, i])) + f32(w[2] * d[2][r, i]))
            assert got[r, i].tobytes() == want.tobytes()
            fused = f32(np.float64(f32(np.float64(w[0]) * np.float64(d[0][r, i]) + np.float64(w[1]) * np.float64(d[1][r, i])))
                        + np.float64(w[2]) * np.float64(d[2][r, i]))
            contracted += fused.tobytes() != want.tobytes()
    assert contracted >= 1                                       # (a contracted evaluation is observable on these inputs)


def test_inputs_are_not_vacuous():
    """Decided on the reference alone (no launch): in every case wide enough to hold them both traps exist; the tie is an exact tie
    between a and b at the row's maximum and a wins; the flip makes k the arg-max of the mix although member 0's arg-max is i
    and member 1's is j.  Every case holds exact zeros.  (The one-element rows of R6-W1-M2 have one candidate: nothing to trap.)"""
    seen = 0
    for c in E.CASES:
        case = E.make_case(*c)
        out, best_id, best_p = E.reference(case)
        assert out.shape == (case["R"], case["W"]) and out.dtype == f32
        assert any((d == 0).any() for d in case["dists"]), c[0]
        if case["traps"] is None:
            assert case["W"] < 8
            continue
        seen += 1
        (a, b), (i, j, k) = case["traps"]
        assert len({a, b, i, j, k}) == 5 and a < b
        assert case["tie_rows"] and case["flip_rows"], c[0]
        for r in case["tie_rows"]:
            assert all(d[r, a].tobytes() == d[r, b].tobytes() for d in case["dists"])
            assert out[r, a].tobytes() == out[r, b].tobytes() == best_p[r].tobytes(), (c[0], r)
            assert best_id[r] == a and out[r, a] == out[r].max(), (c[0], r)
        for r in case["flip_rows"]:
            d0, d1 = case["dists"][0][r], case["dists"][1][r]
            assert int(np.argmax(d0)) == i and int(np.argmax(d1)) == j and i != j, (c[0], r)
            assert int(np.argsort(-d0, kind="stable")[1]) == k and int(np.argsort(-d1, kind="stable")[1]) == k, (c[0], r)
            assert best_id[r] == k and out[r, k] > out[r, i] and out[r, k] > out[r, j], (c[0], r)
    assert seen == len(E.CASES) - 1


# ------------------------------------------------------------------------------------------------ weights
def test_default_weights_are_uniform_in_float32():
    for n in range(1, MAX_MODELS + 1):
        w = ensemble_weights(None, n)
        assert w.dtype == f32 and w.shape == (n,) and all(x.tobytes() == (f32(1) / f32(n)).tobytes() for x in w)


def test_given_weights_are_normalised_in_float64_then_cast():
    w = ensemble_weights((2, 1, 1), 3)
    assert w.dtype == f32 and w.tolist() == [0.5, 0.25, 0.25]
    w = ensemble_weights([0.1, 0.2, 0.7], 3)
    want = (np.array([0.1, 0.2, 0.7], dtype=np.float64) / np.array([0.1, 0.2, 0.7], dtype=np.float64).sum()).astype(f32)
    assert w.tobytes() == want.tobytes()
    assert ensemble_weights((1, 0), 2).tolist() == [1.0, 0.0] and ensemble_weights((3,), 1).tolist() == [1.0]


@pytest.mark.parametrize("bad, word", [((1, -1), "negative"), ((1, float("nan")), "non-finite"), ((1, float("inf")), "non-finite"),
                                       ((0, 0), "sum to 0"), ((1, 2, 3), "3 values for 2"), ((1,), "1 values for 2"),
                                       (("a", 1), "not a sequence of numbers"), (5, "not a sequence of numbers")])
def test_bad_weights_are_value_errors(bad, word):
    with pytest.raises(ValueError, match=word):
        ensemble_weights(bad, 2)


# ------------------------------------------------------------------------------------------------ ABI and argument checks
def test_header_declares_and_library_exports_the_entry():
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    assert re.search(r"\bint\s+fira_mix_dist\s*\(", header)
    assert "#define FIRA_ABI_VERSION 11" in header
    lib = _lib.lib()
    assert lib.fira_abi_version() == 11 and hasattr(lib, "fira_mix_dist") and "fira_mix_dist" in _lib.SIGNATURES


def call(R_=6, W=16, n=2, ptrs=None, weights=None, out=4096, best_id=16, best_p=16, null_arrays=False):
    """fira_mix_dist with pointers that are never dereferenced (every case here fails a check, or R = 0)."""
    p = lambda v: None if v is None else C.c_void_p(v)
    k = max(n, 1)
    ptrs = list(ptrs) if ptrs is not None else [1 << 20 << m for m in range(k)]
    weights = list(weights) if weights is not None else [1.0 / k] * k
    pa, wa = (C.c_void_p * len(ptrs))(*ptrs), (C.c_float * len(weights))(*weights)
    return _lib.lib().fira_mix_dist(None, R_, W, n, None if null_arrays else pa, None if null_arrays else wa, p(out), p(best_id),
                                    p(best_p))


BAD_CALLS = {
    "negative R": (dict(R_=-1), "R = -1"),
    "empty rows": (dict(W=0), "W = 0"),
    "one member": (dict(n=1), "n_members = 1"),
    "nine members": (dict(n=9), "n_members = 9"),
    "negative weight": (dict(weights=[1.5, -0.5]), "weight 1"),
    "nan weight": (dict(weights=[float("nan"), 0.5]), "weight 0"),
    "infinite weight": (dict(weights=[0.5, float("inf")]), "weight 1"),
    "null host arrays": (dict(null_arrays=True), "null host array"),
    "best_id without best_p": (dict(best_p=None), "best_id and best_p"),
    "best_p without best_id": (dict(best_id=None), "best_id and best_p"),
    "null out": (dict(out=None), "null pointer"),
    "null member": (dict(ptrs=[1 << 20, 0]), "null pointer"),
    "out over member 1": (dict(ptrs=[1 << 20, 1 << 21], out=1 << 21), "overlaps dists[1]"),
    "out partly over member 0": (dict(ptrs=[1 << 20, 1 << 21], out=(1 << 20) + 4), "overlaps dists[0]"),
}


@pytest.mark.parametrize("name", sorted(BAD_CALLS))
def test_argument_checks_fire_before_any_launch(name):
    kw, word = BAD_CALLS[name]
    assert call(**kw) != 0
    msg = _lib.lib().fira_last_error().decode()
    assert "fira_mix_dist" in msg and word in msg, msg


def test_empty_call_is_a_no_op():
    assert call(R_=0) == 0
    assert call(R_=0, out=None, best_id=None, best_p=None) == 0
    assert call(R_=0, n=8, W=1) == 0                           # the limits themselves pass the checks


# ------------------------------------------------------------------------------------------------ the Searcher's constructor
def bare_model(cfg, device="cuda:0"):
    """A TransModel that owns no device memory: what the constructor's checks read (cfg, dims, device_), nothing else."""
    import torch
    from fira_icse_amd.model import TransModel
    m = TransModel.__new__(TransModel)
    m.cfg, m.dims, m.device_ = cfg, _lib.make_dims(cfg), torch.device(device)
    return m


@pytest.fixture(scope="module")
def cpu_models():
    """Enough for the constructor's checks, which run before anything is launched."""
    cfg = FiraConfig(vocab_size=40, ast_change_vocab_size=12)
    other = FiraConfig(vocab_size=41, ast_change_vocab_size=12)
    return cfg, [bare_model(cfg) for _ in range(3)], bare_model(other)


def test_searcher_without_members_is_todays_object(cpu_models):
    from fira_icse_amd.decode import Searcher
    cfg, (a, b, c), other = cpu_models
    s = Searcher(a)
    assert s.members == () and s.weights is None and s._ws == {} and s.flags == 0
    assert Searcher(a, kv_bf16=True, members=[]).members == ()


def test_searcher_with_members_takes_weights_primary_first(cpu_models):
    from fira_icse_amd.decode import Searcher
    cfg, (a, b, c), other = cpu_models
    s = Searcher(a, members=(b, c))
    assert s.members == (b, c) and s.weights.tobytes() == ensemble_weights(None, 3).tobytes() and s._ws == {}
    assert Searcher(a, members=[b], weights=(3, 1)).weights.tolist() == [0.75, 0.25]
    lane = s._lane()
    assert lane.members == s.members and lane.weights is s.weights and lane._ws is not s._ws


def test_searcher_constructor_errors(cpu_models):
    from fira_icse_amd.decode import Searcher
    cfg, (a, b, c), other = cpu_models
    with pytest.raises(ValueError, match="vocab"):
        Searcher(a, members=(b, other))
    with pytest.raises(ValueError, match="tar_len"):
        Searcher(a, members=(bare_model(FiraConfig(vocab_size=40, ast_change_vocab_size=12, tar_len=31)),))
    with pytest.raises(ValueError, match="is on cuda:1, the primary on cuda:0"):
        Searcher(a, members=(b, bare_model(cfg, "cuda:1")))
    with pytest.raises(ValueError, match="more than 8"):
        Searcher(a, members=(b,) * 8)
    assert len(Searcher(a, members=(b,) * 7).members) == 7
    with pytest.raises(ValueError, match="not a TransModel"):
        Searcher(a, members=("best_model.pt",))
    for bad, word in (((1, -1), "negative"), ((1, float("nan")), "non-finite"), ((0, 0), "sum to 0"), ((1, 1, 1), "3 values for 2")):
        with pytest.raises(ValueError, match=word):
            Searcher(a, members=(b,), weights=bad)
    with pytest.raises(ValueError, match="2 values for 1"):
        Searcher(a, weights=(1, 1))


def test_sample_and_score_refuse_an_ensemble_before_anything_else(cpu_models):
    from fira_icse_amd.decode import Searcher
    cfg, (a, b, c), other = cpu_models
    s = Searcher(a, members=(b,))
    with pytest.raises(ValueError, match="sample does not combine with an ensemble"):
        s.sample(None, 2)
    with pytest.raises(ValueError, match="score does not combine with an ensemble"):
        s.score(None, None)
    assert s._ws == {}


# ------------------------------------------------------------------------------------------------ command line
@pytest.fixture()
def ckpts(tmp_path):
    paths = [str(tmp_path / ("m%d.pt" % k)) for k in range(2)]
    for p in paths:
        open(p, "wb").close()
    return paths


def test_cli_options_parse(ckpts):
    a = parse_args(["test"])
    assert a.ensemble is None and a.ensemble_weights is None
    a = parse_args(["test", "--ensemble", ckpts[0]])
    assert a.ensemble == [ckpts[0]] and a.ensemble_weights is None and a.beam == 3
    a = parse_args(["test", "--ensemble", ",".join(ckpts), "--ensemble-weights", "2,1,1", "--beam", "1"])
    assert a.ensemble == ckpts and a.ensemble_weights == [2.0, 1.0, 1.0] and a.beam == 1
    assert check_ensemble_args(a) is a
    a = parse_args(["test", "--ensemble", ckpts[0], "--beam", "4", "--no-repeat-ngram", "2", "--min-length", "3", "--ban-words",
                    "<unkm>", "--merge-copies", "--nbest", "--length-penalty", "1", "--beam-groups", "2", "--diversity-penalty",
                    "0.5"])
    assert a.ensemble == [ckpts[0]] and a.merge_copies and a.nbest and a.beam_groups == 2


def refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    return capsys.readouterr().err.strip().split("\n")[-1]


def test_cli_errors_are_raised_while_parsing_before_any_model_loads(ckpts, tmp_path, capsys):
    missing = str(tmp_path / "nowhere.pt")
    for argv, words in (
            (["--ensemble", missing], ("no such file", missing)),
            (["--ensemble", ckpts[0] + "," + missing], ("no such file", missing)),
            (["--ensemble", ckpts[0] + ","], ("empty path",)),
            (["--ensemble", ckpts[0], "--ensemble-weights", "1"], ("1 weights for 2 models",)),
            (["--ensemble", ",".join(ckpts), "--ensemble-weights", "1,1"], ("2 weights for 3 models",)),
            (["--ensemble", ckpts[0], "--ensemble-weights", "1,-1"], ("negative",)),
            (["--ensemble", ckpts[0], "--ensemble-weights", "1,nan"], ("non-finite",)),
            (["--ensemble", ckpts[0], "--ensemble-weights", "0,0"], ("sum to 0",)),
            (["--ensemble", ckpts[0], "--ensemble-weights", "1,x"], ("not a list of numbers",)),
            (["--ensemble", ",".join([ckpts[0]] * 8)], ("more than 8",)),
            (["--ensemble-weights", "1,1"], ("only applies with --ensemble",)),
            (["--ensemble", ckpts[0], "--sample", "3"], ("--ensemble", "not combine with --sample")),
            (["--ensemble", ckpts[0], "--score", "refs"], ("--ensemble", "not combine with --score"))):
        last = refused(["test"] + argv, capsys)
        assert "error" in last and all(w in last for w in words), last
    last = refused(["train", "--ensemble", ckpts[0]], capsys)
    assert "test stage" in last and "--ensemble" in last
