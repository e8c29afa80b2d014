"""Retrieval-augmented search without a GPU: the numpy reference (retrieve_ref.py) on hand-made cases, the host side of
``decode.Neighbour`` (the checks and the coefficients), the refusals of the searches, the command-line options and the
``Datastore`` file with the device parts mocked."""
import types
import warnings

import numpy as np
import pytest
import torch

import util  # noqa: F401
import retrieve_ref as RR
from fira_icse_amd import retrieve
from fira_icse_amd.decode import Neighbour, Searcher, neighbour_coef
from run_model import check_retrieve_args, neighbour_record, parse_args

F32 = np.float32


def fake_db(B):
    return types.SimpleNamespace(B=B, struct=None)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_pool_reference_on_hand_made_rows():
    mem = np.zeros((3, 4, 256), dtype=F32)
    mem[0, 0, 0], mem[0, 2, 0], mem[0, 2, 1] = 3.0, 1.0, 4.0          # rows 0 and 2 valid: mean (2, 2, 0, ...)
    mem[0, 1, :] = np.float32("nan")                                   # an invalid row of NaN must not leak
    mem[1, :, :] = np.float32("nan")                                   # no valid row at all
    mem[2, 3, 5] = -2.0                                                # one valid row
    valid = np.array([[1, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 7]])
    u = RR.pool(mem, valid)
    assert u.dtype == F32 and not np.isnan(u).any()
    want0 = np.zeros(256, F32)
    want0[0] = want0[1] = F32(2.0) / np.sqrt(F32(8.0))
    assert np.array_equal(u[0], want0) and not u[1].any()
    assert u[2, 5] == -1.0 and np.count_nonzero(u[2]) == 1
    assert np.abs(u - RR.pool64(mem, valid)).max() <= 2.0 ** -23


def test_nn_reference_ties_exclusion_nan_and_clamp():
    store = np.zeros((5, 256))
    store[0, 0] = store[1, 1] = store[3, 1] = 1.0                     # rows 1 and 3 are identical
    store[2, :] = np.nan
    store[4, 1] = -1.0
    Q = np.zeros((3, 256))
    Q[0, 1] = 1.0
    Q[1, 0] = 1.0
    Q[2, 1] = -1.0
    idx, sim, margin = RR.nn64(Q, store)
    assert idx.tolist() == [1, 0, 4] and sim.tolist() == [1.0, 1.0, 1.0] and margin[0] == 0.0 and margin[1] == 1.0
    idx, sim, _ = RR.nn64(Q, store, exclude=[1, 0, 4])
    assert idx.tolist() == [3, 1, 0] and sim.tolist() == [1.0, 0.0, 0.0]      # (negative and zero products clamp to 0)


def test_mix_reference_is_separate_float32_operations():
    V, W = 3, 5
    p = np.array([[0.1, 0.2, 0.3, 0.25, 0.15]] * 2, dtype=F32)
    q = np.array([[0.7, 0.0, 0.3, 9.0, 9.0]] * 2, dtype=F32)         # q's copy entries are never read
    cf = RR.coef([1.0, 0.25], 1.0)
    out = RR.mix(p, q, cf, V)
    a, b = cf[0]
    assert out[0, 0] == F32(F32(a * p[0, 0]) + F32(b * q[0, 0])) and out[0, 3] == F32(a * p[0, 3])
    assert abs(float(out[0].sum()) - 1.0) < 1e-6 and abs(float(out[1].sum()) - 1.0) < 1e-6      # normalised: a + b = 1
    same = RR.mix(p, q, RR.coef([0.5, 0.5], 0.0), V)
    assert np.array_equal(same.view(np.int32), p.view(np.int32))      # (1, 0) leaves every bit
    three = RR.mix(np.repeat(p[:1], 6, 0), np.repeat(q[:1], 6, 0), cf, V, rows_per_commit=3)
    assert np.array_equal(three[:3], np.repeat(out[:1], 3, 0)) and np.array_equal(three[3:], np.repeat(out[1:], 3, 0))
    ids, ps = RR.best_of(out)
    assert ids.tolist() == [0, 2] and ps.tolist() == [out[0, 0], out[1, 2]]


# ------------------------------------------------------------------------------------------------ the host side
def test_coefficients_are_formed_in_float64_and_rounded_once():
    assert neighbour_coef([0.3, 1.0], 0.0).tolist() == [[1.0, 0.0], [1.0, 0.0]]                    # lam = 0
    assert neighbour_coef([1.0], 1.0).tolist() == [[0.5, 0.5]]
    assert neighbour_coef([0.2, 0.9], 1.0, min_sim=0.5)[0].tolist() == [1.0, 0.0]                  # below min_sim
    assert neighbour_coef([0.2, 0.9], 1.0, min_sim=1.5).tolist() == [[1.0, 0.0], [1.0, 0.0]]        # min_sim > 1: nobody
    sim = [0.123456789, 0.75, 1.0 / 3.0]
    got = neighbour_coef(sim, 2.5, 0.0)
    assert got.dtype == np.float32 and np.array_equal(got, RR.coef(sim, 2.5))
    for (a, b), s in zip(got, sim):
        c = 2.5 * s
        assert a == np.float32(1.0 / (1.0 + c)) and b == np.float32(c / (1.0 + c))
        assert abs(float(a) + float(b) - 1.0) <= 2.0 ** -24


def test_neighbour_value_is_checked():
    nb = Neighbour(fake_db(2), [0.5, 1.0], lam=2, min_sim=0.25)
    assert nb.lam == 2.0 and nb.min_sim == 0.25 and nb.sim.tolist() == [0.5, 1.0] and nb.check(2) is nb
    assert np.array_equal(nb.coef(), RR.coef([0.5, 1.0], 2.0, 0.25))
    assert Neighbour(fake_db(2), torch.tensor([0.5, 1.0])).sim.tolist() == [0.5, 1.0]
    for kwargs, word in ((dict(sim=[0.5]), "1 similarities for a neighbour batch of 2"), (dict(sim=[0.5, 1.5]), "outside \\[0, 1\\]"),
                         (dict(sim=[0.5, float("nan")]), "outside \\[0, 1\\]"), (dict(sim=[0.5, -0.1]), "outside \\[0, 1\\]"),
                         (dict(sim="ab"), "not a sequence of numbers"), (dict(sim=[0.5, 1.0], lam=-1.0), "lam = -1.0 outside"),
                         (dict(sim=[0.5, 1.0], lam=float("nan")), "lam = nan outside"), (dict(sim=[0.5, 1.0], lam=True), "not a number"),
                         (dict(sim=[0.5, 1.0], min_sim=-0.5), "min_sim = -0.5 outside")):
        with pytest.raises(ValueError, match="Neighbour: .*" + word):
            Neighbour(fake_db(2), **kwargs)
    with pytest.raises(ValueError, match="not a DeviceBatch"):
        Neighbour(object(), [0.5])
    with pytest.raises(ValueError, match="a neighbour batch of 2 commits for a batch of 3"):
        nb.check(3)


class NoLaunch:
    """A Searcher that fails the test if anything reaches the device."""

    def __init__(self, members=()):
        self.members, self.cfg = members, None

    _neighbour = Searcher._neighbour
    _no_neighbour = staticmethod(Searcher._no_neighbour)


def test_searches_refuse_before_any_launch():
    nb = Neighbour(fake_db(2), [0.5, 1.0])
    s = NoLaunch()
    assert s._neighbour(None, 2) is None and s._neighbour(nb, 2) is nb
    with pytest.raises(ValueError, match="expected decode.Neighbour or None"):
        s._neighbour((nb.db, nb.sim), 2)
    with pytest.raises(ValueError, match="batch of 3"):
        s._neighbour(nb, 3)
    with pytest.raises(ValueError, match="does not combine with an ensemble"):
        NoLaunch(members=(object(),))._neighbour(nb, 2)
    for what in ("sample", "sample_distinct", "score"):
        s._no_neighbour(what, None)
        with pytest.raises(ValueError, match="%s does not combine with a neighbour" % what):
            s._no_neighbour(what, nb)
    # the state key gains its component only with a neighbour
    assert Searcher._key(("beam", 4, 3), False, None) == ("beam", 4, 3)
    assert Searcher._key(("beam", 4, 3), True, None, neighbour=True) == ("beam", 4, 3, "merge", "neighbour")


# ------------------------------------------------------------------------------------------------ command line
def test_cli_options_parse_and_the_options_off_namespace_is_unchanged():
    off = vars(parse_args(["test"]))
    for k, v in (("retrieve", False), ("retrieve_lambda", None), ("retrieve_min_sim", None), ("retrieve_store", None),
                 ("retrieve_only", False)):
        assert off.pop(k) == v
    on = vars(parse_args(["test", "--retrieve", "--retrieve-lambda", "2.5", "--retrieve-min-sim", "0.4", "--retrieve-store", "s.pt",
                          "--beam", "1", "--merge-copies", "--no-repeat-ngram", "2", "--prefix", "fix"]))
    assert (on["retrieve"], on["retrieve_lambda"], on["retrieve_min_sim"], on["retrieve_store"]) == (True, 2.5, 0.4, "s.pt")
    assert parse_args(["test", "--retrieve", "--retrieve-only"]).retrieve_only is True
    assert parse_args(["test", "--retrieve", "--require-words", "fix", "--nbest"]).retrieve is True


@pytest.mark.parametrize("args, word", [
    (["test", "--retrieve-lambda", "2"], "--retrieve-lambda needs --retrieve"),
    (["test", "--retrieve-only"], "--retrieve-only needs --retrieve"),
    (["test", "--retrieve-store", "x"], "--retrieve-store needs --retrieve"),
    (["test", "--retrieve-min-sim", "0.5"], "--retrieve-min-sim needs --retrieve"),
    (["train", "--retrieve"], "only applies to the test stage"),
    (["test", "--retrieve", "--sample", "2"], "does not combine with --sample"),
    (["test", "--retrieve", "--score", "refs"], "does not combine with --score"),
    (["test", "--retrieve", "--ensemble", __file__], "does not combine with --ensemble"),   # (any existing file)
    (["test", "--retrieve", "--retrieve-lambda", "-1"], "must be in \\[0, 1024\\]"),
    (["test", "--retrieve", "--retrieve-lambda", "nan"], "must be in \\[0, 1024\\]"),
    (["test", "--retrieve", "--retrieve-min-sim", "-0.5"], "must be >= 0"),
    (["test", "--retrieve", "--retrieve-only", "--retrieve-lambda", "2"], "does not combine with --retrieve-lambda"),
    (["test", "--retrieve", "--retrieve-only", "--nbest"], "does not combine with --nbest")])
def test_cli_conflicts_fail_before_the_model_loads(args, word, capsys):
    with pytest.raises(SystemExit):
        parse_args(args)
    import re
    assert re.search(word, capsys.readouterr().err)


def test_cli_check_raises_value_error_and_help_lists_the_options(capsys):
    with pytest.raises(ValueError, match="needs --retrieve"):
        check_retrieve_args(types.SimpleNamespace(stage="test", retrieve=False, retrieve_lambda=1.0))
    assert check_retrieve_args(types.SimpleNamespace(stage="train")).stage == "train"
    with pytest.raises(SystemExit):
        parse_args(["--help"])
    out = capsys.readouterr().out
    for flag in ("--retrieve", "--retrieve-lambda", "--retrieve-min-sim", "--retrieve-store", "--retrieve-only"):
        assert flag in out
    import json
    assert json.loads(neighbour_record(7, np.float32(0.5), "fix a bug")) == {"train_index": 7, "sim": 0.5, "message": "fix a bug"}


# ------------------------------------------------------------------------------------------------ the store's file
class FakeModel:
    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.flat = types.SimpleNamespace(data=torch.randn(100, generator=g))
        self.device_ = "cpu"


def test_datastore_round_trip_and_the_checksum_warning(tmp_path, monkeypatch):
    model, other = FakeModel(0), FakeModel(1)
    vecs = torch.from_numpy(RR.unit_rows(np.random.RandomState(0), 6))
    # the device parts mocked: one "batch" of pooled vectors per call
    chunks = iter([vecs[:4], vecs[4:]])
    monkeypatch.setattr(retrieve, "pooled_vectors", lambda searcher, db: next(chunks))
    ds = retrieve.Datastore.build(model, [([10, 11, 12, 13], None), ([20, 21], None)], searcher=object())
    assert len(ds) == 6 and ds.index.tolist() == [10, 11, 12, 13, 20, 21] and ds.checksum == retrieve.model_checksum(model)
    assert retrieve.model_checksum(model) != retrieve.model_checksum(other)
    path = str(tmp_path / "store.pt")
    ds.save(path)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        back = retrieve.Datastore.load(path, model)
    assert torch.equal(back.vectors, ds.vectors) and torch.equal(back.index, ds.index) and back.checksum == ds.checksum
    with pytest.warns(UserWarning, match="other model parameters"):
        retrieve.Datastore.load(path, other)
    torch.save({"something": 1}, path)
    with pytest.raises(ValueError, match="not a datastore file"):
        retrieve.Datastore.load(path)
    with pytest.raises(ValueError, match="do not match 2 commit indices"):
        retrieve.Datastore(vecs, [1, 2])
    with pytest.raises(ValueError, match="no batches"):
        retrieve.Datastore.build(model, [], searcher=object())
