"""Token-level retrieval (kNN-MT) without a GPU: the numpy statement's own properties (knn_ref.py), the refusals of
``decode.KnnMT.check`` and of the searches that do not take ``knn=``, and the value-resolution rule on a hand-made batch."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import util
import knn_ref as KR
from fira_icse_amd import _lib, build, retrieve
from fira_icse_amd.decode import KnnMT, Searcher

F32 = np.float32


def fake_store(N=5, width=256):
    return types.SimpleNamespace(keys=torch.zeros(N, width), key_sq=torch.zeros(N), values=torch.zeros(N, dtype=torch.int32),
                                 owner=torch.zeros(N, dtype=torch.int32), N=N)


# ------------------------------------------------------------------------------------------------ the statement
def small_case(rng, R=3, N=40, K=8, W=30):
    keys = rng.randint(-2, 3, (N, 256)).astype(F32)
    Q = rng.randint(-2, 3, (R, 256)).astype(F32)
    key_sq = np.array([KR.sum_sq(k) for k in keys], dtype=F32)
    values = rng.randint(0, W, N).astype(np.int32)
    dist = rng.dirichlet(np.ones(W), R).astype(F32)
    return Q, keys, key_sq, values, dist


def test_search_statement_orders_by_distance_then_index_and_fills_void_slots():
    rng = np.random.RandomState(0)
    Q, keys, key_sq, _, _ = small_case(rng)
    keys[7] = keys[3]                                             # a duplicate: ties to the smaller index
    key_sq[7] = key_sq[3]
    Q[0] = keys[3]
    idx, d2 = KR.knn_search(Q, keys, key_sq, 8, exact=True)
    true = ((Q[:, None, :].astype(np.float64) - keys[None].astype(np.float64)) ** 2).sum(2)
    assert idx[0, 0] == 3 and idx[0, 1] == 7 and d2[0, 0] == 0 and d2[0, 1] == 0
    for r in range(Q.shape[0]):
        order = np.lexsort((np.arange(len(keys)), true[r]))[:8]
        assert np.array_equal(idx[r], order) and np.array_equal(d2[r], true[r][order].astype(F32))
    # the chain form agrees where everything is exact
    idx_c, d2_c = KR.knn_search(Q[:1], keys, key_sq, 8)
    assert np.array_equal(idx_c, idx[:1]) and np.array_equal(d2_c, d2[:1])
    # K > N, exclusion and NaN
    idx, d2 = KR.knn_search(Q, keys[:3], key_sq[:3], 5, exact=True)
    assert (idx[:, 3:] == -1).all() and np.isinf(d2[:, 3:]).all() and (idx[:, :3] >= 0).all()
    owner = np.arange(len(keys)) // 4
    idx, _ = KR.knn_search(Q[:1], keys, key_sq, 8, owner=owner, exclude=[0], exact=True)
    assert 3 not in idx[0] and idx[0, 0] == 7 and (owner[idx[0]] != 0).all()
    bad = keys.copy()
    bad[3, 5] = np.nan
    bad_sq = key_sq.copy()
    bad_sq[3] = np.nan
    idx, _ = KR.knn_search(Q[:1], bad, bad_sq, 8, exact=True)
    assert 3 not in idx[0] and idx[0, 0] == 7


def test_mix_statement_preserves_the_sum_and_leaves_lam_zero_and_void_rows_alone():
    rng = np.random.RandomState(1)
    Q, keys, key_sq, values, dist = small_case(rng)
    idx, d2 = KR.knn_search(Q, keys, key_sq, 8, exact=True)
    out, touched = KR.mix_knn(dist, idx, d2, values, 0.3, 0.1)
    assert touched.any() and np.abs(out.sum(1, dtype=np.float64) - dist.sum(1, dtype=np.float64)).max() < 1e-6
    f64 = KR.mix_knn_f64(dist, idx, d2, values, 0.3, 0.1)
    # (fl(1 - lam) + lam is 1 within one rounding of 1 - lam: 2^-24)
    assert np.abs(out - f64).max() < 1e-6 and np.abs(f64.sum(1) - dist.astype(np.float64).sum(1)).max() <= 2.0 ** -24
    assert np.array_equal(out[~touched], (F32(F32(1) - F32(0.3)) * dist)[~touched])
    same, touched = KR.mix_knn(dist, idx, d2, values, 0.0, 0.1)
    assert same.tobytes() == dist.tobytes() and not touched.any()
    void = np.full_like(idx, -1)
    same, touched = KR.mix_knn(dist, void, np.full_like(d2, np.inf), values, 0.5, 0.1)
    assert same.tobytes() == dist.tobytes() and not touched.any()
    # a word in several slots accumulates; void slots carry no weight
    idx1 = np.array([[2, 4, -1, -1]], dtype=np.int32)
    vals = np.array([0, 0, 6, 0, 6], dtype=np.int32)
    out, touched = KR.mix_knn(dist[:1], idx1, np.array([[1.0, 1.0, np.inf, np.inf]], F32), vals, 0.5, 1.0)
    assert touched.sum() == 1 and touched[0, 6]
    assert abs(float(out[0, 6]) - (0.5 * float(dist[0, 6]) + 0.5)) < 1e-6


# ------------------------------------------------------------------------------------------------ KnnMT.check and the refusals
def test_check_refuses_each_wrong_value():
    st = fake_store()
    assert KnnMT(st).check(3).k == 8 and KnnMT(st, lam=0.0).active is False and KnnMT(st).active is True
    for kw, word in ((dict(k=0), "k = 0 outside 1..16"), (dict(k=17), "outside 1..16"), (dict(k=2.0), "outside 1..16"),
                     (dict(k=True), "outside 1..16"), (dict(lam=-0.1), "lam = .* outside \\[0, 1\\]"),
                     (dict(lam=1.5), "outside \\[0, 1\\]"), (dict(lam=float("nan")), "outside \\[0, 1\\]"),
                     (dict(lam="0.3"), "not a number"), (dict(temperature=0.0), "temperature = .* > 0"),
                     (dict(temperature=-1.0), "> 0"), (dict(temperature=float("inf")), "finite"),
                     (dict(exclude=[1, 2]), "2 exclude values for a batch of 3"), (dict(exclude=7), "not a sequence")):
        with pytest.raises(ValueError, match=word):
            KnnMT(st, **kw).check(3)
    with pytest.raises(ValueError, match="the store is empty"):
        KnnMT(fake_store(N=0)).check(3)
    with pytest.raises(ValueError, match="expected \\[N, 256\\]"):
        KnnMT(fake_store(width=128)).check(3)
    with pytest.raises(ValueError, match="not a retrieve.TokenStore"):
        KnnMT(object()).check(3)
    assert KnnMT(st, exclude=[4, None, -1]).check(3).exclude_rows() == [4, -1, -1]
    assert KnnMT(st, lam=0.25, temperature=4.0).coef().tolist() == [0.25, 0.25]


class NoLaunch:
    """A Searcher that fails the test if anything reaches the device: it has no model, no workspace and no loop."""

    def __init__(self, members=()):
        self.members, self.cfg = members, None

    _knn = Searcher._knn
    _no_knn = staticmethod(Searcher._no_knn)
    sample, score, sample_distinct, contrastive = Searcher.sample, Searcher.score, Searcher.sample_distinct, Searcher.contrastive


def test_the_searches_refuse_before_any_launch():
    st, s = fake_store(), NoLaunch()
    on, off = KnnMT(st), KnnMT(st, lam=0.0)
    for name, args in (("sample", (object(), 2)), ("score", (object(), [[2, 1]])), ("sample_distinct", (object(), 2)),
                       ("contrastive", (object(), 3))):
        with pytest.raises(ValueError, match="%s does not combine with knn=" % name):
            getattr(s, name)(*args, knn=on)
        with pytest.raises(ValueError, match="k = 0 outside"):
            getattr(s, name)(*args, knn=KnnMT(st, k=0))
        with pytest.raises(ValueError, match="expected decode.KnnMT"):
            getattr(s, name)(*args, knn=(st, 8))
        assert "knn" not in inspect.signature(getattr(Searcher, name)).parameters       # taken only to be refused
    assert s._knn(None, 3) is None and s._knn(off, 3) is None
    with pytest.raises(ValueError, match="does not combine with an ensemble"):
        NoLaunch(members=(object(),))._knn(on, 3)
    with pytest.raises(ValueError, match="does not combine with a neighbour"):
        s._knn(on, 3, object())
    with pytest.raises(ValueError, match="expected decode.KnnMT"):
        s._knn("store", 3)
    for name in ("greedy", "greedy_many", "beam", "sample_search"):
        assert inspect.signature(getattr(Searcher, name)).parameters["knn"].default is None


def test_the_key_carries_the_option_only_when_it_is_on():
    st = fake_store()
    kn = KnnMT(st, k=4)
    assert Searcher._key(("greedy", 4), False, None) == ("greedy", 4)
    assert Searcher._key(("greedy", 4), False, None, knn=None) == ("greedy", 4)
    assert Searcher._key(("beam", 4, 3), True, None, knn=kn) == ("beam", 4, 3, "merge", ("knn", 4, id(st)))
    assert Searcher._key(("beam", 4, 3), False, None, knn=KnnMT(st, k=4, lam=0.9, temperature=2.0)) == \
        Searcher._key(("beam", 4, 3), False, None, knn=kn)                    # lam and T are device values


# ------------------------------------------------------------------------------------------------ the store's rows
def test_values_resolve_copy_labels_the_way_an_entry_resolves():
    V, L, S = 10, 4, 3
    sou = np.array([[5, 6, 7, 8], [9, 4, 3, 5]])
    sub = np.array([[6, 9, 4], [7, 7, 8]])
    #               <start>  word  diff slot 2  sub slot 1   <eos>  <pad>
    lab = np.array([[2,      5,    V + 2,       V + L + 1,   1,     0],
                    [2,      V,    1,           0,           0,     0]])
    want = np.array([[2, 5, 7, 9, 1, 0], [2, 9, 1, 0, 0, 0]])
    assert np.array_equal(KR.resolve_labels(lab, sou, sub, V), want)
    assert np.array_equal(retrieve.resolve_labels(lab, sou, sub, V), want)
    b, t, value, owner = KR.store_rows(lab, sou, sub, V, commits=[40, 41])
    # step-major; <eos> is a value, <pad> positions are never stored, t < len - 1
    assert list(zip(b, t, value, owner)) == [(0, 0, 5, 40), (1, 0, 9, 41), (0, 1, 7, 40), (1, 1, 1, 41), (0, 2, 9, 40), (0, 3, 1, 40)]


def test_sum_sq_rows_is_the_ordered_float32_chain():
    rng = np.random.RandomState(3)
    x = (rng.standard_normal((7, 256)) * 3).astype(F32)
    got = retrieve.sum_sq_rows(torch.from_numpy(x)).numpy()
    assert np.array_equal(got.view(np.uint32), np.array([KR.sum_sq(r) for r in x], dtype=F32).view(np.uint32))


def test_token_store_checks_its_fields_and_round_trips(tmp_path):
    keys = torch.arange(3 * 256, dtype=torch.float32).reshape(3, 256) / 100
    st = retrieve.TokenStore(keys, [4, 5, 1], [0, 0, 1], checksum="abc")
    assert st.N == len(st) == 3 and st.values.dtype == torch.int32 and st.owner.tolist() == [0, 0, 1]
    assert torch.equal(st.key_sq, retrieve.sum_sq_rows(keys)) and st.nbytes == 3 * (1024 + 12)
    st.save(str(tmp_path / "tokens.pt"))
    back = retrieve.TokenStore.load(str(tmp_path / "tokens.pt"))
    for f in ("keys", "key_sq", "values", "owner"):
        assert torch.equal(getattr(back, f), getattr(st, f))
    assert back.checksum == "abc" and back.N == 3
    with pytest.raises(ValueError, match="3 keys, 2 values"):
        retrieve.TokenStore(keys, [4, 5], [0, 0, 1])
    torch.save({"format": 1}, str(tmp_path / "other.pt"))
    with pytest.raises(ValueError, match="not a token store file"):
        retrieve.TokenStore.load(str(tmp_path / "other.pt"))


# ------------------------------------------------------------------------------------------------ the ABI
def test_header_library_and_bindings_agree(lib):
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    for name, n_args in (("fira_knn_search_scratch_bytes", 3), ("fira_knn_search", 13), ("fira_mix_knn", 12)):
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert "knn.hip" in build.SOURCES and lib.fira_abi_version() == 11
    assert lib.fira_knn_search_scratch_bytes(0, 5, 8) == 0 and lib.fira_knn_search_scratch_bytes(3, 0, 8) == 0
    assert lib.fira_knn_search_scratch_bytes(3, 5, 17) == 0 and lib.fira_knn_search_scratch_bytes(3, 8388609, 8) == 0
    assert lib.fira_knn_search_scratch_bytes(65, 100, 8) == 2 * 2 * 64 * 8 * 8
    assert 0 < lib.fira_knn_search_scratch_bytes(192, 8388608, 16) <= 8 << 20
