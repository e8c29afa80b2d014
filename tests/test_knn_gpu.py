"""Token-level retrieval (kNN-MT) on the device: fira_knn_search and fira_mix_knn alone against the numpy statement of
knn_ref.py, then ``Searcher.greedy / beam(knn=...)`` on the golden commits: the option-off path, a store built from the batch
itself, exclusion, the other controls beside it and one captured graph for every lam / temperature."""
import ctypes as C

import numpy as np
import pytest
import torch

import knn_ref as KR
from search_kit import (best_pair, bits, count_calls, device_dims, golden_search, last_error, messages, offset_rows,
                        outside_untouched, same_search)
from fira_icse_amd import _lib, retrieve
from fira_icse_amd.config import EOS, START, UNK
from fira_icse_amd.decode import Constraints, KnnMT, Searcher

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 4


def dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype)


# ------------------------------------------------------------------------------------------------ fira_knn_search
def integer_rows(rng, n):
    """Rows with entries in {-2..2}: every product, partial sum and sum of squares is an integer below 2^24, so every fp32
    chain is exact whatever its order."""
    return rng.randint(-2, 3, (n, 256)).astype(F32)


def run_search(Q, keys, key_sq, K, owner=None, exclude=None):
    """The library's result, with guard words around both outputs."""
    lib = _lib.lib()
    R, N = Q.shape[0], keys.shape[0]
    n = R * K
    idx = torch.full((n + 2 * GUARD,), -77, dtype=torch.int32, device="cuda")
    d2 = torch.full((n + 2 * GUARD,), -77.0, dtype=torch.float32, device="cuda")
    nbytes = lib.fira_knn_search_scratch_bytes(R, N, K)
    assert (nbytes > 0) == (R > 0)
    scratch = torch.zeros(max(nbytes, 8) + 16, dtype=torch.uint8, device="cuda")
    scratch[nbytes:] = 0xAB
    dQ = dev(Q) if R else torch.zeros((1, 256), dtype=torch.float32, device="cuda")
    dk, dsq = dev(keys), dev(key_sq)
    dow = None if owner is None else dev(np.asarray(owner, dtype=np.int32))
    dex = None if exclude is None else dev(np.asarray(exclude, dtype=np.int32))
    _lib.check(lib.fira_knn_search(_lib.cur_stream(), _lib.ptr(dQ), R, _lib.ptr(dk), _lib.ptr(dsq), _lib.ptr(dow), _lib.ptr(dex), N, K,
                                   C.c_void_p(idx.data_ptr() + 4 * GUARD), C.c_void_p(d2.data_ptr() + 4 * GUARD),
                                   _lib.ptr(scratch), nbytes), "fira_knn_search")
    torch.cuda.synchronize()
    assert bool((idx[:GUARD] == -77).all()) and bool((idx[GUARD + n:] == -77).all())
    assert bool((d2[:GUARD] == -77).all()) and bool((d2[GUARD + n:] == -77).all())
    assert bool((scratch[nbytes:] == 0xAB).all())
    return idx[GUARD:GUARD + n].view(R, K).cpu().numpy(), d2[GUARD:GUARD + n].view(R, K).cpu().numpy()


def assert_search_equal(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what


# one N that spans several workgroups with a ragged tail: 256 workgroups x 4 waves x 16 rows = 16 384 rows fill the grid once
BIG_N = 16384 + 16 * 5 + 7


@pytest.fixture(scope="module")
def big():
    rng = np.random.RandomState(5)
    keys = integer_rows(rng, BIG_N)
    # duplicated keys across tile (15 | 16), wave (63 | 64 ...) and workgroup-stride boundaries; the tail row too
    for a, b in ((15, 16), (63, 64), (100, 16384 + 3), (31, BIG_N - 1), (4000, 9000)):
        keys[b] = keys[a]
    key_sq = KR.sum_sq_rows(keys)
    assert key_sq[5] == KR.sum_sq(keys[5])
    Q = integer_rows(rng, 65)
    for r, j in enumerate((15, 63, 100, 31, 4000)):
        Q[r] = keys[j]
    return keys, key_sq, Q


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65])
@pytest.mark.parametrize("K", [1, 8, 16])
def test_search_equals_the_statement_at_small_stores(big, N, K):
    """K > N gives void slots (idx -1, d2 +inf); every R in turn on the same store."""
    keys, key_sq, Q = big
    k, sq = keys[:N].copy(), key_sq[:N].copy()
    if N >= 17:
        k[16], sq[16] = k[3], sq[3]                               # a tie across the tile boundary
    for R in (0, 1, 16, 17, 64, 65):
        q = Q[:R].copy()
        if R:
            q[0] = k[min(3, N - 1)]
        got = run_search(q, k, sq, K)
        assert_search_equal(got, KR.knn_search(q, k, sq, K, exact=True), (N, K, R))
        if R and N >= 17 and K >= 2:
            assert got[0][0, 0] == 3 and got[0][0, 1] == 16 and got[1][0, 0] == 0
        if K > N and R:
            assert (got[0][:, N:] == -1).all() and np.isinf(got[1][:, N:]).all()


@pytest.mark.parametrize("R, K", [(1, 16), (17, 8), (64, 1), (65, 16)])
def test_search_equals_the_statement_across_workgroups(big, R, K):
    keys, key_sq, Q = big
    got = run_search(Q[:R], keys, key_sq, K)
    assert_search_equal(got, KR.knn_search(Q[:R], keys, key_sq, K, exact=True), (R, K))
    if K >= 2:                                                    # identical keys tie to the smaller index
        assert tuple(got[0][0, :2]) == (15, 16)
        if R >= 5:
            assert tuple(got[0][2, :2]) == (100, 16384 + 3) and tuple(got[0][3, :2]) == (31, BIG_N - 1)
            assert tuple(got[0][4, :2]) == (4000, 9000)


def test_exclude_removes_the_true_nearest_and_nan_never_wins(big):
    keys, key_sq, Q = big
    N, K, R = 2000, 8, 17
    k, sq, q = keys[:N].copy(), key_sq[:N].copy(), Q[:R].copy()
    owner = (np.arange(N) // 7).astype(np.int32)
    exclude = np.full(R, -1, dtype=np.int32)
    plain = KR.knn_search(q, k, sq, K, exact=True)
    for r in range(0, R, 2):
        exclude[r] = owner[plain[0][r, 0]]                        # the owner of the true nearest
    want = KR.knn_search(q, k, sq, K, owner=owner, exclude=exclude, exact=True)
    got = run_search(q, k, sq, K, owner, exclude)
    assert_search_equal(got, want, "exclude")
    for r in range(R):
        assert (got[0][r, 0] != plain[0][r, 0]) == (r % 2 == 0)
        assert (owner[got[0][r]] != exclude[r]).all()
    assert_search_equal(run_search(q, k, sq, K, owner, None), plain, "owner without exclude")
    # every row of one owner: a store with fewer admissible rows than K
    few = run_search(q[:1], k[:14], sq[:14], K, owner[:14], np.array([0], np.int32))
    assert_search_equal(few, KR.knn_search(q[:1], k[:14], sq[:14], K, owner=owner[:14], exclude=[0], exact=True), "few")
    assert (few[0][0, 7:] == -1).all()
    # a NaN key (and its NaN sum of squares) never wins, wherever it sits
    for j in (int(plain[0][0, 0]), 0, N - 1):
        kb, sb = k.copy(), sq.copy()
        kb[j, 9] = np.nan
        sb[j] = np.nan
        got = run_search(q, kb, sb, K)
        assert not (got[0] == j).any()
        assert_search_equal(got, KR.knn_search(q, kb, sb, K, exact=True), "nan")


def test_search_refuses_bad_arguments_before_any_launch():
    lib = _lib.lib()
    t = torch.zeros(64 * 256, dtype=torch.float32, device="cuda")
    i = torch.zeros(64 * 16, dtype=torch.int32, device="cuda")
    o, o2 = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(64, dtype=torch.float32, device="cuda")
    scratch = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = _lib.ptr
    base = dict(Q=p(t), R=2, keys=p(t), key_sq=p(t), owner=p(i), exclude=p(i), N=20, K=4, idx=p(o), d2=p(o2), scratch=p(scratch),
                nbytes=scratch.numel())

    def call(**kw):
        a = dict(base, **kw)
        return lib.fira_knn_search(_lib.cur_stream(), a["Q"], a["R"], a["keys"], a["key_sq"], a["owner"], a["exclude"], a["N"], a["K"],
                                   a["idx"], a["d2"], a["scratch"], a["nbytes"])
    assert call() == 0
    for kw, word in ((dict(R=-1), "negative"), (dict(N=0), "empty"), (dict(N=8388609), "more than"), (dict(K=0), "K = 0"),
                     (dict(K=17), "K = 17"), (dict(owner=None), "exclude without owner"), (dict(Q=None), "null pointer"),
                     (dict(key_sq=None), "null pointer"), (dict(idx=None), "null pointer"), (dict(scratch=None), "null pointer"),
                     (dict(Q=C.c_void_p(t.data_ptr() + 4)), "16-byte aligned"), (dict(nbytes=8), "needed"),
                     (dict(scratch=C.c_void_p(scratch.data_ptr() + 4)), "8-byte aligned")):
        assert call(**kw) != 0, kw
        assert "fira_knn_search" in last_error() and word in last_error(), (kw, last_error())
    assert call(R=0, Q=None, idx=None, d2=None, scratch=None, nbytes=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ fira_mix_knn
MIX_V, MIX_L, MIX_S = 1061, 7, 4                                  # W = 1072: a head, vectors and a tail at most alignments
MIX_W = MIX_V + MIX_L + MIX_S


def mix_case(rng, R, K, N=50):
    dist = rng.dirichlet(np.ones(MIX_W) * 0.3, R).astype(F32)
    values = rng.permutation(MIX_V)[:N].astype(np.int32)
    idx = np.stack([rng.choice(N, K, replace=False) for _ in range(R)]).astype(np.int32)
    d2 = np.sort(rng.uniform(0, 30, (R, K)).astype(F32), axis=1)
    return dist, values, idx, d2


def run_mix(dist, idx, d2, values, lam, inv_T, offset=0, best=True):
    R, K = idx.shape
    d = device_dims(vocab=MIX_V, sou_len=MIX_L, sub_len=MIX_S)
    buf, view = offset_rows(dist, offset, fill=-3.0)
    bid, bp = best_pair(R, best)
    coef, d_idx, d_d2, d_values = dev(np.array([lam, inv_T], dtype=F32)), dev(idx), dev(d2), dev(values)     # (kept alive)
    _lib.check(_lib.lib().fira_mix_knn(_lib.cur_stream(), C.byref(d), R, _lib.ptr(d_idx), _lib.ptr(d_d2), _lib.ptr(d_values),
                                       len(values), K, _lib.ptr(coef), _lib.ptr(view), _lib.ptr(bid), _lib.ptr(bp)), "fira_mix_knn")
    torch.cuda.synchronize()
    outside_untouched(buf, offset, dist.size, fill=-3.0)
    return view.cpu().numpy(), (None if bid is None else bid.cpu().numpy()), (None if bp is None else bp.cpu().numpy())


def assert_mix(got, dist, idx, d2, values, lam, inv_T, what):
    """Untouched entries fl((1 - lam) p) bit for bit; touched entries within 2e-6 relative of the fp64 statement (one expf, a
    sum of at most 16 terms, one division, two multiplies and one add: under 16 ulp)."""
    out, bid, bp = got
    want, touched = KR.mix_knn(dist, idx, d2, values, lam, inv_T)
    assert np.array_equal(out[~touched].view(np.uint32), want[~touched].view(np.uint32)), what
    f64 = KR.mix_knn_f64(dist, idx, d2, values, lam, inv_T)
    rel = np.abs(out[touched].astype(np.float64) - f64[touched]) / f64[touched]
    print("%s: %d touched entries, max relative error %.3g" % (what, int(touched.sum()), rel.max() if rel.size else 0.0))
    assert (rel <= 2e-6).all(), what
    if bid is not None:                                           # the arg-max of the row as stored, first occurrence
        assert np.array_equal(bid, out.argmax(1)) and np.array_equal(bp.view(np.uint32), out.max(1).view(np.uint32)), what
    return touched


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_mix_equals_the_statement_at_every_row_alignment(offset):
    rng = np.random.RandomState(20 + offset)
    R, K = 5, 8
    dist, values, idx, d2 = mix_case(rng, R, K)
    values[idx[0, 2]] = values[idx[0, 0]]                         # row 0: one word in three slots, accumulated in slot order
    values[idx[0, 5]] = values[idx[0, 0]]
    idx[1, :] = -1                                                # row 1: every slot void -> left alone
    d2[1, :] = np.inf
    idx[2, 3:] = -1                                               # row 2: void slots after three found
    d2[2, 3:] = np.inf
    values[idx[3, 0]] = MIX_V - 1                                 # row 3: the last generator entry, and a value that wins the row
    dist[4, MIX_W - 1] = 0.9                                      # row 4: the arg-max in the tail
    touched = assert_mix(run_mix(dist, idx, d2, values, 0.4, 0.5, offset), dist, idx, d2, values, 0.4, 0.5, "offset %d" % offset)
    words = lambda r: set(values[idx[r][idx[r] >= 0]].tolist())
    assert touched[0].sum() == len(words(0)) <= K - 2 and not touched[1].any() and touched[2].sum() == len(words(2)) <= 3
    out, _, _ = run_mix(dist, idx, d2, values, 0.4, 0.5, offset, best=False)
    assert out[1].tobytes() == dist[1].tobytes()
    # nothing is renormalised: a row that sums to 1 (rows 0..3) still does, within the roundings of its 1072 entries
    assert np.abs(out[:4].sum(1, dtype=np.float64) - dist[:4].sum(1, dtype=np.float64)).max() < 1e-5


@pytest.mark.parametrize("K", [1, 16])
def test_mix_lambda_zero_is_bit_identity_and_lambda_one_keeps_the_words_only(K):
    rng = np.random.RandomState(31 + K)
    dist, values, idx, d2 = mix_case(rng, 3, K)
    dist[0, 5] = -0.0
    out, bid, bp = run_mix(dist, idx, d2, values, 0.0, 0.1, offset=1)
    assert out.tobytes() == dist.tobytes()
    assert np.array_equal(bid, dist.argmax(1)) and np.array_equal(bp, dist.max(1))
    assert_mix(run_mix(dist, idx, d2, values, 1.0, 0.1, offset=2), dist, idx, d2, values, 1.0, 0.1, "lam 1, K %d" % K)
    assert_mix(run_mix(dist, idx, d2, values, 0.3, 2.0), dist, idx, d2, values, 0.3, 2.0, "K %d" % K)


def test_mix_refuses_bad_arguments_before_any_launch():
    lib, d = _lib.lib(), device_dims(vocab=MIX_V, sou_len=MIX_L, sub_len=MIX_S)
    f = torch.zeros(2 * MIX_W + 8, dtype=torch.float32, device="cuda")
    i = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = _lib.ptr
    base = dict(R=2, idx=p(i), d2=p(f), values=p(i), N=10, K=4, coef=p(f), dist=p(f), bid=None, bp=None)

    def call(**kw):
        a = dict(base, **kw)
        return lib.fira_mix_knn(_lib.cur_stream(), C.byref(d), a["R"], a["idx"], a["d2"], a["values"], a["N"], a["K"], a["coef"],
                                a["dist"], a["bid"], a["bp"])
    assert call() == 0
    for kw, word in ((dict(R=-1), "negative"), (dict(N=0), "N = 0"), (dict(K=0), "K = 0"), (dict(K=17), "K = 17"),
                     (dict(idx=None), "null pointer"), (dict(coef=None), "null pointer"), (dict(dist=None), "null pointer"),
                     (dict(bid=p(i)), "together"), (dict(dist=C.c_void_p(f.data_ptr() + 2)), "4-byte aligned")):
        assert call(**kw) != 0, kw
        assert "fira_mix_knn" in last_error() and word in last_error(), (kw, last_error())
    assert call(R=0, idx=None, d2=None, values=None, coef=None, dist=None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the searches
@pytest.fixture(scope="module")
def setup():
    g = golden_search(weights="spread", searchers=2)
    search, builder = g.searchers
    store = retrieve.TokenStore.build(builder, [(list(g.ids), g.db)])
    return dict(cfg=g.cfg, db=g.db, hb=g.host_batch, ids=[int(i) for i in g.ids], model=g.model, search=search, store=store)


def test_the_store_holds_one_row_per_reference_token(setup):
    cfg, hb, store, ids = setup["cfg"], setup["hb"], setup["store"], setup["ids"]
    b, t, value, owner = KR.store_rows(hb.tar_label, hb.sou, hb.sub_token, cfg.vocab_size, ids)
    assert store.N == len(b) > 0 and store.keys.shape == (store.N, 256)
    assert np.array_equal(store.values.cpu().numpy(), value) and np.array_equal(store.owner.cpu().numpy(), owner)
    assert (value != 0).all() and (value == EOS).any()
    keys = store.keys.cpu().numpy()
    assert np.isfinite(keys).all()
    want_sq = np.array([KR.sum_sq(k) for k in keys], dtype=F32)
    assert np.array_equal(store.key_sq.cpu().numpy().view(np.uint32), want_sq.view(np.uint32))


def test_off_and_lambda_zero_are_todays_search_launch_for_launch(setup, monkeypatch):
    db, store, model = setup["db"], setup["store"], setup["model"]
    B = db.B
    fresh = Searcher(model)
    zero = KnnMT(store, lam=0.0)
    want_g, want_b = fresh.greedy(db), fresh.beam(db, 3)
    for kn in (None, zero):
        for use_graphs in (False, True):
            same_search(fresh.greedy(db, use_graphs=use_graphs, knn=kn), want_g)
            same_search(fresh.beam(db, 3, use_graphs=use_graphs, knn=kn), want_b)
    assert set(fresh._ws) == {(B, 3), (B, 1), ("beam", B, 3), ("greedy", B)}          # no new buffer
    plain_g = count_calls(monkeypatch, lambda: fresh.greedy(db, use_graphs=False))
    plain_b = count_calls(monkeypatch, lambda: fresh.beam(db, 3, use_graphs=False))
    for kn in (None, zero):
        assert count_calls(monkeypatch, lambda: fresh.greedy(db, use_graphs=False, knn=kn)) == plain_g
        assert count_calls(monkeypatch, lambda: fresh.beam(db, 3, use_graphs=False, knn=kn)) == plain_b
    assert not any("knn" in name for name in list(plain_g) + list(plain_b))
    # on: three more calls per step
    on = KnnMT(store, k=4)
    fresh.greedy(db, knn=on)
    kw = fresh._ws[("knn", B, 1, 4, id(store))]
    st = fresh._ws[("greedy", B, ("knn", 4, id(store)))]
    assert count_calls(monkeypatch, lambda: fresh._greedy_steps(st, kw, B, 0, 1)) == \
        {"fira_decode_step_ex": 1, "fira_decode_hidden": 1, "fira_knn_search": 1, "fira_mix_knn": 1, "fira_greedy_advance": 1}


def test_greedy_follows_the_reference_messages_of_a_store_built_from_the_batch(setup):
    """The hidden states along a commit's reference path are stored keys (d2 = 0 up to the rounding of the two chains), so
    with a small temperature the slots' weight sits on the row that holds the reference's next word, and with lam = 0.9
    that word has at least 0.9 w_0 of the mixed row."""
    cfg, db, hb, store, search = setup["cfg"], setup["db"], setup["hb"], setup["store"], setup["search"]
    words = KR.resolve_labels(hb.tar_label, hb.sou, hb.sub_token, cfg.vocab_size)
    want = []
    for b in range(db.B):
        n = int((np.asarray(hb.tar_label)[b] != 0).cumprod().sum())
        row = [int(w) for w in words[b, 1:n]]
        want.append(row[:row.index(EOS) + 1] if EOS in row else row)
    for use_graphs in (False, True):
        gen, length, prob = search.greedy(db, use_graphs=use_graphs, knn=KnnMT(store, k=8, lam=0.9, temperature=0.01))
        got = messages(gen, length)
        kw = search._ws[("knn", db.B, 1, 8, id(store))]
        print("d2 of the last step's slots (commit 0):", kw.d2[0].cpu().tolist())
        assert got == want, [(b, g, w) for b, (g, w) in enumerate(zip(got, want)) if g != w]
        assert bool((prob > 0).all())


def test_exclude_keeps_a_commits_own_rows_out_of_its_mix(setup):
    db, store, search, ids = setup["db"], setup["store"], setup["search"], setup["ids"]
    B, beam = db.B, 3
    kn = KnnMT(store, k=8, lam=0.5, temperature=10.0, exclude=ids)
    gen, length, prob = search.beam(db, beam, use_graphs=False, knn=kn)
    assert bool((prob.view(B, beam)[:, 0] > 0).all()) and bool((length.view(B, beam)[:, 0] > 1).all())
    # one instrumented step: what the last step's search returned for every (commit, slot) row
    kw = search._ws[("knn", B, beam, 8, id(store))]
    idx = kw.idx.cpu().numpy()
    owner = store.owner.cpu().numpy()
    assert kw.exclude.cpu().tolist() == [i for i in ids for _ in range(beam)]
    found = 0
    for r in range(B * beam):
        live = idx[r][idx[r] >= 0]
        found += len(live)
        assert (owner[live] != ids[r // beam]).all(), r
    assert found > 0
    # without exclude the nearest row of a commit's first step is its own
    search.greedy(db, use_graphs=False, knn=KnnMT(store, k=8, lam=0.5))
    own = search._ws[("knn", B, 1, 8, id(store))]
    assert own.exclude.cpu().tolist() == [-1] * B


def test_the_other_controls_hold_beside_the_option(setup):
    cfg, db, store, search = setup["cfg"], setup["db"], setup["store"], setup["search"]
    B, beam = db.B, 3
    plain = search.best(*search.greedy(db, merge_copies=True))
    banned = tuple(sorted({w for m in plain for w in m if w > UNK}))[:3]
    con = Constraints(no_repeat_ngram=2, min_length=3, banned=banned)
    first = [w for w in range(UNK + 1, UNK + 40) if w not in banned][:B]
    prefix = [[first[b], first[(b + 1) % B]] if b % 2 == 0 else [] for b in range(B)]
    for use_graphs in (False, True):
        gen, length, prob = search.beam(db, beam, use_graphs=use_graphs, constraints=con, merge_copies=True, prefix=prefix,
                                        knn=KnnMT(store, k=8, lam=0.5, temperature=5.0))
        gen, length, prob = gen.view(B, beam, -1).cpu(), length.view(B, beam).cpu(), prob.view(B, beam).cpu()
        assert bool((prob[:, 0] > 0).all())
        for b in range(B):
            seen = set()
            for s in range(beam):
                if not prob[b, s] > 0:
                    continue
                msg = gen[b, s, 1:int(length[b, s])].tolist()
                assert msg[:len(prefix[b])] == prefix[b], (b, s, msg)
                assert not set(msg) & set(banned), (b, s, msg)
                grams = list(zip(msg, msg[1:]))
                assert len(grams) == len(set(grams)), (b, s, msg)
                if EOS in msg:
                    assert msg.index(EOS) >= 3, (b, s, msg)
                assert tuple(msg) not in seen, (b, s, msg)            # merged: distinct word sequences
                seen.add(tuple(msg))


def test_one_captured_graph_serves_every_lambda_and_temperature(setup):
    db, store, model = setup["db"], setup["store"], setup["model"]
    B = db.B
    graphed, eager = Searcher(model), Searcher(model)
    a, b = KnnMT(store, k=8, lam=0.3, temperature=10.0), KnnMT(store, k=8, lam=0.8, temperature=0.5)
    got_a = graphed.beam(db, 3, knn=a)
    key = ("beam", B, 3, ("knn", 8, id(store)))
    graphs = graphed._ws[key]["graphs"]
    assert graphs is not None and len(graphs) > 0
    keys_before = set(graphed._ws)
    got_b = graphed.beam(db, 3, knn=b)
    assert graphed._ws[key]["graphs"] is graphs and all(x is y for x, y in zip(graphed._ws[key]["graphs"], graphs))
    assert set(graphed._ws) == keys_before                        # no new state, no new capture
    same_search(got_a, eager.beam(db, 3, use_graphs=False, knn=a))
    same_search(got_b, eager.beam(db, 3, use_graphs=False, knn=b))
    assert not all(torch.equal(x, y) for x, y in zip(got_a, got_b))
    g_b = graphed.greedy(db, knn=b)
    same_search(graphed.greedy(db, knn=a), eager.greedy(db, use_graphs=False, knn=a))
    same_search(g_b, eager.greedy(db, use_graphs=False, knn=b))
    with pytest.raises(ValueError, match="does not combine with an ensemble"):
        Searcher(model, members=(model,)).greedy(db, knn=a)
