"""Sampling from the search's edited distribution on the device (fira_sample_dist / Searcher.sample_search): on the fused
sampler's own rows the kernel draws what the fused sampler draws, bit for bit; on synthetic edited rows (unnormalised, with
zeros, at every alignment) it follows the numpy statement (sample_search_ref.py) and reproduces the recorded draws of
tests/golden/sampler_draws.npz bit for bit; the draws follow the filtered law of an edited
row; top_k = 1 is the edit chain's arg-max; sample_search without options is sample, with options it honours them, and its
exact reductions (greedy, a (1, 0) ensemble, a neighbour with lam = 0) hold; the calls per step; the library's argument errors."""
import ctypes as C
import functools
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import sample_ref
import sample_search_ref as ref
import util
from search_kit import (best_pair, bits, count_calls, device_dims, golden_search, last_error, messages, offset_rows,
                        outside_untouched, seed_tensor, spread_state_dict)
from test_sample_gpu import FILTERS
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, START

pytestmark = pytest.mark.gpu

OFF = dict(min_p=0.0, epsilon=0.0, eta=0.0, typical_p=1.0)
# for each cut one setting alone, and one combination of the three thresholds (on top of temperature and top-p)
CUTS = [dict(min_p=0.02), dict(epsilon=0.0005), dict(eta=0.0003), dict(typical_p=0.9),
        dict(temperature=1.3, top_p=0.9, min_p=0.02, epsilon=0.001, eta=0.003)]


def sample_dist(d, R, rpc, step, dist, key, seed, best_id, best_p, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, epsilon=0.0,
                eta=0.0, typical_p=1.0):
    """fira_sample_dist; returns the library's code (0 = launched)."""
    return _lib.lib().fira_sample_dist(_lib.cur_stream(), C.byref(d), R, rpc, step, _lib.ptr(dist), _lib.ptr(key), _lib.ptr(seed),
                                       float(temperature), int(top_k), float(top_p), float(min_p), float(epsilon), float(eta),
                                       float(typical_p), _lib.ptr(best_id), _lib.ptr(best_p))


@pytest.fixture(scope="module")
def setup():
    from fira_icse_amd.model import TransModel
    g = golden_search(weights="peaked", searchers=0, seed=2)
    spread = TransModel(g.cfg, init=False)
    spread.load_state_dict(spread_state_dict(g.cfg))
    spread.eval()
    return g.cfg, g.store, g.ids, g.model, spread, g.db


# ------------------------------------------------------------------------------------------------ 1. the fused sampler's rows
@pytest.mark.parametrize("n", [1, 3])
def test_on_the_fused_samplers_own_rows_the_draw_is_the_fused_samplers_bit_for_bit(setup, n):
    """fira_decode_step_sample_cut with dist out, then fira_sample_dist on that dist: equal best_id, best_p equal as bits, on
    every row, for every filter triple of test_sample_gpu and every cut.  No tolerance, no cap."""
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, db = setup
    search = Searcher(spread)
    m, B, W = spread, db.B, cfg.out_len
    R = B * n
    ws = search._begin(db, n)
    key = torch.tensor([7, 11, 13, 17], dtype=torch.int32, device="cuda")[:B]
    seed = seed_tensor(0x1234567890ABCDEF)
    dist = torch.empty(R, W, device="cuda")
    gen = torch.Generator().manual_seed(5)
    settings = [dict(temperature=t, top_k=k, top_p=p) for t, k, p in FILTERS] + CUTS
    for step in range(6):
        tok = torch.randint(4, 3000, (R,), generator=gen).to(torch.int32).cuda() if step else \
            torch.full((R,), 2, dtype=torch.int32, device="cuda")
        if step not in (0, 1, 5):
            search._step(ws, B, n, step, tok, None, dist, None, None)
            continue
        for kw in settings:
            full = dict(dict(temperature=1.0, top_k=0, top_p=1.0, **OFF), **kw)
            (bid_a, bp_a), (bid_b, bp_b) = best_pair(R), best_pair(R)
            _lib.check(_lib.lib().fira_decode_step_sample_cut(
                _lib.cur_stream(), C.byref(m.dims), _lib.ptr(m.flat.data), _lib.ptr(ws), ws.numel(), B, n, step, _lib.ptr(tok),
                _lib.ptr(key), _lib.ptr(seed), full["temperature"], full["top_k"], full["top_p"], full["min_p"], full["epsilon"],
                full["eta"], full["typical_p"], _lib.ptr(dist), _lib.ptr(bid_a), _lib.ptr(bp_a), 0), "fira_decode_step_sample_cut")
            assert sample_dist(m.dims, R, n, step, dist, key, seed, bid_b, bp_b, **full) == 0, last_error()
            torch.cuda.synchronize()
            assert torch.equal(bid_a, bid_b), (step, kw)
            assert torch.equal(bits(bp_a), bits(bp_b)), (step, kw)
            assert int(bid_b.min()) >= 0 and int(bid_b.max()) < W and float(bp_b.min()) > 0


# ------------------------------------------------------------------------------------------------ 2. synthetic edited rows
GEOMETRIES = [(7, 3, 0), (1025, 5, 4), (25600, 370, 654)]         # the last: the register-resident maximum
ROW_SETTINGS = [dict(), dict(temperature=1.3, top_k=5), dict(temperature=0.8, top_p=0.9), dict(temperature=1.5, top_k=50, top_p=0.9),
                dict(temperature=1.7, epsilon=0.002), dict(top_p=0.95, min_p=0.02, eta=0.003), dict(top_k=40, typical_p=0.8)]
RPC, STEP, SEED = 2, 3, 0x0BADC0FFEE123457
KEYS = [5, 40, 77, 1000003]
GUARD = 7.5                                                          # a guard word read as an entry would win every draw


def synthetic_rows(V, L, S):
    """Eight unnormalised rows (sum about 0.4) as an edit chain may leave them: three random positive rows; the same with 60 %
    of the entries 0, the former maximum among them; a row with one positive entry; an all-zero row."""
    W = V + L + S
    rng = np.random.default_rng(1000 + W)
    full = np.exp(rng.standard_normal((3, W)) * 2.5)
    holed = full.copy()
    for r in range(3):
        gone = rng.random(W) < 0.6
        gone[int(np.argmax(full[r]))] = True
        if gone.all():
            gone[int(np.argmin(full[r]))] = False
        holed[r, gone] = 0.0
    one = np.zeros((1, W))
    one[0, int(rng.integers(0, W))] = 1.0
    rows = np.concatenate([full, holed, one], 0)
    rows = rows * (0.4 / rows.sum(1, keepdims=True))
    return np.concatenate([rows, np.zeros((1, W))], 0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def row_reference(V, L, S):
    """(rows, tar_len, per setting: the statement's (id, clear) per row and the relaxed masks) -- computed once per geometry."""
    rows = synthetic_rows(V, L, S)
    W, T = V + L + S, device_dims(V, L, S).tar_len
    out = []
    for kw in ROW_SETTINGS:
        kw = dict(kw, top_k=min(kw.get("top_k", 0), W))
        draws = [ref.draw(rows[r], KEYS[r // RPC], SEED, r % RPC, T, STEP, **kw) for r in range(len(rows))]
        relaxed = [ref.kept(rows[r], **kw)[1] for r in range(len(rows))]
        out.append((kw, [d[0] for d in draws], [d[2] for d in draws], relaxed))
    return rows, T, out


def test_the_statement_alone_decides_nine_rows_in_ten():
    """The share of (row, setting) pairs whose draw the numpy statement calls clear (gap > 1e-4, strict and relaxed pick agree),
    computed without the device: 1.0 (168 of 168) over the three geometries with the seeds above."""
    clear = [c for g in GEOMETRIES for _, _, cl, _ in row_reference(*g)[2] for c in cl]
    print("clear: %d of %d" % (sum(clear), len(clear)))
    assert sum(clear) >= 0.9 * len(clear)


@pytest.mark.parametrize("V,L,S", GEOMETRIES)
def test_synthetic_edited_rows_at_every_alignment_follow_the_statement(V, L, S):
    rows, T, per_setting = row_reference(V, L, S)
    R, W = rows.shape
    d = device_dims(V, L, S)
    key = torch.tensor(KEYS, dtype=torch.int32, device="cuda")
    seed = seed_tensor(SEED)
    want_bits = bits(rows)
    compared = total = 0
    for offset in range(4):
        buf, view = offset_rows(rows, offset, fill=GUARD)
        for kw, want_id, clear, relaxed in per_setting:
            bid, bp = best_pair(R)
            assert sample_dist(d, R, RPC, STEP, view, key, seed, bid, bp, **kw) == 0, last_error()
            torch.cuda.synchronize()
            got, got_p = bid.cpu().numpy(), bp.cpu().numpy()
            for r in range(R):
                total += 1
                if not (rows[r] > 0).any():                          # the documented pair of a row without a positive entry
                    assert (int(got[r]), float(got_p[r])) == ref.EMPTY and not np.signbit(got_p[r])
                else:
                    assert 0 <= got[r] < W and relaxed[r][got[r]] and rows[r, got[r]] > 0, (offset, kw, r)
                    assert got_p[r].view(np.int32) == rows[r, got[r]].view(np.int32), (offset, kw, r)
                if clear[r]:
                    assert int(got[r]) == want_id[r], (offset, kw, r)
                    compared += 1
            # dist and the guard words: bitwise untouched
            assert torch.equal(bits(view.cpu()), want_bits) and outside_untouched(buf, offset, R * W, fill=GUARD)
    assert compared >= 0.8 * total


def test_recorded_draws_are_reproduced_bit_for_bit():
    """tests/golden/sampler_draws.npz (scripts/record_sampler_draws.py: recorded from the library before the sampler body was
    shared between sample.hip and sample_row.hip) replayed: every best_id equal, every best_p equal as bits -- 3 geometries x
    4 offsets x 9 settings x 32 rows (4 kinds under 8 noise streams) = 3 456 draws, no tolerance.  The small geometries' rows come from the fixture, the large
    one from the script's integer formula."""
    spec = importlib.util.spec_from_file_location("record_sampler_draws", os.path.join(util.REPO, "scripts", "record_sampler_draws.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    fx = np.load(os.path.join(util.REPO, "tests", "golden", "sampler_draws.npz"))
    assert [tuple(g) for g in fx["geometries"].tolist()] == GEOMETRIES and tuple(fx["fields"]) == rec.FIELDS
    compared = 0
    for g in GEOMETRIES:
        name = rec.name(g)
        stored = "rows_" + name in fx.files
        rows = fx["rows_" + name] if stored else rec.pinned_rows(sum(g))
        assert stored == (g in rec.STORED) and [int((r > 0).sum()) for r in rows[2:]] == [1, 0]
        assert (rows[0] > 0).all() and (rows[1] == 0).sum() > 0.4 * rows.shape[1] and rows[1, rows[0].argmax()] == 0
        table = fx["settings_" + name]
        for k, f in enumerate(rec.FIELDS):                                   # every filter and cut is on somewhere, off somewhere
            on = table[:, k] != rec.DEFAULTS[f]
            assert on.any() and not on.all(), f
        ids, p_bits = rec.replay(g, rows, table, int(fx["rpc"]), int(fx["step"]), int(fx["seed"]), fx["keys"].tolist())
        assert np.array_equal(ids, fx["best_id_" + name]), np.argwhere(ids != fx["best_id_" + name])[:5]
        assert np.array_equal(p_bits, fx["best_p_bits_" + name]), np.argwhere(p_bits != fx["best_p_bits_" + name])[:5]
        assert (ids[:, :, 3::4] == 0).all() and (p_bits[:, :, 3::4] == 0).all()   # the empty rows' documented pair
        compared += ids.size
    assert compared == 3456


# ------------------------------------------------------------------------------------------------ 3. the law of the draws
@pytest.mark.parametrize("temp,k,p", [(2.0, 0, 1.0), (1.5, 20, 1.0), (1.0, 0, 0.9)])
def test_draws_follow_the_filtered_law_of_an_edited_row(temp, k, p):
    """64 keys x 8 rows x 8 seeds = 4 096 draws from one synthetic row with zeros at vocab 1025, against the filtered,
    renormalised q of the numpy twin: the bounds of test_sample_gpu.test_draws_follow_the_filtered_distribution."""
    V, L, S = GEOMETRIES[1]
    W, B, n = V + L + S, 64, 8
    row = synthetic_rows(V, L, S)[3]
    assert (row == 0).sum() > 0.5 * W and abs(float(row.sum()) - 0.4) < 0.05
    d = device_dims(V, L, S)
    dist = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(row, (B * n, W)))).cuda()
    key = torch.arange(B, dtype=torch.int32, device="cuda")
    draws = []
    for s in range(8):
        bid, bp = best_pair(B * n)
        assert sample_dist(d, B * n, n, 0, dist, key, seed_tensor(1000 + s), bid, bp, temperature=temp, top_k=k, top_p=p) == 0
        torch.cuda.synchronize()
        draws.append(bid.long().cpu().numpy())
    draws = np.concatenate(draws)
    row64 = row.astype(np.float64)
    q, keep = sample_ref.filtered_q(row64, temp, k, p)
    relaxed = sample_ref.kept_mask(row64, temp, k, p, rel=1e-4) & (row64 > 0)
    assert relaxed[draws].all()
    N = len(draws)
    counts = np.bincount(draws, minlength=W)
    big = q * N >= 5                                  # entries with an expectation of >= 5 draws: one by one
    sig = np.sqrt(N * q * (1 - q))
    assert (np.abs(counts[big] - N * q[big]) <= 5 * sig[big] + 1).all()
    rest_q = q[~big].sum()                            # the long tail as one pooled entry
    assert abs(counts[~big].sum() - N * rest_q) <= 5 * np.sqrt(N * rest_q * (1 - rest_q)) + 1
    assert big.sum() >= 2


# ------------------------------------------------------------------------------------------------ 4. top_k = 1
def test_top_k_one_is_the_edit_chains_arg_max_on_rows_with_a_unique_maximum():
    V, L, S = GEOMETRIES[1]
    rows = synthetic_rows(V, L, S)[:7]                               # (the all-zero row has no unique maximum)
    R, W = rows.shape
    top2 = np.sort(rows, 1)[:, -2:]
    assert (top2[:, 1] > top2[:, 0]).all()
    d = device_dims(V, L, S)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    gen, length, banned = i32(R, d.tar_len), i32(R), i32(1)
    gen[:, 0] = START
    length.fill_(1)
    for offset in (0, 3):
        buf, view = offset_rows(rows, offset, fill=GUARD)
        cid, cp = best_pair(R)
        _lib.check(_lib.lib().fira_constrain_dist(_lib.cur_stream(), C.byref(d), R, 1, _lib.ptr(gen), _lib.ptr(length),
                                                  _lib.ptr(i32(R, L)), _lib.ptr(i32(R, S)), 0, 0, _lib.ptr(banned), 0,
                                                  _lib.ptr(view), _lib.ptr(cid), _lib.ptr(cp)), "fira_constrain_dist")
        for temp in (1.0, 1.7):
            bid, bp = best_pair(R)
            assert sample_dist(d, R, 1, 2, view, torch.arange(R, dtype=torch.int32, device="cuda"), seed_tensor(3), bid, bp,
                               temperature=temp, top_k=1) == 0, last_error()
            torch.cuda.synchronize()
            assert torch.equal(bid, cid) and torch.equal(bits(bp), bits(cp))
            assert np.array_equal(bid.cpu().numpy(), rows.argmax(1))


# ------------------------------------------------------------------------------------------------ 5. without options
def same_samples(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:2], b[:2])) and all(torch.equal(bits(x), bits(y)) for x, y in zip(a[2:], b[2:]))


@pytest.mark.parametrize("n", [1, 3])
def test_without_options_sample_search_is_sample_bit_for_bit(setup, n):
    from fira_icse_amd.decode import Searcher
    from fira_icse_amd.model import DeviceBatch
    cfg, store, ids, peaked, spread, db = setup
    search = Searcher(spread)
    for kw in (dict(), dict(temperature=1.5, top_k=50, top_p=0.9), dict(temperature=0.8, top_p=0.9), dict(temperature=2.0, epsilon=0.02)):
        a = search.sample(db, n, seed=4, use_graphs=False, **kw)
        b = search.sample_search(db, n, seed=4, use_graphs=False, **kw)
        assert same_samples(a, b), kw
        assert a[0].shape == b[0].shape == (db.B, n, cfg.tar_len) and b[3].shape == (db.B, n)
    if n == 1:
        return
    kw = dict(temperature=2.0)
    eager = search.sample_search(db, n, seed=4, use_graphs=False, **kw)
    captured = search.sample_search(db, n, seed=4, **kw)
    replayed = search.sample_search(db, n, seed=4, **kw)
    assert same_samples(eager, captured) and same_samples(eager, replayed)
    assert same_samples(replayed, search.sample(db, n, seed=4, use_graphs=False, **kw))
    other = search.sample_search(db, n, seed=5, **kw)                # the seed is a device value: the same capture
    assert not torch.equal(eager[0], other[0])
    assert ("sample_search", db.B, n, 2.0, 0, 1.0) + Searcher.CUTS_OFF in search._ws
    # a commit's samples depend on its key, not on its row: the batch and the keys permuted together
    perm = [2, 0, 3, 1]
    moved = search.sample_search(DeviceBatch(store.batch([ids[i] for i in perm]), cfg), n, seed=4, keys=perm, use_graphs=False, **kw)
    assert torch.equal(moved[0], eager[0][perm]) and torch.equal(moved[1], eager[1][perm])
    rekeyed = search.sample_search(db, n, seed=4, keys=[9, 8, 7, 6], use_graphs=False, **kw)
    assert not torch.equal(rekeyed[0], eager[0])


# ------------------------------------------------------------------------------------------------ 6. options
def test_options_hold_on_every_sample_and_logp_is_the_running_sum(setup):
    from fira_icse_amd.decode import Constraints, Searcher
    cfg, store, ids, peaked, spread, db = setup
    search = Searcher(spread)
    B, n, T = db.B, 3, cfg.tar_len
    kw = dict(temperature=1.5, top_p=0.95, seed=11, use_graphs=False)
    plain = search.sample_search(db, n, **kw)
    msgs = messages(plain[0], plain[1])
    own = lambda b, j: [w for w in msgs[b * n + j] if w > 3]         # a commit's own drawn words: positive probability for it
    prefix = [own(0, 0)[:2], [], own(2, 1)[:1], []]
    assert len(prefix[0]) == 2 and len(prefix[2]) == 1 and prefix[0][0] != prefix[0][1]
    words = [w for m in msgs for w in m if w > 3 and w not in prefix[0] + prefix[2]]
    banned = tuple(int(w) for w in np.argsort(-np.bincount(words))[:3])
    assert all(any(w in m for m in msgs) for w in banned)            # the ban takes something away
    con = Constraints(no_repeat_ngram=2, min_length=4, banned=banned)
    free = search.sample_search(db, n, constraints=con, merge_copies=True, **kw)
    forced = search.sample_search(db, n, constraints=con, merge_copies=True, prefix=prefix, **kw)
    for toks, lens, prob, logp in (free, forced):
        assert bool(torch.isfinite(logp).all())                      # no entry of probability 0 was ever taken
        for m in messages(toks, lens):
            assert not set(m) & set(banned)
            grams = list(zip(m, m[1:]))
            assert len(grams) == len(set(grams))
            assert EOS not in m[:4]
    for b in range(B):
        for j in range(n):
            m = messages(forced[0][b, j:j + 1], forced[1][b, j:j + 1])[0]
            assert m[:len(prefix[b])] == prefix[b], (b, j)
    for b in (1, 3):                                                 # an empty prefix: the commit's samples without any prefix
        assert torch.equal(forced[0][b], free[0][b]) and torch.equal(forced[1][b], free[1][b])
        assert torch.equal(bits(forced[3][b]), bits(free[3][b]))
    assert not torch.equal(forced[0][0], free[0][0])
    # logp: the float32 running sum of logf(best_p), recomputed from an eager replay of the step's library calls
    key = Searcher._key(("sample_search", B, n, 1.5, 0, C.c_float(0.95).value) + Searcher.CUTS_OFF, True, con, forced=True)
    st = search._ws[key]
    ws = search._begin(db, n)
    search._sample_reset(st)
    run64 = np.zeros(B * n)
    mag = np.zeros(B * n)
    for step in range(T - 1):
        alive = st["alive"].bool().cpu().numpy()
        if not alive.any():
            break
        search._sample_search_steps(st, ws, B, n, step, step + 1, 1.5, 0, C.c_float(0.95).value, Searcher.CUTS_OFF)
        bp = st["best_p"].double().cpu().numpy()
        picked = st["dist"][torch.arange(B * n), st["best_id"].long()]
        assert torch.equal(bits(picked), bits(st["best_p"]))         # best_p is the edited row's value
        term = np.log(np.where(alive, bp, 1.0))
        run64 += term
        mag += np.abs(term)
    assert torch.equal(st["out"].view(B, n, T).long(), forced[0]) and torch.equal(bits(st["logp"].view(B, n)), bits(forced[3]))
    # fp32: each of the <= T - 1 terms is logf (within 2 ulp of the term) and each addition rounds the partial sum, which is
    # at most `mag`: |error| <= (T - 1 + 2) * 2^-24 * mag
    err = np.abs(st["logp"].double().cpu().numpy() - run64)
    assert (err <= (T + 1) * 2.0 ** -24 * mag + 1e-30).all(), (err.max(), mag.max())
    seen = forced[2] > 1e-30                                         # (a product of ~29 probabilities may underflow fp32)
    assert torch.allclose(forced[3][seen].double(), torch.log(forced[2][seen].double()), rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ 7. exact reductions
def test_top_k_one_with_every_option_is_greedy_with_the_same_options(setup):
    from fira_icse_amd.decode import Constraints, Searcher
    cfg, store, ids, peaked, spread, db = setup
    search = Searcher(peaked)
    B, T = db.B, cfg.tar_len
    base = messages(*search.greedy(db, use_graphs=False)[:2])
    prefix = [[w for w in base[0] if w > 3][:2], [], [w for w in base[2] if w > 3][:1], []]
    assert prefix[0] and prefix[2]
    con = Constraints(no_repeat_ngram=2, min_length=3)
    opts = dict(constraints=con, merge_copies=True, prefix=prefix)
    out, length, prob = search.greedy(db, use_graphs=False, **opts)
    # every step's maximum of the EDITED row along the greedy path is unique
    st = search._ws[Searcher._key(("greedy", B), True, con, forced=True)]
    ws = search._begin(db, 1)
    search._greedy_reset(st)
    for step in range(int(length.max()) - 1):
        alive = st["alive"].bool()
        search._greedy_steps(st, ws, B, step, step + 1)
        top2 = torch.topk(st["dist"], 2, dim=1).values
        assert (top2[alive, 0] > top2[alive, 1]).all(), step
    for n in (1, 3):
        toks, lens, p_, logp = search.sample_search(db, n, top_k=1, temperature=1.3, seed=9, use_graphs=False, **opts)
        for j in range(n):
            assert torch.equal(toks[:, j], out) and torch.equal(lens[:, j], length)
            # the same factors, multiplied in one order or another: at most T - 1 roundings apart on either side
            assert torch.allclose(p_[:, j], prob, rtol=2 * (T - 1) * 2.0 ** -24, atol=0)


def test_an_ensemble_of_weights_one_zero_and_a_neighbour_of_lambda_zero_change_nothing(setup):
    from fira_icse_amd.decode import Neighbour, Searcher
    from fira_icse_amd.model import DeviceBatch, TransModel
    cfg, store, ids, peaked, spread, db = setup
    other = TransModel(cfg, init=False)
    other.load_state_dict(spread_state_dict(cfg, seed=3))
    other.eval()
    kw = dict(temperature=1.5, top_k=50, top_p=0.9, seed=21, use_graphs=False, merge_copies=True)
    single = Searcher(spread).sample_search(db, 3, **kw)
    assert same_samples(single, Searcher(spread, members=[other], weights=[1, 0]).sample_search(db, 3, **kw))
    mixed = Searcher(spread, members=[other], weights=[1, 1]).sample_search(db, 3, **kw)
    assert not torch.equal(mixed[0], single[0])                      # (the second member does take part when it has weight)
    nb_db = DeviceBatch(store.batch(list(ids[::-1])), cfg)
    search = Searcher(spread)
    assert same_samples(single, search.sample_search(db, 3, neighbour=Neighbour(nb_db, [0.7] * db.B, lam=0.0), **kw))
    near = search.sample_search(db, 3, neighbour=Neighbour(nb_db, [1.0] * db.B, lam=1024.0), **kw)
    assert not torch.equal(near[0], single[0])


# ------------------------------------------------------------------------------------------------ 8. the calls of a step
def test_calls_per_step_and_a_refused_call_makes_none(setup, monkeypatch):
    from fira_icse_amd.decode import Constraints, Neighbour, Searcher
    from fira_icse_amd.model import DeviceBatch
    cfg, store, ids, peaked, spread, db = setup
    B, n = db.B, 2
    con = Constraints(min_length=2)
    nb = Neighbour(DeviceBatch(store.batch(list(ids[::-1])), cfg), [0.5] * B)
    prefix = [[10], [], [], []]
    args = (1.0, 0, 1.0, Searcher.CUTS_OFF)
    base = ("sample_search", B, n, 1.0, 0, 1.0) + Searcher.CUTS_OFF
    draw = {"fira_sample_dist": 1, "fira_sample_advance": 1}
    edits = {"fira_merge_dist": 1, "fira_force_dist": 1, "fira_constrain_dist": 1}
    plain, pair = Searcher(spread), Searcher(spread, members=[peaked])

    def one_step(search, ws_key, key, **kw):
        search.sample_search(db, n, use_graphs=False, **kw)
        st, ws = search._ws[key], search._ws[ws_key]
        return count_calls(monkeypatch, lambda: search._sample_search_steps(st, ws, B, n, 0, 1, *args))

    assert one_step(plain, (B, n), base) == dict(draw, fira_decode_step_ex=1)
    assert one_step(plain, (B, n), Searcher._key(base, True, con, forced=True), constraints=con, merge_copies=True, prefix=prefix) == \
        dict(draw, fira_decode_step_ex=1, **edits)
    assert one_step(pair, ("members", B, n), base) == dict(draw, fira_decode_step_ex=2, fira_mix_dist=1)
    assert one_step(pair, ("members", B, n), Searcher._key(base, False, con), constraints=con) == \
        dict(draw, fira_decode_step_ex=2, fira_mix_dist=1, fira_constrain_dist=1)
    got = one_step(plain, ("neighbours", B, n), Searcher._key(base, True, None, neighbour=True), neighbour=nb, merge_copies=True)
    assert got == dict(draw, fira_decode_step_ex=2, fira_merge_dist=2, fira_mix_neighbour=1)   # (one merge of q, one of the edit chain)
    assert "fira_decode_step_sample" not in got
    fresh, ens = Searcher(spread), Searcher(spread, members=[peaked])

    def refused():
        for call, word in ((lambda: fresh.sample_search(db, 0), "n = 0"), (lambda: fresh.sample_search(db, 9), "n = 9"),
                           (lambda: fresh.sample_search(db, 2, temperature=0.0), "temperature"),
                           (lambda: fresh.sample_search(db, 2, typical_p=0.5, top_p=0.9), "typical_p .* top_p"),
                           (lambda: fresh.sample_search(db, 2, epsilon=1.0), "epsilon"),
                           (lambda: fresh.sample_search(db, 2, top_k=cfg.out_len + 1), "top_k"),
                           (lambda: fresh.sample_search(db, 2, constraints=Constraints(min_length=cfg.tar_len)), "min_length"),
                           (lambda: fresh.sample_search(db, 2, prefix=[[2], [], [], []]), "prefix: commit 0"),
                           (lambda: fresh.sample_search(db, 2, keys=[1, 2]), "keys: 2 values"),
                           (lambda: ens.sample_search(db, 2, neighbour=nb), "does not combine with an ensemble")):
            with pytest.raises(ValueError, match=word):
                call()
    assert count_calls(monkeypatch, refused) == {} and fresh._ws == {} and ens._ws == {}


# ------------------------------------------------------------------------------------------------ 9. argument errors
def test_library_argument_errors_launch_nothing_and_name_the_argument():
    V, L, S = GEOMETRIES[1]
    W, R = V + L + S, 6
    d = device_dims(V, L, S)
    dist = torch.full((R, W), 0.001, device="cuda")
    key = torch.arange(R, dtype=torch.int32, device="cuda")
    seed = seed_tensor(1)
    nan, inf = float("nan"), float("inf")
    cases = [("best_id and best_p", dict(null="both")), ("best_id and best_p", dict(null="id")), ("best_id and best_p", dict(null="p")),
             ("rows_per_commit = 4 .* divide R = 6", dict(rpc=4)), ("rows_per_commit = 0", dict(rpc=0)),
             ("rows_per_commit = 9 outside 1..8", dict(rpc=9, R=9)), ("R = -2", dict(R=-2, rpc=1)), ("step = -1", dict(step=-1)),
             ("top_k %d outside" % (W + 1), dict(top_k=W + 1)), ("top_k -1", dict(top_k=-1)),
             ("temperature", dict(temperature=0.0)), ("temperature", dict(temperature=inf)), ("temperature", dict(temperature=nan)),
             ("top_p", dict(top_p=0.0)), ("top_p", dict(top_p=1.5)), ("top_p", dict(top_p=nan)),
             ("min_p", dict(min_p=1.0)), ("min_p", dict(min_p=-0.1)), ("min_p", dict(min_p=nan)),
             ("epsilon", dict(epsilon=1.0)), ("epsilon", dict(epsilon=inf)), ("eta", dict(eta=1.5)), ("eta", dict(eta=nan)),
             ("typical_p", dict(typical_p=0.0)), ("typical_p", dict(typical_p=1.5)), ("typical_p", dict(typical_p=nan)),
             ("typical_p .* top_p", dict(typical_p=0.9, top_p=0.9)), ("typical_p .* min_p", dict(typical_p=0.9, min_p=0.1)),
             ("typical_p .* epsilon", dict(typical_p=0.9, epsilon=0.1)), ("typical_p .* eta", dict(typical_p=0.9, eta=0.1)),
             ("vocabulary 3 ", dict(dims=device_dims(3, L, S))), ("vocabulary 25601 ", dict(dims=device_dims(25601, L, S))),
             ("1025 memory slots", dict(dims=device_dims(V, 1000, 25))),
             ("null pointer", dict(null="dist")), ("null pointer", dict(null="key")), ("null pointer", dict(null="seed"))]
    for word, kw in cases:
        kw = dict(kw)
        null, dims, rows, rpc, step = kw.pop("null", None), kw.pop("dims", d), kw.pop("R", R), kw.pop("rpc", 2), kw.pop("step", 0)
        bid, bp = best_pair(R)
        rc = sample_dist(dims, rows, rpc, step, None if null == "dist" else dist, None if null == "key" else key,
                         None if null == "seed" else seed, None if null in ("both", "id") else bid,
                         None if null in ("both", "p") else bp, **kw)
        torch.cuda.synchronize()
        assert rc != 0, (word, kw)
        assert "fira_sample_dist: " in last_error() and re.search(word, last_error()), (word, last_error())
        assert bool((bid == -7).all()) and bool((bp == -7.0).all())
    bid, bp = best_pair(R)
    assert sample_dist(d, 0, 1, 0, None, None, None, bid, bp) == 0   # R == 0: a no-op
    assert sample_dist(d, R, 2, 0, dist, key, seed, bid, bp, typical_p=1.0, top_p=0.9, min_p=0.1, top_k=W) == 0, last_error()   # 1 = off
    torch.cuda.synchronize()
    assert int(bid.min()) >= 0 and int(bid.max()) < W and bool((bp == dist[0, 0]).all())
