"""Retrieval-augmented search on the device: fira_pool_memory, fira_nn_search and fira_mix_neighbour alone against the numpy
statements of retrieve_ref.py, then ``Searcher.greedy / greedy_many / beam(neighbour=...)`` against the host loops of the same
file, the properties that need no loop (lam = 0, min_sim > 1, the commit as its own neighbour), the option-off path, the
refusals, the pooled vectors against the oracle, and the command line with ``--retrieve``."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import util
import retrieve_ref as RR
import search_kit
from search_kit import bits, count_calls, device_dims, golden_search, last_error, run_cli, same_search
from fira_icse_amd import _lib, data, ops, synth
from fira_icse_amd.config import UNK, FiraConfig
from fira_icse_amd.decode import Constraints, Neighbour

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype)


# ------------------------------------------------------------------------------------------------ fira_pool_memory
NAN_BITS = (0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF)          # quiet and signalling NaN patterns, both signs


@pytest.mark.parametrize("B", [1, 3])
def test_pool_equals_the_float32_loop_bit_for_bit_and_invalid_rows_do_not_leak(B):
    """n_b in {0, 1, all} (B = 3: one commit each; B = 1: all, then 1, then 0 in turn).  The invalid rows hold NaN bit patterns.
    Against fp64, with eps = 2^-24 and k_c = (sum_s |mem[s, c]| / n) / |v| the condition of column c's signed sum:
      the mean        |dv_c| / |v| <= ((n - 1) k_c + 1) eps          (n - 1 additions and the division)
      the norm        |d|v|| / |v| <= ((n - 1) |k|_2 + 1 + 130) eps   (dv through the norm; 256 squares and 255 additions, halved
                                                                     by the root: (256 + 2) / 2 + 1 for the root itself)
      the quotient    one eps more, and |u_c| <= 1 multiplies the norm's share
    so |du_c| <= ((n - 1) (k_c + |k|_2) + 134) eps."""
    L, S_ = 5, 2
    S = L + S_
    d = device_dims(sou_len=L, sub_len=S_)
    rng = np.random.RandomState(11 + B)
    patterns = [np.array([1] * S), np.array([0, 0, 0, 1, 0, 0, 0]), np.array([0] * S)]
    for shift in range(3 if B == 1 else 1):
        valid = np.stack([patterns[(b + shift) % 3] for b in range(B)]).astype(np.int32)
        mem = rng.standard_normal((B, S, 256)).astype(F32)
        raw = mem.view(np.uint32)
        for b in range(B):
            for s in range(S):
                if not valid[b, s]:
                    raw[b, s, :] = NAN_BITS[(b + s) % 4]
        want = RR.pool(mem, valid)
        got = ops.pool_memory(d, dev(mem), dev(valid)).cpu()
        assert not torch.isnan(got).any()
        assert torch.equal(bits(got), bits(want)), (B, shift)
        u64 = RR.pool64(mem, valid)
        eps = 2.0 ** -24
        for b in range(B):
            n = int(valid[b].sum())
            if n == 0:
                assert not got[b].any()
                continue
            rows = mem[b][valid[b] != 0].astype(np.float64)
            v = rows.sum(0) / n
            cancel = np.abs(rows).sum(0) / n / np.linalg.norm(v)          # |terms| / |v|: the condition of the signed sum
            bound = ((n - 1) * (cancel + np.linalg.norm(cancel)) + 134) * eps
            err = np.abs(got[b].numpy().astype(np.float64) - u64[b])
            print("pool B=%d b=%d n=%d max err %.3g, bound at it %.3g" % (B, b, n, err.max(), bound[err.argmax()]))
            assert (err <= bound).all(), (b, err.max())


def test_pool_refusals():
    d = device_dims(sou_len=5, sub_len=2)
    lib, out = _lib.lib(), torch.full((2, 256), -3.0, device="cuda")
    mem, valid = torch.zeros((2, 7, 256), device="cuda"), torch.ones((2, 7), dtype=torch.int32, device="cuda")
    assert lib.fira_pool_memory(_lib.cur_stream(), C.byref(d), -1, _lib.ptr(mem), _lib.ptr(valid), _lib.ptr(out)) != 0
    assert "fira_pool_memory" in last_error()
    assert lib.fira_pool_memory(_lib.cur_stream(), C.byref(d), 2, None, _lib.ptr(valid), _lib.ptr(out)) != 0
    assert "null pointer" in last_error()
    assert lib.fira_pool_memory(_lib.cur_stream(), C.byref(d), 0, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())


# ------------------------------------------------------------------------------------------------ fira_nn_search
def make_search_case(N, B, seed):
    """A store of N unit rows and B queries, query b = a chosen store row plus small noise, renormalised."""
    rng = np.random.RandomState(seed)
    store = RR.unit_rows(rng, N)
    target = rng.randint(0, N, size=B)
    q = store[target].astype(np.float64) + 0.05 * rng.standard_normal((B, 256)) / 16.0
    Q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32)
    return store, Q, target


def check_search(store, Q, exclude=None):
    idx64, sim64, margin = RR.nn64(Q, store, exclude)
    assert (margin > RR.DOT_BOUND).all(), margin.min()               # every query: the fp32 arg-max is decided
    ex = None if exclude is None else dev(np.asarray(exclude, dtype=np.int32))
    gi, gs = ops.nn_search(dev(Q), dev(store), ex)
    gi, gs = gi.cpu().numpy(), gs.cpu().numpy().astype(np.float64)
    assert gi.tolist() == idx64.tolist()
    assert (np.abs(gs - sim64) <= RR.DOT_BOUND).all(), np.abs(gs - sim64).max()
    assert (gs >= 0).all() and (gs <= 1).all()
    return gi, gs


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("N", [2, 63, 64, 65, 257, 4099])
def test_search_finds_the_float64_arg_max(N, B):
    store, Q, target = make_search_case(N, B, 100 * N + B)
    gi, _ = check_search(store, Q)
    assert gi.tolist() == target.tolist()
    # exclude on the true winner returns the runner-up (commit 0 only; -1 elsewhere = nothing excluded)
    exclude = np.full(B, -1)
    exclude[0] = target[0]
    gi2, _ = check_search(store, Q, exclude)
    assert gi2[0] != target[0] and gi2[1:].tolist() == target[1:].tolist()


def test_search_past_the_grid_cap_where_a_wave_takes_several_tiles():
    """More than 256 workgroups x 4 waves of 16-row tiles: N = 16 401 is 1 026 tiles, so two waves run their loop twice and
    the last tile holds one row."""
    store, Q, target = make_search_case(16401, 3, 77)
    target[2] = 16400
    Q[2] = store[16400]
    gi, _ = check_search(store, Q)
    assert gi.tolist() == target.tolist()


@pytest.mark.parametrize("B", [1, 3, 64])
def test_search_over_one_row(B):
    """N = 1: one candidate, margin infinite; the product is clamped to [0, 1] (a query opposite to the row: 0)."""
    store, Q, _ = make_search_case(1, B, 7)
    if B > 1:
        Q[1] = -Q[1]
    check_search(store, Q)


def test_duplicate_rows_in_different_chunks_tie_exactly_and_the_lowest_index_wins():
    """Identical rows at 5, 700 (another workgroup's tile) and 4098 (the last, partial tile): every query whose best row is
    the duplicated one must report index 5 -- the products are the same fma chain wherever the row sits."""
    N, B = 4099, 3
    store, Q, target = make_search_case(N, B, 3)
    assert not {5, 700, 4098} & set(target[1:].tolist()) and 5 != target[0]
    for j in (5, 700, 4098):
        store[j] = store[target[0]]
    first = min(5, int(target[0]))
    gi, gs = ops.nn_search(dev(Q), dev(store))
    assert gi.cpu().tolist() == [first] + target[1:].tolist()
    # excluding the first copy gives the next one, with the same similarity bits
    ex = np.full(B, -1, dtype=np.int32)
    ex[0] = first
    gi2, gs2 = ops.nn_search(dev(Q), dev(store), dev(ex))
    assert int(gi2[0]) == sorted({5, 700, 4098, int(target[0])} - {first})[0]
    assert torch.equal(bits(gs2.cpu()), bits(gs.cpu()))


def test_a_nan_row_never_wins_and_an_all_nan_store_reports_minus_one():
    store, Q, target = make_search_case(65, 3, 9)
    victim = (int(target[0]) + 1) % 65
    store[victim] = np.float32("nan")
    assert victim not in target.tolist()
    gi, _ = check_search(store, Q)
    assert gi.tolist() == target.tolist()
    store[:] = np.float32("nan")
    gi, gs = ops.nn_search(dev(Q), dev(store))
    assert gi.cpu().tolist() == [-1, -1, -1] and gs.cpu().tolist() == [0.0, 0.0, 0.0]


def test_search_refusals_return_non_zero_with_a_message_and_launch_nothing():
    lib = _lib.lib()
    store, Q = torch.zeros((4, 256), device="cuda"), torch.zeros((65, 256), device="cuda")
    idx = torch.full((65,), -7, dtype=torch.int32, device="cuda")
    sim = torch.full((65,), -7.0, device="cuda")
    ex = torch.zeros(65, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    p = _lib.ptr

    def call(Q_=Q, B=3, store_=store, N=4, ex_=None, idx_=idx, sim_=sim, scratch_=scratch, nbytes=1 << 20):
        return lib.fira_nn_search(_lib.cur_stream(), p(Q_), B, p(store_), N, p(ex_), p(idx_), p(sim_), p(scratch_), nbytes)
    for kwargs, word in ((dict(N=0), "the store is empty"), (dict(B=65), "more than 64"), (dict(B=0), "at least one"),
                         (dict(B=-2), "at least one"), (dict(N=1, ex_=ex), "leaves no row"), (dict(Q_=None), "null pointer"),
                         (dict(store_=None), "null pointer"), (dict(idx_=None), "null pointer"), (dict(sim_=None), "null pointer"),
                         (dict(scratch_=None), "null pointer"), (dict(nbytes=8), "scratch of 8 bytes")):
        assert call(**kwargs) != 0, kwargs
        assert "fira_nn_search" in last_error() and word in last_error(), (kwargs, last_error())
    assert lib.fira_nn_search_scratch_bytes(0, 5) == 0 and lib.fira_nn_search_scratch_bytes(65, 5) == 0
    assert lib.fira_nn_search_scratch_bytes(3, 0) == 0 and 0 < lib.fira_nn_search_scratch_bytes(64, 75000) <= 1 << 20
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((sim == -7.0).all()) and not bool(scratch.any())
    assert call() == 0


def test_a_captured_search_replays_the_same_bits():
    store, Q, target = make_search_case(4099, 64, 21)
    dQ, dS = dev(Q), dev(store)
    lib = _lib.lib()
    scratch = torch.zeros(lib.fira_nn_search_scratch_bytes(64, 4099), dtype=torch.uint8, device="cuda")
    idx, sim = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(64, device="cuda")

    def launch():
        _lib.check(lib.fira_nn_search(_lib.cur_stream(), _lib.ptr(dQ), 64, _lib.ptr(dS), 4099, None, _lib.ptr(idx), _lib.ptr(sim),
                                      _lib.ptr(scratch), scratch.numel()), "fira_nn_search")
    launch()
    torch.cuda.synchronize()
    want_i, want_s = idx.clone(), sim.clone()
    assert want_i.cpu().tolist() == target.tolist()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for _ in range(2):
        idx.fill_(-7)
        sim.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(idx, want_i) and torch.equal(bits(sim), bits(want_s))


# ------------------------------------------------------------------------------------------------ fira_mix_neighbour
# W = 24 (V = 19 with 5 slots), W = 19 (odd: rows at every 4-byte alignment), W = 45 (geometry_ref's "min": odd, no
# sub-token slots), and the model's own row
MIX_GEOS = {"V19-5slots": dict(vocab=19, sou_len=3, sub_len=2), "W19": dict(vocab=11, sou_len=5, sub_len=3),
            "min-W45": dict(vocab=40, sou_len=5, sub_len=0), "model": {}}
SENTINEL = -3.0


offset_rows = functools.partial(search_kit.offset_rows, fill=SENTINEL)             # this file's guard words hold a sentinel, not 0
outside_untouched = functools.partial(search_kit.outside_untouched, fill=SENTINEL)


def make_mix_case(geo, B, rpc, seed):
    d = device_dims(**geo)
    V, W = d.vocab, d.vocab + d.sou_len + d.sub_len
    rng = np.random.RandomState(seed)
    R = B * rpc
    p = rng.uniform(1e-6, 1.0, size=(R, W)).astype(F32)
    q = rng.uniform(1e-6, 1.0, size=(R, W)).astype(F32)
    q[:, V:] = np.float32("nan")                                     # never read: a NaN here would show
    for r in range(R):
        p[r, rng.randint(0, W, size=3)] = 0.0
    p[0, 1] = p[0, V - 2] = 2.0                                      # a tie between two words with equal q: the lower index wins
    q[0, 1] = q[0, V - 2] = 0.5
    if R > 1:
        p[1, W - 1] = 3.0                                            # a copy entry as the row's maximum
    cf = RR.coef(rng.uniform(0.05, 1.0, size=B), 1.5)
    return d, V, W, p, q, cf


@pytest.mark.parametrize("rpc", [1, 3])
@pytest.mark.parametrize("geo", sorted(MIX_GEOS))
def test_mix_equals_the_float32_loop_bit_for_bit(geo, rpc):
    d, V, W, p, q, cf = make_mix_case(MIX_GEOS[geo], 2, rpc, 5 + rpc)
    want = RR.mix(p, q, cf, V, rpc)
    want_id, want_p = RR.best_of(want)
    R = p.shape[0]
    for p_off, q_off, best in ((0, 0, True), (1, 1, True), (1, 2, True), (3, 0, True), (2, 1, False)):   # 4 bytes apart and more
        pbuf, pv = offset_rows(p, p_off)
        qbuf, qv = offset_rows(q, q_off)
        bid = torch.full((R,), -7, dtype=torch.int32, device="cuda") if best else None
        bp = torch.full((R,), -7.0, device="cuda") if best else None
        _lib.check(_lib.lib().fira_mix_neighbour(_lib.cur_stream(), C.byref(d), R, rpc, _lib.ptr(dev(cf)), _lib.ptr(qv), _lib.ptr(pv),
                                                 _lib.ptr(bid), _lib.ptr(bp)), "fira_mix_neighbour")
        torch.cuda.synchronize()
        assert torch.equal(bits(pv.cpu()), bits(want)), (geo, rpc, p_off, q_off)
        assert outside_untouched(pbuf, p_off, p.size) and outside_untouched(qbuf, q_off, q.size)
        assert torch.equal(bits(qv.cpu()), bits(q))                  # the neighbour's row is read only
        if best:
            assert bid.cpu().tolist() == want_id.tolist() and torch.equal(bits(bp.cpu()), bits(want_p))
            assert int(bid[0]) == 1                                  # the tie trap
    # (1, 0) leaves every bit of dist (q's words finite)
    one = np.tile(np.array([[1.0, 0.0]], dtype=F32), (2, 1))
    got = ops.mix_neighbour(d, rpc, dev(one), dev(np.nan_to_num(q, nan=0.5)), dev(p)).cpu()
    assert torch.equal(bits(got), bits(p))


def test_mix_nan_never_wins_and_an_all_nan_row_reports_index_0():
    d, V, W, p, q, cf = make_mix_case(MIX_GEOS["W19"], 3, 1, 2)
    p[0, 3] = np.float32("nan")
    q[1, 4] = np.float32("nan")
    p[2, :] = np.float32("nan")
    want = RR.mix(p, q, cf, V)
    assert np.isnan(want[0, 3]) and np.isnan(want[1, 4]) and np.isnan(want[2]).all()
    dist = dev(p)
    bid, bp = ops.mix_neighbour(d, 1, dev(cf), dev(q), dist, best=True)
    assert torch.equal(torch.isnan(dist.cpu()), torch.from_numpy(np.isnan(want)))
    assert bid.cpu().tolist() == [1, int(np.nanargmax(want[1])), 0]
    assert float(bp[0]) == float(np.nanmax(want[0])) and float(bp[1]) == float(np.nanmax(want[1])) and float(bp[2]) == float("-inf")


def test_mix_refusals_return_non_zero_with_a_message_and_launch_nothing():
    d, V, W, p, q, cf = make_mix_case(MIX_GEOS["W19"], 2, 1, 2)
    lib, dist, dq, dcf = _lib.lib(), dev(p), dev(np.nan_to_num(q)), dev(cf)
    bid = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    s, pp = _lib.cur_stream(), _lib.ptr
    both = torch.cat([dist.view(-1), dist.view(-1)])                 # an aliased q: it overlaps dist by one row
    alias_dist, alias_q = both[:2 * W].view(2, W), both[W:3 * W].view(2, W)
    for args, word in (((C.byref(d), 2, 1, pp(dcf), pp(alias_q), pp(alias_dist), None, None), "q overlaps dist"),
                       ((C.byref(d), 2, 1, pp(dcf), pp(dist), pp(dist), None, None), "q overlaps dist"),
                       ((C.byref(d), 2, 1, None, pp(dq), pp(dist), None, None), "null pointer"),
                       ((C.byref(d), 2, 1, pp(dcf), None, pp(dist), None, None), "null pointer"),
                       ((C.byref(d), 2, 1, pp(dcf), pp(dq), pp(dist), pp(bid), None), "given together"),
                       ((C.byref(d), 3, 2, pp(dcf), pp(dq), pp(dist), None, None), "rows_per_commit"),
                       ((None, 2, 1, pp(dcf), pp(dq), pp(dist), None, None), "null dims")):
        assert lib.fira_mix_neighbour(s, *args) != 0, word
        assert "fira_mix_neighbour" in last_error() and word in last_error(), last_error()
    torch.cuda.synchronize()
    assert torch.equal(bits(dist.cpu()), bits(p)) and bool((bid == -7).all())
    assert lib.fira_mix_neighbour(s, C.byref(d), 0, 1, None, None, None, None, None) == 0


# ------------------------------------------------------------------------------------------------ through the model
# Untrained weights at tar_len = 8 (tests/test_require_gpu.py has the arithmetic): every entry of a row is positive and no fp32
# product of seven step probabilities underflows, so no comparison below rests on zeros that tie by index.
MODEL_TAR_LEN = 8
SIM = (1.0, 0.5, 0.0625, 0.8)
LAM = 2.0
CON = Constraints(2, 3, (UNK,))


@pytest.fixture(scope="module")
def setup():
    from fira_icse_amd.model import DeviceBatch
    g = golden_search(tar_len=MODEL_TAR_LEN, searchers=3)
    cfg, db = g.cfg, g.db
    nb_db = DeviceBatch(g.store.batch(g.idx["train"][:util.GOLDEN_B]), cfg)
    assert db.B == len(SIM)
    search, own, other = g.searchers
    return dict(cfg=cfg, sd=g.state_dict, model=g.model, hb=g.host_batch, db=db, nb_db=nb_db, search=search, own=own, other=other,
                nb=Neighbour(nb_db, SIM, lam=LAM), cf=RR.coef(SIM, LAM), dims=RR.dims_of(cfg),
                sou=db.sou.cpu().numpy(), sub=db.sub_token.cpu().numpy())


def edit_of(s, rows_per_commit, merge, con):
    import ensemble_ref as E
    return E.make_edit(s["sou"], s["sub"], s["dims"], rows_per_commit, merge, con)


@pytest.fixture(scope="module")
def refs(setup):
    """The reference loops, each run once on first use and then shared, never modified."""
    cache = {}

    def get(kind, merge=False, con=None):
        key = (kind, merge, con)
        if key not in cache:
            s = setup
            if kind == "greedy":
                cache[key] = RR.greedy_neighbour(s["own"], s["other"], s["db"], s["nb_db"], s["cf"], edit_of(s, 1, merge, con))
            else:
                cache[key] = RR.beam_neighbour(s["own"], s["other"], s["db"], s["nb_db"], s["cf"], kind, edit_of(s, kind, merge, con))
        return cache[key]
    return get


def test_pooled_vectors_against_the_oracle(setup):
    """The oracle's encoder memory, pooled in fp64, against ``retrieve.pooled_vectors``.  tests/test_model_gpu.py holds the
    engine's memory to the oracle's within 2e-4 per element; a mean of rows keeps that bound per element, so |dv| <= 2e-4 * 16
    in the Euclidean norm over 256 columns, and u = v / |v| moves by at most 2 |dv| / |v| (the vector and its norm both move)."""
    from fira_icse_amd import retrieve
    from oracle import fira_oracle as O
    cfg, hb, sd = setup["cfg"], setup["hb"], setup["sd"]
    tb = util.to_torch_batch(hb, cfg)
    with torch.no_grad():
        memory, mem_mask = O.encode_memory(sd, cfg, tb["sou"], tb["mark"], tb["ast_change"], tb["edge"], tb["sub_token"])
    got = retrieve.pooled_vectors(setup["search"], setup["db"]).cpu().numpy().astype(np.float64)
    mem64, valid = memory.double().numpy(), mem_mask.numpy()
    want = RR.pool64(mem64, valid)
    for b in range(hb.sou.shape[0]):
        v = mem64[b][valid[b] != 0].mean(0)
        tol = 2 * 2e-4 * 16 / np.linalg.norm(v)
        err = np.abs(got[b] - want[b]).max()
        print("commit %d: |v| = %.4g, max |du| = %.3g, tolerance %.3g" % (b, np.linalg.norm(v), err, tol))
        assert err <= tol and abs(np.linalg.norm(got[b]) - 1.0) < 1e-5


@pytest.mark.parametrize("merge, con", [(False, None), (True, CON)], ids=["plain", "merge-constraints"])
def test_beam_equals_the_reference_loop(setup, refs, merge, con):
    want = refs(3, merge, con)
    for use_graphs in (False, True, True):                    # eager, captured, replayed
        same_search(setup["search"].beam(setup["db"], 3, use_graphs=use_graphs, constraints=con, merge_copies=merge,
                                         neighbour=setup["nb"]), want)


@pytest.mark.parametrize("merge, con", [(False, None), (True, CON)], ids=["plain", "merge-constraints"])
def test_greedy_and_greedy_many_equal_the_reference_loop(setup, refs, merge, con):
    db, search, nb = setup["db"], setup["search"], setup["nb"]
    want = refs("greedy", merge, con)
    for use_graphs in (False, True, True):
        same_search(search.greedy(db, use_graphs=use_graphs, constraints=con, merge_copies=merge, neighbour=nb), want)
    many = search.greedy_many([db, db, db], in_flight=3, constraints=con, merge_copies=merge, neighbour=[nb, nb, nb])
    torch.cuda.synchronize()
    assert len(many) == 3
    for got in many:
        same_search(got, want)


def test_lambda_zero_and_min_sim_above_one_are_the_plain_search_bit_for_bit(setup):
    db, search, nb_db = setup["db"], setup["search"], setup["nb_db"]
    for nb in (Neighbour(nb_db, SIM, lam=0.0), Neighbour(nb_db, SIM, lam=LAM, min_sim=1.5)):
        for use_graphs in (False, True):
            for got, want in ((search.greedy(db, use_graphs=use_graphs, neighbour=nb), search.greedy(db, use_graphs=use_graphs)),
                              (search.beam(db, 3, use_graphs=use_graphs, neighbour=nb), search.beam(db, 3, use_graphs=use_graphs))):
                assert len(got) == len(want) == 3 and all(torch.equal(x, y) for x, y in zip(got, want))


def test_the_commit_as_its_own_neighbour_is_the_merged_search(setup):
    """neighbour = the batch itself, merge_copies=True: q is the merged p, so every word's mass is (a p_w + b (p_w + slots)) +
    a slots' mass folded by the input's merge -- the plain merged value up to rounding (all terms >= 0: no cancellation).
    Counted per entry and step, eps = 2^-24: the mix rounds three times (two products, one sum), a + b = 1 holds within one
    eps, and each of the two merges adds at most L + S terms in another association: (4 + 2 (L + S)) eps; the product over
    the T - 1 steps adds one eps per factor: (T - 1) (5 + 2 (L + S)) eps in all."""
    cfg, db, search = setup["cfg"], setup["db"], setup["search"]
    nb = Neighbour(db, [1.0] * db.B, lam=1.0)
    tol = (cfg.tar_len - 1) * (5 + 2 * (cfg.sou_len + cfg.sub_token_len)) * 2.0 ** -24
    for got, want in ((search.greedy(db, merge_copies=True, neighbour=nb), search.greedy(db, merge_copies=True)),
                      (search.beam(db, 3, merge_copies=True, neighbour=nb), search.beam(db, 3, merge_copies=True))):
        (gen, length, p), (gen_t, len_t, p_t) = [tuple(t.cpu() for t in x) for x in (got, want)]
        rel = ((p - p_t).abs() / p_t.abs().clamp(min=1e-38)).max()
        print("own neighbour: max relative difference of the probabilities %.3g, tolerance %.3g" % (float(rel), tol))
        assert torch.equal(length, len_t)
        live = torch.arange(gen.shape[-1])[(None,) * (gen.dim() - 1)] < length[..., None]
        assert torch.equal(gen * live, gen_t * live)
        assert float(rel) <= tol


def test_a_different_neighbour_with_a_large_lambda_changes_a_message(setup):
    """Built for it: peaked weights (every commit's rows have a clear, commit-specific arg-max), the neighbour of commit b is
    another commit, sim = 1 and lam = 1024: the row is the neighbour's up to 1 / 1025."""
    from fira_icse_amd.model import TransModel, reference_init_state_dict
    from fira_icse_amd.decode import Searcher
    cfg, db, nb_db = setup["cfg"], setup["db"], setup["nb_db"]
    torch.manual_seed(0)
    model = TransModel(cfg, init=False)
    model.load_state_dict(util.peaked_state_dict(reference_init_state_dict(cfg), seed=2))
    model.eval()
    search = Searcher(model)
    nb = Neighbour(nb_db, [1.0] * db.B, lam=1024.0)
    changed = 0
    for kind in ("greedy", "beam"):
        run = (lambda **kw: search.greedy(db, merge_copies=True, **kw)) if kind == "greedy" else \
            (lambda **kw: search.beam(db, 3, merge_copies=True, **kw))
        plain, mixed = search.best(*run()), search.best(*run(neighbour=nb))
        diff = [b for b in range(db.B) if plain[b] != mixed[b]]
        print("%s: commits whose message changes under the neighbour: %s" % (kind, diff))
        changed += len(diff)
    assert changed >= 1


def test_option_off_is_todays_search_and_on_adds_one_step_one_merge_one_mix(setup, monkeypatch):
    from fira_icse_amd.decode import Searcher
    cfg, db, model, nb = setup["cfg"], setup["db"], setup["model"], setup["nb"]
    B = db.B
    fresh = Searcher(model)
    fresh.beam(db, 3, neighbour=None)
    fresh.greedy(db, neighbour=None)
    assert set(fresh._ws) == {(B, 3), (B, 1), ("beam", B, 3), ("greedy", B)}
    assert set(fresh._ws[("greedy", B)]) == {"out", "length", "prob", "alive", "tok", "n_alive", "best_id", "best_p", "con", "sou",
                                             "sub", "graphs", "chunk", "bounds"}
    assert set(fresh._ws[("beam", B, 3)]) == {"gen", "length", "prob", "tok", "parent", "fin", "active", "done", "dist", "con",
                                              "sou", "sub", "graphs", "chunk", "bounds"}
    g, b = fresh._ws[("greedy", B)], fresh._ws[("beam", B, 3)]
    assert count_calls(monkeypatch, lambda: fresh._greedy_steps(g, fresh._ws[(B, 1)], B, 0, 1)) == \
        {"fira_decode_step_ex": 1, "fira_greedy_advance": 1}
    assert count_calls(monkeypatch, lambda: fresh._beam_steps(b, fresh._ws[(B, 3)], B, 3, 0, 1)) == \
        {"fira_beam_prepare": 1, "fira_decode_step_ex": 1, "fira_beam_select": 1}
    assert count_calls(monkeypatch, lambda: fresh._begin(db, 3)) == {"fira_decode_begin_ex": 1}
    # with a neighbour: new keys beside today's, which keep their contents
    fresh.beam(db, 3, neighbour=nb)
    fresh.greedy(db, neighbour=nb)
    new = {("neighbours", B, 3), ("neighbour", B, 3), ("neighbours", B, 1), ("neighbour", B, 1), ("beam", B, 3, "neighbour"),
           ("greedy", B, "neighbour")}
    assert set(fresh._ws) == {(B, 3), (B, 1), ("beam", B, 3), ("greedy", B)} | new
    assert set(fresh._ws[("greedy", B, "neighbour")]) == set(g) | {"dist", "mix_best"}
    assert set(fresh._ws[("beam", B, 3, "neighbour")]) == set(b)
    nw = fresh._ws[("neighbours", B, 3)]
    assert nw.q.shape == (B * 3, cfg.out_len) and nw.coef.shape == (B, 2)
    assert np.array_equal(nw.coef.cpu().numpy(), setup["cf"])
    assert count_calls(monkeypatch, lambda: fresh._greedy_steps(fresh._ws[("greedy", B, "neighbour")], fresh._ws[("neighbours", B, 1)],
                                                                B, 0, 1)) == \
        {"fira_decode_step_ex": 2, "fira_merge_dist": 1, "fira_mix_neighbour": 1, "fira_greedy_advance": 1}
    assert count_calls(monkeypatch, lambda: fresh._beam_steps(fresh._ws[("beam", B, 3, "neighbour")], nw, B, 3, 0, 1)) == \
        {"fira_beam_prepare": 1, "fira_decode_step_ex": 2, "fira_merge_dist": 1, "fira_mix_neighbour": 1, "fira_beam_select": 1}
    assert count_calls(monkeypatch, lambda: fresh._begin(db, 3, nb)) == {"fira_decode_begin_ex": 2}


def test_refusals_launch_nothing(setup, monkeypatch):
    from fira_icse_amd.decode import Searcher
    db, model, nb, nb_db = setup["db"], setup["model"], setup["nb"], setup["nb_db"]
    search, ens = Searcher(model), Searcher(model, members=(model,))
    cand = torch.tensor([[2, 5, 1]] * db.B)
    small = Neighbour(types_batch(nb_db, 2), [0.5, 0.5])

    def run():
        for call, word in ((lambda: search.sample(db, 2, neighbour=nb), "sample does not combine with a neighbour"),
                           (lambda: search.sample_distinct(db, 2, neighbour=nb), "sample_distinct does not combine"),
                           (lambda: search.score(db, cand, neighbour=nb), "score does not combine with a neighbour"),
                           (lambda: ens.greedy(db, neighbour=nb), "does not combine with an ensemble"),
                           (lambda: ens.beam(db, 3, neighbour=nb), "does not combine with an ensemble"),
                           (lambda: search.greedy(db, neighbour=(nb_db, SIM)), "expected decode.Neighbour"),
                           (lambda: search.beam(db, 3, neighbour=small), "a neighbour batch of 2 commits for a batch of 4"),
                           (lambda: search.greedy_many([db, db], neighbour=[nb]), "1 values for 2 batches"),
                           (lambda: search.greedy_many([db, db], neighbour=[nb, small]), "a neighbour batch of 2")):
            with pytest.raises(ValueError, match=word):
                call()
    assert count_calls(monkeypatch, run) == {} and search._ws == {} and ens._ws == {}


def types_batch(db, B):
    """A stand-in with another batch size (the check reads nothing else before it refuses)."""
    import types
    return types.SimpleNamespace(B=B, struct=db.struct)


# ------------------------------------------------------------------------------------------------ command line
BASE = ["test", "--splits", "16,4,4", "--test-batch-size", "4"]


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """The golden synthetic data set (24 commits: 16 train, 4 valid, 4 test) with a peaked checkpoint, and the Python API's
    view of it: the model, the test batch, the train store's batches."""
    from fira_icse_amd.model import TransModel, DeviceBatch, reference_init_state_dict
    root = str(tmp_path_factory.mktemp("retrieve_cli"))
    cfg = FiraConfig()
    raw = util.load_golden_raw()
    synth.write_dataset(root, raw)
    torch.manual_seed(0)
    sd = util.peaked_state_dict(reference_init_state_dict(cfg), seed=2)
    torch.save(sd, os.path.join(root, "best_model.pt"))
    model = TransModel(cfg, init=False)
    model.load_state_dict(sd)
    model.eval()
    full = data.process_raw(cfg, raw)
    idx = data.split_index(*util.GOLDEN_SPLIT, seed=0)
    return dict(root=root, cfg=cfg, raw=raw, model=model, full=full, idx=idx,
                batch=lambda ids: DeviceBatch(full.batch(ids), cfg))


def test_cli_retrieve_writes_what_the_python_api_gives_and_the_second_run_loads_the_store(cli):
    from fira_icse_amd import retrieve, text
    from fira_icse_amd.decode import Searcher
    root, model, idx, raw = cli["root"], cli["model"], cli["idx"], cli["raw"]
    search = Searcher(model)
    train, test = idx["train"], idx["test"]
    ds = retrieve.Datastore.build(model, [(list(range(len(train))), cli["batch"](train))], searcher=search)
    db = cli["batch"](test)
    nn, sim = ds.query(search, db)
    nb = Neighbour(cli["batch"]([train[i] for i in nn.tolist()]), sim, lam=4.0)
    r_vocab = {v: k for k, v in raw["word_vocab"].items()}
    out_f, nb_f = os.path.join(root, "OUTPUT", "output_fira"), os.path.join(root, "OUTPUT", "output_fira_neighbours")
    store_f = os.path.join(root, "OUTPUT", "retrieve_store.pt")
    for n_run, beam in enumerate((3, 1)):
        out = run_cli(BASE + ["--retrieve", "--retrieve-lambda", "4", "--beam", str(beam)], root).stdout
        assert ("retrieve: built 16 vectors" in out) == (n_run == 0) and ("retrieve: loaded 16 vectors" in out) == (n_run == 1)
        assert os.path.isfile(store_f)
        test_index = json.load(open(os.path.join(root, "all_index")))["test"]
        train_index = json.load(open(os.path.join(root, "all_index")))["train"]
        var_maps = json.load(open(os.path.join(root, "DataSet", "variable.json")))
        hyps = search.best(*(search.beam(db, 3, neighbour=nb) if beam == 3 else search.greedy(db, neighbour=nb)))
        want = [text.detokenize(h, r_vocab, var_maps[test_index[i]]) for i, h in enumerate(hyps)]
        lines = open(out_f).read().split("\n")
        assert lines[-1] == "" and lines[:-1] == want, beam
        recs = [json.loads(l) for l in open(nb_f).read().split("\n")[:-1]]
        assert [r["train_index"] for r in recs] == nn.tolist()
        assert [np.float32(r["sim"]) for r in recs] == [np.float32(x) for x in sim.tolist()]
        assert [r["message"] for r in recs] == [text.detokenize(cli["full"].tar[train[i]], r_vocab, var_maps[train_index[i]])
                                                for i in nn.tolist()]
    # --retrieve-only: the neighbours' messages, without decoding
    run_cli(BASE + ["--retrieve", "--retrieve-only"], root)
    assert open(out_f).read().split("\n")[:-1] == [r["message"] for r in recs]


def test_cli_lambda_zero_is_byte_identical_to_no_option(cli):
    root = cli["root"]
    out_f = os.path.join(root, "OUTPUT", "output_fira")
    run_cli(BASE, root)
    plain = open(out_f, "rb").read()
    os.remove(out_f)
    run_cli(BASE + ["--retrieve", "--retrieve-lambda", "0"], root)
    assert open(out_f, "rb").read() == plain and len(plain.split(b"\n")) == 5
