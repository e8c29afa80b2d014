"""The truncation cuts of the on-device sampler (fira_decode_step_sample_cut / Searcher.sample(min_p=, epsilon=, eta=,
typical_p=) / run_model.py test --sample N --epsilon-cutoff ...): the draws lie in and follow the kept set of the numpy twin
(cut_ref.py), degenerate rows, cuts off = the plain sampler bit for bit, the step loop, argument errors, the command line.

Relaxation of the twin's boundary: rel = 1e-4, the amount test_sample_gpu.py uses for top-p.  It also covers the entropy:
H is one fixed-order fp32 block sum of at most 26 terms per thread, 6 shuffle levels and 16 wave partials, so its rounding
error is below 48 * 2^-24 = 2.9e-6 of sum |w ln w| / Z <= H + ln Z < 21, i.e. below 6e-5 absolute, and it enters the eta
threshold as exp(-H) (relative error = that absolute error < rel) and the typical band as an absolute shift that the twin's
band edge allows for with rel * (|ln q_i| + H) >= 1e-4 * H."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import cut_ref
import sample_ref
import util
from search_kit import golden_search, run_cli, seed_tensor, spread_state_dict
from fira_icse_amd import _lib, synth

pytestmark = pytest.mark.gpu

REL = 1e-4
OFF = dict(min_p=0.0, epsilon=0.0, eta=0.0, typical_p=1.0)


@pytest.fixture(scope="module")
def setup():
    from fira_icse_amd.model import TransModel
    g = golden_search(weights="peaked", searchers=0, seed=2)
    cfg = g.cfg
    spread = TransModel(cfg, init=False)
    spread.load_state_dict(spread_state_dict(cfg))
    spread.eval()
    sd = spread_state_dict(cfg)
    sd["copy_net.LinearProb.bias"][1] += 6.0                     # the gate leans to the copy part: rows whose maximum is a copy entry
    copyish = TransModel(cfg, init=False)
    copyish.load_state_dict(sd)
    copyish.eval()
    return cfg, g.store, g.ids, g.model, spread, copyish, g.db


def step_sample(search, ws, B, n, step, tok, key, seed, T, k, p, dist, best_id, best_p, flags=0):
    m = search.model
    _lib.check(_lib.lib().fira_decode_step_sample(_lib.cur_stream(), C.byref(m.dims), _lib.ptr(m.flat.data), _lib.ptr(ws),
                                                  ws.numel(), B, n, step, _lib.ptr(tok), _lib.ptr(key), _lib.ptr(seed),
                                                  float(T), int(k), float(p), _lib.ptr(dist), _lib.ptr(best_id),
                                                  _lib.ptr(best_p), flags), "fira_decode_step_sample")


def step_cut(search, ws, B, n, step, tok, key, seed, dist, best_id, best_p, flags=0, temperature=1.0, top_k=0, top_p=1.0,
             min_p=0.0, epsilon=0.0, eta=0.0, typical_p=1.0):
    m = search.model
    _lib.check(_lib.lib().fira_decode_step_sample_cut(_lib.cur_stream(), C.byref(m.dims), _lib.ptr(m.flat.data), _lib.ptr(ws),
                                                      ws.numel(), B, n, step, _lib.ptr(tok), _lib.ptr(key), _lib.ptr(seed),
                                                      float(temperature), int(top_k), float(top_p), float(min_p),
                                                      float(epsilon), float(eta), float(typical_p), _lib.ptr(dist),
                                                      _lib.ptr(best_id), _lib.ptr(best_p), flags),
               "fira_decode_step_sample_cut")


# ------------------------------------------------------------------------------------------------ step level
@pytest.fixture(scope="module")
def row64(setup):
    """One commit in 64 rows x 8 samples with distinct keys: 8 seeds give 4 096 draws from one step-0 distribution."""
    from fira_icse_amd.model import DeviceBatch
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, copyish, db = setup
    search = Searcher(spread)
    B, n, W = 64, 8, cfg.out_len
    ws = search._begin(DeviceBatch(store.batch([ids[0]] * B), cfg), n)
    bufs = dict(tok=torch.full((B * n,), 2, dtype=torch.int32, device="cuda"),
                key=torch.arange(B, dtype=torch.int32, device="cuda"), dist=torch.empty(B * n, W, device="cuda"),
                bid=torch.empty(B * n, dtype=torch.int32, device="cuda"), bp=torch.empty(B * n, device="cuda"))
    return search, ws, B, n, W, bufs


def draw_4096(row64, **kw):
    search, ws, B, n, W, b = row64
    draws = []
    for s in range(8):
        step_cut(search, ws, B, n, 0, b["tok"], b["key"], seed_tensor(2000 + s), b["dist"], b["bid"], b["bp"], **kw)
        torch.cuda.synchronize()
        assert torch.equal(b["dist"].view(torch.int32), b["dist"][:1].expand_as(b["dist"]).view(torch.int32))
        ids_ = b["bid"].long()
        assert int(ids_.min()) >= 0 and int(ids_.max()) < W and float(b["bp"].min()) > 0
        assert torch.equal(b["bp"].view(torch.int32), b["dist"][torch.arange(B * n), ids_].contiguous().view(torch.int32))
        draws.append(ids_.cpu().numpy())
    return np.concatenate(draws), b["dist"][0].double().cpu().numpy()


STEP_SETTINGS = [dict(min_p=0.02), dict(min_p=0.3), dict(epsilon=0.0005), dict(epsilon=0.02), dict(eta=0.0003), dict(eta=0.05),
                 dict(typical_p=0.3), dict(typical_p=0.9), dict(top_k=50, epsilon=0.005),
                 dict(top_p=0.9, min_p=0.02, eta=0.003, temperature=1.3), dict(top_k=50, typical_p=0.7, temperature=1.5)]


@pytest.mark.parametrize("kw", STEP_SETTINGS, ids=lambda kw: ",".join("%s=%g" % it for it in kw.items()))
def test_draws_lie_in_and_follow_the_kept_set(row64, kw):
    """Every drawn id lies in the relaxed kept set; every strict entry that 4 096 draws miss with probability < 1e-9 is seen;
    the frequencies pass test_sample_gpu's goodness-of-fit bound against q over the strict set.  The settings are such that
    the two sets differ in at most 1 % of the kept mass (asserted), so a wrong threshold cannot hide in the relaxation."""
    draws, p = draw_4096(row64, **kw)
    W, N = len(p), len(draws)
    q, strict, relaxed = cut_ref.cut_q(p, rel=REL, **kw)
    w_rel, _ = cut_ref.tempered(p, relaxed, kw.get("temperature", 1.0))
    w_str, _ = cut_ref.tempered(p, strict, kw.get("temperature", 1.0))
    print("kept", int(strict.sum()), "relaxed", int(relaxed.sum()), "mass ratio", w_str.sum() / w_rel.sum(),
          "base", int(sample_ref.kept_mask(p, kw.get("temperature", 1.0), kw.get("top_k", 0), kw.get("top_p", 1.0)).sum()))
    assert w_rel.sum() - w_str.sum() <= 0.01 * w_str.sum()
    assert strict.sum() < (p > 0).sum()                       # the cut does cut
    assert relaxed[draws].all()
    counts = np.bincount(draws, minlength=W)
    sure = strict & ((1 - q) ** N < 1e-9)
    assert sure.any() and (counts[sure] > 0).all()
    big = q * N >= 5                                          # entries with an expectation of >= 5 draws: one by one
    sig = np.sqrt(N * q * (1 - q))
    assert (np.abs(counts[big] - N * q[big]) <= 5 * sig[big] + 1).all()
    rest_q = q[~big].sum()                                    # the long tail as one pooled entry
    assert abs(counts[~big].sum() - N * rest_q) <= 5 * np.sqrt(N * rest_q * (1 - rest_q)) + 1
    assert big.sum() >= 1


def test_degenerate_cuts_on_the_spread_row(row64):
    """epsilon / min_p = 0.999 leave the maximum alone; the smallest positive typical_p keeps the entry nearest the entropy
    (and the maximum), never an empty row."""
    search, ws, B, n, W, b = row64
    for kw in (dict(epsilon=0.999), dict(min_p=0.999)):
        draws, p = draw_4096(row64, **kw)                     # (checks best_p against dist bit for bit)
        top2 = np.sort(p)[-2:]
        assert top2[0] < 0.999 * top2[1] * (1 - REL)          # a unique maximum, clear of the min_p boundary
        assert (draws == int(np.argmax(p))).all(), kw
    tiny = 1e-45                                              # rounds to the smallest positive float
    draws, p = draw_4096(row64, typical_p=tiny)
    q, strict, relaxed = cut_ref.cut_q(p, typical_p=tiny, rel=REL)
    _, q0 = cut_ref.tempered(p, p > 0, 1.0)
    nearest = int(np.argmin(np.where(q0 > 0, np.abs(-np.log(np.where(q0 > 0, q0, 1.0)) - cut_ref.entropy(q0)), np.inf)))
    assert strict[nearest] and strict[int(np.argmax(p))] and strict.sum() <= 2
    assert relaxed[draws].all() and relaxed.sum() <= 4
    if (1 - q[nearest]) ** len(draws) < 1e-9:
        assert (draws == nearest).any()


@pytest.fixture(scope="module")
def greedy_path(setup):
    """The greedy messages of the peaked weights and the distribution rows along them, (commit, step) -> float64 row."""
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, copyish, db = setup
    search = Searcher(peaked)
    out, length, prob = search.greedy(db)
    B, W = db.B, cfg.out_len
    ws = search._begin(db, 1)
    dist = torch.empty(B, W, device="cuda")
    rows = {}
    for step in range(int(length.max()) - 1):
        live = (length > step) & (out[:, step] != 1)
        tok = torch.where(live, out[:, step], torch.zeros_like(out[:, step])).to(torch.int32)
        search._step(ws, B, 1, step, tok, None, dist, None, None)
        d = dist.double().cpu().numpy()
        for b in range(B):
            if int(length[b]) > step + 1:
                rows[(b, step)] = d[b]
    return search, out, length, prob, rows


@pytest.mark.parametrize("kw, n_alone", [(dict(min_p=0.9), 4), (dict(epsilon=0.9), 4), (dict(eta=0.9), 4), (dict(typical_p=1e-3), 3),
                                         (dict(top_k=20, epsilon=0.9), 4), (dict(top_p=0.95, min_p=0.9, eta=0.9), 4),
                                         (dict(top_k=20, typical_p=1e-3), 3)],
                         ids=lambda v: ",".join("%s=%g" % it for it in v.items()) if isinstance(v, dict) else str(v))
def test_peaked_weights_under_every_cut_equal_greedy(setup, greedy_path, kw, n_alone):
    """A cut that leaves the maximum alone is greedy search.  The twin says for which commits that holds on every step of the
    greedy path (relaxed set = the arg-max alone); those commits' samples are the greedy message.  That is every commit of
    the fixture (asserted; epsilon = 0.9 leaves one entry on any row, since a second one holds at most half) except one under
    typical_p: on one of its steps the entry nearest the entropy is not the maximum, and the band keeps both.
    Temperature 0.1 sharpens the rows first: eta's threshold falls with the entropy (sqrt(eta) e^-H), so on a row with two near
    maxima no eta below 1 leaves one entry; at T = 0.1 a runner-up at 0.9 of the maximum holds 0.26 of q and H is below 0.6."""
    cfg, store, ids, peaked, spread, copyish, db = setup
    search, out, length, prob, rows = greedy_path
    T = 0.1
    alone = np.ones(db.B, dtype=bool)
    for (b, step), p in rows.items():
        relaxed = cut_ref.kept_sets(p, temperature=T, rel=REL, **kw)[1]
        alone[b] &= relaxed.sum() == 1
    print("commits whose every step keeps the maximum alone:", alone.tolist())
    assert int(alone.sum()) == n_alone
    toks, lens, p_, logp = search.sample(db, 2, seed=9, temperature=T, use_graphs=False, **kw)
    sel = torch.from_numpy(alone).cuda()
    for j in range(2):
        assert torch.equal(toks[sel, j], out[sel]) and torch.equal(lens[sel, j], length[sel])
        assert torch.allclose(p_[sel, j], prob[sel], rtol=1e-5, atol=0)


def test_fixture_rows_copy_entries_and_an_odd_row_count(setup):
    """The fixture's B commits x 3 samples (12 rows: no multiple of 8 or 16) over several steps, with the weights whose gate
    leans to the copy part: every draw lies in its own row's relaxed set, and the rows include one whose maximum is a copy
    entry and one that keeps a copy entry above its threshold without it being the maximum."""
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, copyish, db = setup
    B, n, W, V = db.B, 3, cfg.out_len, cfg.vocab_size
    R = B * n
    key = torch.arange(B, dtype=torch.int32, device="cuda")
    dist = torch.empty(R, W, device="cuda")
    bid, bp = torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, device="cuda")
    gen = torch.Generator().manual_seed(5)
    copy_max = copy_kept = 0
    for model in (copyish, spread):
        search = Searcher(model)
        ws = search._begin(db, n)
        for step in range(3):
            tok = torch.randint(4, 3000, (R,), generator=gen).to(torch.int32).cuda() if step else \
                torch.full((R,), 2, dtype=torch.int32, device="cuda")
            for kw in (dict(epsilon=0.01), dict(min_p=0.05, top_p=0.95), dict(typical_p=0.8, top_k=100)):
                step_cut(search, ws, B, n, step, tok, key, seed_tensor(31 + step), dist, bid, bp, **kw)
                torch.cuda.synchronize()
                ids_ = bid.long()
                assert int(ids_.min()) >= 0 and int(ids_.max()) < W
                assert torch.equal(bp.view(torch.int32), dist[torch.arange(R), ids_].contiguous().view(torch.int32))
                d = dist.double().cpu().numpy()
                for r in range(R):
                    strict, relaxed = cut_ref.kept_sets(d[r], rel=REL, **kw)
                    assert relaxed[int(ids_[r])], (step, kw, r)
                    top = int(np.argmax(d[r]))
                    copy_max += top >= V
                    copy_kept += bool(strict[V:].any()) and top < V
    assert copy_max > 0 and copy_kept > 0, (copy_max, copy_kept)


# ------------------------------------------------------------------------------------------------ cuts off
@pytest.mark.parametrize("kv_bf16", [False, True])
@pytest.mark.parametrize("n", [1, 3])
def test_cuts_off_is_the_plain_sampler_bit_for_bit(setup, n, kv_bf16):
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, copyish, db = setup
    search = Searcher(spread, kv_bf16=kv_bf16)
    B, W = db.B, cfg.out_len
    R = B * n
    ws = search._begin(db, n)
    key = torch.tensor([7, 11, 13, 17], dtype=torch.int32, device="cuda")[:B]
    seed = seed_tensor(0x1234567890ABCDEF)
    mk = lambda: (torch.empty(R, W, device="cuda"), torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, device="cuda"))
    (dist_a, bid_a, bp_a), (dist_b, bid_b, bp_b) = mk(), mk()
    gen = torch.Generator().manual_seed(5)
    for step in range(3):
        tok = torch.randint(4, 3000, (R,), generator=gen).to(torch.int32).cuda() if step else \
            torch.full((R,), 2, dtype=torch.int32, device="cuda")
        for (temp, k, p) in ((1.0, 0, 1.0), (1.7, 0, 1.0), (1.3, 5, 1.0), (0.8, 0, 0.9), (1.5, 50, 0.9)):
            step_sample(search, ws, B, n, step, tok, key, seed, temp, k, p, dist_a, bid_a, bp_a, flags=search.flags)
            step_cut(search, ws, B, n, step, tok, key, seed, dist_b, bid_b, bp_b, flags=search.flags, temperature=temp, top_k=k,
                     top_p=p, **OFF)
            torch.cuda.synchronize()
            assert torch.equal(bid_a, bid_b) and torch.equal(bp_a, bp_b) and torch.equal(dist_a, dist_b), (step, temp, k, p)
            if k or p < 1:                                   # a cut too small to remove anything leaves the filters' set alone
                for tiny in (dict(epsilon=1e-45), dict(min_p=1e-45), dict(eta=1e-45)):
                    step_cut(search, ws, B, n, step, tok, key, seed, dist_b, bid_b, bp_b, flags=search.flags, temperature=temp,
                             top_k=k, top_p=p, **tiny)
                    torch.cuda.synchronize()
                    assert torch.equal(bid_a, bid_b) and torch.equal(bp_a, bp_b), (step, temp, k, p, tiny)


def test_searcher_defaults_are_the_plain_call_and_state(setup):
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, copyish, db = setup
    search = Searcher(spread)
    kw = dict(temperature=1.5, top_k=40, top_p=0.95, seed=4)
    a = search.sample(db, 3, **kw)
    keys = set(search._ws)
    b = search.sample(db, 3, **kw, **OFF)
    assert set(search._ws) == keys and ("sample", db.B, 3, 1.5, 40, 0.95) in keys
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ the loop
def test_replay_eager_seeds_keys_and_separate_states(setup):
    from fira_icse_amd.model import DeviceBatch
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, copyish, db = setup
    search = Searcher(spread)
    kw = dict(temperature=2.0, epsilon=0.02)
    a = search.sample(db, 3, seed=4, **kw)                          # captures
    b = search.sample(db, 3, seed=4, **kw)                          # replay
    c = search.sample(db, 3, seed=4, use_graphs=False, **kw)        # eager launches
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[3], y[3])
    d = search.sample(db, 3, seed=5, **kw)
    assert not torch.equal(a[0], d[0])
    twice = DeviceBatch(store.batch([ids[0], ids[0]]), cfg)
    same = search.sample(twice, 2, seed=4, keys=[3, 3], **kw)
    assert torch.equal(same[0][0], same[0][1]) and torch.equal(same[3][0], same[3][1])
    diff = search.sample(twice, 2, seed=4, keys=[3, 4], **kw)
    assert not torch.equal(diff[0][0], diff[0][1])
    # the cut is baked into the captured launches: every value owns a state
    eps = lambda e: ("sample", db.B, 3, 2.0, 0, 1.0) + Searcher._check_cuts(1.0, 0.0, e, 0.0, 1.0)
    assert eps(0.02) in search._ws and eps(0.3) not in search._ws
    e = search.sample(db, 3, seed=4, temperature=2.0, epsilon=0.3)
    assert eps(0.3) in search._ws and search._ws[eps(0.3)] is not search._ws[eps(0.02)]
    assert not torch.equal(a[0], e[0])                              # (a tighter cut draws other messages)
    again = search.sample(db, 3, seed=4, **kw)                      # and the first state still replays its own cut
    assert torch.equal(a[0], again[0]) and torch.equal(a[3], again[3])


# ------------------------------------------------------------------------------------------------ errors
BAD = [("min_p", dict(min_p=1.0)), ("min_p", dict(min_p=-0.1)), ("min_p", dict(min_p=float("nan"))),
       ("epsilon", dict(epsilon=1.0)), ("epsilon", dict(epsilon=-1e-3)), ("epsilon", dict(epsilon=float("inf"))),
       ("eta", dict(eta=1.5)), ("eta", dict(eta=-0.5)), ("eta", dict(eta=float("nan"))),
       ("typical_p", dict(typical_p=0.0)), ("typical_p", dict(typical_p=1.5)), ("typical_p", dict(typical_p=float("nan"))),
       ("top_p", dict(typical_p=0.9, top_p=0.9)), ("min_p", dict(typical_p=0.9, min_p=0.1)),
       ("epsilon", dict(typical_p=0.9, epsilon=0.1)), ("eta", dict(typical_p=0.9, eta=0.1))]


def test_argument_errors_name_the_argument(setup):
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, copyish, db = setup
    search = Searcher(peaked)
    B, W = db.B, cfg.out_len
    ws = search._begin(db, 1)
    tok = torch.full((B,), 2, dtype=torch.int32, device="cuda")
    key = torch.arange(B, dtype=torch.int32, device="cuda")
    dist, bid, bp = torch.empty(B, W, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, device="cuda")
    states = set(search._ws)
    for name, kw in BAD:
        with pytest.raises(_lib.FiraError, match="fira_decode_step_sample_cut: .*%s" % name) as e:
            step_cut(search, ws, B, 1, 0, tok, key, seed_tensor(1), dist, bid, bp, **kw)
        if "typical_p" in kw and len(kw) == 2:
            assert "typical_p" in str(e.value)                # a refused pair: both names
        with pytest.raises(ValueError, match=name):
            search.sample(db, 2, **kw)
        assert set(search._ws) == states                      # refused before a state, a workspace or a launch
    step_cut(search, ws, B, 1, 0, tok, key, seed_tensor(1), dist, bid, bp, typical_p=1.0, top_p=0.9, min_p=0.1)   # 1 = off


# ------------------------------------------------------------------------------------------------ command line
def test_cli_epsilon_cutoff_with_mbr_end_to_end(setup, tmp_path):
    """run_model.py test --sample 4 --epsilon-cutoff 0.02 --rerank mbr_bleu on the synthetic data set: the files are well
    formed, the candidates are Searcher.sample's (the test split is the fixture's batch, keyed by its position), and every
    token of every candidate resolves from an entry of the relaxed kept set of the step that emitted it.  Without the flag
    the command writes what the plain sampler gives."""
    from fira_icse_amd import text
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, copyish, db = setup
    root = str(tmp_path)
    synth.write_dataset(root, util.load_golden_raw())
    torch.save(spread_state_dict(cfg), os.path.join(root, "best_model.pt"))
    base = ["test", "--splits", "16,4,4", "--test-batch-size", "4", "--sample", "4", "--rerank", "mbr_bleu", "--sample-seed", "7"]
    out_f, samp_f = os.path.join(root, "OUTPUT", "output_fira"), os.path.join(root, "OUTPUT", "output_fira_samples")
    vocab = json.load(open(os.path.join(root, "DataSet", "word_vocab.json")))
    var_maps = json.load(open(os.path.join(root, "DataSet", "variable.json")))
    r_vocab = {v: k for k, v in vocab.items()}
    search = Searcher(spread)
    B, n, W, V, L = db.B, 4, cfg.out_len, cfg.vocab_size, cfg.sou_len
    written = {}
    for name, flags, kw in (("cut", ["--epsilon-cutoff", "0.02"], dict(epsilon=0.02)), ("plain", [], {})):
        run_cli(base + flags, root)
        test_index = json.load(open(os.path.join(root, "all_index")))["test"]
        lines, recs = open(out_f).read().split("\n"), [json.loads(l) for l in open(samp_f).read().strip().split("\n")]
        assert len(lines) == B + 1 and lines[-1] == "" and len(recs) == B
        toks, lens, _, logp = search.sample(db, n, seed=7, keys=list(range(B)), **kw)
        pick, _ = search.mbr(toks, lens, logp)
        for k, (line, rec) in enumerate(zip(lines, recs)):
            assert sorted(rec) == ["candidates", "logp", "mbr_bleu"] and len(rec["candidates"]) == len(rec["logp"]) == n
            assert len(rec["mbr_bleu"]) == n
            want = [text.detokenize(toks[k, j, :int(lens[k, j])].tolist(), r_vocab, var_maps[test_index[k]]) for j in range(n)]
            assert rec["candidates"] == want and line == want[int(pick[k])]
            assert np.allclose(rec["logp"], logp[k].tolist(), rtol=1e-6)
        written[name] = (open(out_f, "rb").read(), open(samp_f, "rb").read(), toks, lens)
    assert written["cut"][1] != written["plain"][1]
    # teacher-forced replay of every candidate: the entry that emitted a token lies in that step's relaxed kept set
    toks, lens = written["cut"][2], written["cut"][3]
    sou, sub = db.sou.long().cpu().numpy(), db.sub_token.long().cpu().numpy()
    dist = torch.empty(B, W, device="cuda")
    for j in range(n):
        ws = search._begin(db, 1)
        for step in range(int(lens[:, j].max()) - 1):
            live = lens[:, j] > step + 1
            tok = torch.where(lens[:, j] > step, toks[:, j, step], torch.zeros_like(toks[:, j, step])).to(torch.int32)
            search._step(ws, B, 1, step, tok, None, dist, None, None)
            d = dist.double().cpu().numpy()
            for b in range(B):
                if not bool(live[b]):
                    continue
                word = int(toks[b, j, step + 1])
                _, relaxed = cut_ref.kept_sets(d[b], epsilon=0.02, rel=REL)
                entries = np.concatenate([np.arange(V) == word, sou[b] == word, sub[b] == word])
                assert (relaxed & entries).any(), (j, step, b, word)
