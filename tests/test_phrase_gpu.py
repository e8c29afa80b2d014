"""Phrases in the hard search controls on the device: fira_ban_phrases_dist on synthetic rows and fira_beam_select_phrases on
random states against the numpy statement (phrase_ref.py), the two anchors of the selection (fira_beam_select_required with one-word
items, fira_beam_select with none), and the searches with ``phrases=`` through the golden model."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import phrase_ref as P
import require_ref as R
from constrain_ref import argmax_ref
from search_kit import best_pair, bits, count_calls, device_dims, golden_search, messages, offset_rows, outside_untouched, same_search
from test_require_gpu import MODEL, SMALL, SMALL_ODD, geometry, launch as launch_required, make_state, random_dist
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, START, UNK
from fira_icse_amd.decode import Phrases, Searcher, contains_phrase

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the ban kernel alone
T_ROWS = 8
# eight phrases: (5 6) matches at m = l - 1 = 1; (5 6 9 7) and (6 9 7) block the same word at m = T - 1; (6 8) and (5 6 9 7) on the
# tail 5 6 6: one matches, one misses by one word; the rest never match
PHRASES = [(5, 6), (5, 6, 9), (5, 6, 9, 7), (6, 9, 7), (6, 8), (9, 9, 9, 4), (7, 7), (8, 8, 8)]
ROWS = [([START, 5], {6}),                                    # m = 1: the earliest position of a 2-word phrase; m < l - 1 for (5 6 9)
        ([START, 9, 9, 9, 9, 5, 6, 9], {7}),                  # m = T - 1: two phrases, one word
        ([START, 5, 6, 6], {8}),                              # (5 6 9 7) misses by one word; (6 8) matches
        ([START, 5, EOS], set()),                             # finished
        ([START], set()),                                     # m = 0 < l - 1 for every phrase
        ([START, 9, 5], {6}),
        ([START, 5, 6], {9, 8}),                              # m = 2: the earliest position of (5 6 9); m < l - 1 for (5 6 9 7)
        ([START, 9, 6, 9], {7}),                              # (6 9 7) past its earliest position; (5 6 9) misses by its first word
        ([START, 5, 6, 9], {7})]                              # m = 3: the earliest position of the 4-word phrase
BAN_GEOMETRIES = [("no-sub-x1", (37, 5, 0), 1), ("no-sub-x3", (37, 5, 0), 3), ("small-x1", (37, 5, 3), 1), ("small-x3", (37, 5, 3), 3)]


def ban_case(dims, rpc):
    V, L, S = dims
    n_rows, n_commits = len(ROWS), len(ROWS) // rpc
    rng = np.random.RandomState(7 + rpc + S)
    gen = rng.choice((5, 6, 9, EOS, 0), size=(n_rows, T_ROWS)).astype(np.int32)      # (what stays past the length is junk)
    length = np.zeros(n_rows, dtype=np.int32)
    for r, (row, _) in enumerate(ROWS):
        gen[r, :len(row)] = row
        length[r] = len(row)
    sou = np.tile(np.array([6, 7, 8, EOS, 4], dtype=np.int32), (n_commits, 1))          # diff slots carry the blocked words
    sub = np.tile(np.array([7, 6, 8], dtype=np.int32)[:max(S, 1)], (n_commits, 1))      # ... and sub-token slots
    phrase = np.zeros((n_commits, 8, 4), dtype=np.int32)
    plen = np.zeros((n_commits, 8), dtype=np.int32)
    for q, ph in enumerate(PHRASES):
        phrase[:, q, :len(ph)] = ph
        plen[:, q] = len(ph)
    n = np.full(n_commits, 8, dtype=np.int32)
    n[-1] = 5                                                  # the last commit: the first five phrases only
    dist = rng.uniform(1e-6, 1.0, size=(n_rows, V + L + S)).astype(np.float32)
    return dict(dims=dims, rpc=rpc, R=n_rows, gen=gen, length=length, sou=sou, sub=sub, phrase=phrase, plen=plen, n=n, dist=dist)


def ban_reference(case):
    """(mask, dist, edited, best_id, best_p): an exact tie on two free entries and an overtowering blocked entry built in."""
    rpc = case["rpc"]
    mask = np.stack([P.ban_mask(case["gen"][r], case["length"][r], case["sou"][r // rpc], case["sub"][r // rpc][:case["dims"][2]],
                                case["dims"], P.phrases_of(case["phrase"][r // rpc], case["plen"][r // rpc], case["n"][r // rpc]))
                     for r in range(case["R"])])
    dist = case["dist"].copy()
    for r in range(case["R"]):
        free, blk = np.flatnonzero(~mask[r]), np.flatnonzero(mask[r])
        dist[r, free[len(free) // 3]] = dist[r, free[-1]] = np.float32(2.0)
        if len(blk):
            dist[r, blk] = np.float32(3.0)
    out = np.where(mask, np.float32(0.0), dist)
    best = [argmax_ref(out[r]) for r in range(case["R"])]
    return mask, dist, out, np.array([b[0] for b in best], dtype=np.int32), np.array([b[1] for b in best], dtype=np.float32)


def run_ban(case, dist, want_best, offset):
    n_rows, W = dist.shape
    buf, d_dev = offset_rows(dist, offset)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    gen, length, sou, sub = t(case["gen"]), t(case["length"]), t(case["sou"]), t(case["sub"])
    guard = 5                                                  # guard words around the lists: the kernel reads inside them only
    lists = [torch.full((guard + a.size + guard,), -9, dtype=torch.int32, device="cuda") for a in (case["phrase"], case["plen"], case["n"])]
    for buf_l, a in zip(lists, (case["phrase"], case["plen"], case["n"])):
        buf_l[guard:guard + a.size] = t(a.reshape(-1))
    best_id, best_p = best_pair(n_rows, want_best)
    dd = device_dims(*case["dims"], T_ROWS)
    _lib.check(_lib.lib().fira_ban_phrases_dist(_lib.cur_stream(), C.byref(dd), n_rows, case["rpc"], _lib.ptr(gen), _lib.ptr(length),
                                                _lib.ptr(sou), _lib.ptr(sub), *[C.c_void_p(b.data_ptr() + 4 * guard) for b in lists],
                                                _lib.ptr(d_dev), _lib.ptr(best_id), _lib.ptr(best_p)), "fira_ban_phrases_dist")
    torch.cuda.synchronize()
    outside_untouched(buf, offset, n_rows * W)
    for buf_l in lists:
        assert bool((buf_l[:guard] == -9).all()) and bool((buf_l[-guard:] == -9).all())
    return d_dev.cpu(), None if best_id is None else best_id.cpu(), None if best_p is None else best_p.cpu()


@pytest.mark.parametrize("name, dims, rpc", BAN_GEOMETRIES, ids=[g[0] for g in BAN_GEOMETRIES])
def test_ban_kernel_equals_the_reference_bit_for_bit(name, dims, rpc):
    V, L, S = dims
    case = ban_case(dims, rpc)
    mask, dist, out, best_id, best_p = ban_reference(case)
    words = np.concatenate([np.arange(V), case["sou"][0], case["sub"][0][:S]])
    for r, (_, blocked) in enumerate(ROWS):                    # the inputs say what the comments claim
        assert set(words[mask[r]].tolist()) == blocked, (r, blocked)
        assert not blocked or (mask[r, :V].any() and mask[r, V:V + L].any() and (S == 0 or mask[r, V + L:].any()))
    for want_best in (True, False):                            # (without best the row is never read: the other code path)
        for offset in (0, 1, 2, 3):
            got, gid, gp = run_ban(case, dist, want_best, offset)
            assert torch.equal(bits(got), bits(out)), (name, want_best, offset)
            if want_best:
                assert gid.tolist() == best_id.tolist(), (name, offset)
                assert torch.equal(bits(gp), bits(best_p)), (name, offset)


def test_ban_kernel_without_phrases_leaves_the_rows_alone():
    case = ban_case((37, 5, 3), 3)
    case["n"][:] = 0
    mask, dist, out, best_id, best_p = ban_reference(case)
    assert not mask.any()
    got, gid, gp = run_ban(case, dist, True, 1)
    assert torch.equal(bits(got), bits(dist)) and gid.tolist() == best_id.tolist() and torch.equal(bits(gp), bits(best_p))


# ------------------------------------------------------------------------------------------------ the selection kernel alone
ITEM_SETS = {"none": [], "pair": [[4, 5]], "triple+word": [[4, 4, 5], [6]], "shared": [[4, 5], [5, 6]], "words": [[4], [5], [6], [7]]}


def with_items(st, item_sets):
    B = st["B"]
    words, lens, n = np.zeros((B, 4), dtype=np.int32), np.zeros((B, 4), dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b, items in enumerate(item_sets):
        flat = [w for item in items for w in item]
        words[b, :len(flat)], lens[b, :len(items)], n[b] = flat, [len(i) for i in items], len(items)
    st.update(item_words=words, item_len=lens, n_items=n)
    return st


def launch_phrases(st, dist):
    B, beam = st["B"], st["beam"]
    V, L, S, T = geometry(st["geo"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    gen, length, prob, fin, active = t(st["gen"].reshape(B * beam, T)), t(st["length"].reshape(-1)), t(st["prob"].reshape(-1)), \
        t(st["fin"].reshape(-1)), t(st["active"])
    done = torch.tensor([st["done"]], dtype=torch.int32, device="cuda")
    sou, sub, dist_d = t(st["sou"]), t(st["sub"]), t(dist.reshape(B * beam, -1))
    g_out = torch.full_like(gen, -7)
    l_out, p_out, parent, met = torch.full_like(length, -7), torch.full_like(prob, -7.0), torch.full_like(length, -7), \
        torch.full_like(length, -7)
    words, lens, n = t(st["item_words"]), t(st["item_len"]), t(st["n_items"])
    dd = device_dims(**st["geo"])
    _lib.check(_lib.lib().fira_beam_select_phrases(
        _lib.cur_stream(), C.byref(dd), B, beam, _lib.ptr(dist_d), _lib.ptr(fin), _lib.ptr(active), _lib.ptr(done), _lib.ptr(sou),
        _lib.ptr(sub), _lib.ptr(gen), _lib.ptr(length), _lib.ptr(prob), _lib.ptr(g_out), _lib.ptr(l_out), _lib.ptr(p_out),
        _lib.ptr(parent), _lib.ptr(words), _lib.ptr(lens), _lib.ptr(n), _lib.ptr(met)), "fira_beam_select_phrases")
    torch.cuda.synchronize()
    return g_out.cpu(), l_out.cpu(), p_out.cpu(), parent.cpu(), met.cpu()


def equals_the_reference(st, dist):
    B, beam = st["B"], st["beam"]
    V, L, S, T = geometry(st["geo"])
    g, l, p, parent, met = launch_phrases(st, dist)
    all_picks = []
    for b in range(B):
        rows = slice(b * beam, (b + 1) * beam)
        words = R.words_of(st["sou"][b], st["sub"][b], V)
        items = P.items_of(st["item_words"][b], st["item_len"][b], st["n_items"][b])
        picks = P.select(dist[b], st["fin"][b], st["active"], st["prob"][b], st["length"][b], st["gen"][b], words, items)
        wg, wl, wp, wparent, wmet = R.apply(picks, st["gen"][b].astype(np.int64), st["length"][b].astype(np.int64))
        assert (g[rows].numpy() == wg).all(), ("gen", b)
        assert (l[rows].numpy() == wl).all(), ("len", b)
        assert torch.equal(bits(p[rows]), bits(wp)), ("prob", b, p[rows].tolist(), wp.tolist())
        assert (parent[rows].numpy() - b * beam == wparent).all(), ("parent", b)
        assert (met[rows].numpy() == wmet).all(), ("met", b, met[rows].tolist(), wmet.tolist())
        all_picks.append((items, picks))
    return all_picks


def plant(st, b, j, words, finished=False):
    """Hypothesis j of commit b becomes <start> words [<eos>]."""
    row = [START] + list(words) + ([EOS] if finished else [])
    st["gen"][b, j] = 0
    st["gen"][b, j, :len(row)] = row
    st["length"][b, j] = len(row)
    st["fin"][b, j] = int(finished)
    st["prob"][b, j] = max(st["prob"][b, j], np.float32(0.3))


@pytest.mark.parametrize("beam", [2, 3, 5, 8])
def test_selection_kernel_equals_the_reference(beam):
    rng = np.random.RandomState(200 + beam)
    names = sorted(ITEM_SETS)
    seen_banks, n_phase2 = set(), 0
    for trial in range(6):
        geo = SMALL_ODD if trial % 2 else SMALL
        st = make_state(rng, geo, 3, beam, [0, 0, 0], zero_prob=0.15 if trial else 0.0, words_hi=8)    # words 3..7: overlaps happen
        sets = [ITEM_SETS[names[(trial + b) % len(names)]] for b in range(3)]
        with_items(st, sets)
        st["sou"][:, 1] = EOS                                  # <eos> carried by a copy slot
        plant(st, 0, 0, [4])                                   # mid-phrase for (4 5) and (4 4 5)
        plant(st, 1, 0, [3, 4, 4])                             # the tail 4 4 of (4 4 5): one more 4 restarts at 2
        plant(st, 2, 1, [4, 5, 3])                             # a completed phrase
        plant(st, 1, 1, [4, 4, 5, 6], finished=True)           # a finished hypothesis that holds everything
        st["active"][:beam] = (st["fin"] == 0).any(0)
        st["active"][8] = st["active"][:beam].sum()
        dist = random_dist(rng, st, zeros=0.5 if trial == 3 else 0.1)
        dist[:, :, ::7] = dist[:, :, 3:4]                      # exact ties: the index decides
        if trial == 3:
            st["prob"][:, 1:] = 0                              # few positive candidates: phase 2 fills
            dist[:, 0, 4:] = 0
        if trial == 4:
            st["prob"][:] = np.float32(0.5)                    # every row ties with every other
            dist[:] = np.float32(0.25)
        if trial == 5:                                         # the latch: the state is passed through, met is still written
            st["done"] = 1
            g, l, p, parent, met = launch_phrases(st, dist)
            assert (g.numpy() == st["gen"].reshape(3 * beam, -1)).all() and (l.numpy() == st["length"].reshape(-1)).all()
            assert torch.equal(bits(p), bits(st["prob"].reshape(-1))) and parent.tolist() == list(range(3 * beam))
            want = [P.progress(P.hyp(st["gen"][b, j], st["length"][b, j]), sets[b]) for b in range(3) for j in range(beam)]
            assert met.tolist() == want and max(want) > 0
            continue
        for items, picks in equals_the_reference(st, dist):
            seen_banks |= {p["bank"] for p in picks}
            n_phase2 += sum(1 for p in picks if p["phase"] == 2)
    assert seen_banks >= {0, 1, 2} and n_phase2 > 0            # the inputs are not vacuous


def test_selection_kernel_at_the_models_geometry():
    rng = np.random.RandomState(9)
    st = with_items(make_state(rng, MODEL, 3, 5, [0, 0, 0], words_hi=8), [ITEM_SETS["triple+word"], [], ITEM_SETS["shared"]])
    plant(st, 0, 0, [4, 4])
    plant(st, 2, 0, [7, 4])
    picks = equals_the_reference(st, random_dist(rng, st))
    assert max(p["bank"] for _, ps in picks for p in ps) >= 3


@pytest.mark.parametrize("geo, beam, counts", [(SMALL, 2, [1, 0, 2]), (SMALL_ODD, 3, [2, 0, 1]), (SMALL, 5, [4, 0, 3]),
                                               (SMALL_ODD, 8, [0, 4, 2]), (MODEL, 5, [3, 0, 4])],
                         ids=["small-2", "odd-3", "small-5", "odd-8", "model-5"])
def test_one_word_items_give_beam_select_required_bit_for_bit(geo, beam, counts):
    rng = np.random.RandomState(300 + beam)
    for trial in range(1 if geo is MODEL else 4):
        st = make_state(rng, geo, 3, beam, counts, zero_prob=0.15 if trial else 0.0)
        st["done"] = int(trial == 2)
        st.update(item_words=st["required"], item_len=np.ones((3, 4), dtype=np.int32), n_items=st["n_required"])
        dist = random_dist(rng, st, zeros=0.5 if trial == 3 else 0.1)
        dist[:, :, ::7] = dist[:, :, 3:4]
        want, got = launch_required(st, dist), launch_phrases(st, dist)
        for a, b, name in zip(got, want, ("gen", "len", "prob", "parent", "met")):
            assert torch.equal(bits(a), bits(b)), (trial, name)


@pytest.mark.parametrize("geo, beam", [(SMALL, 2), (SMALL_ODD, 5), (SMALL, 8), (MODEL, 3)], ids=["small-2", "odd-5", "small-8", "model-3"])
def test_without_items_it_is_beam_select_bit_for_bit(geo, beam):
    rng = np.random.RandomState(400 + beam)
    for case in ("mixed", "done", "start"):
        st = make_state(rng, geo, 3, beam, [0, 0, 0])
        if case == "start":
            st = make_state(rng, geo, 3, beam, [0, 0, 0], finished=0.0, max_len=1, zero_prob=0.0)
            st["prob"][:] = 0
            st["prob"][:, 0] = 1
        st["done"] = int(case == "done")
        with_items(st, [[], [], []])
        st["item_words"][:] = st["required"]                   # words in place, the count alone decides
        st["item_len"][:] = 2
        dist = random_dist(rng, st)
        dist[:, :, ::7] = dist[:, :, 3:4]
        want, got = launch_required(st, dist, required=False), launch_phrases(st, dist)
        for a, b, name in zip(got[:4], want[:4], ("gen", "len", "prob", "parent")):
            assert torch.equal(bits(a), bits(b)), (case, name)
        assert (got[4] == 0).all()


def test_selection_refusals_return_non_zero_with_a_message():
    for geo, beam, word in ((dict(SMALL, tar_len=65), 4, "tar_len"), (dict(SMALL, vocab=8), 4, "vocabulary"),
                            (dict(SMALL, sou_len=1000, sub_len=25), 4, "memory slots"), (SMALL, 1, "n_beam"), (SMALL, 9, "n_beam")):
        dd = device_dims(**geo)
        assert _lib.lib().fira_beam_select_phrases(_lib.cur_stream(), C.byref(dd), 3, beam, *([C.c_void_p(16)] * 17)) != 0
        msg = _lib.lib().fira_last_error().decode()
        assert "fira_beam_select_phrases" in msg and word in msg, msg
    dd = device_dims(**SMALL)
    assert _lib.lib().fira_beam_select_phrases(_lib.cur_stream(), C.byref(dd), 3, 4, *([C.c_void_p(16)] * 14), None, None, None) != 0
    assert "null pointer" in _lib.lib().fira_last_error().decode()
    assert _lib.lib().fira_ban_phrases_dist(_lib.cur_stream(), C.byref(dd), 6, 3, *([C.c_void_p(16)] * 4), None, None, None,
                                            C.c_void_p(16), None, None) != 0
    assert "phrase" in _lib.lib().fira_last_error().decode()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ through the model
MODEL_TAR_LEN = 8                                              # test_require_gpu.py says why: raw products stay positive in fp32
BEAM = 5


@pytest.fixture(scope="module")
def setup():
    g = golden_search(tar_len=MODEL_TAR_LEN)
    return g.cfg, g.model, g.db, g.searchers[0]


def bigrams_to_ban(gen, length, prob=None):
    """Per commit, the first bigram of bannable ids in the first message (of positive probability) that has one."""
    out = []
    gen, length = gen.cpu(), length.cpu()
    if gen.dim() == 2:
        gen, length = gen[:, None], length[:, None]
    for b in range(gen.shape[0]):
        found = []
        for j in range(gen.shape[1]):
            if prob is not None and not float(prob[b, j]) > 0:
                continue
            msg = gen[b, j, 1:int(length[b, j])].tolist()
            found = [tuple(msg[o:o + 2]) for o in range(len(msg) - 1) if min(msg[o:o + 2]) >= UNK][:1]
            if found:
                break
        out.append(found)
    return out


def holds_none(result, banned, positive_only=True):
    gen, length, prob = [t.cpu() for t in result[:3]]
    gen, length, prob = gen.reshape(len(banned), -1, gen.shape[-1]), length.reshape(len(banned), -1), prob.reshape(len(banned), -1)
    for b, row in enumerate(banned):
        for j in range(gen.shape[1]):
            if positive_only and not float(prob[b, j]) > 0:
                continue
            msg = gen[b, j, 1:int(length[b, j])].tolist()
            assert not any(contains_phrase(msg, ph) for ph in row), (b, j, msg, row)


@pytest.fixture(scope="module")
def plain_beam(setup):
    cfg, model, db, search = setup
    return [t.cpu().clone() for t in search.beam(db, 3)]


def test_a_banned_bigram_leaves_the_beam(setup, plain_beam, monkeypatch):
    cfg, model, db, search = setup
    banned = bigrams_to_ban(*plain_beam)
    assert sum(1 for row in banned if row) >= 2
    keys = set(search._ws)
    got = search.beam(db, 3, phrases=Phrases(banned=banned))
    assert len(got) == 3 and set(search._ws) - keys == {("beam", db.B, 3, "ban-phrases")}
    holds_none(got, banned)
    assert messages(got[0], got[1]) != messages(plain_beam[0], plain_beam[1])      # at least one message changed
    same_search(search.beam(db, 3, phrases=Phrases(banned=banned), use_graphs=False), got)
    # other lists: the same state and graphs, nothing captured anew
    other = [row[::-1] and [row[0][::-1]] for row in banned]
    graphs = list(search._ws[("beam", db.B, 3, "ban-phrases")]["graphs"])
    captured = []
    monkeypatch.setattr(torch.cuda, "graph", lambda *a, **k: captured.append(1) or (_ for _ in ()).throw(AssertionError("capture")))
    calls = count_calls(monkeypatch, lambda: search.beam(db, 3, phrases=Phrases(banned=other)))
    assert not captured and set(calls) == {"fira_decode_begin_ex"} and search._ws[("beam", db.B, 3, "ban-phrases")]["graphs"] == graphs
    assert set(search._ws) - keys == {("beam", db.B, 3, "ban-phrases")}


def test_a_banned_bigram_leaves_greedy_greedy_many_and_sample_search(setup):
    cfg, model, db, search = setup
    plain = search.greedy(db)
    banned = bigrams_to_ban(plain[0], plain[1])
    assert sum(1 for row in banned if row) >= 2
    ph = Phrases(banned=banned)
    got = search.greedy(db, phrases=ph)
    holds_none(got, banned, positive_only=False)
    assert messages(got[0], got[1]) != messages(plain[0], plain[1])
    assert ("greedy", db.B, "ban-phrases") in search._ws
    same_search(search.greedy(db, phrases=ph, use_graphs=False), got)
    many = search.greedy_many([db, db], in_flight=2, phrases=ph)
    for res in many:
        same_search(res, got)
    kw = dict(temperature=1.0, top_k=50, seed=11)
    drawn = search.sample_search(db, 2, **kw)
    banned_s = bigrams_to_ban(drawn[0], drawn[1])
    assert sum(1 for row in banned_s if row) >= 2
    again = search.sample_search(db, 2, phrases=Phrases(banned=banned_s), **kw)
    holds_none(again, banned_s, positive_only=False)
    assert messages(again[0], again[1]) != messages(drawn[0], drawn[1])


def reference_beam(search, db, beam, items_rows):
    """The beam's loop on the host: the engine's step distribution, phrase_ref.select and require_ref.apply per commit and step."""
    cfg, dev = search.cfg, search.model.device_
    B, T, W, V = db.B, cfg.tar_len, cfg.out_len, cfg.vocab_size
    ws = search._begin(db, beam)
    sou, sub = db.sou.cpu().numpy(), db.sub_token.cpu().numpy()
    gen = np.zeros((B, beam, T), dtype=np.int64)
    gen[:, :, 0] = START
    length = np.ones((B, beam), dtype=np.int64)
    prob = np.zeros((B, beam), dtype=np.float32)
    prob[:, 0] = 1.0
    dist = torch.empty((B * beam, W), dtype=torch.float32, device=dev)
    parent = None
    for step in range(T - 1):
        fin = np.take_along_axis(gen, (length - 1)[:, :, None], 2)[:, :, 0] == EOS
        active = (~fin).any(0).astype(np.int32)
        if not active.any():
            break
        tok = np.where(length > step, gen[:, :, step], 0).astype(np.int32).reshape(-1)
        search._step(ws, B, beam, step, torch.from_numpy(tok).to(dev), parent, dist, None, None)
        d = dist.cpu().numpy().reshape(B, beam, W)
        par = np.zeros((B, beam), dtype=np.int32)
        for b in range(B):
            picks = P.select(d[b], fin[b].astype(np.int32), active, prob[b], length[b], gen[b], R.words_of(sou[b], sub[b], V),
                             [list(i) for i in items_rows[b]])
            gen[b], length[b], prob[b], p_slot, _ = R.apply(picks, gen[b], length[b])
            par[b] = b * beam + p_slot
        parent = torch.from_numpy(par.reshape(-1)).to(dev)
    met = np.array([[P.progress(P.hyp(gen[b, j], length[b, j]), items_rows[b]) for j in range(beam)] for b in range(B)])
    return torch.from_numpy(gen), torch.from_numpy(length), torch.from_numpy(prob), torch.from_numpy(met)


def test_a_required_three_token_item(setup, plain_beam, monkeypatch):
    cfg, model, db, search = setup
    copied = int(next(w for w in db.sou[3].tolist() if w > UNK))   # a word commit 3's diff carries: copy slots count too
    items = [[(700, 1500, 40)], [], [(90, 2300), (41,)], [(copied, 90, 2301)]]
    plain5 = search.beam(db, BEAM)
    for b, row in enumerate(items):
        for msg in messages(plain5[0][b], plain5[1][b]):
            assert not any(contains_phrase(msg, item) for item in row if len(item) > 1)      # the plain beam does not produce them
    keys = set(search._ws)
    got = search.beam(db, BEAM, phrases=Phrases(required=items))
    assert len(got) == 4 and set(search._ws) - keys == {("beam", db.B, BEAM, "require-phrases")}
    gen, length, prob, met = [t.cpu() for t in got]
    want = reference_beam(search, db, BEAM, items)
    same_search(got, want)
    assert torch.equal(met, want[3])
    best = Searcher.best_required(None, gen, length, prob, met)
    for b, row in enumerate(items):
        total = sum(len(i) for i in row)
        for j in range(BEAM):
            msg = gen[b, j, 1:int(length[b, j])].tolist()
            assert int(met[b, j]) == P.progress(msg, row)
            if int(met[b, j]) == total:
                assert all(contains_phrase(msg, item) for item in row), (b, j, msg)
        j_ref = [j for j in range(BEAM) if float(want[2][b, j]) > 0 and int(want[3][b, j]) == total]
        if j_ref and row:                                      # the reference search has one: the pick holds every item
            assert all(contains_phrase(best[b][1:], item) for item in row), (b, best[b])
            assert best[b][-1] == EOS or len(best[b]) == cfg.tar_len
    assert sum(1 for b, row in enumerate(items) if row and (met[b] == sum(len(i) for i in row)).any()) >= 2
    # the commit without items: the plain beam bit for bit
    assert torch.equal(bits(prob[1]), bits(plain5[2][1].cpu())) and (met[1] == 0).all()
    same_search(search.beam(db, BEAM, phrases=Phrases(required=items), use_graphs=False), got)
    # a second call with other lists captures nothing new
    other = [[(90,)], [(700, 40)], [], items[3]]
    graphs = list(search._ws[("beam", db.B, BEAM, "require-phrases")]["graphs"])
    monkeypatch.setattr(torch.cuda, "graph", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a second capture")))
    calls = count_calls(monkeypatch, lambda: search.beam(db, BEAM, phrases=Phrases(required=other)))
    assert set(calls) == {"fira_decode_begin_ex"} and search._ws[("beam", db.B, BEAM, "require-phrases")]["graphs"] == graphs
    assert set(search._ws) - keys == {("beam", db.B, BEAM, "require-phrases")}


def test_one_word_items_are_the_required_words_search(setup):
    cfg, model, db, search = setup
    words = [[700], [1500, 40], [], [90, 2300]]
    want = search.beam(db, BEAM, require=words)
    got = search.beam(db, BEAM, phrases=Phrases(required=[[(w,) for w in row] for row in words]))
    same_search(got, want)
    assert torch.equal(got[3], want[3])


def test_off_is_todays_search_call_for_call(setup, plain_beam, monkeypatch):
    cfg, model, db, search = setup
    fresh = Searcher(model)
    runs = {"beam": lambda **k: fresh.beam(db, 3, use_graphs=False, **k), "greedy": lambda **k: fresh.greedy(db, use_graphs=False, **k),
            "sample_search": lambda **k: fresh.sample_search(db, 2, seed=3, use_graphs=False, **k)}
    for name, run in runs.items():
        base = {}
        run()                                                  # (the first call alone sizes the workspace)
        calls = count_calls(monkeypatch, lambda: base.update(res=run()))
        keys = set(fresh._ws)
        for off in (None, Phrases(), Phrases(banned=[[]] * db.B, required=[[]] * db.B)):
            got = {}
            assert count_calls(monkeypatch, lambda: got.update(res=run(phrases=off))) == calls, (name, off)
            assert len(got["res"]) == len(base["res"]) and set(fresh._ws) == keys
            for a, b in zip(got["res"], base["res"]):
                assert torch.equal(bits(a), bits(b)), (name, off)
        assert "fira_ban_phrases_dist" not in calls and "fira_beam_select_phrases" not in calls
    same_search(fresh.beam(db, 3, phrases=Phrases()), plain_beam)


# ------------------------------------------------------------------------------------------------ scripts/phrase_probe.py
def run_probe(args, root):
    import subprocess
    import sys
    import util
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "scripts", "phrase_probe.py"), "--root", root, "--splits", "16,4,4",
                        "--test-batch-size", "4"] + args, cwd=root, env=dict(os.environ, PYTHONPATH=util.REPO), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r, open(os.path.join(root, "OUTPUT", "output_fira_phrases")).read().split("\n")[:-1]


def plain_words(line):
    return [w for w in line.split() if re.fullmatch(r"w\d+", w)]                  # the synthetic vocabulary's words


def test_the_probe_decodes_counts_and_times(tmp_path):
    import util
    from fira_icse_amd import synth
    from fira_icse_amd.config import FiraConfig
    from fira_icse_amd.model import reference_init_state_dict
    root = str(tmp_path)
    synth.write_dataset(root, util.load_golden_raw())
    torch.manual_seed(0)
    torch.save(util.peaked_state_dict(reference_init_state_dict(FiraConfig()), seed=2), os.path.join(root, "best_model.pt"))
    r, lines = run_probe(["--reps", "0"], root)
    assert len(lines) == 4 and "0 of 0 messages with required items" in r.stdout and "|" not in r.stdout
    pairs = [ws[o:o + 2] for ws in map(str.split, lines) for o in range(len(ws) - 1) if plain_words(" ".join(ws[o:o + 2])) == ws[o:o + 2]]
    assert pairs
    ban = " ".join(pairs[0])
    words = sorted(set(w for line in lines for w in plain_words(line)))
    item = " ".join(words[:3][::-1])
    r, got = run_probe(["--beam", "5", "--reps", "3", "--ban-phrases", ban + ",nosuchword here", "--require-phrases", item,
                        "--out", os.path.join(root, "timing.md")], root)
    assert len(got) == 4 and all(ban not in " %s " % " ".join(l.split()) for l in got) and got != lines
    assert re.search(r"\d of 4 messages with required items hold all their items", r.stdout), r.stdout
    assert "warning: 4 phrases" in r.stderr                        # the unknown phrase, once per commit
    table = open(os.path.join(root, "timing.md")).read()
    for row in ("beam 5, no phrases", "beam 5, require= with the items' words", "beam 5, phrases"):
        assert "| %s |" % row in table, table
