"""Per-commit word sets on the device: fira_wordset_dist on synthetic rows against the numpy statement (wordset_ref.py), bit for
bit, and the whole searches on the golden commits: ``deny`` is ``Constraints(banned=)``, ``boost`` is ``Penalties(bias=)``, the
sets that block nothing are the plain search, and under ``ground`` every written word is one the commit carries."""
import ctypes as C

import numpy as np
import pytest
import torch

import wordset_ref as WR
from search_kit import best_pair, bits, count_calls, device_dims, golden_search, messages, offset_rows, outside_untouched, same_search
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, PAD, START, UNK
from fira_icse_amd.decode import Constraints, Penalties, Searcher, WordSets

pytestmark = pytest.mark.gpu

SETS = ("allow", "deny", "boost", "ground")
COMBOS = [("allow",), ("deny",), ("boost",), ("ground",), SETS]


# ------------------------------------------------------------------------------------------------ the kernel alone
def pack_dirty(ids, V, n_commits):
    """The packed set of every commit with every bit at or past V in the last word SET: the kernel must ignore them."""
    a = WordSets.pack([sorted(ids)] * n_commits, V)
    tail = V - 32 * (a.shape[1] - 1)
    if tail < 32:
        a[:, -1] |= np.uint32((0xFFFFFFFF << tail) & 0xFFFFFFFF)
    return a


def small_case(V, L, S, R, rpc, seed=3):
    """R rows of tar_len 4 over R / rpc commits.  Row r is of kind r % 4: <start> alone (length 0 where r >= 4: clamped to 1);
    finished; one word, and the row whose free entries are all 0; a full buffer with length 9 (clamped to tar_len)."""
    T, NS = 4, L + S
    n_commits = R // rpc
    rng = np.random.RandomState(seed + V + 7 * NS + R + rpc)
    gw = 4 if V > 4 else 3                                     # the grounded word whose slot is invalid in the even commits
    if NS == 2:
        sou = np.array([[3] for b in range(n_commits)], dtype=np.int32)
        sub = np.array([[V + 2 if b % 2 else gw] for b in range(n_commits)], dtype=np.int32)
        valid = np.array([[0b10 if b % 2 else 0b01] for b in range(n_commits)], dtype=np.uint32)
    else:
        # a denied (and grounded) word; an id past the vocabulary; the grounded word; <eos>; <pad> -- then a second grounded word,
        # a negative id, one more word
        sou = np.array([[3, V + 5, gw, EOS, PAD][:L] for b in range(n_commits)], dtype=np.int32)
        sub = np.array([[7 if V > 7 else 3, -1, 5 if V > 5 else 3][:S] for b in range(n_commits)], dtype=np.int32)
        valid = np.array([[0b11101111 if b % 2 else 0b11101011] for b in range(n_commits)], dtype=np.uint32)
    valid |= np.uint32((0xFFFFFFFF << NS) & 0xFFFFFFFF)       # the bits past the last slot are set and must not matter
    gen = rng.choice((3, EOS, 0), size=(R, T)).astype(np.int32)            # (what stays past the length is junk)
    length = np.zeros(R, dtype=np.int32)
    for r in range(R):
        row, n = [([START], 1), ([START, 3, EOS], 3), ([START, 3], 2), ([START, 3, 3, 3], 9)][r % 4]
        gen[r, :len(row)] = row
        length[r] = 0 if (r % 4 == 0 and r >= 4) else n
    pool = range(3, V)
    ids = dict(allow={w for w in pool if w % 2}, deny={w for w in pool if w % 3 == 0},
               boost={w for w in pool if w % 4 in (0, 1)} | {EOS}, ground={w for w in pool if w % 3 == 1} | {3})
    sets = {k: pack_dirty(v, V, n_commits) for k, v in ids.items()}
    factor = np.array([np.float32(np.exp(1.0)), np.float32(0.25), np.float32(3.0)] * 3, dtype=np.float32)[:n_commits]
    dist = rng.uniform(1e-6, 1.0, size=(R, V + NS)).astype(np.float32)
    return dict(dims=(V, L, S), rpc=rpc, R=R, T=T, gen=gen, length=length, sou=sou, sub=sub, valid=valid, sets=sets,
                factor=factor, dist=dist, zero_rows=[r for r in range(R) if r % 4 == 2])


def argmax_no_nan(row):
    """(value descending, index ascending); NaN never wins; nothing but NaN: entry 0."""
    return WR.argmax_ref(np.where(np.isnan(row), np.float32(-np.inf), row))


def reference(case, combo):
    """(dist, edited, blocked, boosted, best_id, best_p) under the sets of ``combo``: an exact tie on two free entries, a towering
    value on every blocked entry, a NaN on entry 0 of the rows that are not left all zero, and the rows that are."""
    S = case["dims"][2]
    given = {k: (case["sets"][k] if k in combo else None) for k in SETS}

    def rows(dist):
        return [WR.wordset_row(dist[r], case["gen"][r], case["length"][r], case["sou"][r // case["rpc"]],
                               case["sub"][r // case["rpc"]][:S], case["dims"],
                               **{k: None if v is None else v[r // case["rpc"]] for k, v in given.items()},
                               slot_valid=case["valid"][r // case["rpc"]], factor=case["factor"][r // case["rpc"]])
                for r in range(case["R"])]
    dist = case["dist"].copy()
    for r, (_, blk, up) in enumerate(rows(dist)):
        free = np.flatnonzero(~blk & ~up)
        if len(free):
            dist[r, free[len(free) // 3]] = dist[r, free[-1]] = np.float32(2.0)
        dist[r, blk] = np.float32(3.0)
        if r in case["zero_rows"]:
            dist[r, ~blk] = np.float32(0.0)
        else:
            dist[r, 0] = np.float32(np.nan)                    # (id 0 is in no boost set: the NaN is zeroed or kept, never multiplied)
    out = rows(dist)
    edited = np.stack([o[0] for o in out])
    best = [argmax_no_nan(edited[r]) for r in range(case["R"])]
    return (dist, edited, np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.array([b[0] for b in best], dtype=np.int32), np.array([b[1] for b in best], dtype=np.float32))


def run_kernel(case, combo, dist, want_best, offset):
    n_rows, W = dist.shape
    buf, d_dev = offset_rows(dist, offset)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    gen, length, sou, sub = t(case["gen"]), t(case["length"]), t(case["sou"]), t(case["sub"])
    sets = [t(case["sets"][k].view(np.int32)) if k in combo else None for k in SETS]
    valid, factor = t(case["valid"].view(np.int32)), t(case["factor"])
    best_id, best_p = best_pair(n_rows, want_best)
    dd = device_dims(*case["dims"], case["T"])
    _lib.check(_lib.lib().fira_wordset_dist(_lib.cur_stream(), C.byref(dd), n_rows, case["rpc"], _lib.ptr(gen), _lib.ptr(length),
                                            _lib.ptr(sou), _lib.ptr(sub), *[_lib.ptr(s) for s in sets],
                                            _lib.ptr(valid) if "ground" in combo else None,
                                            _lib.ptr(factor) if "boost" in combo else None, _lib.ptr(d_dev),
                                            _lib.ptr(best_id), _lib.ptr(best_p)), "fira_wordset_dist")
    torch.cuda.synchronize()
    outside_untouched(buf, offset, n_rows * W)
    return d_dev.cpu(), None if best_id is None else best_id.cpu(), None if best_p is None else best_p.cpu()


def equals_the_reference(case, combo, ref, offsets=(0, 1, 2, 3), tag=None):
    dist, edited, _, _, best_id, best_p = ref
    for want_best in (True, False):                            # (without best the free entries are never read: the other path)
        for offset in offsets:
            got, gid, gp = run_kernel(case, combo, dist, want_best, offset)
            assert torch.equal(bits(got), bits(edited)), (tag, combo, want_best, offset)
            if want_best:
                assert gid.tolist() == best_id.tolist(), (tag, combo, offset)
                assert torch.equal(bits(gp), bits(best_p)), (tag, combo, offset)


GEOMETRIES = [(V, L, S, rpc) for V in (4, 33, 70) for L, S in ((1, 1), (5, 3)) for rpc in (1, 3)]


@pytest.mark.parametrize("V, L, S, rpc", GEOMETRIES, ids=["v%d-%d+%d-x%d" % g for g in GEOMETRIES])
def test_kernel_equals_the_reference_bit_for_bit(V, L, S, rpc):
    for R in ((1, 7) if rpc == 1 else (3, 6)):
        case = small_case(V, L, S, R, rpc)
        for combo in COMBOS:
            ref = reference(case, combo)
            equals_the_reference(case, combo, ref, tag=(V, L, S, rpc, R))


def test_the_rows_hold_what_the_statement_speaks_of():
    """The inputs say what the comments claim (V = 33, 5 + 3 slots, two commits of three rows)."""
    V, L, S = 33, 5, 3
    case = small_case(V, L, S, 6, 3)
    slot = lambda j: V + j
    dist, edited, blk, up, best_id, best_p = reference(case, ("deny",))
    assert not blk[1].any() and torch.equal(bits(edited[1]), bits(dist[1]))           # a finished row: its bits stay
    assert blk[0, 3] and blk[0, slot(0)] and case["sou"][0, 0] == 3                   # a slot that carries a denied word
    assert not blk[0, slot(1)] and case["sou"][0, 1] >= V and not blk[0, slot(L + 1)] and case["sub"][0, 1] < 0
    assert np.isnan(edited[0, 0]) and best_id[0] != 0                                 # a NaN entry never wins
    assert not edited[2].any() and best_id[2] == 0 and best_p[2] == 0                 # a row left all zero reports entry 0
    dist, edited, blk, up, best_id, best_p = reference(case, ("allow",))
    assert blk[0, slot(1)] and blk[0, slot(L + 1)]                                    # ids outside [0, V): blocked under allow
    assert not blk[0, EOS] and not blk[0, slot(3)] and case["sou"][0, 3] == EOS       # <eos> under allow is kept
    assert blk[0, 4] and not blk[0, 5] and blk[0, 0] and edited[0, 0] == 0            # (the NaN of a blocked entry becomes 0)
    dist, edited, blk, up, best_id, best_p = reference(case, ("ground",))
    assert case["sou"][0, 2] == 4 and case["sou"][3 // 3, 2] == 4
    assert blk[0, 4] and blk[0, slot(2)]                       # commit 0: the grounded word 4 sits in an INVALID slot only: blocked
    assert not blk[3, 4] and not blk[3, slot(2)]               # commit 1: the same word in a valid slot: kept
    assert not blk[0, 7] and not blk[0, slot(L)] and blk[0, 10]                       # carried by a sub-token slot; carried by none
    dist, edited, blk, up, best_id, best_p = reference(case, SETS)
    assert up.any() and blk.any() and not (up & blk).any() and up[0, EOS] and up[0, slot(3)]
    assert edited[0, EOS] == np.float32(dist[0, EOS]) * case["factor"][0]


def test_kernel_at_the_limits():
    V, L, S, T = 25600, 600, 424, 64
    NS, R, rpc = L + S, 4, 2
    rng = np.random.RandomState(11)
    ids = {"allow": rng.choice(V, V // 2, replace=False), "deny": rng.choice(V, 1000, replace=False),
           "boost": rng.choice(V, 3000, replace=False), "ground": rng.choice(V, 6000, replace=False)}
    sou = rng.randint(0, V + 100, size=(2, L)).astype(np.int32)
    sub = rng.randint(-3, V, size=(2, S)).astype(np.int32)
    sou[:, :40] = ids["ground"][:40]                           # grounded words in slots, valid and invalid
    valid = rng.randint(0, 1 << 32, size=(2, NS // 32), dtype=np.uint64).astype(np.uint32)
    gen = rng.randint(3, V, size=(R, T)).astype(np.int32)
    gen[:, 0] = START
    gen[1, 20] = EOS
    case = dict(dims=(V, L, S), rpc=rpc, R=R, T=T, gen=gen, length=np.array([1, 21, 64, 40], dtype=np.int32), sou=sou, sub=sub,
                valid=valid, sets={k: WordSets.pack([v, v[::2]], V) for k, v in ids.items()},
                factor=np.array([0.5, 2.0], dtype=np.float32), dist=rng.uniform(1e-6, 1.0, size=(R, V + NS)).astype(np.float32),
                zero_rows=[])
    ref = reference(case, SETS)
    blk, up = ref[2], ref[3]
    assert not blk[1].any() and all(0 < blk[r].sum() < blk[r].size and up[r].any() for r in (0, 2, 3))
    assert blk[0, V:].any() and not blk[0, V:].all()
    equals_the_reference(case, SETS, ref, offsets=(1,))


def test_refusals_return_non_zero_with_a_message():
    lib, p = _lib.lib(), C.c_void_p(16)
    for geo, R, rpc, tail, word in ((dict(tar_len=4), 6, 3, (None, None, None, p, None, None), "slot_valid, which ground needs"),
                                    (dict(tar_len=4), 6, 3, (None, None, p, None, None, None), "boost_factor, which boost needs"),
                                    (dict(tar_len=65), 6, 3, (p, None, None, None, None, None), "tar_len = 65"),
                                    (dict(tar_len=4), 6, 4, (p, None, None, None, None, None), "rows_per_commit = 4")):
        dd = device_dims(37, 5, 3, **geo)
        assert lib.fira_wordset_dist(_lib.cur_stream(), C.byref(dd), R, rpc, p, p, p, p, *tail, p, None, None) != 0
        msg = lib.fira_last_error().decode()
        assert "fira_wordset_dist" in msg and word in msg, msg
    dd = device_dims(37, 5, 3, 4)
    assert lib.fira_wordset_dist(_lib.cur_stream(), C.byref(dd), 6, 3, p, p, p, p, p, None, None, None, None, None, p, p, None) != 0
    assert "best_id and best_p" in lib.fira_last_error().decode()
    assert lib.fira_wordset_dist(_lib.cur_stream(), C.byref(dd), 0, 3, *([None] * 11), None, None) == 0      # R == 0: a no-op
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ through the model
MODEL_TAR_LEN = 8                                              # test_require_gpu.py says why: raw products stay positive in fp32


@pytest.fixture(scope="module")
def setup():
    g = golden_search(tar_len=MODEL_TAR_LEN, weights="spread", searchers=3)
    return g.cfg, g.model, g.db, g.searchers


@pytest.fixture(scope="module")
def plain(setup):
    cfg, model, db, (search, _, _) = setup
    keep = lambda res: [t.cpu().clone() for t in res]
    return dict(greedy=keep(search.greedy(db)), beam3=keep(search.beam(db, 3)), sample3=keep(search.sample_search(db, 3, seed=5)),
                greedy_m=keep(search.greedy(db, merge_copies=True)), beam3_m=keep(search.beam(db, 3, merge_copies=True)),
                sample3_m=keep(search.sample_search(db, 3, seed=5, merge_copies=True)))


def seen_words(plain, key="greedy"):
    return sorted({w for msg in messages(plain[key][0], plain[key][1]) for w in msg if w > UNK})


def test_deny_is_the_ban(setup, plain):
    cfg, model, db, (search, _, _) = setup
    banned = seen_words(plain)[:32]
    assert 3 <= len(banned) <= 32
    con, deny = Constraints(banned=banned), WordSets(deny=banned)
    want = search.greedy(db, constraints=con)
    same_search(search.greedy(db, wordsets=deny), want)
    assert messages(*want[:2]) != messages(*plain["greedy"][:2])
    same_search(search.beam(db, 3, wordsets=deny), search.beam(db, 3, constraints=con))
    per_commit = WordSets(deny=[banned] * db.B)                # one list per commit, the same result
    same_search(search.beam(db, 3, wordsets=per_commit), search.beam(db, 3, constraints=con))


@pytest.mark.parametrize("b", [-2.0, 1.0])
def test_boost_of_one_word_is_the_bias(setup, plain, b):
    cfg, model, db, (search, _, _) = setup
    w = seen_words(plain)[0]
    pen, boost = Penalties(bias={w: b}), WordSets(boost={w}, boost_bias=b)
    same_search(search.greedy(db, wordsets=boost), search.greedy(db, penalties=pen))
    same_search(search.beam(db, 3, wordsets=boost), search.beam(db, 3, penalties=pen))
    got, want = search.sample_search(db, 3, seed=5, wordsets=boost), search.sample_search(db, 3, seed=5, penalties=pen)
    same_search(got, want)
    assert torch.equal(bits(got[3].cpu()), bits(want[3].cpu()))
    if b < 0:
        assert messages(*search.greedy(db, wordsets=boost)[:2]) != messages(*plain["greedy"][:2])


def test_sets_that_block_nothing_are_the_plain_search(setup, plain):
    cfg, model, db, (search, _, _) = setup
    every = [EOS] + list(range(UNK, cfg.vocab_size))
    nothing = WordSets(allow=every, deny=[], boost=every, boost_bias=0.0)
    assert nothing.given == ("allow",)
    same_search(search.greedy(db, wordsets=nothing), plain["greedy"])
    assert ("greedy", db.B, ("wordsets", ("allow",))) in search._ws
    same_search(search.beam(db, 3, wordsets=nothing), plain["beam3"])
    got = search.sample_search(db, 3, seed=5, wordsets=nothing)
    same_search(got, plain["sample3"])
    assert torch.equal(bits(got[3].cpu()), bits(plain["sample3"][3]))
    same_search(search.beam(db, 3, wordsets=nothing, use_graphs=False), plain["beam3"])
    unit = WordSets(boost=[[w] for w in seen_words(plain)[:1]] * db.B, boost_bias=[1e-30] * db.B)      # a factor of exactly 1.0f
    assert unit.given == ("boost",) and unit.arrays(db.B, cfg.vocab_size)["boost_factor"].tolist() == [1.0] * db.B
    same_search(search.greedy(db, wordsets=unit), plain["greedy"])


def test_greedy_many_is_greedy_batch_by_batch(setup, plain):
    cfg, model, db, (search, _, _) = setup
    words = seen_words(plain)
    a, b = WordSets(deny=words[:5]), WordSets(deny=words[5:9], ground=range(4, cfg.vocab_size))
    want_a, want_b = search.greedy(db, wordsets=a), search.greedy(db, wordsets=b)
    for res in search.greedy_many([db, db], in_flight=2, wordsets=a):
        same_search(res, want_a)
    got = search.greedy_many([db, db], in_flight=2, wordsets=[a, b])
    same_search(got[0], want_a)
    same_search(got[1], want_b)
    got = search.greedy_many([db, db], in_flight=2, wordsets=[None, b])
    same_search(got[0], plain["greedy"])
    same_search(got[1], want_b)


def carried_by(db):
    """The words each commit carries, from the batch arrays: the source ids of its valid (non-<pad>) copy slots."""
    ids = torch.cat([db.sou, db.sub_token], 1).cpu().numpy()
    return [set(int(w) for w in row if w != PAD) for row in ids]


def test_under_ground_every_written_word_is_carried(setup, plain):
    cfg, model, db, (search, _, _) = setup
    ground = WordSets(ground=range(4, cfg.vocab_size))
    carried = carried_by(db)
    runs = {"greedy_m": lambda: search.greedy(db, merge_copies=True, wordsets=ground),
            "beam3_m": lambda: search.beam(db, 3, merge_copies=True, wordsets=ground),
            "sample3_m": lambda: search.sample_search(db, 3, seed=5, merge_copies=True, wordsets=ground)}
    for name, run in runs.items():
        gen, length, prob = [x.cpu() for x in run()[:3]]
        gen, length, prob = gen.reshape(db.B, -1, cfg.tar_len), length.reshape(db.B, -1), prob.reshape(db.B, -1)
        n_positive = 0
        for b in range(db.B):
            for j in range(gen.shape[1]):
                if float(prob[b, j]) > 0:
                    msg = gen[b, j, 1:int(length[b, j])].tolist()
                    assert all(w == EOS or w in carried[b] for w in msg), (name, b, j, msg)
                    n_positive += 1
        assert n_positive >= 1, name
        base = plain[name]
        differs = [b for b in range(db.B) if messages(gen[b], length[b]) != messages(base[0].reshape(gen.shape)[b],
                                                                                    base[1].reshape(length.shape)[b])]
        assert differs, name                                   # not vacuous: the plain search writes words no diff carries


def test_two_values_replay_one_captured_graph(setup, plain, monkeypatch):
    cfg, model, db, (search, fresh1, fresh2) = setup
    words = seen_words(plain, "beam3")
    w1 = WordSets(deny=words[:4], ground=range(4, cfg.vocab_size))
    w2 = WordSets(deny=[words[4:6]] * db.B, ground=[w for w in range(4, cfg.vocab_size) if w % 2])
    assert w1.given == w2.given == ("deny", "ground")
    want1, want2 = fresh1.beam(db, 3, wordsets=w1), fresh2.beam(db, 3, wordsets=w2)
    assert messages(*want1[:2]) != messages(*want2[:2])
    keys = set(search._ws)
    first = search.beam(db, 3, wordsets=w1)
    key = ("beam", db.B, 3, ("wordsets", ("deny", "ground")))
    assert key in search._ws and set(search._ws) - keys <= {key}
    n_states, graphs = len(search._ws), list(search._ws[key]["graphs"])
    monkeypatch.setattr(torch.cuda, "graph", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a second capture")))
    got = {}
    calls = count_calls(monkeypatch, lambda: got.update(res=search.beam(db, 3, wordsets=w2)))
    assert set(calls) == {"fira_decode_begin_ex"} and len(search._ws) == n_states and search._ws[key]["graphs"] == graphs
    same_search(first, want1)
    same_search(got["res"], want2)
    same_search(search.beam(db, 3, wordsets=w1), want1)        # and back: the same graphs, the first result


def test_off_is_todays_search_call_for_call(setup, plain, monkeypatch):
    cfg, model, db, _ = setup
    fresh = Searcher(model)
    runs = {"beam": lambda **k: fresh.beam(db, 3, use_graphs=False, **k), "greedy": lambda **k: fresh.greedy(db, use_graphs=False, **k),
            "sample_search": lambda **k: fresh.sample_search(db, 2, seed=3, use_graphs=False, **k)}
    for name, run in runs.items():
        base = {}
        run()                                                  # (the first call alone sizes the workspace)
        calls = count_calls(monkeypatch, lambda: base.update(res=run()))
        keys = set(fresh._ws)
        for off in (None, WordSets()):
            got = {}
            assert count_calls(monkeypatch, lambda: got.update(res=run(wordsets=off))) == calls, (name, off)
            assert len(got["res"]) == len(base["res"]) and set(fresh._ws) == keys
            for a, b in zip(got["res"], base["res"]):
                assert torch.equal(bits(a), bits(b)), (name, off)
        assert "fira_wordset_dist" not in calls
        with_w = count_calls(monkeypatch, lambda: run(wordsets=WordSets(deny=[5])))
        assert with_w.get("fira_wordset_dist", 0) > 0          # one launch per step on top


# ------------------------------------------------------------------------------------------------ scripts/wordset_probe.py
def test_the_probe_decodes_and_counts_no_violation(tmp_path):
    import json
    import os
    import re
    import subprocess
    import sys

    import util
    from search_kit import spread_state_dict
    from fira_icse_amd import synth
    from fira_icse_amd.config import FiraConfig
    root = str(tmp_path)
    synth.write_dataset(root, util.load_golden_raw())
    torch.manual_seed(0)
    torch.save(spread_state_dict(FiraConfig()), os.path.join(root, "best_model.pt"))
    vocab = json.load(open(os.path.join(root, "DataSet", "word_vocab.json")))
    words = sorted(w for w in vocab if re.fullmatch(r"w\d+", w))[:3]
    with open(os.path.join(root, "deny.txt"), "w") as f:
        f.write("\n".join(words + ["nosuchword"]) + "\n")
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "scripts", "wordset_probe.py"), "--root", root, "--splits", "16,4,4",
                        "--test-batch-size", "4", "--beam", "3", "--ground-identifiers", "--deny-file", os.path.join(root, "deny.txt"),
                        "--boost-diff", "1.0", "--reps", "0"], cwd=root, env=dict(os.environ, PYTHONPATH=util.REPO),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = open(os.path.join(root, "OUTPUT", "output_fira_wordsets")).read().split("\n")[:-1]
    assert len(lines) == 4
    m = re.search(r"(\d+) of the (\d+) written words of (\d+) messages of positive probability violate the sets", r.stdout)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) >= 1 and int(m.group(3)) >= 1, r.stdout
    assert "warning: 4 words the vocabulary lacks" in r.stderr                 # the unknown word, once per commit
