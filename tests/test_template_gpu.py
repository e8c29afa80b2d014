"""Template-constrained search on the device: fira_template_dist on synthetic rows against the numpy statement (template_ref.py),
its three anchors through the golden model (the accept-everything template is the plain search, a "w1 w2 then anything" template
is ``prefix=``, a one-class-banned template is ``Constraints(banned=)``), and the property the feature exists for: every message
a search returns with positive probability is one the automaton accepts."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import template_ref as TR
import util
from search_kit import best_pair, bits, count_calls, device_dims, golden_search, messages, offset_rows, outside_untouched, same_search
from test_template import HAND_ACCEPT, HAND_CLASS, HAND_NEXT, hand_template, host_refusals, no_launch
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, START, UNK
from fira_icse_amd.decode import Constraints, Searcher, Template

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the kernel alone
T_ROWS = 8
EVERY = "every"
# (hypothesis, start state, the words that stay free) under test_template.py's automaton; three rows per commit share a start
ROWS = [([START], 0, {4, 5}),                                  # m = 0: a type word or nothing
        ([START, 6], 0, set()),                                # the walk dies: the whole row, the arg-max reports entry 0 with 0
        ([START, 4, 6, 9, EOS], 0, EVERY),                     # finished: untouched
        ([START, 4, 8, 8, 8, 8, 6], 0, "no 7, no eos"),        # len = T - 1 in state 3: only transitions into the accepting state
        ([START, 4, 8, 8, 8, 8], 0, {6}),                      # left = 1 in state 2: staying needs 2 words, the colon 1 -- need cuts
        ([START, 4, 6], 0, "no 7, no eos"),                    # state 3 does not accept: the diff slot that carries <eos> goes too
        ([START], 3, "no 7, no eos"),                          # another start state
        ([START, 9], 3, "no 7"),                               # the accepting state: <eos> is free
        ([START, 9, 9, 9, 9, 9, 9, 9], 3, {EOS})]              # len = T: left = -1, nothing fits but the end
GEOMETRIES = [("no-sub-x1", (37, 5, 0), 1), ("no-sub-x3", (37, 5, 0), 3), ("small-x1", (37, 5, 3), 1), ("small-x3", (37, 5, 3), 3)]


def free_words(spec, V):
    every = set(range(V))
    return {EVERY: every, "no 7, no eos": every - {7, EOS}, "no 7": every - {7}}.get(spec, spec) if isinstance(spec, str) else spec


def case_of(dims, rpc, rows=ROWS, T=T_ROWS, template=None, seed=7):
    V, L, S = dims
    n_rows, n_commits = len(rows), len(rows) // rpc
    rng = np.random.RandomState(seed + rpc + S)
    gen = rng.choice((5, 6, 9, EOS, 0), size=(n_rows, T)).astype(np.int32)           # (what stays past the length is junk)
    length = np.zeros(n_rows, dtype=np.int32)
    for r, (row, _, _) in enumerate(rows):
        gen[r, :len(row)] = row
        length[r] = len(row)
    sou = np.tile(np.resize(np.array([4, 6, EOS, 7, 8], dtype=np.int32), L), (n_commits, 1))      # diff slots carry the words
    sub = np.tile(np.resize(np.array([7, 6, 8], dtype=np.int32), max(S, 1)), (n_commits, 1))      # ... and sub-token slots
    start = [rows[b * rpc][1] for b in range(n_commits)]
    assert all(rows[r][1] == start[r // rpc] for r in range(n_rows))
    template = hand_template(start) if template is None else template
    wc, nxt, need, st = template.arrays(n_commits, V)
    dist = rng.uniform(1e-6, 1.0, size=(n_rows, V + L + S)).astype(np.float32)
    return dict(dims=dims, rpc=rpc, R=n_rows, T=T, gen=gen, length=length, sou=sou, sub=sub, wc=wc, nxt=nxt, need=need, start=st,
                dist=dist)


def reference(case):
    """(mask, dist, edited, best_id, best_p): an exact tie on two free entries and an overtowering blocked entry built in."""
    rpc, S = case["rpc"], case["dims"][2]
    mask = np.stack([TR.template_mask(case["gen"][r], case["length"][r], case["sou"][r // rpc], case["sub"][r // rpc][:S],
                                      case["dims"], case["wc"], case["nxt"], case["need"], case["start"][r // rpc])
                     for r in range(case["R"])])
    dist = case["dist"].copy()
    for r in range(case["R"]):
        free, blk = np.flatnonzero(~mask[r]), np.flatnonzero(mask[r])
        if len(free):
            dist[r, free[len(free) // 3]] = dist[r, free[-1]] = np.float32(2.0)
        if len(blk):
            dist[r, blk] = np.float32(3.0)
    out = np.where(mask, np.float32(0.0), dist)
    best = [TR.argmax_ref(out[r]) for r in range(case["R"])]
    return mask, dist, out, np.array([b[0] for b in best], dtype=np.int32), np.array([b[1] for b in best], dtype=np.float32)


GUARD = 5                                                      # odd: word_class then starts at an odd byte address


def guarded(a, fill):
    """``a`` on the device with GUARD elements of ``fill`` on either side; returns (buffer, pointer to the table)."""
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    buf = torch.full((GUARD + flat.numel() + GUARD,), fill, dtype=flat.dtype, device="cuda")
    buf[GUARD:GUARD + flat.numel()] = flat.to("cuda")
    return buf, C.c_void_p(buf.data_ptr() + GUARD * flat.element_size())


def run_kernel(case, dist, want_best, offset):
    n_rows, W = dist.shape
    buf, d_dev = offset_rows(dist, offset)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    gen, length, sou, sub = t(case["gen"]), t(case["length"]), t(case["sou"]), t(case["sub"])
    # guards around every table: a class byte of 31 / a target of 9 / a need of 0 read by mistake would change the result
    tables = [guarded(case["wc"], 31), guarded(case["nxt"], 9), guarded(case["need"], 0), guarded(case["start"], 4)]
    assert tables[0][1].value % 2 == 1
    best_id, best_p = best_pair(n_rows, want_best)
    dd = device_dims(*case["dims"], case["T"])
    _lib.check(_lib.lib().fira_template_dist(_lib.cur_stream(), C.byref(dd), n_rows, case["rpc"], _lib.ptr(gen), _lib.ptr(length),
                                             _lib.ptr(sou), _lib.ptr(sub), *[p for _, p in tables], _lib.ptr(d_dev),
                                             _lib.ptr(best_id), _lib.ptr(best_p)), "fira_template_dist")
    torch.cuda.synchronize()
    outside_untouched(buf, offset, n_rows * W)
    for (b, _), fill in zip(tables, (31, 9, 0, 4)):
        assert bool((b[:GUARD] == fill).all()) and bool((b[-GUARD:] == fill).all())
    return d_dev.cpu(), None if best_id is None else best_id.cpu(), None if best_p is None else best_p.cpu()


def equals_the_reference(case, ref, offsets=(0, 1, 2, 3), tag=None):
    mask, dist, out, best_id, best_p = ref
    for want_best in (True, False):                            # (without best the row is never read: the other code path)
        for offset in offsets:
            got, gid, gp = run_kernel(case, dist, want_best, offset)
            assert torch.equal(bits(got), bits(out)), (tag, want_best, offset)
            if want_best:
                assert gid.tolist() == best_id.tolist(), (tag, offset)
                assert torch.equal(bits(gp), bits(best_p)), (tag, offset)


@pytest.mark.parametrize("name, dims, rpc", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_kernel_equals_the_reference_bit_for_bit(name, dims, rpc):
    V, L, S = dims
    case = case_of(dims, rpc)
    ref = reference(case)
    mask, _, out, best_id, best_p = ref
    words = np.concatenate([np.arange(V), case["sou"][0], case["sub"][0][:S]])
    for r, (_, _, spec) in enumerate(ROWS):                    # the inputs say what the comments claim
        free = free_words(spec, V)
        assert set(words[~mask[r]].tolist()) == free, (r, spec)
        assert (~mask[r, words == EOS]).all() == (EOS in free) and mask[r, V:V + L].any() == (spec != EVERY)
    assert mask[1].all() and best_id[1] == 0 and best_p[1] == 0                      # the dead row: entry 0 with value 0
    assert mask[5, V + 2] and case["sou"][0][2] == EOS                              # <eos> carried by a diff slot
    equals_the_reference(case, ref, tag=name)


def full_table():
    """32 states, 32 classes: next[s][c] = (s + c) % 32 with holes; the class of word w is w % 32."""
    nxt = [[-1 if (s * c) % 11 == 7 else (s + c) % 32 for c in range(32)] for s in range(32)]
    return nxt, [s for s in range(32) if s % 3 == 0]


def test_kernel_with_the_full_table():
    dims = (70, 5, 3)
    nxt, accept = full_table()
    t = Template([w % 32 for w in range(dims[0])], nxt, accept)
    # <start> 31 visits class 31 and state 31; the next words go on from there
    rows = [([START, 31], 0, None), ([START, 31, 35], 0, None), ([START, 31, 35, 64 + 5, 41], 0, None)]
    assert t.walk([31], 0) == 31 and t.walk([31, 35], 0) == 2 and t.walk([31, 35, 69, 41], 0) == 16
    case = case_of(dims, 3, rows, template=t)
    ref = reference(case)
    assert all(0 < ref[0][r].sum() < ref[0][r].size for r in range(3))
    equals_the_reference(case, ref, offsets=(0, 3))


def test_kernel_at_the_models_geometry():
    dims, T = (24650, 210, 160), 30
    V = dims[0]                                                # 770 * 32 + 10: the last word of the class table holds 10 ids
    t = Template({**HAND_CLASS, V - 1: 3, V - 2: 2, V - 11: 3, 31: 3, 32: 1}, HAND_NEXT, HAND_ACCEPT, [0, 3])
    rows = [([START], 0, None), ([START, 4, V - 2], 0, None), ([START, 32, 9, 9, 9, 9], 0, None),
            ([START, 5] + [12] * 27 + [6], 3, None), ([START, V - 1], 3, None), ([START, 9, 9, EOS], 3, None)]
    case = case_of(dims, 3, rows, T=T, template=t)
    ref = reference(case)
    mask = ref[0]
    assert mask[1, V - 1] and mask[1, V - 11] and not mask[1, V - 2] and not mask[1, V - 3] and mask[1, 31] and not mask[1, 32]
    assert mask[4].all() and not mask[5].any() and set(np.flatnonzero(~mask[0, :V])) == {4, 5, 32}
    equals_the_reference(case, ref, offsets=(1,))


def test_the_accept_everything_template_leaves_the_rows_alone():
    case = case_of((37, 5, 3), 3, ROWS[:6], template=Template({}, [[0]], [0]))
    ref = reference(case)
    assert not ref[0].any()
    equals_the_reference(case, ref, offsets=(1,))


def test_refusals_return_non_zero_with_a_message():
    lib, p = _lib.lib(), C.c_void_p(16)
    for geo, R, rpc, tables, word in ((dict(tar_len=8), 6, 3, (p, None, p, p), "null pointer (word_class, next, need or start)"),
                                      (dict(tar_len=65), 6, 3, (p, p, p, p), "tar_len = 65"),
                                      (dict(tar_len=8), 6, 4, (p, p, p, p), "rows_per_commit = 4")):
        dd = device_dims(37, 5, 3, **geo)
        assert lib.fira_template_dist(_lib.cur_stream(), C.byref(dd), R, rpc, p, p, p, p, *tables, p, None, None) != 0
        msg = lib.fira_last_error().decode()
        assert "fira_template_dist" in msg and word in msg, msg
    dd = device_dims(37, 5, 3, 8)
    assert lib.fira_template_dist(_lib.cur_stream(), C.byref(dd), 0, 3, *([None] * 9), None, None) == 0      # R == 0: a no-op
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ through the model
MODEL_TAR_LEN = 8                                              # test_require_gpu.py says why: raw products stay positive in fp32
EVERYTHING = Template({}, [[0]], [0])


@pytest.fixture(scope="module")
def setup():
    g = golden_search(tar_len=MODEL_TAR_LEN, weights="spread")
    return g.cfg, g.model, g.db, g.searchers[0]


@pytest.fixture(scope="module")
def plain(setup):
    cfg, model, db, search = setup
    keep = lambda res: [t.cpu().clone() for t in res]
    return dict(greedy=keep(search.greedy(db)), beam3=keep(search.beam(db, 3)), beam5=keep(search.beam(db, 5)),
                sample3=keep(search.sample_search(db, 3, seed=5)), sample4=keep(search.sample_search(db, 4, seed=5)))


def test_the_accept_everything_template_is_the_plain_search(setup, plain):
    cfg, model, db, search = setup
    same_search(search.greedy(db, template=EVERYTHING), plain["greedy"])
    assert ("greedy", db.B, "template") in search._ws
    for res in search.greedy_many([db, db], in_flight=2, template=EVERYTHING):
        same_search(res, plain["greedy"])
    same_search(search.beam(db, 3, template=EVERYTHING), plain["beam3"])
    got = search.sample_search(db, 3, seed=5, template=EVERYTHING)
    same_search(got, plain["sample3"])
    assert torch.equal(bits(got[3].cpu()), bits(plain["sample3"][3]))
    same_search(search.beam(db, 3, template=EVERYTHING, use_graphs=False), plain["beam3"])


def two_words_then_anything(pairs):
    """One union automaton for the batch: state 0 takes everything and accepts; commit b starts in a chain that admits exactly
    its two words first.  One class per distinct word."""
    classes = {w: k + 1 for k, w in enumerate(sorted(set(w for pair in pairs for w in pair)))}
    n = len(classes) + 1
    nxt, start = [[0] * n], []
    for pair in pairs:
        state = 0
        for w in reversed(pair):                               # the chain is built from its end
            nxt.append([state if c == classes[w] else -1 for c in range(n)])
            state = len(nxt) - 1
        start.append(state)
    return Template(classes, nxt, [0], start)


def test_two_words_then_anything_is_the_prefix_search(setup, plain):
    cfg, model, db, search = setup
    pairs = []
    for msg in messages(plain["greedy"][0], plain["greedy"][1]):
        head = msg[:2]
        pairs.append(head if len(head) == 2 and min(head) >= UNK else [])
    assert sum(1 for p in pairs if p) >= 2
    pairs = pairs[1:] + pairs[:1]                              # every commit gets another commit's opening
    t = two_words_then_anything(pairs)
    for b, p in enumerate(pairs):
        assert t.accepts(p + [77], b) and (not p or 77 in p or not t.accepts([77] + p, b))
    same_search(search.greedy(db, template=t), search.greedy(db, prefix=pairs))
    same_search(search.beam(db, 3, template=t), search.beam(db, 3, prefix=pairs))
    assert messages(*search.greedy(db, template=t)[:2]) != messages(*plain["greedy"][:2])


def test_one_class_without_a_transition_is_the_ban(setup, plain):
    cfg, model, db, search = setup
    seen = [w for msg in messages(plain["greedy"][0], plain["greedy"][1]) for w in msg if w >= UNK]
    banned = sorted(set(seen))[:6]
    assert len(banned) >= 3
    t = Template({w: 1 for w in banned}, [[0, -1]], [0])
    con = Constraints(banned=banned)
    want = search.greedy(db, constraints=con)
    same_search(search.greedy(db, template=t), want)
    assert messages(*want[:2]) != messages(*plain["greedy"][:2])
    same_search(search.beam(db, 3, template=t), search.beam(db, 3, constraints=con))
    same_search(search.beam(db, 3, template=t, constraints=con), search.beam(db, 3, constraints=con))      # zeroing links commute


def conventional(plain, V, tail):
    """A conventional-commit template whose type words no plain search opens with."""
    msgs = [msg for k in sorted(plain) for msg in messages(plain[k][0], plain[k][1])]
    opened = {msg[0] for msg in msgs if msg}
    # words the model does emit, but never first (so they have probability to spare); then any other ids
    later = [w for w in dict.fromkeys(w for msg in msgs for w in msg[1:]) if w > UNK and w not in opened]
    words = (later + [w for w in range(40, 60) if w not in opened and w not in later])[:4]
    types_, colon = words[:3], words[3]
    assert len(words) == 4 and not opened & set(words)
    return Template.sequence([(types_, 1, 1), (None, 0, 1), ({colon}, 1, 1), tail], V), set(types_), colon


@pytest.mark.parametrize("tail", [(None, 1, None), (None, 1, 3)], ids=["open", "need-cuts"])
def test_every_returned_message_is_accepted(setup, plain, tail):
    cfg, model, db, search = setup
    t, types_, colon = conventional(plain, cfg.vocab_size, tail)
    runs = {"greedy": (lambda: search.greedy(db, template=t), plain["greedy"]),
            "beam5": (lambda: search.beam(db, 5, template=t), plain["beam5"]),
            "sample4": (lambda: search.sample_search(db, 4, seed=5, template=t), plain["sample4"])}
    for name, (run, base) in runs.items():
        gen, length, prob = [x.cpu() for x in run()[:3]]
        gen, length, prob = gen.reshape(db.B, -1, cfg.tar_len), length.reshape(db.B, -1), prob.reshape(db.B, -1)
        n_positive = 0
        for b in range(db.B):
            for j in range(gen.shape[1]):
                if float(prob[b, j]) > 0:
                    msg = gen[b, j, 1:int(length[b, j])].tolist()
                    assert t.accepts(msg, b), (name, b, j, msg)
                    assert msg[0] in types_ and colon in msg[1:3], (name, msg)
                    assert tail[2] is None or len([w for w in msg if w != EOS]) <= 6
                    n_positive += 1
        assert n_positive >= db.B, (name, n_positive)          # not vacuous: every commit has a message ...
        assert messages(gen, length) != messages(base[0], base[1])         # ... and it is not the plain search's


def test_two_templates_replay_one_captured_graph(setup, plain, monkeypatch):
    cfg, model, db, search = setup
    t1, _, _ = conventional(plain, cfg.vocab_size, (None, 1, None))
    keys = set(search._ws)
    first = search.beam(db, 3, template=t1)
    key = ("beam", db.B, 3, "template")
    assert key in search._ws and set(search._ws) - keys <= {key}
    n_states, graphs = len(search._ws), list(search._ws[key]["graphs"])
    monkeypatch.setattr(torch.cuda, "graph", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a second capture")))
    other = hand_template([0, 3, 0, 3][:db.B] + [0] * max(db.B - 4, 0))
    got = {}
    calls = count_calls(monkeypatch, lambda: got.update(res=search.beam(db, 3, template=other)))
    assert set(calls) == {"fira_decode_begin_ex"} and len(search._ws) == n_states and search._ws[key]["graphs"] == graphs
    gen, length, prob = [x.cpu() for x in got["res"]]
    for b in range(db.B):
        for j in range(3):
            if float(prob[b, j]) > 0:
                assert other.accepts(gen[b, j, 1:int(length[b, j])].tolist(), b)
    assert messages(gen, length) != messages(first[0], first[1])
    same_search(search.beam(db, 3, template=t1), first)        # and back: the same graphs, the first result


def test_off_is_todays_search_call_for_call(setup, plain, monkeypatch):
    cfg, model, db, search = setup
    fresh = Searcher(model)
    runs = {"beam": lambda **k: fresh.beam(db, 3, use_graphs=False, **k), "greedy": lambda **k: fresh.greedy(db, use_graphs=False, **k),
            "sample_search": lambda **k: fresh.sample_search(db, 2, seed=3, use_graphs=False, **k)}
    for name, run in runs.items():
        base = {}
        run()                                                  # (the first call alone sizes the workspace)
        calls = count_calls(monkeypatch, lambda: base.update(res=run()))
        keys = set(fresh._ws)
        for off in (None, Template()):
            got = {}
            assert count_calls(monkeypatch, lambda: got.update(res=run(template=off))) == calls, (name, off)
            assert len(got["res"]) == len(base["res"]) and set(fresh._ws) == keys
            for a, b in zip(got["res"], base["res"]):
                assert torch.equal(bits(a), bits(b)), (name, off)
        assert "fira_template_dist" not in calls
        with_t = count_calls(monkeypatch, lambda: run(template=EVERYTHING))
        assert with_t.get("fira_template_dist", 0) > 0         # one launch per step on top


def test_every_host_refusal_comes_before_any_library_call(monkeypatch):
    s = no_launch()

    def reaches_device(run):
        with pytest.raises(AssertionError, match="device work"):
            run()
    calls = count_calls(monkeypatch, lambda: host_refusals(s, types.SimpleNamespace(B=2), reaches_device))
    assert calls == {} and s._ws == {}


# ------------------------------------------------------------------------------------------------ scripts/template_probe.py
def test_the_probe_decodes_and_reports_every_message_accepted(tmp_path):
    from fira_icse_amd import synth
    from fira_icse_amd.config import FiraConfig
    root = str(tmp_path)
    synth.write_dataset(root, util.load_golden_raw())
    torch.manual_seed(0)
    from search_kit import spread_state_dict
    torch.save(spread_state_dict(FiraConfig()), os.path.join(root, "best_model.pt"))
    words = sorted(w for w in synth_words(root))[:3]
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "scripts", "template_probe.py"), "--root", root, "--splits", "16,4,4",
                        "--test-batch-size", "4", "--beam", "3", "--types", ",".join(words[:2]) + ",nosuchword", "--colon", words[2],
                        "--max-words", "6", "--reps", "0"], cwd=root, env=dict(os.environ, PYTHONPATH=util.REPO),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = open(os.path.join(root, "OUTPUT", "output_fira_template")).read().split("\n")[:-1]
    assert len(lines) == 4
    import re
    m = re.search(r"the automaton accepts (\d+) of (\d+) messages of positive probability", r.stdout)
    assert m and m.group(1) == m.group(2) and int(m.group(2)) >= 1, r.stdout
    assert "warning: 4 type words" in r.stderr                 # the unknown type word, once per commit
    shaped = [l for l in lines if l.split()[0] in words[:2] and words[2] in l.split()[1:3]]
    assert len(shaped) >= int(m.group(2)), lines               # the written messages open as the template says


def synth_words(root):
    """The plain words of the synthetic vocabulary a run directory was written with."""
    import json
    import re
    vocab = json.load(open(os.path.join(root, "DataSet", "word_vocab.json")))
    return [w for w in vocab if re.fullmatch(r"w\d+", w)]
