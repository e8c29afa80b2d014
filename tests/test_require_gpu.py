"""fira_beam_select_required on synthetic states -- against fira_beam_select (bit identity without required words) and against
the numpy statement require_ref.py (every output equal: the products are fp32 multiplies on both sides) -- and the search
with required words through the model."""
import ctypes as C

import numpy as np
import pytest
import torch

import require_ref as R
from search_kit import bits, device_dims, golden_search
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, START, UNK

pytestmark = pytest.mark.gpu

SMALL = dict(vocab=11, sou_len=5, sub_len=2, tar_len=8)            # W = 18
SMALL_ODD = dict(vocab=11, sou_len=5, sub_len=3, tar_len=8)        # W = 19: odd, rows at every 4-byte alignment
MODEL = {}                                                          # the model's geometry (FiraConfig's own dims)


def geometry(geo):
    d = device_dims(**geo)
    return d.vocab, d.sou_len, d.sub_len, d.tar_len


def make_state(rng, geo, B, beam, n_required, finished=0.3, inactive_slot=None, max_len=None, zero_prob=0.15, words_hi=None):
    """A consistent search state as fira_beam_prepare leaves it (hypotheses <start> w .. [<eos>], active[j] = some commit still
    runs in slot j), with ``n_required[b]`` distinct required words per commit.  The hypotheses and the copy slots draw from
    the low ids, so they hold required words often."""
    V, L, S, T = geometry(geo)
    hi = words_hi or min(V, 11)
    max_len = max_len or T - 2
    gen = np.zeros((B, beam, T), dtype=np.int32)
    length = rng.randint(1, max_len + 1, size=(B, beam)).astype(np.int32)
    fin = np.zeros((B, beam), dtype=np.int32)
    for b in range(B):
        for j in range(beam):
            n = length[b, j]
            gen[b, j, 0] = START
            gen[b, j, 1:n] = rng.randint(3, hi, size=n - 1)
            if n >= 2 and (rng.rand() < finished or j == inactive_slot):
                gen[b, j, n - 1] = EOS
                fin[b, j] = 1
            elif j == inactive_slot:                               # (a one-id hypothesis cannot be finished: make it two)
                length[b, j] = 2
                gen[b, j, 1] = EOS
                fin[b, j] = 1
    prob = rng.uniform(0.05, 1.0, size=(B, beam)).astype(np.float32)
    prob[rng.rand(B, beam) < zero_prob] = 0.0
    active = np.zeros(9, dtype=np.int32)
    active[:beam] = (fin == 0).any(0)
    active[8] = active[:beam].sum()
    sou = rng.randint(1, hi, size=(B, L)).astype(np.int32)         # id 1: a copy slot may carry <eos>
    sub = rng.randint(3, hi, size=(B, S)).astype(np.int32)
    required = np.zeros((B, 4), dtype=np.int32)
    for b in range(B):
        required[b] = rng.permutation(np.arange(UNK + 1, hi))[:4]  # all four places hold words: the count alone decides
    return dict(geo=geo, B=B, beam=beam, gen=gen, length=length, fin=fin, prob=prob, active=active, sou=sou, sub=sub, done=0,
                required=required, n_required=np.asarray(n_required, dtype=np.int32))


def random_dist(rng, st, zeros=0.2):
    V, L, S, T = geometry(st["geo"])
    dist = rng.uniform(1e-6, 1.0, size=(st["B"], st["beam"], V + L + S)).astype(np.float32)
    dist[rng.rand(*dist.shape) < zeros] = 0.0                      # what the constraint kernels leave behind
    return dist


def launch(st, dist, required=True, want_met=True):
    dev = "cuda"
    B, beam = st["B"], st["beam"]
    V, L, S, T = geometry(st["geo"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gen, length, prob, fin, active = t(st["gen"].reshape(B * beam, T)), t(st["length"].reshape(-1)), t(st["prob"].reshape(-1)), \
        t(st["fin"].reshape(-1)), t(st["active"])
    done = torch.tensor([st["done"]], dtype=torch.int32, device=dev)
    sou, sub, dist_d = t(st["sou"]), t(st["sub"]), t(dist.reshape(B * beam, -1))
    g_out = torch.full_like(gen, -7)
    l_out, p_out, parent = torch.full_like(length, -7), torch.full_like(prob, -7.0), torch.full_like(length, -7)
    met = torch.full_like(length, -7) if required and want_met else None
    dd = device_dims(**st["geo"])
    args = (_lib.cur_stream(), C.byref(dd), B, beam, _lib.ptr(dist_d), _lib.ptr(fin), _lib.ptr(active), _lib.ptr(done), _lib.ptr(sou),
            _lib.ptr(sub), _lib.ptr(gen), _lib.ptr(length), _lib.ptr(prob), _lib.ptr(g_out), _lib.ptr(l_out), _lib.ptr(p_out),
            _lib.ptr(parent))
    if required:
        req, nreq = t(st["required"]), t(st["n_required"])
        _lib.check(_lib.lib().fira_beam_select_required(*args, _lib.ptr(req), _lib.ptr(nreq), _lib.ptr(met)),
                   "fira_beam_select_required")
    else:
        _lib.check(_lib.lib().fira_beam_select(*args), "fira_beam_select")
    torch.cuda.synchronize()
    return g_out.cpu(), l_out.cpu(), p_out.cpu(), parent.cpu(), None if met is None else met.cpu()


def equals_the_reference(st, dist, got=None):
    """Every output of every commit == the reference's; returns the reference's picks per commit."""
    B, beam = st["B"], st["beam"]
    V, L, S, T = geometry(st["geo"])
    g, l, p, parent, met = got if got is not None else launch(st, dist)
    all_picks = []
    for b in range(B):
        rows = slice(b * beam, (b + 1) * beam)
        words = R.words_of(st["sou"][b], st["sub"][b], V)
        req = R.required_of(st["required"][b], st["n_required"][b])
        picks = R.select(dist[b], st["fin"][b], st["active"], st["prob"][b], st["length"][b], st["gen"][b], words, req)
        wg, wl, wp, wparent, wmet = R.apply(picks, st["gen"][b].astype(np.int64), st["length"][b].astype(np.int64))
        assert (g[rows].numpy() == wg).all(), ("gen", b)
        assert (l[rows].numpy() == wl).all(), ("len", b)
        assert p[rows].numpy().tobytes() == wp.tobytes(), ("prob", b, p[rows].tolist(), wp.tolist())
        assert (parent[rows].numpy() - b * beam == wparent).all(), ("parent", b)
        assert (met[rows].numpy() == wmet).all(), ("met", b, met[rows].tolist(), wmet.tolist())
        all_picks.append(picks)
    return all_picks


# ------------------------------------------------------------------------------------------------ the anchor: no required word
@pytest.mark.parametrize("geo, beam", [(SMALL, 2), (SMALL, 3), (SMALL_ODD, 5), (SMALL, 8), (MODEL, 3), (MODEL, 8)],
                         ids=["small-2", "small-3", "odd-5", "small-8", "model-3", "model-8"])
def test_without_required_words_it_is_beam_select_bit_for_bit(geo, beam):
    rng = np.random.RandomState(beam)
    for case in ("mixed", "inactive", "done", "start"):
        st = make_state(rng, geo, 3, beam, [0, 0, 0], inactive_slot=1 if case == "inactive" else None)
        if case == "start":                                        # the reset state: slot 0 at 1, the others at 0
            st = make_state(rng, geo, 3, beam, [0, 0, 0], finished=0.0, max_len=1, zero_prob=0.0)
            st["prob"][:] = 0
            st["prob"][:, 0] = 1
        st["done"] = int(case == "done")
        assert case != "inactive" or st["active"][1] == 0
        dist = random_dist(rng, st)
        dist[:, :, ::7] = dist[:, :, 3:4]                          # equal values: the index decides
        want = launch(st, dist, required=False)
        got = launch(st, dist)
        for a, b, name in zip(got[:4], want[:4], ("gen", "len", "prob", "parent")):
            assert torch.equal(a, b) if name != "prob" else torch.equal(bits(a), bits(b)), (case, name)
        assert (got[4] == 0).all()
        got_nomet = launch(st, dist, want_met=False)
        assert all(torch.equal(a, b) for a, b in zip(got_nomet[:4], got[:4])), case


# ------------------------------------------------------------------------------------------------ exactness against the reference
@pytest.mark.parametrize("geo, beam, counts", [(SMALL, 2, [1, 0, 2]), (SMALL_ODD, 3, [2, 0, 1]), (SMALL, 5, [4, 0, 3]),
                                               (SMALL_ODD, 8, [0, 4, 2]), (MODEL, 5, [3, 0, 4])],
                         ids=["small-2", "odd-3", "small-5", "odd-8", "model-5"])
def test_kernel_equals_the_reference(geo, beam, counts):
    rng = np.random.RandomState(100 + beam)
    n_promoted = n_phase2 = 0
    for trial in range(1 if geo is MODEL else 4):
        st = make_state(rng, geo, 3, beam, counts, zero_prob=0.15 if trial else 0.0)
        dist = random_dist(rng, st, zeros=0.5 if trial == 3 else 0.1)
        if trial == 3:
            st["prob"][:, 1:] = 0                                  # few positive candidates: phase 2 fills
            dist[:, 0, 4:] = 0
        for picks in equals_the_reference(st, dist):
            n_promoted += sum(1 for p in picks if not p["carry"] and p["bank"] > 0)
            n_phase2 += sum(1 for p in picks if p["phase"] == 2)
    assert n_promoted > 0 and (geo is MODEL or n_phase2 > 0)       # the inputs are not vacuous


def small_case(seed, beam=4, counts=(2, 1, 3), **kw):
    rng = np.random.RandomState(seed)
    st = make_state(rng, SMALL_ODD, 3, beam, list(counts), **kw)
    return rng, st, random_dist(rng, st, zeros=0.0)


def test_exact_ties_are_decided_by_index():
    rng, st, dist = small_case(1, zero_prob=0.0)
    dist[:] = np.float32(0.25)                                     # every product of a row ties
    st["prob"][:] = np.float32(0.5)                                # ... and every row with every other
    picks = equals_the_reference(st, dist)
    for per_commit in picks:
        for bank in set(p["bank"] for p in per_commit):
            idx = [p["index"] for p in per_commit if p["bank"] == bank and not p["carry"]]
            assert idx == sorted(idx)


def test_a_required_word_carried_by_a_copy_slot_only():
    rng, st, dist = small_case(2, finished=0.0, zero_prob=0.0)
    V = SMALL_ODD["vocab"]
    for b in range(3):
        w = st["required"][b, 0]
        st["gen"][b][st["gen"][b] == w] = 3                        # nobody holds it yet
        st["required"][b, 1:] = 0                                  # (the other places: no word of the batch)
        st["n_required"][b] = 1
        st["sou"][b, 2] = w
        dist[b, :, w] = 0.0                                        # generator entry 0: the slot alone carries the word
        dist[b, :, V + 2] = 0.9
    picks = equals_the_reference(st, dist)
    for b, per_commit in enumerate(picks):
        top = per_commit[0]
        assert top["bank"] == 1 and top["entry"] >= V and top["word"] == st["required"][b, 0]


def test_a_required_word_carried_by_both_its_entries():
    rng, st, dist = small_case(3, beam=3, counts=(1, 1, 1), finished=0.0, zero_prob=0.0)
    V = SMALL_ODD["vocab"]
    for b in range(3):
        w = st["required"][b, 0]
        st["gen"][b][st["gen"][b] == w] = 3
        st["sou"][b] = 3
        st["sub"][b] = 3
        st["sou"][b, 4] = w
        dist[b] *= np.float32(0.01)
        dist[b, 0, w], dist[b, 0, V + 4] = 0.8, 0.9                # both entries of the word, in the most probable row
        st["prob"][b, 0] = 1.0
    picks = equals_the_reference(st, dist)
    for per_commit in picks:                                       # bank 1 gets two of three slots: the slot, then the generator
        assert [(p["bank"], p["src"], p["entry"]) for p in per_commit[:2]] == [(1, 0, V + 4), (1, 0, int(per_commit[0]["word"]))]


def test_eos_in_a_copy_slot_is_blocked_like_the_generator_entry():
    rng, st, dist = small_case(4, finished=0.0, zero_prob=0.0)
    V = SMALL_ODD["vocab"]
    st["sou"][:, 1] = EOS
    st["length"][1, 0], st["gen"][1, 0, 1:3] = 3, (st["required"][1, 0], 3)     # commit 1: a hypothesis that holds its one word
    st["gen"][2][st["gen"][2] == st["required"][2, 0]] = 3                         # commit 2: nobody holds the first word
    dist[:, :, EOS] = 5.0                                          # <eos> would win every row, both ways
    dist[:, :, V + 1] = 4.0
    g, l, p, parent, met = got = launch(st, dist)
    equals_the_reference(st, dist, got)
    ended = missing = 0
    for r in range(g.shape[0]):
        if g[r, l[r] - 1] == EOS:
            ended += 1
            assert met[r] == st["n_required"][r // st["beam"]], "a message ended before it held all its words"
        else:
            missing += 1
    assert ended > 0 and missing > 0


def test_step_zero_with_only_slot_zero_alive():
    rng = np.random.RandomState(5)
    st = make_state(rng, SMALL, 3, 5, [2, 0, 4], finished=0.0, max_len=1, zero_prob=0.0)
    st["prob"][:] = 0
    st["prob"][:, 0] = 1
    dist = random_dist(rng, st, zeros=0.0)
    picks = equals_the_reference(st, dist)
    assert all(p["src"] == 0 for per_commit in picks for p in per_commit)
    assert set(p["bank"] for p in picks[0]) == {0, 1} == set(p["bank"] for p in picks[2])    # one word at most after one step
    assert all(p["bank"] == 0 for p in picks[1])


def test_finished_hypotheses_are_carried():
    rng, st, dist = small_case(6, beam=5, counts=(2, 1, 0), finished=0.6, zero_prob=0.0)
    assert st["fin"].any(1).all() and not st["fin"].all()
    dist *= np.float32(0.05)                                       # the carried probabilities compete
    picks = equals_the_reference(st, dist)
    assert sum(1 for per_commit in picks for p in per_commit if p["carry"]) >= 3


def test_done_passes_the_state_through_and_still_writes_met():
    rng, st, dist = small_case(7, beam=5, counts=(2, 1, 4))
    st["done"] = 1
    g, l, p, parent, met = launch(st, dist)
    B, beam, T = 3, 5, SMALL_ODD["tar_len"]
    assert (g.numpy() == st["gen"].reshape(B * beam, T)).all() and (l.numpy() == st["length"].reshape(-1)).all()
    assert p.numpy().tobytes() == st["prob"].tobytes() and parent.tolist() == list(range(B * beam))
    want = [R.count_met(st["gen"][b, j, :st["length"][b, j]], R.required_of(st["required"][b], st["n_required"][b]))
            for b in range(B) for j in range(beam)]
    assert met.tolist() == want and max(want) > 0


def test_a_count_outside_the_range_is_clamped():
    rng, st, dist = small_case(8, beam=5, counts=(9, -3, 4))
    equals_the_reference(st, dist)


def test_refusals_return_non_zero_with_a_message():
    rng, st, dist = small_case(9)
    for geo, beam, word in ((dict(SMALL, tar_len=65), 4, "tar_len"), (dict(SMALL, vocab=8), 4, "vocabulary"),
                            (dict(SMALL, sou_len=1000, sub_len=25), 4, "memory slots"), (SMALL, 1, "n_beam"), (SMALL, 9, "n_beam")):
        dd = device_dims(**geo)
        args = [_lib.cur_stream(), C.byref(dd), 3, beam] + [C.c_void_p(16)] * 16
        assert _lib.lib().fira_beam_select_required(*args) != 0
        msg = _lib.lib().fira_last_error().decode()
        assert "fira_beam_select_required" in msg and word in msg, msg
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ through the model
# Untrained weights give near-uniform rows: an entry is about 1 / 25 020 = 4e-5, a step's largest about 1e-4, an unlikely word
# down to 5e-6.  The beam's state is the RAW product, and phase 1 takes positive candidates only, so the guarantee "a
# hypothesis that holds all its words never leaves the beam" reaches as far as that product stays positive in fp32.  At the
# model's own tar_len = 30 every product is 0 after about ten steps (tests/util.py: peaked_state_dict) and the zeros tie by
# index; at tar_len = 8 the least product of the seven steps -- two forced prefix words, three required words, two more --
# is about (5e-6)^5 * (1e-4)^2 = 3e-35, inside the normal range (1.2e-38).  The shape is the smallest with room for a prefix
# beside three required words.
MODEL_TAR_LEN = 8


@pytest.fixture(scope="module")
def setup():
    g = golden_search(tar_len=MODEL_TAR_LEN)                       # untrained: every entry of a row is positive
    cfg, model, db = g.cfg, g.model, g.db
    copied = int(next(w for w in db.sou[3].tolist() if w > UNK))   # a word commit 3's diff carries: copy slots promote too
    words = [[700], [1500, 40], [], [copied, 90, 2300 if copied != 2300 else 2301]]
    return cfg, model, db, g.searchers[0], words


BEAM = 5


def holds_its_words(cfg, result, words, what):
    """The properties of a search with required words: ``best_required``'s message contains all of the commit's words and ends
    in <eos> or fills tar_len; met is the count recomputed from gen."""
    from fira_icse_amd.decode import Searcher
    gen, length, prob, met = [t.cpu() for t in result]
    best = Searcher.best_required(None, gen, length, prob, met)
    for b, (msg, req) in enumerate(zip(best, words)):
        if req:
            assert set(req) <= set(msg[1:]), (what, b, msg, req)
            assert msg[-1] == EOS or len(msg) == cfg.tar_len, (what, b, msg)
    for b in range(gen.shape[0]):
        for j in range(gen.shape[1]):
            assert int(met[b, j]) == R.count_met(gen[b, j, :int(length[b, j])].tolist(), words[b]), (what, b, j)


def test_every_message_holds_its_words_and_the_commit_without_words_is_todays(setup):
    cfg, model, db, search, words = setup
    plain = [t.cpu().clone() for t in search.beam(db, BEAM)]
    keys = set(search._ws)
    assert len(search.beam(db, BEAM, require=None)) == 3 and len(search.beam(db, BEAM, require=[[]] * 4)) == 3
    assert set(search._ws) == keys                                 # off: the plain search's states, nothing beside them
    got = search.beam(db, BEAM, require=words)
    assert len(got) == 4 and set(search._ws) - keys == {("beam", db.B, BEAM, "require")}
    holds_its_words(cfg, got, words, "beam")
    gen, length, prob, met = [t.cpu() for t in got]
    b = 2                                                          # the commit without words: the plain result bit for bit
    assert torch.equal(length[b], plain[1][b]) and torch.equal(bits(prob[b]), bits(plain[2][b])) and (met[b] == 0).all()
    live = torch.arange(cfg.tar_len)[None] < length[b][:, None]
    assert torch.equal(gen[b] * live, plain[0][b] * live)
    # the same state serves other words: one capture, the buffers filled on every call
    again = search.beam(db, BEAM, require=[[90], [], [700, 40], words[3]])
    holds_its_words(cfg, again, [[90], [], [700, 40], words[3]], "second word list")
    assert set(search._ws) - keys == {("beam", db.B, BEAM, "require")}
    live = torch.arange(cfg.tar_len)[None] < length[3][:, None]
    assert torch.equal(again[0][3].cpu() * live, gen[3] * live) and torch.equal(bits(again[2][3].cpu()), bits(prob[3]))


def test_it_combines_with_merge_a_prefix_and_an_ensemble(setup):
    from fira_icse_amd.decode import Constraints, Searcher
    cfg, model, db, search, words = setup
    holds_its_words(cfg, search.beam(db, BEAM, merge_copies=True, require=words), words, "merge")
    prefix = [[words[0][0]], [], [], [words[3][1], 55]]            # prefix words count as met
    got = search.beam(db, BEAM, merge_copies=True, prefix=prefix, require=words, constraints=Constraints(min_length=3))
    holds_its_words(cfg, got, words, "prefix")
    assert ("beam", db.B, BEAM, "merge", "prefix", "require", Constraints(min_length=3)) in search._ws
    gen, length, prob, met = [t.cpu() for t in got]
    assert (prob[0] > 0).any() and (prob[3] > 0).any()
    assert all(int(gen[0, j, 1]) == words[0][0] and int(met[0, j]) == 1 for j in range(BEAM) if prob[0, j] > 0)
    assert all(gen[3, j, 1:3].tolist() == prefix[3] and int(met[3, j]) >= 1 for j in range(BEAM) if prob[3, j] > 0)
    pair = Searcher(model, members=[model])                        # the model with itself: the mix is the model's own distribution
    holds_its_words(cfg, pair.beam(db, BEAM, require=words), words, "ensemble")
