"""Prefix-forced search on the device: fira_force_dist alone on synthetic rows against the numpy statement (prefix_ref.py), then
``Searcher.greedy`` / ``beam`` with ``prefix`` against the host loops of the same file, the properties of the messages, the
option-off paths, one capture for every prefix, the constraints, the scorer's word probabilities, and the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import constrain_ref as R
import prefix_ref as P
import util
from search_kit import best_pair, bits, device_dims, golden_search, messages, offset_rows, outside_untouched, run_cli, same_search
from fira_icse_amd import _lib, synth
from fira_icse_amd.config import EOS, PAD, START, UNK, FiraConfig
from fira_icse_amd.decode import Constraints

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ the kernel alone
ALPHABET = (UNK, 5, 6, 9)                        # four words: copy slots collide
ABSENT = 11                                      # a word no slot ever carries (the generator entry alone)
FAR = 30000                                      # an id outside every vocabulary here: it matches slots only, never an index
SMALL = (37, 5, 3)                               # vocab, sou_len, sub_len: W = 45, not a multiple of 4
MODEL = (24650, 210, 160)
GEOMETRIES = [("small-T8-R7", SMALL, 8, 7, 1), ("small-T8-R6x3", SMALL, 8, 6, 3), ("small-T64-R7", SMALL, 64, 7, 1),
              ("small-T64-R6x3", SMALL, 64, 6, 3), ("model-T30-R6x3", MODEL, 30, 18, 3)]
VARIANTS = (0, 1, 2)                             # rotations of the prefix lengths over the commits
SEED = 5


def make_case(name, dims, T, n_rows, rpc, variant=0, seed=SEED):
    """Synthetic rows: hypotheses, copy sources and prefixes over ALPHABET (+ ABSENT and FAR in the prefixes), prefix lengths 0, 1,
    T - 2, 3, 2 rotated over the commits by ``variant``, lengths 1..T with row 0 at m = 0, row 4 at m == its commit's prefix
    length, some rows finished, junk past the length, random positive probabilities."""
    V, L, S = dims
    n_commits = n_rows // rpc
    rng = np.random.RandomState(seed + 17 * T + n_rows + 101 * variant)
    choices = (0, 1, T - 2, 3, 2)
    prefix_len = np.array([choices[(c + variant) % len(choices)] for c in range(n_commits)], dtype=np.int32)
    prefix = rng.choice(ALPHABET + (ABSENT, FAR), size=(n_commits, T)).astype(np.int32)        # (what stays past prefix_len is junk)
    lengths = rng.randint(1, T + 1, size=n_rows).astype(np.int32)
    lengths[0] = 1
    lengths[2] = T
    lengths[4] = prefix_len[4 // rpc] + 1                                              # m == prefix_len
    gen = rng.choice(ALPHABET + (EOS, 0), size=(n_rows, T)).astype(np.int32)           # (what stays past the length is junk)
    for r in range(n_rows):
        gen[r, 0] = START
        gen[r, 1:lengths[r]] = rng.choice(ALPHABET, size=lengths[r] - 1)
    for r in (3, 5):                                                                   # finished rows
        if lengths[r] < 2:
            lengths[r] = 2
        gen[r, lengths[r] - 1] = EOS
    sou = rng.choice(ALPHABET + (EOS, 7, FAR), size=(n_commits, L)).astype(np.int32)
    sub = rng.choice(ALPHABET + (EOS, 8), size=(n_commits, S)).astype(np.int32)
    dist = rng.uniform(1e-6, 1.0, size=(n_rows, V + L + S)).astype(np.float32)
    return dict(name=name, dims=dims, T=T, R=n_rows, rpc=rpc, gen=gen, length=lengths, sou=sou, sub=sub, dist=dist,
                prefix=prefix, prefix_len=prefix_len)


def case_masks(case, prefix_len=None):
    plen = case["prefix_len"] if prefix_len is None else prefix_len
    return P.masks(case["gen"], case["length"], case["sou"], case["sub"], case["dims"], case["prefix"], plen, case["rpc"])


def reference(case):
    """(mask [R, W], dist, edited dist, best_id [R], best_p [R]) with the traps built into the rows that allow them.  A forced row
    r: a zeroed entry holds 3.0, above everything kept (it must be zeroed and lose); r % 3 == 0 and the word has a generator
    entry and a slot: both hold 2.0 (the generator index must win); r % 3 == 1: every kept entry is 0.0 (entry 0 must be
    reported).  A free row with even r: two entries tie at 2.0."""
    V, L, S = case["dims"]
    mask = case_masks(case)
    dist = case["dist"].copy()
    for r in range(case["R"]):
        forced = mask[r].any()
        kept, zeroed = np.flatnonzero(~mask[r]), np.flatnonzero(mask[r])
        if not forced:
            if r % 2 == 0:
                dist[r, kept[len(kept) // 3]] = dist[r, kept[-1]] = np.float32(2.0)
            continue
        dist[r, zeroed[-1]] = dist[r, zeroed[len(zeroed) // 2]] = np.float32(3.0)
        if r % 3 == 0 and len(kept) >= 2 and kept[0] < V:
            dist[r, kept[0]] = dist[r, kept[-1]] = np.float32(2.0)
        if r % 3 == 1:
            dist[r, kept] = np.float32(0.0)
    out = P.edited(dist, mask)
    best = [P.argmax_ref(out[r]) for r in range(case["R"])]
    return mask, dist, out, np.array([b[0] for b in best], dtype=np.int32), np.array([b[1] for b in best], dtype=np.float32)


def run_kernel(case, dist, want_best, offset=1, prefix_len=None):
    """The entry on a copy of ``dist`` that starts ``offset`` floats into its buffer (rows then begin at every alignment); the
    guard words around the rows must stay 0."""
    dev = "cuda"
    n_rows, W = dist.shape
    buf, d_dev = offset_rows(dist, offset)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gen, length, sou, sub, prefix = t(case["gen"]), t(case["length"]), t(case["sou"]), t(case["sub"]), t(case["prefix"])
    plen = t(case["prefix_len"] if prefix_len is None else prefix_len)
    best_id, best_p = best_pair(n_rows, want_best)
    dd = device_dims(*case["dims"], case["T"])
    _lib.check(_lib.lib().fira_force_dist(_lib.cur_stream(), C.byref(dd), n_rows, case["rpc"], _lib.ptr(gen), _lib.ptr(length),
                                          _lib.ptr(sou), _lib.ptr(sub), _lib.ptr(prefix), _lib.ptr(plen), _lib.ptr(d_dev),
                                          _lib.ptr(best_id), _lib.ptr(best_p)), "fira_force_dist")
    torch.cuda.synchronize()
    outside_untouched(buf, offset, n_rows * W)                                         # nothing outside the rows
    return d_dev.cpu(), None if best_id is None else best_id.cpu(), None if best_p is None else best_p.cpu()


def test_inputs_are_not_vacuous():
    """Decided on the reference alone (no launch): every category the kernel has to get right occurs in the generated inputs."""
    seen = dict(slots0=0, slots1=0, slots_many=0, split=0, plen0=0, plen1=0, plen_max=0, below=0, equal=0, above=0, finished=0,
                finished_inside=0, tie=0, tower=0, all_zero=0, free_tie=0, far=0, far_slot=0)
    for g in GEOMETRIES:
        for variant in VARIANTS:
            case = make_case(*g, variant=variant)
            V, L, S = case["dims"]
            T = case["T"]
            mask, dist, out, best_id, best_p = reference(case)
            seen["plen0"] += int((case["prefix_len"] == 0).sum())
            seen["plen1"] += int((case["prefix_len"] == 1).sum())
            seen["plen_max"] += int((case["prefix_len"] == T - 2).sum())
            for r in range(case["R"]):
                plen, m = int(case["prefix_len"][r // case["rpc"]]), int(case["length"][r]) - 1
                fin = R.is_finished(case["gen"][r], case["length"][r])
                seen["finished"] += fin
                seen["finished_inside"] += fin and m < plen
                seen["below"] += (not fin) and m < plen
                seen["equal"] += m == plen
                seen["above"] += m > plen
                if not mask[r].any():
                    assert fin or m >= plen
                    seen["free_tie"] += int((out[r] == best_p[r]).sum() >= 2)
                    continue
                kept = np.flatnonzero(~mask[r])
                slots = kept[kept >= V]
                far = P.forced_word(case["gen"][r], case["length"][r], case["prefix"][r // case["rpc"]], plen, T) == FAR
                seen["far"] += far
                seen["far_slot"] += far and len(slots) >= 1 and len(kept) == len(slots)
                seen["slots0"] += len(slots) == 0
                seen["slots1"] += len(slots) == 1
                seen["slots_many"] += len(slots) >= 2
                seen["split"] += bool((slots < V + L).any() and (slots >= V + L).any())
                seen["tie"] += len(kept) >= 2 and kept[0] < V and best_id[r] == kept[0] and out[r, kept[-1]] == best_p[r] > 0
                seen["tower"] += dist[r].max() > out[r].max()
                seen["all_zero"] += (not out[r].any()) and best_id[r] == 0 and best_p[r] == 0
    assert min(seen.values()) >= 1, seen


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_kernel_equals_the_reference_bit_for_bit(geometry):
    for variant in VARIANTS:
        case = make_case(*geometry, variant=variant)
        mask, dist, out, best_id, best_p = reference(case)
        for want_best in (True, False):                       # (without best a free row is not touched at all)
            for offset in (1, 0):
                got, gid, gp = run_kernel(case, dist, want_best, offset)
                assert torch.equal(bits(got), bits(out)), (case["name"], variant, want_best, offset)
                if want_best:
                    assert gid.tolist() == best_id.tolist(), (case["name"], variant, offset)
                    assert torch.equal(bits(gp), bits(best_p)), (case["name"], variant, offset)


@pytest.mark.parametrize("geometry", [GEOMETRIES[1], GEOMETRIES[4]], ids=[GEOMETRIES[1][0], GEOMETRIES[4][0]])
def test_no_prefix_leaves_the_rows_alone(geometry):
    case = make_case(*geometry)
    none = np.zeros_like(case["prefix_len"])
    dist = case["dist"].copy()
    dist[0, 7] = dist[0, dist.shape[1] - 2] = np.float32(2.0)            # an exact tie: the lower index
    for plen in (none, none - 3):                                        # (a negative length counts as 0)
        got, gid, gp = run_kernel(case, dist, True, prefix_len=plen)
        assert torch.equal(bits(got), bits(dist))
        assert gid.tolist() == dist.argmax(1).tolist() and gid[0] == 7
        assert torch.equal(bits(gp), bits(dist.max(1)))
        got, _, _ = run_kernel(case, dist, False, prefix_len=plen)
        assert torch.equal(bits(got), bits(dist))


# ------------------------------------------------------------------------------------------------ through the model
@pytest.fixture(scope="module")
def setup():
    g = golden_search(weights="peaked", seed=2)
    return g.cfg, g.model, g.db, g.searchers[0]


@pytest.fixture(scope="module")
def today(setup):
    """Today's searches (no prefix), once: (gen, length, prob) on the host, and the greedy messages without <eos>."""
    cfg, model, db, search = setup
    greedy = tuple(t.cpu().clone() for t in search.greedy(db))
    beam = tuple(t.cpu().clone() for t in search.beam(db, 3))
    words = [[w for w in m if w != EOS] for m in messages(greedy[0], greedy[1])]
    return dict(greedy=greedy, beam=beam, words=words)


@pytest.fixture(scope="module")
def mixed(setup, today):
    """One batch with prefixes of length 0, 1, 3 and tar_len - 2: nothing for commit 0; for commit 1 the word commit 2's own
    message begins with; for commit 2 its own first three words in another order; for commit 3 its own message, cycled to
    tar_len - 2 words."""
    cfg, model, db, search = setup
    w = today["words"]
    assert db.B == 4 and len(w[2]) >= 3 and len(w[3]) >= 1
    long = [w[3][i % len(w[3])] for i in range(cfg.tar_len - 2)]
    rows = [[], [w[2][0]], [w[2][2], w[2][0], w[2][1]], long]
    assert [len(r) for r in rows] == [0, 1, 3, cfg.tar_len - 2]
    return rows


@pytest.fixture(scope="module")
def refs(setup, mixed):
    """The reference loops on the mixed batch, once per configuration (shared, never modified)."""
    cfg, model, db, search = setup
    out = {}
    for merge in (False, True):
        out[merge] = dict(beam=tuple(t.cpu() for t in P.beam_forced(search, db, 3, mixed, merge)),
                          greedy=P.greedy_forced(search, db, mixed, merge))
    return out


def starts_with_its_prefix(result, rows, what):
    """Every hypothesis of positive probability starts with its commit's prefix; returns how many such hypotheses there are
    per commit."""
    gen, length, prob = [t.cpu() for t in result[:3]]
    per = gen.shape[1] if gen.dim() == 3 else 1
    msgs, prob = messages(gen, length), prob.reshape(-1).tolist()
    count = [0] * len(rows)
    for k, (m, p) in enumerate(zip(msgs, prob)):
        if p > 0:
            row = rows[k // per]
            assert m[:len(row)] == list(row), (what, k, m, row)
            count[k // per] += 1
    return count


@pytest.mark.parametrize("merge", [False, True], ids=["entries", "merge"])
def test_greedy_and_beam_equal_the_reference_loops_on_a_mixed_batch(setup, refs, mixed, merge):
    cfg, model, db, search = setup
    want = refs[merge]
    for use_graphs in (False, True, True):                    # eager, captured, replayed
        same_search(search.greedy(db, use_graphs=use_graphs, merge_copies=merge, prefix=mixed), want["greedy"])
        same_search(search.beam(db, 3, use_graphs=use_graphs, merge_copies=merge, prefix=mixed), want["beam"])
    for kind in ("greedy", "beam"):
        count = starts_with_its_prefix(want[kind], mixed, kind)
        print("%s, merge %s: hypotheses of positive probability per commit %s, probabilities %s"
              % (kind, merge, count, want[kind][2].tolist()))
        assert min(count) >= 1, (kind, count)                 # (the property is not vacuous for any of the four lengths)
    many = search.greedy_many([db, db, db], in_flight=2, merge_copies=merge, prefix=[mixed, None, mixed])
    torch.cuda.synchronize()
    same_search(many[0], want["greedy"])
    same_search(many[2], want["greedy"])
    same_search(many[1], search.greedy(db, merge_copies=merge))


def test_forcing_the_searchs_own_words_changes_nothing(setup, today):
    """Self-consistency: the first k words of the unforced greedy message, forced, give that message with the same probability
    bits -- the globally largest entry of a step belongs to the forced word and is kept."""
    cfg, model, db, search = setup
    for k in (1, 3):
        rows = [w[:k] for w in today["words"]]
        assert all(len(r) >= 1 for r in rows)
        for use_graphs in (False, True):
            same_search(search.greedy(db, use_graphs=use_graphs, prefix=rows), today["greedy"])


def test_an_empty_prefix_is_todays_search(setup, today):
    cfg, model, db, search = setup
    from fira_icse_amd.decode import Searcher
    fresh = Searcher(model)
    empty = [[] for _ in range(db.B)]
    for use_graphs in (True, False):
        for prefix in (None, empty, tuple(() for _ in range(db.B))):
            got_g = fresh.greedy(db, use_graphs=use_graphs, prefix=prefix)
            got_b = fresh.beam(db, 3, use_graphs=use_graphs, prefix=prefix)
            assert all(torch.equal(bits(a.cpu()), bits(b)) for a, b in zip(got_g, today["greedy"]))
            assert all(torch.equal(bits(a.cpu()), bits(b)) for a, b in zip(got_b, today["beam"]))
    many = fresh.greedy_many([db, db], in_flight=1, prefix=[empty, None])
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a.cpu()), bits(b)) for got in many for a, b in zip(got, today["greedy"]))
    assert set(fresh._ws) == {(db.B, 3), (db.B, 1), ("beam", db.B, 3), ("greedy", db.B)}     # no state keyed by a prefix
    assert "dist" not in fresh._ws[("greedy", db.B)] and "prefix" not in fresh._ws[("beam", db.B, 3)]


def test_one_capture_serves_every_prefix(setup, today, mixed):
    cfg, model, db, search = setup
    from fira_icse_amd.decode import Searcher
    graphs, eager = Searcher(model), Searcher(model)
    w = today["words"]
    other = [[w[0][0]], [], [w[1][0], w[1][1]], [w[2][0]]]
    for rows in (mixed, other, mixed):
        same_search(graphs.greedy(db, use_graphs=True, prefix=rows), eager.greedy(db, use_graphs=False, prefix=rows))
        same_search(graphs.beam(db, 3, use_graphs=True, prefix=rows), eager.beam(db, 3, use_graphs=False, prefix=rows))
    keys = [k for k in graphs._ws if "prefix" in k]
    assert sorted(keys, key=repr) == sorted([("greedy", db.B, "prefix"), ("beam", db.B, 3, "prefix")], key=repr)
    for k in keys:                                            # captured once, replayed for every prefix; the values are not in the key
        st = graphs._ws[k]
        assert st["graphs"] is not None and st["prefix"].shape == (db.B, cfg.tar_len) and st["prefix_len"].shape == (db.B,)
    a, b = graphs.greedy(db, prefix=mixed), graphs.greedy(db, prefix=other)
    assert not torch.equal(a[0], b[0])                        # (the two prefixes do give different messages)


def test_constraints_see_the_forced_words(setup, today):
    """no_repeat_ngram = 1 with a prefix: no prefix word reappears in the continuation (the forced words are part of the
    hypothesis the constraint kernel reads); a prefix that holds a banned id is refused."""
    cfg, model, db, search = setup
    c = Constraints(no_repeat_ngram=1)
    rows = [[w[0]] + ([w[2]] if len(w) > 2 and w[2] != w[0] else []) for w in today["words"]]
    want_g = P.greedy_forced(search, db, rows, False, c)
    want_b = tuple(t.cpu() for t in P.beam_forced(search, db, 3, rows, True, c))
    got_g = search.greedy(db, constraints=c, prefix=rows)
    got_b = search.beam(db, 3, constraints=c, merge_copies=True, prefix=rows)
    same_search(got_g, want_g)
    same_search(got_b, want_b)
    for what, got in (("greedy", got_g), ("beam", got_b)):
        assert min(starts_with_its_prefix(got, rows, what)) >= 1
        gen, length, prob = [t.cpu() for t in got]
        per = gen.shape[1] if gen.dim() == 3 else 1
        for k, (m, p) in enumerate(zip(messages(gen, length), prob.reshape(-1).tolist())):
            if p > 0:
                assert not R.has_repeated_ngram(m, 1), (what, k, m)
                assert not set(rows[k // per]) & set(m[len(rows[k // per]):]), (what, k, m)
    assert any(R.has_repeated_ngram(m, 1) for m in messages(*search.greedy(db, prefix=rows)[:2]))      # without the constraint they do
    banned = Constraints(banned=(rows[1][0],))
    for call in (lambda: search.greedy(db, constraints=banned, prefix=rows),
                 lambda: search.beam(db, 3, constraints=banned, prefix=rows)):
        with pytest.raises(ValueError, match="commit .*banned"):
            call()


def test_groups_ensemble_and_bf16_cache_take_the_prefix(setup, mixed):
    """The combinations the option promises, held to the one property that does not need a reference loop of their own: every
    hypothesis of positive probability starts with its commit's prefix, in every group."""
    cfg, model, db, search = setup
    from fira_icse_amd.decode import BeamScoring, Searcher
    got = search.beam(db, 4, merge_copies=True, scoring=BeamScoring(1.0, 2, 0.5), prefix=mixed)
    assert len(got) == 4 and min(starts_with_its_prefix(got, mixed, "groups")) >= 2
    assert ("beam", db.B, 4, "merge", "prefix", BeamScoring(1.0, 2, 0.5)) in search._ws
    assert min(starts_with_its_prefix(search.beam(db, 1, prefix=mixed), mixed, "beam 1")) >= 1
    pair = Searcher(model, members=[model])                   # the model with itself: the mix is the model's own distribution
    assert min(starts_with_its_prefix(pair.greedy(db, prefix=mixed), mixed, "ensemble greedy")) >= 1
    assert min(starts_with_its_prefix(pair.beam(db, 3, merge_copies=True, prefix=mixed), mixed, "ensemble beam")) >= 1
    half = Searcher(model, kv_bf16=True)
    assert min(starts_with_its_prefix(half.greedy(db, merge_copies=True, prefix=mixed), mixed, "kv_bf16")) >= 1


NORMAL = 1e-30                                   # below it an fp32 product leaves the normal range and rounds coarser than 2^-24


def test_the_probability_is_the_word_sequences(setup, today, mixed):
    """Under merge_copies the returned probability is the joint probability of prefix and continuation: the sequential fp32
    product of ``Searcher.score``'s per-token p_word of the returned message.  The bound that reasoning gives is 1e-4 relative
    -- at most (sou_len + sub_len) + tar_len fp32 roundings of 2^-24 each, roughly 2.4e-5, times 4; measured on an MI355X, all 16
    scored messages came out bit-identical (with these sharpened heads a word's mass sits on one entry, so the two summation
    orders -- slots first here, generator entry first in the scorer -- round alike), so the assertion is ``==``.  Messages the scorer's contract
    excludes (<pad> or <start> inside) and products below the fp32 normal range are left out; so that no commit is left out,
    commit 2 is forced to its own first three words in their own order (the order of ``mixed`` takes its product to 1e-42)."""
    cfg, model, db, search = setup
    T = cfg.tar_len
    mixed = mixed[:2] + [today["words"][2][:3]] + mixed[3:]
    worst, n_scored = 0.0, 0
    for kind in ("greedy", "beam"):
        gen, length, prob = [t.cpu() for t in (search.greedy(db, merge_copies=True, prefix=mixed) if kind == "greedy" else
                                               search.beam(db, 3, merge_copies=True, prefix=mixed))]
        gen, length, prob = gen.reshape(db.B, -1, T), length.reshape(db.B, -1), prob.reshape(db.B, -1)
        pos = torch.arange(T)[None, None, :]
        inside = (pos >= 1) & (pos < length[:, :, None])
        ok = (prob >= NORMAL) & ~(((gen == PAD) | (gen == START)) & inside).any(2)
        assert bool(ok.any(1).all()), (kind, prob)            # every commit has a message that can be scored
        first = ok.long().argmax(1)                           # a slot that cannot be scored is replaced by one that can
        pick = torch.where(ok, torch.arange(gen.shape[1])[None, :], first[:, None])
        cand = torch.gather(gen, 1, pick[:, :, None].expand_as(gen))
        lens = torch.gather(length, 1, pick)
        sc = search.score(db, cand, lengths=lens)
        p_word = sc["p_word"].cpu().numpy()
        for b in range(db.B):
            for j in range(gen.shape[1]):
                if not ok[b, j]:
                    continue
                acc = np.float32(1.0)
                for t in range(int(lens[b, j]) - 1):
                    acc = np.float32(acc * p_word[b, j, t])
                rel = abs(float(acc) - float(prob[b, j])) / float(prob[b, j])
                worst, n_scored = max(worst, rel), n_scored + 1
                print("%s commit %d slot %d: returned %.9g, product of p_word %.9g, relative difference %.3g"
                      % (kind, b, j, float(prob[b, j]), float(acc), rel))
                assert acc == np.float32(prob[b, j]), (kind, b, j, float(prob[b, j]), float(acc))
    print("messages scored %d, largest relative difference %.3g" % (n_scored, worst))
    assert n_scored >= 2 * db.B


# ------------------------------------------------------------------------------------------------ command line
def test_cli_prefix_and_prefix_file(tmp_path):
    from fira_icse_amd.model import reference_init_state_dict
    root = str(tmp_path)
    cfg = FiraConfig()
    synth.write_dataset(root, util.load_golden_raw())
    torch.manual_seed(0)
    torch.save(util.peaked_state_dict(reference_init_state_dict(cfg), seed=2), os.path.join(root, "best_model.pt"))
    base = ["test", "--splits", "16,4,4", "--test-batch-size", "3"]
    out_f = os.path.join(root, "OUTPUT", "output_fira")
    gold = json.load(open(os.path.join(util.GOLDEN, "decode_ref.json")))
    run_cli(base, root)                                          # without the options: the recorded output of the beam-3 search
    assert open(out_f).read() == "".join(l + "\n" for l in gold["beam3"])
    # every commit starts with the two words the recorded greedy message of commit 1 starts with
    start = " ".join(gold["beam1"][1].split()[:2])
    r = run_cli(base + ["--beam", "1", "--prefix", start], root)
    lines = open(out_f).read().split("\n")
    assert len(lines) == 5 and lines[-1] == ""
    for line in lines[:-1]:
        assert line.split()[:2] == start.split(), line
    assert "warning" not in r.stderr
    # one line per commit: commit 0 as recorded, commit 1 none, commit 2 the first word of commit 0, commit 3 a word the
    # vocabulary lacks (<unkm>, written as the reference's emoji)
    starts = [" ".join(gold["beam1"][0].split()[:3]), "", gold["beam1"][0].split()[0], "nosuchword"]
    path = os.path.join(root, "starts")
    with open(path, "w") as f:
        f.write("".join(s + "\n" for s in starts))
    r = run_cli(base + ["--prefix-file", path, "--merge-copies", "--nbest"], root)          # (the beam-3 search)
    lines = open(out_f).read().split("\n")[:-1]
    assert len(lines) == 4
    for line, s in zip(lines[:3], starts[:3]):
        assert line.split()[:len(s.split())] == s.split(), (line, s)
    assert lines[3].split()[:1] == ["\U0001F605"], lines[3]
    assert "warning: 1 prefix words are not in the vocabulary" in r.stderr
    nbest = [json.loads(l) for l in open(os.path.join(root, "OUTPUT", "output_fira_nbest")).read().split("\n")[:-1]]
    for rec, s in zip(nbest[:3], starts[:3]):                # every message of the beam, not only the first
        assert rec["messages"] and all(m.split()[:len(s.split())] == s.split() for m in rec["messages"]), (rec, s)
