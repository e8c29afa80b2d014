"""Search constraints on the device: fira_constrain_dist alone on synthetic rows against the numpy statement
(constrain_ref.py), then ``Searcher.beam`` / ``greedy`` with ``Constraints`` against the torch / host loops of the same file, the
properties of the messages, the options-off paths, the graph cache key, and the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import constrain_ref as R
import util
from search_kit import best_pair, bits, device_dims, golden_search, messages, offset_rows, outside_untouched, run_cli, same_search
from fira_icse_amd import _lib, synth
from fira_icse_amd.config import EOS, START, UNK, FiraConfig
from fira_icse_amd.decode import Constraints

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ the kernel alone
ALPHABET = (UNK, 5, 6, 9)                        # four words: n-grams repeat, copy slots collide, <unkm> is among them
SMALL = (37, 5, 3)                               # vocab, sou_len, sub_len: W = 45, not a multiple of 4
MODEL = (24650, 210, 160)
GEOMETRIES = [("small-T8-R7", SMALL, 8, 7, 1), ("small-T8-R6x3", SMALL, 8, 6, 3), ("small-T64-R7", SMALL, 64, 7, 1),
              ("small-T64-R6x3", SMALL, 64, 6, 3), ("model-T30-R6x3", MODEL, 30, 6, 3)]
CONSTRAINTS = [Constraints(2, 3, (UNK,)), Constraints(1, 0, ()), Constraints(3, 2, (5, 36)), Constraints(0, 1, ()),
               Constraints(0, 0, (6, 9))]
SEED = 3


def make_case(name, dims, T, n_rows, rpc, seed=SEED):
    """Synthetic rows: hypotheses and copy sources over ALPHABET, lengths 1..T (the first rows take 1, 2, T), some finished, junk
    past the length, random positive probabilities."""
    V, L, S = dims
    rng = np.random.RandomState(seed + 17 * T + n_rows)
    lengths = rng.randint(1, T + 1, size=n_rows).astype(np.int32)
    lengths[:3] = (1, 2, T)
    gen = rng.choice(ALPHABET + (EOS, 0), size=(n_rows, T)).astype(np.int32)           # (what stays past the length is junk)
    for r in range(n_rows):
        gen[r, 0] = START
        gen[r, 1:lengths[r]] = rng.choice(ALPHABET, size=lengths[r] - 1)
    for r in (3, 5):                                                                   # finished rows
        if lengths[r] < 2:
            lengths[r] = 2
        gen[r, lengths[r] - 1] = EOS
    sou = rng.choice(ALPHABET + (EOS, 7), size=(n_rows // rpc, L)).astype(np.int32)
    sub = rng.choice(ALPHABET + (EOS, 8), size=(n_rows // rpc, S)).astype(np.int32)
    dist = rng.uniform(1e-6, 1.0, size=(n_rows, V + L + S)).astype(np.float32)
    return dict(name=name, dims=dims, T=T, R=n_rows, rpc=rpc, gen=gen, length=lengths, sou=sou, sub=sub, dist=dist)


def reference(case, c):
    """(mask [R, W], edited dist, best_id [R], best_p [R]) with an exact tie and an overtowering blocked entry built into the
    rows that allow it: the two largest values of row r sit on two unblocked entries (the lower index must win), and a blocked
    entry holds a still larger one (it must be zeroed and lose)."""
    V, L, S = case["dims"]
    mask = np.stack([R.blocked_mask(case["gen"][r], case["length"][r], case["sou"][r // case["rpc"]],
                                    case["sub"][r // case["rpc"]], case["dims"], c) for r in range(case["R"])])
    dist = case["dist"].copy()
    for r in range(case["R"]):
        free, blk = np.flatnonzero(~mask[r]), np.flatnonzero(mask[r])
        if r % 2 == 0 and len(free) >= 2:
            dist[r, free[len(free) // 3]] = dist[r, free[-1]] = np.float32(2.0)        # a generator entry ties with the last entry
        if len(blk):
            dist[r, blk[-1]] = np.float32(3.0)
    out = R.edited(dist, mask)
    best = [R.argmax_ref(out[r]) for r in range(case["R"])]
    return mask, dist, out, np.array([b[0] for b in best], dtype=np.int32), np.array([b[1] for b in best], dtype=np.float32)


def run_kernel(case, c, dist, want_best, offset=1):
    """The entry on a copy of ``dist`` that starts ``offset`` floats into its buffer (rows then begin at every alignment)."""
    dev = "cuda"
    n_rows, W = dist.shape
    buf, d_dev = offset_rows(dist, offset)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gen, length, sou, sub = t(case["gen"]), t(case["length"]), t(case["sou"]), t(case["sub"])
    banned = torch.tensor(list(c.banned) or [0], dtype=torch.int32, device=dev)
    best_id, best_p = best_pair(n_rows, want_best)
    dd = device_dims(*case["dims"], case["T"])
    _lib.check(_lib.lib().fira_constrain_dist(_lib.cur_stream(), C.byref(dd), n_rows, case["rpc"], _lib.ptr(gen), _lib.ptr(length),
                                              _lib.ptr(sou), _lib.ptr(sub), c.no_repeat_ngram, c.min_length, _lib.ptr(banned),
                                              len(c.banned), _lib.ptr(d_dev), _lib.ptr(best_id), _lib.ptr(best_p)),
               "fira_constrain_dist")
    torch.cuda.synchronize()
    outside_untouched(buf, offset, n_rows * W)                                         # nothing outside the rows
    return d_dev.cpu(), None if best_id is None else best_id.cpu(), None if best_p is None else best_p.cpu()


def test_inputs_are_not_vacuous():
    """Decided on the reference mask alone (no launch): over the cases a generator entry, a diff slot and a sub-token slot are
    blocked, some row blocks nothing, some row is finished, and the tie / overtowering entries exist."""
    gen_hit = sou_hit = sub_hit = clean = fin = tie = tower = 0
    for g in GEOMETRIES:
        case = make_case(*g)
        V, L, S = case["dims"]
        fin += sum(R.is_finished(case["gen"][r], case["length"][r]) for r in range(case["R"]))
        for c in CONSTRAINTS:
            mask, dist, out, best_id, best_p = reference(case, c)
            gen_hit += int(mask[:, :V].any())
            sou_hit += int(mask[:, V:V + L].any())
            sub_hit += int(mask[:, V + L:].any())
            clean += int((~mask.any(1)).sum())
            tie += int(((out == best_p[:, None]).sum(1) >= 2).sum())
            tower += int((dist.max(1) > out.max(1)).sum())
    assert min(gen_hit, sou_hit, sub_hit, clean, fin, tie, tower) >= 1, (gen_hit, sou_hit, sub_hit, clean, fin, tie, tower)


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_kernel_equals_the_reference_bit_for_bit(geometry):
    case = make_case(*geometry)
    for c in CONSTRAINTS:
        mask, dist, out, best_id, best_p = reference(case, c)
        for want_best in (True, False):                       # (without best the row is never read: the other code path)
            for offset in (1, 0):
                got, gid, gp = run_kernel(case, c, dist, want_best, offset)
                assert torch.equal(bits(got), bits(out)), (case["name"], c, want_best, offset)
                if want_best:
                    assert gid.tolist() == best_id.tolist(), (case["name"], c, offset)
                    assert torch.equal(bits(gp), bits(best_p)), (case["name"], c, offset)


@pytest.mark.parametrize("geometry", [GEOMETRIES[1], GEOMETRIES[4]], ids=[GEOMETRIES[1][0], GEOMETRIES[4][0]])
def test_all_constraints_off_leaves_the_rows_alone(geometry):
    case = make_case(*geometry)
    off = Constraints()
    dist = case["dist"].copy()
    dist[0, 7] = dist[0, dist.shape[1] - 2] = np.float32(2.0)            # an exact tie: the lower index
    got, gid, gp = run_kernel(case, off, dist, True)
    assert torch.equal(bits(got), bits(dist))
    assert gid.tolist() == dist.argmax(1).tolist() and gid[0] == 7
    assert torch.equal(bits(gp), bits(dist.max(1)))
    got, _, _ = run_kernel(case, off, dist, False)
    assert torch.equal(bits(got), bits(dist))


# ------------------------------------------------------------------------------------------------ through the model
CASES = [Constraints(2, 3, (UNK,)), Constraints(1, 0, ())]


@pytest.fixture(scope="module")
def setup():
    g = golden_search(weights="peaked", seed=2)
    return g.cfg, g.model, g.db, g.searchers[0]


@pytest.fixture(scope="module")
def refs(setup):
    """The reference loops, once per Constraints value (shared, never modified)."""
    cfg, model, db, search = setup
    out = {}
    for c in CASES:
        out[c] = dict(beam=tuple(t.cpu() for t in R.beam_constrained(search, db, 3, c)), greedy=R.greedy_constrained(search, db, c))
    out[None] = dict(beam=tuple(t.cpu().clone() for t in search.beam(db, 3)), greedy=tuple(t.cpu().clone() for t in search.greedy(db)))
    return out


def check_properties(msgs, c, T):
    for words in msgs:
        body = words[:-1] if words and words[-1] == EOS else words
        if c.no_repeat_ngram:
            assert not R.has_repeated_ngram(words, c.no_repeat_ngram), words
        assert not set(body) & set(c.banned), words
        assert EOS not in body
        if words and words[-1] == EOS:
            assert len(body) >= c.min_length, words
        else:
            assert len(words) == T - 1, words                 # no <eos>: the hypothesis ran to tar_len


@pytest.mark.parametrize("c", CASES, ids=["n2-M3-unk", "n1"])
def test_beam_and_greedy_equal_the_reference_loops(setup, refs, c):
    cfg, model, db, search = setup
    for use_graphs in (False, True, True):                    # eager, captured, replayed
        same_search(search.beam(db, 3, use_graphs=use_graphs, constraints=c), refs[c]["beam"])
        same_search(search.greedy(db, use_graphs=use_graphs, constraints=c), refs[c]["greedy"])
    for kind in ("beam", "greedy"):
        gen, length, prob = refs[c][kind]
        check_properties(messages(gen, length), c, cfg.tar_len)
        gen0, length0, prob0 = refs[None][kind]
        best, best0 = search.best(gen, length, prob), search.best(gen0, length0, prob0)
        assert any(a != b for a, b in zip(best, best0)), kind     # the unconstrained fixture messages repeat themselves
    many = search.greedy_many([db, db], in_flight=2, constraints=c)
    torch.cuda.synchronize()
    for got in many:
        same_search(got, refs[c]["greedy"])


def test_options_off_is_todays_search(setup, refs):
    cfg, model, db, search = setup
    from fira_icse_amd.decode import Searcher
    fresh, today = Searcher(model), Searcher(model)
    for use_graphs in (True, False):
        want_b = tuple(t.clone() for t in today.beam(db, 3, use_graphs=use_graphs))            # the calls as they were
        want_g = tuple(t.clone() for t in today.greedy(db, use_graphs=use_graphs))
        for c in (None, Constraints()):
            got_b = fresh.beam(db, 3, use_graphs=use_graphs, constraints=c)
            got_g = fresh.greedy(db, use_graphs=use_graphs, constraints=c)
            assert all(torch.equal(a, b) for a, b in zip(got_b, want_b)) and all(torch.equal(a, b) for a, b in zip(got_g, want_g))
        if use_graphs:
            assert all(torch.equal(a.cpu(), b) for a, b in zip(want_b, refs[None]["beam"]))
            assert all(torch.equal(a.cpu(), b) for a, b in zip(want_g, refs[None]["greedy"]))
    assert set(fresh._ws) == {(db.B, 3), (db.B, 1), ("beam", db.B, 3), ("greedy", db.B)}     # no state keyed by a Constraints
    assert "dist" not in fresh._ws[("greedy", db.B)] and "banned" not in fresh._ws[("beam", db.B, 3)]


def test_each_constraints_value_has_its_own_graphs(setup, refs):
    cfg, model, db, search = setup
    from fira_icse_amd.decode import Searcher
    fresh = Searcher(model)
    for c in (CASES[0], CASES[1], None, CASES[0]):
        same_search(fresh.beam(db, 3, constraints=c), refs[c]["beam"])
        same_search(fresh.greedy(db, constraints=c), refs[c]["greedy"])
    assert ("greedy", db.B, CASES[0]) in fresh._ws and ("beam", db.B, 3, CASES[1]) in fresh._ws
    assert fresh._ws[("greedy", db.B, CASES[0])]["dist"].shape == (db.B, cfg.out_len)
    with pytest.raises(ValueError):
        fresh.beam(db, 3, constraints=Constraints(banned=(cfg.vocab_size,)))
    with pytest.raises(ValueError):
        fresh.greedy(db, constraints=Constraints(min_length=cfg.tar_len - 1))


def test_kernel_with_everything_off_reports_the_steps_own_best(setup):
    cfg, model, db, search = setup
    B, W = db.B, cfg.out_len
    ws = search._begin(db, 1)
    dev = model.device_
    dist = torch.empty((B, W), dtype=torch.float32, device=dev)
    bid, bp = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
    cid, cp = torch.full_like(bid, -7), torch.full_like(bp, -7.0)
    tok = torch.full((B,), START, dtype=torch.int32, device=dev)
    gen = torch.zeros((B, cfg.tar_len), dtype=torch.int32, device=dev)
    gen[:, 0] = START
    length = torch.ones(B, dtype=torch.int32, device=dev)
    search._step(ws, B, 1, 0, tok, None, dist, bid, bp)
    before = dist.clone()
    _lib.check(_lib.lib().fira_constrain_dist(_lib.cur_stream(), C.byref(model.dims), B, 1, _lib.ptr(gen), _lib.ptr(length),
                                              _lib.ptr(db.sou), _lib.ptr(db.sub_token), 0, 0, None, 0, _lib.ptr(dist), _lib.ptr(cid),
                                              _lib.ptr(cp)), "fira_constrain_dist")
    torch.cuda.synchronize()
    assert torch.equal(cid, bid) and torch.equal(bits(cp), bits(bp)) and torch.equal(bits(dist), bits(before))


# ------------------------------------------------------------------------------------------------ command line
def test_cli_constrained_search(tmp_path):
    from fira_icse_amd.model import reference_init_state_dict
    root = str(tmp_path)
    cfg = FiraConfig()
    synth.write_dataset(root, util.load_golden_raw())
    torch.manual_seed(0)
    torch.save(util.peaked_state_dict(reference_init_state_dict(cfg), seed=2), os.path.join(root, "best_model.pt"))
    base = ["test", "--splits", "16,4,4", "--test-batch-size", "3"]
    out_f = os.path.join(root, "OUTPUT", "output_fira")
    run_cli(base, root)                                          # without the options: the recorded output of the beam-3 search
    gold = json.load(open(os.path.join(util.GOLDEN, "decode_ref.json")))["beam3"]
    assert open(out_f).read() == "".join(l + "\n" for l in gold)
    run_cli(base + ["--no-repeat-ngram", "2", "--min-length", "2"], root)
    lines = open(out_f).read().split("\n")
    assert len(lines) == 5 and lines[-1] == "" and lines[:-1] != gold
    for line in lines[:-1]:
        words = line.split()
        assert not R.has_repeated_ngram(words, 2), line
        assert len(words) >= 2, line
