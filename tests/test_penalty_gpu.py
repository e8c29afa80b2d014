"""Soft word penalties and biases on the device: fira_penalise_dist alone on synthetic rows against the numpy statement
(penalty_ref.py), bit for bit; then ``Searcher.greedy`` / ``greedy_many`` / ``beam`` / ``sample_search`` with ``penalties=`` against
the host loops of merge_ref.py under ``penalty_ref.make_edit``, the options-off paths, the call counts and the one state that
serves every value.  The first test decides on the reference alone that the kernel cases are not vacuous (no launch: it also
runs without a GPU); every other test is marked ``gpu``."""
import ctypes as C

import numpy as np
import pytest
import torch

import merge_ref as M
import penalty_ref as ref
import prefix_ref as P
from search_kit import (CountingLib, best_pair, bits, count_calls, device_dims, dims_of, golden_search, messages, offset_rows,
                        outside_untouched, same_search)
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, START, UNK
from fira_icse_amd.decode import Constraints, Penalties, Searcher

gpu = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ the kernel alone
ALPHABET = (UNK, 5, 6, 9)                        # four words: counts exceed 1, copy slots collide, <unkm> is among them
SMALL = (37, 5, 3)                               # vocab, sou_len, sub_len: W = 45, not a multiple of 4
MODEL = (24650, 210, 160)
GEOMETRIES = [("small-T8-R7", SMALL, 8, 7, 1), ("small-T8-R6x3", SMALL, 8, 6, 3), ("small-T64-R7", SMALL, 64, 7, 1),
              ("small-T64-R6x3", SMALL, 64, 6, 3), ("model-T30-R6x3", MODEL, 30, 6, 3)]
SEED = 5
SIXTEEN = (5, 9, EOS, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 36)      # emitted, <eos>, slot-only and unused words


def zero_table(T):
    """A first repeat halves, a second bans: count factors (1, 0.5, 0, 0, ...)."""
    t = np.zeros(T, dtype=np.float32)
    t[:2] = (1.0, 0.5)
    return t


def spread(n, lo=-2.0, hi=0.0):
    return [lo + (hi - lo) * k / max(n - 1, 1) for k in range(n)]


# name -> (count table of T, bias mapping of commit b).  Row values are in [1e-6, 1] (and 2, 2.5 below) and every factor is 0 or at
# least exp(-0.5 - 0.25 * 63) * exp(-2) = 1.2e-8, so no product is subnormal.
PARAMS = {
    "penalties alone": (lambda T: ref.factor_table(0.5, 0.25, T), lambda b: None),
    "bias alone, n_bias 0 and 16": (lambda T: ref.factor_table(0.0, 0.0, T),
                                    lambda b: dict(zip(SIXTEEN, spread(16))) if b % 2 == 0 else None),
    "both, a word emitted and biased": (lambda T: ref.factor_table(0.5, 0.25, T), lambda b: {5: 0.75, 6: -2.0, 20: 0.5}),
    "bias on <eos>, which a slot carries": (lambda T: ref.factor_table(0.25, 0.0, T), lambda b: {EOS: -1.5}),
    "bias on words only slots bring in": (lambda T: ref.factor_table(0.0, 0.5, T), lambda b: {7: -1.0, 8: -0.5}),
    "a zero count factor": (zero_table, lambda b: {9: -0.25} if b else None),
}


def make_case(name, dims, T, n_rows, rpc, seed=SEED):
    """Synthetic rows: hypotheses and copy sources over ALPHABET, lengths 1..T (the first rows take 1, 2, T), two finished rows,
    junk past the length, random positive values; at T = 64 the row of length T holds ONE word 63 times."""
    V, L, S = dims
    rng = np.random.RandomState(seed + 17 * T + n_rows)
    lengths = rng.randint(1, T + 1, size=n_rows).astype(np.int32)
    lengths[:3] = (1, 2, T)
    gen = rng.choice(ALPHABET + (EOS, 0), size=(n_rows, T)).astype(np.int32)           # (what stays past the length is junk)
    for r in range(n_rows):
        gen[r, 0] = START
        gen[r, 1:lengths[r]] = rng.choice(ALPHABET, size=lengths[r] - 1)
    if T == 64:
        gen[2, 1:] = 6                                                                 # count_factor[63] is read
    for r in (3, 5):                                                                   # finished rows
        if lengths[r] < 2:
            lengths[r] = 2
        gen[r, lengths[r] - 1] = EOS
    sou = rng.choice(ALPHABET + (EOS, 7), size=(n_rows // rpc, L)).astype(np.int32)
    sub = rng.choice(ALPHABET + (EOS, 8), size=(n_rows // rpc, S)).astype(np.int32)
    dist = rng.uniform(1e-6, 1.0, size=(n_rows, V + L + S)).astype(np.float32)
    return dict(name=name, dims=dims, T=T, R=n_rows, rpc=rpc, gen=gen, length=lengths, sou=sou, sub=sub, dist=dist)


def arrays(case, param):
    """(count table [T], bias_id [B, 16], bias_factor [B, 16], n_bias [B]) of a parameter set.  A commit without a mapping keeps
    n_bias = 0 but gets junk pairs, and one commit's count is pushed outside 0..16: the kernel must clamp, not trust."""
    table_of, bias_of = PARAMS[param]
    B = case["R"] // case["rpc"]
    ids, fac, n = ref.bias_arrays([bias_of(b) for b in range(B)], B)
    for b in range(B):
        if n[b] == 0:
            ids[b], fac[b] = ALPHABET * 4, np.float32(0.125)
    if param == "bias alone, n_bias 0 and 16":
        n[0] = 99                                                                      # counts as 16
        if B > 1:
            n[1] = -3                                                                  # counts as 0
    return table_of(case["T"]), ids, fac, n


def reference(case, param):
    """(dist, edited dist, best_id [R], best_p [R], factor [R, W]) with an exact tie and a dethroned maximum built into the rows
    that allow them: the value 2 sits on two untouched entries (the lower index must win), and the touched entry with the
    smallest factor, if that is below 0.8, holds 2.5 (it must be scaled below 2 and lose)."""
    table, ids, fac, n = arrays(case, param)
    edit = lambda d: ref.edited_rows(d, case["gen"], case["length"], case["sou"], case["sub"], case["dims"], case["rpc"], table,
                                     ids, fac, n)
    factor = edit(np.ones_like(case["dist"]))
    dist = case["dist"].copy()
    for r in range(case["R"]):
        free = np.flatnonzero(factor[r] == 1.0)
        if len(free) >= 2:
            dist[r, free[len(free) // 3]] = dist[r, free[-1]] = np.float32(2.0)        # a generator entry ties with a late entry
        low = int(np.argmin(factor[r]))
        if factor[r, low] < 0.8:
            dist[r, low] = np.float32(2.5)
    out = edit(dist)
    best = [ref.argmax_ref(out[r]) for r in range(case["R"])]
    return dist, out, np.array([b[0] for b in best], dtype=np.int32), np.array([b[1] for b in best], dtype=np.float32), factor


def run_kernel(case, param, dist, want_best, offset=1):
    """The entry on a copy of ``dist`` that starts ``offset`` floats into its buffer (rows then begin at every alignment)."""
    dev = "cuda"
    n_rows, W = dist.shape
    buf, d_dev = offset_rows(dist, offset)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    table, ids, fac, n = (t(a) for a in arrays(case, param))
    gen, length, sou, sub = t(case["gen"]), t(case["length"]), t(case["sou"]), t(case["sub"])
    best_id, best_p = best_pair(n_rows, want_best)
    dd = device_dims(*case["dims"], case["T"])
    _lib.check(_lib.lib().fira_penalise_dist(_lib.cur_stream(), C.byref(dd), n_rows, case["rpc"], _lib.ptr(gen), _lib.ptr(length),
                                             _lib.ptr(sou), _lib.ptr(sub), _lib.ptr(table), _lib.ptr(ids), _lib.ptr(fac),
                                             _lib.ptr(n), _lib.ptr(d_dev), _lib.ptr(best_id), _lib.ptr(best_p)),
               "fira_penalise_dist")
    torch.cuda.synchronize()
    outside_untouched(buf, offset, n_rows * W)                                         # nothing outside the rows
    return d_dev.cpu(), None if best_id is None else best_id.cpu(), None if best_p is None else best_p.cpu()


def test_inputs_are_not_vacuous():
    """Decided on the reference alone (no launch): over the cases a generator entry, a diff slot and a sub-token slot are each
    scaled, some unfinished row is untouched, some row is finished, an entry takes both factors, <eos> is scaled through a slot,
    a word nobody emitted is scaled through a slot, a zero factor lands, count_factor[63] is read, and the tie and the
    dethroned maximum exist."""
    seen = dict(gen=0, sou=0, sub=0, clean=0, fin=0, double=0, eos_slot=0, slot_only=0, zero=0, c63=0, tie=0, dethroned=0, n16=0)
    for g in GEOMETRIES:
        case = make_case(*g)
        V, L, S = case["dims"]
        fin = np.array([ref.is_finished(case["gen"][r], case["length"][r]) for r in range(case["R"])])
        seen["fin"] += int(fin.sum())
        seen["c63"] += int(any(max(ref.counts(case["gen"][r], case["length"][r]).values(), default=0) == 63
                               for r in range(case["R"]) if not fin[r]))
        for param in PARAMS:
            table, ids, fac, n = arrays(case, param)
            dist, out, best_id, best_p, factor = reference(case, param)
            changed = bits(out).numpy() != bits(dist).numpy()
            assert not changed[fin].any()
            seen["gen"] += int(changed[:, :V].any())
            seen["sou"] += int(changed[:, V:V + L].any())
            seen["sub"] += int(changed[:, V + L:].any())
            seen["clean"] += int((~changed.any(1) & ~fin).sum())
            seen["zero"] += int(((out == 0) & (dist > 0)).any())
            seen["tie"] += int(((out == best_p[:, None]).sum(1) >= 2).sum())
            seen["dethroned"] += int(((dist.max(1) == 2.5) & (out.max(1) == 2.0)).sum())
            seen["n16"] += int((np.clip(n, 0, 16) == 16).any())
            for r in np.flatnonzero(~fin):
                b = r // case["rpc"]
                c = ref.counts(case["gen"][r], case["length"][r])
                biased = set(ids[b, :min(max(int(n[b]), 0), 16)].tolist())
                words = ref.entry_words(case["sou"][b], case["sub"][b], case["dims"])
                seen["double"] += int(bool(set(c) & biased))
                seen["eos_slot"] += int(EOS in biased and bool(changed[r, V:][words[V:] == EOS].any()))
                seen["slot_only"] += int(any(w not in c and changed[r, V:][words[V:] == w].any() for w in biased))
    assert min(seen.values()) >= 1, seen


@gpu
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_kernel_equals_the_reference_bit_for_bit(geometry):
    case = make_case(*geometry)
    for param in PARAMS:
        dist, out, best_id, best_p, _ = reference(case, param)
        for want_best in (True, False):                       # (without best the row is read at the touched entries only)
            for offset in (1, 0):
                got, gid, gp = run_kernel(case, param, dist, want_best, offset)
                assert torch.equal(bits(got), bits(out)), (case["name"], param, want_best, offset)
                if want_best:
                    assert gid.tolist() == best_id.tolist(), (case["name"], param, offset)
                    assert torch.equal(bits(gp), bits(best_p)), (case["name"], param, offset)


# ------------------------------------------------------------------------------------------------ through the model
B, BEAM = 4, 3
CON = Constraints(no_repeat_ngram=3, min_length=2)


@pytest.fixture(scope="module")
def setup():
    g = golden_search(weights="spread")
    assert g.db.B == B
    return g.cfg, g.model, g.db, g.searchers[0]


@pytest.fixture(scope="module")
def today(setup):
    """The plain searches (shared, never modified), and from their messages the values the tests use: ``pen`` repeats are
    penalised, every commit's first word is biased down and its second up, <eos> down; ``other`` is a second value."""
    cfg, model, db, search = setup
    greedy = tuple(t.cpu().clone() for t in search.greedy(db))
    beam = tuple(t.cpu().clone() for t in search.beam(db, BEAM))
    words = messages(greedy[0], greedy[1])
    first = [next((x for x in w if x >= UNK), 5) for w in words]
    second = [next((x for x in w if x >= UNK and x != f), 6 if f != 6 else 7) for w, f in zip(words, first)]
    pen = dict(presence=1.5, frequency=0.5, bias=[{f: -3.0, s: 1.0, EOS: -1.0} for f, s in zip(first, second)])
    other = dict(presence=0.25, frequency=2.0, bias={EOS: 0.5, first[0]: -1.0})
    prefix = [[first[0]], [first[1]], [], [first[3], first[3]]]
    return dict(greedy=greedy, beam=beam, pen=Penalties(**pen), other=Penalties(**other), pen_kw=pen, other_kw=other,
                prefix=prefix)


def edit_of(setup, kw, rpc, before=None):
    """The reference edit of the keyword arguments ``kw`` of a ``Penalties`` value (restated by penalty_ref, not read from it)."""
    cfg, model, db, search = setup
    ids, fac, n = ref.bias_arrays(kw["bias"], db.B)
    table = ref.factor_table(kw["presence"], kw["frequency"], cfg.tar_len)
    return ref.make_edit(db.sou.cpu().numpy(), db.sub_token.cpu().numpy(), dims_of(cfg), rpc, table, ids, fac, n, before)


@pytest.fixture(scope="module")
def refs(setup, today):
    """The host loops under the reference edit, once per value (shared, never modified)."""
    cfg, model, db, search = setup
    out = {}
    for name in ("pen", "other"):
        p = today[name + "_kw"]
        out[name] = dict(greedy=M.greedy_edited(search, db, edit_of(setup, p, 1))[:3],
                         beam=tuple(t.cpu() for t in M.beam_edited(search, db, BEAM, edit_of(setup, p, BEAM))))
    return out


@gpu
def test_greedy_and_beam_equal_the_reference_loops(setup, today, refs):
    cfg, model, db, search = setup
    p = today["pen"]
    for use_graphs in (False, True, True):                    # eager, captured, replayed
        same_search(search.greedy(db, use_graphs=use_graphs, penalties=p), refs["pen"]["greedy"])
        same_search(search.beam(db, BEAM, use_graphs=use_graphs, penalties=p), refs["pen"]["beam"])
    # the equalities are not vacuous: the penalties change messages, and the score is no longer the plain probability
    for kind in ("greedy", "beam"):
        gen, length, prob = refs["pen"][kind]
        gen0, length0, prob0 = today[kind]
        assert search.best(gen, length, prob) != search.best(gen0, length0, prob0), kind
    assert not torch.equal(refs["pen"]["greedy"][2], today["greedy"][2])


@gpu
def test_with_merge_constraints_and_a_prefix(setup, today):
    cfg, model, db, search = setup
    p, kw, rows = today["pen"], today["pen_kw"], today["prefix"]
    assert any(set(r) & set(b) for r, b in zip(rows, kw["bias"]))                          # a prefix word is biased too
    opts = dict(merge_copies=True, constraints=CON, prefix=rows, penalties=p)
    want_g = M.greedy_edited(search, db, edit_of(setup, kw, 1, P.make_edit(search, db, rows, 1, True, CON)))[:3]
    want_b = tuple(t.cpu() for t in M.beam_edited(search, db, BEAM, edit_of(setup, kw, BEAM, P.make_edit(search, db, rows, BEAM, True, CON))))
    for use_graphs in (False, True):
        same_search(search.greedy(db, use_graphs=use_graphs, **opts), want_g)
        same_search(search.beam(db, BEAM, use_graphs=use_graphs, **opts), want_b)
    key = Searcher._key(("greedy", B), True, CON, forced=True, penalties=True)
    assert key == ("greedy", B, "merge", "prefix", "penalties", CON) and key in search._ws
    for m, r in zip(messages(*want_g[:2]), rows):             # prefix words count as emitted; the messages still begin with them
        assert m[:len(r)] == r


@gpu
def test_sample_search_with_top_k_1_is_greedy(setup, today):
    cfg, model, db, search = setup
    p = today["pen"]
    out, length, prob = search.greedy(db, use_graphs=False, penalties=p)
    # every step's maximum of the EDITED row along the greedy path is unique
    st = search._ws[Searcher._key(("greedy", B), False, None, penalties=True)]
    ws = search._begin(db, 1)
    search._greedy_reset(st)
    for step in range(int(length.max()) - 1):
        alive = st["alive"].bool()
        search._greedy_steps(st, ws, B, step, step + 1)
        top2 = torch.topk(st["dist"], 2, dim=1).values
        assert (top2[alive, 0] > top2[alive, 1]).all(), step
    for n in (1, 2):
        toks, lens, p_, logp = search.sample_search(db, n, top_k=1, seed=9, penalties=p)
        for j in range(n):
            same_search((toks[:, j], lens[:, j], p_[:, j]), (out, length, prob))


@gpu
def test_greedy_many_equals_greedy_per_batch(setup, today, refs):
    cfg, model, db, search = setup
    many = search.greedy_many([db, db, db], in_flight=2, penalties=today["pen"])
    torch.cuda.synchronize()
    assert len(many) == 3
    for got in many:
        same_search(got, refs["pen"]["greedy"])


@gpu
def test_options_off_is_todays_search(setup, today, monkeypatch):
    cfg, model, db, search = setup
    fresh = Searcher(model)
    got = {}

    def run():
        for p in (None, Penalties(), Penalties(bias={UNK: 0.0})):
            for use_graphs in (True, False):
                got[(p, use_graphs)] = (fresh.greedy(db, use_graphs=use_graphs, penalties=p),
                                        fresh.beam(db, BEAM, use_graphs=use_graphs, penalties=p),
                                        fresh.greedy_many([db], in_flight=1, penalties=p)[0])
    calls = count_calls(monkeypatch, run)
    assert "fira_penalise_dist" not in calls and calls["fira_decode_step_ex"] > 0
    for g, b, m in got.values():
        for res, want in ((g, today["greedy"]), (b, today["beam"]), (m, today["greedy"])):
            assert all(torch.equal(bits(x.cpu()), bits(y)) for x, y in zip(res, want))
    assert set(fresh._ws) == {(B, BEAM), (B, 1), ("beam", B, BEAM), ("greedy", B)}        # no state keyed by penalties
    assert "dist" not in fresh._ws[("greedy", B)] and "count_factor" not in fresh._ws[("beam", B, BEAM)]


class RecordingLib(CountingLib):
    """``CountingLib`` that also keeps whether each fira_penalise_dist call carried the best pair (its last two arguments)."""

    def __init__(self, real):
        super().__init__(real)
        self.best = []

    def __getattr__(self, name):
        counted = super().__getattr__(name)
        if name != "fira_penalise_dist":
            return counted

        def recorded(*args):
            self.best.append((args[-2] is not None, args[-1] is not None))
            return counted(*args)
        return recorded


@gpu
def test_one_call_per_step_with_the_best_pair_in_greedy_only(setup, today, monkeypatch):
    cfg, model, db, search = setup
    p = today["pen"]
    fresh = Searcher(model)
    for run, steps, pair in ((lambda: fresh.greedy(db, use_graphs=False, penalties=p), "fira_greedy_advance", (True, True)),
                             (lambda: fresh.beam(db, BEAM, use_graphs=False, penalties=p), "fira_beam_select", (False, False)),
                             (lambda: fresh.sample_search(db, 2, use_graphs=False, penalties=p), "fira_sample_advance", (False, False)),
                             (lambda: fresh.greedy(db, use_graphs=False, merge_copies=True, constraints=CON, penalties=p),
                              "fira_greedy_advance", (True, True))):
        lib = RecordingLib(_lib.lib())
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "_lib", lib)
            run()
        torch.cuda.synchronize()
        assert lib.calls["fira_penalise_dist"] == lib.calls[steps] == lib.calls["fira_decode_step_ex"] > 0
        assert lib.best == [pair] * lib.calls[steps]


@gpu
def test_one_state_and_one_capture_serve_every_value(setup, today, refs):
    cfg, model, db, search = setup
    fresh = Searcher(model)
    keys = [("greedy", B, "penalties"), ("beam", B, BEAM, "penalties")]
    graphs = None
    for name in ("pen", "other", "pen", "other"):
        same_search(fresh.greedy(db, penalties=today[name]), refs[name]["greedy"])
        same_search(fresh.beam(db, BEAM, penalties=today[name]), refs[name]["beam"])
        assert sorted((k for k in fresh._ws if "penalties" in k), key=repr) == sorted(keys, key=repr)
        now = [fresh._ws[k]["graphs"] for k in keys]
        assert all(g is not None for g in now)
        assert graphs is None or all(a is b for a, b in zip(graphs, now))               # captured once, replayed for every value
        graphs = now
    st = fresh._ws[keys[1]]
    assert st["count_factor"].shape == (cfg.tar_len,) and st["bias_id"].shape == (B, 16) and st["n_bias"].shape == (B,)
    assert st["bias_factor"].dtype == torch.float32 and st["dist"].shape == (B * BEAM, cfg.out_len)
    for kind in ("greedy", "beam"):                           # (the two values do give different results)
        assert not torch.equal(refs["pen"][kind][0], refs["other"][kind][0]) or \
            not torch.equal(bits(refs["pen"][kind][2]), bits(refs["other"][kind][2]))
