"""The one chunked step loop behind Searcher.greedy / beam / sample / score (decode._Loop) and the one advance kernel behind
fira_greedy_advance / fira_sample_advance: the chunk size changes no result, every loop stops where its own stop test says, a
captured state refuses another chunk size, and the merged kernel is the torch statement of the bookkeeping for both entry points."""
import ctypes as C

import pytest
import torch

import util
from search_kit import bits, golden_search, spread_state_dict
from fira_icse_amd import _lib

pytestmark = pytest.mark.gpu

CHUNKS = [1, 4, 29]            # one step per graph; a size that does not divide tar_len - 1 = 29; a single chunk
SAMPLE_KW = dict(seed=3, temperature=1.5)


@pytest.fixture(scope="module")
def setup():
    from fira_icse_amd.model import TransModel, DeviceBatch, reference_init_state_dict
    g = golden_search(weights="peaked", searchers=0, seed=2)
    cfg = g.cfg
    assert cfg.tar_len - 1 == 29

    def model_of(sd):
        m = TransModel(cfg, init=False)
        m.load_state_dict(sd)
        m.eval()
        return m
    spread = model_of(spread_state_dict(cfg))
    torch.manual_seed(0)
    sd = util.peaked_state_dict(reference_init_state_dict(cfg), seed=2)
    sd["out_fc.bias"][1] += 30.0                                     # <eos> early: every hypothesis ends well before tar_len
    short = model_of(sd)
    two = DeviceBatch(g.store.batch(g.ids[:2]), cfg)                 # the commits whose beam-3 hypotheses all end early
    return cfg, g.host_batch, dict(peaked=g.model, spread=spread, short=short, two=two), g.db


def run_search(kind, models, db, cand=None, **kw):
    """One call of the search ``kind`` on a FRESH Searcher (twice when it captures: the second call replays).  Returns the
    searcher and the results of every call, each a dict of tensors."""
    from fira_icse_amd.decode import Searcher
    search = Searcher(models["spread" if kind in ("sample", "score") else "peaked"])
    call = dict(greedy=lambda: dict(zip(("ids", "length", "prob"), search.greedy(db, **kw))),
                beam=lambda: dict(zip(("ids", "length", "prob"), search.beam(db, 3, **kw))),
                sample=lambda: dict(zip(("ids", "length", "prob", "logp"), search.sample(db, 2, **SAMPLE_KW, **kw))),
                score=lambda: dict(search.score(db, cand[0], lengths=cand[1], **kw)))[kind]
    return search, [call() for _ in range(2 if kw.get("use_graphs", True) else 1)]


@pytest.fixture(scope="module")
def eager(setup):
    """The eager chunk = 5 result of every search, computed once and left unchanged."""
    cfg, hb, models, db = setup
    T = cfg.tar_len
    ref = {kind: run_search(kind, models, db, chunk=5, use_graphs=False)[1][0] for kind in ("greedy", "beam", "sample")}
    toks, lens = ref["sample"]["ids"], ref["sample"]["length"]
    inside = torch.arange(1, T, device=toks.device)[None, None, :] < lens[:, :, None]
    assert not bool((((toks[:, :, 1:] == 0) | (toks[:, :, 1:] == 2)) & inside).any()), \
        "fixture: a sampled message holds <pad> or <start>"
    ref["cand"] = (toks.clone(), lens.clone())
    ref["score"] = run_search("score", models, db, ref["cand"], chunk=5, use_graphs=False)[1][0]
    return ref


# what the existing eager-vs-graph tests compare bit for bit, and what they hold to rtol = 1e-5, atol = 0 (test_decode_gpu,
# test_sample_gpu; test_score_gpu and the beam bookkeeping test demand bit equality of everything)
CLOSE = dict(greedy=("prob",), sample=("prob",), beam=(), score=())


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("kind", ["greedy", "beam", "sample", "score"])
def test_chunk_size_changes_nothing(setup, eager, kind, chunk):
    cfg, hb, models, db = setup
    search, (captured, replayed) = run_search(kind, models, db, eager["cand"], chunk=chunk)
    want = eager[kind]
    st = [v for k, v in search._ws.items() if isinstance(k[0], str)]
    assert len(st) == 1 and len(st[0]["graphs"]) == -(-29 // chunk) and st[0]["chunk"] == chunk
    assert st[0]["bounds"][-1][1] == 29 and all(hi - lo <= chunk for lo, hi in st[0]["bounds"])
    assert set(captured) == set(want)
    for k in want:
        assert torch.equal(bits(replayed[k]), bits(captured[k])), (k, "replay vs capture")
        if k in CLOSE[kind]:
            print(kind, chunk, k, float(((captured[k] - want[k]).abs() / want[k].abs().clamp(min=1e-30)).max()))
            assert torch.allclose(captured[k], want[k], rtol=1e-5, atol=0), k
        else:
            assert torch.equal(bits(captured[k]), bits(want[k])), k


class Counted:
    def __init__(self, g, i, log):
        self.g, self.i, self.log = g, i, log

    def replay(self):
        self.log.append(self.i)
        self.g.replay()


def count_replays(search, key):
    st = search._ws[key]
    log = []
    st["graphs"] = [Counted(g, i, log) for i, g in enumerate(st["graphs"])]
    return st, log


def test_greedy_stops_after_the_chunk_where_the_last_hypothesis_ended(setup):
    from fira_icse_amd.decode import Searcher
    cfg, hb, models, db = setup
    search = Searcher(models["short"])
    out, length, prob = search.greedy(db)                            # captures (chunk = 5)
    st, log = count_replays(search, ("greedy", db.B))
    out2, length2, prob2 = search.greedy(db)
    assert torch.equal(out, out2) and torch.equal(length, length2) and torch.equal(prob, prob2)
    last_step = int(length.max()) - 2                                # the step that appended the last <eos>
    k = last_step // 5 + 1
    assert log == list(range(k))                                     # n_alive[hi - 1] == 0 is read after chunk k - 1
    assert k < len(st["graphs"]), "the fixture's hypotheses should end before the last chunk"


@pytest.mark.parametrize("batch", ["all", "two"])
def test_beam_stops_after_the_chunk_that_latched_done(setup, batch):
    """``done`` is latched by fira_beam_prepare of the step AFTER the one that appended the last <eos> (it looks at the
    hypotheses it is given), so the last chunk replayed is the one that holds that step.  On the early-<eos> weights the third
    hypothesis of two of the fixture's four commits never ends (measured: it repeats one word up to tar_len), so beam(db, 3)
    on the whole batch must replay every chunk; the first two commits alone end within a few steps: that batch stops early."""
    from fira_icse_amd.decode import Searcher
    cfg, hb, models, db = setup
    db = db if batch == "all" else models["two"]
    search = Searcher(models["short"])
    gen, length, prob = search.beam(db, 3)                           # captures (chunk = 4)
    st, log = count_replays(search, ("beam", db.B, 3))
    gen2, length2, prob2 = search.beam(db, 3)
    assert torch.equal(gen, gen2) and torch.equal(length, length2) and torch.equal(prob, prob2)
    ended = bool((gen.gather(2, (length - 1)[:, :, None]) == 1).all())
    latch_step = int(length.max()) - 2 + 1
    k = min(latch_step // 4 + 1, len(st["graphs"])) if ended else len(st["graphs"])
    print("beam", batch, "lengths", length.tolist(), "ended", ended, "chunks", log)
    assert log == list(range(k))
    if batch == "two":
        assert ended and k < len(st["graphs"]), "the fixture's hypotheses should end before the last chunk"
    else:
        assert not ended, "fixture: a hypothesis of the whole batch is known to run to tar_len"


def test_score_replays_the_chunks_the_longest_candidate_needs(setup):
    from fira_icse_amd.decode import Searcher
    cfg, hb, models, db = setup
    search = Searcher(models["peaked"])
    cand = torch.from_numpy(hb.tar[:, :12].copy())                  # the teacher messages, cut at 12 positions
    lens = (cand != 0).sum(1)
    Lmax = int(lens.max())
    assert Lmax == 12 and int(lens.min()) < 12
    first = search.score(db, cand, lengths=lens)                     # captures (chunk = 5)
    st, log = count_replays(search, ("score", db.B, 1, False))
    again = search.score(db, cand, lengths=lens)
    for k in first:
        assert torch.equal(bits(first[k]), bits(again[k])), k
    want = [i for i, (lo, hi) in enumerate(st["bounds"]) if lo < Lmax - 1]
    assert log == want == [0, 1, 2] and len(want) < len(st["graphs"])


def test_a_captured_state_refuses_another_chunk(setup):
    from fira_icse_amd.decode import Searcher
    cfg, hb, models, db = setup
    search = Searcher(models["peaked"])
    out, length, prob = search.greedy(db)                            # captures with chunk = 5
    with pytest.raises(ValueError, match=r"chunk = 3\b.*chunk = 5\b"):
        search.greedy(db, chunk=3)
    out_e, length_e, prob_e = search.greedy(db, chunk=3, use_graphs=False)
    assert torch.equal(out, out_e) and torch.equal(length, length_e)
    out_r, length_r, prob_r = search.greedy(db)                      # the state is still the chunk-5 one
    assert torch.equal(out, out_r) and torch.equal(prob, prob_r)
    assert search._ws[("greedy", db.B)]["chunk"] == 5


def advance_inputs(cfg, R, n, steps=3):
    """Synthetic inputs of the advance kernel on the CPU (seeded): the commits' id rows, the rows alive on entry, and per step
    the picked entries (all three id ranges, their edges, the last sub slot, <eos> from the vocabulary and through copy slots)
    with random probabilities."""
    V, L, S, W = cfg.vocab_size, cfg.sou_len, cfg.sub_token_len, cfg.out_len
    B = R // n
    assert B * n == R and W == V + L + S
    g = torch.Generator().manual_seed(100 + n)
    sou = torch.randint(4, V, (B, L), generator=g).to(torch.int32)
    sub = torch.randint(4, V, (B, S), generator=g).to(torch.int32)
    sou[::5, 7] = 1                                                  # copy slots that resolve to <eos>
    sub[::7, S - 1] = 1
    alive = (torch.rand(R, generator=g) > 0.15).to(torch.int32)      # some rows dead on entry, in both workgroups
    alive[[0, 63, 64, 255, 256]] = 1
    alive[[1, 65, 257]] = 0
    picks = []
    for step in range(steps):
        w = torch.randint(0, V, (R,), generator=g)
        kind = torch.randint(0, 8, (R,), generator=g)
        w = torch.where(kind == 1, V + torch.randint(0, L, (R,), generator=g), w)            # sou copy slots
        w = torch.where(kind == 2, V + L + torch.randint(0, S, (R,), generator=g), w)        # sub copy slots
        w = torch.where(kind == 3, torch.full_like(w, W - 1), w)                             # the last sub slot (the clamp's edge)
        w = torch.where(kind == 4, torch.full_like(w, 1), w)                                 # <eos> from the vocabulary
        w = torch.where(kind == 5, torch.full_like(w, V + 7), w)                             # <eos> through a sou slot (some commits)
        if step == 0:
            w[0], w[63], w[64], w[255], w[256] = V - 1, V, V + L - 1, V + L, W - 1           # the range edges, both workgroups
        picks.append((w.to(torch.int32), 0.05 + 0.95 * torch.rand(R, generator=g)))
    return sou, sub, alive, picks


def advance_statement(cfg, n, sou, sub, st, bid, bp, step):
    """One step of the bookkeeping as test_sample_gpu.test_bookkeeping_equals_torch_statement states it, on the reference state
    ``st`` (out, length, alive, prob fp32 running product, logp float64 sum); returns the resolved ids as well."""
    V, L, S = cfg.vocab_size, cfg.sou_len, cfg.sub_token_len
    commit = torch.arange(bid.numel(), device=bid.device) // n
    w = bid.long()
    nt = torch.where(w >= V + L, sub[commit, (w - V - L).clamp(0, S - 1)],
                     torch.where(w >= V, sou[commit, (w - V).clamp(0, L - 1)], w)).to(torch.int32)
    live = st["alive"].bool()
    st["out"][live, step + 1] = nt[live]
    st["length"] += live.to(torch.int32)
    st["prob"] = torch.where(live, st["prob"] * bp, st["prob"])
    st["logp"] += torch.where(live, torch.log(bp.double()), torch.zeros_like(st["logp"]))
    st["alive"] = (live & (nt != 1)).to(torch.int32)
    return nt


@pytest.mark.parametrize("n", [1, 3])
def test_merged_advance_kernel_equals_torch_statement(setup, n):
    """R = 258 rows (two workgroups, the second a partial wave; 86 commits at n = 3) through fira_sample_advance, and at n = 1
    through fira_greedy_advance as well, three steps: out / length / alive / tok / n_alive[step] equal the torch statement, prob
    is the running fp32 product bit for bit, logp is within 1e-5 of the float64 sum, and the two entry points agree."""
    cfg, hb, models, db = setup
    dims = models["peaked"].dims
    dev = "cuda"
    R, T = 258, cfg.tar_len
    B = R // n
    sou, sub, alive0, picks = advance_inputs(cfg, R, n)
    sou, sub, alive0 = sou.to(dev), sub.to(dev), alive0.to(dev)

    def fresh():
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
        st = dict(out=i32(R, T), length=i32(R), prob=torch.ones(R, device=dev), logp=torch.zeros(R, device=dev),
                  alive=alive0.clone(), tok=torch.full((R,), 77, dtype=torch.int32, device=dev), n_alive=i32(T))
        st["out"][:, 0] = 2
        st["length"].fill_(1)
        return st
    smp, grd, ref = fresh(), fresh(), fresh()
    ref["logp"] = ref["logp"].double()
    lib, s, p = _lib.lib(), _lib.cur_stream(), _lib.ptr
    for step, (bid, bp) in enumerate(picks):
        bid, bp = bid.to(dev), bp.to(dev)
        before = int(ref["alive"].sum())
        nt = advance_statement(cfg, n, sou, sub, ref, bid, bp, step)
        assert 0 < int(ref["alive"].sum()) < before, "the fixture should end some rows at every step, not all"
        _lib.check(lib.fira_sample_advance(s, C.byref(dims), B, n, step, p(bid), p(bp), p(sou), p(sub), p(smp["out"]),
                                           p(smp["length"]), p(smp["prob"]), p(smp["logp"]), p(smp["alive"]), p(smp["tok"]),
                                           p(smp["n_alive"])), "fira_sample_advance")
        runs = [smp]
        if n == 1:
            _lib.check(lib.fira_greedy_advance(s, C.byref(dims), B, step, p(bid), p(bp), p(sou), p(sub), p(grd["out"]),
                                               p(grd["length"]), p(grd["prob"]), p(grd["alive"]), p(grd["tok"]),
                                               p(grd["n_alive"])), "fira_greedy_advance")
            runs.append(grd)
        for st in runs:
            assert torch.equal(st["out"], ref["out"]) and torch.equal(st["length"], ref["length"]), step
            assert torch.equal(st["alive"], ref["alive"]), step
            assert torch.equal(st["tok"], torch.where(ref["alive"].bool(), nt, torch.zeros_like(nt))), step
            assert int(st["n_alive"][step]) == int(ref["alive"].sum()), step
            assert torch.equal(bits(st["prob"]), bits(ref["prob"])), step
    assert torch.allclose(smp["logp"].double(), ref["logp"], rtol=1e-5, atol=1e-5)
    if n == 1:
        assert not bool(grd["logp"].any())                           # the greedy entry point has no logp: untouched
        for k in ("out", "length", "prob", "alive", "tok", "n_alive"):
            assert torch.equal(bits(smp[k]), bits(grd[k])), k
