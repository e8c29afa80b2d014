"""fira_contrastive_select on synthetic states against the numpy statement contrastive_ref.py, fira_decode_hidden against the
generator head, and ``Searcher.contrastive`` through the model (golden commits, untrained weights, tar_len = 8)."""
import ctypes as C

import numpy as np
import pytest
import torch

import contrastive_ref as CR
from search_kit import device_dims, golden_search
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, START, UNK

pytestmark = pytest.mark.gpu

F32 = np.float32
SMALL = dict(vocab=11, sou_len=5, sub_len=2, tar_len=8)            # W = 18 (the small geometry of test_require_gpu.py)
SMALL_ODD = dict(vocab=11, sou_len=5, sub_len=3, tar_len=8)        # W = 19: odd, rows at every 4-byte alignment
MODEL = dict(tar_len=8)                                            # the model's own row: W = 25 020, several trips of the stream
B = 3
GAP = 1e-4                                                          # a case whose two best scores are closer is redrawn (CPU only)
# sim and score against the float64 statement.  A 256-term fp32 dot product errs by at most 256 * 2^-24 * sum |a_i c_i|
# <= 256 * 2^-24 * |a| |c| whatever the order of the sum, i.e. by 1.5e-5 of the cosine's scale |a| |c| (rows of norm <= 1:
# 1.5e-5 absolute); the two squared norms err by the same relative bound, their roots by half of it each, so the quotient
# dot / (|a| |c|) carries at most 1.5e-5 + 2 * 0.76e-5 = 3.1e-5, plus three roundings of 6e-8.  The score multiplies sim by
# alpha <= 1 and adds three fp32 roundings of values below 1 (1.8e-7): both stay under 5e-5.
TOL = 5e-5


def geometry(geo):
    d = device_dims(**geo)
    return d.vocab, d.sou_len, d.sub_len, d.tar_len


def rows(rng, shape, exact):
    """Hidden / history rows: small integers in -2..2 (every dot product and squared norm exact in fp32 in any order), or
    random fp32 rows of norm in (0.3, 1]."""
    if exact:
        return rng.randint(-2, 3, size=shape + (CR.D,)).astype(F32)
    x = rng.randn(*(shape + (CR.D,)))
    x *= rng.uniform(0.3, 1.0, size=shape + (1,)) / np.linalg.norm(x, axis=-1, keepdims=True)
    x32 = x.astype(F32)
    assert (np.linalg.norm(x32.astype(np.float64), axis=-1) <= 1.0 + 1e-6).all()
    return x32


def make_state(rng, geo, k, step, exact, eos=0.25, void=0.3, zeros=0.2):
    """B commits as the search holds them entering ``step``: one chosen prefix per commit, one candidate word per slot with
    confidences in descending order, some last slots void, a candidate <eos> now and then."""
    V, L, S, T = geometry(geo)
    W = V + L + S
    hi = min(V, 11)
    gen = np.zeros((B, k, T), dtype=np.int32)
    length = np.full((B, k), step + 1, dtype=np.int32)
    p = np.full((B, k), -1.0, dtype=F32)
    fin = np.zeros((B, k), dtype=np.int32)
    for b in range(B):
        gen[b, :, 0] = START
        if step == 0:
            p[b, 0] = 1.0                                          # the reset state: <start> in slot 0, the others void
            continue
        gen[b, :, 1:step] = rng.randint(3, hi, size=step - 1)
        live = k - (rng.randint(1, k) if rng.rand() < void else 0)
        p[b, :live] = np.sort(rng.uniform(0.05, 0.9, size=live).astype(F32))[::-1]
        words = rng.permutation(np.arange(3, 3 + k))               # distinct candidate words
        gen[b, :, step] = words
        if rng.rand() < eos:
            j = rng.randint(0, live)
            gen[b, j, step], fin[b, j] = EOS, 1
        length[b, live:] = step                                    # a void slot holds the prefix alone
        gen[b, live:, step] = 0
    dist = rng.uniform(1e-6, 1.0, size=(B, k, W)).astype(F32)
    dist[rng.rand(*dist.shape) < zeros] = 0.0                      # what the edit chain leaves behind
    dist[:, :, ::7] = dist[:, :, 3:4]                              # equal values: the index decides
    hist = rows(rng, (B, T), exact)
    hist[:, step:] = 7.0                                           # rows the kernel must not read
    return dict(geo=geo, k=k, step=step, gen=gen, length=length, p=p, fin=fin, prob=rng.uniform(0.1, 1.0, size=B).astype(F32),
                dist=dist, hidden=rows(rng, (B, k), exact), hist=hist, ended=np.zeros(B, dtype=np.int32),
                sou=rng.randint(1, hi, size=(B, L)).astype(np.int32), sub=rng.randint(3, hi, size=(B, S)).astype(np.int32))


def reference(st, alpha):
    V = geometry(st["geo"])[0]
    return [CR.select(st["step"], alpha, st["dist"][b], st["hidden"][b], st["fin"][b], st["sou"][b], st["sub"][b], V, st["gen"][b],
                      st["length"][b], st["p"][b], st["prob"][b], st["hist"][b], st["ended"][b]) for b in range(B)]


def min_gap(st, alpha, commits=range(B)):
    gaps = []
    for b in commits:
        sc = CR.scores(st["p"][b], CR.similarities(st["hidden"][b], st["hist"][b, :st["step"]]), alpha)
        gaps.append(CR.best_two_gap(sc, st["p"][b]))
    return min(gaps)


def draw(seed, geo, k, step, exact, alpha, **kw):
    """A state whose picks are decided by more than GAP in every commit: near-ties are redrawn here, on the CPU, with the
    statement alone -- nothing is left out on the GPU."""
    rng = np.random.RandomState(seed)
    for _ in range(1000):
        st = make_state(rng, geo, k, step, exact, **kw)
        if min_gap(st, alpha) >= GAP:
            return st
    raise AssertionError("no decided case in 1000 draws")


def launch(st, alpha, optional=True):
    dev = "cuda"
    k, step = st["k"], st["step"]
    V, L, S, T = geometry(st["geo"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gen, length, p, fin = t(st["gen"].reshape(B * k, T)), t(st["length"].reshape(-1)), t(st["p"].reshape(-1)), t(st["fin"].reshape(-1))
    prob, dist, hidden, hist, ended = t(st["prob"]), t(st["dist"].reshape(B * k, -1)), t(st["hidden"].reshape(B * k, CR.D)), \
        t(st["hist"]), t(st["ended"])
    sou, sub = t(st["sou"]), t(st["sub"])
    g_out, l_out, p_out, parent = torch.full_like(gen, -7), torch.full_like(length, -7), torch.full_like(p, -7.0), \
        torch.full_like(length, -7)
    prob_out = torch.full_like(prob, -7.0)
    pick, sim, score = (torch.full_like(ended, -7), torch.full_like(p, -7.0), torch.full_like(p, -7.0)) if optional else (None,) * 3
    dd = device_dims(**st["geo"])
    _lib.check(_lib.lib().fira_contrastive_select(
        _lib.cur_stream(), C.byref(dd), B, k, step, float(alpha), _lib.ptr(dist), _lib.ptr(hidden), _lib.ptr(fin), _lib.ptr(sou),
        _lib.ptr(sub), _lib.ptr(gen), _lib.ptr(length), _lib.ptr(p), _lib.ptr(prob), _lib.ptr(hist), _lib.ptr(ended),
        _lib.ptr(g_out), _lib.ptr(l_out), _lib.ptr(p_out), _lib.ptr(prob_out), _lib.ptr(parent), _lib.ptr(pick), _lib.ptr(sim),
        _lib.ptr(score)), "fira_contrastive_select")
    torch.cuda.synchronize()
    n = lambda x: None if x is None else x.cpu().numpy()
    return dict(gen=n(g_out).reshape(B, k, T), length=n(l_out).reshape(B, k), p=n(p_out).reshape(B, k), prob=n(prob_out),
                parent=n(parent).reshape(B, k), pick=n(pick), sim=None if sim is None else n(sim).reshape(B, k),
                score=None if score is None else n(score).reshape(B, k), hist=n(hist), ended=n(ended))


def equals_the_reference(st, alpha, got=None, want=None):
    """Every discrete output == the statement's, p_out and prob_out bit for bit, sim and score within TOL; the history row of
    the step is the winner's and no other row moved.  Returns the statement's results."""
    k, step = st["k"], st["step"]
    got = got or launch(st, alpha)
    want = want or reference(st, alpha)
    for b, w in enumerate(want):
        assert got["pick"][b] == w["pick"], ("pick", b, got["score"][b], w["score"])
        assert (got["parent"][b] - b * k == w["parent"]).all(), ("parent", b)
        assert (got["gen"][b] == w["gen"]).all(), ("gen", b, got["gen"][b], w["gen"])
        assert (got["length"][b] == w["length"]).all(), ("len", b)
        assert got["p"][b].tobytes() == w["p"].tobytes(), ("p", b, got["p"][b], w["p"])
        assert got["prob"][b].tobytes() == w["prob"].tobytes(), ("prob", b)
        assert got["ended"][b] == w["ended"], ("ended", b)
        assert np.abs(got["sim"][b] - w["sim"]).max() <= TOL, ("sim", b, got["sim"][b], w["sim"])
        assert np.abs(got["score"][b].astype(np.float64) - w["score"]).max() <= TOL, ("score", b)
        assert got["hist"][b].tobytes() == w["hist"].tobytes(), ("hist", b)
    return want


CASES = [(SMALL, 2), (SMALL_ODD, 3), (SMALL, 8), (SMALL_ODD, 8), (MODEL, 3), (MODEL, 5)]
IDS = ["small-2", "odd-3", "small-8", "odd-8", "model-3", "model-5"]


# ------------------------------------------------------------------------------------------------ the kernel against the statement
@pytest.mark.parametrize("geo, k", CASES, ids=IDS)
def test_exact_rows_give_the_statements_outputs(geo, k):
    """Integer rows in -2..2: every dot product and squared norm is exact in fp32 in any order, so the kernel's cosines are
    the statement's up to the two roots and the division."""
    T = geometry(geo)[3]
    for step in (0, 1, T - 2):
        st = draw(10 * k + step, geo, k, step, True, 0.6)
        want = equals_the_reference(st, 0.6)
        if step:                                                   # the candidates are the picked row's own entries
            for b, w in enumerate(want):
                for m, e in enumerate(w["entries"]):
                    assert e < 0 or st["dist"][b, w["pick"], e].tobytes() == w["p"][m].tobytes()
    st = draw(77 + k, geo, k, T - 2, True, 0.6)
    got = launch(st, 0.6, optional=False)                          # the three optional outputs left out: the rest unchanged
    full = launch(st, 0.6)
    for name in ("gen", "length", "p", "prob", "parent", "hist", "ended"):
        assert got[name].tobytes() == full[name].tobytes(), name


@pytest.mark.parametrize("geo, k", CASES, ids=IDS)
def test_random_rows_give_the_statements_picks_and_close_scores(geo, k):
    T = geometry(geo)[3]
    for step in (0, 1, T - 2):
        for alpha in (0.6, 1.0):
            equals_the_reference(draw(1000 + 10 * k + step, geo, k, step, False, alpha), alpha)


def test_the_penalty_turns_the_pick():
    """p = (0.5, 0.4); the first candidate's state equals a history row (sim 1), the second is orthogonal to all of them:
    alpha = 0.6 takes the second (0.2 - 0.6 < 0.16 - 0), alpha = 0 the first."""
    st = draw(5, SMALL_ODD, 2, 4, False, 0.6, eos=0.0, void=0.0)
    st["p"][:] = (0.5, 0.4)
    st["hist"][:, :4, 0] = 0.0                                     # nobody has a component along axis 0 ...
    st["hidden"][:, 0] = st["hist"][:, 2]
    st["hidden"][:, 1] = 0.0
    st["hidden"][:, 1, 0] = 0.5                                    # ... but the second candidate, which has nothing else
    got = launch(st, 0.6)
    assert got["pick"].tolist() == [1, 1, 1] and np.abs(got["sim"] - [1.0, 0.0]).max() <= TOL
    assert np.abs(got["score"] - [F32(0.4) * F32(0.5) - F32(0.6), F32(0.4) * F32(0.4)]).max() <= TOL
    equals_the_reference(st, 0.6, got)
    got = launch(st, 0.0)
    assert got["pick"].tolist() == [0, 0, 0] and got["score"].tobytes() == st["p"].tobytes()
    equals_the_reference(st, 0.0, got)


def test_edges():
    V, L, S, T = geometry(SMALL_ODD)
    # fewer than k positive entries leave void slots
    st = draw(6, SMALL_ODD, 5, 3, True, 0.6, eos=0.0, void=0.0)
    st["dist"][:] = 0.0
    st["dist"][:, :, [2, V + 1, 9]] = (0.25, 0.5, 0.25)
    got = launch(st, 0.6)
    want = equals_the_reference(st, 0.6, got)
    assert all(w["entries"] == [V + 1, 2, 9, -1, -1] for w in want)
    assert (got["p"][:, 3:] == -1).all() and (got["length"][:, 3:] == 4).all() and (got["length"][:, :3] == 5).all()
    # an <eos> pick ends the commit and fills every slot with the chosen hypothesis
    st = draw(7, SMALL_ODD, 3, 3, True, 0.0, eos=0.0, void=0.0)
    st["gen"][:, 0, 3], st["fin"][:, 0] = EOS, 1                   # alpha = 0: slot 0, the most probable, wins
    got = launch(st, 0.0)
    equals_the_reference(st, 0.0, got)
    assert got["ended"].tolist() == [1, 1, 1] and (got["gen"] == st["gen"][:, :1]).all() and (got["gen"][:, :, 3] == EOS).all()
    assert (got["length"] == 4).all() and got["prob"].tobytes() == (st["prob"] * st["p"][:, 0]).astype(F32).tobytes()
    # a zero-norm row gives sim 0 (candidate and history row alike); equal slots tie to the lowest
    st = draw(8, SMALL_ODD, 3, 3, False, 0.6, eos=0.0, void=0.0)
    st["hidden"][0, 1] = 0.0
    st["hist"][1, 1] = 0.0
    st["p"][2], st["hidden"][2] = F32(0.3), st["hidden"][2, 0]
    assert min_gap(st, 0.6, (0, 1)) >= GAP and min_gap(st, 0.6, (2,)) == 0.0
    got = launch(st, 0.6)
    equals_the_reference(st, 0.6, got)
    assert got["sim"][0, 1] == 0.0 and np.isfinite(got["sim"]).all() and got["pick"][2] == 0
    assert got["score"][2].tolist() == [got["score"][2, 0]] * 3
    # the ended state copies through (every commit ended: what the `done` latch leaves to copy), history untouched
    st = draw(9, SMALL_ODD, 4, 5, False, 0.6)
    st["ended"][:] = (1, 0, 1)
    got = launch(st, 0.6)
    equals_the_reference(st, 0.6, got)
    for b in (0, 2):
        assert (got["gen"][b] == st["gen"][b]).all() and got["p"][b].tobytes() == st["p"][b].tobytes() and got["pick"][b] == -1
        assert got["parent"][b].tolist() == list(range(4 * b, 4 * b + 4)) and got["hist"][b].tobytes() == st["hist"][b].tobytes()
    # no live slot: the commit ends where it is
    st["ended"][:] = 0
    st["p"][1] = -1.0
    assert min_gap(st, 0.6) >= GAP
    got = launch(st, 0.6)
    equals_the_reference(st, 0.6, got)
    assert got["ended"][1] == 1 and got["pick"][1] == -1


def test_refusals_return_non_zero_with_a_message():
    for geo, k, step, alpha, word in ((dict(SMALL, tar_len=65), 4, 0, 0.5, "tar_len"), (dict(SMALL, vocab=8), 4, 0, 0.5, "vocabulary"),
                                      (dict(SMALL, sou_len=1000, sub_len=25), 4, 0, 0.5, "memory slots"), (SMALL, 1, 0, 0.5, "k = 1"),
                                      (SMALL, 9, 0, 0.5, "k = 9"), (SMALL, 3, 7, 0.5, "step"), (SMALL, 3, -1, 0.5, "step"),
                                      (SMALL, 3, 0, 1.5, "alpha"), (SMALL, 3, 0, float("nan"), "alpha"), (SMALL, 3, 0, -0.1, "alpha")):
        dd = device_dims(**geo)
        args = [_lib.cur_stream(), C.byref(dd), B, k, step, alpha] + [C.c_void_p(16)] * 19
        assert _lib.lib().fira_contrastive_select(*args) != 0
        msg = _lib.lib().fira_last_error().decode()
        assert "fira_contrastive_select" in msg and word in msg, msg
    dd = device_dims(**SMALL)
    args = [_lib.cur_stream(), C.byref(dd), B, 3, 0, 0.5] + [C.c_void_p(16)] * 16 + [None] * 3
    args[6 + 3] = None                                             # sou
    assert _lib.lib().fira_contrastive_select(*args) != 0 and b"null pointer" in _lib.lib().fira_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ through the model
MODEL_TAR_LEN = 8                                                   # as test_require_gpu.py: seven products stay normal in fp32
K = 3


@pytest.fixture(scope="module")
def setup():
    g = golden_search(tar_len=MODEL_TAR_LEN)                       # untrained: every entry of a row is positive
    return g.cfg, g.model, g.db, g.searchers[0]


def test_alpha_zero_is_greedy_search_over_words(setup):
    cfg, model, db, search = setup
    want = [t.cpu() for t in search.greedy(db, merge_copies=True)]
    got = [t.cpu() for t in search.contrastive(db, K, alpha=0.0)]
    assert got[0].shape == (db.B, cfg.tar_len) and got[0].dtype == torch.int64
    assert torch.equal(got[1], want[1]) and (want[1] > 1).all()
    live = torch.arange(cfg.tar_len)[None] < want[1][:, None]
    assert torch.equal(got[0] * live, want[0] * live)
    assert (want[2] > 0).all() and ((got[2] - want[2]).abs() <= 1e-6 * want[2]).all(), (got[2], want[2])


def test_decode_hidden_is_the_input_of_the_generator_head(setup):
    """After an eager step the rows of fira_decode_hidden, taken through out_fc in float64, reproduce the step's generator
    logits.  The step publishes them as dist[r, i] = s_r * exp(logit_i - max_r) for i < vocab, so
    log dist[r, i] - log dist[r, 0] = logit_i - logit_0.  Tolerance per entry, from the formats alone (DESIGN.md section 4 holds
    an fp32 product to the fp64 one): a 256-term fp32 product errs by at most 256 * 2^-24 * sum |x_j w_ij| (the three-term split
    of the matrix cores stays inside it), the bias sum and the subtraction of the row maximum round at 2^-24 of |logit| <= the
    same sum + |b_i|, exp and log carry 2 ulp each: 4 * 2^-23 relative on dist = 4.8e-7 absolute on its logarithm; a difference
    of two entries doubles everything."""
    cfg, model, db, search = setup
    ws = search._begin(db, 1)
    dev = model.device_
    tok = torch.full((db.B,), START, dtype=torch.int32, device=dev)
    dist = torch.zeros((db.B, cfg.out_len), dtype=torch.float32, device=dev)
    best_id, best_p = torch.zeros(db.B, dtype=torch.int32, device=dev), torch.zeros(db.B, dtype=torch.float32, device=dev)
    search._step(ws, db.B, 1, 0, tok, None, dist, best_id, best_p)
    hidden = torch.full((db.B, 256), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().fira_decode_hidden(_lib.cur_stream(), C.byref(model.dims), _lib.ptr(ws), ws.numel(), db.B, 1, search.flags,
                                             _lib.ptr(hidden)), "fira_decode_hidden")
    torch.cuda.synchronize()
    sd = model.state_dict()
    Wt, bias = sd["out_fc.weight"].detach().cpu().double(), sd["out_fc.bias"].detach().cpu().double()
    x = hidden.cpu().double()
    assert torch.isfinite(x).all() and (x.abs().sum(1) > 0).all()
    assert (x.mean(1).abs() < 0.5).all() and ((x.std(1) - 1).abs() < 0.5).all()      # a LayerNorm output (affine near identity)
    logits = x @ Wt.t() + bias
    mag = x.abs() @ Wt.abs().t() + bias.abs()
    V = cfg.vocab_size
    g = dist[:, :V].cpu().double()
    assert (g > 0).all()
    got = torch.log(g) - torch.log(g[:, :1])
    want = logits - logits[:, :1]
    tol = (256 + 2) * 2.0 ** -24 * (mag + mag[:, :1]) + 2 * 4.8e-7
    assert ((got - want).abs() <= tol).all(), float(((got - want).abs() / tol).max())
    assert float(want.abs().max()) > 100 * float(tol.max())          # the check has something to tell apart
    # a workspace that is too small and a misaligned buffer are refused before the launch
    assert _lib.lib().fira_decode_hidden(_lib.cur_stream(), C.byref(model.dims), _lib.ptr(ws), 16, db.B, 1, search.flags,
                                         _lib.ptr(hidden)) != 0
    assert b"workspace too small" in _lib.lib().fira_last_error()
    assert _lib.lib().fira_decode_hidden(_lib.cur_stream(), C.byref(model.dims), _lib.ptr(ws), ws.numel(), db.B, 1, search.flags,
                                         C.c_void_p(hidden.data_ptr() + 4)) != 0


def test_every_step_of_the_search_against_the_statement(setup):
    """The search run eagerly one step at a time with alpha = 0.6.  After every step the state still holds what the selection
    saw (dist, hidden, the `cur` buffers, the history below the step): the statement is run on it, the device's pick must be a
    slot whose statement score is within 1e-4 of the statement's best, and what the device wrote must be the statement's
    result for that pick.  The search continues from the device's choice, so no decision is left out."""
    cfg, model, db, search = setup
    T, V, alpha = cfg.tar_len, cfg.vocab_size, 0.6
    loop = search._contrastive_loop(db, K, alpha, 1, False)
    st = loop.st
    n = lambda x: x.detach().cpu().numpy().copy()
    ended = np.zeros(db.B, dtype=np.int32)
    sou, sub = n(st["sou"]), n(st["sub"])
    n_penalised = 0
    for step in range(T - 1):
        cur, nxt = step & 1, (step + 1) & 1
        loop.launch()
        torch.cuda.synchronize()
        dist, hidden, hist = n(st["dist"]).reshape(db.B, K, -1), n(st["hidden"]).reshape(db.B, K, 256), n(st["hist"])
        gen, length, p = n(st["gen"][cur]).reshape(db.B, K, T), n(st["length"][cur]).reshape(db.B, K), n(st["p"][cur]).reshape(db.B, K)
        fin, prob, pick = n(st["fin"]).reshape(db.B, K), n(st["prob"][cur]), n(st["pick"])
        g2, l2, p2 = n(st["gen"][nxt]).reshape(db.B, K, T), n(st["length"][nxt]).reshape(db.B, K), n(st["p"][nxt]).reshape(db.B, K)
        prob2, sim_d = n(st["prob"][nxt]), n(st["sim"]).reshape(db.B, K)
        for b in range(db.B):
            if ended[b]:
                assert pick[b] == -1 and (g2[b] == gen[b]).all() and prob2[b] == prob[b]
                continue
            sim = CR.similarities(hidden[b], hist[b, :step])
            sc = CR.scores(p[b], sim, alpha).astype(np.float64)
            live = CR.live(p[b])
            j = int(pick[b])
            assert 0 <= j < K and live[j] and sc[j] >= sc[live].max() - 1e-4, (step, b, j, sc, p[b])
            assert np.abs(sim_d[b][live] - sim[live]).max() <= TOL
            assert hist[b, step].tobytes() == hidden[b, j].tobytes()
            # the statement, told the device's pick (the other live slots void), must write what the device wrote
            forced = np.where(np.arange(K) == j, p[b], F32(-1)).astype(F32)
            w = CR.select(step, alpha, dist[b], hidden[b], fin[b], sou[b], sub[b], V, gen[b], length[b], forced, prob[b], hist[b], 0)
            assert w["pick"] == j and (g2[b] == w["gen"]).all() and (l2[b] == w["length"]).all()
            assert p2[b].tobytes() == w["p"].tobytes() and prob2[b].tobytes() == w["prob"].tobytes()
            ended[b] = w["ended"]
            n_penalised += int(step > 0 and sim[live].max() > 0.05)
        if loop.done():                                              # (advances the loop; True after the last step or at `done`)
            break
    assert step == T - 2 or ended.all()
    assert (n(st["ended"]) == ended).all()
    assert n_penalised > 0                                           # the penalty had something to weigh
    tokens, lengths, prob = search._contrastive_result(loop, db.B, K)
    assert (lengths.cpu() >= 2).all() and (tokens[:, 0] == START).all()


def test_eager_captured_and_replayed_runs_agree(setup):
    from fira_icse_amd.decode import Searcher
    cfg, model, db, _ = setup
    search = Searcher(model)
    eager = [t.cpu().clone() for t in search.contrastive(db, K, alpha=0.6, use_graphs=False)]
    key = ("contrastive", db.B, K, 0.6, "merge")
    assert key in search._ws and search._ws[key]["graphs"] is None
    captured = [t.cpu().clone() for t in search.contrastive(db, K, alpha=0.6)]
    assert search._ws[key]["graphs"] is not None
    replayed = [t.cpu().clone() for t in search.contrastive(db, K, alpha=0.6)]
    for a, b, c in zip(eager, captured, replayed):
        assert torch.equal(a, b) and torch.equal(a, c)
    other = [t.cpu() for t in search.contrastive(db, K, alpha=0.25)]
    assert ("contrastive", db.B, K, 0.25, "merge") in search._ws and search._ws[key]["graphs"] is not None
    assert all(torch.equal(a, b.cpu()) for a, b in zip(eager, search.contrastive(db, K, alpha=0.6)))
    assert other[0].shape == eager[0].shape
    with pytest.raises(ValueError, match="chunk = 2"):
        search.contrastive(db, K, alpha=0.6, chunk=2)


def test_constraints_and_a_prefix_pass_through(setup):
    from fira_icse_amd.decode import Constraints
    cfg, model, db, search = setup
    tokens, lengths, prob = [t.cpu() for t in search.contrastive(db, K, alpha=0.6)]
    words = sorted({int(w) for b in range(db.B) for w in tokens[b, 1:int(lengths[b])].tolist() if w > UNK})
    banned = tuple(words[:4])
    assert banned
    con = Constraints(banned=banned, no_repeat_ngram=1)
    t2, l2, p2 = [t.cpu() for t in search.contrastive(db, K, alpha=0.6, constraints=con)]
    assert ("contrastive", db.B, K, 0.6, "merge", con) in search._ws
    for b in range(db.B):
        msg = t2[b, 1:int(l2[b])].tolist()
        assert not set(msg) & set(banned), (b, msg, banned)
        assert len(set(msg)) == len(msg), (b, msg)                   # no word twice
    prefix = [[700, 40], [], [1500], [90, 2300, 55]]
    t3, l3, p3 = [t.cpu() for t in search.contrastive(db, K, alpha=0.6, prefix=prefix)]
    assert ("contrastive", db.B, K, 0.6, "merge", "prefix") in search._ws
    for b, row in enumerate(prefix):
        assert t3[b, 1:1 + len(row)].tolist() == row and int(l3[b]) >= 1 + len(row), (b, t3[b].tolist())
    assert torch.equal(t3[1], tokens[1]) and torch.equal(p3[1], prob[1])     # the commit without a prefix: the plain result
    assert (p3 > 0).all() and (p2 > 0).all()
