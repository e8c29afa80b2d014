"""METEOR alignment on the device: the dev kernel and the all-pairs kernel against the literal two-loop oracle (exact, with and
without a class table), ``Searcher.mbr(..., utility="meteor_exact")`` against the host loop over ``metrics.meteor_exact``
(``==``), and ``DevEvaluator(meteor_exact=True)``: the device pass against the host pass."""
import math

import numpy as np
import pytest
import torch

import util
import dev_bleu_ref
import meteor_ref as R
from search_kit import count_calls, golden_search, offset_rows, outside_untouched
from fira_icse_amd import _lib, data, devset, metrics, ops
from fira_icse_amd.config import FiraConfig

pytestmark = pytest.mark.gpu

dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
DEV_SHAPE = (12, 7, 5)                      # V, L, S


# ------------------------------------------------------------------------------------------------ the dev kernel
@pytest.fixture(scope="module")
def dev_cases():
    """Per T the 13 rows, the class table and the oracle's rows without and with it; computed once, left unchanged."""
    V, L, S = DEV_SHAPE
    out = {}
    for T in (1, 30, 64):
        rows = R.dev_rows(T, V, L, S, seed=T)
        table = R.merging_table(V, seed=T)
        want = {name: np.array([R.dev_stats_ref(*[a[b] for a in rows], V, L, S, cls) for b in range(R.DEV_B)], dtype=np.int32)
                for name, cls in (("exact", None), ("classes", table))}
        out[T] = (rows, table, want)
    return out


def test_dev_rows_hold_what_the_issue_names(dev_cases):
    (ids, sou, sub, tar), table, want = dev_cases[64]
    ex, cl = want["exact"], want["classes"]
    assert ex[0].tolist()[2:] == [64, 63] and ex[0, 0] > 40                              # a hypothesis in all 64 positions
    assert ex[1].tolist() == [0, 0, 0, 2] and ex[2].tolist() == [0, 0, 2, 0]             # an empty hypothesis, an empty reference
    assert ex[3].tolist() == [3, 3, 64, 6]                                               # one word 64 times against 3 occurrences
    assert ex[4].tolist() == [5, 1, 6, 6]                                                # copies resolved; the copied <unkm> unmatched
    assert ex[5].tolist() == [2, 2, 4, 4] and cl[5, 0] <= 3                              # <unkm> matches nothing, with classes neither
    assert ex[6].tolist() == [5, 5, 8, 5] and ex[7].tolist() == [3, 3, 3, 3]
    assert (cl[:, 0] > ex[:, 0]).any() and (cl[:, 0] >= ex[:, 0]).all() and np.array_equal(cl[:, 2:], ex[:, 2:])
    assert (ids >= DEV_SHAPE[0]).any() and (ids >= DEV_SHAPE[0] + DEV_SHAPE[1]).any()
    assert dev_cases[30][2]["exact"][3].tolist() == [3, 3, 30, 6] and dev_cases[1][2]["exact"][:, 3].max() == 0


@pytest.mark.parametrize("T", [1, 30, 64])
@pytest.mark.parametrize("B", [1, 5, 13])
def test_dev_kernel_is_exactly_the_two_loop_oracle(dev_cases, T, B):
    V, L, S = DEV_SHAPE
    rows, table, want = dev_cases[T]
    for lo in range(0, R.DEV_B - B + 1, B):                                              # B = 1: every row alone
        part = [dev(a[lo:lo + B]) for a in rows]
        rouge = ops.dev_rouge_l_stats(*part, V).cpu().numpy()
        for name, cls in (("exact", None), ("classes", table)):
            guard = torch.full((B + 2, 4), 77, dtype=torch.int32, device="cuda")
            got = ops.dev_meteor_stats(*part, V, classes=dev(cls), stats=guard[1:B + 1]).cpu().numpy()
            assert np.array_equal(got, want[name][lo:lo + B]), (name, lo, np.argwhere(got != want[name][lo:lo + B])[:5])
            assert bool((guard[0] == 77).all()) and bool((guard[B + 1] == 77).all())
            assert np.array_equal(got[:, 2:4], rouge[:, 1:3])                            # the lengths the ROUGE-L kernel reports


def test_dev_kernel_refusals_and_no_commits():
    V, L, S = DEV_SHAPE
    T = 30
    lib, s, p = _lib.lib(), _lib.cur_stream(), _lib.ptr
    ids, sou, sub, tar = [dev(a[:2]) for a in R.dev_rows(T, V, L, S, seed=T)]
    cls = dev(R.merging_table(V))
    guard = torch.full((2, 4), 77, dtype=torch.int32, device="cuda")
    a = (p(ids), p(sou), p(sub), p(tar), p(cls), p(guard))
    assert lib.fira_dev_meteor_stats(s, 0, T, V, L, S, *a) == 0
    assert lib.fira_dev_meteor_stats(s, 0, T, V, L, S, None, None, None, None, None, None) == 0
    for args, word in (((1, 65, V, L, S) + a, b"T = 65"), ((1, 0, V, L, S) + a, b"T = 0"), ((1, T, 3, L, S) + a, b"V = 3"),
                       ((1, T, V, 0, S) + a, b"L = 0"), ((1, T, V, L, 0) + a, b"S = 0"), ((-1, T, V, L, S) + a, b"B = -1"),
                       ((1, T, V, L, S) + a[:5] + (None,), b"null pointer"), ((1, T, V, L, S, None) + a[1:], b"null pointer")):
        assert lib.fira_dev_meteor_stats(s, *args) != 0, args
        assert word in lib.fira_last_error() and b"fira_dev_meteor_stats" in lib.fira_last_error(), lib.fira_last_error()
    torch.cuda.synchronize()
    assert bool((guard == 77).all())
    e = torch.empty((0, T), dtype=torch.int32, device="cuda")
    s0 = ops.dev_meteor_stats(e, torch.empty((0, L), dtype=torch.int32, device="cuda"),
                              torch.empty((0, S), dtype=torch.int32, device="cuda"), e.clone(), V, classes=cls)
    assert tuple(s0.shape) == (0, 4)


# ------------------------------------------------------------------------------------------------ the all-pairs kernel
@pytest.fixture(scope="module")
def pair_cases():
    """The case sets with the class table and the oracle's rows without and with it; computed once, left unchanged."""
    table = R.merging_table(R.PAIR_V)
    return table, [(tokens, length, {"exact": R.stats_ref_all(tokens, length), "classes": R.stats_ref_all(tokens, length, table)})
                   for tokens, length in R.all_pair_cases()]


@pytest.mark.parametrize("k", range(len(R.PAIR_SHAPES)), ids=["B%d_n%d_T%d" % s for s in R.PAIR_SHAPES])
def test_all_pairs_kernel_is_exactly_the_two_loop_oracle(pair_cases, k):
    table, cases = pair_cases
    tokens, length, want = cases[k]
    B, n, T = R.PAIR_SHAPES[k]
    assert tokens.shape == (B, n, T)
    t, l, count = dev(tokens), dev(length), B * n * n * 4
    for offset, (name, cls) in zip((0, 1, 2, 3), (("exact", None), ("classes", table)) * 2):
        buf, view = offset_rows(np.zeros((B * n * n, 4), dtype=np.float32), offset, fill=77.0)
        stats = view.view(torch.int32).view(B, n, n, 4)
        ops.mbr_meteor_stats(t, l, classes=dev(cls), stats=stats)
        got = stats.cpu().numpy()
        assert np.array_equal(got, want[name]), (name, offset, np.argwhere(got != want[name])[:5])
        assert outside_untouched(buf, offset, count, fill=77.0)
    d = want["exact"][:, np.arange(n), np.arange(n)]                                     # the diagonal: (len, len > 0, len, len)
    assert np.array_equal(d[..., 1], (d[..., 0] > 0).astype(np.int32)) and np.array_equal(d[..., 0], d[..., 3])
    if n > 2:
        assert (want["classes"][..., 0] > want["exact"][..., 0]).any()
    for b in range(B):                                                                   # commits do not depend on their neighbours
        one = ops.mbr_meteor_stats(dev(tokens[b:b + 1]), dev(length[b:b + 1]), classes=dev(table)).cpu().numpy()
        assert np.array_equal(one[0], want["classes"][b]), b


def test_all_pairs_kernel_refusals_and_no_commits():
    t = torch.zeros((1, 8, 30), dtype=torch.int32, device="cuda")
    l = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    cls = dev(R.merging_table(R.PAIR_V))
    stats = torch.full((1, 8, 8, 4), 77, dtype=torch.int32, device="cuda")
    lib, s, p = _lib.lib(), _lib.cur_stream(), _lib.ptr
    V = R.PAIR_V
    assert lib.fira_mbr_meteor_stats(s, 0, 8, 30, p(t), p(l), V, p(cls), p(stats)) == 0
    assert lib.fira_mbr_meteor_stats(s, 0, 8, 30, None, None, 0, None, None) == 0
    for args, word in (((1, 33, 30, p(t), p(l), V, p(cls), p(stats)), b"n = 33"), ((1, 0, 30, p(t), p(l), V, p(cls), p(stats)), b"n = 0"),
                       ((1, 8, 65, p(t), p(l), V, p(cls), p(stats)), b"T = 65"), ((1, 8, 0, p(t), p(l), V, p(cls), p(stats)), b"T = 0"),
                       ((-1, 8, 30, p(t), p(l), V, p(cls), p(stats)), b"B = -1"), ((1, 8, 30, p(t), p(l), 3, p(cls), p(stats)), b"V = 3"),
                       ((1, 8, 30, None, p(l), V, p(cls), p(stats)), b"null pointer"),
                       ((1, 8, 30, p(t), None, 0, None, p(stats)), b"null pointer"),
                       ((1, 8, 30, p(t), p(l), 0, None, None), b"null pointer")):
        assert lib.fira_mbr_meteor_stats(s, *args) != 0, args
        assert word in lib.fira_last_error() and b"fira_mbr_meteor_stats" in lib.fira_last_error(), lib.fira_last_error()
    torch.cuda.synchronize()
    assert bool((stats == 77).all())
    s0 = ops.mbr_meteor_stats(torch.empty((0, 8, 30), dtype=torch.int32, device="cuda"),
                              torch.empty((0, 8), dtype=torch.int32, device="cuda"))
    assert tuple(s0.shape) == (0, 8, 8, 4)


# ------------------------------------------------------------------------------------------------ Searcher.mbr
@pytest.fixture(scope="module")
def sampled():
    g = golden_search(weights="spread")
    search, db = g.searchers[0], g.db
    draws = [search.sample(db, 4, temperature=1.3, top_k=30, seed=seed) for seed in (5, 6)]
    return search, draws


def host_loop(toks, lens, classes=None):
    """Expected ``meteor_exact`` by ``metrics.meteor_exact`` on the candidates' words, written out here."""
    toks, lens = toks.cpu().tolist(), lens.cpu().tolist()
    word_class = None if classes is None else {"w%d" % i: c for i, c in enumerate(classes)}
    out = []
    for rows, ns in zip(toks, lens):
        ws = [["w%d" % t for t in R.words(row, k)] for row, k in zip(rows, ns)]
        n = len(ws)
        out.append([math.fsum(metrics.meteor_exact(ws[j], ws[i], word_class) for j in range(n) if j != i) / (n - 1)
                    if n > 1 else 0.0 for i in range(n)])
    return out


def check_mbr(search, toks, lens, logp, classes=None):
    pick, util_ = search.mbr(toks, lens, logp, utility="meteor_exact", classes=classes)
    B, n, _ = toks.shape
    want = host_loop(toks, lens, None if classes is None else [int(c) for c in classes])
    assert util_.dtype == torch.float64 and tuple(util_.shape) == (B, n) and not util_.is_cuda
    assert util_.tolist() == want
    assert pick == R.pick_ref(want, logp.tolist())                                       # ties: the larger logp, then the lower index
    assert search.mbr(toks, lens, utility="meteor_exact", classes=classes)[0] == R.pick_ref(want)
    return pick, want


def test_searcher_mbr_by_meteor_exact_on_sampled_candidates(sampled):
    search, draws = sampled
    (toks, lens, _, logp), (toks2, lens2, _, logp2) = draws
    B, V = toks.shape[0], search.cfg.vocab_size
    pick, want = check_mbr(search, toks, lens, logp)
    assert any(u > 0 for row in want for u in row) and any(len(set(row)) > 1 for row in want)
    pooled = (torch.cat([toks, toks2], 1), torch.cat([lens, lens2], 1), torch.cat([logp, logp2], 1))
    assert pooled[0].shape[1] == 8
    pick8, want8 = check_mbr(search, *pooled)
    table = R.merging_table(V, seed=2, n_classes=7)
    _, want_c = check_mbr(search, *pooled, classes=torch.from_numpy(table))
    check_mbr(search, *pooled, classes=table.tolist())                                   # a plain sequence
    assert want_c != want8
    # a tie in utility: two copies of one candidate set; the copy with the larger logp wins, then the lower index
    twice = (torch.cat([toks, toks], 1), torch.cat([lens, lens], 1), torch.cat([logp, logp + 1.0], 1))
    assert all(p >= 4 for p in check_mbr(search, *twice)[0])
    assert all(p < 4 for p in search.mbr(twice[0], twice[1], torch.cat([logp, logp], 1), utility="meteor_exact")[0])
    print("picks by meteor_exact", pick8, "by ROUGE-L", search.mbr(*pooled, utility="rouge_l")[0], "by BLEU", search.mbr(*pooled)[0])
    p1, u1 = search.mbr(toks[:, :1], lens[:, :1], logp[:, :1], utility="meteor_exact")
    assert p1 == [0] * B and u1.tolist() == [[0.0]] * B
    assert search.mbr(toks.int().cpu(), lens.int().cpu(), logp.cpu(), utility="meteor_exact")[0] == pick


def test_searcher_mbr_refuses_bad_arguments_with_no_library_call(sampled, monkeypatch):
    search, draws = sampled
    toks, lens, _, logp = draws[0]
    V = search.cfg.vocab_size
    table = torch.from_numpy(R.merging_table(V))

    def refusals():
        for args in ((toks[0], lens[0]), (toks, lens[:, :3]), (toks.repeat(1, 9, 1), lens.repeat(1, 9)),
                     (torch.cat([toks, toks, toks], 2), lens), (toks[:, :, :0], lens), (toks.float(), lens),
                     (toks, lens.float()), (toks, lens, logp[:, :2])):
            with pytest.raises(ValueError):
                search.mbr(*args, utility="meteor_exact")
        for bad in (table[:-1], torch.cat([table, table[:1]]), table.float(), table.view(1, -1), table.long() + (1 << 40)):
            with pytest.raises(ValueError, match="classes"):
                search.mbr(toks, lens, logp, utility="meteor_exact", classes=bad)
        for other in ("bleu", "rouge_l"):
            with pytest.raises(ValueError, match="classes"):
                search.mbr(toks, lens, logp, utility=other, classes=table)
        for bad in ("meteor", "METEOR", "meteor_exact ", None):
            with pytest.raises(ValueError, match="utility"):
                search.mbr(toks, lens, logp, utility=bad)

    assert count_calls(monkeypatch, refusals) == {}


def test_other_utilities_launch_what_they_launched(sampled, monkeypatch):
    search, draws = sampled
    toks, lens, _, logp = draws[0]
    out = {}
    calls = count_calls(monkeypatch, lambda: out.update(kw=search.mbr(toks, lens, logp, utility="bleu")))
    assert calls == {"fira_mbr_bleu_stats": 1}
    assert count_calls(monkeypatch, lambda: out.update(plain=search.mbr(toks, lens, logp))) == calls
    assert out["kw"][0] == out["plain"][0] and torch.equal(out["kw"][1], out["plain"][1])
    assert count_calls(monkeypatch, lambda: search.mbr(toks, lens, logp, utility="rouge_l")) == {"fira_mbr_rouge_l_stats": 1}
    assert count_calls(monkeypatch, lambda: search.mbr(toks, lens, logp, utility="meteor_exact")) == {"fira_mbr_meteor_stats": 1}


# ------------------------------------------------------------------------------------------------ DevEvaluator
def test_dev_evaluator_with_meteor_exact_on_the_golden_commits(monkeypatch):
    from fira_icse_amd.model import TransModel
    raw = util.load_golden_raw()
    cfg = FiraConfig(batch_size=8)
    store = data.process_raw(cfg, raw)
    r_vocab = {i: w for w, i in raw["word_vocab"].items()}
    n = len(store)
    torch.manual_seed(0)
    model = TransModel(cfg)
    model.eval()
    table = dev_bleu_ref.label_ids_table(store, cfg, seed=0)
    make = lambda **kw: devset.DevEvaluator(model, store, cfg, r_vocab, raw["variable"], list(range(n)),
                                            ids_fn=dev_bleu_ref.table_ids_fn(table), **kw)
    classes = R.merging_table(cfg.vocab_size, seed=1, n_classes=5)
    plain, ev, ev_c = make(rouge_l=True), make(rouge_l=True, meteor_exact=True), make(meteor_exact=True, meteor_classes=classes)
    p_total, p_lines = plain.device_pass()
    assert plain.last_meteor_exact == [] and n == util.GOLDEN_N
    stat_calls = lambda calls: {k: v for k, v in calls.items() if k.endswith("_stats")}
    for e in (ev, ev_c):
        h_total, h_lines = e.host_pass()
        h_meteor, h_rouge = list(e.last_meteor_exact), list(e.last_rouge_l)
        e.device_pass()                                                                  # (builds the resident set)
        out = {}
        calls = count_calls(monkeypatch, lambda: out.update(r=e.device_pass()))
        d_total, d_lines = out["r"]
        assert len(h_meteor) == n and e.last_meteor_exact == h_meteor and sum(v > 0 for v in h_meteor) >= n // 2
        assert d_total == h_total == p_total and d_lines() == h_lines() == p_lines() and e.last_scores == plain.last_scores
        assert e.last_rouge_l == h_rouge == (plain.last_rouge_l if e.rouge_l else [])
        want_calls = {"fira_dev_bleu_stats": 3, "fira_dev_meteor_stats": 3}
        if e.rouge_l:
            want_calls["fira_dev_rouge_l_stats"] = 3
        assert stat_calls(calls) == want_calls
    assert ev_c.last_meteor_exact != ev.last_meteor_exact
    calls_p = count_calls(monkeypatch, plain.device_pass)
    assert stat_calls(calls_p) == {"fira_dev_bleu_stats": 3, "fira_dev_rouge_l_stats": 3}
    T = cfg.tar_len
    assert plain._out.numel() == n * (16 + T) and ev._out.numel() == n * (20 + T) and ev_c._out.numel() == n * (16 + T)
    print("mean meteor_exact %.4f (with classes %.4f), mean BLEU %.4f over %d commits"
          % (sum(ev.last_meteor_exact) / n, sum(ev_c.last_meteor_exact) / n, p_total / n, n))
