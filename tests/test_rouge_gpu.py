"""ROUGE-L on the device: the all-pairs LCS kernel against its DP oracle (exact), the dev kernel against the string oracle and
against the BLEU kernel's lengths, ``Searcher.mbr(..., utility="rouge_l")`` against the host loop over ``metrics.rouge_l``
(``==``), and ``DevEvaluator(rouge_l=True)``: the device pass against the host pass."""
import math

import numpy as np
import pytest
import torch

import dev_bleu_ref
import rouge_ref as R
from search_kit import count_calls, golden_search
from fira_icse_amd import _lib, devset, metrics, ops
from fira_icse_amd.config import EOS, PAD, START, UNK

pytestmark = pytest.mark.gpu

dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_kernel(tokens, length):
    return ops.mbr_rouge_l_stats(dev(tokens), dev(length)).cpu().numpy()


@pytest.fixture(scope="module")
def case_list():
    """The case sets with their oracle rows, computed once and left unchanged."""
    cases = R.all_cases()
    R.check_cases(cases)
    return [(tokens, length, R.stats_ref_all(tokens, length)) for tokens, length in cases]


@pytest.mark.parametrize("k", range(len(R.SHAPES)), ids=["B%d_n%d_T%d" % s for s in R.SHAPES])
def test_kernel_is_exactly_the_dp_oracle(case_list, k):
    tokens, length, want = case_list[k]
    assert tokens.shape == R.SHAPES[k]
    n = tokens.shape[1]
    stats = run_kernel(tokens, length)
    assert stats.shape == want.shape and stats.dtype == np.int32
    assert np.array_equal(stats, want), np.argwhere(stats != want)[:5]
    diag = stats[:, np.arange(n), np.arange(n)]
    assert np.array_equal(diag[:, :, 0], diag[:, :, 1]) and np.array_equal(diag[:, :, 1], diag[:, :, 2])
    assert not stats[..., 3].any()
    assert np.array_equal(stats[..., 0], stats[..., 0].transpose(0, 2, 1))
    assert np.array_equal(stats[..., 1], stats[..., 2].transpose(0, 2, 1))


def test_kernel_rows_do_not_depend_on_their_neighbours(case_list):
    for tokens, length, want in case_list[2:4] + case_list[6:]:
        for b in range(tokens.shape[0]):
            assert np.array_equal(run_kernel(tokens[b:b + 1], length[b:b + 1])[0], want[b]), b


def test_kernel_ignores_what_lies_behind_a_length(case_list):
    for tokens, length, want in case_list:
        other = R.regarbage(tokens, length, seed=99)
        behind = np.arange(tokens.shape[2])[None, None, :] >= length[:, :, None]
        assert np.array_equal(other[~behind], tokens[~behind])
        if behind.any():
            assert (other[behind] != tokens[behind]).any()
        assert np.array_equal(run_kernel(other, length), want)


def test_kernel_with_no_commits_writes_nothing(case_list):
    tokens, length, _ = case_list[1]
    _, n, T = tokens.shape
    t, l = dev(tokens), dev(length)
    stats = torch.full((2, n, n, 4), 77, dtype=torch.int32, device="cuda")
    rc = _lib.lib().fira_mbr_rouge_l_stats(_lib.cur_stream(), 0, n, T, _lib.ptr(t), _lib.ptr(l), _lib.ptr(stats))
    torch.cuda.synchronize()
    assert rc == 0 and bool((stats == 77).all())
    assert _lib.lib().fira_mbr_rouge_l_stats(_lib.cur_stream(), 0, n, T, None, None, None) == 0
    s0 = ops.mbr_rouge_l_stats(torch.empty((0, n, T), dtype=torch.int32, device="cuda"),
                               torch.empty((0, n), dtype=torch.int32, device="cuda"))
    assert tuple(s0.shape) == (0, n, n, 4)


def test_kernel_refuses_what_it_cannot_serve():
    t = torch.zeros((1, 8, 30), dtype=torch.int32, device="cuda")
    l = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    stats = torch.full((1, 8, 8, 4), 77, dtype=torch.int32, device="cuda")
    lib, s = _lib.lib(), _lib.cur_stream()
    p = _lib.ptr
    for args, word in (((1, 33, 30, p(t), p(l), p(stats)), b"n = 33"), ((1, 0, 30, p(t), p(l), p(stats)), b"n = 0"),
                       ((1, 8, 65, p(t), p(l), p(stats)), b"T = 65"), ((1, 8, 0, p(t), p(l), p(stats)), b"T = 0"),
                       ((-1, 8, 30, p(t), p(l), p(stats)), b"B = -1"), ((1, 8, 30, None, p(l), p(stats)), b"null pointer"),
                       ((1, 8, 30, p(t), None, p(stats)), b"null pointer"), ((1, 8, 30, p(t), p(l), None), b"null pointer")):
        assert lib.fira_mbr_rouge_l_stats(s, *args) != 0, args
        assert word in lib.fira_last_error() and b"fira_mbr_rouge_l_stats" in lib.fira_last_error(), lib.fira_last_error()
    torch.cuda.synchronize()
    assert bool((stats == 77).all())
    with pytest.raises(_lib.FiraError, match="n = 33"):
        ops.mbr_rouge_l_stats(torch.zeros((1, 33, 30), dtype=torch.int32, device="cuda"),
                              torch.zeros((1, 33), dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------------------------ the dev kernel
def crafted_rows(T, V, L, S):
    """(ids, tar, sou, sub) rows for the properties the seeded rows need not hold."""
    pad = lambda row: row + [PAD] * (T - len(row))
    return [
        ([5, 6, 7, 8] * (T // 4) + [5] * (T % 4), pad([START, 5, 7, 8, 6, EOS]), None, None),       # no <eos> in ids
        (pad([EOS, 5, 6]), pad([START, 5, 6, EOS]), None, None),                                     # <eos> at 0: empty hypothesis
        (pad([5, V + L + S + 9, 6, EOS]), pad([START, 5, 9, 6, 4, EOS]), None, [5] * (S - 1) + [9]),   # an id out of range: clamped
        (pad([UNK, 5, UNK, EOS]), pad([START, UNK, 5, UNK, EOS]), None, None),                       # <unkm> never matches <unkm>
        (pad([V, 5, EOS]), pad([START, UNK, 5, EOS]), [UNK] + [5] * (L - 1), None),                  # ... nor does a copied one
        ([7] * T, [START] + [7] * (T - 1), None, None),                                              # one word, every bit
        ([9] + [5] * (T - 1), [START] + [6] * (T - 3) + [9, EOS], None, None),        # the only match: first word against last
    ]


def dev_inputs(B, T, V, L, S, seed):
    ids, sou, sub, tar = dev_bleu_ref.kernel_cases(B, T, V, L, S, seed)
    ids, sou, sub, tar = ids.copy(), sou.copy(), sub.copy(), tar.copy()
    for k, (i_row, t_row, so_row, su_row) in enumerate(crafted_rows(T, V, L, S)):
        b = B - 1 - k
        ids[b], tar[b] = i_row, t_row
        if so_row is not None:
            sou[b] = so_row
        if su_row is not None:
            sub[b] = su_row
    return ids, sou, sub, tar


@pytest.mark.parametrize("T,V", [(30, 12), (64, 90)], ids=["T30", "T64"])
def test_dev_kernel_is_the_string_oracle_and_has_the_bleu_kernels_lengths(T, V):
    L, S, B = 7, 5, 37                                                  # 37: a workgroup with one live wave at the end
    ids, sou, sub, tar = dev_inputs(B, T, V, L, S, seed=4)
    in_range = np.minimum(ids, V + L + S - 1)                           # the kernel's rule for an id past the last copy entry
    assert (in_range != ids).sum() == 1
    want = np.array([R.dev_stats_ref(in_range[b], sou[b], sub[b], tar[b], V, L, S) for b in range(B)], dtype=np.int32)
    assert (want[:, 0] < np.minimum(want[:, 1], want[:, 2])).any() and (want[:, 0] > 3).any()
    assert want[B - 4].tolist() == [1, 3, 3, 0] and want[B - 5].tolist() == [1, 2, 2, 0] and want[B - 2, 0] == 0
    assert want[B - 6].tolist() == [T - 1, T, T - 1, 0] and want[B - 7].tolist() == [1, T, T - 2, 0]
    assert want[B - 3].tolist() == [3, 3, 4, 0]
    guard = torch.full((B + 2, 4), 77, dtype=torch.int32, device="cuda")
    stats = ops.dev_rouge_l_stats(dev(ids), dev(sou), dev(sub), dev(tar), V, stats=guard[1:B + 1])
    got = stats.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert bool((guard[0] == 77).all()) and bool((guard[B + 1] == 77).all())
    _, bleu = ops.dev_bleu_stats(dev(ids), dev(sou), dev(sub), dev(tar), V)
    assert np.array_equal(got[:, 1:3], bleu.cpu().numpy()[:, 8:10])
    if T == 64:
        assert int(want[:, 1].max()) == 64
    for b in (0, B - 3, B - 1):                                          # rows do not depend on their neighbours
        one = ops.dev_rouge_l_stats(dev(ids[b:b + 1]), dev(sou[b:b + 1]), dev(sub[b:b + 1]), dev(tar[b:b + 1]), V)
        assert np.array_equal(one.cpu().numpy(), want[b:b + 1])


def test_dev_kernel_on_the_golden_commits_and_its_refusals():
    g = golden_search()
    cfg, db = g.cfg, g.db
    V, L, S, T = cfg.vocab_size, cfg.sou_len, cfg.sub_token_len, cfg.tar_len
    ids = g.model.forward_dev(db)
    db.wait_ready()
    got = ops.dev_rouge_l_stats(ids, db.sou, db.sub_token, db.tar, V).cpu().numpy()
    h = [t.cpu().numpy() for t in (ids, db.sou, db.sub_token, db.tar)]
    r_vocab = {i: "w%d" % i for i in range(4, V)}
    r_vocab.update(dev_bleu_ref.toy_r_vocab(4))
    want = [R.dev_stats_ref(h[0][b], h[1][b], h[2][b], h[3][b], V, L, S, r_vocab) for b in range(db.B)]
    assert got.tolist() == want
    # no commits: nothing written, null pointers accepted; refusals name their value and leave the buffer alone
    lib, s, p = _lib.lib(), _lib.cur_stream(), _lib.ptr
    guard = torch.full((db.B, 4), 77, dtype=torch.int32, device="cuda")
    a = (p(ids), p(db.sou), p(db.sub_token), p(db.tar), p(guard))
    assert lib.fira_dev_rouge_l_stats(s, 0, T, V, L, S, *a) == 0
    assert lib.fira_dev_rouge_l_stats(s, 0, T, V, L, S, None, None, None, None, None) == 0
    for args, word in (((1, 65, V, L, S) + a, b"T = 65"), ((1, 0, V, L, S) + a, b"T = 0"), ((1, T, 3, L, S) + a, b"V = 3"),
                       ((1, T, V, 0, S) + a, b"L = 0"), ((1, T, V, L, 0) + a, b"S = 0"), ((-1, T, V, L, S) + a, b"B = -1"),
                       ((1, T, V, L, S) + a[:4] + (None,), b"null pointer"), ((1, T, V, L, S, None) + a[1:], b"null pointer")):
        assert lib.fira_dev_rouge_l_stats(s, *args) != 0, args
        assert word in lib.fira_last_error() and b"fira_dev_rouge_l_stats" in lib.fira_last_error(), lib.fira_last_error()
    torch.cuda.synchronize()
    assert bool((guard == 77).all())
    e = torch.empty((0, T), dtype=torch.int32, device="cuda")
    s0 = ops.dev_rouge_l_stats(e, torch.empty((0, L), dtype=torch.int32, device="cuda"),
                               torch.empty((0, S), dtype=torch.int32, device="cuda"), e.clone(), V)
    assert tuple(s0.shape) == (0, 4)


# ------------------------------------------------------------------------------------------------ Searcher.mbr
@pytest.fixture(scope="module")
def sampled():
    g = golden_search(weights="spread")
    search, db = g.searchers[0], g.db
    draws = [search.sample(db, 4, temperature=1.3, top_k=30, seed=seed) for seed in (5, 6)]
    return search, draws


def host_loop(toks, lens):
    """Expected ROUGE-L by ``metrics.rouge_l`` on the candidates' words, written out here."""
    toks, lens = toks.cpu().tolist(), lens.cpu().tolist()
    out = []
    for rows, ns in zip(toks, lens):
        ws = [["w%d" % t for t in R.words(row, k)] for row, k in zip(rows, ns)]
        n = len(ws)
        out.append([math.fsum(metrics.rouge_l(ws[j], ws[i]) for j in range(n) if j != i) / (n - 1) if n > 1 else 0.0
                    for i in range(n)])
    return out


def check_mbr(search, toks, lens, logp):
    pick, util_ = search.mbr(toks, lens, logp, utility="rouge_l")
    B, n, _ = toks.shape
    want = host_loop(toks, lens)
    assert util_.dtype == torch.float64 and tuple(util_.shape) == (B, n) and not util_.is_cuda
    assert util_.tolist() == want
    assert pick == R.pick_ref(want, logp.tolist())
    assert search.mbr(toks, lens, utility="rouge_l")[0] == R.pick_ref(want)
    return pick, want


def test_searcher_mbr_by_rouge_l_on_sampled_candidates(sampled):
    search, draws = sampled
    (toks, lens, _, logp), (toks2, lens2, _, logp2) = draws
    B = toks.shape[0]
    pick, want = check_mbr(search, toks, lens, logp)
    assert any(u > 0 for row in want for u in row) and any(len(set(row)) > 1 for row in want)
    pooled = (torch.cat([toks, toks2], 1), torch.cat([lens, lens2], 1), torch.cat([logp, logp2], 1))
    assert pooled[0].shape[1] == 8
    pick8, _ = check_mbr(search, *pooled)
    print("picks by ROUGE-L", pick8, "by BLEU", search.mbr(*pooled)[0])
    p1, u1 = search.mbr(toks[:, :1], lens[:, :1], logp[:, :1], utility="rouge_l")
    assert p1 == [0] * B and u1.tolist() == [[0.0]] * B
    assert search.mbr(toks.int().cpu(), lens.int().cpu(), logp.cpu(), utility="rouge_l")[0] == pick


def test_searcher_mbr_refuses_bad_arguments_before_any_launch(sampled, monkeypatch):
    search, draws = sampled
    toks, lens, _, logp = draws[0]
    launched = []
    monkeypatch.setattr(ops, "mbr_rouge_l_stats", lambda *a, **k: launched.append(1))
    monkeypatch.setattr(ops, "mbr_bleu_stats", lambda *a, **k: launched.append(1))
    for args in ((toks[0], lens[0]), (toks, lens[:, :3]), (toks.repeat(1, 9, 1), lens.repeat(1, 9)),
                 (torch.cat([toks, toks, toks], 2), lens), (toks[:, :, :0], lens), (toks.float(), lens),
                 (toks, lens.float()), (toks + (1 << 40), lens), (toks, lens, logp[:, :2])):
        with pytest.raises(ValueError):
            search.mbr(*args, utility="rouge_l")
    for bad in ("rouge", "meteor", None):
        with pytest.raises(ValueError, match="utility"):
            search.mbr(toks, lens, logp, utility=bad)
    assert not launched


def test_default_utility_launches_what_it_launched(sampled, monkeypatch):
    search, draws = sampled
    toks, lens, _, logp = draws[0]
    out = {}
    calls = count_calls(monkeypatch, lambda: out.update(kw=search.mbr(toks, lens, logp, utility="bleu")))
    assert calls.get("fira_mbr_bleu_stats") == 1 and calls.get("fira_mbr_rouge_l_stats", 0) == 0
    calls0 = count_calls(monkeypatch, lambda: out.update(plain=search.mbr(toks, lens, logp)))
    assert calls0 == calls
    assert out["kw"][0] == out["plain"][0] and torch.equal(out["kw"][1], out["plain"][1])
    calls_r = count_calls(monkeypatch, lambda: search.mbr(toks, lens, logp, utility="rouge_l"))
    assert calls_r.get("fira_mbr_rouge_l_stats") == 1 and calls_r.get("fira_mbr_bleu_stats", 0) == 0


# ------------------------------------------------------------------------------------------------ DevEvaluator
def test_dev_evaluator_with_rouge_l(monkeypatch):
    from fira_icse_amd.model import TransModel
    cfg, store, r_vocab, var_maps, valid_index = dev_bleu_ref.synthetic_valid(23, 8)
    torch.manual_seed(0)
    model = TransModel(cfg)
    model.eval()
    table = dev_bleu_ref.label_ids_table(store, cfg, seed=0)
    make = lambda **kw: devset.DevEvaluator(model, store, cfg, r_vocab, var_maps, valid_index,
                                            ids_fn=dev_bleu_ref.table_ids_fn(table), **kw)
    plain, ev = make(), make(rouge_l=True)
    p_total, p_lines = plain.device_pass()
    assert plain.last_rouge_l == []
    h_total, h_lines = ev.host_pass()
    h_rouge = list(ev.last_rouge_l)
    ev.device_pass()                                                    # (builds the resident set)
    out = {}
    stat_calls = lambda calls: {k: v for k, v in calls.items() if k.endswith("_stats")}
    calls = count_calls(monkeypatch, lambda: out.update(r=ev.device_pass()))
    d_total, d_lines = out["r"]
    assert len(h_rouge) == 23 and ev.last_rouge_l == h_rouge and sum(v > 0 for v in h_rouge) >= 12
    assert d_total == h_total == p_total and d_lines() == h_lines() == p_lines() and ev.last_scores == plain.last_scores
    assert stat_calls(calls) == {"fira_dev_bleu_stats": 3, "fira_dev_rouge_l_stats": 3}
    calls_p = count_calls(monkeypatch, plain.device_pass)
    assert stat_calls(calls_p) == {"fira_dev_bleu_stats": 3} and set(calls) - set(calls_p) == {"fira_dev_rouge_l_stats"}
    assert plain._out.numel() == 23 * (12 + cfg.tar_len) and ev._out.numel() == 23 * (16 + cfg.tar_len)
    print("mean ROUGE-L %.4f, mean BLEU %.4f over 23 commits" % (sum(h_rouge) / 23, h_total / 23))
