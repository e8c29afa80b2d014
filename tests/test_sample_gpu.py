"""On-device sampling (fira_decode_step_sample / fira_sample_advance / Searcher.sample): the distribution row it forms is
the decode step's, bit for bit; the draw is the Gumbel-max of the numpy twin (sample_ref.py) over the filtered set; the
draws follow the filtered distribution; replay, eager launches and seeds behave; the bookkeeping and the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import sample_ref
import util
from search_kit import golden_search, run_cli, seed_tensor, spread_state_dict
from fira_icse_amd import _lib, synth
from fira_icse_amd.config import FiraConfig

pytestmark = pytest.mark.gpu

FILTERS = [(1.0, 0, 1.0), (1.7, 0, 1.0), (1.0, 1, 1.0), (1.3, 5, 1.0), (1.0, 50, 1.0), (1.0, 0, 0.5), (0.8, 0, 0.9),
           (1.5, 50, 0.9)]


@pytest.fixture(scope="module")
def setup():
    from fira_icse_amd.model import TransModel
    g = golden_search(weights="peaked", searchers=0, seed=2)
    spread = TransModel(g.cfg, init=False)
    spread.load_state_dict(spread_state_dict(g.cfg))
    spread.eval()
    return g.cfg, g.store, g.ids, g.model, spread, g.db


def step_sample(search, ws, B, n, step, tok, key, seed, T, k, p, dist, best_id, best_p, flags=0):
    m = search.model
    _lib.check(_lib.lib().fira_decode_step_sample(_lib.cur_stream(), C.byref(m.dims), _lib.ptr(m.flat.data), _lib.ptr(ws),
                                                  ws.numel(), B, n, step, _lib.ptr(tok), _lib.ptr(key), _lib.ptr(seed),
                                                  float(T), int(k), float(p), _lib.ptr(dist), _lib.ptr(best_id),
                                                  _lib.ptr(best_p), flags), "fira_decode_step_sample")


def test_step_dist_is_the_decode_steps_and_the_draw_is_the_twins(setup):
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, db = setup
    search = Searcher(spread)
    B, W, T = db.B, cfg.out_len, cfg.tar_len
    ws = search._begin(db, 1)
    key = torch.tensor([7, 11, 13, 17], dtype=torch.int32, device="cuda")[:B]
    seed = seed_tensor(0x1234567890ABCDEF)
    dist_a = torch.empty(B, W, device="cuda")
    dist_b = torch.empty(B, W, device="cuda")
    bid = torch.empty(B, dtype=torch.int32, device="cuda")
    bp = torch.empty(B, device="cuda")
    gen = torch.Generator().manual_seed(5)
    checked = 0
    for step in range(6):
        tok = torch.randint(4, 3000, (B,), generator=gen).to(torch.int32).cuda() if step else \
            torch.full((B,), 2, dtype=torch.int32, device="cuda")
        search._step(ws, B, 1, step, tok, None, dist_a, None, None)
        if step not in (0, 1, 5):
            continue
        for (temp, k, p) in FILTERS:
            step_sample(search, ws, B, 1, step, tok, key, seed, temp, k, p, dist_b, bid, bp)
            torch.cuda.synchronize()
            assert torch.equal(dist_a.view(torch.int32), dist_b.view(torch.int32)), (step, temp, k, p)
            ids_ = bid.long()
            assert torch.equal(bp.view(torch.int32), dist_b[torch.arange(B), ids_].contiguous().view(torch.int32))
            d = dist_b.double().cpu().numpy()
            for r in range(B):
                relaxed = sample_ref.kept_mask(d[r], temp, k, p, rel=1e-4)
                assert relaxed[ids_[r]], (step, temp, k, p, r)
                g = sample_ref.gumbel(sample_ref.row_stream(int(key[r]), 0x1234567890ABCDEF, 0, T, step), W)
                keep = sample_ref.kept_mask(d[r], temp, k, p)
                i_ref, gap = sample_ref.gumbel_argmax(d[r], keep, temp, g)
                i_rel, _ = sample_ref.gumbel_argmax(d[r], relaxed, temp, g)
                if gap > 1e-4 and i_ref == i_rel:
                    assert int(ids_[r]) == i_ref, (step, temp, k, p, r)
                    checked += 1
    assert checked > 0.8 * 3 * len(FILTERS) * B


@pytest.mark.parametrize("temp,k,p", [(2.0, 0, 1.0), (1.5, 20, 1.0), (1.0, 0, 0.9)])
def test_draws_follow_the_filtered_distribution(setup, temp, k, p):
    """One commit in 64 rows x 8 samples with distinct keys, 8 seeds: 4 096 draws from one step-0 distribution."""
    from fira_icse_amd.model import DeviceBatch
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, db = setup
    search = Searcher(spread)
    B, n, W = 64, 8, cfg.out_len
    db64 = DeviceBatch(store.batch([ids[0]] * B), cfg)
    ws = search._begin(db64, n)
    tok = torch.full((B * n,), 2, dtype=torch.int32, device="cuda")
    key = torch.arange(B, dtype=torch.int32, device="cuda")
    dist = torch.empty(B * n, W, device="cuda")
    bid = torch.empty(B * n, dtype=torch.int32, device="cuda")
    bp = torch.empty(B * n, device="cuda")
    draws = []
    for s in range(8):
        step_sample(search, ws, B, n, 0, tok, key, seed_tensor(1000 + s), temp, k, p, dist, bid, bp)
        torch.cuda.synchronize()
        assert torch.equal(dist.view(torch.int32), dist[:1].expand_as(dist).view(torch.int32))
        draws.append(bid.long().cpu().numpy())
    draws = np.concatenate(draws)
    q, keep = sample_ref.filtered_q(dist[0].double().cpu().numpy(), temp, k, p)
    relaxed = sample_ref.kept_mask(dist[0].double().cpu().numpy(), temp, k, p, rel=1e-4)
    assert relaxed[draws].all()
    N = len(draws)
    counts = np.bincount(draws, minlength=W)
    big = q * N >= 5                                  # entries with an expectation of >= 5 draws: one by one
    sig = np.sqrt(N * q * (1 - q))
    assert (np.abs(counts[big] - N * q[big]) <= 5 * sig[big] + 1).all()
    rest_q = q[~big].sum()                            # the long tail as one pooled entry
    assert abs(counts[~big].sum() - N * rest_q) <= 5 * np.sqrt(N * rest_q * (1 - rest_q)) + 1
    assert big.sum() >= 2


def test_top_k_one_is_greedy(setup):
    cfg, store, ids, peaked, spread, db = setup
    from fira_icse_amd.decode import Searcher
    search = Searcher(peaked)
    out, length, prob = search.greedy(db)
    B, T, W = db.B, cfg.tar_len, cfg.out_len
    # every step's maximum along the greedy path is unique
    ws = search._begin(db, 1)
    dist = torch.empty(B, W, device="cuda")
    for step in range(int(length.max()) - 1):
        live = (length > step) & (out[:, step] != 1)
        tok = torch.where(live, out[:, step], torch.zeros_like(out[:, step])).to(torch.int32)
        search._step(ws, B, 1, step, tok, None, dist, None, None)
        top2 = torch.topk(dist, 2, dim=1).values
        alive = length > step + 1
        assert (top2[alive, 0] > top2[alive, 1]).all(), step
    for n in (1, 3):
        toks, lens, p_, logp = search.sample(db, n, top_k=1, temperature=1.3, seed=9)
        for j in range(n):
            assert torch.equal(toks[:, j], out) and torch.equal(lens[:, j], length)
            assert torch.allclose(p_[:, j], prob, rtol=1e-5, atol=0)


def test_replay_eager_seeds_and_keys(setup):
    from fira_icse_amd.model import DeviceBatch
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, db = setup
    search = Searcher(spread)
    kw = dict(temperature=2.0, top_k=0, top_p=1.0)
    a = search.sample(db, 3, seed=4, **kw)                          # captures
    b = search.sample(db, 3, seed=4, **kw)                          # replay
    c = search.sample(db, 3, seed=4, use_graphs=False, **kw)        # eager launches
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[3], y[3])
    d = search.sample(db, 3, seed=5, **kw)
    assert not torch.equal(a[0], d[0])
    twice = DeviceBatch(store.batch([ids[0], ids[0]]), cfg)
    same = search.sample(twice, 2, seed=4, keys=[3, 3], **kw)
    assert torch.equal(same[0][0], same[0][1]) and torch.equal(same[3][0], same[3][1])
    diff = search.sample(twice, 2, seed=4, keys=[3, 4], **kw)
    assert not torch.equal(diff[0][0], diff[0][1])


def test_bookkeeping_equals_torch_statement(setup):
    """Ids resolve through the sou / sub-token row of commit r / n; logp = sum of log best_p; early stop at <eos>."""
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, db = setup
    search = Searcher(spread)
    B, n, T, W = db.B, 3, cfg.tar_len, cfg.out_len
    V, L = cfg.vocab_size, cfg.sou_len
    R = B * n
    ws = search._begin(db, n)
    dev = "cuda"
    key = torch.arange(B, dtype=torch.int32, device=dev)
    seed = seed_tensor(77)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    out, length, alive, tok, n_alive = i32(R, T), i32(R), i32(R), i32(R), i32(T)
    prob, logp = torch.ones(R, device=dev), torch.zeros(R, device=dev)
    out[:, 0] = 2
    length.fill_(1); alive.fill_(1); tok.fill_(2)
    sou, sub = db.sou.to(torch.int32).contiguous(), db.sub_token.to(torch.int32).contiguous()
    bid, bp = i32(R), torch.empty(R, device=dev)
    dist = torch.empty(R, W, device=dev)
    ref_out, ref_len, ref_alive = out.clone(), length.clone(), alive.clone()
    ref_logp = torch.zeros(R, dtype=torch.float64, device=dev)
    commit = torch.arange(R, device=dev) // n
    for step in range(T - 1):
        step_sample(search, ws, B, n, step, tok, key, seed, 1.5, 0, 0.95, dist, bid, bp)
        w = bid.long()
        nt = torch.where(w >= V + L, sub[commit, (w - V - L).clamp(0, sub.shape[1] - 1)],
                         torch.where(w >= V, sou[commit, (w - V).clamp(0, L - 1)], w)).to(torch.int32)
        live = ref_alive.bool()
        ref_out[live, step + 1] = nt[live]
        ref_len += live.to(torch.int32)
        ref_logp += torch.where(live, torch.log(bp.double()), torch.zeros_like(ref_logp))
        ref_alive = (live & (nt != 1)).to(torch.int32)
        _lib.check(_lib.lib().fira_sample_advance(_lib.cur_stream(), C.byref(search.model.dims), B, n, step, _lib.ptr(bid),
                                                  _lib.ptr(bp), _lib.ptr(sou), _lib.ptr(sub), _lib.ptr(out), _lib.ptr(length),
                                                  _lib.ptr(prob), _lib.ptr(logp), _lib.ptr(alive), _lib.ptr(tok),
                                                  _lib.ptr(n_alive)), "fira_sample_advance")
        assert torch.equal(out, ref_out) and torch.equal(length, ref_len) and torch.equal(alive, ref_alive), step
        assert torch.equal(tok, torch.where(ref_alive.bool(), nt, torch.zeros_like(nt)))
        assert int(n_alive[step]) == int(ref_alive.sum())
    assert torch.allclose(logp.double(), ref_logp, rtol=1e-5, atol=1e-5)
    # Searcher.sample: logp is the log of the product it reports, and the loop stops once every sample has ended
    toks, lens, p_, lp = search.sample(db, n, temperature=1.5, top_p=0.95, seed=77)
    assert torch.allclose(lp.double(), torch.log(p_.double()), rtol=1e-4, atol=1e-4) or (p_ == 0).any()
    from fira_icse_amd.model import TransModel, reference_init_state_dict
    torch.manual_seed(0)
    sd = util.peaked_state_dict(reference_init_state_dict(cfg), seed=2)
    sd["out_fc.bias"][1] += 30.0                                     # <eos> early: every sample ends well before tar_len
    short = TransModel(cfg, init=False)
    short.load_state_dict(sd)
    short.eval()
    peaked_search = Searcher(short)
    toks, lens, _, _ = peaked_search.sample(db, 2, seed=1)           # captures
    st = peaked_search._ws[("sample", B, 2, 1.0, 0, 1.0)]
    replays = []

    class Counted:
        def __init__(self, g, i):
            self.g, self.i = g, i

        def replay(self):
            replays.append(self.i)
            self.g.replay()
    st["graphs"] = [Counted(g, i) for i, g in enumerate(st["graphs"])]
    toks2, lens2, _, _ = peaked_search.sample(db, 2, seed=1)
    assert torch.equal(toks, toks2) and torch.equal(lens, lens2)
    last_step = int(lens.max()) - 2                                  # the step that appended the last <eos>
    assert replays == list(range(last_step // 5 + 1))                # no chunk after the one where every sample ended
    assert last_step // 5 + 1 < len(st["graphs"]), "the fixture's samples should end before the last chunk"


def test_bf16_kv_sampler_dist_agrees_with_fp32(setup):
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, db = setup
    B, W = db.B, cfg.out_len
    key = torch.arange(B, dtype=torch.int32, device="cuda")
    seed = seed_tensor(3)
    dists = []
    for flags in (0, 1):
        s = Searcher(peaked, kv_bf16=bool(flags))
        ws = s._begin(db, 1)
        dist = torch.empty(B, W, device="cuda")
        bid, bp = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, device="cuda")
        tok = torch.full((B,), 2, dtype=torch.int32, device="cuda")
        step_sample(s, ws, B, 1, 0, tok, key, seed, 1.0, 5, 0.9, dist, bid, bp, flags=flags)
        torch.cuda.synchronize()
        dists.append(dist.clone())
    top = dists[0].argmax(1)
    assert torch.allclose(dists[1][torch.arange(B), top], dists[0][torch.arange(B), top], rtol=5e-2)
    toks, lens, p_, _ = Searcher(peaked, kv_bf16=True).sample(db, 2, top_k=1)
    out0, len0, prob0 = Searcher(peaked).greedy(db)
    assert float((toks[:, 0] == out0).float().mean()) > 0.95


def test_shape_and_argument_errors(setup):
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, peaked, spread, db = setup
    s = Searcher(peaked)
    for kw in (dict(temperature=0.0), dict(temperature=float("inf")), dict(top_k=-1), dict(top_k=cfg.out_len + 1),
               dict(top_p=0.0), dict(top_p=1.5)):
        with pytest.raises(_lib.FiraError):
            s.sample(db, 2, use_graphs=False, **kw)
    with pytest.raises(_lib.FiraError):
        s.sample(db, 9, use_graphs=False)


# ------------------------------------------------------------------------------------------------ command line
def test_cli_sample_end_to_end(tmp_path):
    root = str(tmp_path)
    synth.write_dataset(root, util.load_golden_raw())
    torch.save(spread_state_dict(FiraConfig()), os.path.join(root, "best_model.pt"))
    base = ["test", "--splits", "16,4,4", "--test-batch-size", "3"]
    opts = ["--sample", "3", "--temperature", "1.5", "--top-p", "0.9"]
    out_f, samp_f = os.path.join(root, "OUTPUT", "output_fira"), os.path.join(root, "OUTPUT", "output_fira_samples")
    run_cli(base + opts + ["--sample-seed", "7"], root)
    best, samples = open(out_f).read(), open(samp_f).read()
    lines, recs = best.split("\n"), [json.loads(l) for l in samples.strip().split("\n")]
    assert len(lines) == 5 and lines[-1] == "" and len(recs) == 4
    for line, rec in zip(lines, recs):
        assert len(rec["candidates"]) == 3 and len(rec["logp"]) == 3
        assert line == rec["candidates"][int(np.argmax(rec["logp"]))]
    run_cli(base + opts + ["--sample-seed", "7"], root)
    assert open(out_f).read() == best and open(samp_f).read() == samples
    run_cli(base + opts + ["--sample-seed", "8"], root)
    assert open(samp_f).read() != samples
    os.remove(samp_f)
    run_cli(base, root)                                          # without --sample: the beam-3 search, as before
    default = open(out_f).read()
    assert not os.path.exists(samp_f) and len(default.split("\n")) == 5
    run_cli(base + ["--beam", "3"], root)
    assert open(out_f).read() == default
