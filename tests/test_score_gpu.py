"""Teacher-forced scoring on the device (fira_decode_step_score / Searcher.score / run_model.py test --score): the
distribution row is the decode step's, bit for bit; the word marginal, its largest entry and the copy share are the numpy
statement's (score_ref.py) on that row; the labelled entry agrees with the CPU oracle; greedy and sampled messages score
consistently with what the searches report; candidates share a commit's memory without changing a bit; the command line."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import score_ref
import util
from search_kit import bits, golden_search, run_cli, spread_state_dict
from fira_icse_amd import _lib, synth, text
from fira_icse_amd.config import EOS, PAD, START, UNK, FiraConfig

pytestmark = pytest.mark.gpu

U24, U23 = 2.0 ** -24, 2.0 ** -23


@pytest.fixture(scope="module")
def setup():
    from fira_icse_amd.model import TransModel
    g = golden_search(weights="peaked", searchers=0, seed=2)
    sds = dict(peaked=g.state_dict, spread=spread_state_dict(g.cfg))
    models = dict(peaked=g.model, spread=TransModel(g.cfg, init=False))
    models["spread"].load_state_dict(sds["spread"])
    models["spread"].eval()
    return g.cfg, g.store, g.ids, sds, models, g.db


class StepOut:
    def __init__(self, R, W, labelled=True):
        f = lambda: torch.zeros(R, device="cuda")
        i = lambda: torch.zeros(R, dtype=torch.int32, device="cuda")
        self.dist = torch.empty(R, W, device="cuda")
        self.p_word, self.p_entry, self.copy_share, self.p_label = f(), f(), f(), f()
        self.entry, self.top_id = i(), i()
        self.logp_word, self.logp_entry, self.logp_label = f(), f(), f()
        self.labelled = labelled


def step_score(search, ws, B, n, step, tok, target, label, sou, sub, o, flags=0):
    m = search.model
    lab = o.labelled
    _lib.check(_lib.lib().fira_decode_step_score(
        _lib.cur_stream(), C.byref(m.dims), _lib.ptr(m.flat.data), _lib.ptr(ws), ws.numel(), B, n, step, _lib.ptr(tok),
        _lib.ptr(target), _lib.ptr(label) if lab else None, _lib.ptr(sou), _lib.ptr(sub), _lib.ptr(o.dist), _lib.ptr(o.p_word),
        _lib.ptr(o.p_entry), _lib.ptr(o.entry), _lib.ptr(o.copy_share), _lib.ptr(o.p_label) if lab else None,
        _lib.ptr(o.top_id), _lib.ptr(o.logp_word), _lib.ptr(o.logp_entry), _lib.ptr(o.logp_label) if lab else None, flags),
        "fira_decode_step_score")


def i32(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(torch.int32).cuda().contiguous()


def special_targets(cfg, hb):
    """Per commit: a word in several valid diff positions, a word that occurs nowhere in the memory, a sub-token word."""
    multi, nowhere, subw = [], [], []
    for b in range(hb.sou.shape[0]):
        sou, sub = hb.sou[b], hb.sub_token[b]
        ids_, counts = np.unique(sou[sou != 0], return_counts=True)
        assert (counts >= 2).any(), "fixture: commit %d has no word in several diff positions" % b
        multi.append(int(ids_[np.argmax(counts)]))
        present = set(sou.tolist()) | set(sub.tolist())
        nowhere.append(next(w for w in range(4, cfg.vocab_size) if w not in present))
        assert (sub != 0).any(), "fixture: commit %d has no sub-token" % b
        subw.append(int(sub[sub != 0][0]))
    return multi, nowhere, subw


def test_step_is_the_decode_steps_and_the_row_outputs_are_the_numpy_statement(setup):
    """Six teacher-forced steps on both weight sets.  dist, top_id and every single-entry probability are bit-identical
    to fira_decode_step_ex's; p_word is within (k - 1) * 2^-24 relative of the exact sum of its k entries (a fixed-order fp32
    sum of k non-negative terms makes at most k - 1 roundings); copy_share, a quotient of two such sums, within (k + 1) * 2^-24;
    entry exactly, ties included; the running sums are the logs of what was reported."""
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, sds, models, db = setup
    hb = store.batch(ids)
    B, W, V, L = db.B, cfg.out_len, cfg.vocab_size, cfg.sou_len
    multi, nowhere, subw = special_targets(cfg, hb)
    sou, sub = i32(hb.sou), i32(hb.sub_token)
    src = np.concatenate([hb.sou, hb.sub_token], 1)
    valid = src != 0                                               # the memory mask (oracle.encode_memory)
    targets = [hb.tar[:, 1], np.array(multi), np.array(nowhere), hb.tar[:, 4], np.array(subw), np.full(B, UNK)]
    targets[3] = np.where(np.arange(B) % 2 == 0, targets[3], 0)    # some rows with nothing to score
    for name in ("spread", "peaked"):
        search = Searcher(models[name])
        ws = search._begin(db, 1)
        o = StepOut(B, W)
        dist_a = torch.empty(B, W, device="cuda")
        bid = torch.empty(B, dtype=torch.int32, device="cuda")
        bp = torch.empty(B, device="cuda")
        sums = np.zeros((3, B))
        seen_multi = 0
        for step in range(6):
            tok = i32(hb.tar[:, step])
            y = targets[step]
            label = hb.tar_label[:, step + 1].copy()
            if step in (1, 2, 4, 5):                                # a made-up target: label one entry that resolves to it, or none
                label = np.where(y < V, y, -1)
            search._step(ws, B, 1, step, tok, None, dist_a, bid, bp)
            step_score(search, ws, B, 1, step, tok, i32(y), i32(label), sou, sub, o)
            torch.cuda.synchronize()
            assert torch.equal(bits(dist_a), bits(o.dist)), (name, step)
            assert torch.equal(o.top_id, bid), (name, step)
            d = o.dist.cpu().numpy()
            got = {k: getattr(o, k).cpu().numpy() for k in ("p_word", "p_entry", "entry", "copy_share", "p_label")}
            for b in range(B):
                ref = score_ref.score_row(d[b], src[b], valid[b], V, int(y[b]), int(label[b]))
                print(name, step, b, "y", int(y[b]), "k", ref["k"], "p_word", got["p_word"][b], ref["p_word"], "entry",
                      got["entry"][b], ref["entry"], "share", got["copy_share"][b], ref["copy_share"])
                assert int(got["entry"][b]) == ref["entry"], (name, step, b)
                if y[b] == 0:
                    assert (got["p_word"][b], got["p_entry"][b], got["copy_share"][b], got["p_label"][b]) == (0, 0, 0, 0)
                    continue
                if ref["entry"] >= 0:
                    assert got["p_entry"][b] == d[b, ref["entry"]]                       # the same bits
                    assert text.resolve_copy(ref["entry"], hb.sou[b], hb.sub_token[b], V, L) == int(y[b])
                else:
                    assert got["p_entry"][b] == 0
                assert got["p_label"][b] == (d[b, label[b]] if label[b] >= 0 else 0)
                assert abs(float(got["p_word"][b]) - ref["p_word"]) <= max(ref["k"] - 1, 0) * U24 * ref["p_word"], (name, step, b)
                assert abs(float(got["copy_share"][b]) - ref["copy_share"]) <= (ref["k"] + 1) * U24 * ref["copy_share"]
                seen_multi += ref["k"] >= 3
                sums[0, b] += math.log(max(float(got["p_word"][b]), 1e-10))
                sums[1, b] += math.log(max(float(got["p_entry"][b]), 1e-10))
                if label[b] >= 0:
                    sums[2, b] += math.log(max(float(got["p_label"][b]), 1e-10))
        assert seen_multi >= B                                       # every commit had a target with >= 2 copy entries
        for j, k in enumerate(("logp_word", "logp_entry", "logp_label")):
            assert np.allclose(getattr(o, k).cpu().numpy(), sums[j], rtol=1e-5, atol=1e-5), (name, k)
        # without labels: the same scores
        o2 = StepOut(B, W, labelled=False)
        step_score(search, ws, B, 1, 5, i32(hb.tar[:, 5]), i32(targets[5]), None, sou, sub, o2)
        assert torch.equal(bits(o2.p_word), bits(o.p_word)) and torch.equal(o2.entry, o.entry)


def test_label_probability_equals_the_oracle(setup):
    """p_label of the golden messages with their copy labels against the CPU oracle's full teacher-forced recompute, to the
    bound test_step_distribution_equals_full_recompute holds the step to: 2e-4 of the row's maximum."""
    from fira_icse_amd.decode import Searcher
    from oracle import fira_oracle as O
    cfg, store, ids, sds, models, db = setup
    hb = store.batch(ids)
    tb = util.to_torch_batch(hb, cfg)
    B, T = db.B, cfg.tar_len
    for name in ("spread", "peaked"):
        with torch.no_grad():
            memory, mem_mask = O.encode_memory(sds[name], cfg, tb["sou"], tb["mark"], tb["ast_change"], tb["edge"], tb["sub_token"])
            dec = O.decoder(sds[name], cfg, tb["tar"], memory, mem_mask, tb["tar"] != 0)
            ref = O.output_distribution(sds[name], memory, mem_mask, dec)
        sc = Searcher(models[name]).score(db, hb.tar, labels=hb.tar_label)
        p_label = sc.p_label.cpu()
        n = 0
        nll = np.zeros(B)
        for b in range(B):
            for t in range(T - 1):
                if hb.tar[b, t + 1] == 0:
                    assert float(p_label[b, 0, t]) == 0
                    continue
                want = float(ref[b, t, int(hb.tar_label[b, t + 1])])
                err = abs(float(p_label[b, 0, t]) - want)
                print(name, b, t, float(p_label[b, 0, t]), want, err / float(ref[b, t].max()))
                assert err <= 2e-4 * float(ref[b, t].max()), (name, b, t)
                nll[b] += math.log(max(float(p_label[b, 0, t]), 1e-10))
                n += 1
        assert n == int((hb.tar[:, 1:] != 0).sum()) and n > 4 * B
        assert sc.length.cpu().tolist() == [[int((row != 0).sum())] for row in hb.tar]
        assert np.allclose(sc.logp_label.cpu().numpy()[:, 0], nll, rtol=1e-5, atol=1e-5)
        # the word marginal includes the labelled entry
        assert bool((sc.p_word.cpu() >= p_label).all())


def test_greedy_and_sampled_messages_score_consistently(setup):
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, sds, models, db = setup
    hb = store.batch(ids)
    B, T, W, V, L = db.B, cfg.tar_len, cfg.out_len, cfg.vocab_size, cfg.sou_len
    search = Searcher(models["peaked"])
    out, length, prob = search.greedy(db)
    ws = search._begin(db, 1)
    bid = torch.empty(B, dtype=torch.int32, device="cuda")
    bp = torch.empty(B, device="cuda")
    best_p = torch.zeros(T - 1, B)
    for step in range(int(length.max()) - 1):
        search._step(ws, B, 1, step, out[:, step].to(torch.int32).contiguous(), None, None, bid, bp)
        best_p[step] = bp.cpu()
    sc = search.score(db, out, lengths=length)
    out_c, len_c = out.cpu(), length.cpu()
    for b in range(B):
        for t in range(int(len_c[b]) - 1):
            top = int(sc.top_id[b, 0, t])
            assert text.resolve_copy(top, hb.sou[b], hb.sub_token[b], V, L) == int(out_c[b, t + 1]), (b, t)
            assert float(sc.p_entry[b, 0, t]) == float(best_p[t, b]), (b, t)
        assert bool((sc.top_id[b, 0, int(len_c[b]) - 1:] == -1).all())
        got, want = math.exp(float(sc.logp_entry[b, 0])), float(prob[b])
        print("greedy", b, int(len_c[b]), got, want, abs(got - want) / want)
        assert abs(got - want) <= T * U23 * want, (b, got, want)
    assert torch.equal(sc.length[:, 0], length)
    # sampled candidates: the word marginal cannot be below the drawn entries (one rounding of slack per summed term)
    search = Searcher(models["spread"])
    toks, lens, _, logp = search.sample(db, 4, temperature=1.0, top_k=20, seed=11)
    inner = (toks[:, :, 1:] == PAD) | (toks[:, :, 1:] == START)
    inside = torch.arange(1, T, device=toks.device)[None, None, :] < lens[:, :, None]
    assert not bool((inner & inside).any()), "fixture: a sampled message holds <pad> or <start>"
    sc = search.score(db, toks, lengths=lens)
    lw, lp = sc.logp_word.double().cpu(), logp.double().cpu()
    print("sampled logp_word", lw.tolist(), "logp", lp.tolist())
    assert bool((lw >= lp - T * U23 * lp.abs().clamp(min=1)).all())
    assert bool((sc.logp_word >= sc.logp_entry).all())
    le = sc.logp_entry.double().cpu()                               # the largest entry of the word is at least the drawn one
    assert bool((le >= lp - T * U23 * lp.abs().clamp(min=1)).all())
    # ranking: first on ties, the three keys
    assert search.rank(sc, "logp_word") == torch.argmax(sc.logp_word, 1).tolist()
    assert search.rank(sc, "mean_logp_word") == torch.argmax(sc.logp_word / (sc.length - 1).clamp(min=1), 1).tolist()
    tie = type(sc)(logp_entry=torch.zeros(2, 3), logp_word=torch.zeros(2, 3), length=torch.full((2, 3), 5))
    assert search.rank(tie, "logp_entry") == [0, 0]
    with pytest.raises(ValueError):
        search.rank(sc, "logp")


def equal_scores(a, b, sel_a=slice(None), sel_b=slice(None)):
    for k in a:
        x, y = a[k][sel_a], b[k][sel_b]
        assert torch.equal(bits(x) if x.dtype == torch.float32 else x, bits(y) if y.dtype == torch.float32 else y), k


def test_candidates_share_memory_batches_replays_and_bf16(setup):
    from fira_icse_amd.model import DeviceBatch
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, sds, models, db = setup
    hb = store.batch(ids)
    B, T = db.B, cfg.tar_len
    search = Searcher(models["peaked"])
    greedy, glen, _ = search.greedy(db)
    cand = np.zeros((B, 3, T), dtype=np.int64)
    cand[:, 0] = hb.tar
    cand[:, 1] = greedy.cpu().numpy()
    cand[:, 2] = np.roll(hb.tar, 1, axis=0)                          # another commit's message
    three = search.score(db, cand)                                   # captures
    for j in range(3):
        one = search.score(db, cand[:, j])
        equal_scores(one, three, (slice(None), slice(0, 1)), (slice(None), slice(j, j + 1)))
    again = search.score(db, cand)                                   # a second replay
    eager = search.score(db, cand, use_graphs=False)
    equal_scores(three, again)
    equal_scores(three, eager)
    # a commit's scores do not depend on the other commits of its batch
    eight = list(range(8))
    hb8 = store.batch(eight)
    s8 = search.score(DeviceBatch(hb8, cfg), hb8.tar, labels=hb8.tar_label)
    for lo in (0, 4):
        hb4 = store.batch(eight[lo:lo + 4])
        s4 = search.score(DeviceBatch(hb4, cfg), hb4.tar, labels=hb4.tar_label)
        equal_scores(s4, s8, slice(None), slice(lo, lo + 4))
    # bf16 K|V: runs, stays close and ranks the candidates like fp32
    half = Searcher(models["peaked"], kv_bf16=True).score(db, cand)
    assert search.rank(half, "logp_word") == search.rank(three, "logp_word")
    assert search.rank(three, "logp_word") == [1] * B                # the model's own greedy message is its most probable
    assert bool(torch.isfinite(half.logp_word).all()) and torch.equal(half.length, three.length)


def test_invalid_candidates_raise_before_anything_is_launched(setup):
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, sds, models, db = setup
    hb = store.batch(ids)
    search = Searcher(models["peaked"])
    B, T = db.B, cfg.tar_len
    ok = hb.tar.copy()
    bad = []
    x = ok.copy(); x[0, 0] = 7; bad.append(x)                        # no <start>
    x = ok.copy(); x[1, 1] = cfg.vocab_size; bad.append(x)           # a token outside the vocabulary
    x = ok.copy(); x[2, 1] = 0; bad.append(x)                        # id 0 inside a message
    x = ok.copy(); x[3, 1] = EOS; bad.append(x)                      # <eos> before the end
    bad.append(np.repeat(ok[:, None, :], 9, axis=1))                 # n outside 1..8
    bad.append(ok[:2])                                               # not this batch
    bad.append(np.concatenate([ok, ok], 1))                          # longer than tar_len
    for c in bad:
        with pytest.raises(ValueError):
            search.score(db, c)
    assert not any(k[0] == "score" for k in search._ws if isinstance(k, tuple) and isinstance(k[0], str))
    with pytest.raises(_lib.FiraError):                              # the library refuses n_cand itself as well
        o = StepOut(B * 9, cfg.out_len)
        ws = search._begin(db, 8)
        z = torch.zeros(B * 9, dtype=torch.int32, device="cuda")
        step_score(search, ws, B, 9, 0, z, z, z, i32(hb.sou), i32(hb.sub_token), o)


# ------------------------------------------------------------------------------------------------ command line
def test_cli_score_and_rerank_end_to_end(tmp_path):
    from fira_icse_amd.model import reference_init_state_dict
    root = str(tmp_path)
    cfg = FiraConfig()
    synth.write_dataset(root, util.load_golden_raw())
    torch.manual_seed(0)
    torch.save(util.peaked_state_dict(reference_init_state_dict(cfg), seed=2), os.path.join(root, "best_model.pt"))
    base = ["test", "--splits", "16,4,4", "--test-batch-size", "3"]
    out_f, samp_f, score_f = (os.path.join(root, "OUTPUT", n) for n in ("output_fira", "output_fira_samples", "output_fira_scores"))
    # the test split's own messages
    stdout = run_cli(base + ["--score", "refs"], root).stdout
    recs = [json.loads(l) for l in open(score_f).read().strip().split("\n")]
    assert len(recs) == 4 and not os.path.exists(out_f)
    for r in recs:
        n = r["n_tokens"]
        assert n >= 1 and all(len(r[k]) == n for k in ("p_word", "copy_share", "source", "tokens", "top"))
        assert r["logp_word"] >= r["logp_label"] - 1e-4 and all(s == "gen" or s == "none" or s.split(":")[0] in ("diff", "sub")
                                                                for s in r["source"])
    ppl = float(stdout.split("perplexity ")[1].split()[0])
    assert math.isfinite(ppl) and ppl >= 1.0
    assert abs(ppl - math.exp(-sum(r["logp_word"] for r in recs) / sum(r["n_tokens"] for r in recs))) <= 1e-3 * ppl
    assert "label entries only" in stdout
    # a greedy run's own output: the greedy path is the arg-max path
    run_cli(base + ["--beam", "1"], root)
    lines = open(out_f).read().split("\n")[:-1]
    given = os.path.join(root, "given")
    shutil.copy(out_f, given)
    os.remove(out_f)
    run_cli(base + ["--score", given], root)
    recs = [json.loads(l) for l in open(score_f).read().strip().split("\n")]
    assert len(recs) == len(lines) == 4 and not os.path.exists(out_f)
    checked = 0
    for line, r in zip(lines, recs):
        assert r["n_tokens"] == min(len(line.split()) + 1, cfg.tar_len - 1) and "logp_label" not in r
        if "\U0001F605" not in line:
            assert r["top"] == r["tokens"], line
            checked += 1
    assert checked >= 1
    with open(given, "a") as f:
        f.write("one line too many\n")
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "run_model.py")] + base + ["--score", given], cwd=root,
                       env=dict(os.environ, PYTHONPATH=util.REPO), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "5 lines for 4 test commits" in r.stderr
    # sampling: unchanged without --rerank; with it, the pick follows the key
    torch.save(spread_state_dict(cfg), os.path.join(root, "best_model.pt"))
    opts = ["--sample", "4", "--temperature", "1.2", "--top-k", "30", "--sample-seed", "5"]
    run_cli(base + opts, root)
    plain_best, plain = open(out_f).read(), open(samp_f).read()
    for line, l in zip(plain_best.split("\n"), plain.strip().split("\n")):
        rec = json.loads(l)
        assert sorted(rec) == ["candidates", "logp"] and line == rec["candidates"][int(np.argmax(rec["logp"]))]
    run_cli(base + opts + ["--rerank", "logp_word"], root)
    for line, l, l0 in zip(open(out_f).read().split("\n"), open(samp_f).read().strip().split("\n"), plain.strip().split("\n")):
        rec, rec0 = json.loads(l), json.loads(l0)
        assert rec["candidates"] == rec0["candidates"] and rec["logp"] == rec0["logp"] and len(rec["logp_word"]) == 4
        vals = [-math.inf if v is None else v for v in rec["logp_word"]]
        assert line == rec["candidates"][int(np.argmax(vals))]
        assert all(v is None or v >= lp - 1e-3 * max(1.0, abs(lp)) for v, lp in zip(rec["logp_word"], rec["logp"]))
    # the candidates file of the sampling run can be scored as it is
    run_cli(base + ["--score", samp_f], root)
    recs = [json.loads(l) for l in open(score_f).read().strip().split("\n")]
    assert len(recs) == 4 and all(len(r["candidates"]) == 4 for r in recs)
    run_cli(base + opts, root)
    assert open(out_f).read() == plain_best and open(samp_f).read() == plain
