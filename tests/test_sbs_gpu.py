"""Stochastic beam search on the device (fira_beam_select_gumbel / Searcher.sample_distinct / --without-replacement): the
kernel is the numpy twin (sbs_ref.py) on synthetic rows; one slot is the sampler; the hypotheses are distinct; slot 0 is an
exact sample; replay, batch placement, seeds, constraints and ensembles behave; bad arguments are refused; the command line."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sample_ref
import sbs_ref
import util
from search_kit import device_dims, golden_search, run_cli, spread_state_dict
from fira_icse_amd import _lib, synth
from fira_icse_amd.config import FiraConfig

pytestmark = pytest.mark.gpu

KEYS = [7, 11, 13, 17]


@pytest.fixture(scope="module")
def setup():
    g = golden_search(weights="spread", searchers=0)
    return g.cfg, g.store, g.ids, g.model, g.db


def call_kernel(d, n, temp, a, step=sbs_ref.CASE_STEP, seed=sbs_ref.CASE_SEED, B=sbs_ref.CASE_B):
    """fira_beam_select_gumbel on the arrays of a case; returns (rc, outputs as numpy)."""
    dev = "cuda"
    i32 = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.int32).to(dev)
    f32 = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(dev)
    R, T = a["gen"].shape
    fin = (a["gen"][np.arange(R), a["length"] - 1] == sbs_ref.EOS)
    t = dict(dist=f32(a["dist"]), fin=i32(fin), done=i32([0]), sou=i32(a["sou"]), sub=i32(a["sub"]), key=i32(a["key"]),
             seed=torch.tensor([seed], dtype=torch.int64, device=dev), gen=i32(a["gen"]), length=i32(a["length"]),
             phi=f32(a["phi"]), G=f32(a["G"]), logp=f32(a["logp"]))
    out = dict(gen=torch.full((R, T), -7, dtype=torch.int32, device=dev), length=torch.full((R,), -7, dtype=torch.int32, device=dev),
               phi=torch.full((R,), 7.0, device=dev), G=torch.full((R,), 7.0, device=dev), logp=torch.full((R,), 7.0, device=dev),
               parent=torch.full((R,), -7, dtype=torch.int32, device=dev))
    dims = device_dims(d["V"], d["L"], d["S"], d["T"])
    rc = _lib.lib().fira_beam_select_gumbel(
        _lib.cur_stream(), C.byref(dims), B, n, step, float(temp), _lib.ptr(t["dist"]), _lib.ptr(t["fin"]), _lib.ptr(t["done"]),
        _lib.ptr(t["sou"]), _lib.ptr(t["sub"]), _lib.ptr(t["key"]), _lib.ptr(t["seed"]), _lib.ptr(t["gen"]),
        _lib.ptr(t["length"]), _lib.ptr(t["phi"]), _lib.ptr(t["G"]), _lib.ptr(t["logp"]), _lib.ptr(out["gen"]),
        _lib.ptr(out["length"]), _lib.ptr(out["phi"]), _lib.ptr(out["G"]), _lib.ptr(out["logp"]), _lib.ptr(out["parent"]))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def test_kernel_equals_the_twin_on_synthetic_rows():
    """Every commit whose smallest key gap (twin, n + 1 best) exceeds sbs_ref.MARGIN: gen, length, parent and the slot order
    equal the twin's exactly; phi, G and logp within sbs_ref.TOLERANCE.  At most 10 % of the commits may be skipped (the twin's
    own share is under 5 %: test_sbs.py).  Prints the largest |key_device - key_twin|; the margin is at least 8 times it."""
    cfg = FiraConfig()
    model = dict(V=cfg.vocab_size, L=cfg.sou_len, S=cfg.sub_token_len, T=cfg.tar_len)
    total = skipped = 0
    worst = {"G": 0.0, "phi": 0.0, "logp": 0.0}
    for name, d, n, temp, a in sbs_ref.kernel_cases(model):
        rc, out = call_kernel(d, n, temp, a)
        assert rc == 0, _lib.lib().fira_last_error()
        for k in ("phi", "G", "logp"):
            assert not np.isnan(out[k]).any(), (name, n, temp, k)
        for b, ref in enumerate(sbs_ref.twin_of_case(d, n, temp, a)):
            total += 1
            if not ref["gap"] > sbs_ref.MARGIN:
                skipped += 1
                continue
            r = slice(b * n, (b + 1) * n)
            where = (name, n, temp, b)
            assert np.array_equal(out["gen"][r], ref["gen"]), where
            assert np.array_equal(out["length"][r], ref["length"]), where
            assert np.array_equal(out["parent"][r], b * n + ref["parent"]), where
            for k in ("phi", "G", "logp"):
                dev_v, ref_v = out[k][r].astype(np.float64), ref[k]
                void = ref_v == -np.inf
                assert np.array_equal(dev_v == -np.inf, void), (where, k)
                if (~void).any():
                    err = float(np.abs(dev_v[~void] - ref_v[~void]).max())
                    worst[k] = max(worst[k], err)
                    assert err <= sbs_ref.TOLERANCE, (where, k, err)
    print("largest |device - twin|: key %.3g, phi %.3g, logp %.3g; %d of %d commits below the margin"
          % (worst["G"], worst["phi"], worst["logp"], skipped, total))
    assert skipped <= 0.10 * total
    assert sbs_ref.MARGIN >= 8 * worst["G"]


@pytest.mark.parametrize("temp", [1.0, 1.5])
def test_one_slot_is_the_sampler(setup, temp):
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, spread, db = setup
    search = Searcher(spread)
    toks, lens, _, logp = search.sample(db, 1, temperature=temp, seed=21, keys=KEYS)
    t2, l2, lp2, phi, key = search.sample_distinct(db, 1, temperature=temp, seed=21, keys=KEYS, merge_copies=False)
    assert torch.equal(t2, toks) and torch.equal(l2, lens)
    assert torch.equal(lp2.view(torch.int32), logp.view(torch.int32))
    assert (key == 0).all()


def test_hypotheses_are_distinct_and_in_key_order(setup):
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, spread, db = setup
    search = Searcher(spread)
    for seed in (1, 2, 3):
        toks, lens, logp, phi, key = search.sample_distinct(db, 8, temperature=1.3, seed=seed, keys=KEYS)
        assert not torch.isnan(key).any() and not torch.isnan(phi).any() and not torch.isnan(logp).any()
        assert (key[:, 1:] <= key[:, :-1]).all() and (key[:, 0] <= 0).all()
        for b in range(db.B):
            live = [tuple(toks[b, j, :int(lens[b, j])].tolist()) for j in range(8) if key[b, j] > float("-inf")]
            assert len(live) >= 2 and len(set(live)) == len(live), (seed, b)


def test_first_slot_is_an_exact_sample(setup):
    """One commit in 64 rows with distinct keys, 8 seeds: 512 first words of slot 0 against the step-0 distribution of words
    (the chi-square of test_draws_follow_the_filtered_distribution: entries expected >= 5 times one by one within 5 sigma + 1,
    the tail pooled)."""
    from fira_icse_amd.model import DeviceBatch
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, spread, db = setup
    search = Searcher(spread)
    B, n, temp, W, V, L = 64, 4, 2.0, cfg.out_len, cfg.vocab_size, cfg.sou_len
    db64 = DeviceBatch(store.batch([ids[0]] * B), cfg)
    ws = search._begin(db64, 1)
    dist = torch.empty(B, W, device="cuda")
    search._step(ws, B, 1, 0, torch.full((B,), 2, dtype=torch.int32, device="cuda"), None, dist, None, None)
    torch.cuda.synchronize()
    q, _ = sample_ref.filtered_q(dist[0].double().cpu().numpy(), temp, 0, 1.0)
    word = np.concatenate([np.arange(V), db64.sou[0].cpu().numpy(), db64.sub_token[0].cpu().numpy()])
    qw = np.bincount(word, weights=q, minlength=V)                    # the distribution of the first WORD
    draws = []
    for s in range(8):
        toks, lens, _, _, key = search.sample_distinct(db64, n, temperature=temp, seed=1000 + s, keys=list(range(B)),
                                                       merge_copies=False)
        assert (lens[:, 0] >= 2).all()
        draws.append(toks[:, 0, 1].cpu().numpy())
    draws = np.concatenate(draws)
    N = len(draws)
    assert (qw[draws] > 0).all()
    counts = np.bincount(draws, minlength=V)
    big = qw * N >= 5
    sig = np.sqrt(N * qw * (1 - qw))
    assert (np.abs(counts[big] - N * qw[big]) <= 5 * sig[big] + 1).all()
    rest = qw[~big].sum()
    assert abs(counts[~big].sum() - N * rest) <= 5 * np.sqrt(N * rest * (1 - rest)) + 1
    assert big.sum() >= 2


def test_replay_placement_and_seeds(setup):
    from fira_icse_amd.model import DeviceBatch
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, spread, db = setup
    search = Searcher(spread)
    kw = dict(temperature=1.4, keys=KEYS)
    same = lambda x, y: all(torch.equal(u, v) if u.dtype != torch.float32 else torch.equal(u.view(torch.int32), v.view(torch.int32))
                            for u, v in zip(x, y))
    a = search.sample_distinct(db, 5, seed=4, **kw)                     # captures
    b = search.sample_distinct(db, 5, seed=4, **kw)                     # replay
    c = search.sample_distinct(db, 5, seed=4, use_graphs=False, **kw)   # eager launches
    assert same(a, b) and same(a, c)
    d = search.sample_distinct(db, 5, seed=5, **kw)
    assert not torch.equal(a[0], d[0])
    # a commit's result depends on its key, not on its row nor on the batch size
    names = ("tokens", "lengths", "logp", "phi", "key")
    perm = [2, 0, 3, 1]
    moved = search.sample_distinct(DeviceBatch(store.batch([ids[k] for k in perm]), cfg), 5, seed=4, temperature=1.4,
                                   keys=[KEYS[k] for k in perm])
    sub = search.sample_distinct(DeviceBatch(store.batch([ids[2], ids[0]]), cfg), 5, seed=4, temperature=1.4,
                                 keys=[KEYS[2], KEYS[0]])
    for what, res, rows in (("another row", moved, perm), ("a batch of 2", sub, [2, 0])):
        for name, x, y in zip(names, res, a):
            for r, k in enumerate(rows):
                print("%s, commit %d, %s: %s" % (what, k, name, "equal" if same([x[r]], [y[k]]) else
                                                  "DIFFERENT (max |d| %g)" % float((x[r].double() - y[k].double()).abs().max())))
    for x, y in zip(moved, a):                                       # another row of the same batch size: bit for bit
        for r, k in enumerate(perm):
            assert same([x[r]], [y[k]])
    # Another batch size: the messages are the same.  The values are not bit-equal, and cannot be: the decode step's own
    # distribution of a commit differs in its last bits between B = 2 and B = 4 (measured on fira_decode_step_ex alone: 2.7e-7
    # on an entry), so the sums differ by roundings.  Bound: logp and phi are sums of tar_len - 1 fp32 terms, each addition
    # within one ulp of the running sum; a key is formed from differences of values of phi's magnitude (g_i = (phi_j - lnZ) +
    # s_i), so it inherits their absolute rounding, one ulp of max(|phi|, |logp|) per step, whatever its own magnitude.
    for r, k in enumerate([2, 0]):
        assert torch.equal(sub[0][r], a[0][k]) and torch.equal(sub[1][r], a[1][k])
        ulp = float(np.spacing(np.float32(max(float(a[2][k].abs().max()), float(a[3][k].abs().max())))))
        for x, y in zip(sub[2:], a[2:]):
            assert float((x[r].double() - y[k].double()).abs().max()) <= (cfg.tar_len - 1) * ulp


def test_constraints_and_ensemble(setup):
    from fira_icse_amd.model import TransModel, reference_init_state_dict
    from fira_icse_amd.decode import Searcher, Constraints
    cfg, store, ids, spread, db = setup
    search = Searcher(spread)
    base = search.sample_distinct(db, 4, temperature=1.2, seed=6, keys=KEYS)
    words = base[0][:, :, 1:].flatten()
    words = words[words > 3]
    w = int(torch.mode(words).values)
    con = Constraints(no_repeat_ngram=1, banned=(w,))
    toks, lens, logp, phi, key = search.sample_distinct(db, 4, temperature=1.2, seed=6, keys=KEYS, constraints=con)
    assert not torch.isnan(key).any()
    n_live = 0
    for b in range(db.B):
        for j in range(4):
            if key[b, j] > float("-inf"):
                msg = toks[b, j, 1:int(lens[b, j])].tolist()
                assert w not in msg and len(set(msg)) == len(msg), (b, j, msg)
                n_live += 1
    assert n_live >= db.B
    torch.manual_seed(0)
    other = TransModel(cfg, init=False)
    other.load_state_dict(util.peaked_state_dict(reference_init_state_dict(cfg), seed=2))
    other.eval()
    mixed = Searcher(spread, members=(other,), weights=(1, 0)).sample_distinct(db, 4, temperature=1.2, seed=6, keys=KEYS)
    for x, y in zip(mixed, base):
        assert torch.equal(x, y) if x.dtype != torch.float32 else torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_bad_arguments_are_refused(setup):
    from fira_icse_amd.decode import Searcher
    cfg, store, ids, spread, db = setup
    name, d, n, temp, a = next(c for c in sbs_ref.kernel_cases() if c[2] == 2)
    sentinel = None
    for kw, dd in ((dict(n=0), d), (dict(n=9), d), (dict(temp=0.0), d), (dict(temp=float("inf")), d),
                   (dict(), dict(d, V=8))):
        rc, out = call_kernel(dd, kw.get("n", n), kw.get("temp", temp), a)
        assert rc != 0 and b"fira_beam_select_gumbel" in _lib.lib().fira_last_error(), kw
        assert (out["length"] == -7).all() and (out["G"] == 7.0).all() and (out["gen"] == -7).all()     # nothing was launched
    s = Searcher(spread)
    for kw in (dict(n=0), dict(n=9), dict(n=2, temperature=0.0), dict(n=2, temperature=float("inf")),
               dict(n=2, temperature=float("nan"))):
        with pytest.raises(ValueError, match="sample_distinct"):
            s.sample_distinct(db, kw.pop("n"), **kw)
    assert not any(k[0] == "sbs" for k in s._ws if isinstance(k, tuple))


# ------------------------------------------------------------------------------------------------ command line
def run(args, cwd, poison=False):
    """run_model.py in a fresh process; `poison`: the new kernel's binding and Searcher.sample_distinct raise when touched."""
    if not poison:
        return run_cli(args, cwd).stdout
    env = dict(os.environ, PYTHONPATH=util.REPO)
    code = ("import sys; sys.argv = ['run_model.py'] + %r\n"
            "import run_model\n"
            "from fira_icse_amd import _lib, decode\n"
            "def boom(*a, **k): raise AssertionError('the option-off path touched the new code')\n"
            "decode.Searcher.sample_distinct = boom\n"
            "decode.Searcher._sbs_steps = boom\n"
            "_lib.lib().fira_beam_select_gumbel = boom\n"
            "run_model.main()\n" % (args,))
    r = subprocess.run([sys.executable, "-c", code], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_cli_without_replacement_end_to_end(tmp_path):
    root = str(tmp_path)
    synth.write_dataset(root, util.load_golden_raw())
    torch.save(spread_state_dict(FiraConfig()), os.path.join(root, "best_model.pt"))
    base = ["test", "--splits", "16,4,4", "--test-batch-size", "3"]
    out_f, samp_f = os.path.join(root, "OUTPUT", "output_fira"), os.path.join(root, "OUTPUT", "output_fira_samples")
    run(base + ["--sample", "4", "--without-replacement", "--temperature", "1.5", "--sample-seed", "7", "--rerank", "mbr_bleu",
                "--no-repeat-ngram", "2"], root)
    lines = open(out_f).read().split("\n")
    recs = [json.loads(l) for l in open(samp_f).read().strip().split("\n")]
    assert len(lines) == 5 and lines[-1] == "" and len(recs) == 4
    for line, rec in zip(lines, recs):
        m = len(rec["candidates"])
        assert 1 <= m <= 4 and len(set(rec["candidates"])) == m
        assert len(rec["logp"]) == m and len(rec["key"]) == m and len(rec["mbr_bleu"]) == m
        assert all(a >= b for a, b in zip(rec["key"], rec["key"][1:])) and rec["key"][0] <= 0
        assert line in rec["candidates"]
    # without the option: the sampler as before, and the same bytes when the new code raises on any touch
    opts = ["--sample", "3", "--temperature", "1.5", "--top-p", "0.9", "--sample-seed", "7"]
    run(base + opts, root)
    best, samples = open(out_f).read(), open(samp_f).read()
    assert all("key" not in json.loads(l) for l in samples.strip().split("\n"))
    os.remove(out_f), os.remove(samp_f)
    run(base + opts, root, poison=True)
    assert open(out_f).read() == best and open(samp_f).read() == samples
