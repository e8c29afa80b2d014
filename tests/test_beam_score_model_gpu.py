"""``Searcher.beam(..., scoring=BeamScoring(...))`` on the golden fixture model and commits: the inactive value is today's search,
an active one is deterministic over graphs / chunks / runs, composes with merge and constraints, every step of it is a valid
selection under the numpy statement (beamscore_ref.py), and the command line writes what it says."""
import json
import os

import numpy as np
import pytest
import torch

import util
import beamscore_ref as R
from search_kit import golden_search, run_cli
from fira_icse_amd import synth
from fira_icse_amd.config import FiraConfig
from fira_icse_amd.decode import BeamScoring, Constraints, _Loop

pytestmark = pytest.mark.gpu

SC = BeamScoring(length_alpha=1.0, groups=2, diversity=0.5)
BEAM = 4
B = 3


@pytest.fixture(scope="module")
def setup():
    """The golden synthetic commits under the peaked weights of the decode parity tests (util.peaked_state_dict, seed 2).  Under
    unsharpened weights the probability product of a hypothesis that a length penalty keeps running underflows fp32 to 0 within
    a dozen steps, every key is -inf and the search decides nothing."""
    g = golden_search(weights="peaked", batch=B, seed=2)
    return g.cfg, g.model, g.db, g.searchers[0]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_inactive_scoring_is_todays_search(setup):
    from fira_icse_amd.decode import Searcher
    cfg, model, db, search = setup
    fresh = Searcher(model)
    for use_graphs in (False, True):
        plain = tuple(t.clone() for t in search.beam(db, 3, use_graphs=use_graphs))
        for sc in (None, BeamScoring()):
            got = fresh.beam(db, 3, use_graphs=use_graphs, scoring=sc)
            assert len(got) == 3 and same(got, plain)
    assert set(fresh._ws) == {(db.B, 3), ("beam", db.B, 3)}
    st = fresh._ws[("beam", db.B, 3)]
    assert "scoring" not in st and "key" not in st and "inv_lp" not in st
    with pytest.raises(ValueError, match="beam"):
        fresh.beam(db, 1, scoring=BeamScoring(1.0))
    with pytest.raises(ValueError, match="divide"):
        fresh.beam(db, 3, scoring=SC)
    with pytest.raises(ValueError, match="BeamScoring"):
        fresh.beam(db, 4, scoring="length")
    assert set(fresh._ws) == {(db.B, 3), ("beam", db.B, 3)}          # refused before any state


def test_active_scoring_same_bits_over_graphs_chunks_and_runs(setup):
    cfg, model, db, search = setup
    want = tuple(t.clone() for t in search.beam(db, BEAM, chunk=1, use_graphs=False, scoring=SC))
    assert len(want) == 4 and want[3].shape == (db.B, BEAM) and want[3].dtype == torch.float32
    for chunk, use_graphs in ((4, True), (4, False), (4, True), (1, False)):     # captured, eager, replayed, eager
        assert same(search.beam(db, BEAM, chunk=chunk, use_graphs=use_graphs, scoring=SC), want), (chunk, use_graphs)
    key = ("beam", db.B, BEAM, SC)
    assert key in search._ws and search._ws[key]["inv_lp"].shape == (cfg.tar_len + 1,) and search._ws[key]["graphs"] is not None
    # the key of every slot is ln(prob) * inv_lp[length - 1], -inf at probability 0, and best() picks by it
    gen, length, prob, k = (t.cpu() for t in want)
    inv = R.inv_lp_table(SC.length_alpha, cfg.tar_len)
    ref = R.key64(prob.numpy(), inv[(length.numpy() - 1).clip(0, cfg.tar_len)])
    finite = np.isfinite(ref)
    assert (finite == np.isfinite(k.numpy())).all() and (k.numpy()[~finite] == -np.inf).all()
    assert finite.any() and np.abs(ref[finite] - k.numpy().astype(np.float64)[finite]).max() <= R.TOL
    best = search.best(*want[:2], want[3])
    for b in range(db.B):
        j = int(np.argmax(k[b].numpy()))
        assert best[b] == gen[b, j, :int(length[b, j])].tolist()
    # and the search is another one than today's at the same beam
    plain = search.beam(db, BEAM)
    assert not same(plain, want[:3])


def test_composes_with_merge_and_constraints(setup):
    cfg, model, db, search = setup
    con = Constraints(no_repeat_ngram=2)
    gen, length, prob, key = (t.cpu() for t in search.beam(db, BEAM, scoring=SC, merge_copies=True, constraints=con))
    assert ("beam", db.B, BEAM, "merge", con, SC) in search._ws
    n_checked = 0
    for b in range(db.B):
        for j in range(BEAM):
            if prob[b, j] > 0:
                words = gen[b, j, 1:int(length[b, j])].tolist()
                grams = list(zip(words, words[1:]))
                assert len(grams) == len(set(grams)), (b, j, words)
                assert key[b, j] > float("-inf")
                n_checked += 1
            else:
                assert key[b, j] == float("-inf")
    print("hypotheses of positive probability: %d of %d" % (n_checked, db.B * BEAM))
    assert n_checked >= 1
    again = search.beam(db, BEAM, scoring=SC, merge_copies=True, constraints=con)
    assert same([t.cpu() for t in again], [gen, length, prob, key])


@pytest.mark.parametrize("sc, beam", [(SC, 4), (BeamScoring(length_alpha=0.6), 3), (BeamScoring(0.0, 3, 2.0), 3)],
                         ids=["a1-G2-l0.5-beam4", "a0.6-beam3", "G3-l2-beam3"])
def test_every_step_is_a_valid_selection(setup, sc, beam):
    """``_beam_steps`` one step at a time: after each step the state it read (the ``cur`` buffers, ``fin`` / ``active`` / ``done`` of
    prepare, the step's ``dist``) and the state it wrote are copied back and held against the statement, so a divergence of the
    trajectories can neither hide nor fake an error."""
    cfg, model, db, search = setup
    search.beam(db, beam, use_graphs=False, scoring=sc)               # builds the state under its key
    loop = _Loop(search, db, beam, search._key(("beam", db.B, beam), False, None, sc), None, 1, False)
    st, ws = loop.st, loop.ws
    search._beam_reset(st, db.B, beam)
    T, V = cfg.tar_len, cfg.vocab_size
    inv = R.inv_lp_table(sc.length_alpha, T)
    assert torch.equal(st["inv_lp"].cpu(), torch.from_numpy(inv))
    sou, sub = db.sou.cpu().numpy(), db.sub_token.cpu().numpy()
    n = lambda t: t.cpu().numpy()
    steps_checked = 0
    for step in range(T - 1):
        cur, nxt = step & 1, (step + 1) & 1
        search._beam_steps(st, ws, db.B, beam, step, step + 1)
        torch.cuda.synchronize()
        gen_in, len_in, prob_in = n(st["gen"][cur]).reshape(db.B, beam, T), n(st["length"][cur]).reshape(db.B, beam), n(st["prob"][cur]).reshape(db.B, beam)
        gen_out, len_out, prob_out = n(st["gen"][nxt]).reshape(db.B, beam, T), n(st["length"][nxt]).reshape(db.B, beam), n(st["prob"][nxt]).reshape(db.B, beam)
        parent, key = n(st["parent"]).reshape(db.B, beam), n(st["key"]).reshape(db.B, beam)
        if int(st["done"].item()):                                   # the latch: the state is copied through
            assert (gen_out == gen_in).all() and (len_out == len_in).all() and prob_out.tobytes() == prob_in.tobytes()
            break
        fin, active, dist = n(st["fin"]).reshape(db.B, beam), n(st["active"]), n(st["dist"]).reshape(db.B, beam, -1)
        for b in range(db.B):
            R.check_step(dist[b], fin[b], active, prob_in[b], len_in[b], gen_in[b].astype(np.int64), R.words_of(sou[b], sub[b], V), inv,
                         sc.groups, sc.diversity, (gen_out[b].astype(np.int64), len_out[b].astype(np.int64), prob_out[b],
                                                   parent[b] - b * beam, key[b]))
        steps_checked += 1
    assert steps_checked >= 2
    if sc.groups > 1:                                                # the reset seeded every group
        search._beam_reset(st, db.B, beam)
        seeded = n(st["prob"][0]).reshape(db.B, beam)
        assert (seeded[:, ::beam // sc.groups] == 1).all() and seeded.sum() == db.B * sc.groups


# ------------------------------------------------------------------------------------------------ command line
def test_cli_scored_search_and_options_off(tmp_path):
    from fira_icse_amd.model import reference_init_state_dict
    root = str(tmp_path)
    cfg = FiraConfig()
    synth.write_dataset(root, util.load_golden_raw())
    torch.manual_seed(0)
    torch.save(util.peaked_state_dict(reference_init_state_dict(cfg), seed=2), os.path.join(root, "best_model.pt"))
    base = ["test", "--splits", "16,4,4", "--test-batch-size", "3"]
    out_f, nbest_f = os.path.join(root, "OUTPUT", "output_fira"), os.path.join(root, "OUTPUT", "output_fira_nbest")
    # without the options: the output recorded before they existed, byte for byte, and an n-best line without a key
    run_cli(base + ["--nbest"], root)
    gold = json.load(open(os.path.join(util.GOLDEN, "decode_ref.json")))["beam3"]
    assert open(out_f, "rb").read() == "".join(l + "\n" for l in gold).encode()
    for rec in open(nbest_f).read().split("\n")[:-1]:
        assert sorted(json.loads(rec)) == ["messages", "prob"]
    os.remove(nbest_f)
    run_cli(base + ["--beam", "4", "--beam-groups", "2", "--diversity-penalty", "0.5", "--length-penalty", "1", "--nbest"], root)
    lines = open(out_f).read().split("\n")
    recs = open(nbest_f).read().split("\n")
    assert len(lines) == 5 and lines[-1] == "" and len(recs) == 5 and recs[-1] == ""
    for line, rec in zip(lines[:-1], recs[:-1]):
        rec = json.loads(rec)
        assert sorted(rec) == ["key", "messages", "prob"] and 1 <= len(rec["messages"]) == len(rec["prob"]) == len(rec["key"]) <= 4
        assert rec["key"] == sorted(rec["key"], reverse=True) and all(p > 0 for p in rec["prob"])
        assert rec["messages"][0] == line
