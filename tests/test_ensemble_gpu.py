"""Ensemble decoding on the device: fira_mix_dist alone on synthetic rows against the numpy statement (ensemble_ref.py), then
``Searcher(model, members=...)``'s ``beam`` / ``greedy`` / ``greedy_many`` against the host loops of the same file, plain and composed
with ``merge_copies``, ``Constraints`` and ``BeamScoring``, the two properties that need no loop (weights (1, 0); the same model
twice), the flag-off path, the refusals, and the command line with ``--ensemble``."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import util
import beamscore_ref as BS
import ensemble_ref as E
from search_kit import best_pair, bits, count_calls, golden_search, last_error, offset_rows, outside_untouched, run_cli, same_search
from fira_icse_amd import _lib, synth
from fira_icse_amd.config import UNK, FiraConfig
from fira_icse_amd.decode import BeamScoring, Constraints, _Loop, ensemble_weights

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the kernel alone
SENTINEL = -3.0


class Rows:
    """[R, W] floats that start ``offset`` floats into a zeroed buffer."""

    def __init__(self, n_rows, W, offset, fill=None):
        values = fill if isinstance(fill, np.ndarray) else np.full((n_rows, W), 0.0 if fill is None else fill, dtype=np.float32)
        self.n, self.offset = n_rows * W, offset
        self.buf, self.view = offset_rows(values, offset)

    def outside_is_untouched(self):
        return outside_untouched(self.buf, self.offset, self.n)


def mix_call(members, weights, out, best_id, best_p, n_members=None):
    """The entry as the Searcher calls it; returns its return code."""
    n_rows, W = members[0].view.shape
    ptrs = (C.c_void_p * len(members))(*[m.view.data_ptr() for m in members])
    w = (C.c_float * len(weights))(*[float(x) for x in weights])
    return _lib.lib().fira_mix_dist(_lib.cur_stream(), n_rows, W, len(members) if n_members is None else n_members, ptrs, w,
                                    _lib.ptr(out.view), _lib.ptr(best_id), _lib.ptr(best_p))


def run_kernel(case, alias, want_best, offsets=None, out_offset=1):
    """``out`` and every input start 1 float into a larger buffer (or ``offsets[m]`` / ``out_offset`` floats: every alignment
    phase).  ``alias``: out is member 0's buffer.  Asserts that nothing outside the rows, and no input but an aliased one, changed."""
    n_rows, W, n = case["R"], case["W"], case["M"]
    offsets = [1] * n if offsets is None else offsets
    members = [Rows(n_rows, W, offsets[m], case["dists"][m]) for m in range(n)]
    out = members[0] if alias else Rows(n_rows, W, out_offset, SENTINEL)
    best_id, best_p = best_pair(n_rows, want_best)
    _lib.check(mix_call(members, case["weights"], out, best_id, best_p), "fira_mix_dist")
    torch.cuda.synchronize()
    assert out.outside_is_untouched() and all(m.outside_is_untouched() for m in members)
    for m in range(1 if alias else 0, n):
        assert torch.equal(bits(members[m].view.cpu()), bits(case["dists"][m])), ("input changed", m)
    return out.view.cpu(), None if best_id is None else best_id.cpu(), None if best_p is None else best_p.cpu()


@pytest.mark.parametrize("c", E.CASES, ids=[c[0] for c in E.CASES])
def test_kernel_equals_the_reference_bit_for_bit(c):
    case = E.make_case(*c)
    out, best_id, best_p = E.reference(case)
    runs = [(alias, want_best, None, 1) for alias in (False, True) for want_best in (True, False)]
    # every pointer at another 16-byte phase (members m % 4, out 2 or -- in place -- member 0's 0), and everything aligned
    runs += [(False, True, [m % 4 for m in range(case["M"])], 2), (True, True, [m % 4 for m in range(case["M"])], 0),
             (False, True, [0] * case["M"], 0)]
    for alias, want_best, offsets, out_offset in runs:
        got, gid, gp = run_kernel(case, alias, want_best, offsets, out_offset)
        assert torch.equal(bits(got), bits(out)), (case["name"], alias, want_best, offsets)
        if want_best:
            assert gid.tolist() == best_id.tolist(), (case["name"], alias, offsets)
            assert torch.equal(bits(gp), bits(best_p)), (case["name"], alias, offsets)


def test_nan_never_wins_and_an_all_nan_row_reports_index_0():
    case = E.make_case("nan", 3, 45, 2, None)
    case["dists"][1][0, 7] = np.float32("nan")                # beside the tie trap of row 0
    case["dists"][0][1, 20] = np.float32("nan")               # beside the flip trap of row 1
    case["dists"][0][2, :] = np.float32("nan")
    out = E.mix(case["dists"], case["weights"])
    assert np.isnan(out[0, 7]) and np.isnan(out[1, 20]) and np.isnan(out[2]).all()
    got, gid, gp = run_kernel(case, False, True)
    assert torch.equal(torch.isnan(got), torch.from_numpy(np.isnan(out)))
    (a, b), (i, j, k) = case["traps"]
    assert gid.tolist() == [a, k, 0]
    assert gp[0] == float(np.nanmax(out[0])) and gp[1] == float(np.nanmax(out[1])) and gp[2] == float("-inf")


@pytest.mark.parametrize("name, n_members, weights, word", [
    ("one member", 1, (1.0,), "n_members = 1"), ("nine members", 9, (0.125,) * 9, "n_members = 9"),
    ("negative weight", 2, (1.5, -0.5), "weight 1"), ("nan weight", 2, (0.5, float("nan")), "weight 1")])
def test_invalid_arguments_return_non_zero_with_a_message_and_launch_nothing(name, n_members, weights, word):
    members = [Rows(4, 45, 1, 0.5) for _ in range(n_members)]
    out = Rows(4, 45, 1, SENTINEL)
    best_id = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    best_p = torch.full((4,), -7.0, dtype=torch.float32, device="cuda")
    assert mix_call(members, weights, out, best_id, best_p) != 0
    msg = last_error()
    assert "fira_mix_dist" in msg and word in msg, msg
    torch.cuda.synchronize()
    assert bool((out.view == SENTINEL).all()) and bool((best_id == -7).all()) and bool((best_p == -7.0).all())


def test_a_captured_launch_bakes_pointers_and_weights_in_and_replays_the_same_bits():
    case = E.make_case(*E.CASES[1])
    want, best_id, best_p = E.reference(case)
    members = [Rows(case["R"], case["W"], 1, d) for d in case["dists"]]
    out = Rows(case["R"], case["W"], 1, SENTINEL)
    gid = torch.zeros(case["R"], dtype=torch.int32, device="cuda")
    gp = torch.zeros(case["R"], dtype=torch.float32, device="cuda")
    _lib.check(mix_call(members, case["weights"], out, gid, gp), "fira_mix_dist")      # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(mix_call(members, case["weights"], out, gid, gp), "fira_mix_dist")  # (the host arrays die with the call)
    for _ in range(2):
        out.view.fill_(SENTINEL)
        gid.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out.view.cpu()), bits(want)) and gid.cpu().tolist() == best_id.tolist()
        assert torch.equal(bits(gp.cpu()), bits(best_p))


# ------------------------------------------------------------------------------------------------ through the models
CON = Constraints(2, 3, (UNK,))
SC = BeamScoring(length_alpha=1.0, groups=2, diversity=0.5)
# (torch seed of the initialisation, seed of util.peaked_state_dict) per model: A, B, C
MODEL_SEEDS = ((0, 2), (1, 3), (2, 4))
WEIGHTS3 = (0.5, 0.3, 0.2)
CONFIGS = {"plain": (False, None), "merge": (True, None), "constraints": (False, CON), "merge-constraints": (True, CON)}


def make_model(cfg, init_seed, peak_seed):
    from fira_icse_amd.model import TransModel, reference_init_state_dict
    torch.manual_seed(init_seed)
    model = TransModel(cfg, init=False)
    model.load_state_dict(util.peaked_state_dict(reference_init_state_dict(cfg), seed=peak_seed))
    model.eval()
    return model


@pytest.fixture(scope="module")
def setup():
    """The golden synthetic commits (B = 4) under three peaked models: different initialisations, different perturbations."""
    from fira_icse_amd.decode import Searcher
    g = golden_search(weights="peaked", searchers=0, seed=MODEL_SEEDS[0][1])
    assert MODEL_SEEDS[0][0] == 0                              # (the kit's torch seed)
    cfg, db = g.cfg, g.db
    models = [g.model] + [make_model(cfg, *s) for s in MODEL_SEEDS[1:]]
    singles = [Searcher(m) for m in models]
    ens3 = Searcher(models[0], members=models[1:], weights=WEIGHTS3)
    return dict(cfg=cfg, db=db, models=models, singles=singles, ens3=ens3, w3=ensemble_weights(WEIGHTS3, 3),
                sou=db.sou.cpu().numpy(), sub=db.sub_token.cpu().numpy(), dims=E.dims_of(cfg))


@pytest.fixture(scope="module")
def refs(setup):
    """The reference loops of the three-model ensemble, each run once on first use and then shared, never modified."""
    cache = {}

    def get(kind, config):
        if (kind, config) not in cache:
            merge, con = CONFIGS[config]
            s = setup
            if kind == "greedy":
                res = E.greedy_ensemble(s["singles"], s["w3"], s["db"], E.make_edit(s["sou"], s["sub"], s["dims"], 1, merge, con))[:3]
            else:
                res = E.beam_ensemble(s["singles"], s["w3"], s["db"], kind, E.make_edit(s["sou"], s["sub"], s["dims"], kind, merge, con))
            cache[kind, config] = res
        return cache[kind, config]
    return get


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("beam", [3, 4])
def test_beam_equals_the_reference_loop(setup, refs, beam, config):
    merge, con = CONFIGS[config]
    want = refs(beam, config)
    for use_graphs in (False, True, True):                    # eager, captured, replayed
        same_search(setup["ens3"].beam(setup["db"], beam, use_graphs=use_graphs, constraints=con, merge_copies=merge), want)


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_greedy_and_greedy_many_equal_the_reference_loop(setup, refs, config):
    merge, con = CONFIGS[config]
    db, search = setup["db"], setup["ens3"]
    want = refs("greedy", config)
    for use_graphs in (False, True, True):
        same_search(search.greedy(db, use_graphs=use_graphs, constraints=con, merge_copies=merge), want)
    many = search.greedy_many([db, db, db], in_flight=3, constraints=con, merge_copies=merge)
    torch.cuda.synchronize()
    assert len(many) == 3
    for got in many:
        same_search(got, want)


def test_scored_beam_every_step_mixes_what_the_reference_mixes_and_selects_validly(setup):
    """Beam 4 under BeamScoring(1.0, groups=2, 0.5) with merge and constraints, ``_beam_steps`` one step at a time, by the rule of
    test_beam_score_model_gpu.py: after each step the distribution the selection read must be, bit for bit, the numpy mix of the
    members' own single-model steps on the same tokens and parents with the edit hook applied, and the state the step wrote must
    be a valid selection under beamscore_ref.check_step (same tolerance: BS.TOL)."""
    cfg, db, search = setup["cfg"], setup["db"], setup["ens3"]
    beam, B, T, V = 4, setup["db"].B, setup["cfg"].tar_len, setup["cfg"].vocab_size
    got = search.beam(db, beam, scoring=SC, merge_copies=True, constraints=CON)           # builds the state under its key
    assert len(got) == 4
    again = search.beam(db, beam, use_graphs=False, scoring=SC, merge_copies=True, constraints=CON)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    loop = _Loop(search, db, beam, search._key(("beam", B, beam), True, CON, SC), None, 1, False)
    st, ws = loop.st, loop.ws
    search._beam_reset(st, B, beam)
    ref = E.RefEnsemble(setup["singles"], setup["w3"])
    ref_ws = ref._begin(db, beam)
    edit = E.make_edit(setup["sou"], setup["sub"], setup["dims"], beam, True, CON)
    inv = BS.inv_lp_table(SC.length_alpha, T)
    ref_dist = torch.zeros((B * beam, cfg.out_len), dtype=torch.float32, device="cuda")
    n = lambda t: t.cpu().numpy()
    steps_checked, prev_parent = 0, None
    for step in range(T - 1):
        cur, nxt = step & 1, (step + 1) & 1
        search._beam_steps(st, ws, B, beam, step, step + 1)
        torch.cuda.synchronize()
        gen_in, len_in, prob_in = n(st["gen"][cur]).reshape(B, beam, T), n(st["length"][cur]).reshape(B, beam), n(st["prob"][cur]).reshape(B, beam)
        gen_out, len_out, prob_out = n(st["gen"][nxt]).reshape(B, beam, T), n(st["length"][nxt]).reshape(B, beam), n(st["prob"][nxt]).reshape(B, beam)
        parent, key = n(st["parent"]).reshape(B, beam), n(st["key"]).reshape(B, beam)
        if int(st["done"].item()):
            break
        ref._step(ref_ws, B, beam, step, st["tok"], prev_parent, ref_dist, None, None)
        want = edit(n(ref_dist), gen_in.reshape(B * beam, T), len_in.reshape(B * beam))
        assert torch.equal(bits(st["dist"].cpu()), bits(want)), step
        fin, active, dist = n(st["fin"]).reshape(B, beam), n(st["active"]), n(st["dist"]).reshape(B, beam, -1)
        for b in range(B):
            BS.check_step(dist[b], fin[b], active, prob_in[b], len_in[b], gen_in[b].astype(np.int64),
                          BS.words_of(setup["sou"][b], setup["sub"][b], V), inv, SC.groups, SC.diversity,
                          (gen_out[b].astype(np.int64), len_out[b].astype(np.int64), prob_out[b], parent[b] - b * beam, key[b]))
        prev_parent = st["parent"].clone()
        steps_checked += 1
    assert steps_checked >= 2


def test_weights_one_and_zero_are_the_primary_alone(setup):
    """1 * p + 0 * q == p bit for bit for finite q >= 0: the very tensors of the single-model search."""
    from fira_icse_amd.decode import Searcher
    db, (a, b, c) = setup["db"], setup["models"]
    ens, single = Searcher(a, members=(b,), weights=(1, 0)), setup["singles"][0]
    for use_graphs in (False, True):
        for got, want in ((ens.greedy(db, use_graphs=use_graphs), single.greedy(db, use_graphs=use_graphs)),
                          (ens.beam(db, 3, use_graphs=use_graphs), single.beam(db, 3, use_graphs=use_graphs))):
            assert len(got) == len(want) == 3 and all(torch.equal(x, y) for x, y in zip(got, want))


def test_the_same_model_twice_is_the_model(setup):
    """A second instance loaded from the same state dict: 0.5 p + 0.5 p == p except for subnormal p, so the ids are the single
    model's and the probabilities agree within 1e-6 relative."""
    from fira_icse_amd.decode import Searcher
    db, single = setup["db"], setup["singles"][0]
    ens = Searcher(setup["models"][0], members=(make_model(setup["cfg"], *MODEL_SEEDS[0]),))
    for got, want in ((ens.greedy(db), single.greedy(db)), (ens.beam(db, 3), single.beam(db, 3))):
        (gen, length, p), (gen_t, len_t, p_t) = [tuple(t.cpu() for t in x) for x in (got, want)]
        assert torch.equal(length, len_t)
        live = torch.arange(gen.shape[-1])[(None,) * (gen.dim() - 1)] < length[..., None]
        assert torch.equal(gen * live, gen_t * live)
        assert bool(((p - p_t).abs() <= 1e-6 * p_t.abs()).all())


def test_the_ensemble_is_not_one_of_its_members(setup):
    """Non-vacuity, decided on the reference loop: for at least one commit the uniform ensemble of (A, B) emits a greedy or a
    beam-3 message that neither A alone nor B alone emits under the same search."""
    db, singles = setup["db"], setup["singles"][:2]
    w = ensemble_weights(None, 2)
    ident = E.make_edit(setup["sou"], setup["sub"], setup["dims"], 1)
    msgs = lambda s, res: [tuple(m) for m in s.best(*[t for t in res[:3]])]
    new = 0
    for kind in ("greedy", 3):
        if kind == "greedy":
            ens = E.greedy_ensemble(singles, w, db, ident)[:3]
            alone = [tuple(t.cpu() for t in s.greedy(db)) for s in singles]
        else:
            ens = E.beam_ensemble(singles, w, db, 3, ident)
            alone = [tuple(t.cpu() for t in s.beam(db, 3)) for s in singles]
        e, a, b = msgs(singles[0], ens), msgs(singles[0], alone[0]), msgs(singles[0], alone[1])
        fresh = [k for k in range(db.B) if e[k] != a[k] and e[k] != b[k]]
        print("%s: commits whose ensemble message is neither member's: %s; members differ on %s"
              % (kind, fresh, [k for k in range(db.B) if a[k] != b[k]]))
        new += len(fresh)
    assert new >= 1


def test_flag_off_is_todays_search(setup, monkeypatch):
    """members=(): today's state keys, buffers and library calls per step; with members only ``_step`` changes what is called."""
    from fira_icse_amd.decode import Searcher
    cfg, db, model = setup["cfg"], setup["db"], setup["models"][0]
    B = db.B
    fresh, today = Searcher(model, members=()), setup["singles"][0]
    for use_graphs in (True, False):
        for got, want in ((fresh.beam(db, 3, use_graphs=use_graphs), today.beam(db, 3, use_graphs=use_graphs)),
                          (fresh.greedy(db, use_graphs=use_graphs), today.greedy(db, use_graphs=use_graphs))):
            assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert fresh.members == () and fresh.weights is None
    assert set(fresh._ws) == {(B, 3), (B, 1), ("beam", B, 3), ("greedy", B)}
    assert torch.is_tensor(fresh._ws[(B, 3)]) and fresh._ws[(B, 3)].dtype == torch.uint8
    assert set(fresh._ws[("greedy", B)]) == {"out", "length", "prob", "alive", "tok", "n_alive", "best_id", "best_p", "con", "sou",
                                             "sub", "graphs", "chunk", "bounds"}
    assert set(fresh._ws[("beam", B, 3)]) == {"gen", "length", "prob", "tok", "parent", "fin", "active", "done", "dist", "con",
                                              "sou", "sub", "graphs", "chunk", "bounds"}
    g, b = fresh._ws[("greedy", B)], fresh._ws[("beam", B, 3)]
    assert count_calls(monkeypatch, lambda: fresh._greedy_steps(g, fresh._ws[(B, 1)], B, 0, 1)) == \
        {"fira_decode_step_ex": 1, "fira_greedy_advance": 1}
    assert count_calls(monkeypatch, lambda: fresh._beam_steps(b, fresh._ws[(B, 3)], B, 3, 0, 1)) == \
        {"fira_beam_prepare": 1, "fira_decode_step_ex": 1, "fira_beam_select": 1}
    assert count_calls(monkeypatch, lambda: fresh._begin(db, 3)) == {"fira_decode_begin_ex": 1}
    # the three-model ensemble: the same state keys, one workspace and one buffer per member, M steps and one mix per step
    ens = setup["ens3"]
    ens.greedy(db)
    ens.beam(db, 3)
    assert {("greedy", B), ("beam", B, 3), (B, 1), (B, 3), ("members", B, 1), ("members", B, 3), ("member", 1, B, 3),
            ("member", 2, B, 3)} <= set(ens._ws)
    assert set(ens._ws[("greedy", B)]) == set(g) and set(ens._ws[("beam", B, 3)]) == set(b)
    mem = ens._ws[("members", B, 3)]
    assert len(mem.ws) == len(mem.dist) == 3 and all(d.shape == (B * 3, cfg.out_len) for d in mem.dist)
    assert count_calls(monkeypatch, lambda: ens._greedy_steps(ens._ws[("greedy", B)], ens._ws[("members", B, 1)], B, 0, 1)) == \
        {"fira_decode_step_ex": 3, "fira_mix_dist": 1, "fira_greedy_advance": 1}
    assert count_calls(monkeypatch, lambda: ens._beam_steps(ens._ws[("beam", B, 3)], mem, B, 3, 0, 1)) == \
        {"fira_beam_prepare": 1, "fira_decode_step_ex": 3, "fira_mix_dist": 1, "fira_beam_select": 1}
    assert count_calls(monkeypatch, lambda: ens._begin(db, 3)) == {"fira_decode_begin_ex": 3}


def test_sample_and_score_refuse_an_ensemble_and_launch_nothing(setup, monkeypatch):
    from fira_icse_amd.decode import Searcher
    db, (a, b, c) = setup["db"], setup["models"]
    ens = Searcher(a, members=(b,))
    cand = torch.tensor([[2, 5, 1]] * db.B)

    def run():
        with pytest.raises(ValueError, match="sample does not combine with an ensemble"):
            ens.sample(db, 2)
        with pytest.raises(ValueError, match="score does not combine with an ensemble"):
            ens.score(db, cand)
    assert count_calls(monkeypatch, run) == {} and ens._ws == {}


# ------------------------------------------------------------------------------------------------ command line
@pytest.fixture(scope="module")
def cli_root(tmp_path_factory):
    from fira_icse_amd.model import reference_init_state_dict
    root = str(tmp_path_factory.mktemp("ensemble_cli"))
    cfg = FiraConfig()
    synth.write_dataset(root, util.load_golden_raw())
    sds = []
    for (init_seed, peak_seed), name in zip(MODEL_SEEDS[:2], ("best_model.pt", "second.pt")):
        torch.manual_seed(init_seed)
        sds.append(util.peaked_state_dict(reference_init_state_dict(cfg), seed=peak_seed))
        torch.save(sds[-1], os.path.join(root, name))
    return root, os.path.join(root, "second.pt")


BASE = ["test", "--splits", "16,4,4", "--test-batch-size", "4"]


def test_cli_ensemble_writes_what_the_python_api_gives(setup, cli_root):
    """Beam 3 and --beam 1 with a second checkpoint: the lines of OUTPUT/output_fira are the detokenised best messages of
    ``Searcher(A, members=(B,))`` on the same commits (the test split of the golden data set is the fixture's batch)."""
    from fira_icse_amd import text
    from fira_icse_amd.decode import Searcher
    root, second = cli_root
    db, (a, b, c) = setup["db"], setup["models"]
    vocab = json.load(open(os.path.join(root, "DataSet", "word_vocab.json")))
    var_maps = json.load(open(os.path.join(root, "DataSet", "variable.json")))
    r_vocab = {v: k for k, v in vocab.items()}
    ens = Searcher(a, members=(b,))
    for beam in (3, 1):
        run_cli(BASE + ["--ensemble", second, "--beam", str(beam)], root)
        test_index = json.load(open(os.path.join(root, "all_index")))["test"]      # (written by the first run)
        lines = open(os.path.join(root, "OUTPUT", "output_fira")).read().split("\n")
        hyps = ens.best(*(ens.beam(db, 3) if beam == 3 else ens.greedy(db)))
        want = [text.detokenize(h, r_vocab, var_maps[test_index[i]]) for i, h in enumerate(hyps)]
        assert lines[-1] == "" and lines[:-1] == want, beam


def test_cli_weights_one_and_zero_are_byte_identical_to_no_ensemble(cli_root):
    root, second = cli_root
    out_f = os.path.join(root, "OUTPUT", "output_fira")
    run_cli(BASE, root)
    plain = open(out_f, "rb").read()
    os.remove(out_f)
    run_cli(BASE + ["--ensemble", second, "--ensemble-weights", "1,0"], root)
    assert open(out_f, "rb").read() == plain and len(plain.split(b"\n")) == 5


def test_cli_ensemble_with_nbest_and_merge_copies(cli_root):
    root, second = cli_root
    out_f, nbest_f = os.path.join(root, "OUTPUT", "output_fira"), os.path.join(root, "OUTPUT", "output_fira_nbest")
    run_cli(BASE + ["--ensemble", second, "--nbest", "--merge-copies"], root)
    lines = open(out_f).read().split("\n")
    recs = open(nbest_f).read().split("\n")
    assert len(lines) == 5 and lines[-1] == "" and len(recs) == 5 and recs[-1] == ""
    for line, rec in zip(lines[:-1], recs[:-1]):
        rec = json.loads(rec)
        assert sorted(rec) == ["messages", "prob"] and 1 <= len(rec["messages"]) == len(rec["prob"]) <= 3
        assert rec["messages"][0] == line
        assert all(p > 0 for p in rec["prob"]) and rec["prob"] == sorted(rec["prob"], reverse=True)
        assert len(set(rec["messages"])) == len(rec["messages"]), rec
