"""Soft word penalties and biases, the parts that need no GPU: the ABI and every argument check of ``fira_penalise_dist``,
``decode.Penalties`` and its ``check``, its tables against the numpy statement (penalty_ref.py) as bits, the statement itself on
hand-written rows, and the searches that refuse ``penalties=`` ahead of any device work."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import penalty_ref as ref
import util
from search_kit import bits, device_dims as dims
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, PAD, START, UNK, FiraConfig
from fira_icse_amd.decode import Penalties

A, B_, C_, D = 10, 11, 12, 13          # four ordinary words


# ------------------------------------------------------------------------------------------------ ABI and argument checks
def test_header_declares_library_exports_and_the_binding_matches():
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    assert "#define FIRA_ABI_VERSION 11" in header
    m = re.search(r"\bint\s+fira_penalise_dist\s*\(([^;]*)\)\s*;", header)
    assert m, "fira_penalise_dist is not declared"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    kinds = "".join("P" if "*" in p else "F" if p.startswith("float") else "I" for p in params)
    assert kinds == "PPIIPPPPPPPPPPP"
    res, args = _lib.SIGNATURES["fira_penalise_dist"]
    assert res is _lib._I and len(args) == len(kinds) and args[1] is _lib._DP
    assert all(t in ((_lib._P, _lib._DP) if k == "P" else (_lib._I,)) for t, k in zip(args, kinds))
    lib = _lib.lib()
    assert lib.fira_abi_version() == 11 and hasattr(lib, "fira_penalise_dist")
    assert '"penalise.hip"' in open(os.path.join(util.REPO, "fira_icse_amd", "build.py")).read()
    assert "`fira_penalise_dist`" in open(os.path.join(util.REPO, "INTEGRATION.md")).read()


def call(d=None, R_=6, rpc=3, gen=16, length=16, sou=16, sub=16, table=16, bias_id=16, bias_factor=16, n_bias=16, dist=16,
         best_id=16, best_p=16):
    """fira_penalise_dist with pointers that are never dereferenced (every case here fails a check, or R = 0)."""
    p = lambda v: None if v is None else C.c_void_p(v)
    d = d if d is not None else dims()
    return _lib.lib().fira_penalise_dist(None, C.byref(d), R_, rpc, p(gen), p(length), p(sou), p(sub), p(table), p(bias_id),
                                         p(bias_factor), p(n_bias), p(dist), p(best_id), p(best_p))


BAD_CALLS = {
    "negative R": (dict(R_=-1, rpc=1), "R = -1"),
    "rows_per_commit 0": (dict(rpc=0), "rows_per_commit"),
    "rows_per_commit does not divide R": (dict(R_=7, rpc=3), "rows_per_commit"),
    "tar_len 65": (dict(d=dims(tar_len=65)), "tar_len"),
    "tar_len 1": (dict(d=dims(tar_len=1)), "tar_len"),
    "vocabulary too wide": (dict(d=dims(vocab=25601)), "vocabulary"),
    "vocabulary too small": (dict(d=dims(vocab=3)), "vocabulary"),
    "too many memory slots": (dict(d=dims(sou_len=900, sub_len=125)), "memory slots"),
    "best_id without best_p": (dict(best_p=None), "best_id and best_p"),
    "best_p without best_id": (dict(best_id=None), "best_id and best_p"),
    "null gen": (dict(gen=None), "gen"),
    "null length": (dict(length=None), "length"),
    "null sou": (dict(sou=None), "sou"),
    "null sub_token": (dict(sub=None), "sub_token"),
    "null dist": (dict(dist=None), "dist"),
    "null count_factor": (dict(table=None), "count_factor"),
    "null bias_id": (dict(bias_id=None), "bias_id"),
    "null bias_factor": (dict(bias_factor=None), "bias_factor"),
    "null n_bias": (dict(n_bias=None), "n_bias"),
}


@pytest.mark.parametrize("name", sorted(BAD_CALLS))
def test_argument_checks_fire_before_any_launch(name):
    kw, word = BAD_CALLS[name]
    assert call(**kw) != 0
    msg = _lib.lib().fira_last_error().decode()
    assert "fira_penalise_dist" in msg and word in msg, msg
    if name.startswith("null"):
        assert "null pointer" in msg, msg


def test_null_dims_is_refused_by_name():
    assert _lib.lib().fira_penalise_dist(None, None, 0, 1, *([None] * 11)) != 0
    msg = _lib.lib().fira_last_error().decode()
    assert "fira_penalise_dist" in msg and "dims" in msg, msg


def test_empty_call_is_a_no_op():
    assert call(R_=0) == 0
    none = dict(gen=None, length=None, sou=None, sub=None, table=None, bias_id=None, bias_factor=None, n_bias=None, dist=None,
                best_id=None, best_p=None)
    assert call(R_=0, **none) == 0                                  # R == 0 returns before the pointer checks
    # the limits themselves pass the checks (R = 0: nothing is launched)
    assert call(R_=0, d=dims(tar_len=64, vocab=25600, sou_len=512, sub_len=512)) == 0
    assert call(R_=0, d=dims(tar_len=2, vocab=4, sou_len=0, sub_len=0), best_id=None, best_p=None) == 0


# ------------------------------------------------------------------------------------------------ decode.Penalties
def test_penalties_value():
    p = Penalties()
    assert (p.presence, p.frequency, p.bias) == (0.0, 0.0, None) and not p.active
    assert not Penalties(bias={}).active and not Penalties(bias={A: 0.0}).active and not Penalties(bias=[None, {A: 0}]).active
    assert Penalties(presence=0.5).active and Penalties(frequency=1).active and Penalties(bias={A: -1}).active
    assert Penalties(bias=[{}, {A: 0.5}]).active
    assert Penalties(10, 10, {EOS: -30, UNK: 30}).bias == ((EOS, -30.0), (UNK, 30.0))
    assert Penalties(bias={B_: 1, A: 2}) == Penalties(bias={A: 2.0, B_: 1.0})            # stored sorted
    assert Penalties(bias=[{A: 1}, None]).bias == (((A, 1.0),), ())
    assert Penalties(bias={np.int64(A): np.float32(0.5)}).bias == ((A, 0.5),)
    with pytest.raises(Exception):
        p.presence = 1.0                                             # frozen
    cfg = FiraConfig()
    full = {UNK + k: 1.0 for k in range(16)}
    assert Penalties(bias=full).check(cfg, 4) is not None and Penalties(bias=[full] * 4).check(cfg, 4) is not None
    assert Penalties(bias={cfg.vocab_size - 1: -30.0, EOS: 3.0}).check(cfg, 1) is not None


@pytest.mark.parametrize("kw, word", [
    (dict(presence=-0.1), "presence"), (dict(presence=10.5), "presence"), (dict(presence=float("nan")), "presence"),
    (dict(presence="1"), "presence .* not a number"), (dict(presence=True), "presence .* not a number"),
    (dict(frequency=-1), "frequency"), (dict(frequency=11), "frequency"), (dict(frequency=float("inf")), "frequency"),
    (dict(frequency=None), "frequency .* not a number"),
    (dict(bias=5), "neither a mapping"), (dict(bias=[5]), "commit 0 .* not a mapping"), (dict(bias=[{A: 1}, (A, 1)]), "commit 1"),
    (dict(bias={A: 30.5}), "bias 30.5 of id 10 is outside"), (dict(bias={A: -31}), "outside"),
    (dict(bias={A: float("nan")}), "outside"), (dict(bias={A: "1"}), "not a number"), (dict(bias={A: True}), "not a number"),
    (dict(bias={PAD: 1.0}), "id 0 .*<pad> and <start>"), (dict(bias={START: 1.0}), "id 2 .*<pad> and <start>"),
    (dict(bias={-1: 1.0}), "id -1"), (dict(bias={4.0: 1.0}), "not an integer"), (dict(bias={True: 1.0}), "not an integer"),
    (dict(bias={UNK + k: 1.0 for k in range(17)}), "17 ids, more than 16"),
    (dict(bias=[{}, {UNK + k: 1.0 for k in range(17)}]), "commit 1: 17 ids"),
])
def test_penalties_refuses_bad_values(kw, word):
    with pytest.raises(ValueError, match=word):
        Penalties(**kw)


def test_penalties_against_the_model_and_the_batch():
    cfg = FiraConfig()
    assert cfg.tar_len == 30
    with pytest.raises(ValueError, match="id %d outside the vocabulary" % cfg.vocab_size):
        Penalties(bias={cfg.vocab_size: 1.0}).check(cfg, 2)
    with pytest.raises(ValueError, match="commit 1: id %d outside" % (cfg.vocab_size + 5)):
        Penalties(bias=[{A: 1.0}, {cfg.vocab_size + 5: 1.0}]).check(cfg, 2)
    with pytest.raises(ValueError, match="3 bias mappings for a batch of 4"):
        Penalties(bias=[{A: 1.0}, {}, None]).check(cfg, 4)
    # the overflow bound: max(b, 0) * (tar_len - 1) <= 87
    assert Penalties(bias={A: 3.0}).check(cfg, 1) is not None                            # 3.0 * 29 = 87
    with pytest.raises(ValueError, match=r"commit 0: the bias 3\.1 of id 10 .* 87"):
        Penalties(bias={A: 3.1}).check(cfg, 1)
    with pytest.raises(ValueError, match=r"commit 2: the bias 30 of id 11 .* 87"):
        Penalties(bias=[{}, {A: 3.0}, {B_: 30.0}]).check(cfg, 3)
    assert Penalties(bias={A: -30.0}).check(cfg, 1) is not None                          # a negative bias cannot overflow
    assert Penalties(bias={A: 30.0}).check(FiraConfig(tar_len=3), 1) is not None         # 30 * 2 = 60
    assert Penalties(presence=10, frequency=10).check(cfg, 7) is not None


@pytest.mark.parametrize("presence, frequency", [(0.0, 0.0), (0.5, 0.25), (0.0, 1.0), (2.0, 0.0), (10.0, 10.0), (0.1, 1.7)])
def test_tables_equal_the_statements_as_bits(presence, frequency):
    for T in (2, 8, 30, 64):
        got, want = Penalties(presence, frequency).table(T), ref.factor_table(presence, frequency, T)
        assert got.dtype == np.float32 and got.shape == (T,) and np.array_equal(bits(got).numpy(), bits(want).numpy())
        assert got[0] == 1.0
    assert Penalties(10.0, 10.0).table(64)[63] == 0.0 and Penalties(10.0, 10.0).table(64)[1] > 0           # underflow: a ban
    assert np.array_equal(Penalties().table(30), np.ones(30, dtype=np.float32))


def test_bias_arrays_equal_the_statements_as_bits():
    shared = {EOS: -1.5, B_: 3.0, A: -30.0, 400: 0.25}
    per = [{A: 1.0}, None, {}, {UNK + k: 0.1 * k - 0.8 for k in range(16)}]
    for bias, B in ((None, 3), (shared, 3), (per, 4)):
        got, want = Penalties(bias=bias).bias_arrays(B), ref.bias_arrays(bias, B)
        for g, w, dt, shape in zip(got, want, (np.int32, np.float32, np.int32), ((B, 16), (B, 16), (B,))):
            assert g.dtype == dt and g.shape == shape and np.array_equal(bits(g).numpy(), bits(w).numpy())
    ids, fac, n = Penalties(bias=per).bias_arrays(4)
    assert n.tolist() == [1, 0, 0, 16] and ids[0, 0] == A and fac[0, 0] == np.float32(np.e) and fac[1].tolist() == [1.0] * 16


# ------------------------------------------------------------------------------------------------ the reference statement
DIMS = (20, 4, 3)
SOU, SUB = [A, 5, A, EOS], [6, A, 7]
V, L, S = DIMS


def row_of(values=None):
    return np.linspace(0.25, 1.0, V + L + S, dtype=np.float32) if values is None else np.asarray(values, dtype=np.float32)


def test_counts_ignore_start_and_what_lies_past_the_length():
    gen = np.array([START, A, B_, A, A, 9, 9], dtype=np.int32)
    assert ref.counts(gen, 1) == {} and ref.counts(gen, 2) == {A: 1} and ref.counts(gen, 5) == {A: 3, B_: 1}
    assert ref.counts(gen, 0) == {} and ref.counts(gen, 99) == {A: 3, B_: 1, 9: 2}                          # the length is clamped
    assert ref.counts(np.array([START, START, START]), 3) == {START: 2}                                    # position 0 only


def test_a_word_is_scaled_through_generator_diff_and_sub_token_entries_at_once():
    table = np.array([7.0, 0.5, 0.25, 0.125, 0.0625, 0.03125], dtype=np.float32)                           # (t[0] is never read)
    gen = np.array([START, A, 5, A, 0, 0], dtype=np.int32)
    row = row_of()
    out = ref.edited(row, gen, 4, SOU, SUB, DIMS, table, [], [])
    twice, once = [A, V + 0, V + 2, V + L + 1], [5, V + 1]
    for i in range(V + L + S):
        want = row[i] * np.float32(0.25) if i in twice else row[i] * np.float32(0.5) if i in once else row[i]
        assert out[i] == want and out.dtype == np.float32, i
    # ids past the length are not part of the hypothesis
    gen2 = np.array([START, A, 5, A, 6, 7], dtype=np.int32)
    assert np.array_equal(ref.edited(row, gen2, 4, SOU, SUB, DIMS, table, [], []), out)
    assert np.array_equal(row, row_of())                                                                   # the input is not written


def test_bias_reaches_eos_and_slot_only_words_and_uses_the_first_of_equal_ids():
    table = np.ones(6, dtype=np.float32)
    gen = np.array([START, 0, 0, 0, 0, 0], dtype=np.int32)
    row = row_of()
    out = ref.edited(row, gen, 1, SOU, SUB, DIMS, table, [EOS, 7, 7, V + 5, -1], np.array([4.0, 0.5, 9.0, 3.0, 3.0], dtype=np.float32))
    changed = {EOS: 4.0, V + 3: 4.0, 7: 0.5, V + L + 2: 0.5}            # <eos> and its diff slot; word 7 and its sub-token slot
    for i in range(V + L + S):
        assert out[i] == row[i] * np.float32(changed.get(i, 1.0)), i      # ids outside [0, V) are ignored; 7's second factor too


def test_the_two_multiplications_round_separately_and_in_order():
    x, f1, f2 = np.float32(0.7), np.float32(np.exp(-0.75)), np.float32(np.exp(1.0))
    assert np.float32(np.float32(x * f1) * f2) != np.float32(np.float64(x) * np.float64(f1) * np.float64(f2))   # (a case that shows it)
    table = np.array([1.0, f1], dtype=np.float32)
    gen = np.array([START, A], dtype=np.int32)
    row = row_of(np.full(V + L + S, x))
    out = ref.edited(row, gen, 2, SOU, SUB, DIMS, table, [A], [f2])
    assert bits(out[[A]]).tolist() == bits(np.array([np.float32(np.float32(x * f1) * f2)])).tolist()
    assert out[A] == out[V] == out[V + 2] == out[V + L + 1] and out[5] == x


def test_a_finished_row_is_left_alone_and_a_zero_factor_bans():
    table = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    row = row_of()
    done = np.array([START, A, EOS], dtype=np.int32)
    assert np.array_equal(ref.edited(row, done, 3, SOU, SUB, DIMS, table, [5], [2.0]), row)
    out = ref.edited(row, done, 2, SOU, SUB, DIMS, table, [5], [2.0])      # the same ids one position shorter: not finished
    assert out[A] == 0.0 and out[V] == 0.0 and out[5] == row[5] * np.float32(2.0) and out[6] == row[6]
    assert ref.argmax_ref(np.array([0.25, 0.5, 0.5, 0.125], dtype=np.float32)) == (1, np.float32(0.5))


def test_make_edit_chains_after_the_links_before_it():
    table = np.array([1.0, 0.5, 0.25], dtype=np.float32)
    ids, fac, n = ref.bias_arrays([{5: np.log(2.0)}, None], 2)
    sou, sub = np.array([SOU, SOU]), np.array([SUB, SUB])
    dist = np.stack([row_of()] * 4)
    gen = np.array([[START, A, 0]] * 4, dtype=np.int32)
    length = np.array([2, 1, 2, 2])
    halve = lambda d, g, l: d * np.float32(0.5)
    out = ref.make_edit(sou, sub, DIMS, 2, table, ids, fac, n, before=halve)(dist, gen, length)
    assert out[0, A] == dist[0, A] * np.float32(0.25) and out[1, A] == dist[1, A] * np.float32(0.5)
    assert out[0, 5] == np.float32(dist[0, 5] * np.float32(0.5)) * fac[0, 0] and out[2, 5] == dist[2, 5] * np.float32(0.5)
    plain = ref.make_edit(sou, sub, DIMS, 2, table, ids, fac, n)(dist, gen, length)
    assert plain[3, A] == dist[3, A] * np.float32(0.5) and plain[3, 6] == dist[3, 6]


# ------------------------------------------------------------------------------------------------ the searches that refuse
def no_launch():
    """A Searcher whose every device path raises: a refusal must come before any of them."""
    from fira_icse_amd.decode import Searcher

    class NoLaunch(Searcher):
        def __init__(self, members=()):
            self.members = members
            self.cfg = FiraConfig()
            self._ws = {}

        def _begin(self, *a, **k):
            raise AssertionError("device work before the refusal")
        _state = _workspace = _begin
    return NoLaunch


def test_the_four_refusing_searches_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("a library call before the refusal")
    monkeypatch.setattr(_lib, "lib", no_library)
    s = no_launch()()
    db = types.SimpleNamespace(B=4)
    cand = np.full((4, 1, 3), START)
    for p in (Penalties(presence=0.5), Penalties(bias={A: 1.0}), "presence"):
        for name, run in (("sample", lambda: s.sample(db, 2, penalties=p)), ("score", lambda: s.score(db, cand, penalties=p)),
                          ("sample_distinct", lambda: s.sample_distinct(db, 2, penalties=p)),
                          ("contrastive", lambda: s.contrastive(db, 2, penalties=p))):
            with pytest.raises(ValueError, match="^%s does not take penalties" % name):
                run()
    assert s._ws == {}
    # the searches that take the option refuse a wrong value before any device work too, and an accepted one reaches it
    for run in (lambda p: s.greedy(db, penalties=p), lambda p: s.beam(db, 3, penalties=p),
                lambda p: s.sample_search(db, 2, penalties=p), lambda p: s.greedy_many([db, db], penalties=p)):
        with pytest.raises(ValueError, match="expected decode.Penalties"):
            run({"presence": 0.5})
        with pytest.raises(ValueError, match="commit 0: the bias 3.1 of id 10"):
            run(Penalties(bias={A: 3.1}))
        with pytest.raises(ValueError, match="2 bias mappings for a batch of 4"):
            run(Penalties(bias=[{A: 1.0}, {}]))
    assert s._ws == {}
    with pytest.raises(AssertionError, match="device work"):
        s.greedy(db, penalties=Penalties(presence=0.5))


# ------------------------------------------------------------------------------------------------ scripts/penalty_probe.py
def probe():
    import importlib.util
    spec = importlib.util.spec_from_file_location("penalty_probe", os.path.join(util.REPO, "scripts", "penalty_probe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_probe_options_parse_and_missing_words_are_dropped_and_counted(capsys):
    pp = probe()
    a = pp.parse_args(["--root", "x"])
    assert (a.beam, a.sample, a.presence_penalty, a.frequency_penalty, a.word_bias) == (3, None, 0.0, 0.0, None)
    assert not pp.penalties_from_args(a, {})[0].active
    a = pp.parse_args(["--root", "x", "--sample", "4", "--presence-penalty", "0.5", "--frequency-penalty", "0.25",
                       "--word-bias", "fix=1.5,<eos>=-2,nosuchword=1,a=b=0.5,other=3"])
    assert a.beam is None and a.sample == 4
    vocab = {"<pad>": PAD, "<eos>": EOS, "<start>": START, "<unkm>": UNK, "fix": 4, "a=b": 9}
    p, dropped = pp.penalties_from_args(a, vocab, FiraConfig(), 3)
    assert dropped == 2 and p == Penalties(0.5, 0.25, {4: 1.5, EOS: -2.0, 9: 0.5})
    assert pp.parse_bias(" fix=1 , ,the=-0.5") == [("fix", 1.0), ("the", -0.5)] and pp.parse_bias(None) == []
    for argv, word in ((["--word-bias", "fix"], "WORD=b"), (["--word-bias", "fix=much"], "not a number"),
                       (["--word-bias", "fix=31"], "outside"), (["--presence-penalty", "11"], "presence"),
                       (["--frequency-penalty", "-1"], "frequency"), (["--beam", "3", "--sample", "2"], "do not combine"),
                       (["--sample", "9"], "1..8"), (["--beam", "0"], "1..8"), (["--reps", "2"], "--reps")):
        with pytest.raises(SystemExit) as e:
            pp.parse_args(["--root", "x"] + argv)
        assert e.value.code == 2
        assert word in capsys.readouterr().err.strip().split("\n")[-1]
    with pytest.raises(ValueError, match="<pad> and <start>"):
        pp.penalties_from_args(pp.parse_args(["--root", "x", "--word-bias", "<start>=1"]), vocab)
    with pytest.raises(ValueError, match="87"):
        pp.penalties_from_args(pp.parse_args(["--root", "x", "--word-bias", "fix=3.5"]), vocab, FiraConfig(), 1)
