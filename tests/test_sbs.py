"""Stochastic beam search on the CPU: the numpy twin (sbs_ref.py) samples without replacement from the exact law, its stable
key equals the naive one, void inputs stay void, the kernel test's inputs are mostly above the comparison margin, and the
command line refuses what does not combine with --without-replacement."""
import itertools

import numpy as np
import pytest

import util  # noqa: F401
import sample_ref
import sbs_ref
from run_model import parse_args


def test_ordered_triples_follow_the_without_replacement_law():
    """A 6-entry one-step model, n = 3, 20 000 seeds: the ordered triple (a, b, c) of the three slots has the probability
    p_a * p_b / (1 - p_a) * p_c / (1 - p_a - p_b).  Chi-square over the 120 triples against the exact law at the 5-sigma level
    test_sample_gpu.py uses for its counts (one-sided p = 2.9e-7): the critical value by Wilson-Hilferty,
    df * (1 - 2 / (9 df) + 5 * sqrt(2 / (9 df)))^3 = 211.6 at df = 119 (the exact quantile is 212.2)."""
    p = np.array([0.35, 0.25, 0.15, 0.12, 0.08, 0.05])
    n, W, N = 3, 6, 20000
    gen = np.zeros((n, 2), dtype=np.int64)
    gen[:, 0] = sbs_ref.START
    st = sbs_ref.initial_state(n, 2)
    dist = np.tile(p.astype(np.float32), (n, 1))
    none = np.zeros(0, dtype=np.int64)
    triples = list(itertools.permutations(range(W), 3))
    where = {t: k for k, t in enumerate(triples)}
    counts = np.zeros(len(triples))
    for seed in range(N):
        out = sbs_ref.select_step(dist, st["gen"], st["length"], st["phi"], st["G"], st["logp"], none, none, W, 5, seed, 0, 1.0)
        assert all(c is not None and c[0] == 0 for c in out["cand"])
        assert out["G"][0] <= 0 and (np.diff(out["G"]) <= 0).all()
        counts[where[tuple(c[1] for c in out["cand"])]] += 1
    pf = dist[0].astype(np.float64) / dist[0].astype(np.float64).sum()
    law = np.array([pf[a] * pf[b] / (1 - pf[a]) * pf[c] / (1 - pf[a] - pf[b]) for a, b, c in triples])
    assert abs(law.sum() - 1) < 1e-12 and (N * law).min() >= 5
    chi2 = float((((counts - N * law) ** 2) / (N * law)).sum())
    df = len(triples) - 1
    crit = df * (1 - 2 / (9 * df) + 5 * np.sqrt(2 / (9 * df))) ** 3
    print("chi2 = %.1f, df = %d, critical value = %.1f" % (chi2, df, crit))
    assert chi2 < crit


def test_n_one_is_ancestral_gumbel_max_sampling():
    """With one slot the search takes, step by step, the sampler's Gumbel-max draw of (key, seed, slot 0, step)."""
    rng = np.random.default_rng(3)
    V, T = 12, 7
    table = rng.random((V, V)) ** 3
    table[:, sbs_ref.EOS] *= 2.0
    table[rng.random((V, V)) < 0.2] = 0.0
    table[:, 5] += 0.01
    table = (table / table.sum(1, keepdims=True)).astype(np.float32)
    none = np.zeros(0, dtype=np.int64)
    for seed in range(40):
        for temp in (1.0, 1.5):
            st, _ = sbs_ref.search(lambda step, gen, length: table[gen[:, step]], 1, T, none, none, V, 9, seed, temp)
            ids, logp = [sbs_ref.START], 0.0
            for step in range(T - 1):
                row = table[ids[-1]].astype(np.float64)
                g = sample_ref.gumbel(sample_ref.row_stream(9, seed, 0, T, step), V)
                inv = np.float64(np.float32(1) / np.float32(temp))
                with np.errstate(divide="ignore"):
                    i = int(np.argmax(np.where(row > 0, np.log(row) * inv + g, -np.inf)))
                ids.append(i)
                logp += np.log(row[i])
                if i == sbs_ref.EOS:
                    break
            assert st["gen"][0, :st["length"][0]].tolist() == ids
            assert abs(st["logp"][0] - logp) < 1e-12 and st["G"][0] == 0.0


def test_stable_key_equals_the_naive_form_where_that_is_finite():
    rng = np.random.default_rng(0)
    checked = 0
    for _ in range(2000):
        G, Z = rng.normal(0, 6, 2)
        g = Z - rng.exponential(3.0, 8)
        naive = sbs_ref.naive_key(G, Z, g)
        stable = sbs_ref.stable_key(G, Z, g)
        ok = np.isfinite(naive)
        # the naive form cancels: exp(-G) - exp(-Z) + exp(-g) loses up to max(exp(-G), exp(-Z)) / sum of its 2^-53
        scale = np.maximum(np.exp(-G), np.exp(-Z)) / (np.exp(-G) - np.exp(-Z) + np.exp(-g))
        assert (np.abs(naive - stable)[ok] <= 1e-15 * scale[ok] * 8 + 1e-12).all()
        assert (stable <= G).all()
        checked += int(ok.sum())
    assert checked > 10000
    # far from the range of exp: the naive form overflows, the stable one does not
    assert np.isfinite(sbs_ref.stable_key(-800.0, -790.0, np.array([-795.0, -900.0]))).all()
    assert sbs_ref.stable_key(3.0, 5.0, np.array([5.0]))[0] == 3.0           # the row's maximum takes the parent's key


def test_void_and_infinite_inputs_give_no_nan():
    ninf = -np.inf
    for G, Z, g in ((ninf, 1.0, [0.5, ninf]), (2.0, 1.0, [ninf, 1.0, 0.0]), (ninf, ninf, [ninf]), (0.0, ninf, [ninf])):
        k = sbs_ref.stable_key(G, Z, np.array(g))
        assert not np.isnan(k).any()
        assert all(v == ninf for v, x in zip(k, g) if x == ninf or G == ninf)
    # a step whose rows are all zero, NaN or void: every slot stays void, nothing is NaN
    n, W, T = 4, 7, 5
    st = sbs_ref.initial_state(n, T)
    dist = np.zeros((n, W), dtype=np.float32)
    dist[0, 2] = np.nan
    none = np.zeros(0, dtype=np.int64)
    out = sbs_ref.select_step(dist, st["gen"], st["length"], st["phi"], st["G"], st["logp"], none, none, W, 1, 2, 0, 1.0)
    assert (out["G"] == ninf).all() and (out["phi"] == ninf).all() and (out["length"] == 1).all() and out["cand"] == [None] * n
    dist[0, 3] = 1.0                                                         # one positive entry: one live slot
    out = sbs_ref.select_step(dist, st["gen"], st["length"], st["phi"], st["G"], st["logp"], none, none, W, 1, 2, 0, 0.7)
    assert out["cand"][0] == (0, 3) and out["G"][0] == 0.0 and abs(out["phi"][0]) < 1e-12 and (out["G"][1:] == ninf).all()
    for k in ("G", "phi", "logp"):
        assert not np.isnan(out[k]).any()


def test_kernel_cases_are_mostly_above_the_margin():
    """The cap of test_sbs_gpu.py's kernel-against-twin test: on its own inputs the twin's sub-margin share is under 5 %."""
    from fira_icse_amd.config import FiraConfig
    cfg = FiraConfig()
    model = dict(V=cfg.vocab_size, L=cfg.sou_len, S=cfg.sub_token_len, T=cfg.tar_len)
    total = below = 0
    exhausted = 0
    for name, d, n, temp, a in sbs_ref.kernel_cases(model):
        for b, r in enumerate(sbs_ref.twin_of_case(d, n, temp, a)):
            total += 1
            below += r["gap"] < sbs_ref.MARGIN
            for k in ("G", "phi", "logp"):
                assert not np.isnan(r[k]).any()
            if b == 2 and n == 8:                                            # exhaustion: 3 live slots, 5 void
                assert (r["G"][:3] > -np.inf).all() and (r["G"][3:] == -np.inf).all() and (r["length"][3:] == 1).all()
                exhausted += 1
    assert total == 3 * 13 and exhausted == 4
    assert below < 0.05 * total, (below, total)


REFUSED = [
    (["--without-replacement"], "--sample"),
    (["--sample", "4", "--without-replacement", "--top-k", "5"], "--top-k"),
    (["--sample", "4", "--without-replacement", "--top-p", "0.9"], "--top-p"),
    (["--sample", "4", "--without-replacement", "--beam", "3"], "--beam"),
    (["--sample", "4", "--without-replacement", "--score", "refs"], "--score"),
    (["--sample", "4", "--without-replacement", "--prefix", "fix"], "--prefix"),
    (["--sample", "4", "--without-replacement", "--prefix-file", "nowhere"], "--prefix-file"),
    (["--sample", "4", "--without-replacement", "--length-penalty", "1"], "--length-penalty"),
    (["--sample", "4", "--without-replacement", "--beam-groups", "2", "--diversity-penalty", "1"], "--beam-groups"),
]


@pytest.mark.parametrize("argv,named", REFUSED)
def test_cli_refusals_name_the_option(argv, named, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(["test"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--without-replacement" in err and named in err


def test_cli_accepts_what_combines():
    a = parse_args(["test", "--sample", "8", "--without-replacement", "--temperature", "0.7", "--sample-seed", "3",
                    "--no-repeat-ngram", "2", "--min-length", "3", "--ban-words", "fix", "--rerank", "mbr_bleu",
                    "--merge-copies"])
    assert a.without_replacement and a.sample == 8 and a.beam == 1 and a.temperature == 0.7 and a.top_k == 0 and a.top_p == 1.0
    assert not parse_args(["test", "--sample", "3"]).without_replacement
    # without the option --sample refuses the search options as before
    for argv in (["--sample", "3", "--no-repeat-ngram", "2"], ["--sample", "3", "--merge-copies"]):
        with pytest.raises(SystemExit):
            parse_args(["test"] + argv)
