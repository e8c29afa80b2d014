"""Dev-set model selection, the parts that need no GPU: the score from integer statistics is bit for bit the string scorer's,
the string oracle of the BLEU kernel agrees with that scorer, the vocabulary check, and the host pass with injected ids."""
import random

import pytest

import util
import dev_bleu_ref as R
from fira_icse_amd import devset, metrics, synth, text
from fira_icse_amd.config import EOS, PAD, START, UNK

WORDS = ["a", "b", "c", "d", "e", "f"]


def string_stats(hyp, ref):
    from collections import Counter
    num, cnt = [], []
    for n in range(1, 5):
        hc = Counter(tuple(hyp[i:i + n]) for i in range(len(hyp) - n + 1))
        rc = Counter(tuple(ref[i:i + n]) for i in range(len(ref) - n + 1))
        num.append(sum(min(c, rc[g]) for g, c in hc.items()))
        cnt.append(sum(hc.values()))
    return num, cnt, len(hyp), len(ref)


def pairs():
    rnd = random.Random(20240)
    out = []
    for _ in range(2400):
        hyp = [rnd.choice(WORDS) for _ in range(rnd.randint(0, 30))]
        if rnd.random() < 0.5:                                          # a reference near the hypothesis: long matches
            ref = [w if rnd.random() < 0.8 else rnd.choice(WORDS) for w in hyp][:rnd.randint(0, 30)]
        else:
            ref = [rnd.choice(WORDS) for _ in range(rnd.randint(0, 30))]
        out.append((hyp, ref))
    out += [([], ["a", "b"]), ([], []), (["a", "b"], ["c", "d", "e"]), (["a"], ["a"]), (["a"], ["a", "b", "c"]),
            (["a", "b"], ["a", "b"]), (["a", "b", "c"], ["a", "b", "c"]), (["a", "b", "c"], ["c", "b", "a"]),
            (["a", "b"], []), (["a"] * 30, ["a", "b", "a"]), (["a", "b", "c", "d", "e"], ["a", "b"]),
            (["a", "b"], ["a", "b", "c", "d", "e", "f"]), (["a", "b", "c", "d"], ["a", "b", "c", "d"])]
    return out


def test_score_from_stats_is_bit_for_bit_the_old_string_scorer():
    n_zero = n_pos = 0
    for hyp, ref in pairs():
        want = R.old_sentence_bleu_method2([ref], hyp)
        assert metrics.bleu_method2_from_stats(*string_stats(hyp, ref)) == want, (hyp, ref)
        assert metrics.sentence_bleu_method2([ref], hyp) == want, (hyp, ref)
        n_zero += want == 0.0
        n_pos += want > 0.0
    assert n_zero > 20 and n_pos > 1000
    # several references (not used by dev(), still the old values)
    refs = [["a", "b", "c", "d"], ["a", "b"], ["c", "d", "e", "f", "a", "b"]]
    for hyp in (["a", "b", "c"], ["a", "b", "c", "d", "e"], ["f"], []):
        assert metrics.sentence_bleu_method2(refs, hyp) == R.old_sentence_bleu_method2(refs, hyp)


def test_stats_oracle_agrees_with_the_string_scorer():
    B, T, V, L, S = 37, 30, 12, 7, 5
    ids, sou, sub, tar = R.kernel_cases(B, T, V, L, S, seed=0)
    assert all(R.coverage(ids, sou, sub, tar, V, L, S).values())
    for b in range(B):
        st, hyp_ids = R.stats_ref(ids[b], sou[b], sub[b], tar[b], V, L, S)
        hyp, ref = R.strings_ref(ids[b], sou[b], sub[b], tar[b], V, L, S)
        assert metrics.bleu_method2_from_stats(st[0:4], st[4:8], st[8], st[9]) == R.old_sentence_bleu_method2([ref], hyp)
        assert len(hyp_ids) == T and st[8] == len(hyp) and st[10:] == [0, 0]
        assert PAD not in hyp_ids[:st[8]] and all(t == -1 for t in hyp_ids[st[8]:])
    # <unkm> never matches: same ids on both sides, no unigram in common
    st, hyp_ids = R.stats_ref([UNK, UNK, EOS] + [PAD] * 27, sou[0], sub[0], [START, UNK, UNK, EOS] + [PAD] * 26, V, L, S)
    assert st[0:4] == [0, 0, 0, 0] and st[4:10] == [2, 1, 0, 0, 2, 2] and hyp_ids[:2] == [UNK, UNK]


def test_vocabulary_check():
    good = {i: w for w, i in synth.make_vocab(200).items()}
    devset.check_vocabulary(good, 200)
    devset.check_vocabulary(R.toy_r_vocab(12), 12)
    for bad_word in ("", "two words", "tab\tbed", " lead", text.UNK_EMOJI, "x<pad>", "<pad><pad>", "a<unkm>b", "<unkm>s"):
        bad = dict(good)
        bad[77] = bad_word
        with pytest.raises(ValueError):
            devset.check_vocabulary(bad, 200)
    for tok_id in (PAD, UNK):                                            # the two tokens must be themselves
        bad = dict(good)
        bad[tok_id] = "other"
        with pytest.raises(ValueError):
            devset.check_vocabulary(bad, 200)
    hole = dict(good)
    del hole[50]
    with pytest.raises(ValueError):
        devset.check_vocabulary(hole, 200)


def test_host_pass_with_injected_ids_runs_without_a_gpu():
    cfg, store, r_vocab, var_maps, valid_index = R.synthetic_valid()
    table = R.label_ids_table(store, cfg, seed=0)
    assert (table >= cfg.vocab_size).any()                               # copy labels are in
    ev = devset.DevEvaluator(None, store, cfg, r_vocab, var_maps, valid_index, ids_fn=R.table_ids_fn(table), device="cpu")
    total, lines = ev.host_pass()
    scores = ev.last_scores
    print("mean BLEU %.4f, non-zero %d of %d" % (total / len(store), sum(s > 0 for s in scores), len(scores)))
    assert len(scores) == len(store) == 23
    assert total / len(store) > 0 and sum(s > 0 for s in scores) >= (len(scores) + 1) // 2
    out = lines()
    assert len(out) == 23 and all(l.rsplit(",", 1)[1] == str(s) for l, s in zip(out, scores))
    # the oracle of the kernel gives the same per-commit scores on these rows
    V, L, S = cfg.vocab_size, cfg.sou_len, cfg.sub_token_len
    for i in range(len(store)):
        st, _ = R.stats_ref(table[i], store.sou[i], store.sub_token[i], store.tar[i], V, L, S, r_vocab)
        assert metrics.bleu_method2_from_stats(st[0:4], st[4:8], st[8], st[9]) == scores[i]
    # sharding: the two halves of a 2-rank run are the one-rank run
    halves = [devset.DevEvaluator(None, store, cfg, r_vocab, var_maps, valid_index, rank=r, world=2,
                                  ids_fn=R.table_ids_fn(table), device="cpu") for r in (0, 1)]
    parts = [h.host_pass()[0] for h in halves]
    assert halves[0].last_scores + halves[1].last_scores == scores and halves[0].bs == 4
    assert abs(sum(parts) - total) <= 1e-12 * max(1.0, total)


def test_device_pass_refuses_a_bad_valid_set_before_any_device_work():
    cfg, store, r_vocab, var_maps, valid_index = R.synthetic_valid(n=6)
    table = R.label_ids_table(store, cfg, seed=0)
    bad_vocab = dict(r_vocab)
    bad_vocab[100] = "has blank"
    ev = devset.DevEvaluator(None, store, cfg, bad_vocab, var_maps, valid_index, ids_fn=R.table_ids_fn(table), device="cpu")
    with pytest.raises(ValueError, match="white space"):
        ev.device_pass()
    store.tar = store.tar.copy()
    store.tar[4][store.tar[4] == EOS] = 7                                # a target without <eos>: the host pass raises too
    ev = devset.DevEvaluator(None, store, cfg, r_vocab, var_maps, valid_index, ids_fn=R.table_ids_fn(table), device="cpu")
    with pytest.raises(ValueError, match="no <eos>"):
        ev.device_pass()
    with pytest.raises(ValueError):
        ev.host_pass()
