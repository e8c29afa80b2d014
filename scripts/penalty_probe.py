"""Soft word penalties and biases as a driver and as an instrument: decode the test split of a run directory with a search under
``decode.Penalties``, write the messages, and time a step with and without the options.

    python scripts/penalty_probe.py --root DIR [--beam K | --sample N [--temperature T] [--top-k K] [--top-p P] [--sample-seed S]]
        [--presence-penalty X] [--frequency-penalty Y] [--word-bias WORD=b[,WORD=b...]] [--merge-copies]
        [--test-batch-size B] [--splits a,b,c] [--reps 20] [--out profiles/penalty_probe.md]

``--root DIR`` is a run directory of run_model.py (DataSet/, all_index, best_model.pt).  ``--beam 1`` is greedy search, ``--beam K``
(default 3) the beam search, ``--sample N`` draws N candidates per commit with ``Searcher.sample_search`` and keeps the one of
highest score.  ``--word-bias``: vocabulary words (``<eos>`` among them) with the bias added to their log-probability at every
step; a word the vocabulary lacks is dropped, and the drops are counted in one warning.  Values outside what ``decode.Penalties``
takes are refused with its reason before anything is loaded.  Written, in all_index['test'] order:

    DIR/OUTPUT/output_fira_penalty            one message per commit
    DIR/OUTPUT/output_fira_penalty_samples    with --sample: one JSON line per commit in the format of output_fira_samples,
                                              {"candidates": [...], "logp": [...]} -- under penalties the values are scores

Timing, on the first batch of the split: the search without the options and the same search with them, interleaved call by call;
two warm-up rounds (which capture the graphs) are thrown away, every call is timed by a host clock between two device
synchronisations, and the median with min and max over ``--reps`` repetitions is reported per call and per step run (a call stops
at the first chunk boundary after every hypothesis has ended).  The two searches may run different numbers of steps -- the
penalties change the messages -- so the per-step column is the one to compare.  ``--reps 0`` writes the files and times nothing.
Without a GPU the script fails; it never falls back."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)


def parse_bias(text):
    """'WORD=b,WORD=b' -> [(word, b)]; raises ValueError naming the item."""
    pairs = []
    for item in (text or "").split(","):
        if not item.strip():
            continue
        word, sep, value = item.strip().rpartition("=")
        if not sep or not word:
            raise ValueError("--word-bias: %r is not WORD=b" % item)
        try:
            pairs.append((word, float(value)))
        except ValueError:
            raise ValueError("--word-bias: the bias %r of %s is not a number" % (value, word)) from None
    return pairs


def penalties_from_args(a, vocab, cfg=None, B=1):
    """(the ``Penalties`` value of the command line, the number of --word-bias words the vocabulary lacks).  A word given twice
    keeps its last bias.  Raises ValueError with ``Penalties``' own reason."""
    from fira_icse_amd.decode import Penalties
    bias, dropped = {}, 0
    for word, b in parse_bias(a.word_bias):
        if word in vocab:
            bias[int(vocab[word])] = b
        else:
            dropped += 1
    p = Penalties(presence=a.presence_penalty, frequency=a.frequency_penalty, bias=bias or None)
    return (p.check(cfg, B) if cfg is not None else p), dropped


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True, help="a run directory of run_model.py (DataSet/, all_index, best_model.pt)")
    ap.add_argument("--beam", type=int, default=None, help="beam size (default 3; 1 = greedy)")
    ap.add_argument("--sample", type=int, default=None, help="candidates per commit, 1..8, instead of a beam")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--sample-seed", type=int, default=0)
    ap.add_argument("--presence-penalty", type=float, default=0.0)
    ap.add_argument("--frequency-penalty", type=float, default=0.0)
    ap.add_argument("--word-bias", default=None, help="WORD=b[,WORD=b...]")
    ap.add_argument("--merge-copies", action="store_true", help="search words, not entries")
    ap.add_argument("--test-batch-size", type=int, default=20)
    ap.add_argument("--splits", default=None, help="as run_model.py --splits")
    ap.add_argument("--reps", type=int, default=20, help="timed repetitions after 2 warm-ups (0: no timing)")
    ap.add_argument("--out", default=None, help="append the timing as markdown to this file")
    a = ap.parse_args(argv)
    try:
        if a.beam is not None and a.sample is not None:
            raise ValueError("--beam and --sample do not combine")
        if a.sample is not None and not 1 <= a.sample <= 8:
            raise ValueError("--sample %d: outside 1..8" % a.sample)
        a.beam = 3 if a.beam is None and a.sample is None else a.beam
        if a.beam is not None and not 1 <= a.beam <= 8:
            raise ValueError("--beam %d: outside 1..8" % a.beam)
        if a.test_batch_size < 1:
            raise ValueError("--test-batch-size %d: at least 1" % a.test_batch_size)
        if a.reps < 0 or 0 < a.reps < 3:
            raise ValueError("--reps %d: 0 (no timing) or at least 3" % a.reps)
        # the values themselves, ahead of any file (every word stands for some id: only the numbers are looked at)
        penalties_from_args(a, {word: 3 + k for k, (word, _) in enumerate(parse_bias(a.word_bias)[:16])})
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    import run_model
    from fira_icse_amd import text
    from fira_icse_amd.decode import Searcher
    from fira_icse_amd.model import TransModel
    assert torch.cuda.is_available(), "penalty_probe.py needs a GPU"
    run = run_model.Run(run_model.parse_args(["test", "--root", a.root, "--test-batch-size", str(a.test_batch_size)]
                                             + (["--splits", a.splits] if a.splits else [])))
    cfg, store, test_index = run.cfg, run.sets["test"].store, run.all_index["test"]
    penalties, dropped = penalties_from_args(a, run.vocab, cfg)
    if dropped:
        print("warning: %d biased words are not in the vocabulary and are dropped" % dropped, file=sys.stderr, flush=True)
    run.model = model = TransModel(cfg, device="cuda:%d" % run.local, init=False)
    model.load_state_dict(torch.load(os.path.join(a.root, "best_model.pt"), map_location="cpu"))
    model.eval()
    search = Searcher(model)
    chunk = 5 if a.beam in (None, 1) else 4

    def decode(db, idx, pen):
        """(tokens, lengths, value) per hypothesis of the batch under ``pen``."""
        if a.sample is not None:
            toks, lens, _, logp = search.sample_search(db, a.sample, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p,
                                                       seed=a.sample_seed, keys=idx, merge_copies=a.merge_copies, penalties=pen)
            return toks, lens, logp
        if a.beam == 1:
            return search.greedy(db, merge_copies=a.merge_copies, penalties=pen)
        return search.beam(db, a.beam, merge_copies=a.merge_copies, penalties=pen)

    batches = [list(range(lo, min(lo + a.test_batch_size, len(store)))) for lo in range(0, len(store), a.test_batch_size)]
    lines, samples, first = [], [], None
    for idx in batches:
        db = run.device_batch(store, idx)
        first = (db, idx) if first is None else first
        toks, lens, value = decode(db, idx, penalties)
        best = search.best(toks, lens, value)
        for k, i in enumerate(idx):
            var_map = run.var_maps[test_index[i]]
            lines.append(text.detokenize(best[k], run.r_vocab, var_map))
            if a.sample is not None:
                cands = [text.detokenize(toks[k, j, :int(lens[k, j])].tolist(), run.r_vocab, var_map) for j in range(a.sample)]
                samples.append(json.dumps({"candidates": cands, "logp": value[k].tolist()}))
    written = [("output_fira_penalty", lines)] + ([("output_fira_penalty_samples", samples)] if a.sample is not None else [])
    for name, rows in written:
        with open(run.out(name), "w") as f:
            f.write("".join(l + "\n" for l in rows))
    print("wrote %d messages to %s" % (len(lines), ", ".join(run.out(name) for name, _ in written)), flush=True)
    if a.reps == 0:
        return
    db, idx = first
    what = "sample_search n = %d" % a.sample if a.sample is not None else "greedy" if a.beam == 1 else "beam %d" % a.beam
    configs = [(what + ", no penalties", None)] + ([(what + ", penalties", penalties)] if penalties.active else [])
    T = cfg.tar_len
    ms, steps = {name: [] for name, _ in configs}, {}
    for rep in range(a.reps + 2):
        for name, pen in configs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = decode(db, idx, pen)
            torch.cuda.synchronize()
            if rep >= 2:
                ms[name].append(1e3 * (time.perf_counter() - t0))
            ended = int(out[1].max()) - 1                                # the step count after which every hypothesis had ended
            steps[name] = min(T - 1, -(-ended // chunk) * chunk)
    rows = ["| search | median ms / call | min | max | steps run | median ms / step | / without |", "|---|---|---|---|---|---|---|"]
    base = statistics.median(ms[configs[0][0]]) / steps[configs[0][0]]
    for name, _ in configs:
        med = statistics.median(ms[name])
        rows.append("| %s | %.3f | %.3f | %.3f | %d | %.4f | %.3f |" % (name, med, min(ms[name]), max(ms[name]), steps[name],
                                                                      med / steps[name], med / steps[name] / base))
    given = " ".join(argv if argv is not None else sys.argv[1:])
    out = "\n".join(["### %s: B = %d, %d interleaved repetitions after 2 warm-ups, graphs of %d steps" % (
        torch.cuda.get_device_name(0), db.B, a.reps, chunk), "", "`%s`" % given, ""] + rows + [""])
    print(out, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
