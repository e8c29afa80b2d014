"""Sampling from the search's edited distribution as a driver and as an instrument: decode the test split of a run directory
with ``Searcher.sample_search`` under the searches' options, write the messages and the candidates, and time a step against the
fused sampler.

    python scripts/sample_search_probe.py --root DIR --sample N [--temperature T] [--top-k K] [--top-p P] [--min-p X]
        [--epsilon-cutoff E] [--eta-cutoff E] [--typical-p P] [--sample-seed S] [--ban-words W,...] [--no-repeat-ngram N]
        [--min-length M] [--merge-copies] [--prefix WORDS | --prefix-file PATH] [--ensemble PATH,... [--ensemble-weights W,...]]
        [--rerank mbr_bleu] [--test-batch-size B] [--splits a,b,c] [--reps 20] [--out profiles/sample_search_probe.md]

``--root DIR`` is a run directory of run_model.py (DataSet/, all_index, best_model.pt).  The options are run_model.py's own, with
its own parsing and checks (check_sample_args, check_cut_args, check_constraint_args, check_prefix_args, check_ensemble_args,
constraints_from_args, prefixes_from_args): what run_model.py refuses for a value, this script refuses; only the refusal of the
search options next to --sample is lifted, which is the point.  Written, in all_index['test'] order:

    DIR/OUTPUT/output_fira_sample_search            one message per commit: the candidate of highest log-probability, or with
                                                    --rerank mbr_bleu the one of highest expected BLEU among the candidates
    DIR/OUTPUT/output_fira_sample_search_samples    one JSON line per commit in the format of output_fira_samples:
                                                    {"candidates": [...], "logp": [...]} and the N utilities under "mbr_bleu"

The noise of a commit is keyed by its index in the test split, as ``run_model.py test --sample`` keys it.

Timing, on the first batch of the split: ``sample`` (the fused sampler; one model, no option), ``sample_search`` without options
(same draws, bit for bit: the cost of the distribution hand-off alone) and ``sample_search`` with the options given.  The three
are interleaved call by call, two warm-up rounds (which capture the graphs) are thrown away, every call is timed by a host clock
between two device synchronisations, and the median with min and max over ``--reps`` repetitions is reported per call and per
step run (a call stops at the first chunk boundary after every sample has ended: steps = the chunks replayed times 5).
``--reps 0`` writes the files and times nothing.  Without a GPU the script fails; it never falls back."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

CHUNK = 5


def parse_args(argv=None):
    """The probe's namespace, checked with run_model.py's own checks; exits with code 2 and the reason on a refusal."""
    import run_model
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True, help="a run directory of run_model.py (DataSet/, all_index, best_model.pt)")
    ap.add_argument("--sample", type=int, required=True, help="candidates per commit, 1..8")
    ap.add_argument("--temperature", type=float, default=None)
    ap.add_argument("--top-k", type=int, default=None)
    ap.add_argument("--top-p", type=float, default=None)
    ap.add_argument("--min-p", type=float, default=None)
    ap.add_argument("--epsilon-cutoff", type=float, default=None)
    ap.add_argument("--eta-cutoff", type=float, default=None)
    ap.add_argument("--typical-p", type=float, default=None)
    ap.add_argument("--sample-seed", type=int, default=None)
    ap.add_argument("--ban-words", default=None, help="comma-separated vocabulary words no candidate may hold")
    ap.add_argument("--no-repeat-ngram", type=int, default=None)
    ap.add_argument("--min-length", type=int, default=None)
    ap.add_argument("--merge-copies", action="store_true", help="sample words, not entries")
    ap.add_argument("--prefix", default=None, help="how every candidate begins")
    ap.add_argument("--prefix-file", default=None, help="one prefix per test commit, one per line")
    ap.add_argument("--ensemble", default=None, help="further checkpoints, comma-separated")
    ap.add_argument("--ensemble-weights", default=None, help="one weight per model, best_model.pt first")
    ap.add_argument("--rerank", default=None, choices=["mbr_bleu"])
    ap.add_argument("--test-batch-size", type=int, default=20)
    ap.add_argument("--splits", default=None, help="as run_model.py --splits")
    ap.add_argument("--reps", type=int, default=20, help="timed repetitions after 2 warm-ups (0: no timing)")
    ap.add_argument("--out", default=None, help="append the timing as markdown to this file")
    a = ap.parse_args(argv)
    a.stage, a.beam, a.score, a.without_replacement = "test", None, None, False
    searching = argparse.Namespace(**dict(vars(a), sample=None))       # the search options as run_model.py checks them for a search
    try:
        run_model.check_sample_args(a)
        run_model.check_cut_args(a)
        run_model.check_constraint_args(searching)
        run_model.check_prefix_args(searching)
        run_model.check_ensemble_args(searching)
        if a.test_batch_size < 1:
            raise ValueError("--test-batch-size %d: at least 1" % a.test_batch_size)
        if a.reps < 0 or 0 < a.reps < 3:
            raise ValueError("--reps %d: 0 (no timing) or at least 3" % a.reps)
    except ValueError as e:
        ap.error(str(e))
    a.ensemble, a.ensemble_weights = searching.ensemble, searching.ensemble_weights
    return a


def options_given(a) -> bool:
    return bool(a.ban_words or a.no_repeat_ngram or a.min_length or a.merge_copies or a.prefix is not None
                or a.prefix_file is not None or a.ensemble)


def main(argv=None):
    a = parse_args(argv)
    import torch
    import run_model
    from fira_icse_amd import text
    from fira_icse_amd.decode import Searcher
    from fira_icse_amd.model import TransModel
    assert torch.cuda.is_available(), "sample_search_probe.py needs a GPU"
    run = run_model.Run(run_model.parse_args(["test", "--root", a.root, "--test-batch-size", str(a.test_batch_size)]
                                             + (["--splits", a.splits] if a.splits else [])))
    cfg, store, test_index = run.cfg, run.sets["test"].store, run.all_index["test"]
    run_model.check_sample_args(a, cfg.out_len)                        # top-k against this vocabulary
    constraints = run_model.constraints_from_args(a, run.vocab, cfg)
    prefixes, n_unk = run_model.prefixes_from_args(a, run.vocab, [run.var_maps[i] for i in test_index], cfg.tar_len)
    if n_unk:
        print("warning: %d prefix words are not in the vocabulary and are forced as <unkm>" % n_unk, file=sys.stderr, flush=True)

    def load(path):
        m = TransModel(cfg, device="cuda:%d" % run.local, init=False)
        m.load_state_dict(torch.load(path, map_location="cpu"))
        m.eval()
        return m
    run.model = model = load(os.path.join(a.root, "best_model.pt"))
    plain = Searcher(model)
    search = Searcher(model, members=[load(p) for p in a.ensemble], weights=a.ensemble_weights) if a.ensemble else plain
    filters = dict(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    filters.update({kw: getattr(a, name) for (name, _), kw in zip(run_model.CUT_OPTIONS, ("min_p", "epsilon", "eta", "typical_p"))
                    if getattr(a, name) is not None})
    batches = [list(range(lo, min(lo + a.test_batch_size, len(store)))) for lo in range(0, len(store), a.test_batch_size)]

    def options(idx):
        return dict(constraints=constraints, merge_copies=a.merge_copies,
                    prefix=None if prefixes is None else [prefixes[i] for i in idx])

    lines, samples, first = [], [], None
    for idx in batches:
        db = run.device_batch(store, idx)
        first = (db, idx) if first is None else first
        toks, lens, _, logp = search.sample_search(db, a.sample, seed=a.sample_seed, keys=idx, chunk=CHUNK, **filters, **options(idx))
        best, values = search.best_sample(toks, lens, logp), None
        if a.rerank == "mbr_bleu":
            pick, util = search.mbr(toks, lens, logp)
            best = [toks[k, j, :int(lens[k, j])].tolist() for k, j in enumerate(pick)]
            values = util.tolist()
        toks, lens, logp = toks.tolist(), lens.tolist(), logp.tolist()
        for k, i in enumerate(idx):
            var_map = run.var_maps[test_index[i]]
            lines.append(text.detokenize(best[k], run.r_vocab, var_map))
            rec = {"candidates": [text.detokenize(toks[k][j][:lens[k][j]], run.r_vocab, var_map) for j in range(a.sample)],
                   "logp": logp[k]}
            if values is not None:
                rec[a.rerank] = values[k]
            samples.append(json.dumps(rec))
    for name, rows in (("output_fira_sample_search", lines), ("output_fira_sample_search_samples", samples)):
        with open(run.out(name), "w") as f:
            f.write("".join(l + "\n" for l in rows))
    print("wrote %d messages to %s and their candidates to %s" % (len(lines), run.out("output_fira_sample_search"),
                                                                 run.out("output_fira_sample_search_samples")), flush=True)
    if a.reps == 0:
        return
    db, idx = first
    kw = dict(seed=a.sample_seed, keys=idx, chunk=CHUNK, **filters)
    configs = [("sample (fused)", lambda: plain.sample(db, a.sample, **kw)),
               ("sample_search, no option", lambda: plain.sample_search(db, a.sample, **kw))]
    if options_given(a):
        configs.append(("sample_search, options", lambda: search.sample_search(db, a.sample, **kw, **options(idx))))
    T = cfg.tar_len
    ms, steps = {name: [] for name, _ in configs}, {}
    for rep in range(a.reps + 2):
        for name, fn in configs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if rep >= 2:
                ms[name].append(1e3 * (time.perf_counter() - t0))
            ended = int(out[1].max()) - 1                                # the step count after which every sample had ended
            steps[name] = min(T - 1, -(-ended // CHUNK) * CHUNK)
    rows = ["| search | median ms / call | min | max | steps run | median ms / step | / fused |", "|---|---|---|---|---|---|---|"]
    base = statistics.median(ms[configs[0][0]]) / steps[configs[0][0]]
    for name, _ in configs:
        med = statistics.median(ms[name])
        rows.append("| %s | %.3f | %.3f | %.3f | %d | %.4f | %.2f |" % (name, med, min(ms[name]), max(ms[name]), steps[name],
                                                                      med / steps[name], med / steps[name] / base))
    given = " ".join(argv if argv is not None else sys.argv[1:])
    out = "\n".join(["### %s: B = %d, n = %d, %d interleaved repetitions after 2 warm-ups, graphs of %d steps" % (
        torch.cuda.get_device_name(0), db.B, a.sample, a.reps, CHUNK), "", "`%s`" % given, ""] + rows + [""])
    print(out, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
