"""``meteor_exact`` as a reported figure and as an MBR utility, on a run directory of run_model.py.

    python scripts/meteor_probe.py --root DIR [--synthetic N] [--splits a,b,c] [--test-batch-size 64]
        [--sample N [--temperature T] [--top-k K] [--top-p P] [--sample-seed S] [--pool 4] [--reps 7] [--out profiles/meteor_probe.md]]

``--root DIR`` is a run directory (DataSet/, all_index, best_model.pt).  ``--synthetic N`` first WRITES one there: N synth.py
commits and, as best_model.pt, the seeded initialisation with a sharpened generator (what scripts/rouge_probe.py samples from) --
an untrained model, so every figure below is about the machinery, not about message quality.

``meteor_exact`` is NLTK's METEOR alignment and score (alpha 0.9, beta 3, gamma 0.5) with exact word matches only: no stemmer, no
WordNet (``metrics.meteor_exact``).  It is NOT the reference's ``meteor_score`` and no figure printed here is comparable with the
paper's METEOR column; identity with NLTK has not been checked.

Always: if DIR/OUTPUT/output_fira exists, prints ``metrics.meteor_exact_corpus`` of it against the test split's reference
messages (the targets written as text by ``text.detokenize``, in all_index['test'] order).

With ``--sample N`` (1..8): draws N candidates per test commit (``Searcher.sample``, the noise keyed by the commit's index as
``run_model.py test --sample`` keys it), picks by expected BLEU, ROUGE-L and meteor_exact (``Searcher.mbr``), and writes

    DIR/OUTPUT/output_fira_mbr_meteor_exact            one message per commit: the candidate of highest expected meteor_exact
    DIR/OUTPUT/output_fira_mbr_meteor_exact_samples    one JSON line per commit in the format of output_fira_samples:
                                                       {"candidates": [...], "logp": [...], "mbr_bleu": [...], "mbr_rouge_l": [...],
                                                        "mbr_meteor_exact": [...]}

then reports in how many commits the three picks differ and the corpus figures of the three sets of picks.

Timing (``--reps`` >= 5, 0: none), on the first batch of the split, at n = N and at n = N x ``--pool`` candidates (further
draws with other seeds pooled along n, at most 32): per repetition, in this order, ``Searcher.mbr(..., utility="meteor_exact")``
as a whole, its three parts apart (the kernel as the mean of ``--launches`` back-to-back launches between two synchronisations,
the copy of the statistics, forming utilities and pick on the host) and the host loop (``text.detokenize`` -> ``split`` ->
``metrics.meteor_exact`` for all ordered pairs, ``math.fsum`` mean, ``metrics.mbr_pick``) -- same process, same candidates,
interleaved; two warm-up repetitions are thrown away; medians, min and max over the rest.  The comparison is device path against
host loop, never the kernel against itself.  Without a GPU the script fails; it never falls back."""
import argparse
import json
import math
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

UTILITIES = ("bleu", "rouge_l", "meteor_exact")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True, help="a run directory of run_model.py (DataSet/, all_index, best_model.pt)")
    ap.add_argument("--synthetic", type=int, default=None, help="write N synthetic commits and an untrained model to --root first")
    ap.add_argument("--splits", default=None, help="as run_model.py --splits")
    ap.add_argument("--test-batch-size", type=int, default=64)
    ap.add_argument("--sample", type=int, default=None, help="candidates per commit, 1..8")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0, help="0: off")
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--sample-seed", type=int, default=0)
    ap.add_argument("--pool", type=int, default=4, help="timing: also at N x POOL candidates (further draws pooled), at most 32")
    ap.add_argument("--reps", type=int, default=7, help="timed repetitions after 2 warm-ups (0: no timing)")
    ap.add_argument("--launches", type=int, default=50, help="kernel launches inside one timed window")
    ap.add_argument("--out", default=None, help="append the result as markdown to this file")
    a = ap.parse_args(argv)
    if a.sample is not None and not 1 <= a.sample <= 8:
        ap.error("--sample %d: 1..8 candidates per draw" % a.sample)
    if a.pool < 1 or (a.sample or 1) * a.pool > 32:
        ap.error("--pool %d: N x POOL must lie in 1..32" % a.pool)
    if a.reps < 0 or 0 < a.reps < 5:
        ap.error("--reps %d: 0 (no timing) or at least 5" % a.reps)
    if a.test_batch_size < 1:
        ap.error("--test-batch-size %d: at least 1" % a.test_batch_size)
    return a


def host_loop(toks, lens, logp, r_vocab, var_maps):
    """What the selection costs without the kernel: every candidate to text and back to words, all ordered pairs scored."""
    from fira_icse_amd import metrics, text
    toks, lens, logp = toks.tolist(), lens.tolist(), logp.tolist()
    util = []
    for b, var_map in enumerate(var_maps):
        ws = [text.detokenize(row[:n], r_vocab, var_map).split() for row, n in zip(toks[b], lens[b])]
        n = len(ws)
        util.append([math.fsum(metrics.meteor_exact(ws[j], ws[i]) for j in range(n) if j != i) / (n - 1) if n > 1 else 0.0
                     for i in range(n)])
    return metrics.mbr_pick(util, logp), util


def main(argv=None):
    a = parse_args(argv)
    import torch
    import run_model
    from rouge_probe import write_synthetic
    from fira_icse_amd import metrics, ops, text
    from fira_icse_amd.config import EOS
    from fira_icse_amd.decode import Searcher
    from fira_icse_amd.model import TransModel
    assert torch.cuda.is_available(), "meteor_probe.py needs a GPU"
    if a.synthetic is not None:
        write_synthetic(a.root, a.synthetic)
    run = run_model.Run(run_model.parse_args(["test", "--root", a.root, "--test-batch-size", str(a.test_batch_size)]
                                             + (["--splits", a.splits] if a.splits else [])))
    cfg, store, test_index = run.cfg, run.sets["test"].store, run.all_index["test"]
    var_maps = [run.var_maps[test_index[i]] for i in range(len(store))]
    refs = []
    for i in range(len(store)):
        tar = [int(t) for t in store.tar[i]]
        refs.append(text.detokenize(tar[:tar.index(EOS)] if EOS in tar else tar, run.r_vocab, var_maps[i]))
    report = []

    def say(line=""):
        print(line, flush=True)
        report.append(line)

    out_fira = run.out("output_fira")
    if os.path.exists(out_fira):
        preds = open(out_fira).read().split("\n")
        preds = preds[:-1] if preds and preds[-1] == "" else preds
        say("`%s`: corpus meteor_exact %.2f over %d messages (exact matches only, x 100; not NLTK's METEOR)"
            % (out_fira, metrics.meteor_exact_corpus(refs, preds), len(preds)))
    else:
        say("`%s` does not exist: no corpus figure" % out_fira)
    if a.sample is None:
        return

    model = TransModel(cfg, device="cuda:%d" % run.local, init=False)
    model.load_state_dict(torch.load(os.path.join(a.root, "best_model.pt"), map_location="cpu"))
    model.eval()
    run.model = model
    search = Searcher(model)
    filters = dict(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
    batches = [list(range(lo, min(lo + a.test_batch_size, len(store)))) for lo in range(0, len(store), a.test_batch_size)]
    seed0 = a.sample_seed

    lines = {u: [] for u in UTILITIES}
    samples = []
    differ = {"bleu": 0, "rouge_l": 0, "all three differ": 0, "any two differ": 0}
    for idx in batches:
        db = run.device_batch(store, idx)
        toks, lens, _, logp = search.sample(db, a.sample, seed=a.sample_seed, keys=idx, **filters)
        picks, utils = {}, {}
        for u in UTILITIES:
            picks[u], util = search.mbr(toks, lens, logp, utility=u)
            utils[u] = util.tolist()
        toks_l, lens_l, logp_l = toks.tolist(), lens.tolist(), logp.tolist()
        for k, i in enumerate(idx):
            cands = [text.detokenize(toks_l[k][j][:lens_l[k][j]], run.r_vocab, var_maps[i]) for j in range(a.sample)]
            for u in UTILITIES:
                lines[u].append(cands[picks[u][k]])
            three = [picks[u][k] for u in UTILITIES]
            differ["bleu"] += three[2] != three[0]
            differ["rouge_l"] += three[2] != three[1]
            differ["all three differ"] += len(set(three)) == 3
            differ["any two differ"] += len(set(three)) > 1
            samples.append(json.dumps({"candidates": cands, "logp": logp_l[k], "mbr_bleu": utils["bleu"][k],
                                       "mbr_rouge_l": utils["rouge_l"][k], "mbr_meteor_exact": utils["meteor_exact"][k]}))
    for name, rows in (("output_fira_mbr_meteor_exact", lines["meteor_exact"]), ("output_fira_mbr_meteor_exact_samples", samples)):
        with open(run.out(name), "w") as f:
            f.write("".join(l + "\n" for l in rows))
    n_commits = len(store)
    say("%d test commits, %d candidates each (temperature %s, top-k %s, top-p %s): the pick by expected meteor_exact differs from "
        "the pick by expected BLEU in %d commits (%.1f %%), from the pick by expected ROUGE-L in %d (%.1f %%); the three picks are "
        "not all the same in %d commits and all different in %d"
        % (n_commits, a.sample, a.temperature, a.top_k, a.top_p, differ["bleu"], 100.0 * differ["bleu"] / max(n_commits, 1),
           differ["rouge_l"], 100.0 * differ["rouge_l"] / max(n_commits, 1), differ["any two differ"], differ["all three differ"]))
    for u in UTILITIES:
        blank = sum(not l.strip() for l in lines[u])
        scored = [(r, l) for r, l in zip(refs, lines[u]) if l.strip() and r.strip()]
        say("  picked by %-12s: corpus meteor_exact %.2f, ROUGE-L %.2f (all commits), B-Norm BLEU %.2f (%d commits; %d empty picks "
            "left out)" % (u, metrics.meteor_exact_corpus(refs, lines[u]), metrics.rouge_l_corpus(refs, lines[u]),
                           metrics.bnorm_bleu([r for r, _ in scored], [l for _, l in scored]) if scored else float("nan"),
                           len(scored), blank))
    say("wrote %s and %s" % (run.out("output_fira_mbr_meteor_exact"), run.out("output_fira_mbr_meteor_exact_samples")))
    if a.reps == 0:
        return

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    idx = batches[0]
    db = run.device_batch(store, idx)
    B = len(idx)
    say()
    for draws in sorted({1, a.pool}):
        n = a.sample * draws
        parts = [search.sample(db, a.sample, seed=seed0 + 101 * d, keys=idx, **filters) for d in range(draws)]
        toks, lens, logp = (torch.cat([p[k] for p in parts], 1) for k in (0, 1, 3))
        t32, l32 = toks.to(torch.int32).contiguous(), lens.clamp(min=0, max=toks.shape[2]).to(torch.int32).contiguous()
        t = {k: [] for k in ("mbr", "kernel", "copy", "form", "host")}
        same = True
        for rep in range(a.reps + 2):
            dt_mbr, (pick, util) = timed(lambda: search.mbr(toks, lens, logp, utility="meteor_exact"))
            stats = ops.mbr_meteor_stats(t32, l32)

            def launches():
                for _ in range(a.launches):
                    ops.mbr_meteor_stats(t32, l32, stats=stats)

            dt_kernel, _ = timed(launches)
            dt_copy, host_stats = timed(stats.cpu)
            t0 = time.perf_counter()
            util2 = metrics.mbr_utilities(host_stats, "meteor_exact")
            pick2 = metrics.mbr_pick(util2, logp.cpu())
            dt_form = time.perf_counter() - t0
            t0 = time.perf_counter()
            h_pick, h_util = host_loop(toks, lens, logp, run.r_vocab, [var_maps[i] for i in idx])
            dt_host = time.perf_counter() - t0
            same &= h_pick == pick == pick2 and h_util == util.tolist() == util2
            if rep >= 2:
                for k, v in (("mbr", dt_mbr), ("kernel", dt_kernel / a.launches), ("copy", dt_copy), ("form", dt_form),
                             ("host", dt_host)):
                    t[k].append(v)
        med = {k: statistics.median(v) for k, v in t.items()}
        words = [len(text.detokenize(row[:k], run.r_vocab, var_maps[i]).split())
                 for i, rows, ks in zip(idx, toks.tolist(), lens.tolist()) for row, k in zip(rows, ks)]
        names = (("mbr", '`Searcher.mbr(utility="meteor_exact")` (launch + copy + host forming)'),
                 ("kernel", "  kernel alone (mean of %d back-to-back launches)" % a.launches),
                 ("copy", "  copy of the statistics to the host (%.1f kB)" % (B * n * n * 16 / 1e3)),
                 ("form", "  utilities and pick on the host (`mbr_utilities`, `mbr_pick`)"),
                 ("host", "host loop: detokenize, split, %d x `metrics.meteor_exact`" % (B * n * (n - 1))))
        say("### B = %d commits, n = %d candidates (T = %d), %d repetitions after 2 warm-ups, %s"
            % (B, n, cfg.tar_len, a.reps, torch.cuda.get_device_name(0)))
        say()
        say("candidates: %.1f words on average (max %d); picks and utilities identical (`==`) between `Searcher.mbr` and the host "
            "loop in every repetition: %s" % (sum(words) / len(words), max(words), same))
        say()
        say("| part | median ms | min ms | max ms |")
        say("|---|---|---|---|")
        for k, name in names:
            say("| %s | %.3f | %.3f | %.3f |" % (name, 1e3 * med[k], 1e3 * min(t[k]), 1e3 * max(t[k])))
        say()
        say("host loop / `Searcher.mbr`: %.1fx" % (med["host"] / med["mbr"]))
        say()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("`%s`\n\n" % " ".join(argv if argv is not None else sys.argv[1:]) + "\n".join(report) + "\n")


if __name__ == "__main__":
    main()
