"""Per-commit word sets as a driver and as an instrument: decode the test split of a run directory under ``decode.WordSets``, write
the messages, count the written words that violate the sets, and time a step with and without the option.

    python scripts/wordset_probe.py --root DIR [--beam K | --sample N] [--ground-identifiers] [--allow-file PATH] [--deny-file PATH]
        [--boost-diff B] [--test-batch-size B] [--splits a,b,c] [--reps 20] [--out profiles/wordset_probe.md]
    python scripts/wordset_probe.py --steps [--parent DIR] [--batch 64] [--reps 7] [--rounds 2] [--out profiles/wordset_probe.md]

``--root DIR`` is a run directory of run_model.py (DataSet/, all_index, best_model.pt).  ``--ground-identifiers``: every
identifier-like word of the vocabulary (``WordSets.grounded``: a digit, ``_``, ``.``, ``/`` or an inner capital) may be written only
where the commit's diff carries it.  ``--allow-file`` / ``--deny-file``: one word per line; every word goes through each commit's
variable map as ``--ban-words`` of the other probes does, so the sets are per commit; a word the vocabulary lacks is dropped and
the drops are counted in one warning; <eos> is always allowed.  ``--boost-diff B``: every word the commit's diff carries is
multiplied by exp(B) at every step.  ``--beam 1`` is greedy search, ``--beam K`` (default 3) the beam search, ``--sample N``
``sample_search`` with N samples.  Written, in all_index['test'] order:

    DIR/OUTPUT/output_fira_wordsets           one message per commit (the search's best)

and printed: how many written words of the messages of positive probability violate the sets -- a word outside ``allow``, a word
in ``deny``, a grounded word the commit does not carry (counted on the host from the batch arrays).  That count is 0, or the
script exits non-zero.  Timing, on the first batch, interleaved call by call: the search without the option and with it.  Two
warm-up rounds (which capture the graphs) are thrown away, every call is timed by a host clock between two device
synchronisations; the median with min and max over ``--reps`` repetitions is reported per call and per step run.  ``--reps 0``
writes the file and times nothing.

``--steps`` times whole calls on synthetic commits (the scheme of scripts/template_probe.py: sharpened seeded weights, every call
runs its tar_len - 1 steps) in child processes of their own, one per tree, interleaved (parent, this, parent, this, ...): a beam-3
and a greedy call without the option on either tree, and on this tree with ``ground`` alone (every id from 4 on), with an
``allow`` of about 2 000 words, and under ``prefix=`` as the nearest neighbour (also a row of zero stores).  ``--parent DIR`` is
a checkout of the parent commit with its library built; the options-off difference is reported beside the run-to-run spread of
either side.  Without a GPU the script fails; it never falls back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def read_words(path):
    if path is None:
        return None
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def ids_of(words, vocab, var_map):
    """(the vocabulary ids of the words for one commit, through its variable map; the number of words the vocabulary lacks)"""
    ids = [vocab.get(var_map.get(w, w)) for w in words]
    return sorted(set(i for i in ids if i is not None)), sum(1 for i in ids if i is None)


def median_table(ms, steps, configs):
    rows = ["| search | median ms / call | min | max | steps run | median ms / step | / without |", "|---|---|---|---|---|---|---|"]
    base = statistics.median(ms[configs[0]]) / steps[configs[0]]
    for name in configs:
        med = statistics.median(ms[name])
        rows.append("| %s | %.3f | %.3f | %.3f | %d | %.4f | %.3f |" % (name, med, min(ms[name]), max(ms[name]), steps[name],
                                                                      med / steps[name], med / steps[name] / base))
    return rows


def emit(out, path):
    print(out, flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(out + "\n")


# ------------------------------------------------------------------------------------------------ --root: decode, count, time
def decode_root(a, argv):
    sys.path.insert(0, REPO)
    import torch
    import run_model
    from fira_icse_amd import text
    from fira_icse_amd.config import EOS, PAD, START
    from fira_icse_amd.decode import Searcher, WordSets
    from fira_icse_amd.model import TransModel
    assert torch.cuda.is_available(), "wordset_probe.py needs a GPU"
    run = run_model.Run(run_model.parse_args(["test", "--root", a.root, "--test-batch-size", str(a.test_batch_size)]
                                             + (["--splits", a.splits] if a.splits else [])))
    cfg, store, test_index = run.cfg, run.sets["test"].store, run.all_index["test"]
    var_maps = [run.var_maps[test_index[i]] for i in range(len(store))]
    allow_words, deny_words = read_words(a.allow_file), read_words(a.deny_file)
    dropped = 0
    allow_ids, deny_ids = [None] * len(store), [None] * len(store)
    for i, var_map in enumerate(var_maps):
        if allow_words is not None:
            ids, d = ids_of(allow_words, run.vocab, var_map)
            allow_ids[i] = sorted(set(w for w in ids if w > START) | {EOS})
            dropped += d
        if deny_words is not None:
            ids, d = ids_of(deny_words, run.vocab, var_map)
            deny_ids[i] = [w for w in ids if w > START]
            dropped += d
    if dropped:
        print("warning: %d words the vocabulary lacks are dropped" % dropped, file=sys.stderr, flush=True)
    ground = ()
    if a.ground_identifiers:
        r_vocab = run.r_vocab
        words = [(r_vocab.get(w, "") if hasattr(r_vocab, "get") else r_vocab[w]) for w in range(cfg.vocab_size)]
        ground = WordSets.grounded(words).ground
    run.model = model = TransModel(cfg, device="cuda:%d" % run.local, init=False)
    model.load_state_dict(torch.load(os.path.join(a.root, "best_model.pt"), map_location="cpu"))
    model.eval()
    search = Searcher(model)
    chunk = 4 if a.sample is None and a.beam > 1 else 5

    def carried_of(db):
        ids = torch.cat([db.sou, db.sub_token], 1).cpu().tolist() if cfg.sub_token_len else db.sou.cpu().tolist()
        return [set(w for w in row if w != PAD) for row in ids]

    def sets_of(group, carried):
        return WordSets(allow=None if allow_words is None else [allow_ids[i] for i in group],
                        deny=None if deny_words is None else [deny_ids[i] for i in group],
                        boost=None if a.boost_diff is None else [sorted(w for w in c if w > START or w == EOS) for c in carried],
                        boost_bias=0.0 if a.boost_diff is None else a.boost_diff, ground=ground or None)

    def decode(db, **kw):
        """(the best message per commit, its probability or score, the lengths of everything returned)"""
        if a.sample is not None:
            tok, length, prob, logp = search.sample_search(db, a.sample, seed=a.seed, **kw)
            j = torch.argmax(logp, dim=1)
            return search.best_sample(tok, length, logp), prob[torch.arange(db.B), j].tolist(), length
        if a.beam == 1:
            out = search.greedy(db, **kw)
            return search.best(*out), out[2].tolist(), out[1]
        out = search.beam(db, a.beam, **kw)
        return search.best(*out[:3]), out[2].max(dim=1).values.tolist(), out[1]

    grounded = set(ground)
    batches = [list(range(lo, min(lo + a.test_batch_size, len(store)))) for lo in range(0, len(store), a.test_batch_size)]
    lines, n_positive, n_words, n_violations, first = [None] * len(store), 0, 0, 0, None
    for group in batches:
        db = run.device_batch(store, group)
        carried = carried_of(db)
        sets = sets_of(group, carried)
        first = (db, sets) if first is None else first
        best, prob, _ = decode(db, wordsets=sets)
        for k, i in enumerate(group):
            lines[i] = text.detokenize(best[k], run.r_vocab, var_maps[i])
            if prob[k] > 0:
                n_positive += 1
                for w in best[k][1:]:
                    n_words += 1
                    n_violations += int((allow_ids[i] is not None and w != EOS and w not in allow_ids[i])
                                        or (deny_ids[i] is not None and w in deny_ids[i])
                                        or (w in grounded and w not in carried[k]))
    with open(run.out("output_fira_wordsets"), "w") as f:
        f.write("".join(l + "\n" for l in lines))
    print("wrote %d messages to %s" % (len(lines), run.out("output_fira_wordsets")), flush=True)
    print("%d of the %d written words of %d messages of positive probability violate the sets" % (n_violations, n_words, n_positive),
          flush=True)
    if n_violations:
        raise SystemExit("a message of positive probability holds a word its sets block")
    if a.reps == 0:
        return
    db, sets = first
    what = "sample_search %d" % a.sample if a.sample is not None else "greedy" if a.beam == 1 else "beam %d" % a.beam
    configs = {what + ", no word sets": {}, what + ", word sets (%s)" % ", ".join(sets.given): {"wordsets": sets}}
    ms, steps = {name: [] for name in configs}, {}
    for rep in range(a.reps + 2):
        for name, kw in configs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            length = decode(db, **kw)[2]
            torch.cuda.synchronize()
            if rep >= 2:
                ms[name].append(1e3 * (time.perf_counter() - t0))
            ended = int(length.max()) - 1                       # the step count after which every hypothesis had ended
            steps[name] = max(1, min(cfg.tar_len - 1, -(-ended // chunk) * chunk))
    emit("\n".join(["### %s: B = %d, %d interleaved repetitions after 2 warm-ups, graphs of %d steps" % (
        torch.cuda.get_device_name(0), db.B, a.reps, chunk), "", "`%s`" % " ".join(argv), ""]
        + median_table(ms, steps, list(configs)) + [""]), a.out)


# ------------------------------------------------------------------------------------------------ --steps: this tree and the parent
LABEL = {"off": "no `wordsets` argument", "ground": "`ground` alone (every id from 4 on)", "allow": "an `allow` of 2 000 words",
         "prefix": "`prefix=` of two words"}


def steps_child(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from fira_icse_amd import data, decode, synth
    from fira_icse_amd.config import EOS, FiraConfig
    from fira_icse_amd.decode import Searcher
    from fira_icse_amd.model import DeviceBatch, TransModel
    assert os.path.abspath(decode.__file__).startswith(os.path.abspath(a.tree) + os.sep), decode.__file__
    B = a.batch
    cfg = FiraConfig()
    store = data.process_raw(cfg, synth.generate_dataset(B, seed=5))
    torch.manual_seed(0)
    model = TransModel(cfg)
    with torch.no_grad():
        sd = model.state_dict()
        sd["out_fc.weight"] = sd["out_fc.weight"] * 10.0
        model.load_state_dict(sd)
    model.eval()
    search = Searcher(model)
    db = DeviceBatch(store.batch(list(range(B))), cfg)
    configs = [("off", {})]
    if a.with_wordsets:
        W_ = decode.WordSets
        allow = [EOS] + list(range(4, cfg.vocab_size, cfg.vocab_size // 2000))[:2000]
        configs += [("ground", dict(wordsets=W_(ground=range(4, cfg.vocab_size)))), ("allow", dict(wordsets=W_(allow=allow))),
                    ("prefix", dict(prefix=[[40, 43]] * B))]
    res = {}
    for name, kw in configs:
        for kind, fn in (("beam3", lambda: search.beam(db, 3, **kw)), ("greedy", lambda: search.greedy(db, **kw))):
            ts = []
            for rep in range(a.reps + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                if rep >= 2:
                    ts.append(time.perf_counter() - t0)
            length = out[1].float()
            res["%s/%s" % (kind, name)] = dict(ms=[1e3 * t for t in ts], mean_len=float(length.mean()), max_len=int(length.max()))
    print("RESULT " + json.dumps(dict(tree=a.tree, device=torch.cuda.get_device_name(0), steps=cfg.tar_len - 1, res=res)), flush=True)


def steps_parent(a):
    def run_child(tree, with_wordsets):
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", "--child", "--tree", tree, "--batch", str(a.batch),
               "--reps", str(a.reps)] + (["--with-wordsets"] if with_wordsets else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("child for %s failed (%d):\n%s" % (tree, r.returncode, (r.stdout + r.stderr)[-3000:]))
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])

    pooled, per_process, info = {}, {}, {}
    for rnd in range(a.rounds):
        for side, tree in (("parent", a.parent), ("this", REPO)):
            if tree is None:
                continue
            r = run_child(tree, side == "this")
            info = r if side == "this" else info
            for k, v in r["res"].items():
                pooled.setdefault((side, k), []).extend(v["ms"])
                per_process.setdefault((side, k), []).append(statistics.median(v["ms"]))
    steps = info["steps"]
    med = {k: statistics.median(v) for k, v in pooled.items()}
    rows = ["| search | configuration | median ms / call | min | max | median ms / step |", "|---|---|---|---|---|---|"]
    notes = []
    for kind in ("beam3", "greedy"):
        for side in ("parent", "this"):
            for name in LABEL:
                k = (side, "%s/%s" % (kind, name))
                if k in pooled:
                    rows.append("| %s | %s, %s | %.3f | %.3f | %.3f | %.4f |" % (
                        kind, "parent commit" if side == "parent" else "this tree", LABEL[name], med[k], min(pooled[k]),
                        max(pooled[k]), med[k] / steps))
        off = med[("this", kind + "/off")]
        for name in ("ground", "allow", "prefix"):
            on = med[("this", "%s/%s" % (kind, name))]
            notes.append("%s: %s - off = %+.4f ms per step (%+.2f %%)" % (kind, LABEL[name], (on - off) / steps, 100.0 * (on - off) / off))
        own = per_process[("this", kind + "/off")]
        notes.append("%s: option off, this tree against itself: the processes' medians span %.3f ms per call (%s)"
                     % (kind, max(own) - min(own), ", ".join("%.3f" % m for m in own)))
        if ("parent", kind + "/off") in med:
            par = med[("parent", kind + "/off")]
            theirs = per_process[("parent", kind + "/off")]
            notes.append("%s: option off, this tree - parent commit = %+.3f ms per call (%+.2f %%); the parent's processes' medians "
                         "span %.3f ms per call (%s)" % (kind, off - par, 100.0 * (off - par) / par, max(theirs) - min(theirs),
                                                         ", ".join("%.3f" % m for m in theirs)))
    lens = ", ".join("%s: mean %.1f / max %d" % (k, v["mean_len"], v["max_len"]) for k, v in sorted(info["res"].items()))
    emit("\n".join(["### B = %d commits, %d steps per call, %d rounds x %d repetitions after 2 warm-ups, %s" % (
        a.batch, steps, a.rounds, a.reps, info["device"]), "",
        "hypothesis lengths (this tree; tar_len = %d means the search ran every step): %s" % (steps + 1, lens), ""]
        + rows + [""] + ["- " + n for n in notes] + [""]), a.out)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=None, help="a run directory of run_model.py (DataSet/, all_index, best_model.pt)")
    ap.add_argument("--beam", type=int, default=None, help="beam size (default 3; 1 = greedy)")
    ap.add_argument("--sample", type=int, default=None, metavar="N", help="sample_search with N samples per commit instead of a beam")
    ap.add_argument("--seed", type=int, default=0, help="the seed of --sample")
    ap.add_argument("--ground-identifiers", action="store_true", help="identifier-like words only where the diff carries them")
    ap.add_argument("--allow-file", default=None, metavar="PATH", help="one word per line: only these words may be written")
    ap.add_argument("--deny-file", default=None, metavar="PATH", help="one word per line: these words may not be written")
    ap.add_argument("--boost-diff", type=float, default=None, metavar="B", help="multiply every word the diff carries by exp(B)")
    ap.add_argument("--test-batch-size", type=int, default=20)
    ap.add_argument("--splits", default=None, help="as run_model.py --splits")
    ap.add_argument("--reps", type=int, default=None, help="timed repetitions after 2 warm-ups (--root: default 20, 0 = none)")
    ap.add_argument("--out", default=None, help="append the timing as markdown to this file")
    ap.add_argument("--steps", action="store_true", help="time whole calls on synthetic commits, this tree against --parent")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=2, help="interleaved (parent, this) rounds")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=REPO, help=argparse.SUPPRESS)
    ap.add_argument("--with-wordsets", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    try:
        if a.steps:
            a.reps = 7 if a.reps is None else a.reps
            if a.reps < 3:
                raise ValueError("--reps %d: at least 3" % a.reps)
            return a
        a.reps = 20 if a.reps is None else a.reps
        if a.root is None:
            raise ValueError("one of --root DIR and --steps is required")
        if a.beam is not None and a.sample is not None:
            raise ValueError("--beam and --sample are mutually exclusive")
        a.beam = 3 if a.beam is None else a.beam
        if not 1 <= a.beam <= 8:
            raise ValueError("--beam %d: outside 1..8" % a.beam)
        if a.sample is not None and not 1 <= a.sample <= 8:
            raise ValueError("--sample %d: outside 1..8" % a.sample)
        if not (a.ground_identifiers or a.allow_file or a.deny_file or a.boost_diff is not None):
            raise ValueError("no set given: one of --ground-identifiers, --allow-file, --deny-file and --boost-diff")
        if a.test_batch_size < 1:
            raise ValueError("--test-batch-size %d: at least 1" % a.test_batch_size)
        if a.reps < 0 or 0 < a.reps < 3:
            raise ValueError("--reps %d: 0 (no timing) or at least 3" % a.reps)
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    a = parse_args(argv)
    if a.steps:
        return steps_child(a) if a.child else steps_parent(a)
    try:
        decode_root(a, argv)
    except ValueError as e:
        raise SystemExit("wordset_probe.py: %s" % e)


if __name__ == "__main__":
    main()
