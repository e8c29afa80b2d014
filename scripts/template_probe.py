"""Template-constrained search as a driver and as an instrument: decode the test split of a run directory under a
conventional-commit template (``decode.Template``), write the messages, count the messages the host automaton accepts, and time a
step with and without the option.

    python scripts/template_probe.py --root DIR [--beam K | --sample N] --types "fix,add,update" [--colon :] [--max-words 12]
        [--ban-words "wip,tmp"] [--test-batch-size B] [--splits a,b,c] [--reps 20] [--out profiles/template_probe.md]
    python scripts/template_probe.py --steps [--parent DIR] [--batch 64] [--reps 7] [--rounds 2] [--out profiles/template_probe.md]

``--root DIR`` is a run directory of run_model.py (DataSet/, all_index, best_model.pt).  The template reads: one of the type words,
then optionally one word of scope, then the colon word, then 1 .. ``--max-words`` words, none of them a ``--ban-words`` word
(``Template.sequence``).  Every word goes through each commit's variable map as a prefix does, so the template is per commit:
commits whose words map to the same ids are decoded together.  A type word the vocabulary lacks is dropped for that commit and the
drops are counted in one warning; a commit left without a type word, or without the colon word, is an error.  ``--beam 1`` is
greedy search, ``--beam K`` (default 3) the beam search, ``--sample N`` ``sample_search`` with N samples.  Written, in
all_index['test'] order:

    DIR/OUTPUT/output_fira_template           one message per commit (the search's best)

and printed: of the written messages of positive probability, how many ``Template.accepts`` accepts -- all of them, or the script
fails.  Timing, on the first batch, interleaved call by call: the search without the option, with the template, and with
``prefix=`` of the first type word and the colon as the nearest neighbour among the hard controls.  Two warm-up rounds (which
capture the graphs) are thrown away, every call is timed by a host clock between two device synchronisations; the median with
min and max over ``--reps`` repetitions is reported per call and per step run.  ``--reps 0`` writes the file and times nothing.

``--steps`` times whole calls on synthetic commits (the scheme of scripts/merge_probe.py: sharpened seeded weights, every call
runs its tar_len - 1 steps) in child processes of their own, one per tree, interleaved (parent, this, parent, this, ...): a beam-3
and a greedy call without the option on either tree, and on this tree under the accept-everything template, a conventional
template and ``prefix=``.  ``--parent DIR`` is a checkout of the parent commit with its library built; the options-off difference
is reported beside the run-to-run spread of either side.  Without a GPU the script fails; it never falls back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def split_words(text):
    return [w.strip() for w in (text or "").split(",") if w.strip()]


def word_id(word, vocab, var_map):
    """The vocabulary id of a word for one commit (through its variable map), or None if the vocabulary lacks it."""
    return vocab.get(var_map.get(word, word))


def commit_ids(a, vocab, var_map):
    """((type ids, colon id, banned ids) of one commit, the number of type words dropped).  Raises ValueError."""
    types = [word_id(w, vocab, var_map) for w in split_words(a.types)]
    dropped = sum(1 for t in types if t is None)
    types = tuple(sorted(set(t for t in types if t is not None)))
    colon = word_id(a.colon, vocab, var_map)
    if not types:
        raise ValueError("--types %s: the vocabulary lacks every type word" % a.types)
    if colon is None:
        raise ValueError("--colon %s: the vocabulary lacks the word" % a.colon)
    bans = tuple(sorted(set(i for i in (word_id(w, vocab, var_map) for w in split_words(a.ban_words)) if i is not None)))
    return (types, colon, bans), dropped


def template_of(key, max_words, vocab_size):
    from fira_icse_amd.config import EOS
    from fira_icse_amd.decode import Template
    types, colon, bans = key
    body = None if not bans else set(range(vocab_size)) - {EOS} - set(bans)
    return Template.sequence([(types, 1, 1), (None, 0, 1), ({colon}, 1, 1), (body, 1, max_words)], vocab_size)


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
    from fira_icse_amd.decode import Searcher
    from fira_icse_amd.model import TransModel
    assert torch.cuda.is_available(), "template_probe.py needs a GPU"
    run = run_model.Run(run_model.parse_args(["test", "--root", a.root, "--test-batch-size", str(a.test_batch_size)]
                                             + (["--splits", a.splits] if a.splits else [])))
    cfg, store, test_index = run.cfg, run.sets["test"].store, run.all_index["test"]
    var_maps = [run.var_maps[test_index[i]] for i in range(len(store))]
    keys, dropped = [], 0
    for var_map in var_maps:
        key, d = commit_ids(a, run.vocab, var_map)
        keys.append(key)
        dropped += d
    if dropped:
        print("warning: %d type words the vocabulary lacks are dropped" % dropped, file=sys.stderr, flush=True)
    templates = {key: template_of(key, a.max_words, cfg.vocab_size) for key in set(keys)}
    run.model = model = TransModel(cfg, device="cuda:%d" % run.local, init=False)
    model.load_state_dict(torch.load(os.path.join(a.root, "best_model.pt"), map_location="cpu"))
    model.eval()
    search = Searcher(model)
    chunk = 4 if a.sample is None and a.beam > 1 else 5

    def decode(db, **kw):
        """(the best message per commit, its probability, the lengths of everything returned)"""
        if a.sample is not None:
            tok, length, prob, logp = search.sample_search(db, a.sample, seed=a.seed, **kw)
            j = torch.argmax(logp, dim=1)
            return search.best_sample(tok, length, logp), prob[torch.arange(db.B), j].tolist(), length
        if a.beam == 1:
            out = search.greedy(db, **kw)
            return search.best(*out), out[2].tolist(), out[1]
        out = search.beam(db, a.beam, **kw)
        return search.best(*out[:3]), out[2].max(dim=1).values.tolist(), out[1]

    batches = [list(range(lo, min(lo + a.test_batch_size, len(store)))) for lo in range(0, len(store), a.test_batch_size)]
    lines, n_positive, n_accepted, first = [None] * len(store), 0, 0, None
    for idx in batches:
        for key in sorted(set(keys[i] for i in idx)):           # commits whose words map to the same ids: one template
            group = [i for i in idx if keys[i] == key]
            db = run.device_batch(store, group)
            first = (db, key) if first is None else first
            best, prob, _ = decode(db, template=templates[key])
            for k, i in enumerate(group):
                lines[i] = text.detokenize(best[k], run.r_vocab, var_maps[i])
                if prob[k] > 0:
                    n_positive += 1
                    n_accepted += int(templates[key].accepts(best[k][1:]))
    with open(run.out("output_fira_template"), "w") as f:
        f.write("".join(l + "\n" for l in lines))
    print("wrote %d messages to %s" % (len(lines), run.out("output_fira_template")), flush=True)
    print("the automaton accepts %d of %d messages of positive probability" % (n_accepted, n_positive), flush=True)
    if n_accepted != n_positive:
        raise SystemExit("a message of positive probability is not accepted by its template")
    if a.reps == 0:
        return
    db, key = first
    what = "sample_search %d" % a.sample if a.sample is not None else "greedy" if a.beam == 1 else "beam %d" % a.beam
    configs = {what + ", no template": {}, what + ", template": {"template": templates[key]},
               what + ", prefix= of a type word and the colon": {"prefix": [[key[0][0], key[1]]] * db.B}}
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
def steps_child(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from fira_icse_amd import data, decode, synth
    from fira_icse_amd.config import FiraConfig
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
    if a.with_template:
        T_ = decode.Template
        types, colon = (40, 41, 42), 43
        configs += [("everything", dict(template=T_({}, [[0]], [0]))),
                    ("conventional", dict(template=T_.sequence([(types, 1, 1), (None, 0, 1), ({colon}, 1, 1), (None, 1, None)],
                                                               cfg.vocab_size))),
                    ("prefix", dict(prefix=[[types[0], colon]] * B))]
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
    def run_child(tree, with_template):
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", "--child", "--tree", tree, "--batch", str(a.batch),
               "--reps", str(a.reps)] + (["--with-template"] if with_template else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("child for %s failed (%d):\n%s" % (tree, r.returncode, (r.stdout + r.stderr)[-3000:]))
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])

    pooled, info = {}, {}
    for rnd in range(a.rounds):
        for side, tree in (("parent", a.parent), ("this", REPO)):
            if tree is None:
                continue
            r = run_child(tree, side == "this")
            info = r if side == "this" else info
            for k, v in r["res"].items():
                pooled.setdefault((side, k), []).extend(v["ms"])
    steps = info["steps"]
    med = {k: statistics.median(v) for k, v in pooled.items()}
    label = {"off": "no `template` argument", "everything": "the accept-everything template", "conventional":
             "a conventional-commit template", "prefix": "`prefix=` of a type word and the colon"}
    rows = ["| search | configuration | median ms / call | min | max | median ms / step |", "|---|---|---|---|---|---|"]
    notes = []
    for kind in ("beam3", "greedy"):
        for side in ("parent", "this"):
            for name in label:
                k = (side, "%s/%s" % (kind, name))
                if k in pooled:
                    rows.append("| %s | %s, %s | %.3f | %.3f | %.3f | %.4f |" % (
                        kind, "parent commit" if side == "parent" else "this tree", label[name], med[k], min(pooled[k]),
                        max(pooled[k]), med[k] / steps))
        off = med[("this", kind + "/off")]
        for name in ("everything", "conventional", "prefix"):
            on = med[("this", "%s/%s" % (kind, name))]
            notes.append("%s: %s - off = %+.4f ms per step (%+.2f %%)" % (kind, label[name], (on - off) / steps, 100.0 * (on - off) / off))
        if ("parent", kind + "/off") in med:
            par = med[("parent", kind + "/off")]
            spread = {s: max(pooled[(s, kind + "/off")]) - min(pooled[(s, kind + "/off")]) for s in ("parent", "this")}
            notes.append("%s: option off, this tree - parent commit = %+.3f ms per call (%+.2f %%); run-to-run spread (max - min "
                         "over the processes of one side): parent %.3f ms, this tree %.3f ms"
                         % (kind, off - par, 100.0 * (off - par) / par, spread["parent"], spread["this"]))
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
    ap.add_argument("--types", default=None, help="WORD[,WORD...]: the words a message may open with")
    ap.add_argument("--colon", default=":", help="the word that follows the type and the optional scope (default ':')")
    ap.add_argument("--max-words", type=int, default=12, help="the most words after the colon (default 12)")
    ap.add_argument("--ban-words", default=None, help="WORD[,WORD...]: words that may not follow the colon")
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
    ap.add_argument("--with-template", action="store_true", help=argparse.SUPPRESS)
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
        if not split_words(a.types):
            raise ValueError("--types: no type word given")
        if not 1 <= a.max_words <= 27:
            raise ValueError("--max-words %d: outside 1..27 (the type, the scope and the colon take four of the 32 states)" % a.max_words)
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
        raise SystemExit("template_probe.py: %s" % e)


if __name__ == "__main__":
    main()
