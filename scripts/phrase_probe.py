"""Phrases in the hard search controls as a driver and as an instrument: decode the test split of a run directory with banned and
required word sequences (``decode.Phrases``), write the messages, count the messages that hold all their items, and time a step
with and without the options.

    python scripts/phrase_probe.py --root DIR [--beam K] [--ban-phrases "minor changes,fix bug"]
        [--require-phrases "abc-123,revert" | --require-phrase-file PATH] [--merge-copies]
        [--test-batch-size B] [--splits a,b,c] [--reps 20] [--out profiles/phrase_probe.md]

``--root DIR`` is a run directory of run_model.py (DataSet/, all_index, best_model.pt).  ``--beam 1`` is greedy search (banned
phrases only), ``--beam K`` (default 3) the beam search; required items need ``K`` at least their number of words plus one.
Phrases are separated by commas.  A phrase is split at punctuation as the scorer splits messages (``metrics.split_punct``:
``abc-123`` is ``abc - 123``), tokenised with ``text.tokenize_message`` and so sent through each commit's variable map as a prefix
is (the commit's identifiers to their placeholders): the lists are per commit.  A phrase with a word the vocabulary lacks is
dropped for that commit, and the drops are counted in one warning; so is a banned phrase of one word (``Constraints.banned`` bans
words).  ``--require-phrase-file PATH`` has one line per test commit (an empty line: no item).  What ``decode.Phrases`` refuses
-- more than 8 banned phrases, a phrase of more than 4 words, more than 4 required words per commit -- is refused with its
reason.  Written, in all_index['test'] order:

    DIR/OUTPUT/output_fira_phrases            one message per commit (``best_required``'s pick with required items)

Timing, on the first batch of the split, interleaved call by call: the search without the options, the search with them and,
with required items, ``beam(require=)`` with the items' words as single words (at most 4).  Two warm-up rounds (which capture
the graphs) are thrown away, every call is timed by a host clock between two device synchronisations, and the median with min and
max over ``--reps`` repetitions is reported per call and per step run.  ``--reps 0`` writes the file and times nothing.  Without a
GPU the script fails; it never falls back."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)


def parse_phrases(text):
    """'a b,c-1' -> [['a', 'b'], ['c', '-', '1']]: commas separate phrases, punctuation is split off as the scorer splits it."""
    from fira_icse_amd.metrics import split_punct
    return [split_punct(item).split() for item in (text or "").split(",") if item.strip()]


def phrase_ids(words, vocab, var_map):
    """The vocabulary ids of a phrase for one commit (``text.tokenize_message`` without <start> / <eos>), or None if the
    vocabulary lacks a word."""
    from fira_icse_amd import text
    if any(var_map.get(w, w) not in vocab for w in words):
        return None
    return tuple(text.tokenize_message(" ".join(words), vocab, var_map, len(words) + 2)[1:-1])


def read_lines(path, n_commits):
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if len(lines) != n_commits:
        raise ValueError("--require-phrase-file %s: %d lines for %d test commits" % (path, len(lines), n_commits))
    return lines


def phrases_from_args(a, vocab, var_maps):
    """(the ``Phrases`` value of the command line for the test commits in order, the number of phrases dropped).  A phrase that
    maps to the same ids as an earlier one of its commit is kept once.  Raises ValueError with ``Phrases``' own reason."""
    from fira_icse_amd.decode import Phrases
    n = len(var_maps)
    ban_words = parse_phrases(a.ban_phrases)
    if a.require_phrase_file is not None:
        req_words = [parse_phrases(line) for line in read_lines(a.require_phrase_file, n)]
    else:
        req_words = [parse_phrases(a.require_phrases)] * n
    banned, required, dropped = [], [], 0
    for var_map, req in zip(var_maps, req_words):
        rows = []
        for words, least in ((ban_words, 2), (req, 1)):
            row = []
            for ph in words:
                ids = phrase_ids(ph, vocab, var_map)
                if ids is None or len(ids) < least:
                    dropped += 1
                elif ids not in row:
                    row.append(ids)
            rows.append(row)
        banned.append(rows[0])
        required.append(rows[1])
    return Phrases(banned=banned if any(banned) else (), required=required if any(required) else ()), dropped


def holds_all(message_ids, items):
    from fira_icse_amd.decode import contains_phrase
    return all(contains_phrase(message_ids, item) for item in items)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True, help="a run directory of run_model.py (DataSet/, all_index, best_model.pt)")
    ap.add_argument("--beam", type=int, default=3, help="beam size (default 3; 1 = greedy)")
    ap.add_argument("--ban-phrases", default=None, help="PHRASE[,PHRASE...]: word sequences no message may contain")
    ap.add_argument("--require-phrases", default=None, help="ITEM[,ITEM...]: word sequences every message must contain")
    ap.add_argument("--require-phrase-file", default=None, metavar="PATH", help="one line of items per test commit")
    ap.add_argument("--merge-copies", action="store_true", help="search words, not entries")
    ap.add_argument("--test-batch-size", type=int, default=20)
    ap.add_argument("--splits", default=None, help="as run_model.py --splits")
    ap.add_argument("--reps", type=int, default=20, help="timed repetitions after 2 warm-ups (0: no timing)")
    ap.add_argument("--out", default=None, help="append the timing as markdown to this file")
    a = ap.parse_args(argv)
    try:
        if not 1 <= a.beam <= 8:
            raise ValueError("--beam %d: outside 1..8" % a.beam)
        if a.require_phrases is not None and a.require_phrase_file is not None:
            raise ValueError("--require-phrases and --require-phrase-file are mutually exclusive")
        if a.require_phrase_file is not None and not os.path.isfile(a.require_phrase_file):
            raise ValueError("--require-phrase-file %s: no such file" % a.require_phrase_file)
        if (a.require_phrases is not None or a.require_phrase_file is not None) and a.beam < 2:
            raise ValueError("required items divide a beam into banks: they do not combine with --beam %d" % a.beam)
        for flag, value in (("--ban-phrases", a.ban_phrases), ("--require-phrases", a.require_phrases)):
            if value is not None and not parse_phrases(value):
                raise ValueError("%s: no phrase given" % flag)
        if a.test_batch_size < 1:
            raise ValueError("--test-batch-size %d: at least 1" % a.test_batch_size)
        if a.reps < 0 or 0 < a.reps < 3:
            raise ValueError("--reps %d: 0 (no timing) or at least 3" % a.reps)
        # the shape of the lists, ahead of any file (every word stands for some id: only counts and lengths are looked at)
        words = {w: 7 + k for k, w in enumerate(sorted(set(w for t in (a.ban_phrases, a.require_phrases) for ph in parse_phrases(t)
                                                               for w in ph)))}
        words.update({"<pad>": 0, "<eos>": 1, "<start>": 2, "<unkm>": 3})
        shape = argparse.Namespace(ban_phrases=a.ban_phrases, require_phrases=a.require_phrases, require_phrase_file=None)
        value, _ = phrases_from_args(shape, words, [{}])
        total = sum(len(item) for item in value.required[0]) if value.required else 0
        if total and a.beam < total + 1:
            raise ValueError("--require-phrases: %d words need --beam %d at least, --beam is %d" % (total, total + 1, a.beam))
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    import run_model
    from fira_icse_amd import text
    from fira_icse_amd.decode import Phrases, Searcher
    from fira_icse_amd.model import TransModel
    assert torch.cuda.is_available(), "phrase_probe.py needs a GPU"
    run = run_model.Run(run_model.parse_args(["test", "--root", a.root, "--test-batch-size", str(a.test_batch_size)]
                                             + (["--splits", a.splits] if a.splits else [])))
    cfg, store, test_index = run.cfg, run.sets["test"].store, run.all_index["test"]
    var_maps = [run.var_maps[test_index[i]] for i in range(len(store))]
    phrases, dropped = phrases_from_args(a, run.vocab, var_maps)
    if dropped:
        print("warning: %d phrases hold a word the vocabulary lacks (or are one banned word) and are dropped" % dropped,
              file=sys.stderr, flush=True)
    run.model = model = TransModel(cfg, device="cuda:%d" % run.local, init=False)
    model.load_state_dict(torch.load(os.path.join(a.root, "best_model.pt"), map_location="cpu"))
    model.eval()
    search = Searcher(model)
    chunk = 5 if a.beam == 1 else 4
    banned_all = phrases.banned_rows(len(store)) if phrases.ban_active else [()] * len(store)
    required_all = list(phrases.required) if phrases.require_active else [()] * len(store)

    def batch_value(idx):
        ban, req = [banned_all[i] for i in idx], [required_all[i] for i in idx]
        return Phrases(banned=ban if any(ban) else (), required=req if any(req) else ())

    def decode(db, ph=None, require=None):
        if a.beam == 1:
            return search.greedy(db, merge_copies=a.merge_copies, phrases=ph)
        return search.beam(db, a.beam, merge_copies=a.merge_copies, phrases=ph, require=require)

    def pick(out):
        return search.best_required(*out) if len(out) == 4 else search.best(*out)

    batches = [list(range(lo, min(lo + a.test_batch_size, len(store)))) for lo in range(0, len(store), a.test_batch_size)]
    lines, n_hold, n_with, first = [], 0, 0, None
    for idx in batches:
        db = run.device_batch(store, idx)
        first = (db, idx) if first is None else first
        best = pick(decode(db, batch_value(idx)))
        for k, i in enumerate(idx):
            lines.append(text.detokenize(best[k], run.r_vocab, var_maps[i]))
            if required_all[i]:
                n_with += 1
                n_hold += int(holds_all(best[k][1:], required_all[i]))
    with open(run.out("output_fira_phrases"), "w") as f:
        f.write("".join(l + "\n" for l in lines))
    print("wrote %d messages to %s" % (len(lines), run.out("output_fira_phrases")), flush=True)
    print("%d of %d messages with required items hold all their items" % (n_hold, n_with), flush=True)
    if a.reps == 0:
        return
    db, idx = first
    what = "greedy" if a.beam == 1 else "beam %d" % a.beam
    value = batch_value(idx)
    configs = [(what + ", no phrases", {})]
    if value.require_active:
        words = [list(dict.fromkeys(w for item in row for w in item if w > 3))[:4] for row in value.required]
        configs.append((what + ", require= with the items' words", {"require": words}))
    if value.active:
        configs.append((what + ", phrases", {"ph": value}))
    T = cfg.tar_len
    ms, steps = {name: [] for name, _ in configs}, {}
    for rep in range(a.reps + 2):
        for name, kw in configs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = decode(db, **kw)
            torch.cuda.synchronize()
            if rep >= 2:
                ms[name].append(1e3 * (time.perf_counter() - t0))
            ended = int(out[1].max()) - 1                                # the step count after which every hypothesis had ended
            steps[name] = max(1, min(T - 1, -(-ended // chunk) * chunk))
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
