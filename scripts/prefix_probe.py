"""ms per search step of greedy and beam-3 search with the prefix option off, with an empty-but-active prefix state, and with a
3-word prefix, same process, interleaved -- and the option-off searches of this tree against the same searches of another
checkout (the parent commit), in alternating fresh processes.

    python scripts/prefix_probe.py [--reps 9] [--inner 8]
    python scripts/prefix_probe.py --pair PATH [--rounds 5]      PATH: a built checkout of the commit to compare against
    python scripts/prefix_probe.py --only off --tree PATH        (what --pair starts: one form, the package of PATH)

Batch 20 (run_model.py's test batch), fp32, the seeded initialisation with sharpened output heads and no <eos> bias: a call is
meant to run all tar_len - 1 = 29 steps, and ms per step is the call divided by 29 (the mean message length is printed beside
every figure: below 30, some calls stopped early and the figure is too low for all forms alike).  Three forms take
turns inside every repetition, each on its own captured graphs: (off) no prefix argument -- today's search; (empty) the prefix
state with every prefix_len 0 -- the step writes its distribution and fira_force_dist runs, but no row is forced: under greedy
search it streams every row once for the arg-max, under beam search it ends after its two small loads; (three) every commit
forced to a 3-word prefix, so 3 of the 29 steps store their rows' zeros.  A timed window is `inner` calls ended by a device
synchronise; medians over the repetitions.  The spread of (off) against itself (min / max over its own repetitions) is the margin
inside which a difference means nothing.

--pair: the acceptance check for the option-off path.  The two trees take turns, each measurement in a fresh process, so that
clocks and the state of the box drift over both alike; the medians and each side's min / max are printed."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("off", "empty", "three")
SEARCHES = ("greedy", "beam3")


def peaked(sd):
    """Sharper generator / copy heads (the decode tests' weights without their <eos> bias: the messages do not end early)."""
    sd["out_fc.weight"] = sd["out_fc.weight"] * 24.0
    sd["copy_net.LinearRes.weight"] = sd["copy_net.LinearRes.weight"] * 24.0
    return sd


def run_config(B, reps, inner, only=None):
    import torch
    from fira_icse_amd import data, synth
    from fira_icse_amd.config import FiraConfig
    from fira_icse_amd.decode import Searcher
    from fira_icse_amd.model import DeviceBatch, TransModel, reference_init_state_dict
    cfg = FiraConfig()
    store = data.process_raw(cfg, synth.generate_dataset(64, seed=3))
    torch.manual_seed(0)
    model = TransModel(cfg, init=False)
    model.load_state_dict(peaked(reference_init_state_dict(cfg)))
    model.eval()
    db = DeviceBatch(store.batch(list(range(B))), cfg, model.device_)
    kinds = [k for k in KINDS if not only or k in only]
    search = {k: Searcher(model) for k in kinds}              # one Searcher per form: its own states and graphs
    g = search[kinds[0]].greedy(db)
    # the unforced message's own first words (always forceable), cut where a message is shorter than three words
    three = [row[1:1 + min(3, next((i for i, w in enumerate(row[1:4]) if w < 3), 3))] for row in g[0].tolist()]
    args = {"off": {}, "empty": {"prefix": [[] for _ in range(B)]}, "three": {"prefix": three}}
    if "empty" in search:                                     # an all-empty prefix is today's search by contract: keep it active
        search["empty"]._prefix_rows = lambda prefix, B_, con: [list(p) for p in prefix]

    def call(kind, what):
        s = search[kind]
        return s.greedy(db, **args[kind]) if what == "greedy" else s.beam(db, 3, **args[kind])

    def window(kind, what):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            call(kind, what)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / inner / (cfg.tar_len - 1) * 1e3

    res = {"batch": B, "inner": inner, "reps": reps, "steps_per_call": cfg.tar_len - 1}
    for what in SEARCHES:
        for k in kinds:                                       # warm-up: capture
            out = call(k, what)
            res["%s_%s_mean_length" % (what, k)] = round(float(out[1].float().mean()), 2)
        times = {k: [] for k in kinds}
        for _ in range(reps):
            for k in kinds:
                times[k].append(window(k, what))
        for k, v in times.items():
            res["%s_%s_ms" % (what, k)] = round(statistics.median(v), 4)
            res["%s_%s_min_max" % (what, k)] = [round(min(v), 4), round(max(v), 4)]
        if "off" in times:
            a = statistics.median(times["off"])
            for k in times:
                if k != "off":
                    res["%s_%s_minus_off_ms" % (what, k)] = round(statistics.median(times[k]) - a, 4)
    return res


def pair(other, rounds, reps, inner):
    """This tree and `other`, option off, in alternating fresh processes."""
    trees = (("this", os.path.dirname(HERE)), ("other", os.path.abspath(other)))
    got = {(k, w): [] for k, _ in trees for w in SEARCHES}
    for _ in range(rounds):
        for name, tree in trees:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "off", "--tree", tree, "--reps", str(reps),
                                "--inner", str(inner)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit("%s (%s) failed:\n%s" % (name, tree, r.stderr[-2000:]))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            for w in SEARCHES:
                got[name, w].append(rec["%s_off_ms" % w])
    res = {"pair": "option off, ms per search step, batch 20 fp32", "rounds": rounds}
    for (k, w), v in got.items():
        res["%s_%s_ms" % (k, w)] = round(statistics.median(v), 4)
        res["%s_%s_min_max" % (k, w)] = [round(min(v), 4), round(max(v), 4)]
    for w in SEARCHES:
        res["this_over_other_%s" % w] = round(statistics.median(got["this", w]) / statistics.median(got["other", w]), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=8, help="search calls per timed window")
    ap.add_argument("--only", default=None, help="comma-separated subset of off,empty,three")
    ap.add_argument("--tree", default=os.path.dirname(HERE), help="the checkout whose fira_icse_amd package is measured")
    ap.add_argument("--pair", default=None, metavar="PATH", help="compare the option-off searches with the built checkout at PATH")
    ap.add_argument("--rounds", type=int, default=5, help="with --pair: alternations")
    a = ap.parse_args()
    if a.pair:
        print(json.dumps(pair(a.pair, a.rounds, a.reps, a.inner)), flush=True)
        return
    sys.path.insert(0, os.path.abspath(a.tree))
    only = tuple(a.only.split(",")) if a.only else None
    print(json.dumps(run_config(20, a.reps, a.inner, only)), flush=True)


if __name__ == "__main__":
    main()
