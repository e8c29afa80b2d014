"""ms per search step of beam-3 and beam-5 search with 0, 1 and 3 required words per commit, same process, interleaved -- and the
options-off searches of this tree against the same searches of another checkout (the parent commit), in alternating fresh
processes.

    python scripts/require_probe.py [--reps 9] [--inner 8]
    python scripts/require_probe.py --pair PATH [--rounds 5]      PATH: a built checkout of the commit to compare against
    python scripts/require_probe.py --only off --tree PATH        (what --pair starts: one form, the package of PATH)

Batch 20 (run_model.py's test batch), fp32, the seeded initialisation with sharpened output heads and no <eos> bias: a call is
meant to run all tar_len - 1 = 29 steps, and ms per step is the call divided by 29 (the mean message length is printed beside
every figure: below 30, some calls stopped early and the figure is too low for all forms alike).  Four forms take turns inside
every repetition, each on its own captured graphs: (off) no require argument -- today's search with fira_beam_select; (zero) the
require state with every n_required 0 -- fira_beam_select_required runs with one bank and returns fira_beam_select's result;
(one) one required word per commit; (three) three (beam 5 only: a beam needs a bank per count).  The words are fixed ids of
the vocabulary; the mean number of words met over the returned slots is printed beside the figures (0 means the words had no
positive probability under these weights, and the higher banks stayed empty).  A timed window is
`inner` calls ended by a device synchronise; medians over the repetitions.  The spread of (off) against itself (min / max over
its own repetitions) is the margin inside which a difference means nothing.

--pair: the acceptance check for the options-off path.  The two trees take turns, each measurement in a fresh process, so that
clocks and the state of the box drift over both alike; the medians and each side's min / max are printed."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("off", "zero", "one", "three")
BEAMS = (3, 5)
WORDS = (700, 1500, 2300)


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
    args = {"off": {}, "zero": {"require": [[] for _ in range(B)]}, "one": {"require": [list(WORDS[:1])] * B},
            "three": {"require": [list(WORDS)] * B}}
    if "zero" in search:                                      # an all-empty list is today's search by contract: keep it active
        search["zero"]._required_rows = lambda require, B_, beam, con, scoring: [list(p) for p in require]

    def call(kind, beam):
        return search[kind].beam(db, beam, **args[kind])

    def window(kind, beam):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            call(kind, beam)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / inner / (cfg.tar_len - 1) * 1e3

    res = {"batch": B, "inner": inner, "reps": reps, "steps_per_call": cfg.tar_len - 1}
    for beam in BEAMS:
        what = "beam%d" % beam
        mine = [k for k in kinds if not (k == "three" and beam < len(WORDS) + 1)]
        for k in mine:                                        # warm-up: capture
            out = call(k, beam)
            res["%s_%s_mean_length" % (what, k)] = round(float(out[1].float().mean()), 2)
            if len(out) == 4 and k != "zero":
                res["%s_%s_mean_met" % (what, k)] = round(float(out[3].float().mean()), 2)
        times = {k: [] for k in mine}
        for _ in range(reps):
            for k in mine:
                times[k].append(window(k, beam))
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
    """This tree and `other`, options off, in alternating fresh processes."""
    trees = (("this", os.path.dirname(HERE)), ("other", os.path.abspath(other)))
    names = ["beam%d" % b for b in BEAMS]
    got = {(k, w): [] for k, _ in trees for w in names}
    for _ in range(rounds):
        for name, tree in trees:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "off", "--tree", tree, "--reps", str(reps),
                                "--inner", str(inner)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit("%s (%s) failed:\n%s" % (name, tree, r.stderr[-2000:]))
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            for w in names:
                got[name, w].append(rec["%s_off_ms" % w])
    res = {"pair": "options off, ms per search step, batch 20 fp32", "rounds": rounds}
    for (k, w), v in got.items():
        res["%s_%s_ms" % (k, w)] = round(statistics.median(v), 4)
        res["%s_%s_min_max" % (k, w)] = [round(min(v), 4), round(max(v), 4)]
    for w in names:
        res["this_over_other_%s" % w] = round(statistics.median(got["this", w]) / statistics.median(got["other", w]), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=8, help="search calls per timed window")
    ap.add_argument("--only", default=None, help="comma-separated subset of off,zero,one,three")
    ap.add_argument("--tree", default=os.path.dirname(HERE), help="the checkout whose fira_icse_amd package is measured")
    ap.add_argument("--pair", default=None, metavar="PATH", help="compare the options-off searches with the built checkout at PATH")
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
