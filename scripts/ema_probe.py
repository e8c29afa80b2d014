"""ms per training step with and without the weight average (Trainer(ema_decay=...)), same process, interleaved -- and the
option-off step of this tree against the same step of another checkout (the parent commit), in alternating fresh processes.

    python scripts/ema_probe.py [--reps 9] [--inner 64]
    python scripts/ema_probe.py --pair PATH [--rounds 5]         PATH: a built checkout of the commit to compare against
    python scripts/ema_probe.py --only off --tree PATH           (what --pair starts: one form, the package of PATH)

Batch 32, fp32.  Three trainers on three replicas of one model take turns inside every repetition: (off) Trainer(model),
(k32) ema_decay=0.999 at the default cadence 32 -- one plain streaming pass every 32nd step, on the step that has just written
every embedding row -- and (k1) ema_every=1: an update per step, reading the rows the row-sparse Adam still owes updates with
those updates replayed in registers.  A timed window is `inner` steps (a multiple of 32, so every window of k32 holds the same
number of updates) on four rotating batches, dropout on, ended by a device synchronise; medians over the repetitions.  The spread
of (off) against itself (min / max over its own repetitions) is the margin inside which a difference means nothing.

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
KINDS = (("off", None), ("k32", 32), ("k1", 1))


def window(tr, batches, inner):
    import torch
    t0 = time.perf_counter()
    for i in range(inner):
        tr.step(batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e3


def run_config(B, dtype, reps, inner, only=None):
    import torch
    from fira_icse_amd import data, synth
    from fira_icse_amd.config import FiraConfig
    from fira_icse_amd.model import DeviceBatch, TransModel
    from fira_icse_amd.train import Trainer
    cfg = FiraConfig()
    store = data.process_raw(cfg, synth.generate_dataset(256, seed=3))
    trainers = {}
    batches = None
    for name, every in KINDS:
        if only and name not in only:
            continue
        torch.manual_seed(0)
        model = TransModel(cfg)
        model.compute_dtype = dtype
        model.train()
        model.set_dropout_stream(3, 0)
        if batches is None:
            batches = [DeviceBatch(store.batch(list(range(B * i, B * i + B))), cfg, model.device_) for i in range(4)]
        trainers[name] = Trainer(model) if every is None else Trainer(model, ema_decay=0.999, ema_every=every)
    times = {k: [] for k in trainers}
    for tr in trainers.values():                                # warm-up: every shape, every code object, one update of k32
        window(tr, batches, 32)
    for _ in range(reps):
        for k, tr in trainers.items():
            times[k].append(window(tr, batches, inner))
    res = {"batch": B, "dtype": dtype, "inner": inner, "reps": reps}
    for k, v in times.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
        res[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    if "off" in times:
        a = statistics.median(times["off"])
        for k in times:
            if k != "off":
                res[k + "_over_off"] = round(statistics.median(times[k]) / a, 4)
                res[k + "_minus_off_ms"] = round(statistics.median(times[k]) - a, 4)
    for k, tr in trainers.items():
        if getattr(tr, "ema", None) is not None:
            res[k + "_updates"] = tr.ema_updates
    return res


def pair(other, rounds, reps, inner):
    """This tree and `other`, option off, in alternating fresh processes."""
    trees = (("this", os.path.dirname(HERE)), ("other", os.path.abspath(other)))
    got = {k: [] for k, _ in trees}
    for _ in range(rounds):
        for name, tree in trees:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "off", "--tree", tree, "--reps", str(reps),
                                "--inner", str(inner)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit("%s (%s) failed:\n%s" % (name, tree, r.stderr[-2000:]))
            got[name].append(json.loads(r.stdout.strip().splitlines()[-1])["off_ms"])
    res = {"pair": "option off, ms per step, batch 32 fp32", "rounds": rounds}
    for k, v in got.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
        res[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
        res[k + "_all"] = [round(x, 4) for x in v]
    res["this_over_other"] = round(statistics.median(got["this"]) / statistics.median(got["other"]), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=64, help="steps per timed window (a multiple of 32)")
    ap.add_argument("--only", default=None, help="comma-separated subset of off,k32,k1")
    ap.add_argument("--tree", default=os.path.dirname(HERE), help="the checkout whose fira_icse_amd package is measured")
    ap.add_argument("--pair", default=None, metavar="PATH", help="compare the option-off step with the built checkout at PATH")
    ap.add_argument("--rounds", type=int, default=5, help="with --pair: alternations")
    a = ap.parse_args()
    if a.inner % 32:
        ap.error("--inner must be a multiple of 32")
    if a.pair:
        print(json.dumps(pair(a.pair, a.rounds, a.reps, a.inner)), flush=True)
        return
    sys.path.insert(0, os.path.abspath(a.tree))
    only = tuple(a.only.split(",")) if a.only else None
    print(json.dumps(run_config(32, "f32", a.reps, a.inner, only)), flush=True)


if __name__ == "__main__":
    main()
