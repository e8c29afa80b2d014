"""ms per training step with and without a learning-rate schedule, same process, interleaved.

    python scripts/sched_probe.py [--reps 9] [--inner 20]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/sched_probe.py --profile 10      (kernel rows of a scheduled run)

Per configuration (batch 32 in fp32, batch 64 in bf16) two trainers on two replicas of one model take turns inside every
repetition: (a) Trainer(model) -- no schedule, (b) a cosine schedule with warmup (the rate changes at every step).  A timed
window is `inner` steps on four rotating batches, dropout on, ended by a device synchronise; medians over the repetitions.  The
spread of (a) against itself (min / max over its own repetitions) is the margin inside which a difference means nothing: a
schedule adds no launch and no synchronisation (the rate of every step a lazy row owes travels in the argument block), so (b)
is expected inside it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from fira_icse_amd import data, synth                      # noqa: E402
from fira_icse_amd.config import FiraConfig                 # noqa: E402
from fira_icse_amd.model import DeviceBatch, TransModel     # noqa: E402
from fira_icse_amd.train import Trainer                     # noqa: E402


def kinds(cfg):
    return (("a_no_schedule", None),
            ("b_cosine", dict(kind="cosine", base_lr=cfg.lr, warmup_steps=50, decay_steps=2000, min_lr=0.1 * cfg.lr)))


def window(tr, batches, inner):
    t0 = time.perf_counter()
    for i in range(inner):
        tr.step(batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e3


def run_config(cfg, store, B, dtype, reps, inner, only=None):
    trainers = {}
    batches = None
    for name, schedule in kinds(cfg):
        if only and name not in only:
            continue
        torch.manual_seed(0)
        model = TransModel(cfg)
        model.compute_dtype = dtype
        model.train()
        model.set_dropout_stream(3, 0)
        if batches is None:
            batches = [DeviceBatch(store.batch(list(range(B * i, B * i + B))), cfg, model.device_) for i in range(4)]
        trainers[name] = Trainer(model, lr_schedule=schedule)
    times = {k: [] for k in trainers}
    for tr in trainers.values():                                # warm-up: every shape, every code object
        window(tr, batches, 8)
    for _ in range(reps):
        for k, tr in trainers.items():
            times[k].append(window(tr, batches, inner))
    res = {"batch": B, "dtype": dtype}
    for k, v in times.items():
        res[k + "_ms"] = round(statistics.median(v), 4)
        res[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    if "a_no_schedule" in times and "b_cosine" in times:
        res["b_over_a"] = round(statistics.median(times["b_cosine"]) / statistics.median(times["a_no_schedule"]), 4)
        lo, hi = min(times["a_no_schedule"]), max(times["a_no_schedule"])
        res["b_within_spread_of_a"] = bool(lo <= statistics.median(times["b_cosine"]) <= hi)
    for k, tr in trainers.items():
        res[k + "_last_lr"] = tr.last_lr()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20, help="steps per timed window")
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="no timing: N scheduled steps at batch 32 fp32 (for a "
                    "kernel trace)")
    a = ap.parse_args()
    cfg = FiraConfig()
    store = data.process_raw(cfg, synth.generate_dataset(256, seed=3))
    if a.profile:
        print(json.dumps(run_config(cfg, store, 32, "f32", 1, a.profile, only=("b_cosine",))))
        return
    for B, dtype in ((32, "f32"), (64, "bf16")):
        print(json.dumps(run_config(cfg, store, B, dtype, a.reps, a.inner)), flush=True)


if __name__ == "__main__":
    main()
