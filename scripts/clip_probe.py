"""ms per training step with and without clipping by the global gradient norm, same process, interleaved.

    python scripts/clip_probe.py [--reps 9] [--inner 20]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/clip_probe.py --profile 10      (kernel rows of a clipped run)

Per configuration (batch 32 and 64 in fp32, batch 64 in bf16) three trainers on three replicas of one model take turns inside
every repetition: (a) Trainer(model) -- the unclipped step, (b) clip_grad_norm=inf (the norm is computed, the threshold never
binds), (c) clip_grad_norm=1.0.  A timed window is `inner` steps on four rotating batches, dropout on, ended by a device
synchronise; medians over the repetitions.  The spread of (a) against itself (min / max over its own repetitions) is the
margin inside which a difference means nothing.  Reading the norm back (Trainer.last_grad_norm) synchronises and stays out of
the timed windows."""
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

KINDS = (("a_unclipped", None), ("b_clip_inf", float("inf")), ("c_clip_1", 1.0))


def window(tr, batches, inner):
    t0 = time.perf_counter()
    for i in range(inner):
        tr.step(batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e3


def run_config(cfg, store, B, dtype, reps, inner, only=None):
    trainers = {}
    batches = None
    for name, clip in KINDS:
        if only and name not in only:
            continue
        torch.manual_seed(0)
        model = TransModel(cfg)
        model.compute_dtype = dtype
        model.train()
        model.set_dropout_stream(3, 0)
        if batches is None:
            batches = [DeviceBatch(store.batch(list(range(B * i, B * i + B))), cfg, model.device_) for i in range(4)]
        trainers[name] = Trainer(model, clip_grad_norm=clip)
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
    if "a_unclipped" in times:
        a = statistics.median(times["a_unclipped"])
        for k in times:
            if k != "a_unclipped":
                res[k + "_over_a"] = round(statistics.median(times[k]) / a, 4)
    for k, tr in trainers.items():
        if tr.clip is not None:
            res[k + "_last"] = [round(float(x), 5) for x in tr.last_grad_norm()]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20, help="steps per timed window")
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="no timing: N clipped steps at batch 32 fp32 (for a "
                    "kernel trace)")
    a = ap.parse_args()
    cfg = FiraConfig()
    store = data.process_raw(cfg, synth.generate_dataset(256, seed=3))
    if a.profile:
        print(json.dumps(run_config(cfg, store, 32, "f32", 1, a.profile, only=("c_clip_1",))))
        return
    for B, dtype in ((32, "f32"), (64, "f32"), (64, "bf16")):
        print(json.dumps(run_config(cfg, store, B, dtype, a.reps, a.inner)), flush=True)


if __name__ == "__main__":
    main()
