"""ms per OPTIMIZER step and commits/s of Trainer.step_many against Trainer.step, same process, interleaved -- and the run-to-run
distance of the bf16 big-batch step against itself, the yardstick of tests/test_accum_gpu.py.

    python scripts/accum_probe.py [--dtype f32,bf16] [--reps 5] [--inner 8] [--forms 128x1,64x2,32x4,170x4]
    python scripts/accum_probe.py --noise [--runs 4]

A form BxK is one optimizer step over K micro-batches of B commits (K = 1: Trainer.step, the option-off path).  For every form
with K > 1 the probe also times K PLAIN steps of B commits -- the same passes with K updates instead of one: the difference
is what the K - 1 saved Adam passes over the live parameters and moments are worth.  A timed window is `inner` optimizer steps
on rotating batches, dropout on, ended by a device synchronise; the forms take turns inside every repetition so that clocks
drift over all alike; medians and min / max over the repetitions are printed, one JSON line per form.

--noise: three steps of the 4-commit golden batch in bf16 (and fp32), `runs` fresh models; the largest relative L2 distance of
params / m / v between any two runs after each step."""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def parse_forms(text):
    forms = []
    for f in text.split(","):
        b, k = f.lower().split("x")
        forms.append((int(b), int(k)))
    return forms


def timing(a):
    import torch
    from fira_icse_amd import data, synth
    from fira_icse_amd.config import FiraConfig
    from fira_icse_amd.model import DeviceBatch, TransModel
    from fira_icse_amd.train import Trainer
    cfg = FiraConfig()
    forms = parse_forms(a.forms)
    n_commits = max(b * k for b, k in forms) * 2
    store = data.process_raw(cfg, synth.generate_dataset(n_commits, seed=3))
    for dtype in a.dtype.split(","):
        torch.manual_seed(0)
        model = TransModel(cfg)
        model.compute_dtype = dtype
        model.train()
        model.set_dropout_stream(3, 0)
        tr = Trainer(model)
        runs = {}
        for b, k in forms:
            # two rotating global batches per form, cut into K micro-batches of B commits in order
            glob = [[DeviceBatch(store.batch(list(range(g * b * k + i * b, g * b * k + i * b + b))), cfg, model.device_)
                     for i in range(k)] for g in range(2)]
            if k == 1:
                runs["%dx1" % b] = (b, 1, lambda i, glob=glob: tr.step(glob[i % 2][0]))
            else:
                runs["%dx%d" % (b, k)] = (b, k, lambda i, glob=glob: tr.step_many(glob[i % 2]))
                runs["%dx%d plain steps" % (b, k)] = (b, k, lambda i, glob=glob: [tr.step(db) for db in glob[i % 2]])
        times = {name: [] for name in runs}
        for name, (b, k, fn) in runs.items():                    # warm-up: every shape, every workspace
            fn(0); fn(1)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for name, (b, k, fn) in runs.items():
                t0 = time.perf_counter()
                for i in range(a.inner):
                    fn(i)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / a.inner * 1e3)
        for name, (b, k, fn) in runs.items():
            med = statistics.median(times[name])
            print(json.dumps({"dtype": dtype, "form": name, "global_batch": b * k, "ms_per_optimizer_step": round(med, 3),
                              "min": round(min(times[name]), 3), "max": round(max(times[name]), 3),
                              "commits_per_s": round(b * k / med * 1e3, 1)}), flush=True)
        del tr, model, runs
        torch.cuda.empty_cache()


def noise(a):
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import util
    from fira_icse_amd import data
    from fira_icse_amd.config import FiraConfig
    from fira_icse_amd.model import DeviceBatch, TransModel, reference_init_state_dict
    from fira_icse_amd.train import Trainer
    cfg = FiraConfig()
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = list(data.split_index(*util.GOLDEN_SPLIT, seed=0)["train"][:util.GOLDEN_B])
    torch.manual_seed(0)
    sd = util.perturb_state_dict(reference_init_state_dict(cfg), seed=1)
    for dtype in ("bf16", "f32"):
        snaps = []
        for _ in range(a.runs):
            model = TransModel(cfg, init=False)
            model.load_state_dict(sd)
            model.compute_dtype = dtype
            model.eval()
            db = DeviceBatch(store.batch(idx), cfg)
            tr = Trainer(model)
            per = []
            for _ in range(3):
                tr.step(db)
                tr.sync()
                live = model.layout.live
                per.append((model.flat.data[:live].clone(), tr.m[:live].clone(), tr.v[:live].clone()))
            snaps.append(per)
        worst = {"params": 0.0, "m": 0.0, "v": 0.0}
        for x, y in itertools.combinations(snaps, 2):
            for step in range(3):
                for k, key in enumerate(worst):
                    d = float((x[step][k].double() - y[step][k].double()).norm() / y[step][k].double().norm())
                    worst[key] = max(worst[key], d)
        print(json.dumps({"dtype": dtype, "runs": a.runs, "self_distance_max": worst}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtype", default="f32,bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--forms", default="128x1,64x2,32x4,170x4")
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--runs", type=int, default=4)
    a = ap.parse_args()
    noise(a) if a.noise else timing(a)


if __name__ == "__main__":
    main()
