"""ms per step of the replayed decode loop at 64 rows: greedy against teacher-forced scoring (Searcher.score).

    python scripts/score_probe.py [--reps 9]

Both loops run all tar_len - 1 steps (the captured graphs are timed directly, alternating between the two), so the time
per step is the chain's, whatever the messages hold.  Medians over the repetitions; the minimum is reported too."""
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
from fira_icse_amd.decode import Searcher                   # noqa: E402
from fira_icse_amd.model import DeviceBatch, TransModel     # noqa: E402


def time_once(graphs):
    t0 = time.perf_counter()
    for g in graphs:
        g.replay()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20, help="replays of the whole loop per timed window")
    a = ap.parse_args()
    cfg = FiraConfig()
    store = data.process_raw(cfg, synth.generate_dataset(64, seed=3))
    torch.manual_seed(0)
    model = TransModel(cfg)
    model.eval()
    search = Searcher(model)
    steps = cfg.tar_len - 1
    loops = {}
    hb = store.batch(list(range(64)))
    db64 = DeviceBatch(hb, cfg, model.device_)
    search.greedy(db64)
    loops["greedy_B64"] = search._ws[("greedy", 64)]["graphs"]
    search.score(db64, hb.tar, labels=hb.tar_label)
    loops["score_B64_n1_labels"] = search._ws[("score", 64, 1, True)]["graphs"]
    search.score(db64, hb.tar)
    loops["score_B64_n1"] = search._ws[("score", 64, 1, False)]["graphs"]
    hb16 = store.batch(list(range(16)))
    search.score(DeviceBatch(hb16, cfg, model.device_), hb16.tar[:, None, :].repeat(4, 1))
    loops["score_B16_n4"] = search._ws[("score", 16, 4, False)]["graphs"]
    times = {k: [] for k in loops}
    for k, g in loops.items():                                  # warm-up
        time_once(g)
    for _ in range(a.reps):                                     # alternate the loops inside every repetition
        for k, g in loops.items():
            times[k].append(time_once(g * a.inner) / (steps * a.inner) * 1e3)
    res = {k + "_ms_per_step": round(statistics.median(v), 4) for k, v in times.items()}
    res.update({k + "_min": round(min(v), 4) for k, v in times.items()})
    res["ratio_score_vs_greedy"] = round(statistics.median(times["score_B64_n1"]) / statistics.median(times["greedy_B64"]), 4)
    res["ratio_score_labels_vs_greedy"] = round(statistics.median(times["score_B64_n1_labels"]) /
                                                statistics.median(times["greedy_B64"]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
