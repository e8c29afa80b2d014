"""ms per step of the replayed decode loop at 64 rows: greedy against on-device sampling (Searcher.sample).

    python scripts/sample_probe.py [--reps 5]

Peaked fixture-style weights are not needed: the loop runs all tar_len - 1 steps (the early stop is disabled by timing
the captured graphs directly), so the time per step is the chain's, whatever the samples emit."""
import argparse
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from fira_icse_amd import data, synth                      # noqa: E402
from fira_icse_amd.config import FiraConfig                 # noqa: E402
from fira_icse_amd.decode import Searcher                   # noqa: E402
from fira_icse_amd.model import DeviceBatch, TransModel     # noqa: E402


def time_graphs(graphs, reps):
    for g in graphs:
        g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        for g in graphs:
            g.replay()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    cfg = FiraConfig()
    store = data.process_raw(cfg, synth.generate_dataset(64, seed=3))
    torch.manual_seed(0)
    model = TransModel(cfg)
    model.eval()
    search = Searcher(model)
    steps = cfg.tar_len - 1
    res = {}
    db64 = DeviceBatch(store.batch(list(range(64))), cfg, model.device_)
    search.greedy(db64)
    res["greedy_B64"] = time_graphs(search._ws[("greedy", 64)]["graphs"], a.reps) / steps * 1e3
    for name, B, n, T, k, p in (("sample_B64_n1_T", 64, 1, 0.8, 0, 1.0), ("sample_B64_n1_T_k50_p95", 64, 1, 0.8, 50, 0.95),
                                ("sample_B16_n4_T_k50_p95", 16, 4, 0.8, 50, 0.95)):
        db = db64 if B == 64 else DeviceBatch(store.batch(list(range(B))), cfg, model.device_)
        search.sample(db, n, temperature=T, top_k=k, top_p=p, seed=1)
        res[name] = time_graphs(search._ws[("sample", B, n, float(T), int(k), float(p))]["graphs"], a.reps) / steps * 1e3
    res["ratio_filtered_vs_greedy"] = res["sample_B64_n1_T_k50_p95"] / res["greedy_B64"]
    print(json.dumps({k: round(v, 4) for k, v in res.items()}))


if __name__ == "__main__":
    main()
