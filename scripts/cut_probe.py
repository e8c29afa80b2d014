"""ms per step of the replayed sampling loop (Searcher.sample) with each truncation cut against the cuts-off call, and every
row of this tree's library against another build of it (the parent commit's).

    python scripts/cut_probe.py [--reps 5] [--rounds 2] [--parent-lib PATH/libfira_hip.so] [--md profiles/cut_probe.md]

Every library is timed in a process of its own (FIRA_HIP_LIB), the two alternating over the rounds.  The loop runs all
tar_len - 1 steps (the captured graphs are timed directly, so the early stop does not shorten it): the time per step is
the chain's, whatever the samples emit.  Both libraries are timed on every row."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

B, N = 16, 4
BASE = dict(temperature=0.8, top_k=0, top_p=1.0)
CASES = [("off", {}), ("off_k50_p95", dict(top_k=50, top_p=0.95)), ("min_p_0.05", dict(min_p=0.05)),
         ("epsilon_0.02", dict(epsilon=0.02)), ("eta_0.003", dict(eta=0.003)), ("typical_0.9", dict(typical_p=0.9)),
         ("k50_p95_min_p_eps_eta", dict(top_k=50, top_p=0.95, min_p=0.05, epsilon=0.001, eta=0.003)),
         ("k50_typical_0.9", dict(top_k=50, typical_p=0.9))]
CUT_NAMES = ("min_p", "epsilon", "eta", "typical_p")


def worker(reps):
    import torch
    from fira_icse_amd import data, synth
    from fira_icse_amd.config import FiraConfig
    from fira_icse_amd.decode import Searcher
    from fira_icse_amd.model import DeviceBatch, TransModel
    cfg = FiraConfig()
    store = data.process_raw(cfg, synth.generate_dataset(B, seed=3))
    torch.manual_seed(0)
    model = TransModel(cfg)
    model.eval()
    search = Searcher(model)
    db = DeviceBatch(store.batch(list(range(B))), cfg, model.device_)
    steps = cfg.tar_len - 1
    res = {"device": torch.cuda.get_device_name(0)}
    for name, kw in CASES:
        kw = dict(BASE, **kw)
        search.sample(db, N, seed=1, **kw)
        key = ("sample", B, N, float(kw["temperature"]), int(kw["top_k"]), float(kw["top_p"]))
        if any(k in kw for k in CUT_NAMES):                  # the state key of a call with a cut on: the four values appended
            key += Searcher._check_cuts(kw["top_p"], kw.get("min_p", 0.0), kw.get("epsilon", 0.0), kw.get("eta", 0.0),
                                        kw.get("typical_p", 1.0))
        graphs = search._ws[key]["graphs"]
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
        res[name] = best / steps * 1e3
    print("RESULT " + json.dumps(res))


def run_worker(lib, reps):
    env = dict(os.environ)
    if lib:
        env["FIRA_HIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(reps)], env=env, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("worker failed (%d):\n%s" % (r.returncode, (r.stdout + r.stderr)[-3000:]))
    return json.loads([l for l in r.stdout.split("\n") if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.reps)
    runs = {"this tree": [], "parent commit": []}
    for _ in range(a.rounds):
        runs["this tree"].append(run_worker(None, a.reps))
        if a.parent_lib:
            runs["parent commit"].append(run_worker(os.path.abspath(a.parent_lib), a.reps))
    device = runs["this tree"][0]["device"]
    rows = []
    for tree, rs in runs.items():
        for name, _ in CASES:
            vals = [r[name] for r in rs if name in r]
            if vals:
                rows.append((tree, name, statistics.median(vals), min(vals), max(vals)))
    med = {(t, n): m for t, n, m, _, _ in rows}
    out = ["### B = %d commits x n = %d samples, temperature %.1f, %d rounds x %d repetitions (best of a round), %s"
           % (B, N, BASE["temperature"], a.rounds, a.reps, device), "",
           "| library | filters and cuts | median ms / step | min | max | against off (this tree) |", "|---|---|---|---|---|---|"]
    for t, n, m, lo, hi in rows:
        out.append("| %s | %s | %.4f | %.4f | %.4f | %+.4f |" % (t, n, m, lo, hi, m - med[("this tree", "off")]))
    for n, _ in CASES:
        if ("parent commit", n) in med:
            d = med[("this tree", n)] - med[("parent commit", n)]
            out.append("")
            out.append("- %s, this tree - parent commit = %+.4f ms per step (%+.2f %%)" % (n, d, 100 * d / med[("parent commit", n)]))
    text = "\n".join(out) + "\n"
    print(text)
    print(json.dumps({"%s/%s" % k: round(v, 4) for k, v in med.items()}))
    if a.md:
        with open(a.md, "a") as f:
            f.write("\n" + text)


if __name__ == "__main__":
    main()
