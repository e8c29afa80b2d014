"""Milliseconds per search step of ``Searcher.sample_distinct(n=8)`` (stochastic beam search: ``fira_beam_select_gumbel`` as the
selection) against ``beam(8, merge_copies=True)`` and ``sample(n=8)``, the number of distinct messages among 8 from ``sample``
and from ``sample_distinct``, and the option-off searches of this tree against another checkout (the parent commit) on the
same box.

    python scripts/sbs_probe.py [--batch 64] [--reps 7] [--parent DIR] [--out profiles/sbs_probe.md]

The scheme of scripts/beamscore_probe.py: synthetic commits (synth.py), the seeded initialisation with a sharpened generator, so
every search runs its tar_len - 1 steps and "per step" is the time of a whole call (graphs captured before, results ready after)
over that number.  Every measurement runs in a child process of its own (``--child``), one per tree, strictly one after the
other and interleaved (parent, this, parent, this, ...).  ``--parent DIR`` is a checkout of the parent commit with its library
built; a child of it runs ``beam`` and ``sample`` only.  Two warm-up calls per configuration are thrown away.  Medians, min and
max over the repetitions of all rounds."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def distinct(toks, lens, live=None):
    """Mean number of distinct id sequences among a commit's candidates."""
    toks, lens = toks.tolist(), lens.tolist()
    n = []
    for b in range(len(toks)):
        n.append(len({tuple(toks[b][j][:lens[b][j]]) for j in range(len(toks[b])) if live is None or live[b][j]}))
    return sum(n) / len(n)


def child(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from fira_icse_amd import data, decode, synth
    from fira_icse_amd.config import FiraConfig
    from fira_icse_amd.decode import Searcher
    from fira_icse_amd.model import DeviceBatch, TransModel
    assert os.path.abspath(decode.__file__).startswith(os.path.abspath(a.tree) + os.sep), decode.__file__
    B = a.batch
    cfg = FiraConfig()
    store = data.process_raw(cfg, synth.generate_dataset(B, seed=5))
    torch.manual_seed(0)
    model = TransModel(cfg)
    with torch.no_grad():
        sd = model.state_dict()
        sd["out_fc.weight"] = sd["out_fc.weight"] * 10.0
        model.load_state_dict(sd)
    model.eval()
    search = Searcher(model)
    db = DeviceBatch(store.batch(list(range(B))), cfg)
    seeds = iter(range(1000))
    configs = [("beam8 merge_copies", lambda: search.beam(db, 8, merge_copies=True)),
               ("sample n=8", lambda: search.sample(db, 8, seed=next(seeds)))]
    if a.sbs:
        configs.append(("sample_distinct n=8", lambda: search.sample_distinct(db, 8, seed=next(seeds))))
    res = {}
    for name, fn in configs:
        ts, dis = [], []
        for rep in range(a.reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if rep >= 2:
                ts.append(time.perf_counter() - t0)
                if name.startswith("sample_distinct"):
                    dis.append(distinct(out[0], out[1], (out[4] > float("-inf")).tolist()))
                elif name.startswith("sample"):
                    dis.append(distinct(out[0], out[1]))
        res[name] = dict(ms=[1e3 * t for t in ts], mean_len=float(out[1].float().mean()), distinct=dis)
    print("RESULT " + json.dumps(dict(tree=a.tree, device=torch.cuda.get_device_name(0), steps=cfg.tar_len - 1, res=res)), flush=True)


def run_child(tree, a, sbs):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--batch", str(a.batch), "--reps", str(a.reps)]
    if sbs:
        cmd.append("--sbs")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("child for %s failed (%d):\n%s" % (tree, r.returncode, (r.stdout + r.stderr)[-3000:]))
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2, help="interleaved (parent, this) rounds")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=None, help="append the result as markdown to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=REPO, help=argparse.SUPPRESS)
    ap.add_argument("--sbs", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    assert a.reps >= 3
    pooled, dis, info = {}, {}, {}
    for rnd in range(a.rounds):
        for side, tree in (("parent", a.parent), ("this", REPO)):
            if tree is None:
                continue
            r = run_child(tree, a, sbs=side == "this")
            info = r if side == "this" else info
            for k, v in r["res"].items():
                pooled.setdefault((side, k), []).extend(v["ms"])
                dis.setdefault((side, k), []).extend(v["distinct"])
    steps = info["steps"]
    med = {k: statistics.median(v) for k, v in pooled.items()}
    rows = ["| tree | search | median ms / call | min | max | median ms / step | distinct messages of 8 (mean) |",
            "|---|---|---|---|---|---|---|"]
    for side in ("parent", "this"):
        for name in ("beam8 merge_copies", "sample n=8", "sample_distinct n=8"):
            k = (side, name)
            if k in pooled:
                rows.append("| %s | %s | %.3f | %.3f | %.3f | %.4f | %s |" % (
                    "parent commit" if side == "parent" else "this tree", name, med[k], min(pooled[k]), max(pooled[k]),
                    med[k] / steps, "%.2f" % statistics.mean(dis[k]) if dis[k] else "-"))
    notes = []
    for name in ("beam8 merge_copies", "sample n=8"):
        if ("parent", name) in med:
            par, off = med[("parent", name)], med[("this", name)]
            spread = max(max(pooled[(s, name)]) - min(pooled[(s, name)]) for s in ("parent", "this"))
            notes.append("%s, this tree - parent commit = %+.3f ms per call (%+.2f %%); run-to-run spread (max - min of one "
                         "side) %.3f ms" % (name, off - par, 100.0 * (off - par) / par, spread))
    lens = ", ".join("%s: %.1f" % (k, v["mean_len"]) for k, v in sorted(info["res"].items()))
    out = "\n".join([
        "### B = %d commits, %d steps per call, %d rounds x %d repetitions after 2 warm-ups, %s" % (
            a.batch, steps, a.rounds, a.reps, info["device"]),
        "",
        "mean hypothesis length (this tree; %d means the search ran every step): %s" % (steps + 1, lens),
        "",
    ] + rows + [""] + ["- " + n for n in notes] + [""])
    print(out, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
