"""Milliseconds per search step of beam-3 and greedy search under an ensemble of M = 1, 2, 4 models (``Searcher(model,
members=...)``), and the single-model search of this tree against another checkout (the parent commit) on the same box.

    python scripts/ensemble_probe.py [--batch 64] [--reps 7] [--parent DIR] [--out profiles/ensemble_probe.md]

The scheme of scripts/merge_probe.py: the commits are synthetic (synth.py) and the weights seeded initialisations with a
sharpened generator (one torch seed per member), so every search runs its tar_len - 1 steps and "per step" is the time of a whole
``Searcher.beam`` / ``Searcher.greedy`` call (graphs captured before, results ready after) over that number.  Every measurement
runs in a child process of its own (``--child``) under a time limit, one per tree, strictly one after the other and interleaved
(parent, this, parent, this, ...): the pair is then exposed to the same drift of the box.  ``--parent DIR`` is a checkout of the
parent commit with its library built; a child imports ``fira_icse_amd`` from its tree and never passes ``members`` there.  Two
warm-up calls per configuration are thrown away.  Medians, min and max over the repetitions of all rounds.

What to read off: M members cost about M single-model steps plus one fira_mix_dist launch per step, which moves
(M + 1) * R * out_len * 4 bytes (R = batch x beam rows); the single-model pair (this tree, parent commit) must agree within the
run-to-run spread the table reports."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
MEMBERS = (1, 2, 4)
CHILD_TIMEOUT_S = 600


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

    def make(seed):
        torch.manual_seed(seed)
        model = TransModel(cfg)
        with torch.no_grad():
            sd = model.state_dict()
            sd["out_fc.weight"] = sd["out_fc.weight"] * 10.0
            model.load_state_dict(sd)
        model.eval()
        return model
    counts = MEMBERS if a.ensemble else (1,)
    models = [make(seed) for seed in range(max(counts))]
    db = DeviceBatch(store.batch(list(range(B))), cfg)
    res = {}
    for M in counts:
        search = Searcher(models[0]) if M == 1 else Searcher(models[0], members=models[1:M])
        for kind, fn in (("beam3", lambda: search.beam(db, 3)), ("greedy", lambda: search.greedy(db))):
            ts = []
            for rep in range(a.reps + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                if rep >= 2:
                    ts.append(time.perf_counter() - t0)
            length = out[1].float()
            res["%s/M%d" % (kind, M)] = dict(ms=[1e3 * t for t in ts], mean_len=float(length.mean()), max_len=int(length.max()))
        del search
    print("RESULT " + json.dumps(dict(tree=a.tree, device=torch.cuda.get_device_name(0), steps=cfg.tar_len - 1,
                                      out_len=cfg.out_len, res=res)), flush=True)


def run_child(tree, a, ensemble):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--batch", str(a.batch), "--reps", str(a.reps)]
    if ensemble:
        cmd.append("--ensemble")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    if r.returncode != 0:                                    # (a fault, an abort or a failure: nothing more is started)
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
    ap.add_argument("--ensemble", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    assert a.reps >= 3
    pooled = {}                                              # (side, key) -> all ms
    info = {}
    for rnd in range(a.rounds):
        for side, tree in (("parent", a.parent), ("this", REPO)):
            if tree is None:
                continue
            r = run_child(tree, a, ensemble=side == "this")
            info = r if side == "this" else info
            for k, v in r["res"].items():
                pooled.setdefault((side, k), []).extend(v["ms"])
    steps = info["steps"]
    med = {k: statistics.median(v) for k, v in pooled.items()}
    rows = ["| search | configuration | median ms / call | min | max | median ms / step | x single model |", "|---|---|---|---|---|---|---|"]
    for kind in ("beam3", "greedy"):
        for side in ("parent", "this"):
            for M in MEMBERS:
                k = (side, "%s/M%d" % (kind, M))
                if k in pooled:
                    what = "no `members` argument" if M == 1 else "%d models" % M
                    rows.append("| %s | %s, %s | %.3f | %.3f | %.3f | %.4f | %.2f |" % (
                        kind, "parent commit" if side == "parent" else "this tree", what, med[k], min(pooled[k]), max(pooled[k]),
                        med[k] / steps, med[k] / med[(side, kind + "/M1")]))
    lens = ", ".join("%s: mean %.1f / max %d" % (k, v["mean_len"], v["max_len"]) for k, v in sorted(info["res"].items()))
    notes = []
    for kind, rows_per_commit in (("beam3", 3), ("greedy", 1)):
        one = med[("this", kind + "/M1")]
        for M in MEMBERS[1:]:
            m = med[("this", "%s/M%d" % (kind, M))]
            mib = (M + 1) * a.batch * rows_per_commit * info["out_len"] * 4 / 2.0 ** 20
            notes.append("%s: %d models - %d x single model = %+.4f ms per step (the mix launch moves %.1f MiB per step)"
                         % (kind, M, M, (m - M * one) / steps, mib))
        if ("parent", kind + "/M1") in med:
            par = med[("parent", kind + "/M1")]
            spread = max(max(pooled[(s, kind + "/M1")]) - min(pooled[(s, kind + "/M1")]) for s in ("parent", "this"))
            notes.append("%s: single model, this tree - parent commit = %+.3f ms per call (%+.2f %%); run-to-run spread "
                         "(max - min of one side) %.3f ms" % (kind, one - par, 100.0 * (one - par) / par, spread))
    out = "\n".join([
        "### B = %d commits, %d steps per call, %d rounds x %d repetitions after 2 warm-ups, %s" % (
            a.batch, steps, a.rounds, a.reps, info["device"]),
        "",
        "hypothesis lengths (this tree; tar_len = %d means the search ran every step): %s" % (steps + 1, lens),
        "",
    ] + rows + [""] + ["- " + n for n in notes] + [""])
    print(out, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
