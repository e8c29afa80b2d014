"""Milliseconds per search step of beam search with and without ``scoring`` (length-normalised ranking, diverse beam groups:
``fira_beam_select_scored`` in place of ``fira_beam_select``), and the option-off search of this tree against another checkout (the
parent commit) on the same box.

    python scripts/beamscore_probe.py [--batch 64] [--reps 7] [--parent DIR] [--out profiles/beamscore_probe.md]

The scheme of scripts/constrain_probe.py: the commits are synthetic (synth.py) and the weights the seeded initialisation with a
sharpened generator, so every search runs its tar_len - 1 steps and "per step" is the time of a whole ``Searcher.beam`` /
call (graphs captured before, results ready after) over that number.  Every measurement runs in a child
process of its own (``--child``), one per tree, strictly one after the other and interleaved (parent, this, parent, this, ...):
the pair is then exposed to the same drift of the box.  ``--parent DIR`` is a checkout of the parent commit with its library
built; a child imports ``fira_icse_amd`` from its tree and never passes ``scoring`` there.  Two warm-up calls per
configuration are thrown away.  Medians, min and max over the repetitions of all rounds."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


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
    configs = [("off", {})]
    if a.scored:
        from fira_icse_amd.decode import BeamScoring
        configs += [("inactive", dict(scoring=BeamScoring())), ("alpha", dict(scoring=BeamScoring(length_alpha=1.0))),
                    ("groups", dict(scoring=BeamScoring(length_alpha=1.0, groups=2, diversity=0.5)))]
    res = {}
    for name, kw in configs:
        for kind, fn in (("beam4", lambda: search.beam(db, 4, **kw)), ("beam8", lambda: search.beam(db, 8, **kw))):
            ts = []
            for rep in range(a.reps + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                if rep >= 2:
                    ts.append(time.perf_counter() - t0)
            length = out[1].float()
            res["%s/%s" % (kind, name)] = dict(ms=[1e3 * t for t in ts], mean_len=float(length.mean()), max_len=int(length.max()))
    print("RESULT " + json.dumps(dict(tree=a.tree, device=torch.cuda.get_device_name(0), steps=cfg.tar_len - 1, res=res)), flush=True)


def run_child(tree, a, scored):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--batch", str(a.batch), "--reps", str(a.reps)]
    if scored:
        cmd.append("--scored")
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
    ap.add_argument("--scored", action="store_true", help=argparse.SUPPRESS)
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
            r = run_child(tree, a, scored=side == "this")
            info = r if side == "this" else info
            for k, v in r["res"].items():
                pooled.setdefault((side, k), []).extend(v["ms"])
    steps = info["steps"]
    med = {k: statistics.median(v) for k, v in pooled.items()}
    rows = ["| search | configuration | median ms / call | min | max | median ms / step |", "|---|---|---|---|---|---|"]
    label = {"off": "no `scoring` argument", "inactive": "`scoring=BeamScoring()`", "alpha": "`BeamScoring(length_alpha=1)`",
             "groups": "`BeamScoring(1, groups=2, diversity=0.5)`"}
    for kind in ("beam4", "beam8"):
        for side in ("parent", "this"):
            for name in ("off", "inactive", "alpha", "groups"):
                k = (side, "%s/%s" % (kind, name))
                if k in pooled:
                    rows.append("| %s | %s, %s | %.3f | %.3f | %.3f | %.4f |" % (
                        kind, "parent commit" if side == "parent" else "this tree", label[name], med[k], min(pooled[k]),
                        max(pooled[k]), med[k] / steps))
    lens = ", ".join("%s: mean %.1f / max %d" % (k, v["mean_len"], v["max_len"]) for k, v in sorted(info["res"].items()))
    notes = []
    for kind in ("beam4", "beam8"):
        off = med[("this", kind + "/off")]
        for name in ("alpha", "groups"):
            on = med[("this", "%s/%s" % (kind, name))]
            notes.append("%s: %s against fira_beam_select = %+.4f ms per step (%+.2f %%)" % (kind, label[name], (on - off) / steps,
                                                                                           100.0 * (on - off) / off))
        if ("parent", kind + "/off") in med:
            par = med[("parent", kind + "/off")]
            spread = max(max(pooled[(s, kind + "/off")]) - min(pooled[(s, kind + "/off")]) for s in ("parent", "this"))
            notes.append("%s: option off, this tree - parent commit = %+.3f ms per call (%+.2f %%); run-to-run spread "
                         "(max - min of one side) %.3f ms" % (kind, off - par, 100.0 * (off - par) / par, spread))
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
