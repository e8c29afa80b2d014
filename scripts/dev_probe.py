"""Seconds per dev pass over a valid split: the host loop against the device pass, same process, interleaved.

    python scripts/dev_probe.py [--commits 8000] [--batch 170] [--reps 7] [--out profiles/dev_probe.md]

The valid set is synthetic (synth.py): `--distinct` commits are generated and preprocessed, then repeated up to `--commits`
(8 000 at batch 170 are the reference's valid split and batch).  The weights are the seeded initialisation, so the hypotheses
are what an untrained model writes: mostly full-length rows without <eos> -- the host loop's string work per commit is then at
its LONGEST; `--ids labels` scores injected label rows (20 % corrupted, about the length of real messages) instead, with
`forward_dev` still run and timed in both passes.  Per repetition, in this order: host_pass, device_pass (no text), device_pass
+ the text of dev_output (what a new best costs), and forward_dev alone over the resident batches.  The first device_pass, which
builds the resident set, is timed on its own.  Medians, min and max over the repetitions."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from fira_icse_amd import data, synth                      # noqa: E402
from fira_icse_amd.config import FiraConfig                 # noqa: E402
from fira_icse_amd.devset import DevEvaluator               # noqa: E402
from fira_icse_amd.model import TransModel                  # noqa: E402


def label_table(store, cfg, seed=0, corrupt=0.2):
    lab = np.asarray(store.tar_label)
    ids = np.concatenate([lab[:, 1:], np.zeros((lab.shape[0], 1), lab.dtype)], axis=1).astype(np.int32)
    rng = np.random.default_rng(seed)
    flat = ids.reshape(-1)
    where = rng.permutation(flat.size)[:int(round(corrupt * flat.size))]
    flat[where] = rng.integers(0, cfg.out_len, size=where.size)
    return ids


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commits", type=int, default=8000)
    ap.add_argument("--distinct", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=170)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ids", choices=["model", "labels"], default="model")
    ap.add_argument("--out", default=None, help="append the result as markdown to this file")
    a = ap.parse_args()
    assert a.reps >= 5
    cfg = FiraConfig(batch_size=a.batch)
    raw = synth.generate_dataset(min(a.distinct, a.commits), seed=5)
    full = data.process_raw(cfg, raw)
    which = [i % len(full) for i in range(a.commits)]
    store = data._subset(full, which)
    r_vocab = {i: w for w, i in raw["word_vocab"].items()}
    torch.manual_seed(0)
    model = TransModel(cfg)
    model.eval()
    ids_fn = None
    if a.ids == "labels":
        table = torch.from_numpy(label_table(store, cfg)).to(model.device_)

        def ids_fn(db):
            model.forward_dev(db)                            # run (and paid for) as in a real pass; its output is replaced
            return table[torch.as_tensor(db.commits, device=table.device)].contiguous()

    ev = DevEvaluator(model, store, cfg, r_vocab, raw["variable"], which, ids_fn=ids_fn)
    ev.host_pass()                                           # warm-up: code objects, workspaces, the pinned ring
    t_first, (d_total, _) = timed(ev.device_pass)

    def forward_only():
        for db in ev._batches:
            model.forward_dev(db)

    def device_with_text():
        total, lines = ev.device_pass()
        return total, "\n".join(lines()) + "\n"

    def host_with_text():
        total, lines = ev.host_pass()
        return total, "\n".join(lines()) + "\n"

    t = {"host": [], "device": [], "device_text": [], "forward": []}
    same = True
    for _ in range(a.reps):
        dt, (h_total, h_text) = timed(host_with_text)
        t["host"].append(dt)
        dt, (total, _) = timed(ev.device_pass)
        t["device"].append(dt)
        same &= total == h_total
        dt, (total, d_text) = timed(device_with_text)
        t["device_text"].append(dt)
        same &= total == h_total and d_text == h_text
        dt, _ = timed(forward_only)
        t["forward"].append(dt)
    med = {k: statistics.median(v) for k, v in t.items()}
    rows = ["| pass | median s | min s | max s |", "|---|---|---|---|"]
    names = (("host", "host_pass (always builds the text)"), ("device", "device_pass, no text"),
             ("device_text", "device_pass + dev_output text (a new best)"), ("forward", "forward_dev alone, resident batches"))
    for k, name in names:
        rows.append("| %s | %.4f | %.4f | %.4f |" % (name, med[k], min(t[k]), max(t[k])))
    n_batches = len(ev._batches)
    lines = [
        "### %d commits (%d distinct), batch %d (%d batches), ids: %s, %d repetitions, %s" % (
            a.commits, len(full), a.batch, n_batches, a.ids, a.reps, torch.cuda.get_device_name(0)),
        "",
        "mean BLEU %.6f; totals and dev_output text identical between the two passes in every repetition: %s" % (
            d_total / a.commits, same),
        "",
        "first device_pass (collates and uploads the resident set, %.1f MB): %.4f s" % (ev.resident_bytes / 1e6, t_first),
        "",
    ] + rows + [
        "",
        "host / device (no text): %.2fx; host / device + text: %.2fx; forward_dev share of the device pass: %.0f %%" % (
            med["host"] / med["device"], med["host"] / med["device_text"], 100.0 * med["forward"] / med["device"]),
        "",
    ]
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
