"""Two steps of every form of the training call ("Step forms") in one process: fp32, the golden batch, no dropout.

    python scripts/step_forms_probe.py [--steps 2] [--only NAME]
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/step_forms_probe.py
    python scripts/step_forms_probe.py --count OUT [--markdown]

The first form drives the ten training entries of include/fira_hip.h through TransModel's train_* methods, row by row of the
table: fwd_bwd, step (dense / rows / clipped dense / clipped rows), accum_micro + accum_last (dense, rows, clipped), and the
two-call forms -- begin / end back to back on one device, with a recorded event standing in for the collective's (own token
counter, a count, by rows, and end with adam = NULL).  One JSON line per form with the loss of its last step.

--count reads the kernel trace(s) under OUT and prints the number of launches per (kernel name, grid, workgroup size), sorted:
the table two builds of the library are compared by (order across concurrent streams is not stable in a trace; counts are)."""
import argparse
import collections
import csv
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def run(a):
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import util
    from fira_icse_amd import data, ops
    from fira_icse_amd.config import FiraConfig
    from fira_icse_amd.model import DeviceBatch, TransModel, reference_init_state_dict
    cfg = FiraConfig()
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = list(data.split_index(*util.GOLDEN_SPLIT, seed=0)["train"][:util.GOLDEN_B])
    torch.manual_seed(0)
    sd = util.perturb_state_dict(reference_init_state_dict(cfg), seed=1)
    model = TransModel(cfg, init=False)
    model.eval()                                                  # dropout off
    dev = model.gbuf.device
    db = DeviceBatch(store.batch(idx), cfg)
    half = [DeviceBatch(store.batch(idx[:len(idx) // 2]), cfg), DeviceBatch(store.batch(idx[len(idx) // 2:]), cfg)]
    lr = 1e-3
    st = {}

    def fresh():
        """The same start for every form: weights, zero moments, zero row stamps, a clean clip state."""
        model.load_state_dict(sd)
        model.sync_params()
        st["m"], st["v"] = torch.zeros_like(model.flat.data), torch.zeros_like(model.flat.data)
        st["rows"] = torch.zeros(2 * cfg.vocab_size, dtype=torch.int32, device=dev)
        st["clip"] = (1.0,) + tuple(ops.clip_state(dev))
        st["stats"] = torch.zeros(2, dtype=torch.float32, device=dev)
        st["total"] = torch.zeros(1, dtype=torch.int32, device=dev)
        st["mid"], st["early"] = torch.cuda.Event(), torch.cuda.Event()
        st["mid"].record(); st["early"].record()

    def rows_tuple(t):
        return (st["m"], st["v"], lr, t, 0.9, 0.999, 1e-8, st["rows"])

    def accum(t, rows, clip):
        a, b = half
        model.train_accum_micro(a, True, rows=rows_tuple(t) if rows else None)
        ops.accum_stats(model.loss_sum, model.n_tok, st["stats"], st["total"], True)
        return model.train_accum_last(b, st["m"], st["v"], lr, t, st["stats"], st["total"], row_step=st["rows"] if rows else None,
                                      clip=st["clip"] if clip else None)

    def two_call(t, rows, count, update=True):
        out = model.train_step_begin(db, st["mid"], rows=rows_tuple(t) if rows else None)
        st["early"].record()                                      # where the collective of [0, split) would end
        if count:
            ops.pack_stats(model.loss_sum, model.n_tok, st["stats"])
        model.train_step_end(st["m"], st["v"], lr, t, early_event=st["early"], count=st["stats"][1:2] if count else None,
                             row_step=st["rows"] if rows else None, update=update)
        return out

    forms = [
        ("fwd_bwd", lambda t: model.train_fwd_bwd(db)),
        ("fwd_bwd mid_event", lambda t: model.train_fwd_bwd(db, mid_event=st["mid"])),
        ("step", lambda t: model.train_step(db, st["m"], st["v"], lr, t)),
        ("step_rows", lambda t: model.train_step(db, st["m"], st["v"], lr, t, row_step=st["rows"])),
        ("step_clip dense", lambda t: model.train_step(db, st["m"], st["v"], lr, t, clip=st["clip"])),
        ("step_clip rows", lambda t: model.train_step(db, st["m"], st["v"], lr, t, row_step=st["rows"], clip=st["clip"])),
        ("accum dense", lambda t: accum(t, False, False)),
        ("accum rows", lambda t: accum(t, True, False)),
        ("accum dense clipped", lambda t: accum(t, False, True)),
        ("accum rows clipped", lambda t: accum(t, True, True)),
        ("begin/end own n_tok", lambda t: two_call(t, False, False)),
        ("begin/end count", lambda t: two_call(t, False, True)),
        ("begin_rows/end_rows count", lambda t: two_call(t, True, True)),
        ("begin/end adam NULL", lambda t: two_call(t, False, False, update=False)),
    ]
    for name, fn in forms:
        if a.only and a.only != name:
            continue
        fresh()
        for t in range(1, a.steps + 1):
            loss_sum, n_tok = fn(t)
        torch.cuda.synchronize()
        print(json.dumps({"form": name, "steps": a.steps, "loss": float(loss_sum.item()) / max(int(n_tok.item()), 1)}), flush=True)


def count(a):
    tally = collections.Counter()
    for path in glob.glob(os.path.join(a.count, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                grid = "x".join(r.get(k, "1") for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
                wg = "x".join(r.get(k, "1") for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z"))
                tally[(r["Kernel_Name"], grid, wg)] += 1
    if not tally:
        sys.exit("no *kernel_trace.csv under %s" % a.count)
    if a.markdown:
        print("| kernel | grid | workgroup | launches |\n|---|---|---|---|")
    for (name, grid, wg), n in sorted(tally.items()):
        print(("| `%s` | %s | %s | %d |" if a.markdown else "%s\t%s\t%s\t%d") % (name, grid, wg, n))
    print(("\n%d launches, %d distinct (kernel, grid, workgroup)" % (sum(tally.values()), len(tally))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--only", default=None)
    ap.add_argument("--count", default=None, metavar="DIR")
    ap.add_argument("--markdown", action="store_true")
    a = ap.parse_args()
    count(a) if a.count else run(a)


if __name__ == "__main__":
    main()
