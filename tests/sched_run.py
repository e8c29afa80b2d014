"""Child process of tests/test_lr_schedule_gpu.py: the golden batch through Trainer(lr_schedule=...) for the two schedules of
tests/golden/sched_ref.json -- the fused one-call path and the fwd_bwd + separate update path in fp32, the fused path in
bf16 -- under whatever FIRA_ADAM_ROWS the parent set (the switch is read once per process).  Writes
{"rows": bool, "<schedule>/<dtype>/<path>": {"lr": [8], "curve": [9]}} as JSON.

    python tests/sched_run.py OUT.json
"""
import json
import os
import sys

import torch

import util
from fira_icse_amd import data
from fira_icse_amd.config import FiraConfig


def main(out_path):
    from fira_icse_amd.model import DeviceBatch, TransModel, reference_init_state_dict
    from fira_icse_amd.train import Trainer
    with open(os.path.join(util.GOLDEN, "sched_ref.json")) as f:
        ref = json.load(f)
    cfg = FiraConfig()
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = data.split_index(*util.GOLDEN_SPLIT, seed=0)
    hb = store.batch(idx["train"][:util.GOLDEN_B])
    torch.manual_seed(0)
    sd = util.perturb_state_dict(reference_init_state_dict(cfg), seed=1)
    model = TransModel(cfg, init=False)
    db = DeviceBatch(hb, cfg)
    out = {}
    for name, run in ref["runs"].items():
        for dtype, fused in (("f32", True), ("f32", False), ("bf16", True)):
            model.load_state_dict(sd)
            model.eval()
            model.compute_dtype = dtype
            tr = Trainer(model, lr_schedule=run["schedule"])
            out["rows"] = tr.row_step is not None
            tr.fused_step = fused
            lrs, curve = [], []
            for _ in range(ref["steps"]):
                tr.step(db)
                lrs.append(tr.last_lr())
                curve.append(tr.last_loss())
            model.sync_params()
            loss, ntok = model.train_fwd_bwd(db)
            curve.append(float(loss) / float(ntok))
            out["%s/%s/%s" % (name, dtype, "fused" if fused else "two_call")] = {"lr": lrs, "curve": curve}
            model.compute_dtype = "f32"
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1])
