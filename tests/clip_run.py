"""Child process of tests/test_clip_gpu.py: the golden batch through Trainer(clip_grad_norm=1.0) -- the fused one-call path and
the fwd_bwd + separate update path in fp32, the fused path in bf16 -- under whatever FIRA_ADAM_ROWS the parent set (the switch
is read once per process).  Writes {"rows": bool, "<dtype>/<path>": {"norm": [3], "coef": [3], "curve": [4]}} as JSON.

    python tests/clip_run.py OUT.json
"""
import json
import sys

import torch

import util
from fira_icse_amd import data
from fira_icse_amd.config import FiraConfig


def main(out_path):
    from fira_icse_amd.model import DeviceBatch, TransModel, reference_init_state_dict
    from fira_icse_amd.train import Trainer
    cfg = FiraConfig()
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = data.split_index(*util.GOLDEN_SPLIT, seed=0)
    hb = store.batch(idx["train"][:util.GOLDEN_B])
    torch.manual_seed(0)
    sd = util.perturb_state_dict(reference_init_state_dict(cfg), seed=1)
    model = TransModel(cfg, init=False)
    db = DeviceBatch(hb, cfg)
    out = {}
    for dtype, fused in (("f32", True), ("f32", False), ("bf16", True)):
        model.load_state_dict(sd)
        model.eval()
        model.compute_dtype = dtype
        tr = Trainer(model, clip_grad_norm=1.0)
        out["rows"] = tr.row_step is not None
        tr.fused_step = fused
        norm, coef, curve = [], [], []
        for _ in range(3):
            tr.step(db)
            g = tr.last_grad_norm()
            norm.append(g[0]); coef.append(g[1])
            curve.append(tr.last_loss())
        assert tr.last_grad_norm()[2:] == (3, 0)
        model.sync_params()
        loss, ntok = model.train_fwd_bwd(db)
        curve.append(float(loss) / float(ntok))
        out["%s/%s" % (dtype, "fused" if fused else "two_call")] = {"norm": norm, "coef": coef, "curve": curve}
        model.compute_dtype = "f32"
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1])
