"""Generate sched_ref.json by running THE REFERENCE ITSELF under a learning-rate schedule (same set-up as make_golden.py:
the reference's modules are imported at run time, nothing is copied; build container only):

    python tests/golden/make_golden_sched.py

The golden batch (first 4 train commits, perturbed initialisation, dropout off), eight steps of

    loss.backward(); Adam.step(); LambdaLR.step()

with ``torch.optim.Adam(lr=BASE)`` and ``LambdaLR(lambda e: lr_formula(e + 1) / BASE)`` -- optimisation step t = 1, 2, ... runs
at ``lr_formula(t)``, the schedule definition of include/fira_hip.h written out here in Python (float64, rounded to float32
once), which also gives the recorded per-step ``lr``.  Two schedules: inv_sqrt with W = 4, and cosine with W = 2, N = 8,
min = 0.1 * BASE.  Each run records its 9-point loss curve (the loss ahead of each step and after the last); a constant-rate
run at BASE is recorded with them.

The script refuses to write the fixture unless
  * the same loop at the golden rate, constant, reproduces model_ref.npz's loss curve (this script IS the golden set-up);
  * each scheduled curve differs from the constant-rate curve at BASE by max |delta| / max(curve) >= 2e-3, ten times the
    tolerance the GPU test compares curves with -- otherwise that test could not tell a schedule from its absence;
  * every loss is finite and stays below the starting loss + 1.
"""
import json
import math
import os
import random
import sys
import tempfile

import numpy as np
import torch

from make_golden import HERE, Args, ref_args        # noqa: F401  (also puts the repository, tests/ and the reference on sys.path)

from fira_icse_amd import synth            # noqa: E402
from fira_icse_amd.config import FiraConfig  # noqa: E402
import util                                  # noqa: E402  (tests/util.py)

# the peak rate: halved from 1e-3 until the reference alone meets the three conditions above.  At 1e-3 and 5e-4 the
# constant-rate run's second loss climbs to 10.89 / 10.61 from 9.08, more than + 1; at 2.5e-4 every curve stays below and the
# schedules separate from the constant rate by 1.1e-1 (inv_sqrt) and 7.0e-2 (cosine).  (Another rate to try: first argument;
# another output file: second.)
BASE = float(sys.argv[1]) if len(sys.argv) > 1 else 2.5e-4
OUT = sys.argv[2] if len(sys.argv) > 2 else None
STEPS = 8
SCHEDULES = {
    "inv_sqrt": {"kind": "inv_sqrt", "base_lr": BASE, "warmup_steps": 4, "decay_steps": 0, "min_lr": 0.0},
    "cosine": {"kind": "cosine", "base_lr": BASE, "warmup_steps": 2, "decay_steps": 8, "min_lr": 0.1 * BASE},
}
MIN_SEPARATION = 2e-3


def lr_formula(s, t):
    """The rate of step t = 1, 2, ... under schedule dict ``s``: float64 arithmetic, rounded to float32 once."""
    base, mn = float(np.float32(s["base_lr"])), float(np.float32(s["min_lr"]))
    W, N = s["warmup_steps"], s["decay_steps"]
    w = min(1.0, t / W) if W > 0 else 1.0
    if s["kind"] == "constant":
        r = base * w
    elif s["kind"] == "inv_sqrt":
        r = base * min(t / W, math.sqrt(W / t))
    elif t <= W:
        r = base * w
    else:
        q = min(max((t - W) / (N - W), 0.0), 1.0)
        if s["kind"] == "cosine":
            r = mn + (base - mn) * 0.5 * (1.0 + math.cos(math.pi * q))
        else:
            r = mn + (base - mn) * (1.0 - q)
    return float(np.float32(r))


def run(TransModel, args, batch, base, sched, steps):
    torch.manual_seed(0)
    model = TransModel(args)
    sd = util.perturb_state_dict({k: v.clone() for k, v in model.state_dict().items()}, seed=1)
    model.load_state_dict(sd)
    model.eval()                                   # dropout off; the stage string selects the output
    opt = torch.optim.Adam(model.parameters(), base)
    lam = (lambda e: lr_formula(sched, e + 1) / base) if sched is not None else (lambda e: 1.0)
    lrs = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    curve = []
    for it in range(steps):
        loss_sum, n_tok = model(*batch, "train")
        loss = loss_sum / n_tok
        opt.zero_grad()
        loss.backward()
        opt.step()
        lrs.step()
        curve.append(loss.item())
    loss_sum, n_tok = model(*batch, "train")
    curve.append((loss_sum / n_tok).item())
    return curve


def main():
    torch.set_num_threads(8)
    cfg = FiraConfig()
    scratch = tempfile.mkdtemp(prefix="fira_golden_sched_")
    synth.write_dataset(scratch, synth.generate_dataset(util.GOLDEN_N, seed=0, overlong_every=6))
    os.chdir(scratch)
    import Dataset as RefDataset
    RefDataset.num_train, RefDataset.num_valid, RefDataset.num_test = util.GOLDEN_SPLIT
    random.seed(0)
    args = ref_args(cfg)
    train = RefDataset.TransDataset(args, "train")
    from Model import TransModel
    B = util.GOLDEN_B
    batch = [torch.from_numpy(np.stack([np.asarray(train[i][k]) for i in range(B)])) for k in range(8)]

    gold = util.golden_npz("model_ref.npz")
    check = run(TransModel, args, batch, args.lr, None, len(gold["loss_curve"]) - 1)
    assert np.allclose(check, gold["loss_curve"], rtol=1e-6), (check, gold["loss_curve"])

    const = run(TransModel, args, batch, BASE, None, STEPS)
    out = {"base_lr": BASE, "steps": STEPS, "golden_check_curve": check, "constant": {"loss_curve": const}, "runs": {}}
    for name, s in SCHEDULES.items():
        curve = run(TransModel, args, batch, BASE, s, STEPS)
        sep = max(abs(a - b) for a, b in zip(curve, const)) / max(curve)
        print(name, "separation from the constant-rate curve: %.3e" % sep, curve)
        assert sep >= MIN_SEPARATION, "%s: the curve is within %.1e of the constant-rate curve" % (name, sep)
        out["runs"][name] = {"schedule": s, "lr": [lr_formula(s, t) for t in range(1, STEPS + 1)], "loss_curve": curve,
                             "separation": sep}
    for curve in [const] + [r["loss_curve"] for r in out["runs"].values()]:
        assert all(math.isfinite(x) and x < curve[0] + 1.0 for x in curve), curve
    with open(OUT or os.path.join(HERE, "sched_ref.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("sched_ref.json written:", json.dumps(out))


if __name__ == "__main__":
    main()
