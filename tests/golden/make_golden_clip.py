"""Generate clip_ref.json by running THE REFERENCE ITSELF with gradient clipping (same set-up as make_golden.py: the
reference's modules are imported at run time, nothing is copied; build container only):

    python tests/golden/make_golden_clip.py

The golden batch (first 4 train commits, perturbed initialisation, dropout off), three steps of

    loss.backward(); torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0); Adam.step()

recording per step the pre-clip global gradient norm twice -- ``norm`` as clip_grad_norm_ returns it (fp32) and ``norm64`` =
sqrt(sum p.grad.double()^2) -- and the 4-point loss curve.  The two norms differ by the fp32 summation error of torch's own
reduction (3.8e-5 relative at step 1), so implementations are compared with ``norm64``; ``norm`` is kept to show the gap.
As a check that this script IS the golden set-up, the same loop with max_norm = 100 (which never binds) must reproduce
model_ref.npz's loss curve; the script refuses to write the fixture otherwise.
"""
import json
import os
import random
import tempfile

import numpy as np
import torch

from make_golden import HERE, Args, ref_args        # noqa: F401  (also puts the repository, tests/ and the reference on sys.path)

from fira_icse_amd import synth            # noqa: E402
from fira_icse_amd.config import FiraConfig  # noqa: E402
import util                                  # noqa: E402  (tests/util.py)

MAX_NORM = 1.0


def run(TransModel, args, batch, max_norm):
    torch.manual_seed(0)
    model = TransModel(args)
    sd = util.perturb_state_dict({k: v.clone() for k, v in model.state_dict().items()}, seed=1)
    model.load_state_dict(sd)
    model.eval()                                   # dropout off; the stage string selects the output
    opt = torch.optim.Adam(model.parameters(), args.lr)
    curve, norms, norms64 = [], [], []
    for it in range(3):
        loss_sum, n_tok = model(*batch, "train")
        loss = loss_sum / n_tok
        opt.zero_grad()
        loss.backward()
        norms64.append(float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.grad is not None))))
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)))
        opt.step()
        curve.append(loss.item())
    loss_sum, n_tok = model(*batch, "train")
    curve.append((loss_sum / n_tok).item())
    return curve, norms, norms64


def main():
    torch.set_num_threads(8)
    cfg = FiraConfig()
    scratch = tempfile.mkdtemp(prefix="fira_golden_clip_")
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

    curve100, _, n64 = run(TransModel, args, batch, 100.0)
    gold = util.golden_npz("model_ref.npz")
    assert np.allclose(curve100, gold["loss_curve"], rtol=1e-6), (curve100, gold["loss_curve"])
    g64 = float(np.sqrt((gold["grad_norm"][gold["grad_norm"] > 0] ** 2).sum()))
    assert abs(n64[0] - g64) <= 1e-6 * g64, (n64[0], g64)

    curve, norms, norms64 = run(TransModel, args, batch, MAX_NORM)
    out = {"max_norm": MAX_NORM, "norm": norms, "norm64": norms64, "loss_curve": curve, "unclipped_check_curve": curve100}
    with open(os.path.join(HERE, "clip_ref.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("clip_ref.json written:", json.dumps(out))


if __name__ == "__main__":
    main()
