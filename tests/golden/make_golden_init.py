"""Generate init_ref.json by running THE REFERENCE ITSELF (its modules are imported, never copied):

    python tests/golden/make_golden_init.py <path of the reference tree>

Records what tests/test_oracle.py::test_init_and_position_table_match_live_reference compares against:
  keys / shapes / dtypes / sha256   the reference ``Model.TransModel(args)`` state dict under ``torch.manual_seed(0)``:
                                    every tensor's SHA-256 over its raw bytes (bit-identical initialisation)
  position_table_sha256             ``gnn_transformer.position_encoding(210, 256)``, same hash
  forward_valid3                    the reference's eval-mode forward (loss_sum, n_tok) on the first 3 validation commits
                                    of the golden synthetic DataSet with those freshly initialised weights
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from fira_icse_amd import data              # noqa: E402
from fira_icse_amd.config import FiraConfig  # noqa: E402
import util                                  # noqa: E402  (tests/util.py)


def tensor_sha256(t: torch.Tensor) -> str:
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


class Args(dict):
    __getattr__ = dict.__getitem__


def main(ref_root):
    sys.path.insert(0, ref_root)
    from Model import TransModel
    import gnn_transformer
    torch.set_num_threads(8)
    cfg = FiraConfig()
    args = Args(sou_len=cfg.sou_len, tar_len=cfg.tar_len, att_len=cfg.att_len, ast_change_len=cfg.ast_change_len,
                sub_token_len=cfg.sub_token_len, dropout_rate=cfg.dropout_rate, num_head=cfg.num_head,
                embedding_dim=cfg.embedding_dim, vocab_size=cfg.vocab_size, ast_change_vocab_size=cfg.ast_change_vocab_size)
    torch.manual_seed(0)
    ref = TransModel(args)
    rsd = ref.state_dict()
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = data.split_index(*util.GOLDEN_SPLIT, seed=0)
    tb = util.to_torch_batch(store.batch(idx["valid"][:3]), cfg)
    ref.eval()
    with torch.no_grad():
        ls, nt = ref(tb["sou"], tb["tar"], None, tb["mark"], tb["ast_change"], tb["edge"], tb["tar_label"],
                     tb["sub_token"], "train")
    out = {"keys": list(rsd.keys()),
           "shapes": {k: list(v.shape) for k, v in rsd.items()},
           "dtypes": {k: str(v.dtype) for k, v in rsd.items()},
           "sha256": {k: tensor_sha256(v) for k, v in rsd.items()},
           "position_table_sha256": tensor_sha256(gnn_transformer.position_encoding(210, 256)),
           "position_table_dtype": str(gnn_transformer.position_encoding(210, 256).dtype),
           "forward_valid3": {"loss_sum": float(ls), "n_tok": int(nt)}}
    with open(os.path.join(HERE, "init_ref.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("init_ref.json: %d tensors, loss_sum %.9g over %d tokens" % (len(rsd), float(ls), int(nt)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(os.path.abspath(sys.argv[1]))
