"""The contract between the host list builders and embed_grouped_bwd_kernel: no item of model.embedding_items or of
fira_host_node_lists holds more than 32 rows (the kernel silently caps an item at 64) and the items of one word are adjacent
(a word with a single item is written without atomics: a second, non-adjacent item would race with it).  On the id arrays
of tests/test_tail_gpu.py: words occurring 1, 31, 32, 33, 64, 65 and 1000 times (no GPU needed)."""
import os

import numpy as np
import pytest

import util  # noqa: F401
import tail_ref as R
from fira_icse_amd import model as M
from fira_icse_amd.config import FiraConfig


def check_items(tok, ptr, n_rows, counts):
    tok, ptr = np.asarray(tok), np.asarray(ptr)
    assert ptr[0] == 0 and ptr[-1] == n_rows == sum(counts.values()) and len(ptr) == len(tok) + 1
    size = np.diff(ptr)
    assert size.min() >= 1 and size.max() <= 32
    starts = np.flatnonzero(np.concatenate([[True], tok[1:] != tok[:-1]]))
    assert len(set(tok[starts].tolist())) == len(starts), "the items of one word are not adjacent"
    assert 0 not in tok
    for w, n in counts.items():
        sel = tok == w
        assert int(size[sel].sum()) == n and int(sel.sum()) == (n + 31) // 32, w


@pytest.mark.parametrize("path", ["numpy", "native"])
@pytest.mark.parametrize("seed", [0, 1])
def test_items_hold_at_most_32_rows_and_one_words_items_are_adjacent(path, seed):
    cfg = FiraConfig()
    hb = R.grouped_ids_batch(cfg, seed)
    tok, ptr, rows = M.embedding_items(hb, cfg)
    check_items(tok, ptr, len(rows), R.GROUP_COUNTS)
    if path == "numpy":
        os.environ["FIRA_HOST_LISTS"] = "numpy"
    try:
        lists = M.batch_lists(hb, cfg, True)
    finally:
        os.environ.pop("FIRA_HOST_LISTS", None)
    node_rows, tok2, ptr2, rows2 = lists[0], lists[8], lists[9], lists[10]
    check_items(tok2, ptr2, len(rows2), R.GROUP_COUNTS)
    assert np.array_equal(tok2, tok) and np.array_equal(ptr2, ptr)
    assert np.array_equal(np.asarray(node_rows)[np.asarray(rows2)], rows)          # compact ids of the same nodes
    ids = np.concatenate([hb.sou, hb.sub_token], axis=1)
    N, L = cfg.graph_len, cfg.sou_len + cfg.sub_token_len
    assert np.array_equal(ids[rows // N, rows % N], np.repeat(tok, np.diff(ptr)))   # every row carries its item's word
    assert rows.max() % N < L
