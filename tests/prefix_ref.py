"""Test-only statement of the prefix-forced search (include/fira_hip.h: fira_force_dist) in plain numpy, and the greedy and beam
searches on top of the engine's per-step distribution with that statement applied before ranking (``merge_ref``'s loops with
their ``edit`` hook: merge, then the prefix, then the constraint mask -- the order of ``Searcher``).  ``tests/test_prefix_gpu.py``
holds the kernel and ``Searcher.beam`` / ``greedy`` with ``prefix`` against them.  Not part of the product package."""
import numpy as np

import constrain_ref as R
import merge_ref as M
from constrain_ref import argmax_ref, dims_of, entry_words, is_finished            # noqa: F401  (re-exported for the tests)


def forced_word(gen_row, length, prefix_row, prefix_len, T):
    """The word row must take next, or None where the row is not forced (finished, or past its commit's prefix)."""
    length = min(max(int(length), 1), T)
    m = length - 1
    if is_finished(gen_row, length) or m >= min(max(int(prefix_len), 0), T):
        return None
    return int(prefix_row[m])


def forced_mask(gen_row, length, sou_row, sub_row, dims, prefix_row, prefix_len) -> np.ndarray:
    """bool[W]: the entries fira_force_dist sets to 0 for this row -- every entry whose word is not the forced one."""
    words = entry_words(sou_row, sub_row, dims)
    y = forced_word(gen_row, length, prefix_row, prefix_len, len(gen_row))
    if y is None:
        return np.zeros(words.shape, dtype=bool)
    return words != y


def edited(dist: np.ndarray, mask: np.ndarray) -> np.ndarray:
    return np.where(mask, np.float32(0.0), dist)


def masks(gen, length, sou, sub, dims, prefix, prefix_len, rows_per_commit) -> np.ndarray:
    gen, length = np.asarray(gen), np.asarray(length)
    return np.stack([forced_mask(gen[r], length[r], sou[r // rows_per_commit], sub[r // rows_per_commit], dims,
                                 prefix[r // rows_per_commit], prefix_len[r // rows_per_commit]) for r in range(gen.shape[0])])


def prefix_arrays(rows, T):
    """B lists of ids -> (prefix [B, T] int32 zero-padded, prefix_len [B] int32): the layout of the device buffers."""
    prefix = np.zeros((len(rows), T), dtype=np.int32)
    for b, row in enumerate(rows):
        prefix[b, :len(row)] = row
    return prefix, np.array([len(row) for row in rows], dtype=np.int32)


def make_edit(search, db, rows, rows_per_commit, merge=False, constraints=None):
    """edit(dist, gen, length) for merge_ref's loops: merge (optional), the prefix, the constraint mask (optional)."""
    cfg = search.cfg
    dims = dims_of(cfg)
    sou, sub = db.sou.cpu().numpy(), db.sub_token.cpu().numpy()
    prefix, prefix_len = prefix_arrays(rows, cfg.tar_len)

    def edit(dist, gen, length):
        out = M.merged_rows(dist, sou, sub, dims, rows_per_commit) if merge else dist
        out = edited(out, masks(gen, length, sou, sub, dims, prefix, prefix_len, rows_per_commit))
        if constraints is not None:
            out = R.edited(out, R._masks(gen, length, sou, sub, dims, constraints, rows_per_commit))
        return out
    return edit


def greedy_forced(search, db, rows, merge=False, constraints=None):
    """(tokens, lengths, probability) of the greedy loop on the host with the prefix statement applied at every step."""
    return M.greedy_edited(search, db, make_edit(search, db, rows, 1, merge, constraints))[:3]


def beam_forced(search, db, beam, rows, merge=False, constraints=None):
    return M.beam_edited(search, db, beam, make_edit(search, db, rows, beam, merge, constraints))
