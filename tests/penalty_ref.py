"""Test-only statement of the soft word penalties and biases (include/fira_hip.h: fira_penalise_dist) in plain numpy: the count
of a word in a hypothesis, the factor table and the bias factors (restated here, not imported from decode.py), the edit of one
row with float32 multiplications in the defined order, and ``make_edit`` in the shape ``merge_ref.greedy_edited`` /
``beam_edited`` take, so the host search loops are theirs.  ``tests/test_penalty.py`` and ``tests/test_penalty_gpu.py`` hold
``decode.Penalties``, the kernel and the searches against it.  Not part of the product package."""
import numpy as np

from constrain_ref import argmax_ref, dims_of, entry_words, is_finished            # noqa: F401  (re-exported for the tests)

MAX_BIASED = 16


def counts(gen_row, length) -> dict:
    """{word: c(word)} over the positions 1 .. len - 1 of the hypothesis, len = clamp(length, 1, T)."""
    length = min(max(int(length), 1), len(gen_row))
    out = {}
    for w in gen_row[1:length]:
        out[int(w)] = out.get(int(w), 0) + 1
    return out


def factor_table(presence, frequency, tar_len) -> np.ndarray:
    """t[c] = float32(exp(-(float64(presence) + float64(frequency) * c))) for c >= 1, t[0] = 1."""
    t = np.ones(tar_len, dtype=np.float32)
    for c in range(1, tar_len):
        t[c] = np.float32(np.exp(-(np.float64(presence) + np.float64(frequency) * np.float64(c))))
    return t


def bias_arrays(rows, B):
    """``rows``: None, one mapping {id: b} for every commit, or B mappings (or None) -> (bias_id [B, 16] int32, bias_factor
    [B, 16] float32 = float32(exp(float64(b))), n_bias [B] int32), the ids of a commit ascending: the device buffers' layout."""
    if rows is None or hasattr(rows, "items"):
        rows = [rows] * B
    assert len(rows) == B
    ids = np.zeros((B, MAX_BIASED), dtype=np.int32)
    fac = np.ones((B, MAX_BIASED), dtype=np.float32)
    n = np.zeros(B, dtype=np.int32)
    for k, row in enumerate(rows):
        for q, w in enumerate(sorted(row or {})):
            ids[k, q] = w
            fac[k, q] = np.float32(np.exp(np.float64(row[w])))
        n[k] = len(row or {})
    return ids, fac, n


def edited(dist_row, gen_row, length, sou_row, sub_row, dims, table, bias_ids, bias_factors) -> np.ndarray:
    """The row after fira_penalise_dist.  ``bias_ids`` / ``bias_factors``: the commit's pairs in force (the first n_bias, clamped to
    0 .. 16).  Two np.float32 multiplications per touched entry, the count factor first; a finished row is returned as it is."""
    V, L, S = dims
    row = np.array(dist_row, dtype=np.float32, copy=True)
    if is_finished(gen_row, min(max(int(length), 1), len(gen_row))):
        return row
    c = counts(gen_row, length)
    words = entry_words(sou_row, sub_row, dims)
    bias = {}
    for w, f in zip(bias_ids, bias_factors):
        if 0 <= int(w) < V and int(w) not in bias:           # an id outside the vocabulary is ignored; the first of equal ids
            bias[int(w)] = np.float32(f)
    for w, n in c.items():                                   # (float32 array * float32 scalar: one rounding per element)
        at = words == w
        row[at] = row[at] * np.float32(table[n])
    for w, f in bias.items():
        at = words == w
        row[at] = row[at] * f
    return row


def edited_rows(dist, gen, length, sou, sub, dims, rows_per_commit, table, bias_id, bias_factor, n_bias) -> np.ndarray:
    gen, length = np.asarray(gen), np.asarray(length)
    out = []
    for r in range(dist.shape[0]):
        b = r // rows_per_commit
        n = min(max(int(n_bias[b]), 0), MAX_BIASED)
        out.append(edited(dist[r], gen[r], length[r], sou[b], sub[b], dims, table, bias_id[b, :n], bias_factor[b, :n]))
    return np.stack(out)


def make_edit(sou, sub, dims, rows_per_commit, table, bias_id, bias_factor, n_bias, before=None):
    """edit(dist [R, W] float32 numpy, gen [R, T], length [R]) for merge_ref's loops: ``before`` (the edit of the links ahead in
    the chain -- merge, prefix, constraints -- or None), then the penalties."""
    def edit(dist, gen, length):
        out = dist if before is None else before(dist, gen, length)
        return edited_rows(out, gen, length, sou, sub, dims, rows_per_commit, table, bias_id, bias_factor, n_bias)
    return edit
