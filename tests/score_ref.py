"""A numpy statement of what the scoring kernel (csrc/score.hip, fira_decode_step_score) reports for one row: from the row's
distribution over V + S entries, the source id of every memory slot and the slot mask.  Sums are float64."""
import numpy as np


def score_row(dist, src_ids, valid, V, y, label=-1):
    """dist [V + S] probabilities, src_ids [S] the vocabulary id every memory slot copies (sou row then sub-token row), valid
    [S] the memory mask, y the target word (0 = nothing to score), label an entry index or -1.

    Returns p_word (float64 sum over every entry that resolves to y), p_entry / entry (the largest such entry, lowest index
    on ties; 0 / -1 when there is none), copy_share, p_label, top_id (first maximum of the row) and k, the number of terms
    in p_word."""
    dist = np.asarray(dist)
    src_ids, valid = np.asarray(src_ids), np.asarray(valid).astype(bool)
    S = len(src_ids)
    assert dist.shape == (V + S,)
    out = dict(p_word=0.0, p_entry=0.0, entry=-1, copy_share=0.0, p_label=0.0, top_id=int(np.argmax(dist)), k=0)
    if y == 0:
        return out
    entries = ([y] if 0 <= y < V else []) + [V + int(s) for s in np.nonzero(valid & (src_ids == y))[0]]
    if 0 <= label < V + S:
        out["p_label"] = float(dist[label])
    if not entries:
        return out
    vals = dist[entries].astype(np.float64)
    copy = float(vals[1:].sum()) if 0 <= y < V else float(vals.sum())
    out["p_word"] = float(vals.sum())
    out["k"] = len(entries)
    j = int(np.argmax(vals))                                   # first maximum; `entries` is in ascending index order
    out["p_entry"], out["entry"] = float(dist[entries[j]]), entries[j]
    out["copy_share"] = copy / out["p_word"] if out["p_word"] > 0 else 0.0
    return out


def message_logp(p, floor=1e-10):
    """Sum of log max(p, floor) over a message's scored tokens (the clamp of the training loss)."""
    return float(np.log(np.maximum(np.asarray(p, dtype=np.float64), floor)).sum())
