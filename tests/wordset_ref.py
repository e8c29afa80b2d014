"""Test-only statement of the per-commit word sets (include/fira_hip.h: fira_wordset_dist) in plain numpy /
Python, written from its definition, row by row, with np.float32 arithmetic.  Not part of the product.

A set is None (not given) or the commit's row of packed uint32 words: bit w % 32 of word w / 32 for id w; the bits at or past V are
ignored.  For an unfinished row (len = clamp(length, 1, T); finished: the last id is <eos>) the word w is blocked iff
    allow is given and w != <eos> and not in(allow, w),   or   in(deny, w),   or   in(ground, w) and not carried(w)
with in(S, w) = S is given and 0 <= w < V and the bit is set, carried(w) = some slot whose bit in slot_valid is set has the source
id w.  A blocked entry becomes +0.0f; an entry that is not blocked with in(boost, w) becomes float32(dist * factor); every other
element keeps its bits."""
import numpy as np

from constrain_ref import argmax_ref, entry_words, is_finished  # noqa: F401  (argmax_ref: the arg-max the kernel reports)

EOS = 1


def in_set(words, w, V) -> bool:
    w = int(w)
    return words is not None and 0 <= w < V and bool((int(words[w >> 5]) >> (w & 31)) & 1)


def carried_words(sou_row, sub_row, slot_valid, dims) -> set:
    V, L, S = dims
    src = entry_words(sou_row, sub_row, dims)[V:]
    return {int(w) for j, w in enumerate(src) if (int(slot_valid[j >> 5]) >> (j & 31)) & 1}


def blocked(w, V, allow, deny, ground, carried) -> bool:
    w = int(w)
    return ((allow is not None and w != EOS and not in_set(allow, w, V)) or in_set(deny, w, V)
            or (in_set(ground, w, V) and w not in carried))


def wordset_row(dist_row, gen_row, length, sou_row, sub_row, dims, allow=None, deny=None, boost=None, ground=None, slot_valid=None,
                factor=None):
    """(the edited row, bool[W] blocked, bool[W] boosted) of one row."""
    V = dims[0]
    words = entry_words(sou_row, sub_row, dims)
    out = np.array(dist_row, dtype=np.float32, copy=True)
    blk, up = np.zeros(words.shape, dtype=bool), np.zeros(words.shape, dtype=bool)
    n = min(max(int(length), 1), len(gen_row))
    if is_finished(gen_row, n):
        return out, blk, up
    carried = carried_words(sou_row, sub_row, slot_valid, dims) if ground is not None else set()
    for i, w in enumerate(words):
        if blocked(w, V, allow, deny, ground, carried):
            blk[i] = True
            out[i] = np.float32(0.0)
        elif in_set(boost, w, V):
            up[i] = True
            out[i] = np.float32(out[i]) * np.float32(factor)
    return out, blk, up
