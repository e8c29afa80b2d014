"""numpy statement (float64) of fira_sample_dist (csrc/sample_row.hip): the sampler's filters, cuts and Gumbel-max draw on a
distribution row as it stands in memory -- unnormalised, possibly with zeros where an edit removed entries.  Built from the
sampler's own twins: sample_ref (noise, top-k, top-p, the draw) and cut_ref (the four cuts), which already take every quantity
relative to the row they are given: the weights relative to ``p.max()`` -- the maximum of the row itself, as the kernel's pmax --
the top-p mass relative to the kept mass, q = w / sum w.  What this module adds is the row without a positive entry."""
from __future__ import annotations

import numpy as np

import cut_ref
import sample_ref

REL = 1e-4                       # the relaxation of test_sample_gpu.py / test_cut_gpu.py
EMPTY = (0, 0.0)                 # (best_id, best_p) of a row without a positive entry: ArgMax's report for an all-zero row


def kept(p, rel=REL, **kw):
    """(strict, relaxed) masks of the entries the filters and cuts ``kw`` (temperature, top_k, top_p, min_p, epsilon, eta,
    typical_p) keep of row ``p``; an entry with p = 0 is in neither.  A row without a positive entry keeps nothing."""
    p = np.asarray(p, dtype=np.float64)
    if not (p > 0).any():
        none = np.zeros(p.shape, dtype=bool)
        return none, none
    strict, relaxed = cut_ref.kept_sets(p, rel=rel, **kw)
    return strict & (p > 0), relaxed & (p > 0)


def draw(p, key: int, seed: int, j: int, tar_len: int, step: int, rel=REL, **kw):
    """The draw of sample ``j`` of the commit with ``key`` at ``step`` on row ``p``: (id, gap, clear).  ``id`` is the Gumbel-max
    over the strict kept set, ``gap`` its distance to the runner-up, ``clear`` says that the decision does not hang on fp32
    rounding -- the rule of test_sample_gpu.py: gap > 1e-4, and the strict and the relaxed set give the same pick.  A row
    without a positive entry: (EMPTY[0], inf, True)."""
    p = np.asarray(p, dtype=np.float64)
    strict, relaxed = kept(p, rel=rel, **kw)
    if not strict.any():
        return EMPTY[0], float("inf"), True
    T = kw.get("temperature", 1.0)
    g = sample_ref.gumbel(sample_ref.row_stream(int(key), int(seed), int(j), int(tar_len), int(step)), len(p))
    i_ref, gap = sample_ref.gumbel_argmax(p, strict, T, g)
    i_rel, _ = sample_ref.gumbel_argmax(p, relaxed, T, g)
    return i_ref, gap, bool(gap > 1e-4 and i_ref == i_rel)
