"""Test-only statement of ensemble decoding (include/fira_hip.h: fira_mix_dist) in plain numpy, and the host side of the searches
under an ensemble.  ``tests/test_ensemble.py`` (CPU) and ``tests/test_ensemble_gpu.py`` hold the kernel and ``Searcher(model,
members=...)`` against them.  Not part of the product package.

The searches are ``merge_ref.beam_edited`` / ``greedy_edited`` themselves (stable sort: value descending, flattened index
ascending), run on a ``RefEnsemble``: an object with the ``_begin`` / ``_step`` of a Searcher whose step is every member's own
single-model ``Searcher._step`` followed by the numpy mix on the host.  The edit hook composes merge, then the constraint mask."""
import numpy as np
import torch

import constrain_ref as R
import merge_ref as M
from constrain_ref import argmax_ref, dims_of                    # noqa: F401  (re-exported for the tests)


def mix(dists, weights) -> np.ndarray:
    """The mix of fira_mix_dist: a member-ordered sum of weighted terms, every multiply and every add an np.float32 operation of
    its own (numpy never fuses them)."""
    w = [np.float32(x) for x in weights]
    d = [np.asarray(x, dtype=np.float32) for x in dists]
    assert len(w) == len(d) >= 1
    acc = w[0] * d[0]
    for m in range(1, len(d)):
        t = w[m] * d[m]
        acc = acc + t
    assert acc.dtype == np.float32
    return acc


def best_of(rows: np.ndarray):
    """(best_id int32 [R], best_p float32 [R]) of fira_mix_dist: largest value, lowest index among equals."""
    best = [argmax_ref(rows[r]) for r in range(rows.shape[0])]
    return np.array([b[0] for b in best], dtype=np.int32), np.array([b[1] for b in best], dtype=np.float32)


def make_edit(sou, sub, dims, rows_per_commit, merge=False, constraints=None):
    """edit(dist [R, W] float32 numpy, gen [R, T], length [R]) -> the distribution the search ranks: merge (if asked), then the
    constraint mask (if any); the identity with neither."""
    def edit(dist, gen, length):
        out = M.merged_rows(dist, sou, sub, dims, rows_per_commit) if merge else dist
        if constraints is not None:
            out = R.edited(out, R._masks(gen, length, sou, sub, dims, constraints, rows_per_commit))
        return out
    return edit


class RefEnsemble:
    """Stands in for a Searcher in ``merge_ref.beam_edited`` / ``greedy_edited``: ``searchers`` are single-model Searchers (one
    per member, the primary first), ``weights`` the float32 weights the ensemble under test uses."""

    def __init__(self, searchers, weights):
        self.searchers, self.weights = list(searchers), [np.float32(w) for w in weights]
        self.cfg, self.model = searchers[0].cfg, searchers[0].model
        assert len(self.searchers) == len(self.weights)

    def _begin(self, db, beam):
        return [s._begin(db, beam) for s in self.searchers]

    def _step(self, ws, B, beam, step, tokens, parent, dist, best_id, best_p):
        assert best_id is None and best_p is None
        parts = []
        for s, w in zip(self.searchers, ws):
            d = torch.zeros_like(dist)
            s._step(w, B, beam, step, tokens, parent, d, None, None)
            parts.append(d.cpu().numpy())
        dist.copy_(torch.from_numpy(mix(parts, self.weights)))


def beam_ensemble(searchers, weights, db, beam, edit):
    return tuple(t.cpu() for t in M.beam_edited(RefEnsemble(searchers, weights), db, beam, edit))


def greedy_ensemble(searchers, weights, db, edit):
    return M.greedy_edited(RefEnsemble(searchers, weights), db, edit)


# ------------------------------------------------------------------------------------------------ inputs of the kernel tests
# (name, R, W, n_members, weights as given -- None = uniform); W = 45 is no multiple of 4, 1 061 = 37 + 600 + 424 is the widest
# synthetic row of the merge tests, 25 020 the model's
CASES = [("R7-W45-M2", 7, 45, 2, None), ("R7-W45-M3", 7, 45, 3, (0.5, 0.3, 0.2)), ("R7-W45-M8", 7, 45, 8, None),
         ("R6-W1-M2", 6, 1, 2, (0.25, 0.75)), ("R4-W1061-M3", 4, 37 + 600 + 424, 3, None), ("R6-W25020-M2", 6, 25020, 2, (2.0, 1.0))]
SEED = 5


def trap_indices(W):
    """(a, b) of the tie trap and (i, j, k) of the flip trap: five distinct indices that fall into the head, the body and the
    tail of a row cut at 16-byte boundaries.  None for a row too narrow to hold them."""
    if W < 8:
        return None
    return (1, W - 2), (2, W - 1, W // 2)


def make_case(name, n_rows, W, n_members, weights, seed=SEED):
    """Member rows uniform in (1e-6, 1) with a handful of exact 0.0f.  Forced into the rows, so no property rests on the draw
    (rows at least 8 wide; a row of one element has one candidate and nothing to trap):
      tie    (even rows) indices a < b carry the same value in every member -- 2 + m / 4 in member m, above everything drawn -- so
             the mix holds identical bits at a and b, they are the row's maximum, and a must win;
      flip   (odd rows) member 0's largest entry is i (3.0), member 1's is j (3.0), and k holds 2.5 in EVERY member: k is no
             member's arg-max among the first two, but the mix gives it 2.5 sum(w) against at most 3 w_m + (1 - w_m) < 2.5 for
             i and j (every weight of members 0 and 1 is below 0.75 in CASES)."""
    from fira_icse_amd.decode import ensemble_weights
    rng = np.random.RandomState(seed + 31 * W + n_rows + n_members)
    w = ensemble_weights(weights, n_members)
    dists = [rng.uniform(1e-6, 1.0, size=(n_rows, W)).astype(np.float32) for _ in range(n_members)]
    for d in dists:
        for r in range(n_rows):
            d[r, rng.randint(0, W, size=min(3, W))] = np.float32(0.0)
    case = dict(name=name, R=n_rows, W=W, M=n_members, weights=w, dists=dists, tie_rows=[], flip_rows=[], traps=trap_indices(W))
    if case["traps"] is not None:
        (a, b), (i, j, k) = case["traps"]
        for r in range(n_rows):
            if r % 2 == 0:
                for m, d in enumerate(dists):
                    d[r, a] = d[r, b] = np.float32(2.0 + 0.25 * m)
                case["tie_rows"].append(r)
            else:
                dists[0][r, i] = np.float32(3.0)
                dists[1][r, j] = np.float32(3.0)
                for d in dists:
                    d[r, k] = np.float32(2.5)
                case["flip_rows"].append(r)
    return case


def reference(case):
    out = mix(case["dists"], case["weights"])
    return (out,) + best_of(out)
