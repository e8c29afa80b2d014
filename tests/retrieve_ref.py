"""Test-only statement of retrieval-augmented search (include/fira_hip.h: fira_pool_memory, fira_nn_search, fira_mix_neighbour)
in plain numpy, and the host side of the searches with a neighbour.  ``tests/test_retrieve.py`` (CPU) and
``tests/test_retrieve_gpu.py`` hold the kernels and ``Searcher.greedy / greedy_many / beam(neighbour=...)`` against them.  Not
part of the product package.

The searches are ``merge_ref.beam_edited`` / ``greedy_edited`` themselves, run on a ``RefNeighbour``: an object with the
``_begin`` / ``_step`` of a Searcher whose step is two single-model ``Searcher._step`` calls (the input batch, the neighbour
batch) followed by the numpy merge of the neighbour's row and the numpy mix, on the host."""
import numpy as np
import torch

import merge_ref as M
from constrain_ref import argmax_ref, dims_of                    # noqa: F401  (re-exported for the tests)

D = 256
F32 = np.float32


# ------------------------------------------------------------------------------------------------ pool
def pool(mem, valid) -> np.ndarray:
    """u [B, 256] of fira_pool_memory: every operation one np.float32 operation, in the kernel's order.  Rows with valid == 0
    are never read."""
    mem = np.asarray(mem, dtype=F32)
    B, S, _ = mem.shape
    out = np.zeros((B, D), dtype=F32)
    for b in range(B):
        acc, n = np.zeros(D, dtype=F32), 0
        for s in range(S):
            if valid[b, s] != 0:
                acc = acc + mem[b, s]
                n += 1
        if n == 0:
            continue
        v = acc / F32(n)
        ss = F32(0)
        for c in range(D):
            t = v[c] * v[c]
            ss = ss + t
        nrm = np.sqrt(ss)
        assert nrm.dtype == F32 and v.dtype == F32
        if nrm > 0:
            out[b] = v / nrm
    return out


def pool64(mem, valid) -> np.ndarray:
    """The same vector in float64 (valid rows only)."""
    mem = np.asarray(mem)
    B = mem.shape[0]
    out = np.zeros((B, D), dtype=np.float64)
    for b in range(B):
        rows = mem[b][np.asarray(valid[b]) != 0].astype(np.float64)
        if rows.shape[0] == 0:
            continue
        v = rows.sum(0) / rows.shape[0]
        n = np.sqrt((v * v).sum())
        if n > 0:
            out[b] = v / n
    return out


# ------------------------------------------------------------------------------------------------ nearest neighbour
DOT_BOUND = 2 * 256 * 2.0 ** -24       # |fp32 dot - exact| of two unit vectors of 256 elements, any summation order, doubled


def nn64(Q, store, exclude=None):
    """(idx, sim clamped to [0, 1], margin to the runner-up) in float64; NaN rows never win; ties: the lowest index."""
    scores = np.asarray(Q, dtype=np.float64) @ np.asarray(store, dtype=np.float64).T
    B, N = scores.shape
    idx, sim, margin = np.zeros(B, np.int64), np.zeros(B), np.full(B, np.inf)
    for b in range(B):
        s = scores[b].copy()
        s[np.isnan(s)] = -np.inf
        if exclude is not None and exclude[b] >= 0:
            s[exclude[b]] = -np.inf
        j = int(np.argmax(s))                        # first maximum
        idx[b], sim[b] = j, min(max(s[j], 0.0), 1.0)
        rest = np.delete(s, j)
        if rest.size:
            margin[b] = s[j] - rest.max()
    return idx, sim, margin


def unit_rows(rng, n) -> np.ndarray:
    x = rng.standard_normal((n, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


# ------------------------------------------------------------------------------------------------ mix
def coef(sim, lam, min_sim=0.0) -> np.ndarray:
    """(a, b) per commit as the host forms them: float64, then one rounding to float32."""
    out = []
    for s in np.asarray(sim, dtype=np.float64).reshape(-1):
        c = float(lam) * float(s)
        out.append((1.0, 0.0) if s < min_sim else (1.0 / (1.0 + c), c / (1.0 + c)))
    return np.array(out, dtype=np.float64).astype(F32).reshape(-1, 2)


def mix(p, q, cf, V, rows_per_commit=1) -> np.ndarray:
    """fira_mix_neighbour: every multiply and add an np.float32 operation of its own; q is not read from V on."""
    p, q = np.asarray(p, dtype=F32), np.asarray(q, dtype=F32)
    out = np.empty_like(p)
    for r in range(p.shape[0]):
        a, b = F32(cf[r // rows_per_commit, 0]), F32(cf[r // rows_per_commit, 1])
        x = a * p[r]
        y = b * q[r, :V]
        out[r] = x
        out[r, :V] = x[:V] + y
    assert out.dtype == F32
    return out


def best_of(rows):
    best = [argmax_ref(rows[r]) for r in range(rows.shape[0])]
    return np.array([b[0] for b in best], dtype=np.int32), np.array([b[1] for b in best], dtype=F32)


# ------------------------------------------------------------------------------------------------ the searches
class RefNeighbour:
    """Stands in for a Searcher in ``merge_ref.beam_edited`` / ``greedy_edited``: ``own`` and ``other`` are two single-model
    Searchers over the SAME model (two workspaces), ``nb_db`` the neighbour batch, ``cf`` the float32 coefficients [B, 2]."""

    def __init__(self, own, other, nb_db, cf):
        self.own, self.other, self.nb_db, self.cf = own, other, nb_db, np.asarray(cf, dtype=F32)
        self.cfg, self.model = own.cfg, own.model
        self.dims = dims_of(own.cfg)
        self.sou, self.sub = nb_db.sou.cpu().numpy(), nb_db.sub_token.cpu().numpy()

    def _begin(self, db, beam):
        return self.own._begin(db, beam), self.other._begin(self.nb_db, beam)

    def _step(self, ws, B, beam, step, tokens, parent, dist, best_id, best_p):
        assert best_id is None and best_p is None
        p, q = torch.zeros_like(dist), torch.zeros_like(dist)
        self.own._step(ws[0], B, beam, step, tokens, parent, p, None, None)
        self.other._step(ws[1], B, beam, step, tokens, parent, q, None, None)
        qm = M.merged_rows(q.cpu().numpy(), self.sou, self.sub, self.dims, beam)
        dist.copy_(torch.from_numpy(mix(p.cpu().numpy(), qm, self.cf, self.dims[0], beam)))


def identity_edit(dist, gen, length):
    return dist


def beam_neighbour(own, other, db, nb_db, cf, beam, edit=identity_edit):
    return tuple(t.cpu() for t in M.beam_edited(RefNeighbour(own, other, nb_db, cf), db, beam, edit))


def greedy_neighbour(own, other, db, nb_db, cf, edit=identity_edit):
    return M.greedy_edited(RefNeighbour(own, other, nb_db, cf), db, edit)[:3]
