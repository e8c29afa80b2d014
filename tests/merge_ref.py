"""Test-only statement of the search over words (include/fira_hip.h: fira_merge_dist) in plain numpy, and the beam and greedy
searches written in torch ops / on the host on top of the engine's per-step distribution with an ``edit(dist, gen, length)`` hook
applied before ranking.  ``tests/test_merge_gpu.py`` holds the kernel and ``Searcher.beam`` / ``greedy`` with ``merge_copies``
against them.  Not part of the product package.  The loops follow ``constrain_ref``'s (stable sort: value descending, flattened
index ascending -- folded slots are exact zeros and tie by construction); the hook composes merge, then the constraint mask."""
import numpy as np
import torch

import constrain_ref as R
from constrain_ref import argmax_ref, dims_of                    # noqa: F401  (re-exported for the tests)
from search_ref import _resolve
from fira_icse_amd.config import EOS, START


def merged(row: np.ndarray, sou_row, sub_row, dims) -> np.ndarray:
    """The row after fira_merge_dist: np.float32 additions in the stated order -- the word's slots in ascending slot index, the
    generator entry last."""
    V, L, S = dims
    row = np.asarray(row, dtype=np.float32)
    out = row.copy()
    words = R.entry_words(sou_row, sub_row, dims)[V:]            # the source id of every slot
    slots = {}
    for s in range(L + S):                                       # ascending
        w = int(words[s])
        if 0 <= w < V:
            slots.setdefault(w, []).append(s)
    for w, ss in slots.items():
        acc = row[V + ss[0]]
        for s in ss[1:]:
            acc = np.float32(acc + row[V + s])
        out[w] = np.float32(acc + row[w])
        for s in ss:
            out[V + s] = np.float32(0.0)
    return out


def merged_rows(dist: np.ndarray, sou, sub, dims, rows_per_commit: int = 1) -> np.ndarray:
    return np.stack([merged(dist[r], sou[r // rows_per_commit], sub[r // rows_per_commit], dims) for r in range(dist.shape[0])])


def make_edit(sou, sub, dims, rows_per_commit, constraints=None):
    """edit(dist [R, W] float32 numpy, gen [R, T], length [R]) -> the distribution the search ranks: merge, then the mask."""
    def edit(dist, gen, length):
        out = merged_rows(dist, sou, sub, dims, rows_per_commit)
        if constraints is not None:
            out = R.edited(out, R._masks(gen, length, sou, sub, dims, constraints, rows_per_commit))
        return out
    return edit


@torch.no_grad()
def beam_edited(search, db, beam: int, edit):
    """constrain_ref.beam_constrained with ``edit`` in place of the mask."""
    cfg, dev = search.cfg, search.model.device_
    B, T, W = db.B, cfg.tar_len, cfg.out_len
    BR = B * beam
    ws = search._begin(db, beam)
    sou, sub = db.sou.long(), db.sub_token.long()
    gen = torch.zeros((B, beam, T), dtype=torch.int64, device=dev)
    gen[:, :, 0] = START
    length = torch.ones((B, beam), dtype=torch.int64, device=dev)
    prob = torch.zeros((B, beam), dtype=torch.float32, device=dev)
    prob[:, 0] = 1.0
    dist = torch.zeros((BR, W), dtype=torch.float32, device=dev)
    parent = None
    slot = torch.arange(beam, device=dev)
    rowbase = (torch.arange(B, device=dev) * beam)[:, None]
    for step in range(T - 1):
        last = torch.gather(gen, 2, (length - 1)[:, :, None])[:, :, 0]
        finished = last == EOS
        active = (~finished).any(0)
        active_slots = active.nonzero().view(-1)
        n_act = int(active_slots.numel())
        if n_act == 0:
            break
        tok = torch.where(length > step, gen[:, :, step], torch.zeros_like(last)).to(torch.int32).reshape(-1)
        search._step(ws, B, beam, step, tok.contiguous(), parent, dist, None, None)
        d = torch.from_numpy(edit(dist.cpu().numpy(), gen.reshape(BR, T).cpu().numpy(), length.reshape(BR).cpu().numpy())).to(dev)
        cand = d.view(B, beam, W) * prob[:, :, None]
        cand = torch.where(finished[:, :, None], torch.full_like(cand, -1.0), cand)
        blocks = cand[:, active_slots, :].reshape(B, n_act * W)
        order = torch.argsort(torch.where(finished, slot[None, :], slot[None, :] + beam), dim=1, stable=True)
        n_fin = finished.sum(1, keepdim=True)
        carried = torch.where(slot[None, :] < n_fin, torch.gather(prob, 1, order), torch.full_like(prob, -1.0))
        allv = torch.cat([blocks, carried], 1)
        top_p, top_i = torch.sort(allv, descending=True, dim=-1, stable=True)
        top_p, top_i = top_p[:, :beam], top_i[:, :beam]
        which, tokidx = top_i // W, top_i % W
        carry = which == n_act
        src_slot = torch.where(carry, torch.gather(order, 1, tokidx.clamp(max=beam - 1)),
                               active_slots[which.clamp(max=n_act - 1)])
        new_tok = _resolve(cfg, tokidx.clamp(max=W - 1), sou, sub)
        src_len = torch.gather(length, 1, src_slot)
        gen = torch.gather(gen, 1, src_slot[:, :, None].expand(B, beam, T)).clone()
        pos = src_len.clamp(max=T - 1)
        appended = gen.scatter(2, pos[:, :, None], new_tok[:, :, None])
        gen = torch.where(carry[:, :, None], gen, appended)
        length = torch.where(carry, src_len, src_len + 1)
        prob = top_p.contiguous()
        parent = (rowbase + src_slot).to(torch.int32).reshape(-1).contiguous()
    return gen, length, prob


@torch.no_grad()
def greedy_edited(search, db, edit):
    """constrain_ref.greedy_constrained with ``edit`` in place of the mask.  Also returns factors [B, T - 1]: the value the
    search multiplied in at every step (0 where the hypothesis had ended)."""
    cfg = search.cfg
    B, T, W = db.B, cfg.tar_len, cfg.out_len
    V, L, S = dims_of(cfg)
    ws = search._begin(db, 1)
    sou_h, sub_h = db.sou.cpu().numpy(), db.sub_token.cpu().numpy()
    out = np.zeros((B, T), dtype=np.int64)
    out[:, 0] = START
    length = np.ones(B, dtype=np.int64)
    prob = np.ones(B, dtype=np.float32)
    alive = np.ones(B, dtype=bool)
    tok = np.full(B, START, dtype=np.int32)
    factors = np.zeros((B, T - 1), dtype=np.float32)
    dist = torch.zeros((B, W), dtype=torch.float32, device=search.model.device_)
    for step in range(T - 1):
        if not alive.any():
            break
        search._step(ws, B, 1, step, torch.from_numpy(tok).to(dist.device), None, dist, None, None)
        d = edit(dist.cpu().numpy(), out, length)
        for b in range(B):
            if not alive[b]:
                tok[b] = 0
                continue
            i, p = argmax_ref(d[b])
            nt = i if i < V else (int(sou_h[b, i - V]) if i < V + L else int(sub_h[b, i - V - L]))
            out[b, step + 1] = nt
            factors[b, step] = p
            prob[b] = np.float32(prob[b]) * np.float32(p)
            length[b] += 1
            alive[b] = nt != EOS
            tok[b] = nt if alive[b] else 0
    return torch.from_numpy(out), torch.from_numpy(length), torch.from_numpy(prob), torch.from_numpy(factors)
