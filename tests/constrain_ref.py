"""Test-only statement of the search constraints (include/fira_hip.h: fira_constrain_dist) in plain Python / numpy, and the
beam and greedy searches written in torch ops on top of the engine's per-step distribution with that statement applied
before ranking.  ``tests/test_constrain_gpu.py`` holds the kernel and ``Searcher.beam`` / ``greedy`` against them.  Not part of
the product package.  The beam loop follows ``search_ref.beam_torch`` (which has no hook for an edit of the distribution), with
one difference: the sort is STABLE, i.e. (value descending, flattened index ascending) -- the device's documented order --
because zeroed entries tie by construction."""
from typing import Sequence, Tuple

import numpy as np
import torch

from search_kit import dims_of
from fira_icse_amd.config import EOS, START


def blocked_words(hyp_words: Sequence[int], n: int, min_length: int, banned: Sequence[int]) -> set:
    """The blocked words of an UNFINISHED hypothesis h_1 .. h_m (``hyp_words``, without <start>)."""
    h = [int(w) for w in hyp_words]
    m = len(h)
    out = set(int(w) for w in banned)
    if n >= 1:
        tail = h[m - (n - 1):] if n > 1 else []              # the last n - 1 words
        for j in range(1, m + 1):                            # 1-based start of a completed n-gram h_j .. h_{j+n-1}
            if j + n - 1 > m:
                break
            if h[j - 1:j + n - 2] == tail:
                out.add(h[j + n - 2])
    if m < min_length:
        out.add(EOS)
    return out


def entry_words(sou_row, sub_row, dims) -> np.ndarray:
    """w(i) for every entry i of the V + L + S wide row (search_ref._resolve)."""
    V, L, S = dims
    return np.concatenate([np.arange(V, dtype=np.int64), np.asarray(sou_row, dtype=np.int64)[:L],
                           np.asarray(sub_row, dtype=np.int64)[:S]])


def is_finished(gen_row, length) -> bool:
    return int(gen_row[int(length) - 1]) == EOS


def blocked_mask(gen_row, length, sou_row, sub_row, dims, constraints) -> np.ndarray:
    """bool[W]: the entries fira_constrain_dist sets to 0 for this row."""
    words = entry_words(sou_row, sub_row, dims)
    if is_finished(gen_row, length):
        return np.zeros(words.shape, dtype=bool)
    hyp = [int(w) for w in gen_row[1:int(length)]]
    blk = blocked_words(hyp, constraints.no_repeat_ngram, constraints.min_length, constraints.banned)
    return np.isin(words, np.array(sorted(blk), dtype=np.int64))


def edited(dist: np.ndarray, mask: np.ndarray) -> np.ndarray:
    return np.where(mask, np.float32(0.0), dist)


def argmax_ref(row: np.ndarray) -> Tuple[int, np.float32]:
    """Largest value, lowest index among equals (np.argmax returns the first maximum)."""
    i = int(np.argmax(row))
    return i, row[i]


def _masks(gen, length, sou, sub, dims, constraints, rows_per_commit) -> np.ndarray:
    gen, length = np.asarray(gen), np.asarray(length)
    return np.stack([blocked_mask(gen[r], length[r], sou[r // rows_per_commit], sub[r // rows_per_commit], dims, constraints)
                     for r in range(gen.shape[0])])


def _resolve(cfg, idx, sou, sub):
    V, L = cfg.vocab_size, cfg.sou_len
    from_sou = torch.gather(sou, 1, (idx - V).clamp(0, sou.shape[1] - 1))
    from_sub = torch.gather(sub, 1, (idx - V - L).clamp(0, sub.shape[1] - 1))
    return torch.where(idx >= V + L, from_sub, torch.where(idx >= V, from_sou, idx))


@torch.no_grad()
def beam_constrained(search, db, beam: int, constraints):
    """search_ref.beam_torch with the blocked entries of every row zeroed before the candidates are ranked."""
    cfg, dev = search.cfg, search.model.device_
    B, T, W = db.B, cfg.tar_len, cfg.out_len
    BR = B * beam
    dims = dims_of(cfg)
    ws = search._begin(db, beam)
    sou, sub = db.sou.long(), db.sub_token.long()
    sou_h, sub_h = sou.cpu().numpy(), sub.cpu().numpy()
    gen = torch.zeros((B, beam, T), dtype=torch.int64, device=dev)
    gen[:, :, 0] = START
    length = torch.ones((B, beam), dtype=torch.int64, device=dev)
    prob = torch.zeros((B, beam), dtype=torch.float32, device=dev)
    prob[:, 0] = 1.0
    dist = torch.empty((BR, W), dtype=torch.float32, device=dev)
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
        mask = _masks(gen.reshape(BR, T).cpu().numpy(), length.reshape(BR).cpu().numpy(), sou_h, sub_h, dims, constraints, beam)
        d = torch.where(torch.from_numpy(mask).to(dev), torch.zeros_like(dist), dist)
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
def greedy_constrained(search, db, constraints):
    """The greedy loop (fira_greedy_advance's bookkeeping) on the host: per step the engine's distribution, the blocked entries
    zeroed, the arg-max (lowest index among equals), the fp32 running product."""
    cfg = search.cfg
    B, T, W = db.B, cfg.tar_len, cfg.out_len
    V, L, S = dims = dims_of(cfg)
    ws = search._begin(db, 1)
    sou_h, sub_h = db.sou.cpu().numpy(), db.sub_token.cpu().numpy()
    out = np.zeros((B, T), dtype=np.int64)
    out[:, 0] = START
    length = np.ones(B, dtype=np.int64)
    prob = np.ones(B, dtype=np.float32)
    alive = np.ones(B, dtype=bool)
    tok = np.full(B, START, dtype=np.int32)
    dist = torch.empty((B, W), dtype=torch.float32, device=search.model.device_)
    for step in range(T - 1):
        if not alive.any():
            break
        search._step(ws, B, 1, step, torch.from_numpy(tok).to(dist.device), None, dist, None, None)
        d = dist.cpu().numpy()
        mask = _masks(out, length, sou_h, sub_h, dims, constraints, 1)
        for b in range(B):
            if not alive[b]:
                tok[b] = 0
                continue
            i, p = argmax_ref(edited(d[b], mask[b]))
            nt = i if i < V else (int(sou_h[b, i - V]) if i < V + L else int(sub_h[b, i - V - L]))
            out[b, step + 1] = nt
            prob[b] = np.float32(prob[b]) * np.float32(p)
            length[b] += 1
            alive[b] = nt != EOS
            tok[b] = nt if alive[b] else 0
    return torch.from_numpy(out), torch.from_numpy(length), torch.from_numpy(prob)


# ------------------------------------------------------------------------------------------------ properties of a message
def has_repeated_ngram(words: Sequence, n: int) -> bool:
    grams = [tuple(words[i:i + n]) for i in range(len(words) - n + 1)]
    return len(set(grams)) != len(grams)
