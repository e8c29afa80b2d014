"""Test-only statement of the phrase controls (include/fira_hip.h: fira_ban_phrases_dist, fira_beam_select_phrases) in plain
numpy / Python, written from their definitions.  Not part of the product.

Banned phrases, for an unfinished row with the words h_1 .. h_m: the phrase (w_1 .. w_l) blocks w_l iff m >= l - 1 and the last
l - 1 words equal w_1 .. w_{l-1}; every entry whose word is blocked becomes 0.0f, everything else keeps its bits.

Required items, for a hypothesis h and the items I_0 .. I_{n-1}:
    done(h)     = the items that occur contiguously in h
    partial(h)  = the largest q >= 1 for which some item outside done(h) has its first q words as a PROPER prefix and those words
                  are the last q words of h; 0 if there is none
    progress(h) = sum of len(I) over done(h) + partial(h);   total = sum of len(I);   bank(h) = progress(h)
    running   entry i of running slot j: p = fp32(dist[j, i] * prob[j]), bank = progress(h_j . w(i))
    carried   a finished hypothesis: p = prob[j], bank = progress(h_j)
    void      the row of a finished hypothesis, the padding of the carried list, and every entry with w(i) == <eos> of a
              running row with progress(h_j) < total
and the two phases and the written order of require_ref.py with C = total."""
import numpy as np

from constrain_ref import entry_words, is_finished

EOS = 1
MAX_ITEMS = 4


# ------------------------------------------------------------------------------------------------ banned phrases
def blocked_by_phrases(hyp_words, phrases) -> set:
    """The words the phrases block after the UNFINISHED hypothesis h_1 .. h_m (``hyp_words``, without <start>)."""
    h = [int(w) for w in hyp_words]
    out = set()
    for ph in phrases:
        ph = [int(w) for w in ph]
        head = ph[:-1]
        if len(h) >= len(head) and h[len(h) - len(head):] == head:
            out.add(ph[-1])
    return out


def phrases_of(phrase, phrase_len, n_phrases):
    """The phrases of a commit from its device rows, as the kernel reads them: the count clamped to 0..8, a phrase with a length
    outside 2..4 ignored."""
    n = min(max(int(n_phrases), 0), 8)
    return [[int(w) for w in phrase[q][:int(phrase_len[q])]] for q in range(n) if 2 <= int(phrase_len[q]) <= 4]


def ban_mask(gen_row, length, sou_row, sub_row, dims, phrases) -> np.ndarray:
    """bool[W]: the entries fira_ban_phrases_dist sets to 0 for this row."""
    words = entry_words(sou_row, sub_row, dims)
    n = min(max(int(length), 1), len(gen_row))
    if is_finished(gen_row, n):
        return np.zeros(words.shape, dtype=bool)
    blk = blocked_by_phrases(gen_row[1:n], phrases)
    return np.isin(words, np.array(sorted(blk), dtype=np.int64))


# ------------------------------------------------------------------------------------------------ required items
def occurs(h, item) -> bool:
    return any(h[o:o + len(item)] == item for o in range(len(h) - len(item) + 1))


def done_set(h, items):
    return [k for k, item in enumerate(items) if occurs(h, item)]


def progress(h, items) -> int:
    h = [int(w) for w in h]
    items = [[int(w) for w in item] for item in items]
    done = done_set(h, items)
    partial = 0
    for k, item in enumerate(items):
        if k in done:
            continue
        for q in range(1, len(item)):                         # proper prefixes only
            if q <= len(h) and h[len(h) - q:] == item[:q]:
                partial = max(partial, q)
    return sum(len(items[k]) for k in done) + partial


def items_of(words_row, item_len_row, n_items):
    """The items of a commit from its device rows, as the kernel reads them: the count clamped to 0..4, each length clamped so
    that the lengths sum to at most 4."""
    n = min(max(int(n_items), 0), MAX_ITEMS)
    items, off = [], 0
    for k in range(n):
        l = min(max(int(item_len_row[k]), 0), 4 - off)
        if l:
            items.append([int(w) for w in words_row[off:off + l]])
        off += l
    return items


def hyp(gen_row, length):
    n = min(max(int(length), 1), len(gen_row))
    return [int(g) for g in gen_row[1:n]]


def select(dist, fin, active, prob, length, gen, words, items):
    """The picks of one commit and step in WRITTEN order: dicts (src, carry, entry, word, p, bank, phase, index)."""
    beam, W = dist.shape
    total = sum(len(i) for i in items)
    h = [hyp(gen[j], length[j]) for j in range(beam)]
    prog = [progress(h[j], items) for j in range(beam)]
    cols = {n: [] for n in ("p", "void", "bank", "src", "entry", "carry")}

    def add(**kw):                                             # scalars are broadcast over the longest column
        n = max(np.size(v) for v in kw.values())
        for name, v in kw.items():
            cols[name].append(np.broadcast_to(np.asarray(v), (n,)).copy())

    for j in range(beam):                                      # running slots in slot order
        if not active[j]:
            continue
        if fin[j]:
            add(p=np.float32(-1.0), void=True, bank=-1, src=j, entry=np.arange(W), carry=False)
            continue
        p = (dist[j].astype(np.float32) * np.float32(prob[j])).astype(np.float32)
        # progress(h_j . w) depends on w only through its equality with the items' words: one value per such word, and one for
        # every other word (spelled -1)
        bank = np.full(W, progress(h[j] + [-1], items), dtype=np.int64)
        for w in sorted(set(w for item in items for w in item)):
            bank[words == w] = progress(h[j] + [w], items)
        void = (words == EOS) & (prog[j] < total)
        add(p=np.where(void, np.float32(-1.0), p).astype(np.float32), void=void, bank=np.where(void, -1, bank), src=j,
            entry=np.arange(W), carry=False)
    n_fin = 0
    for j in range(beam):                                      # the carried list: finished hypotheses, slot order
        if fin[j]:
            add(p=np.array([prob[j]], dtype=np.float32), void=False, bank=prog[j], src=j, entry=n_fin, carry=True)
            n_fin += 1
    for q in range(n_fin, beam):                               # its padding
        add(p=np.array([-1.0], dtype=np.float32), void=True, bank=-1, src=0, entry=q, carry=True)
    c = {n: np.concatenate(v) for n, v in cols.items()}
    P, VOID, BANK, SRC, ENTRY, CARRY = (c[n] for n in ("p", "void", "bank", "src", "entry", "carry"))
    P = P.astype(np.float32)
    idx = np.arange(len(P))
    p64 = P.astype(np.float64)
    left = {}
    for bank in range(total + 1):
        mine = idx[(BANK == bank) & (P > 0) & ~VOID]
        left[bank] = list(mine[np.lexsort((mine, -p64[mine]))])
    picked = []
    while len(picked) < beam and any(left.values()):           # phase 1: round robin from the fullest bank down
        for bank in range(total, -1, -1):
            if len(picked) < beam and left[bank]:
                picked.append((int(left[bank].pop(0)), 1))
    if len(picked) < beam:                                     # phase 2: fill
        taken = np.zeros(len(idx), dtype=bool)
        taken[[n for n, _ in picked]] = True
        rest = idx[~taken]
        rest = rest[np.lexsort((rest, -p64[rest]))]
        for n in rest[:beam - len(picked)]:
            assert not VOID[n], "a void candidate was reached"
            picked.append((int(n), 2))
    order = sorted(range(beam), key=lambda o: (not P[picked[o][0]] > 0, -int(BANK[picked[o][0]]), -float(P[picked[o][0]]), o))
    picks = []
    for o in order:
        n, phase = picked[o]
        picks.append(dict(src=int(SRC[n]), carry=bool(CARRY[n]), entry=int(ENTRY[n]), word=None if CARRY[n] else int(words[ENTRY[n]]),
                          p=np.float32(P[n]), bank=int(BANK[n]), phase=phase, index=n))
    return picks
