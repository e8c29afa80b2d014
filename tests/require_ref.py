"""Test-only statement of the beam selection with required words (include/fira_hip.h: fira_beam_select_required) in plain
numpy / Python, for ONE commit and ONE step.  Not part of the product.  The products are np.float32 multiplies, as the kernel
forms them, so a comparison with the device is exact.

    C = n_required clamped to 0..4, R_k = required[k] for k < C
    met(h)   = { k : R_k among gen[1 .. length - 1] },  bank(h) = |met(h)|
    running   entry i of running slot j: p = fp32(dist[j, i] * prob[j]), bank = |met(h_j) u { k : R_k == w(i) }|
    carried   a finished hypothesis: p = prob[j], bank = bank(h_j)
    void      the row of a finished hypothesis, the padding of the carried list, and every entry with w(i) == <eos> of a
              running row with bank(h_j) < C
    phase 1   candidates with p > 0, ranked within a bank by (p descending, index ascending): repeat "for c = C .. 0: pick the
              best unpicked of bank c if there is one" until beam picks are made or none is left
    phase 2   the free slots take the remaining candidates by (value descending with void = -1, index ascending)
    written   sorted by (p > 0 first, bank descending, p descending, pick order ascending)
"""
import numpy as np

EOS = 1
MAX_REQUIRED = 4


def words_of(sou_row, sub_row, V):
    """w(i) for every entry i of a row: the generator id, or the id of the copy slot."""
    return np.concatenate([np.arange(V, dtype=np.int64), np.asarray(sou_row, dtype=np.int64), np.asarray(sub_row, dtype=np.int64)])


def required_of(required_row, n_required):
    """R_0 .. R_{C-1} of a commit from its device row and count (clamped as the kernel clamps it)."""
    C = min(max(int(n_required), 0), MAX_REQUIRED)
    return [int(w) for w in list(required_row)[:C]]


def met_set(gen_row, length, req):
    T = len(gen_row)
    n = min(max(int(length), 1), T)
    have = set(int(g) for g in gen_row[1:n])
    return frozenset(k for k, w in enumerate(req) if w in have)


def candidates(dist, fin, active, prob, length, gen, words, req):
    """The candidates of one commit in flattened-index order, as arrays: p (fp32; -1 where void), void, bank, src (slot), entry
    (the index in the carried list for a carried one), carry."""
    beam, W = dist.shape
    C = len(req)
    met = [met_set(gen[j], length[j], req) for j in range(beam)]
    promo = [np.array([w == r for w in words.tolist()]) for r in req]          # entry carries R_k
    cols = {n: [] for n in ("p", "void", "bank", "src", "entry", "carry")}

    def add(**kw):
        n = len(kw["p"])
        for name, v in kw.items():
            cols[name].append(np.broadcast_to(np.asarray(v), (n,)).copy())

    for j in range(beam):                                      # running slots in slot order
        if not active[j]:
            continue
        if fin[j]:
            add(p=np.full(W, -1.0, dtype=np.float32), void=True, bank=-1, src=j, entry=np.arange(W), carry=False)
            continue
        p = (dist[j].astype(np.float32) * np.float32(prob[j])).astype(np.float32)
        bank = np.full(W, 0, dtype=np.int64)
        for k in range(C):
            bank += (promo[k] | (k in met[j])).astype(np.int64)
        void = (words == EOS) & (len(met[j]) < C)
        add(p=np.where(void, np.float32(-1.0), p).astype(np.float32), void=void, bank=np.where(void, -1, bank), src=j,
            entry=np.arange(W), carry=False)
    n_fin = 0
    for j in range(beam):                                      # the carried list: finished hypotheses, slot order
        if fin[j]:
            add(p=np.array([prob[j]], dtype=np.float32), void=False, bank=len(met[j]), src=j, entry=n_fin, carry=True)
            n_fin += 1
    for q in range(n_fin, beam):                               # its padding
        add(p=np.array([-1.0], dtype=np.float32), void=True, bank=-1, src=0, entry=q, carry=True)
    return {n: np.concatenate(v) for n, v in cols.items()}


def select(dist, fin, active, prob, length, gen, words, req):
    """The picks of one commit and step in WRITTEN order: a list over the beam slots of dicts (src, carry, entry, word, p, bank,
    phase, index = the flattened index)."""
    beam = dist.shape[0]
    C = len(req)
    c = candidates(dist, fin, active, prob, length, gen, words, req)
    idx = np.arange(len(c["p"]))
    p64 = c["p"].astype(np.float64)
    left = {}                                                  # bank -> its positive candidates, best first
    for bank in range(C + 1):
        mine = idx[(c["bank"] == bank) & (c["p"] > 0) & ~c["void"]]
        left[bank] = list(mine[np.lexsort((mine, -p64[mine]))])
    picked = []
    while len(picked) < beam and any(left.values()):           # phase 1
        for bank in range(C, -1, -1):
            if len(picked) < beam and left[bank]:
                picked.append((int(left[bank].pop(0)), 1))
    if len(picked) < beam:                                     # phase 2
        taken = np.zeros(len(idx), dtype=bool)
        taken[[n for n, _ in picked]] = True
        rest = idx[~taken]
        rest = rest[np.lexsort((rest, -p64[rest]))]
        for n in rest[:beam - len(picked)]:
            assert not c["void"][n], "a void candidate was reached"
            picked.append((int(n), 2))
    order = sorted(range(beam), key=lambda o: (not c["p"][picked[o][0]] > 0, -int(c["bank"][picked[o][0]]),
                                               -float(c["p"][picked[o][0]]), o))
    picks = []
    for o in order:
        n, phase = picked[o]
        carry, entry = bool(c["carry"][n]), int(c["entry"][n])
        picks.append(dict(src=int(c["src"][n]), carry=carry, entry=entry, word=None if carry else int(words[entry]),
                          p=np.float32(c["p"][n]), bank=int(c["bank"][n]), phase=phase, index=n))
    return picks


def apply(picks, gen, length):
    """The state the picks leave: (gen_out, len_out, prob_out, parent (slot), met)."""
    beam, T = gen.shape
    g_out, l_out = np.zeros_like(gen), np.zeros_like(length)
    p_out, parent, met = np.zeros(beam, dtype=np.float32), np.zeros(beam, dtype=np.int64), np.zeros(beam, dtype=np.int64)
    for o, pk in enumerate(picks):
        src = pk["src"]
        g_out[o] = gen[src]
        l_out[o] = length[src]
        if not pk["carry"]:
            g_out[o, min(int(length[src]), T - 1)] = pk["word"]
            l_out[o] = length[src] + 1
        p_out[o], parent[o], met[o] = pk["p"], src, pk["bank"]
    return g_out, l_out, p_out, parent, met


def step(dist, fin, active, prob, length, gen, sou_row, sub_row, V, required_row, n_required):
    """select + apply from the device's own inputs of one commit."""
    words = words_of(sou_row, sub_row, V)
    return apply(select(dist, fin, active, prob, length, gen, words, required_of(required_row, n_required)), gen, length)


def count_met(message, req):
    """How many of ``req`` occur in a message (ids after <start>)."""
    have = set(int(w) for w in message[1:])
    return sum(1 for w in req if w in have)
