"""Test-only statement of the length-normalised, group-diverse beam selection (include/fira_hip.h: fira_beam_select_scored) in
plain numpy, for ONE commit and ONE step: float64 keys on fp32 products.  Not part of the product.

    key(p, m) = ln(p) * inv_lp[m],  inv_lp[m] = fp32(1 / ((5 + m) / 6)^alpha),  m = words emitted = length - 1,  ln 0 = -inf
    running candidate  entry i of running slot j: p = fp32(dist[j, i] * prob[j]), m = len_j
    carried candidate  a finished hypothesis:     p = prob[j],                    m = len_j - 1
    void               entries of a finished hypothesis's row, padding of the carried list
    order              void last, penalised key descending, p descending, flattened index ascending
    groups             G groups of k consecutive slots in ascending order; group g picks its k best among its own slots'
                       candidates; a running candidate's penalised key is key - lam * c, c = earlier groups' picks of this step
                       that EXTENDED a hypothesis with the same word (multiplicity counts); carried: never penalised, no count
"""
import numpy as np

EOS = 1


def inv_lp_table(alpha, tar_len):
    return np.array([1.0 / ((5.0 + m) / 6.0) ** float(alpha) for m in range(tar_len + 1)], dtype=np.float64).astype(np.float32)


def words_of(sou_row, sub_row, V):
    """w(i) for every entry i of a row: the generator id, or the id of the copy slot."""
    return np.concatenate([np.arange(V, dtype=np.int64), np.asarray(sou_row, dtype=np.int64), np.asarray(sub_row, dtype=np.int64)])


def key64(p, inv):
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(p > 0, np.log(np.where(p > 0, p, 1.0)) * np.float64(inv), -np.inf)


def group_candidates(dist, fin, active, prob, length, words, inv_lp, g, k, lam, counts):
    """The candidates of group g in flattened-index order, as arrays: void, pkey (penalised), key, p (fp32), src (slot), entry
    (-1 for the carried list), carry.  ``counts``: word -> picks of earlier groups that extended with it."""
    W = dist.shape[1]
    T = len(inv_lp) - 1
    slots = range(g * k, g * k + k)
    cnt = np.array([counts.get(int(w), 0) for w in words], dtype=np.float64) if counts else np.zeros(W)
    out = {n: [] for n in ("void", "pkey", "key", "p", "src", "entry", "carry")}

    def add(void, pkey, key, p, src, entry, carry):
        for n, v in zip(("void", "pkey", "key", "p", "src", "entry", "carry"), (void, pkey, key, p, src, entry, carry)):
            out[n].append(np.broadcast_to(np.asarray(v), np.shape(p)).reshape(-1))

    for j in slots:                                            # running slots in slot order
        if not active[j]:
            continue
        if fin[j]:
            add(True, -np.inf, -np.inf, np.full(W, -1.0, dtype=np.float32), j, np.arange(W), False)
            continue
        p = (dist[j].astype(np.float32) * np.float32(prob[j])).astype(np.float32)
        key = key64(p, inv_lp[min(max(int(length[j]), 0), T)])
        add(False, key - np.float64(np.float32(lam)) * cnt, key, p, j, np.arange(W), False)
    n_fin = 0
    for j in slots:                                            # the carried list: finished hypotheses, slot order
        if fin[j]:
            p = np.array([prob[j]], dtype=np.float32)
            key = key64(p, inv_lp[min(max(int(length[j]) - 1, 0), T)])
            add(False, key, key, p, j, -1, True)
            n_fin += 1
    for _ in range(k - n_fin):                                 # its padding
        add(True, -np.inf, -np.inf, np.array([-1.0], dtype=np.float32), g * k, -1, True)
    return {n: np.concatenate(v) for n, v in out.items()}


def best_order(c):
    """Indices of the candidates in the total order."""
    idx = np.arange(len(c["p"]))
    return np.lexsort((idx, -c["p"].astype(np.float64), -c["pkey"], c["void"]))


def select(dist, fin, active, prob, length, words, inv_lp, groups, lam):
    """The picks of one commit and step: a list over the beam slots of dicts (src, carry, entry, word, p, pkey, key)."""
    beam = dist.shape[0]
    k = beam // groups
    counts, picks = {}, []
    for g in range(groups):
        c = group_candidates(dist, fin, active, prob, length, words, inv_lp, g, k, lam, counts)
        new = []
        for n in best_order(c)[:k]:
            carry, entry = bool(c["carry"][n]), int(c["entry"][n])
            new.append(dict(src=int(c["src"][n]), carry=carry, entry=entry, word=None if carry else int(words[entry]),
                            p=np.float32(c["p"][n]), pkey=float(c["pkey"][n]), key=float(c["key"][n]), void=bool(c["void"][n])))
        for pk in new:                                         # counted only once the group is complete
            if not pk["carry"]:
                counts[pk["word"]] = counts.get(pk["word"], 0) + 1
        picks += new
    return picks


def apply(picks, gen, length, inv_lp):
    """The state the picks leave: (gen_out, len_out, prob_out, parent (slot), key_out float64)."""
    beam, T = gen.shape
    g_out, l_out = np.zeros_like(gen), np.zeros_like(length)
    p_out, parent, key = np.zeros(beam, dtype=np.float32), np.zeros(beam, dtype=np.int64), np.zeros(beam, dtype=np.float64)
    for o, pk in enumerate(picks):
        src = pk["src"]
        g_out[o] = gen[src]
        l_out[o] = length[src]
        if not pk["carry"]:
            g_out[o, min(int(length[src]), T - 1)] = pk["word"]
            l_out[o] = length[src] + 1
        p_out[o], parent[o] = pk["p"], src
        key[o] = key64(pk["p"], inv_lp[min(max(int(l_out[o]) - 1, 0), T)])
    return g_out, l_out, p_out, parent, key


TOL = 1e-4      # |ln p| <= 104 for a positive fp32; a few ulp of the device logarithm there (2.5e-5), the table's and the
                # product's rounding (6e-6 each, inv_lp <= 1 for m >= 1), lam <= 2: well inside 1e-4


def check_step(dist, fin, active, prob, length, gen, words, inv_lp, groups, lam, got, tol=TOL):
    """Validity of a device step WITHOUT excluding anything, for one commit: ``got`` = (gen_out, len_out, prob_out, parent (slot
    within the commit), key_out) as numpy.  Every pick must be a real candidate of its group (bit-exact fp32 product with an entry
    that resolves to the appended word, or the carried probability), no entry is used more often than it exists, every pick's
    float64 penalised key reaches the reference's k-th best (under the counts of the device's own earlier picks) within ``tol``,
    the picks of a group do not increase by more than ``tol``, and key_out is ln(prob) * inv_lp within ``tol``."""
    g_out, l_out, p_out, parent, key_out = got
    beam, W = dist.shape
    T = gen.shape[1]
    k = beam // groups
    counts = {}
    lam64 = np.float64(np.float32(lam))
    for g in range(groups):
        c = group_candidates(dist, fin, active, prob, length, words, inv_lp, g, k, lam, counts)
        kth = c["pkey"][best_order(c)[k - 1]]
        used, new_words, last = {}, [], np.inf
        for o in range(g * k, g * k + k):
            src = int(parent[o])
            assert g * k <= src < g * k + k, ("parent outside the group", g, o, src)
            p_bits = np.float32(p_out[o]).tobytes()
            if fin[src]:                                       # carried
                assert p_bits == np.float32(prob[src]).tobytes() and l_out[o] == length[src], ("carried", g, o)
                assert (g_out[o] == gen[src]).all()
                unit, n_exist, pkey = ("carry", src), 1, float(key64(prob[src], inv_lp[min(max(int(length[src]) - 1, 0), T)]))
            else:
                assert active[src], ("extends a slot that does not run", g, o, src)
                at = min(int(length[src]), T - 1)
                word = int(g_out[o, at])
                assert l_out[o] == length[src] + 1 and (np.delete(g_out[o], at) == np.delete(gen[src], at)).all(), ("extended", g, o)
                prods = (dist[src].astype(np.float32) * np.float32(prob[src])).astype(np.float32)
                same = (words == word) & (prods.view(np.int32) == np.float32(p_out[o]).view(np.int32))
                n_exist = int(same.sum())
                assert n_exist >= 1, ("no entry of the word has this product", g, o, word, float(p_out[o]))
                unit = (src, word, p_bits)
                pkey = float(key64(p_out[o], inv_lp[min(max(int(length[src]), 0), T)])) - lam64 * counts.get(word, 0)
                new_words.append(word)
            used[unit] = used.get(unit, 0) + 1
            assert used[unit] <= n_exist, ("an entry is used more often than it exists", g, o, unit)
            assert pkey >= kth - tol, ("below the reference's k-th best", g, o, pkey, float(kth))
            assert pkey <= last + tol, ("picks increase", g, o, pkey, last)
            last = pkey
            want_key = float(key64(p_out[o], inv_lp[min(max(int(l_out[o]) - 1, 0), T)]))
            assert (want_key == key_out[o]) or abs(want_key - float(key_out[o])) <= tol, ("key_out", g, o, want_key, float(key_out[o]))
        for w in new_words:
            counts[w] = counts.get(w, 0) + 1
