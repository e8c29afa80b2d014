"""Test-only statement of the contrastive-search selection (include/fira_hip.h: fira_contrastive_select) in plain numpy, one
commit at a time.  The reference project has no contrastive search, so this file is the definition the kernel is held to.

The cosines are formed in float64 (the kernel's fp32 sums are compared with a tolerance); everything after them follows the
header to the letter: the score's two products and its difference are separate float32 operations, the arg-max takes the
lowest slot on ties, the probability is one float32 product, and the new candidates are the k largest positive entries of the
picked row by (value descending, index ascending)."""
import numpy as np

F32 = np.float32
EOS = 1
D = 256


def cosine(a, c):
    """dot / (|a| |c|) in float64; 0 where a norm is 0."""
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    na, nc = float(a @ a), float(c @ c)
    if na == 0.0 or nc == 0.0:
        return 0.0
    return float(a @ c) / (np.sqrt(na) * np.sqrt(nc))


def similarities(hidden, hist):
    """sim[j] = max_i cos(hidden[j], hist[i]) over the rows of ``hist`` (the positions chosen so far); 0 with no history."""
    hist = np.asarray(hist).reshape(-1, D)
    return np.array([max((cosine(h, g) for g in hist), default=0.0) for h in np.asarray(hidden).reshape(-1, D)], dtype=np.float64)


def scores(p, sim, alpha):
    """fp32(fp32((1 - alpha) * p) - fp32(alpha * sim)), 1 - alpha formed in float32; sim is rounded to float32 first."""
    a = F32(alpha)
    one_minus = F32(F32(1.0) - a)
    p, sim = np.asarray(p, dtype=F32), np.asarray(sim).astype(F32)
    return (one_minus * p).astype(F32) - (a * sim).astype(F32)


def live(p):
    return np.asarray(p) > 0


def pick(score, p):
    """The live slot of the largest score, the lowest on ties; -1 without a live slot."""
    best = -1
    for j in range(len(score)):
        if live(p)[j] and (best < 0 or score[j] > score[best]):
            best = j
    return best


def entry_word(i, sou, sub, V):
    """The vocabulary id entry i resolves to: itself below V, the id of its copy slot above."""
    L = len(sou)
    return int(i) if i < V else int(sou[i - V]) if i < V + L else int(sub[i - V - L])


def top_positive(row, k):
    """The (index, value) of the k largest positive entries by (value descending, index ascending); fewer if fewer are positive."""
    row = np.asarray(row, dtype=F32)
    idx = [i for i in range(len(row)) if row[i] > 0]
    idx.sort(key=lambda i: (-float(row[i]), i))
    return [(i, row[i]) for i in idx[:k]]


def select(step, alpha, dist, hidden, fin, sou, sub, V, gen, length, p, prob, hist, ended):
    """One commit's selection.  dist [k, W], hidden [k, 256], fin [k], gen [k, T], length [k], p [k] float32, prob float32,
    hist [T, 256] (rows below ``step`` are read), ended 0 / 1.  Returns a dict: gen, length, p, prob, parent (slot within the
    commit), pick, sim, score (float64 / float32, 0 where the kernel writes 0), entries (the candidates' entry indices, -1 for a
    void slot), hist (a copy with row ``step`` appended) and ended."""
    k, T = gen.shape
    gen, length = np.array(gen, dtype=np.int64), np.array(length, dtype=np.int64)
    p, hist = np.array(p, dtype=F32), np.array(hist, dtype=F32)
    out = dict(gen=gen.copy(), length=length.copy(), p=p.copy(), prob=F32(prob), parent=np.arange(k), pick=-1,
               sim=np.zeros(k), score=np.zeros(k, dtype=F32), entries=[-1] * k, hist=hist, ended=int(ended))
    if ended:
        return out
    sim = similarities(hidden, hist[:step])
    sc = scores(p, sim, alpha)
    js = pick(sc, p)
    if js < 0:
        out["ended"] = 1
        return out
    out.update(pick=js, sim=np.where(live(p), sim, 0.0), score=np.where(live(p), sc, F32(0)).astype(F32),
               prob=F32(F32(prob) * p[js]), parent=np.full(k, js))
    hist[step] = np.asarray(hidden, dtype=F32).reshape(k, D)[js]
    if fin[js]:
        out["gen"][:], out["length"][:], out["p"][:], out["ended"] = gen[js], length[js], p[js], 1
        return out
    cands = top_positive(np.asarray(dist)[js], k)
    for m in range(k):
        out["gen"][m], out["length"][m], out["p"][m] = gen[js], length[js], F32(-1)
        if m < len(cands):
            i, v = cands[m]
            out["gen"][m, min(length[js], T - 1)] = entry_word(i, sou, sub, V)
            out["length"][m], out["p"][m], out["entries"][m] = length[js] + 1, v, i
    return out


def best_two_gap(score, p):
    """The gap between the two largest live scores (inf with fewer than two live slots): a test redraws below its threshold."""
    s = sorted((float(x) for x, l in zip(score, live(p)) if l), reverse=True)
    return s[0] - s[1] if len(s) >= 2 else float("inf")
