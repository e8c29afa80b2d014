"""Test-only statement of token-level retrieval (include/fira_hip.h: fira_knn_search, fira_mix_knn; retrieve.TokenStore) in plain
numpy.  Nothing here is imported by the package."""
import numpy as np

F = np.float32


def sum_sq(x):
    """The sum of squares of a row in ascending column order, every multiply and add rounded to fp32."""
    s = F(0)
    for v in np.asarray(x, dtype=F):
        s = F(s + F(v * v))
    return s


def sum_sq_rows(x):
    """``sum_sq`` of every row of x [N, C]: numpy's cumulative sum adds in ascending order, one fp32 operation each."""
    x = np.asarray(x, dtype=F)
    return np.cumsum((x * x).astype(F), axis=1, dtype=F)[:, -1]


def dot_chain(q, key):
    """<q, key> as the kernels form it: one ordered fp32 fma chain over the columns in fira_nn_search's fixed permutation
    (for m = 0..15, for c = 0..3, for g = 0..3: column 16 m + 4 g + c).  The same chain for every row, so identical keys tie."""
    acc = np.float64(0)
    q, key = np.asarray(q, dtype=F), np.asarray(key, dtype=F)
    for m in range(16):
        for c in range(4):
            for g in range(4):
                k = 16 * m + 4 * g + c
                acc = np.float64(F(np.float64(q[k]) * np.float64(key[k]) + acc))      # one fma: exact product, one rounding
    return F(acc)


def knn_search(Q, keys, key_sq, K, owner=None, exclude=None, exact=False):
    """(idx [R, K] int32, d2 [R, K] float32).  ``exact``: the products as a float64 matrix product rounded to fp32 -- the chain's
    value wherever every partial sum is an integer below 2^24 (the tests' integer entries)."""
    Q, keys, key_sq = np.asarray(Q, dtype=F), np.asarray(keys, dtype=F), np.asarray(key_sq, dtype=F)
    R, N = Q.shape[0], keys.shape[0]
    idx = np.full((R, K), -1, dtype=np.int32)
    d2 = np.full((R, K), np.inf, dtype=F)
    if exact:
        dots = (Q.astype(np.float64) @ keys.astype(np.float64).T).astype(F)
    for r in range(R):
        dot = dots[r] if exact else np.array([dot_chain(Q[r], keys[j]) for j in range(N)], dtype=F)
        with np.errstate(invalid="ignore", over="ignore"):
            s = (key_sq - F(2) * dot).astype(F)
        ok = ~np.isnan(s)
        if owner is not None and exclude is not None:
            ok &= np.asarray(owner) != int(exclude[r])
        cand = np.nonzero(ok)[0]
        order = cand[np.lexsort((cand, s[cand]))][:K]             # s ascending, then j ascending
        q_sq = sum_sq(Q[r])
        idx[r, :len(order)] = order
        with np.errstate(invalid="ignore", over="ignore"):
            d2[r, :len(order)] = np.maximum(F(0), (q_sq + s[order]).astype(F))
    return idx, d2


def mix_weights(idx, d2, inv_T, N):
    """The weights of one row's slots in float64 (0 in the void slots); None when every slot is void."""
    idx, d2 = np.asarray(idx), np.asarray(d2, dtype=np.float64)
    live = (idx >= 0) & (idx < N)
    if not live.any():
        return None
    e = np.where(live, np.exp(-(np.where(live, d2, 0.0) - d2[0]) * float(inv_T)), 0.0)
    return e / e.sum()


def mix_knn(dist, idx, d2, values, lam, inv_T):
    """The rows after fira_mix_knn: (the row in fp32 arithmetic with float64 weights rounded once -- the statement the kernel's
    touched entries are held to within a tolerance --, the mask of touched entries)."""
    dist = np.array(dist, dtype=F, copy=True)
    touched = np.zeros(dist.shape, dtype=bool)
    lam32 = F(lam)
    if lam32 == 0:
        return dist, touched
    a = F(F(1) - lam32)
    for r in range(dist.shape[0]):
        w = mix_weights(idx[r], d2[r], inv_T, len(values))
        if w is None:
            continue
        dist[r] = (a * dist[r]).astype(F)
        for k in range(idx.shape[1]):
            if 0 <= idx[r, k] < len(values):
                v = int(values[idx[r, k]])
                if 0 <= v < dist.shape[1]:
                    dist[r, v] = F(dist[r, v] + F(lam32 * F(w[k])))
                    touched[r, v] = True
    return dist, touched


def mix_knn_f64(dist, idx, d2, values, lam, inv_T):
    """The same in float64 throughout, from the fp32 inputs (lam and inv_T as the fp32 values the kernel reads)."""
    out = np.array(dist, dtype=np.float64, copy=True)
    lam, inv_T = float(F(lam)), float(F(inv_T))
    if lam == 0:
        return out
    for r in range(out.shape[0]):
        w = mix_weights(idx[r], d2[r], inv_T, len(values))
        if w is None:
            continue
        out[r] *= float(F(F(1) - F(lam)))
        for k in range(idx.shape[1]):
            if 0 <= idx[r, k] < len(values) and 0 <= int(values[idx[r, k]]) < out.shape[1]:
                out[r, int(values[idx[r, k]])] += lam * w[k]
    return out


def resolve_labels(tar_label, sou, sub_token, vocab):
    """The vocabulary id every label of tar_label [B, T] stands for: itself below ``vocab``, else the id of the diff slot
    (label - vocab < sou_len) or of the sub-token slot it addresses -- fira_merge_dist's rule for an entry."""
    tar_label, sou, sub_token = np.asarray(tar_label), np.asarray(sou), np.asarray(sub_token)
    L = sou.shape[1]
    out = np.array(tar_label, dtype=np.int64, copy=True)
    for b in range(out.shape[0]):
        for t in range(out.shape[1]):
            e = int(tar_label[b, t])
            if e >= vocab + L:
                out[b, t] = sub_token[b, e - vocab - L]
            elif e >= vocab:
                out[b, t] = sou[b, e - vocab]
    return out


def store_rows(tar_label, sou, sub_token, vocab, commits):
    """The rows of a batch in the store's order, step-major as ``TokenStore.build`` appends them: for t = 0, 1, ..., for
    every commit b with a word at t + 1 (label != 0): value =
    the resolved label at t + 1, owner = commits[b].  Returns (b [n], t [n], value [n], owner [n])."""
    words = resolve_labels(tar_label, sou, sub_token, vocab)
    lab = np.asarray(tar_label)
    bs, ts, vs, os_ = [], [], [], []
    for t in range(lab.shape[1] - 1):
        for b in range(lab.shape[0]):
            if lab[b, :t + 2].all():                              # positions 0 .. t + 1 hold words: t < len_b - 1
                bs.append(b), ts.append(t), vs.append(int(words[b, t + 1])), os_.append(int(commits[b]))
    return np.array(bs, np.int64), np.array(ts, np.int64), np.array(vs, np.int32), np.array(os_, np.int32)
