"""numpy twin of the stochastic beam search (csrc/beam_gumbel.hip, fira_beam_select_gumbel): one
selection step and a whole search over given distributions.  The noise is the sampler's (sample_ref: mix32, row_stream,
gumbel, bit for bit); scores and keys are float64.  A step also reports the smallest gap between adjacent keys among the
n + 1 best candidates of the commit: where it is below the comparison margin an fp32 implementation may order otherwise."""
from __future__ import annotations

import numpy as np

import sample_ref

EOS, START = 1, 2
NINF = -np.inf


def naive_key(G, Z, g):
    """-log(exp(-G) - exp(-Z) + exp(-g)): the key of an entry with perturbed value g in a row whose maximum is Z, conditioned on
    the parent's key G (float64; overflows or cancels where the stable form does not)."""
    with np.errstate(all="ignore"):
        return -np.log(np.exp(-G) - np.exp(-Z) + np.exp(-g))


def stable_key(G, Z, g):
    """The same value as  v = G - g + log1p(-exp(g - Z)),  G - max(0, v) - log1p(exp(-|v|)).  g >= Z (the row's maximum, or a
    tie with it) gives G.  No infinite operand reaches the formula: g = -inf (a void entry) or G = -inf (a void parent) gives
    -inf, never NaN."""
    G, Z, g = np.float64(G), np.float64(Z), np.atleast_1d(np.asarray(g, dtype=np.float64))
    out = np.full(g.shape, NINF)
    if not G > NINF:
        return out
    live = np.isfinite(g)
    out[live & (g >= Z)] = G
    low = live & (g < Z)
    v = G - g[low] + np.log1p(-np.exp(g[low] - Z))
    out[low] = G - np.maximum(0.0, v) - np.log1p(np.exp(-np.abs(v)))
    return out


def entry_word(w, sou, sub, V, L):
    return int(w) if w < V else int(sou[w - V]) if w < V + L else int(sub[w - V - L])


def select_step(dist, gen, length, phi, G, logp, sou, sub, V, key, seed, step, temperature):
    """One fira_beam_select_gumbel step of one commit.  dist [n, W] (any float dtype; read as it stands), gen [n, T] ids,
    length / phi / G / logp [n]; sou [L], sub [S] the commit's id rows; returns a dict with the new gen, length, phi, G, logp,
    parent (slot indices), `cand` (per new slot: (source slot, entry) of an extension, (source slot, -1) of a carried
    hypothesis, None of a void slot), `gap` (the smallest gap between adjacent keys among the n + 1 best candidates; inf with
    fewer than two) and `keys` (the sorted keys of all candidates)."""
    dist = np.asarray(dist)
    n, W = dist.shape
    T, L = gen.shape[1], len(sou)
    inv = np.float64(np.float32(1.0) / np.float32(temperature))      # the fp32 reciprocal the kernel multiplies by
    cands = []                                                       # (-key, class, index, slot, entry, phi, logp)
    n_carried = 0
    for j in range(n):
        fin = gen[j, length[j] - 1] == EOS
        if not G[j] > NINF:
            continue
        if fin:
            cands.append((-float(G[j]), 1, n * W + n_carried, j, -1, float(phi[j]), float(logp[j])))
            n_carried += 1
            continue
        p = dist[j].astype(np.float64)
        ok = (p > 0) & np.isfinite(p)
        if not ok.any():
            continue
        with np.errstate(all="ignore"):
            lp = np.where(ok, np.log(np.where(ok, p, 1.0)), NINF)
        u = lp * inv
        m = u[ok].max()
        lnZ = m + np.log(np.exp(u[ok] - m).sum())
        g = sample_ref.gumbel(sample_ref.row_stream(int(key), int(seed), j, T, step), W).astype(np.float64)
        s = np.where(ok, u + g, NINF)
        a = int(np.argmax(s))
        gi = (phi[j] - lnZ) + s
        k = stable_key(G[j], gi[a], gi)
        k[a] = G[j]
        for i in np.nonzero(ok)[0]:
            cands.append((-float(k[i]), 0 if i == a else 1, j * W + int(i), j, int(i), float(phi[j] + (u[i] - lnZ)),
                          float(logp[j] + lp[i])))
    cands.sort(key=lambda c: c[:3])
    keys = np.array([-c[0] for c in cands])
    head = keys[:n + 1]
    out = dict(gen=np.zeros_like(gen), length=np.ones(n, dtype=np.int64), phi=np.full(n, NINF), G=np.full(n, NINF),
               logp=np.full(n, NINF), parent=np.arange(n), cand=[None] * n, keys=keys,
               gap=float(np.min(head[:-1] - head[1:])) if len(head) > 1 else np.inf)
    out["gen"][:, 0] = START
    for c, (nk, _, _, j, i, ph, lp_) in enumerate(cands[:n]):
        out["gen"][c] = gen[j]
        out["length"][c] = length[j]
        if i >= 0:
            out["gen"][c, min(length[j], T - 1)] = entry_word(i, sou, sub, V, L)
            out["length"][c] = length[j] + 1
        out["phi"][c], out["G"][c], out["logp"][c], out["parent"][c], out["cand"][c] = ph, -nk, lp_, j, (j, i)
    return out


def initial_state(n, T):
    gen = np.zeros((n, T), dtype=np.int64)
    gen[:, 0] = START
    z = np.full(n, NINF)
    z[0] = 0.0
    return dict(gen=gen, length=np.ones(n, dtype=np.int64), phi=z.copy(), G=z.copy(), logp=z.copy())


def search(step_dist, n, T, sou, sub, V, key, seed, temperature):
    """A whole search of one commit: step_dist(step, gen, length) -> the [n, W] distributions of the step.  Returns the final
    state dict and the smallest key gap over the steps."""
    st, gap = initial_state(n, T), np.inf
    for step in range(T - 1):
        live = st["G"] > NINF
        if all(st["gen"][j, st["length"][j] - 1] == EOS for j in range(n) if live[j]) and live.any():
            break
        out = select_step(step_dist(step, st["gen"], st["length"]), st["gen"], st["length"], st["phi"], st["G"], st["logp"],
                          sou, sub, V, key, seed, step, temperature)
        gap = min(gap, out["gap"])
        st = {k: out[k] for k in ("gen", "length", "phi", "G", "logp")}
    return st, gap


# ------------------------------------------------------------------------------------------------ the kernel test's inputs
SMALL = dict(V=9, L=3, S=2, T=6)                 # W = 14: not a multiple of 4
N_BEAMS = (1, 2, 5, 8)
TEMPERATURES = (1.0, 0.7, 1.8)
CASE_B, CASE_STEP, CASE_SEED = 3, 2, 0x5B5C0FFEE
MARGIN = 1e-4                                    # log-space key gap below which a commit's order is not compared
# |device - twin| on phi, G and logp.  Every value is a short chain of fp32 operations (at most ~16 roundings from p to the key)
# on magnitudes below 32: 16 * 2^-24 * 32 = 3.1e-5; the twin itself is float64 on the same fp32 inputs.
TOLERANCE = 3.1e-5


def kernel_cases(model_dims=None):
    """The inputs of the kernel-against-twin test, shared by the CPU cap check and the GPU test: (name, dims, n, temperature,
    arrays) with arrays = dist [B * n, W] fp32, gen [B * n, T], length, phi, G, logp [B * n], sou [B, L], sub [B, S], key [B].
    Every state is one at step 2 (hypotheses of 3 ids).  Commit 0 has a finished slot and a copy slot with a generator entry's
    id, commit 1 a void slot and a row with a NaN entry, commit 2 is exhausted: one running row with 3 positive entries, every
    other slot void.  `model_dims` adds one case at that geometry with n = 8."""
    cases = [("small", SMALL, n, t) for n in N_BEAMS for t in TEMPERATURES]
    if model_dims is not None:
        cases.append(("model", model_dims, 8, 1.0))
    for ci, (name, d, n, temp) in enumerate(cases):
        rng = np.random.default_rng(1000 + ci)
        V, L, S, T = d["V"], d["L"], d["S"], d["T"]
        W, B = V + L + S, CASE_B
        dist = rng.random((B * n, W)) ** 4 + 1e-6
        dist[rng.random((B * n, W)) < 0.2] = 0.0
        dist /= dist.sum(1, keepdims=True)
        dist = dist.astype(np.float32)
        gen = np.zeros((B * n, T), dtype=np.int64)
        gen[:, 0] = START
        gen[:, 1:3] = rng.integers(3, V, (B * n, 2))
        length = np.full(B * n, 3, dtype=np.int64)
        phi = -rng.random((B, n)) * 8.0
        G = -np.sort(-(phi + rng.gumbel(size=(B, n))), axis=1)          # keys near phi, in slot order
        logp = phi * 1.25
        sou, sub = rng.integers(3, V, (B, L)), rng.integers(3, V, (B, S))
        sou[:, 0] = 4                                                    # the id of generator entry 4 on a copy slot
        phi, G, logp = phi.reshape(-1), G.reshape(-1), logp.reshape(-1)
        if n >= 2:
            gen[0 * n + 1, 2] = EOS                                      # commit 0: slot 1 is finished
            G[1 * n + n - 1] = phi[1 * n + n - 1] = logp[1 * n + n - 1] = NINF     # commit 1: the last slot is void
            gen[1 * n + n - 1, 1:] = 0
            length[1 * n + n - 1] = 1
        dist[1 * n, 5] = np.nan                                          # commit 1: a NaN entry in the first row
        for j in range(1, n):                                            # commit 2: exhausted
            r = 2 * n + j
            G[r] = phi[r] = logp[r] = NINF
            gen[r, 1:] = 0
            length[r] = 1
        keep = rng.choice(W, 3, replace=False)
        row = np.zeros(W, dtype=np.float32)
        row[keep] = np.array([0.5, 0.3, 0.2], dtype=np.float32)
        dist[2 * n] = row
        yield name, d, n, temp, dict(dist=dist, gen=gen, length=length, phi=phi.astype(np.float32).astype(np.float64),
                                     G=G.astype(np.float32).astype(np.float64),
                                     logp=logp.astype(np.float32).astype(np.float64), sou=sou, sub=sub,
                                     key=np.array([7, 11, 13]))


def twin_of_case(d, n, temp, a):
    """select_step for every commit of a case: a list of B result dicts."""
    res = []
    for b in range(CASE_B):
        r = slice(b * n, (b + 1) * n)
        res.append(select_step(a["dist"][r], a["gen"][r], a["length"][r], a["phi"][r], a["G"][r], a["logp"][r], a["sou"][b],
                               a["sub"][b], d["V"], int(a["key"][b]), CASE_SEED, CASE_STEP, temp))
    return res
