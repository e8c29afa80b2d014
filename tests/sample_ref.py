"""numpy twin of the on-device sampler (csrc/sample.hip, fira_decode_step_sample): the counter-hash noise bit for bit,
and the filters (temperature, top-k, top-p) in float64 on the kernel's own distribution row."""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def row_stream(key: int, seed: int, j: int, tar_len: int, step: int) -> int:
    """The noise stream of sample j of the commit with `key` at `step`."""
    seed &= (1 << 64) - 1
    inner = mix32((seed >> 32) + 0x632BE5AB)
    base = mix32((key & M32) ^ int(mix32((seed & M32) ^ int(inner))))
    return int(mix32((int(base) + 0x9E3779B9 * ((j * tar_len + step + 1) & M32)) & M32))


def gumbel(stream: int, n: int) -> np.ndarray:
    """g_i = -log(-log(u_i)) for the entries 0..n-1 of a row, in float32 like the kernel."""
    h = mix32(np.arange(n, dtype=np.uint64) ^ np.uint64(stream))
    u = ((h >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    u = np.minimum(u, np.nextafter(np.float32(1), np.float32(0)))
    return -np.log(-np.log(u))


def thresholds(p: np.ndarray, temperature: float, top_k: int, top_p: float, mass_slack: float = 0.0) -> float:
    """The p-space threshold of the kept set {p_i >= tau} (float64): top-k on p counted with multiplicity, then top-p on
    q ~ p^(1/T) renormalised over what top-k kept -- the largest tau whose upper set holds >= top_p (+ mass_slack) of it."""
    p = np.asarray(p, dtype=np.float64)
    tau = 0.0
    if top_k > 0:
        tau = np.sort(p)[::-1][top_k - 1]
    if top_p < 1.0:
        kept = p[p >= tau]
        vals = np.sort(np.unique(kept))[::-1]
        w = (kept / kept.max()) ** (1.0 / temperature)
        z = w.sum()
        # mass of the upper set of every distinct value, largest value first
        order = np.argsort(-kept, kind="stable")
        ks, ws = kept[order], np.cumsum(w[order])
        last = np.searchsorted(-ks, -vals, side="right") - 1          # last position holding a value >= v
        mass = ws[last]
        need = min(top_p + mass_slack, 1.0) * z
        hit = np.nonzero(mass >= need * (1 - 1e-12))[0]
        tau = max(tau, vals[hit[0]] if len(hit) else vals[-1])
    return float(tau)


def kept_mask(p, temperature, top_k, top_p, rel=0.0):
    """Entries the filters keep; rel > 0 relaxes the boundary (threshold and top-p mass) by that relative amount."""
    p = np.asarray(p, dtype=np.float64)
    tau = thresholds(p, temperature, top_k, top_p, mass_slack=rel if rel else 0.0)
    return p >= tau * (1 - rel)


def filtered_q(p, temperature, top_k, top_p):
    """The sampling distribution: q ~ p^(1/T) on the kept set, renormalised (float64)."""
    p = np.asarray(p, dtype=np.float64)
    keep = kept_mask(p, temperature, top_k, top_p) & (p > 0)
    q = np.where(keep, (p / p.max()) ** (1.0 / temperature), 0.0)
    return q / q.sum(), keep


def gumbel_argmax(p, keep, temperature, g):
    """(arg-max, gap to the runner-up) of log p / T + g over the kept entries (float64 scores)."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore"):
        s = np.where(keep & (p > 0), np.log(p) / temperature + g.astype(np.float64), -np.inf)
    i = int(np.argmax(s))
    top2 = np.sort(s)[-2:]
    return i, float(top2[1] - top2[0])
