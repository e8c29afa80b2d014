"""numpy twin (float64) of the truncation cuts of fira_decode_step_sample_cut (csrc/sample.hip): min-p, epsilon, eta and
locally typical sampling on top of the sampler's own filters, whose twin is sample_ref (imported, not repeated).

q is the tempered distribution p^(1/T) renormalised over the entries top-k and then top-p kept; H = -sum q ln q over them.
    min_p      keep q_i >= min_p * max q
    epsilon    keep q_i >= epsilon
    eta        keep q_i >= min(eta, sqrt(eta) * exp(-H))
    typical_p  s_i = |-ln q_i - H|; keep s_i <= sigma, sigma the smallest value whose lower set holds >= typical_p of the mass
Every cut keeps the row's maximum with its ties; an entry with p = 0 is never kept.

Like sample_ref.kept_mask(rel=) every set comes strict and relaxed.  The relaxed one loosens each boundary by the relative
amount ``rel``: the filters' as sample_ref does, a lower threshold on q by the factor (1 - rel) and on the smaller of the two
thresholds that the strict and the relaxed filter set give (Z and H move with the set), the typical mass by + rel and the
band's edge by rel * (|ln q_i| + H) -- s is a difference, and the device's fp32 rounding is relative to its operands."""
from __future__ import annotations

import numpy as np

import sample_ref


def tempered(p, base, temperature):
    """(w, q): w_i = (p_i / max p)^(1/T) on ``base`` (0 elsewhere) and q = w / sum w."""
    p = np.asarray(p, dtype=np.float64)
    w = np.where(base & (p > 0), (p / p.max()) ** (1.0 / temperature), 0.0)
    return w, w / w.sum()


def entropy(q) -> float:
    """H = -sum q ln q; an entry with q = 0 contributes 0."""
    q = np.asarray(q, dtype=np.float64)
    nz = q > 0
    return float(-(q[nz] * np.log(q[nz])).sum())


def eta_threshold(eta: float, H: float) -> float:
    return min(eta, np.sqrt(eta) * np.exp(-H))


def lower_threshold(q, min_p=0.0, epsilon=0.0, eta=0.0) -> float:
    """The q-space threshold of the three lower cuts together: the largest one decides."""
    thr = max(min_p * float(np.max(q)), epsilon)
    if eta > 0:
        thr = max(thr, eta_threshold(eta, entropy(q)))
    return thr


def typical_sigma(q, typical_p: float) -> float:
    """The smallest sigma whose lower set {s_i <= sigma} holds at least typical_p of the mass (ties at sigma included)."""
    nz = q > 0
    s = np.abs(-np.log(q[nz]) - entropy(q))
    order = np.argsort(s, kind="stable")
    ss, mass = s[order], np.cumsum(q[nz][order])
    vals = np.unique(ss)
    last = np.searchsorted(ss, vals, side="right") - 1                  # last position holding a value <= v
    hit = np.nonzero(mass[last] >= min(typical_p, 1.0) * (1 - 1e-12))[0]
    return float(vals[hit[0]] if len(hit) else vals[-1])


def kept_sets(p, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, epsilon=0.0, eta=0.0, typical_p=1.0, rel=1e-4):
    """(strict, relaxed) boolean masks of the entries the filters and the cuts keep."""
    p = np.asarray(p, dtype=np.float64)
    if typical_p < 1 and (top_p < 1 or min_p > 0 or epsilon > 0 or eta > 0):
        raise ValueError("typical_p combines with temperature and top_k only")
    top = (p == p.max())
    base_s = sample_ref.kept_mask(p, temperature, top_k, top_p) & (p > 0)
    base_r = sample_ref.kept_mask(p, temperature, top_k, top_p, rel=rel) & (p > 0)
    w_s, q_s = tempered(p, base_s, temperature)
    w_r, q_r = tempered(p, base_r, temperature)
    if typical_p < 1:
        H = entropy(q_s)
        with np.errstate(divide="ignore"):
            nlq = np.where(q_s > 0, -np.log(np.where(q_s > 0, q_s, 1.0)), np.inf)
        s = np.abs(nlq - H)
        strict = base_s & (s <= typical_sigma(q_s, typical_p))
        sigma_r = typical_sigma(q_s, min(typical_p + rel, 1.0))
        relaxed = base_s & (s <= sigma_r * (1 + rel) + rel * (np.where(np.isfinite(nlq), nlq, 0.0) + H))
        return strict | top, relaxed | strict | top
    if min_p > 0 or epsilon > 0 or eta > 0:
        thr_s = lower_threshold(q_s, min_p, epsilon, eta)
        thr_r = lower_threshold(q_r, min_p, epsilon, eta)
        strict = base_s & (q_s >= thr_s)
        # in w-space (q Z), where the strict and the relaxed filter set share one scale
        thr_w = min(thr_s * w_s.sum(), thr_r * w_r.sum()) * (1 - rel)
        relaxed = base_r & (w_r >= thr_w)
        return strict | top, relaxed | strict | top
    return base_s | top, base_r | top


def cut_q(p, temperature=1.0, **kw):
    """(q, strict, relaxed): the sampling distribution q ~ p^(1/T) renormalised over the strict kept set."""
    strict, relaxed = kept_sets(p, temperature, **kw)
    _, q = tempered(p, strict, temperature)
    return q, strict, relaxed
