"""Operands OFF unit scale for the nonlinear kernels, and fp64 / fp32 statements of the same formulas.

The per-kernel suites draw every operand from randn() at a scale of 0.03 .. 2: no soft-max has a dominant entry, no exponential
underflows, no tanh saturates, no LayerNorm row has a mean far from zero, no probability is near the loss clamp.  The builders
here reach those edges.  Every reference takes a dtype: evaluated in float64 it is ``want``; evaluated in float32 with the same
plain torch ops it is ``plain32``, whose own error ``e32`` is the yardstick (a kernel is held to 3 * e32 + t0, t0 the unit-scale
tolerance of its existing test).  Pure torch: runs on any device, tests/test_ranges.py checks the fixtures on the CPU.
"""
import math

import torch
import torch.nn.functional as F

H, DH, D = 8, 32, 256


# ---------------------------------------------------------------------------------------------------------------- error measures
def rel_err(a, b):
    """Frobenius ratio over the whole tensor: for weight-shaped reductions only (one wrong row of many hides in it)."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _rows(t):
    return t.double().reshape(-1, t.shape[-1]) if t.dim() > 1 else t.double().reshape(-1, 1)


def row_errs(got, want, floor):
    """Per row r: |got_r - want_r| / max(|want_r|, floor_r), in fp64.  ``floor`` (a number or one value per row) is the
    absolute scale below which a row is compared absolutely."""
    g, w = _rows(got), _rows(want)
    fl = torch.as_tensor(floor, dtype=torch.float64, device=w.device).reshape(-1)
    return (g - w).norm(dim=1) / torch.maximum(w.norm(dim=1), fl.expand(w.shape[0]) if fl.numel() == 1 else fl)


def row_err(got, want, floor):
    e = row_errs(got, want, floor)
    return float(e.max()) if e.numel() else 0.0


def randn(*shape, seed=0, scale=1.0, device="cpu"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(device)


def r16(t):
    """bf16 rounding of a product's operand, kept in the dtype of the computation"""
    return t.float().bfloat16().to(t.dtype)


# ---------------------------------------------------------------------------------------------------------------- 1. attention
ATT_REGIMES = ("sharp", "flat", "planted", "common")
ATT_SHAPES = ((7, 33, False), (30, 70, False), (30, 30, True), (7, 7, True))   # (Tq, Tk, causal): one / three key tiles


def attention_case(regime, Tq, Tk, causal, device="cpu", B=3):
    """q, k, v, do [B, T, 256] fp32, key_valid [B, Tk] with holes (position 0 valid).
      sharp    q, k at scale 6: per-head scores of std ~36, nearly one-hot rows
      flat     q, k at scale 1e-3: uniform rows
      planted  every row has ONE key whose score exceeds the others by > 120: all other probabilities are exactly 0 in fp32.
               Per head u_h is a unit vector; key 0 carries +200 u_h, key j2 carries -400 u_h, query rows a component +-6 u_h:
               rows with +6 see key 0 at ~212 (key j2 at -424), rows with -6 see key j2 at ~424 (key 0 at -212); everything
               else is |score| < 30.  Causal: only rows t >= j2 take the minus sign.
      common   q += 8 u, k += 8 u (u_h a unit vector per head): every score of a row carries the same offset 8 q.u_h + 64"""
    q = randn(B, Tq, D, seed=1, device=device)
    k = randn(B, Tk, D, seed=2, device=device)
    v = randn(B, Tk, D, seed=3, device=device)
    do = randn(B, Tq, D, seed=5, device=device)
    g = torch.Generator().manual_seed(4)
    valid = (torch.rand(B, Tk, generator=g) > 0.3).to(torch.int32)
    valid[:, 0] = 1
    u = randn(H, DH, seed=6)
    u = (u / u.norm(dim=1, keepdim=True)).reshape(D).to(device)
    if regime == "sharp":
        q, k = q * 6, k * 6
    elif regime == "flat":
        q, k = q * 1e-3, k * 1e-3
    elif regime == "common":
        q, k = q + 8 * u, k + 8 * u
    elif regime == "planted":
        q, k = q * 0.3, k * 0.3
        j2 = Tk // 2
        valid[:, j2] = 1
        sign = torch.ones(Tq)
        sign[1::2] = -1
        if causal:
            sign[:j2] = 1
        q = q + 6 * sign.to(device)[None, :, None] * u
        k[:, 0] += 200 * u
        k[:, j2] -= 400 * u
    else:
        raise ValueError(regime)
    return dict(q=q.contiguous(), k=k.contiguous(), v=v, do=do, key_valid=valid.to(device), causal=causal)


def _heads(t):
    return t.reshape(t.shape[0], t.shape[1], H, DH).transpose(1, 2)


def _merge(t):
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], D)


def attention_math(case, dt, bf=False):
    """Forward and backward of gnn_transformer.py:149-156 written out (no autograd), in dtype ``dt``.  bf: the four products
    of each direction on bf16-ROUNDED operands, as the dtype-1 kernels run them (attention.hip: chain16<true>): S = q k^T,
    O = P v;  dP = dO v^T, dQ = dS k, dK = dS^T q, dV = P^T dO -- soft-max, delta = rowsum(dO * O) and dS in full precision."""
    rq = r16 if bf else (lambda t: t)
    q, k, v, do = (_heads(case[n].to(dt)) for n in ("q", "k", "v", "do"))
    Tq, Tk = q.shape[2], k.shape[2]
    dev = q.device
    mask = case["key_valid"][:, None, None, :].bool()
    if case["causal"]:
        mask = mask & (torch.arange(Tk, device=dev)[None, :] <= torch.arange(Tq, device=dev)[:, None])[None, None]
    s = (rq(q) @ rq(k).transpose(-1, -2)) / math.sqrt(DH)
    p = torch.softmax(s.masked_fill(~mask, -1e9), -1)
    o = rq(p) @ rq(v)
    delta = (do * o).sum(-1, keepdim=True)
    dp = rq(do) @ rq(v).transpose(-1, -2)
    ds = (p * (dp - delta) / math.sqrt(DH)).masked_fill(~mask, 0.0)
    dq = rq(ds) @ rq(k)
    dk = rq(ds).transpose(-1, -2) @ rq(q)
    dv = rq(p).transpose(-1, -2) @ rq(do)
    return dict(o=_merge(o), dq=_merge(dq), dk=_merge(dk), dv=_merge(dv), p=p, mask=mask)


def attention_floors(case):
    """Absolute scale of a row of O, dQ, dK, dV: 1e-6 of the bound of that row.  O is a convex combination of value rows;
    dV_j = sum_t P_tj dO_t; |dS_tj| <= 2 max_j |dO_t . v_j| / sqrt(32), dQ_t = sum_j dS_tj k_j, dK_j = sum_t dS_tj q_t -- with
    head rows of norm <= the full row's."""
    n = lambda t: float(t.double().norm(dim=-1).max())
    vq, dn = n(case["v"]), n(case["do"])
    g = 2 * dn * vq / math.sqrt(DH)
    return dict(o=1e-6 * vq, dv=1e-6 * dn, dq=1e-6 * g * n(case["k"]), dk=1e-6 * g * n(case["q"]))


# ---------------------------------------------------------------------------------------------------------------- 2. two-way gate
def gate_case(M, device="cpu"):
    """q | k at scale 20, v at scale 1: a - b = q (k - v) / sqrt(32) has std ~70 and spans more than +-200 -- the gates
    saturate and exp2(-|a - b| log2 e) underflows to 0; every 5th row has q = 0: a = b exactly, gates 0.5 / 0.5."""
    qk = randn(M, 512, seed=1, scale=20.0, device=device)
    qk[::5, :256] = 0
    vtab = randn(4, 256, seed=2, device=device)
    mark = (torch.arange(M) % 4).to(torch.int32).to(device)
    dout = randn(M, 256, seed=3, device=device)
    return dict(qk=qk, vtab=vtab, mark=mark, dout=dout)


def gate_ref(case, dt, mask=None):
    """combination_layer.py:7-17 and its autograd (the reference of test_combination_gate_fwd_bwd) in dtype dt"""
    qk = case["qk"].to(dt).requires_grad_(True)
    vtab = case["vtab"].to(dt).requires_grad_(True)
    q, k = qk[:, :256], qk[:, 256:]
    v = vtab[case["mark"].long()]
    s = math.sqrt(32)
    w = torch.softmax(torch.stack([q * k / s, q * v / s], -1), -1)
    out = (w * torch.stack([k, v], -1)).sum(-1)
    if mask is not None:
        out = out * mask.to(dt)
    dqk, dvtab = torch.autograd.grad(out, (qk, vtab), case["dout"].to(dt))
    return dict(out=out.detach(), dqk=dqk, dvtab=dvtab, a_minus_b=(q * (k - v) / s).detach())


# ---------------------------------------------------------------------------------------------------------------- 3. copy score
COPY_SCALES = {"cancel": 1e-3, "unit": 1.0, "saturated": 30.0}


def copy_case(kind, device="cpu", B=2, T=9, S=70):
    """src [B,S,256] + tgt [B,T,256] at scale 1e-3 (tanh_fast's cancelling region: 1 - 2/(1+e) with e ~ 1), 1, or 30 (every
    tanh saturated but a few: 1 - th^2 = 0 in the backward); "mixed": the rows of src cycle through the three scales."""
    src, tgt = randn(B, S, 256, seed=1, device=device), randn(B, T, 256, seed=2, device=device)
    if kind == "mixed":
        sc = torch.tensor([1e-3, 1.0, 30.0])
        src = src * sc[torch.arange(S) % 3].to(device)[None, :, None]
        tgt = tgt * sc[torch.arange(T) % 2].to(device)[None, :, None]
    else:
        src, tgt = src * COPY_SCALES[kind], tgt * COPY_SCALES[kind]
    w = randn(256, seed=3, scale=0.1, device=device)
    b = randn(1, seed=4, device=device)
    ds = randn(B, T, S, seed=5, device=device)
    g = torch.Generator().manual_seed(0)
    valid = (torch.rand(B, S, generator=g) > 0.4).to(torch.int32).to(device)
    return dict(src=src.contiguous(), tgt=tgt.contiguous(), w=w, b=b, ds=ds, valid=valid)


def copy_ref(case, dt, masked=False):
    """Model.py:15-20 and its autograd in dtype dt; masked: no gradient flows through a masked slot (masked_fill)"""
    src, tgt, w, b = (case[n].to(dt).requires_grad_(True) for n in ("src", "tgt", "w", "b"))
    score = (torch.tanh(src[:, None] + tgt[:, :, None]) * w).sum(-1) + b
    ds = case["ds"].to(dt)
    if masked:
        ds = ds * case["valid"][:, None, :].to(dt)
    dsrc, dtgt, dw, db = torch.autograd.grad(score, (src, tgt, w, b), ds)
    return dict(score=score.detach(), dsrc=dsrc, dtgt=dtgt, dw=dw, db=db)


def tanh_sweep(device="cpu", B=4, S=70):
    """x values for the element-wise check of tanh_fast: [-50, 50] linearly and geometrically (1e-7 .. 50, both signs),
    the points 9.9e-3 on both sides, and +-1e-6, +-1e-4, +-88 (e^{2x} = inf), +-100."""
    pos = torch.logspace(-7, math.log10(50.0), 66, dtype=torch.float64)
    extra = torch.tensor([1e-6, 1e-4, 88.0, 100.0, 9.9e-3, 5e-3, 0.3, 9.0], dtype=torch.float64)
    x = torch.cat([torch.linspace(-50, 50, 132, dtype=torch.float64), pos, -pos, extra, -extra]).float()
    assert x.numel() == B * S
    return x.view(B, S).to(device)


# ---------------------------------------------------------------------------------------------------------------- 4. head loss
CLAMP = 1e-10
BAND = (1e-11, 1e-9)                      # no labelled probability may lie here: the fp64 clamp decision survives fp32 rounding
HL_TARGETS = (1e-12, 1e-8, 1e-3, 0.3, 1e-13, 1e-7, 1e-5, 0.9)
HL_GATES = ((40.0, -40.0), (-40.0, 40.0), (12.0, -12.0), (-12.0, 12.0), (0.0, 0.0), (12.0, 0.0), (0.0, 12.0), (-40.0, -12.0))


def head_loss_case(V, device="cpu", B=4, T=30, S=37):
    """The label layout of test_head_loss_fwd_bwd with logits at scale 12 plus a per-row offset of +-1e4, copy scores at scale
    12, gate logits from {+-40, +-12, 0}.  Every labelled row's probability is PLANTED by solving for the label's own logit /
    score in fp64: the targets cycle through 1e-12, 1e-8, 1e-3, 0.3, 1e-13, 1e-7, 1e-5, 0.9 (capped by what the row's gate
    leaves to that part, and moved out of BAND), so generator and copy labels fall on both sides of the clamp at 1e-10; row
    (0, 0) is a generator label at p > 0.999999 under a gate of (40, -40)."""
    g = torch.Generator().manual_seed(0)
    R = B * T
    logits = torch.randn(R, V, generator=g) * 12
    logits = (logits + torch.where(torch.arange(R) % 2 == 0, 1e4, -1e4)[:, None]).float()
    score = (torch.randn(R, S, generator=g) * 12).float()
    gate = torch.tensor([HL_GATES[(r * 5 + r // 7) % len(HL_GATES)] for r in range(R)], dtype=torch.float32)
    gate[0] = torch.tensor([40.0, -40.0])
    valid = (torch.rand(B, S, generator=g) > 0.4).to(torch.int32)
    valid[:, :3] = 1
    lab = torch.zeros(B, T, dtype=torch.int64)
    lab[:, 0] = 2
    for b in range(B):
        n = 8 + 3 * b
        lab[b, 1:n] = torch.randint(4, V, (n - 1,), generator=g)
        vs = valid[b].nonzero().view(-1)
        for i, pos in enumerate((2, 3, 6)):
            lab[b, pos] = V + int(vs[(1 + 2 * i + b) % len(vs)])        # copy labels on valid slots
        lab[b, 4] = V + int((valid[b] == 0).nonzero().view(-1)[0])      # copy label on a masked slot: p = 0 exactly
        lab[b, n] = 1
    label = torch.cat([lab[:, 1:], torch.zeros_like(lab[:, :1])], 1).view(-1)
    gt = torch.softmax(gate.double(), -1)
    n_planted = 0
    for r in range(R):
        y = int(label[r])
        if y == 0:
            continue
        b = r // T
        if y < V:
            row, j, part, live = logits[r], y, float(gt[r, 0]), torch.ones(V, dtype=torch.bool)
        else:
            row, j, part, live = score[r], y - V, float(gt[r, 1]), valid[b].bool().clone()
            if not live[j]:
                continue
        target = (1 - 1e-7) if r == 0 else HL_TARGETS[n_planted % len(HL_TARGETS)]
        n_planted += 1
        qs = [target / part] + [0.5, 1e-3, 1e-6]
        qy = next((x for x in qs if x <= 0.9999999 and not (BAND[0] / 5 < x * part < BAND[1] * 5)), 1e-9)
        live[j] = False
        lse = torch.logsumexp(row.double()[live], 0)
        row[j] = float(lse + math.log(qy) - math.log1p(-qy))
    t = lambda a: a.to(device)
    return dict(logits=t(logits), score=t(score), gate=t(gate), valid=t(valid), lab=t(lab), label=t(label), V=V, B=B, T=T, S=S)


def head_loss_ref(case, dt):
    """Model.py:54-86 in dtype dt: loss sum, token count, gradients through clamp(min=1e-10, max=1), the probability of every
    labelled row, the clamp decision, the arg-max over [gen ; copy] and its relative top-two gap."""
    B, T, S, V = case["B"], case["T"], case["S"], case["V"]
    logits, score, gate = (case[n].to(dt).requires_grad_(True) for n in ("logits", "score", "gate"))
    label = case["label"]
    p_gen = torch.softmax(logits, -1).view(B, T, V)
    p_copy = torch.softmax(score.view(B, T, S).masked_fill(case["valid"][:, None, :] == 0, -1e9), -1)
    gt = torch.softmax(gate, -1).view(B, T, 2)
    p = torch.cat([gt[..., :1] * p_gen, gt[..., 1:] * p_copy], -1).view(B * T, V + S)
    logp = torch.log(p.clamp(min=CLAMP, max=1))
    nll = F.nll_loss(logp, label, reduction="none").masked_fill(label == 0, 0)
    dl, dsc, dg = torch.autograd.grad(nll.sum(), (logits, score, gate))
    labelled = label != 0
    p_lab = p.detach().gather(1, label[:, None]).view(-1)
    top = p.detach().topk(2, dim=1).values
    return dict(loss=float(nll.sum().detach()), ntok=int(labelled.sum()), dlogits=dl, dscore=dsc, dgate=dg, p_label=p_lab,
                labelled=labelled, clamped=labelled & ((p_lab < CLAMP) | (p_lab > 1)), ids=p.detach().argmax(-1),
                gap=(top[:, 0] - top[:, 1]) / top[:, 0])


# ---------------------------------------------------------------------------------------------------------------- 5. LayerNorm
LN_SPECIAL = {"constant": (0, 1), "std1e-3": (2, 3, 4, 5), "std1e3": (6, 7, 8, 9)}


def ln_case(M, c, device="cpu"):
    """x + res with a common component: res = randn + c, x = randn (unit spread, |mean| = c >> std).  The first rows are
    special: rows 0-1 constant (x = 0, res = c: variance exactly 0, rstd = 1 / sqrt(1e-5)), rows 2-5 of std 1e-3 around c,
    rows 6-9 of std 1e3 around c."""
    x, res = randn(M, 256, seed=1, device=device), randn(M, 256, seed=2, device=device) + c
    for r in LN_SPECIAL["constant"]:
        x[r], res[r] = 0.0, c
    for r in LN_SPECIAL["std1e-3"]:
        x[r], res[r] = x[r] * 1e-3, c
    for r in LN_SPECIAL["std1e3"]:
        x[r], res[r] = x[r] * 1e3, c
    gamma, beta = 1 + randn(256, seed=3, scale=0.1, device=device), randn(256, seed=4, scale=0.1, device=device)
    dy = randn(M, 256, seed=5, device=device)
    return dict(x=x, res=res, gamma=gamma, beta=beta, dy=dy, c=c)


def ln_groups(M):
    """Row groups that are held to the bound separately (a row of std 1e-3 at mean 1e3 has an fp32 error of per cent: it
    must not set the bound of the ordinary rows)."""
    first = max(max(v) for v in LN_SPECIAL.values()) + 1
    return dict(LN_SPECIAL, regular=tuple(range(first, M)))


def ln_ref(s, gamma, beta, dy, dt):
    """F.layer_norm of the rows s and its autograd in dtype dt: y, mean, rstd, ds, dgamma, dbeta"""
    s_ = s.to(dt).requires_grad_(True)
    g_, b_ = gamma.to(dt).requires_grad_(True), beta.to(dt).requires_grad_(True)
    y = F.layer_norm(s_, (256,), g_, b_, 1e-5)
    ds, dg, db = torch.autograd.grad(y, (s_, g_, b_), dy.to(dt))
    sd = s_.detach()
    return dict(y=y.detach(), mean=sd.mean(1), rstd=1.0 / torch.sqrt(sd.var(1, unbiased=False) + 1e-5), ds=ds, dgamma=dg, dbeta=db)


def zero_mean_rows(w):
    """w with the mean of every row removed: (c 1) w^T = 0, so a common component of the input does not reach the product"""
    return (w.double() - w.double().mean(1, keepdim=True)).float()
