"""The nonlinear kernels OFF unit scale, against fp64 (fixtures and references: tests/ranges_ref.py).

Every bound is  err(kernel, want) <= 3 * e32 + t0:  want = the formula in fp64, e32 = the error of the same formula in fp32 with
plain torch ops on the same operands, t0 = the tolerance the entry's existing unit-scale test uses, 3 = the margin the three-term
tests give a kernel over "the fp32 chain".  Outputs with rows are compared per row (row_err: one wrong row cannot hide in a
Frobenius ratio over the tensor); rows of different regimes are held to the bound of their own group.  Each test prints its
figures (pytest -s) before it asserts.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util  # noqa: F401
import ranges_ref as rr
from ranges_ref import rel_err, row_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32


def hold(name, got, want, plain32, floor, t0, rows=None):
    """row_err(got, want) <= 3 * row_err(plain32, want) + t0 on the rows listed (all), and everything finite"""
    if rows is not None:
        idx = torch.as_tensor(list(rows), device=want.device, dtype=torch.long)
        pick = lambda t: t.reshape(-1, t.shape[-1])[idx] if t.dim() > 1 else t[idx]
        got, want, plain32 = pick(got), pick(want), pick(plain32)
        if torch.is_tensor(floor) and floor.numel() > 1:
            floor = floor.reshape(-1)[idx]
    assert bool(torch.isfinite(got).all()), name
    e, e32 = row_err(got, want, floor), row_err(plain32, want, floor)
    print(f"  {name}: err {e:.3e}  e32 {e32:.3e}  bound {3 * e32 + t0:.3e}")
    assert e <= 3 * e32 + t0, (name, e, e32)


def hold_w(name, got, want, plain32, t0):
    """the same rule with rel_err: weight-shaped reductions only"""
    e, e32 = rel_err(got, want), rel_err(plain32, want)
    print(f"  {name}: err {e:.3e}  e32 {e32:.3e}  bound {3 * e32 + t0:.3e}")
    assert math.isfinite(e) and e <= 3 * e32 + t0, (name, e, e32)


# ---------------------------------------------------------------------------------------------------------------- 1. attention
def _ragged(case, Tq, Tk):
    """Compact query rows (commit b has a prefix of its Tq positions); causal: keys / values are the same compact rows.  The
    reference is the dense computation with dO = 0 on the rows that do not exist (and their keys masked)."""
    B = case["q"].shape[0]
    lens = [Tq, 1, max(Tq - 2, 1)][:B]
    dev = case["q"].device
    off = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev)
    rows = torch.cat([torch.arange(n) + b * Tq for b, n in enumerate(lens)]).to(dev)
    exists = torch.zeros(B * Tq, dtype=torch.bool, device=dev)
    exists[rows] = True
    c2 = dict(case, do=case["do"] * exists.view(B, Tq, 1))
    if case["causal"]:
        c2["key_valid"] = case["key_valid"] * exists.view(B, Tq).to(torch.int32)
    return c2, off, rows


@pytest.mark.parametrize("Tq,Tk,causal", rr.ATT_SHAPES)
@pytest.mark.parametrize("regime", rr.ATT_REGIMES)
def test_attention_off_unit_scale(regime, Tq, Tk, causal):
    """attention_fwd / attention_bwd, attention_ragged_fwd / _bwd (dtype 0) and decode_attention against the fp64 soft-max.
      sharp    (scores of std 36) and planted (one key > 120 above the rest): exp2f(st - mx) of attention.hip:356 / :443 and the
               forward's twin underflow to exactly 0 for every key but one; 1 / sum is 1; dS = P (dP - delta) cancels to ~0
      flat     (scale 1e-3): every exponential is ~1, the row sums are the key counts
      common   (q, k += 8 u): the offset of a row's scores must cancel in st - mx, not in the exponential's argument range
    One key tile (Tk <= 32: FIRA_ATT_BWD(1)) and three (12 waves); the causal form on the self-attention shapes; key masks with
    holes.  dK / dV of masked keys are exactly 0.  t0: 2e-6 forward, 5e-6 backward (test_attention_fwd_bwd)."""
    from fira_icse_amd import ops
    case = rr.attention_case(regime, Tq, Tk, causal, device=DEV)
    want, p32 = rr.attention_math(case, F64), rr.attention_math(case, F32)
    fl = rr.attention_floors(case)
    q, k, v, do, kv = case["q"], case["k"], case["v"], case["do"], case["key_valid"]
    B = q.shape[0]
    o = ops.attention_fwd(q, k, v, kv, causal)
    hold("O", o, want["o"], p32["o"], fl["o"], 2e-6)
    dq, dk, dv = ops.attention_bwd(q, k, v, kv, o, do, causal)
    for n, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        hold(n, got, want[n], p32[n], fl[n], 5e-6)
    masked = kv == 0
    if bool(masked.any()):
        assert float(dk[masked].abs().max()) == 0.0 and float(dv[masked].abs().max()) == 0.0
    # the engine's form: ragged query rows
    c2, off, rows = _ragged(case, Tq, Tk)
    w2, q2 = rr.attention_math(c2, F64), rr.attention_math(c2, F32)
    flat = lambda t: t.reshape(-1, 256)
    qc, doc = flat(q)[rows].contiguous(), flat(c2["do"])[rows].contiguous()
    kc, vc = (flat(k)[rows].contiguous(), flat(v)[rows].contiguous()) if causal else (flat(k), flat(v))
    pk = (lambda t: flat(t)[rows]) if causal else flat
    o2 = ops.attention_ragged_fwd(qc, kc, vc, c2["key_valid"], off, Tq, Tk, causal=causal, self_kv=causal)
    hold("ragged O", o2, flat(w2["o"])[rows], flat(q2["o"])[rows], fl["o"], 2e-6)
    dq2, dk2, dv2 = ops.attention_ragged_bwd(qc, kc, vc, c2["key_valid"], o2, doc, off, Tq, Tk, causal=causal, self_kv=causal,
                                             fill=float("nan"))
    hold("ragged dq", dq2, flat(w2["dq"])[rows], flat(q2["dq"])[rows], fl["dq"], 5e-6)
    hold("ragged dk", dk2, pk(w2["dk"]), pk(q2["dk"]), fl["dk"], 5e-6)
    hold("ragged dv", dv2, pk(w2["dv"]), pk(q2["dv"]), fl["dv"], 5e-6)
    m2 = pk(c2["key_valid"].reshape(-1, 1).expand(-1, 256)) == 0
    if bool(m2.any()):
        assert float(dk2[m2].abs().max()) == 0.0 and float(dv2[m2].abs().max()) == 0.0
    if not causal:                                   # one query per commit: the decode step's kernel
        od = ops.decode_attention(q[:, 0].contiguous(), k, v, kv, tk=Tk)
        hold("decode O", od, want["o"][:, 0], p32["o"][:, 0], fl["o"], 2e-6)


@pytest.mark.parametrize("Tq,Tk,causal", rr.ATT_SHAPES)
@pytest.mark.parametrize("regime", rr.ATT_REGIMES)
def test_attention_bf16_operands_off_unit_scale(regime, Tq, Tk, causal):
    """attention_ragged_fwd / _bwd with dtype 1 in the same four regimes, against the fp64 result of the bf16-ROUNDED operands
    of each product (rr.attention_math(bf=True) states the rounding points of attention.hip's chain16<true> calls: q, k for S;
    P, v for O; dO, v for dP; dS, k for dQ; dS, q for dK; P, dO for dV; soft-max, delta and dS in fp32) -- per row, forward and
    all three gradients.  e32 is the same emulation in fp32: it differs from fp64 where an fp32 P or dS lands on the other side of
    a bf16 rounding boundary, which is also what the kernel may do.  t0: 5e-5 forward (the existing comparison), 1e-4 backward."""
    from fira_icse_amd import ops
    case = rr.attention_case(regime, Tq, Tk, causal, device=DEV)
    c2, off, rows = _ragged(case, Tq, Tk)
    want, p32 = rr.attention_math(c2, F64, bf=True), rr.attention_math(c2, F32, bf=True)
    fl = rr.attention_floors(case)
    flat = lambda t: t.reshape(-1, 256)
    qc, doc = flat(c2["q"])[rows].contiguous(), flat(c2["do"])[rows].contiguous()
    kc, vc = (flat(c2["k"])[rows].contiguous(), flat(c2["v"])[rows].contiguous()) if causal else (flat(c2["k"]), flat(c2["v"]))
    pk = (lambda t: flat(t)[rows]) if causal else flat
    o = ops.attention_ragged_fwd(qc, kc, vc, c2["key_valid"], off, Tq, Tk, causal=causal, self_kv=causal, dtype=1)
    hold("bf16 O", o, flat(want["o"])[rows], flat(p32["o"])[rows], fl["o"], 5e-5)
    dq, dk, dv = ops.attention_ragged_bwd(qc, kc, vc, c2["key_valid"], o, doc, off, Tq, Tk, causal=causal, self_kv=causal,
                                          dtype=1, fill=float("nan"))
    hold("bf16 dq", dq, flat(want["dq"])[rows], flat(p32["dq"])[rows], fl["dq"], 1e-4)
    hold("bf16 dk", dk, pk(want["dk"]), pk(p32["dk"]), fl["dk"], 1e-4)
    hold("bf16 dv", dv, pk(want["dv"]), pk(p32["dv"]), fl["dv"], 1e-4)
    m2 = pk(c2["key_valid"].reshape(-1, 1).expand(-1, 256)) == 0
    if bool(m2.any()):
        assert float(dk[m2].abs().max()) == 0.0 and float(dv[m2].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 2. two-way gate
@pytest.mark.parametrize("M", [37, 530])
def test_gate_saturated_and_balanced(M):
    """combination_fwd / combination_bwd (rowops.hip:219 / :288 -> gate_elem, common.h:140) with a - b spanning +-200:
    v_exp_f32 of -|a - b| log2 e underflows to 0, big = rcp(1 + 0) = 1, small = 0 -- and q = 0 rows where a = b exactly and both
    gates are rcp(2).  fp64 autograd of test_combination_gate_fwd_bwd.  Row floors: 1e-6 of the row of (k, v) the output mixes,
    1e-6 of the incoming gradient row.  t0: 1e-6 forward, 2e-6 backward, 1e-5 dvtab (the existing test)."""
    from fira_icse_amd import ops
    case = rr.gate_case(M, device=DEV)
    want, p32 = rr.gate_ref(case, F64), rr.gate_ref(case, F32)
    out = ops.combination_fwd(case["qk"], case["vtab"], case["mark"])
    hold("out", out, want["out"], p32["out"], 1e-6 * case["qk"][:, 256:].double().norm(dim=1), 1e-6)
    bal = torch.arange(0, M, 5, device=DEV)
    half = 0.5 * (case["qk"][bal, 256:].double() + case["vtab"].double()[case["mark"][bal].long()])
    assert row_err(out[bal], half, 1e-6) <= 1e-6                    # gates 0.5 / 0.5
    dqk, dvtab = ops.combination_bwd(case["qk"], case["vtab"], case["mark"], case["dout"])
    hold("dqk", dqk, want["dqk"], p32["dqk"], 1e-6 * case["dout"].double().norm(dim=1), 2e-6)
    hold_w("dvtab", dvtab, want["dvtab"], p32["dvtab"], 1e-5)


def _block_inputs(n, wscale, c=0.0, zero_rows=False):
    Xc = rr.randn(n, 256, seed=1, device=DEV) + c
    if zero_rows:
        Xc[::5] = 0
    Wqk = rr.randn(512, 256, seed=2, scale=wscale)
    if c:
        Wqk = rr.zero_mean_rows(Wqk)
    Wqk = Wqk.to(DEV)
    bqk = rr.randn(512, seed=3, scale=0.1, device=DEV) * (0.0 if zero_rows else 1.0)
    Wo, bo = rr.randn(256, 256, seed=4, scale=0.08, device=DEV), rr.randn(256, seed=5, scale=0.1, device=DEV)
    vtab = rr.randn(4, 256, seed=6, device=DEV)
    mark = (torch.arange(n) % 4).to(torch.int32).to(DEV)
    gamma, beta = 1 + rr.randn(256, seed=7, scale=0.1, device=DEV), rr.randn(256, seed=8, scale=0.1, device=DEV)
    return Xc, Wqk, bqk, Wo, bo, vtab, mark, gamma, beta


def _block_ref(inp, dt, mg, mo, bf=False):
    """the Combination block of gnn_transformer.py:176-205 in dtype dt (the fp64 statement of test_combination_block_fused_fwd)"""
    Xc, Wqk, bqk, Wo, bo, vtab, mark, gamma, beta = (t.to(dt) if t.is_floating_point() else t for t in inp)
    rq = rr.r16 if bf else (lambda t: t)
    q = rq(Xc) @ rq(Wqk[:256]).t() + bqk[:256]
    k = rq(Xc) @ rq(Wqk[256:]).t() + bqk[256:]
    v = vtab[mark.long()]
    g = torch.softmax(torch.stack([q * k / math.sqrt(32), q * v / math.sqrt(32)], -1), -1)
    c = (g[..., 0] * k + g[..., 1] * v) * mg.to(dt)
    s = (rq(c) @ rq(Wo).t() + bo) * mo.to(dt) + Xc
    y = F.layer_norm(s, (256,), gamma, beta, 1e-5)
    return dict(q=q, k=k, c=c, s=s, y=y, mean=s.mean(1), rstd=1.0 / torch.sqrt(s.var(1, unbiased=False) + 1e-5))


def _block_bwd_ref(inp, dt, summ, qk, dy, mg, mo, bf=False):
    """backward of the block in dtype dt from the SAVED q | k and pre-norm rows (what the kernel reads), as the fp64 statement of
    test_combination_block_fused_bwd: LayerNorm backward, dYc = ds * mask, d c = dYc Wo, the gate's backward, dX = dq Wq + dk Wk;
    bf: the operands of the three products rounded to bf16"""
    Xc, Wqk, bqk, Wo, bo, vtab, mark, gamma, beta = (t.to(dt) if t.is_floating_point() else t for t in inp)
    rq = rr.r16 if bf else (lambda t: t)
    leaf = lambda t: t.detach().clone().to(dt).requires_grad_(True)
    s_, g_, b_ = leaf(summ), leaf(gamma), leaf(beta)
    ds, dgam, dbet = torch.autograd.grad(F.layer_norm(s_, (256,), g_, b_, 1e-5), (s_, g_, b_), dy.to(dt))
    dYc = ds * mo.to(dt)
    dc = rq(dYc) @ rq(Wo)
    q_, k_, vt_ = leaf(qk[:, :256]), leaf(qk[:, 256:]), leaf(vtab)
    v_ = vt_[mark.long()]
    gg = torch.softmax(torch.stack([q_ * k_ / math.sqrt(32), q_ * v_ / math.sqrt(32)], -1), -1)
    cc = (gg[..., 0] * k_ + gg[..., 1] * v_) * mg.to(dt)
    dq, dk, dvt = torch.autograd.grad(cc, (q_, k_, vt_), dc)
    dX = rq(dq) @ rq(Wqk[:256]) + rq(dk) @ rq(Wqk[256:])
    return dict(dYc=dYc, dqk=torch.cat([dq, dk], 1), dG=ds + dX, dgamma=dgam, dbeta=dbet, dvtab=dvt)


def _hold_block_bwd(tag, inp, qk, summ, stats, mg, mo, p, seed, sg, so, dtype, bf, t1, tv):
    """combination_block_bwd on a forward launch's outputs: dYc, dq | dk and the dG rows per row (floor: 1e-6 of the incoming
    gradient row times the row's rstd, the scale of ds), dgamma / dbeta / dvtab by rel_err; rows not listed stay untouched"""
    from fira_icse_amd import ops
    Xc, Wqk, bqk, Wo, bo, vtab, mark, gamma, beta = inp
    n = summ.shape[0]
    rows = torch.randperm(2 * n, generator=torch.Generator().manual_seed(3))[:n].to(torch.int32).to(DEV)
    dG0 = rr.randn(2 * n, 256, seed=9, device=DEV)
    dG = dG0.clone()
    dYc, dqk, dgamma, dbeta, dvtab = ops.combination_block_bwd(dG, rows, summ, stats, gamma, Wo, Wqk, qk, vtab, mark, dropout=p,
                                                               seed=seed, site_gate=sg, site_out=so, dtype=dtype)
    dy = dG0[rows.long()]
    want, p32 = (_block_bwd_ref(inp, dt, summ, qk, dy, mg, mo, bf) for dt in (F64, F32))
    fl = 1e-6 * dy.double().norm(dim=1) * stats[:, 1].double()
    hold(f"{tag} dYc", dYc, want["dYc"], p32["dYc"], fl, 5e-6)
    hold(f"{tag} dqk", dqk, want["dqk"], p32["dqk"], fl, t1)
    hold(f"{tag} dG", dG[rows.long()], want["dG"], p32["dG"], fl, t1)
    untouched = torch.ones(2 * n, dtype=torch.bool, device=DEV)
    untouched[rows.long()] = False
    assert torch.equal(dG[untouched], dG0[untouched])
    hold_w(f"{tag} dgamma", dgamma, want["dgamma"], p32["dgamma"], 1e-5)
    hold_w(f"{tag} dbeta", dbeta, want["dbeta"], p32["dbeta"], 1e-5)
    hold_w(f"{tag} dvtab", dvtab, want["dvtab"], p32["dvtab"], tv)


def _graph_batch(B, N, density, seed):
    """B symmetric random adjacency blocks with a full diagonal and one hub node (row / column 0 connected to every node: more
    than 16 entries, the tail path of the fused gather) -> block-diagonal CSR + the dense blocks"""
    rng = np.random.default_rng(seed)
    m = rng.random((B, N, N)) < density / 2
    m[:, 0, :] = True
    m = m | m.transpose(0, 2, 1) | np.eye(N, dtype=bool)[None]
    dense = np.where(m, rng.uniform(0.05, 1.0, (B, N, N)), 0.0).astype(np.float32)
    b, r, c = np.nonzero(dense)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(b * N + r, minlength=B * N))])
    t = lambda a, dt: torch.tensor(np.asarray(a, dtype=dt), device=DEV)
    return t(rowptr, np.int32), t(b * N + c, np.int32), t(dense[b, r, c], np.float32), torch.tensor(dense, device=DEV)


@pytest.mark.parametrize("n", [37, 530])
def test_combination_block_gate_saturated(n):
    """combination_block_fwd / combination_block_bwd (dtype 0; comb_fused.hip:261 and :885 -> gate_elem, common.h:140) with
    q | k projections of std 20: a - b spans +-200 inside the fused launches; rows with Xc = 0 and no bias give q = k = 0, gates
    0.5 / 0.5.  Backward on the forward's outputs: dq | dk through the saturated / balanced gates, the dG rows, dvtab.  t0: 2e-6
    for q | k, 5e-6 for the gate's output, 5e-6 / 1e-5 for sum / y (test_combination_block_fused_fwd); 5e-6 for dYc, dq | dk and
    dG, 1e-5 for dgamma, dbeta, dvtab (test_combination_block_fused_bwd)."""
    from fira_icse_amd import ops
    inp = _block_inputs(n, 20.0 / 16, zero_rows=True)
    p, seed, sg, so = 0.1, 4321, 17, 18
    qk, c, summ, y, stats = ops.combination_block_fwd(*inp, dropout=p, seed=seed, site_gate=sg, site_out=so, dtype=0)
    mg = ops.dropout_mask(seed, sg, n * 256, p).view(n, 256)
    mo = ops.dropout_mask(seed, so, n * 256, p).view(n, 256)
    want, p32 = _block_ref(inp, F64, mg, mo), _block_ref(inp, F32, mg, mo)
    d = want["q"] * (want["k"] - inp[5].double()[inp[6].long()]) / math.sqrt(32)
    assert float(d.max()) > 200 and float(d.min()) < -200
    fq = 1e-6 * 20 * 16
    hold("q", qk[:, :256], want["q"], p32["q"], fq, 2e-6)
    hold("k", qk[:, 256:], want["k"], p32["k"], fq, 2e-6)
    hold("c", c, want["c"], p32["c"], fq, 5e-6)
    hold("sum", summ, want["s"], p32["s"], fq, 5e-6)
    hold("y", y, want["y"], p32["y"], 1e-6 * 16, 1e-5)
    _hold_block_bwd("bwd", inp, qk, summ, stats, mg, mo, p, seed, sg, so, 0, False, 5e-6, 1e-5)


# ---------------------------------------------------------------------------------------------------------------- 3. copy score
def _copy_floors(case):
    wn = float(case["w"].double().norm())
    ds = case["ds"].double()
    return 1e-6 * wn * ds.norm(dim=1).reshape(-1), 1e-6 * wn * ds.norm(dim=2).reshape(-1)     # rows of dsrc [B,S], dtgt [B,T]


def _hold_score(name, sc, want, p32, w):
    e = float((sc.double() - want).abs().max())
    e32 = float((p32.double() - want).abs().max())
    bound = 2e-7 * float(w.double().abs().sum()) + 3 * e32
    print(f"  {name}: |err| {e:.3e}  e32 {e32:.3e}  bound {bound:.3e}")
    assert bool(torch.isfinite(sc).all()) and e <= bound, (name, e, e32)


@pytest.mark.parametrize("kind", ["cancel", "unit", "saturated", "mixed"])
def test_copy_score_off_unit_scale(kind):
    """copy_score_fwd / copy_score_bwd (copyhead.hip:68-71, :175-179 -> tanh_fast, copyhead.hip:22) with src + tgt at scale
    1e-3 (e^{2x} ~ 1: 1 - 2 / (1 + e) cancels), 1, 30 (e^{2x} = inf or 0: th = +-1, 1 - th^2 = 0 in the backward) and rows of
    all three.  Forward, per element: |score - score64| <= 2e-7 sum|w| + 3 e32 (tanh_fast's written bound times the weights).
    Backward: rows of dsrc / dtgt with floor 1e-6 |w| |ds_r|, t0 5e-6; dw / db by rel_err, t0 1e-5 (test_copy_score_fwd_bwd).
    MEASURED EXCEPTION, dw at scale 1e-3: err 4.15e-5 with e32 1.3e-7.  dw = sum ds * th, and tanh_fast is accurate absolutely
    (measured 1.6e-7, written 2e-7), not relatively: at |x| ~ 1e-3 every th carries ~1e-4 of itself, and so does their weighted
    sum.  That is inside the function's written claim (|dw_d - dw64_d| <= 2e-7 sum|ds|, asserted below) and is what the issue's
    absolute rule for the forward pass already grants; a relatively accurate tanh would cost the hot loop a compare and a
    cubic.  The bound of that case is the measured 4.2e-5 + 3 e32 instead of 1e-5 + 3 e32."""
    from fira_icse_amd import ops
    case = rr.copy_case(kind, device=DEV)
    want, p32 = rr.copy_ref(case, F64), rr.copy_ref(case, F32)
    sc = ops.copy_score_fwd(case["src"], case["tgt"], case["w"], case["b"])
    _hold_score("score", sc, want["score"], p32["score"], case["w"])
    dsrc, dtgt, dw, db = ops.copy_score_bwd(case["src"], case["tgt"], case["w"], case["ds"])
    f_src, f_tgt = _copy_floors(case)
    hold("dsrc", dsrc, want["dsrc"], p32["dsrc"], f_src, 5e-6)
    hold("dtgt", dtgt, want["dtgt"], p32["dtgt"], f_tgt, 5e-6)
    hold_w("dw", dw, want["dw"], p32["dw"], 4.2e-5 if kind == "cancel" else 1e-5)
    assert float((dw.double() - want["dw"]).abs().max()) <= 2e-7 * float(case["ds"].double().abs().sum()) + 3 * float(
        (p32["dw"].double() - want["dw"]).abs().max())
    hold_w("db", db, want["db"], p32["db"], 1e-5)


def test_copy_score_engine_form_with_key_mask():
    """copy_score_fwd_ex / copy_score_bwd_ex with a key mask on the mixed-scale rows: masked slots score exactly 0 and pass
    no gradient (copyhead.hip:60, :114, :138), the others are held as in test_copy_score_off_unit_scale."""
    from fira_icse_amd import ops
    case = rr.copy_case("mixed", device=DEV)
    B, S, T = case["src"].shape[0], case["src"].shape[1], case["tgt"].shape[1]
    want, p32 = rr.copy_ref(case, F64, masked=True), rr.copy_ref(case, F32, masked=True)
    sc = torch.full((B * T, S), float("nan"), device=DEV)
    ops.copy_score_fwd_ex(case["src"], case["tgt"].view(B * T, 256), case["w"], case["b"], sc, T, mem_valid=case["valid"])
    live = case["valid"][:, None, :].expand(B, T, S).bool()
    sc = sc.view(B, T, S)
    assert float(sc[~live].abs().max()) == 0.0
    _hold_score("score", torch.where(live, sc, want["score"].float()), want["score"], p32["score"], case["w"])
    dsrc, dtgt = torch.full_like(case["src"], float("nan")), torch.zeros_like(case["tgt"])
    dw, db = torch.zeros(256, device=DEV), torch.zeros(1, device=DEV)
    ops.copy_score_bwd_ex(case["src"], case["tgt"].view(B * T, 256), case["w"], case["ds"], dsrc, dtgt.view(B * T, 256), dw, db, T,
                          mem_valid=case["valid"])
    f_src, f_tgt = _copy_floors(case)
    hold("dsrc", dsrc, want["dsrc"], p32["dsrc"], f_src, 5e-6)
    hold("dtgt", dtgt, want["dtgt"], p32["dtgt"], f_tgt, 5e-6)
    assert float(dsrc[case["valid"] == 0].abs().max()) == 0.0
    hold_w("dw", dw, want["dw"], p32["dw"], 1e-5)


def test_tanh_fast_holds_its_written_bound():
    """The claim in copyhead.hip:20 -- |abs error| < 2e-7 over the whole range, correct saturation -- element by element: one
    launch with w = e_0, tgt = 0, bias 0, so score[b, 0, j] = tanh_fast(src[b, j, 0]) exactly (the other 255 terms are
    0 * tanh_fast(0) = 0 and the wave sum adds zeros).  x sweeps [-50, 50] linearly and geometrically from 1e-7, plus +-1e-6,
    +-1e-4 (the cancelling region), +-88 (e^{2x} overflows to inf: 2 / inf = 0) and +-100."""
    from fira_icse_amd import ops
    x = rr.tanh_sweep(device=DEV)
    B, S = x.shape
    src = torch.zeros(B, S, 256, device=DEV)
    src[:, :, 0] = x
    w = torch.zeros(256, device=DEV)
    w[0] = 1.0
    sc = ops.copy_score_fwd(src, torch.zeros(B, 1, 256, device=DEV), w, torch.zeros(1, device=DEV))[:, 0]
    err = (sc.double() - torch.tanh(x.double())).abs()
    i = int(err.argmax())
    print(f"  tanh_fast: max |err| {float(err.max()):.3e} at x = {float(x.reshape(-1)[i]):.4g}")
    assert bool(torch.isfinite(sc).all()) and float(err.max()) <= 2e-7
    big = x.abs() >= 20
    assert bool((sc[big] == torch.sign(x[big])).all())               # saturates to exactly +-1


# ---------------------------------------------------------------------------------------------------------------- 4. head loss
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("V", [1000, 1001])
def test_head_loss_around_the_clamp(V, compact):
    """head_loss on rr.head_loss_case: logits at scale 12 with row offsets of +-1e4 (shift invariance; fmaf(x, L2E, c) of
    copyhead.hip:465 / :472 at |x| = 1e4), copy scores at scale 12, gates from {+-40, +-12, 0}, and labels planted at p ~ 1e-12 /
    1e-8 in the generator and in the copy part, p = 0 (masked slot) and p > 0.999999: the clamp test `p >= 1e-10f && p <= 1`
    (copyhead.hip:355 in head_loss_kernel, :485 in head_loss_train_kernel) decides on an fp32 p from exp2 / expf, the reference
    on the fp64 p; the fixture keeps every labelled p out of [1e-11, 1e-9] (tests/test_ranges.py).  V = 1000: the register
    kernels (training form, and the arg-max form in the dense case), V = 1001: the streaming kernel.  Loss to 2e-6 relative,
    ntok, gradient rows (floor 1e-12, t0 5e-6, by row group: unlabelled, clamped, the p > 0.999999 row, the others), clamped
    rows exactly 0, arg-max ids where the fp64 top-two gap exceeds 1e-3 relative."""
    from fira_icse_amd import ops
    case = rr.head_loss_case(V, device=DEV)
    want, p32 = rr.head_loss_ref(case, F64), rr.head_loss_ref(case, F32)
    B, T, S = case["B"], case["T"], case["S"]
    label, lab32 = case["label"], case["lab"].to(torch.int32)
    rows_l = torch.arange(B * T, device=DEV)
    compact_row = None
    lg0 = case["logits"]
    if compact:
        rows_l = ((label > 0) & (label < V)).nonzero().view(-1)
        lg0 = lg0[rows_l].contiguous()
        compact_row = torch.full((B * T,), -1, dtype=torch.int32, device=DEV)
        compact_row[rows_l] = torch.arange(rows_l.numel(), dtype=torch.int32, device=DEV)
    runs = [dict(argmax=False)] + ([] if compact else [dict(argmax=True)])
    for kw in runs:
        lg, sc, gl = lg0.clone(), case["score"].clone(), case["gate"].clone()
        loss, ntok, ids = ops.head_loss(lg, sc, case["valid"], gl, lab32, V, compact_row=compact_row, **kw)
        print(f"  loss {float(loss):.6f} want {want['loss']:.6f}  ntok {int(ntok)}")
        assert int(ntok) == want["ntok"]
        assert abs(float(loss) - want["loss"]) / want["loss"] < 2e-6
        clamped, labelled = want["clamped"], want["labelled"]
        top = want["p_label"] > 0.999999
        groups = dict(unlabelled=~labelled, clamped=clamped, top=top, passing=labelled & ~clamped & ~top)
        assert int(clamped.sum()) >= 4 and int(top.sum()) == 1
        for name, sel in groups.items():
            r = sel.nonzero().view(-1)
            in_l = sel[rows_l].nonzero().view(-1)                     # the same rows among those that have logits
            hold(f"dlogits[{name}]", lg[in_l], want["dlogits"][rows_l][in_l], p32["dlogits"][rows_l][in_l], 1e-12, 5e-6)
            hold(f"dscore[{name}]", sc[r], want["dscore"][r], p32["dscore"][r], 1e-12, 5e-6)
            hold(f"dgate[{name}]", gl[r], want["dgate"][r], p32["dgate"][r], 1e-12, 5e-6)
        zero = clamped | ~labelled
        assert float(sc[zero].abs().max()) == 0.0 and float(gl[zero].abs().max()) == 0.0
        assert float(lg[zero[rows_l]].abs().max()) == 0.0
        if kw["argmax"]:
            sure = want["gap"] > 1e-3
            assert int(sure.sum()) > B * T // 2
            assert torch.equal(ids.view(-1).long()[sure], want["ids"][sure])


# ---------------------------------------------------------------------------------------------------------------- 5. LayerNorm
def hold_mean(name, got, want, p32, rows=None):
    """the row mean, with its error in units of the row's own sqrt(var + eps) -- what an error of the mean does to y -- and not of
    |mean| ~ c, against which a unit-scale tolerance would be vacuous.  t0 1e-6, the LayerNorm forward tolerance."""
    z = want["rstd"].double()
    one = torch.ones_like(z)
    hold(name, one + (got.double() - want["mean"]) * z, one, one + (p32["mean"].double() - want["mean"]) * z, 1.0, 1e-6, rows=rows)


def _hold_ln(tag, groups, got, want, p32, names, t0s):
    for gname, rows in groups.items():
        for n in names:
            if n == "mean":
                hold_mean(f"{tag} mean[{gname}]", got[n], want, p32, rows=rows)
                continue
            floor = 1e-6 * (16 if n in ("y", "ds") else 1)
            hold(f"{tag} {n}[{gname}]", got[n], want[n], p32[n], floor, t0s[n], rows=rows)


LN_T0 = dict(y=1e-6, rstd=1e-5, ds=5e-6)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("c", [1e2, 1e3])
@pytest.mark.parametrize("M", [33, 530])
def test_add_layernorm_with_a_common_component(M, c, p):
    """add_layernorm_fwd / add_layernorm_bwd (rowops.hip:355-358: mean, then the variance of the centred values; :429-445: the
    backward's xh = (s - mean) rstd and ds) on rows x + res with mean c = 1e2 / 1e3 and unit spread, plus rows of
    variance exactly 0 (rstd = 1 / sqrt(1e-5)), of std 1e-3 and of std 1e3 -- against fp64 F.layer_norm and its autograd with the
    entry's own dropout mask.  e32 is torch's own fp32 layer_norm on the same rows.  PURPOSE: every LayerNorm of the library is
    two-pass; a one-pass variance E[x^2] - mean^2 loses x^2 eps = 1e6 * 6e-8 = 0.06 of a unit variance at c = 1e3 and fails
    rstd, y and ds here by orders of magnitude, where the two-pass form passes.  No unit-scale test notices the difference.
    t0: 1e-6 for y, 5e-6 for ds, 1e-5 for dgamma / dbeta (test_add_layernorm_fwd_bwd_and_dropout_mask), 1e-5 for rstd (the
    stats checks of the fused tests); the mean is held in units of the row's sqrt(var + eps) at 1e-6 (hold_mean)."""
    from fira_icse_amd import ops
    case = rr.ln_case(M, c, device=DEV)
    seed, site = 77, 5
    mask = ops.dropout_mask(seed, site, M * 256, p).view(M, 256) if p > 0 else torch.ones(M, 256, device=DEV)
    y, s, stats = ops.add_layernorm_fwd(case["x"].clone(), case["res"], case["gamma"], case["beta"], p, seed=seed, site=site)
    s64 = case["x"].double() * mask.double() + case["res"].double()
    s32 = case["x"] * mask + case["res"]
    groups = rr.ln_groups(M)
    hold("sum", s, s64, s32, 1e-6 * 16, 1e-7)
    want, p32 = (rr.ln_ref(si, case["gamma"], case["beta"], case["dy"], dt) for si, dt in ((s64, F64), (s32, F32)))
    got = dict(y=y, mean=stats[:, 0], rstd=stats[:, 1])
    _hold_ln("fwd", groups, got, want, p32, ("y", "mean", "rstd"), LN_T0)
    # backward from the SAVED pre-norm rows and statistics (what the kernel reads)
    wb, pb = (rr.ln_ref(s, case["gamma"], case["beta"], case["dy"], dt) for dt in (F64, F32))
    ds, dxd, dg, db = ops.add_layernorm_bwd(case["dy"], s, stats, case["gamma"], p, seed=seed, site=site, want_dx_drop=True)
    _hold_ln("bwd", groups, dict(ds=ds), wb, pb, ("ds",), LN_T0)
    _hold_ln("bwd", groups, dict(ds=dxd), dict(ds=wb["ds"] * mask.double()), dict(ds=pb["ds"] * mask), ("ds",), LN_T0)
    hold_w("dgamma", dg, wb["dgamma"], pb["dgamma"], 1e-5)
    hold_w("dbeta", db, wb["dbeta"], pb["dbeta"], 1e-5)


@pytest.mark.parametrize("c", [1e2, 1e3])
@pytest.mark.parametrize("M", [33, 530])
def test_layernorm_prologues_with_a_common_component(M, c):
    """ln_linear (LayerNorm in the prologue of a product, gemm_small.hip:310-318: variance of the centred values, rstd, the
    normalised operand) and ln_bwd_linear (its backward in the prologue of the data-gradient product, gemm_small.hip:351-352 xh,
    :407-410 ds) on the rows of rr.ln_case: y, mean, rstd, the product of the normalised rows;
    ds, dgamma, dbeta and dX.  Purpose and tolerances as in test_add_layernorm_with_a_common_component; 5e-6 / 3e-6 for the
    products (test_residual_block_split_at_its_layernorm, test_layernorm_backward_in_the_dgrad_prologue)."""
    from fira_icse_amd import ops
    case = rr.ln_case(M, c, device=DEV)
    s = case["x"] + case["res"]
    groups = rr.ln_groups(M)
    w2, b2 = rr.randn(256, 256, seed=7, scale=1 / 16, device=DEV), rr.randn(256, seed=8, device=DEV)
    out, y, stats = ops.ln_linear(s, w2, b2, case["gamma"], case["beta"])
    want, p32 = (rr.ln_ref(s, case["gamma"], case["beta"], case["dy"], dt) for dt in (F64, F32))
    _hold_ln("ln_linear", groups, dict(y=y, mean=stats[:, 0], rstd=stats[:, 1]), want, p32, ("y", "mean", "rstd"), LN_T0)
    o64, o32 = F.linear(want["y"], w2.double(), b2.double()), F.linear(p32["y"], w2, b2)
    for gname, rows in groups.items():
        hold(f"ln_linear out[{gname}]", out, o64, o32, 1e-6 * 8, 5e-6, rows=rows)
    # backward: statistics in fp32 as a forward launch leaves them
    stats32 = torch.stack([want["mean"], want["rstd"]], 1).float()
    Wt = rr.randn(256, 256, seed=5, scale=1 / 16, device=DEV)
    dX, ds, dxd, dg, db = ops.ln_bwd_linear(case["dy"], Wt, s, stats32, case["gamma"])
    _hold_ln("ln_bwd_linear", groups, dict(ds=ds), want, p32, ("ds",), LN_T0)
    for gname, rows in groups.items():
        hold(f"ln_bwd_linear dX[{gname}]", dX, want["ds"] @ Wt.double(), p32["ds"] @ Wt, 1e-6 * 16, 3e-6, rows=rows)
    hold_w("dgamma", dg, want["dgamma"], p32["dgamma"], 1e-5)
    hold_w("dbeta", db, want["dbeta"], p32["dbeta"], 1e-5)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("c", [1e2, 1e3])
@pytest.mark.parametrize("M", [33, 530])
def test_fused_blocks_normalise_rows_with_a_common_component(M, c, p):
    """The launches that form the normalised sum themselves, with c added to the RESIDUAL input (their products see weights
    whose rows have zero mean, so the common component reaches the LayerNorm only): linear_layernorm_bf16_fwd
    (gemm_bf16_panel.hip:406-407, the epilogue's variance and rstd), ffn_fwd / ffn_bwd (dtype 0; engine.hip:1974 linear_ln and
    :1992 ln_bwd_dgrad, the LayerNorm code of gemm_small.hip:310-318 / :351-410 and rowops.hip:355-358) and
    combination_block_fwd / _bwd (dtype 0 and 2; comb_fused.hip:322-326 forward, :824-831 xh and ds in the backward) -- sum, y,
    mean, rstd against the fp64 statement with the entry's dropout mask; the backward halves on the forward's saved outputs
    (h / q | k, sum, stats: what the kernels read), against the LayerNorm's fp64 autograd carried through the block: dx / dYc,
    dq | dk, dG per row, the parameter gradients by rel_err.  The special rows of rr.ln_case reach these launches in
    test_fused_layernorms_on_special_rows.  Purpose as in test_add_layernorm_with_a_common_component.  t0: the unit-scale
    tolerances of the entries' tests (1e-5 for every ffn_bwd output, 5e-6 / 1e-5 for the block's backward)."""
    from fira_icse_amd import ops
    seed, site = 99, 46
    mask = (lambda: ops.dropout_mask(seed, site, M * 256, p).view(M, 256)) if p > 0 else (lambda: torch.ones(M, 256, device=DEV))
    lnst = lambda s: dict(mean=s.mean(1), rstd=1.0 / torch.sqrt(s.var(1, unbiased=False) + 1e-5))
    gamma, beta = 1 + rr.randn(256, seed=6, scale=0.1, device=DEV), rr.randn(256, seed=7, scale=0.1, device=DEV)
    # ---- bf16 panel product + LayerNorm epilogue: res carries c
    Mb = M if M >= 64 else M + 64                    # (the panel kernel takes M >= 64: 97 rows = one ragged panel)
    maskb = (lambda: ops.dropout_mask(seed, site, Mb * 256, p).view(Mb, 256)) if p > 0 else (lambda: torch.ones(Mb, 256, device=DEV))
    x, res = rr.randn(Mb, 256, seed=31, device=DEV), rr.randn(Mb, 256, seed=34, device=DEV) + c
    w, b = rr.randn(256, 256, seed=32, device=DEV) / 16, rr.randn(256, seed=33, device=DEV)
    wb, _ = ops.weight_shadow(w)
    y, s, stats = ops.linear_layernorm_bf16_fwd(x, wb, b, res, gamma, beta, p, seed=seed, site=site)
    ref = {}
    for dt in (F64, F32):
        si = (rr.r16(x.to(dt)) @ rr.r16(w.to(dt)).t() + b.to(dt)) * maskb().to(dt) + res.to(dt)
        ref[dt] = dict(lnst(si), s=si, y=F.layer_norm(si, (256,), gamma.to(dt), beta.to(dt), 1e-5))
    for n, t0 in (("s", 2e-6), ("y", 1e-5), ("rstd", 1e-5)):
        hold(f"linear_layernorm_bf16 {n}", dict(y=y, s=s, rstd=stats[:, 1])[n], ref[F64][n], ref[F32][n], 1e-6 * 16, t0)
    hold_mean("linear_layernorm_bf16 mean", stats[:, 0], ref[F64], ref[F32])
    # ---- FeedForward block: x carries c, the rows of W1 have zero mean
    F_ = 1024
    x = rr.randn(M, 256, seed=1, device=DEV) + c
    w1, b1 = rr.zero_mean_rows(rr.randn(F_, 256, seed=2, scale=0.06)).to(DEV), rr.randn(F_, seed=3, scale=0.1, device=DEV)
    w2, b2 = rr.randn(256, F_, seed=4, scale=0.03, device=DEV), rr.randn(256, seed=5, scale=0.1, device=DEV)
    h, summ, y, stats = ops.ffn_fwd(x, w1, b1, w2, b2, gamma, beta, dropout=p, seed=seed, site=site, dtype=0)
    ref = {}
    for dt in (F64, F32):
        hh = torch.relu(x.to(dt) @ w1.to(dt).t() + b1.to(dt))
        si = (hh @ w2.to(dt).t() + b2.to(dt)) * mask().to(dt) + x.to(dt)
        ref[dt] = dict(lnst(si), h=hh, s=si, y=F.layer_norm(si, (256,), gamma.to(dt), beta.to(dt), 1e-5))
    assert float(ref[F64]["s"].std(1).max()) < 3.0                   # the spread stayed at unit scale
    for n, t0 in (("h", 2e-6), ("s", 2e-6), ("y", 4e-6), ("rstd", 1e-5)):
        hold(f"ffn {n}", dict(h=h, y=y, s=summ, rstd=stats[:, 1])[n], ref[F64][n], ref[F32][n], 1e-6 * 16, t0)
    hold_mean("ffn mean", stats[:, 0], ref[F64], ref[F32])
    # backward from the SAVED h, pre-norm rows and statistics: the ReLU mask is the forward launch's own
    dy = rr.randn(M, 256, seed=8, device=DEV)
    dx, dw1, db1, dw2, db2, dg, db = ops.ffn_bwd(dy, x, h, summ, stats, w1, w2, gamma, dropout=p, seed=seed, site=site, dtype=0)
    bw = {}
    for dt in (F64, F32):
        r = rr.ln_ref(summ, gamma, beta, dy, dt)
        dyf = r["ds"] * mask().to(dt)
        dh = (dyf @ w2.to(dt)) * (h > 0)
        bw[dt] = dict(dx=r["ds"] + dh @ w1.to(dt), dw1=dh.t() @ x.to(dt), db1=dh.sum(0), dw2=dyf.t() @ h.to(dt), db2=dyf.sum(0),
                      dgamma=r["dgamma"], dbeta=r["dbeta"])
    hold("ffn dx", dx, bw[F64]["dx"], bw[F32]["dx"], 1e-6 * dy.double().norm(dim=1) * stats[:, 1].double(), 1e-5)
    for n, got in (("dw1", dw1), ("db1", db1), ("dw2", dw2), ("db2", db2), ("dgamma", dg), ("dbeta", db)):
        hold_w(f"ffn {n}", got, bw[F64][n], bw[F32][n], 1e-5)
    # ---- Combination block: Xc carries c, the rows of Wqk have zero mean
    inp = _block_inputs(M, 0.08, c=c)
    sg, so = 17, 18
    mg = ops.dropout_mask(seed, sg, M * 256, p).view(M, 256) if p > 0 else torch.ones(M, 256, device=DEV)
    mo = ops.dropout_mask(seed, so, M * 256, p).view(M, 256) if p > 0 else torch.ones(M, 256, device=DEV)
    want, p32 = _block_ref(inp, F64, mg, mo), _block_ref(inp, F32, mg, mo)
    for dtype in (0, 2):
        qk, cc, summ, y, stats = ops.combination_block_fwd(*inp, dropout=p, seed=seed, site_gate=sg, site_out=so, dtype=dtype)
        for n, t0 in (("s", 5e-6), ("y", 1e-5), ("rstd", 1e-5)):
            hold(f"combination_block[{dtype}] {n}", dict(y=y, s=summ, rstd=stats[:, 1])[n], want[n], p32[n], 1e-6 * 16, t0)
        hold_mean(f"combination_block[{dtype}] mean", stats[:, 0], want, p32)
        _hold_block_bwd(f"combination_block[{dtype}] bwd", inp, qk, summ, stats, mg, mo, p, seed, sg, so, dtype, False, 5e-6, 1e-5)


@pytest.mark.parametrize("dtype", [0, 2])
@pytest.mark.parametrize("c", [1e2, 1e3])
@pytest.mark.parametrize("N,density,p", [(33, 0.2, 0.1), (177, 0.1, 0.0)])
def test_gcn_layer_normalises_rows_with_a_common_component(N, density, p, c, dtype):
    """gcn_layer_fwd (gcn_fused.hip:370-371: the variance of the centred values and rstd; dtype 0 and 2) with c added to the node rows X, which are the residual input; the rows of
    W21 have zero mean, so the aggregate's common component c (A_hat 1) does not reach the product: sum, y, mean, rstd against
    the fp64 statement of test_gcn_layer_fused_fwd_bwd.  Purpose as in test_add_layernorm_with_a_common_component."""
    from fira_icse_amd import ops
    c = float(c)
    B = 3
    rowptr, col, val, dense = _graph_batch(B, N, density, seed=N + 1)
    n = B * N
    X = rr.randn(n, 256, seed=1, device=DEV) + c
    W21 = rr.zero_mean_rows(rr.randn(256, 256, seed=2, scale=0.06)).to(DEV)
    b2, c21 = rr.randn(256, seed=3, scale=0.1, device=DEV), rr.randn(256, seed=4, scale=0.1, device=DEV)
    gamma, beta = 1 + rr.randn(256, seed=5, scale=0.1, device=DEV), rr.randn(256, seed=6, scale=0.1, device=DEV)
    seed, site = 1234, 19
    summ, y, stats, rs = ops.gcn_layer_fwd(rowptr, col, val, X, W21.t().contiguous(), b2, c21, gamma, beta, dropout=p, seed=seed,
                                           site=site, dtype=dtype)
    mask = ops.dropout_mask(seed, site, n * 256, p).view(n, 256) if p > 0 else torch.ones(n, 256, device=DEV)
    ref = {}
    for dt in (F64, F32):
        A = torch.block_diag(*[dense[b] for b in range(B)]).to(dt)
        pre = (A @ X.to(dt)) @ W21.to(dt).t() + b2.to(dt) + A.sum(1, keepdim=True) * c21.to(dt)
        si = pre * mask.to(dt) + X.to(dt)
        ref[dt] = dict(s=si, y=F.layer_norm(si, (256,), gamma.to(dt), beta.to(dt), 1e-5), mean=si.mean(1),
                       rstd=1.0 / torch.sqrt(si.var(1, unbiased=False) + 1e-5))
    for name, t0 in (("s", 2e-6), ("y", 1e-5), ("rstd", 1e-5)):
        hold(f"gcn[{dtype}] {name}", dict(s=summ, y=y, rstd=stats[:, 1])[name], ref[F64][name], ref[F32][name], 1e-6 * 16, t0)
    hold_mean(f"gcn[{dtype}] mean", stats[:, 0], ref[F64], ref[F32])


@pytest.mark.parametrize("c", [1e2, 1e3])
@pytest.mark.parametrize("M", [97, 530])
def test_fused_layernorms_on_special_rows(M, c):
    """The special rows of rr.ln_case -- variance exactly 0, std 1e-3 and std 1e3 around c -- inside the launches that form
    their sum themselves.  With the LAST product's weight and bias zero (and dropout 0.1 of that zero), the launch's sum is its
    residual input bit for bit (asserted), so its own LayerNorm code normalises exactly those rows: ffn_fwd (W2 = 0),
    combination_block_fwd (Wo = 0; dtype 0 and 2; comb_fused.hip:322-326), gcn_layer_fwd (W21 = 0, c21 = 0; dtype 0 and 2;
    gcn_fused.hip:370-371), linear_layernorm_bf16_fwd (W = 0; gemm_bf16_panel.hip:406-407; it takes M >= 64, hence 97 rows).
    y, mean, rstd per row group against fp64 F.layer_norm; e32 = torch's fp32 layer_norm.  Purpose and t0 as in
    test_add_layernorm_with_a_common_component."""
    from fira_icse_amd import ops
    case = rr.ln_case(M, c, device=DEV)
    s = case["x"] + case["res"]
    gamma, beta = case["gamma"], case["beta"]
    want, p32 = (rr.ln_ref(s, gamma, beta, case["dy"], dt) for dt in (F64, F32))
    groups = rr.ln_groups(M)
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    names = ("y", "mean", "rstd")
    p, seed = 0.1, 7
    w1, b1 = rr.randn(1024, 256, seed=2, scale=0.06, device=DEV), rr.randn(1024, seed=3, scale=0.1, device=DEV)
    h, summ, y, stats = ops.ffn_fwd(s, w1, b1, z(256, 1024), z(256), gamma, beta, dropout=p, seed=seed, site=46, dtype=0)
    assert torch.equal(summ, s)
    _hold_ln("ffn", groups, dict(y=y, mean=stats[:, 0], rstd=stats[:, 1]), want, p32, names, LN_T0)
    Xc, Wqk, bqk, Wo, bo, vtab, mark, _, _ = _block_inputs(M, 0.08)
    for dtype in (0, 2):
        qk, cc, summ, y, stats = ops.combination_block_fwd(s, Wqk, bqk, z(256, 256), z(256), vtab, mark, gamma, beta, dropout=p,
                                                           seed=seed, site_gate=17, site_out=18, dtype=dtype)
        assert torch.equal(summ, s)
        _hold_ln(f"combination_block[{dtype}]", groups, dict(y=y, mean=stats[:, 0], rstd=stats[:, 1]), want, p32, names, LN_T0)
    B = 1 if M < 100 else 2
    rowptr, col, val, dense = _graph_batch(B, M // B, 0.1, seed=M)
    for dtype in (0, 2):
        summ, y, stats, rs = ops.gcn_layer_fwd(rowptr, col, val, s, z(256, 256), z(256), z(256), gamma, beta, dropout=p, seed=seed,
                                               site=19, dtype=dtype)
        assert torch.equal(summ, s)
        _hold_ln(f"gcn[{dtype}]", groups, dict(y=y, mean=stats[:, 0], rstd=stats[:, 1]), want, p32, names, LN_T0)
    wb, _ = ops.weight_shadow(z(256, 256))
    y, summ, stats = ops.linear_layernorm_bf16_fwd(rr.randn(M, 256, seed=31, device=DEV), wb, z(256), s, gamma, beta, p, seed=seed,
                                                   site=46)
    assert torch.equal(summ, s)
    _hold_ln("linear_layernorm_bf16", groups, dict(y=y, mean=stats[:, 0], rstd=stats[:, 1]), want, p32, names, LN_T0)


# ---------------------------------------------------------------------------------------------------------------- 6. bf16, per row
@pytest.mark.parametrize("M", [37, 530])
def test_one_plane_products_per_row(M):
    """linear_x3, linear_dgrad_x3, dgrad_x3_splitk (dtype 3: one bf16 plane; K = 250 and 1000 for the split-K form) and
    gemm_wgrad_panel (dtype 1) on the unit-scale operands of their existing tests, against the fp64 product of the ROUNDED
    operands -- per row.  With the Frobenius ratio those tests use, one wrong row of 530 adds 0.04 and fails too, but one of the
    2960 rows of a dK passes a 2e-2 tolerance; per row nothing hides at any size.  Bound: 3x the row_err of a torch fp32 product
    of the same rounded operands + the existing tolerance (2e-6; 3e-6 for the weight gradient)."""
    from fira_icse_amd import ops
    bf = lambda t: t.bfloat16().double()
    b32 = lambda t: t.bfloat16().float()
    x = rr.randn(M, 256, seed=1, device=DEV)
    W, b = rr.randn(512, 256, seed=2, scale=0.06, device=DEV), rr.randn(512, seed=3, scale=0.1, device=DEV)
    hold("linear_x3", ops.linear_x3(x, W, b, dtype=3), bf(x) @ bf(W).t() + b.double(), b32(x) @ b32(W).t() + b, 1e-6, 2e-6)
    dy, Wd, base = rr.randn(M, 512, seed=4, device=DEV), rr.randn(512, 256, seed=5, scale=0.06, device=DEV), rr.randn(M, 256, seed=6, device=DEV)
    dx = base.clone()
    ops.linear_dgrad_x3(dy, Wd, dx, dtype=3)
    hold("linear_dgrad_x3", dx, base.double() + bf(dy) @ bf(Wd), base + b32(dy) @ b32(Wd), 1e-6, 2e-6)
    for K in (250, 1000):
        pitch = (K + 63) // 64 * 64
        full = torch.full((M, pitch), float("nan"), device=DEV)
        full[:, :K] = rr.randn(M, K, seed=7, scale=0.05, device=DEV)
        dyk, Wk = full[:, :K], rr.randn(K, 256, seed=8, scale=0.06, device=DEV)
        dx = ops.dgrad_x3_splitk(dyk, Wk, base.clone(), dtype=3)
        hold(f"dgrad_x3_splitk K={K}", dx, base.double() + bf(dyk) @ bf(Wk), base + b32(dyk) @ b32(Wk), 1e-6, 2e-6)
    A, Bm = rr.randn(M, 256, seed=1, device=DEV), rr.randn(M, 256, seed=2, device=DEV)          # C [256, 256] += A^T B over M rows
    C0 = rr.randn(256, 256, seed=3, device=DEV)
    for split in (True, False):
        C = C0.clone()
        ops.gemm_wgrad_panel(A, Bm, C, None, dtype=1, split=split)
        hold(f"wgrad_panel split={split}", C, C0.double() + bf(A).t() @ bf(Bm), C0 + b32(A).t() @ b32(Bm), 1e-6, 3e-6)


@pytest.mark.parametrize("dtype", [1, 3])
@pytest.mark.parametrize("n", [37, 530])
def test_bf16_fused_blocks_per_row(n, dtype):
    """combination_block_fwd / combination_block_bwd and gcn_layer_fwd / gcn_layer_bwd with bf16 operands (dtype 1) and one plane (dtype 3) on unit-scale
    operands, per row, against the fp64 result of the rounded operands.  e32: the same statement in fp32.  The kernel rounds ITS
    fp32 aggregate / gate output to bf16, the references theirs: a few elements fall on the other side of a rounding boundary in
    each -- which is why t0 is the existing tests' 3e-5 / 5e-5 and not 2e-6."""
    from fira_icse_amd import ops
    p, seed, sg, so = 0.1, 4321, 17, 18
    inp = _block_inputs(n, 0.08)
    qk, c, summ, y, stats = ops.combination_block_fwd(*inp, dropout=p, seed=seed, site_gate=sg, site_out=so, dtype=dtype)
    mg = ops.dropout_mask(seed, sg, n * 256, p).view(n, 256)
    mo = ops.dropout_mask(seed, so, n * 256, p).view(n, 256)
    want, p32 = _block_ref(inp, F64, mg, mo, bf=True), _block_ref(inp, F32, mg, mo, bf=True)
    hold("block q", qk[:, :256], want["q"], p32["q"], 1e-6, 2e-6)
    hold("block k", qk[:, 256:], want["k"], p32["k"], 1e-6, 2e-6)
    hold("block c", c, want["c"], p32["c"], 1e-6, 5e-6)
    hold("block sum", summ, want["s"], p32["s"], 1e-6, 5e-5)
    hold("block y", y, want["y"], p32["y"], 1e-6, 1e-4)
    # backward, per row: dYc at 5e-6, dq | dk and dG at the existing test's bf16 t1 = 2e-4, dvtab 2e-4
    _hold_block_bwd("block bwd", inp, qk, summ, stats, mg, mo, p, seed, sg, so, dtype, True, 2e-4, 2e-4)
    N = n if n < 100 else 177
    B = 3
    rowptr, col, val, dense = _graph_batch(B, N, 0.1, seed=N + 1)
    m = B * N
    X = rr.randn(m, 256, seed=1, device=DEV)
    W21 = rr.randn(256, 256, seed=2, scale=0.06, device=DEV)
    b2, c21 = rr.randn(256, seed=3, scale=0.1, device=DEV), rr.randn(256, seed=4, scale=0.1, device=DEV)
    gamma, beta = inp[7], inp[8]
    summ, y, stats, rs = ops.gcn_layer_fwd(rowptr, col, val, X, W21.t().contiguous(), b2, c21, gamma, beta, dropout=p, seed=seed,
                                           site=19, dtype=dtype)
    mask = ops.dropout_mask(seed, 19, m * 256, p).view(m, 256)
    dY, dX0 = rr.randn(m, 256, seed=7, device=DEV), rr.randn(m, 256, seed=8, device=DEV)
    dX = dX0.clone()
    V = ops.gcn_layer_bwd(rowptr, col, val, dY, W21, dX, dtype=dtype)
    ref = {}
    for dt in (F64, F32):
        A = torch.block_diag(*[dense[b] for b in range(B)]).to(dt)
        pre = rr.r16(A @ X.to(dt)) @ rr.r16(W21.to(dt)).t() + b2.to(dt) + A.sum(1, keepdim=True) * c21.to(dt)
        si = pre * mask.to(dt) + X.to(dt)
        Vr = A @ dY.to(dt)
        ref[dt] = dict(s=si, y=F.layer_norm(si, (256,), gamma.to(dt), beta.to(dt), 1e-5), V=Vr,
                       dX=dX0.to(dt) + rr.r16(Vr) @ rr.r16(W21.to(dt)))
    for name, got, t0 in (("s", summ, 3e-5), ("y", y, 1.5e-4), ("V", V, 1e-6), ("dX", dX, 3e-5)):
        hold(f"gcn {name}", got, ref[F64][name], ref[F32][name], 1e-6, t0)
