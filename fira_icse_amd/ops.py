"""Thin tensor-level wrappers over the op-level C ABI (one reference op each; see include/fira_hip.h).

They take/return ``torch`` CUDA tensors, launch on the current stream and never fall back to PyTorch maths.
Used by the piecewise drop-in surface (``model.encoder`` / ``decoder`` / ``out_fc`` / ``copy_net``) and by the
per-kernel parity tests.
"""
from __future__ import annotations

import dataclasses

import torch

from . import _lib
from ._lib import check, cur_stream, ptr


def _f32(t):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "expected a contiguous fp32 CUDA tensor"
    return t


def _i32(t):
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous(), "expected a contiguous int32 CUDA tensor"
    return t


def gemm(A, B, *, transA=False, transB=True, bias=None, relu=False, out=None, accumulate=False, splitk=1,
         tile=0, dtype="f32"):
    """C = op(A) op(B) (+bias)(relu).  transB=True: B is an nn.Linear weight [N,K].  dtype "bf16": operands rounded to
    bf16 on the way to the matrix cores, fp32 accumulation and storage (fira_gemm_bf16)."""
    for t in (A, B):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1
    M, K = (A.shape[1], A.shape[0]) if transA else A.shape
    N = B.shape[0] if transB else B.shape[1]
    assert (B.shape[1] if transB else B.shape[0]) == K
    if out is None:
        out = torch.zeros((M, N), dtype=torch.float32, device=A.device) if accumulate else \
            torch.empty((M, N), dtype=torch.float32, device=A.device)
    flags = (1 if relu else 0) | (2 if accumulate else 0) | (tile << 4)     # tile: 0 auto, 1 128x128, 2 64x128, 3 64x64
    fn = _lib.lib().fira_gemm_bf16 if dtype == "bf16" else _lib.lib().fira_gemm_f32
    check(fn(cur_stream(), int(transA), int(transB), M, N, K, ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(out),
             out.stride(0), ptr(bias), flags, splitk), "fira_gemm_%s" % dtype)
    return out


def weight_shadow(W):
    """bf16 shadows of a 2-D fp32 weight: (as stored [rows, cols], transposed [cols, rows]), raw bf16 in int16 tensors."""
    rows, cols = W.shape
    wb = torch.empty((rows, cols), dtype=torch.int16, device=W.device)
    wbt = torch.empty((cols, rows), dtype=torch.int16, device=W.device)
    check(_lib.lib().fira_weight_shadow(cur_stream(), rows, cols, ptr(_f32(W)), ptr(wb), ptr(wbt)), "fira_weight_shadow")
    return wb, wbt


def gemm_wb(A, Bb, *, bias=None, relu=False, out=None, accumulate=False, splitk=1):
    """C = A . Bb^T with Bb a bf16 shadow [N, K] (int16 tensor, any row pitch that is a multiple of 8)."""
    M, K = A.shape
    N = Bb.shape[0]
    assert Bb.shape[1] == K and Bb.dtype == torch.int16 and Bb.stride(1) == 1
    if out is None:
        out = (torch.zeros if accumulate else torch.empty)((M, N), dtype=torch.float32, device=A.device)
    flags = (1 if relu else 0) | (2 if accumulate else 0)
    check(_lib.lib().fira_gemm_bf16_wb(cur_stream(), M, N, K, ptr(A), A.stride(0), ptr(Bb), Bb.stride(0), ptr(out),
                                       out.stride(0), ptr(bias), flags, splitk), "fira_gemm_bf16_wb")
    return out


def csr_spmm(rowptr, col, val, X, graph_rows=0, variant=0, out=None, dtype=0, auto=False):
    """Z = A_hat X over a block-diagonal CSR.  variant 1/2: CSR gather kernels, 3/4: block-dense fp32 / bf16 MFMA;
    ``auto`` (with variant 0): the library picks by density (fira_csr_spmm), ``dtype`` 1 allows bf16 operands."""
    for t in (X,) + ((out,) if out is not None else ()):      # rows may be strided (a column block of a wider buffer)
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1
    Y = torch.empty_like(X, memory_format=torch.contiguous_format) if out is None else out
    assert Y.shape == X.shape
    if auto or variant >= 3:
        check(_lib.lib().fira_csr_spmm(cur_stream(), X.shape[0], int(col.numel()), ptr(_i32(rowptr)), ptr(_i32(col)),
                                       ptr(_f32(val)), ptr(X), X.stride(0), ptr(Y), Y.stride(0), graph_rows, variant, dtype),
              "fira_csr_spmm")
        return Y
    check(_lib.lib().fira_csr_spmm_f32(cur_stream(), X.shape[0], ptr(_i32(rowptr)), ptr(_i32(col)), ptr(_f32(val)),
                                       ptr(X), X.stride(0), ptr(Y), Y.stride(0), graph_rows, variant),
          "fira_csr_spmm_f32")
    return Y


def embed_gather(idx, table, pos=None, out=None, out_bstride=None, out_off=0):
    B, L = idx.shape
    if out is None:
        out = torch.empty((B, L, 256), dtype=torch.float32, device=table.device)
        out_bstride = L
    check(_lib.lib().fira_embed_gather_fwd(cur_stream(), B, L, ptr(_i32(idx)), ptr(_f32(table)), ptr(pos), ptr(out),
                                           out_bstride, out_off), "fira_embed_gather_fwd")
    return out


def embed_scatter_add(idx, dtable, dout, out_bstride, out_off, padding_idx):
    B, L = idx.shape
    check(_lib.lib().fira_embed_gather_bwd(cur_stream(), B, L, ptr(_i32(idx)), ptr(_f32(dtable)), ptr(_f32(dout)),
                                           out_bstride, out_off, padding_idx), "fira_embed_gather_bwd")
    return dtable


def combination_fwd(qk, vtab, mark, dropout=0.0, seed=0, site=0):
    M = qk.shape[0]
    out = torch.empty((M, 256), dtype=torch.float32, device=qk.device)
    check(_lib.lib().fira_combination_fwd(cur_stream(), M, ptr(_f32(qk)), ptr(_f32(vtab)), ptr(_i32(mark)), ptr(out),
                                          dropout, seed, site), "fira_combination_fwd")
    return out


def combination_bwd(qk, vtab, mark, dout, dropout=0.0, seed=0, site=0):
    M = qk.shape[0]
    dqk = torch.empty_like(qk)
    dvtab = torch.zeros_like(vtab)
    check(_lib.lib().fira_combination_bwd(cur_stream(), M, ptr(_f32(qk)), ptr(_f32(vtab)), ptr(_i32(mark)),
                                          ptr(_f32(dout)), ptr(dqk), ptr(dvtab), dropout, seed, site),
          "fira_combination_bwd")
    return dqk, dvtab


def add_layernorm_fwd(x, res, gamma, beta, dropout=0.0, seed=0, site=0):
    """Returns (y, pre-norm sum, stats[M,2]); ``x`` is consumed (overwritten with the sum)."""
    M = x.shape[0]
    y = torch.empty_like(x)
    stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
    check(_lib.lib().fira_add_layernorm_fwd(cur_stream(), M, ptr(_f32(x)), ptr(res), ptr(_f32(gamma)), ptr(_f32(beta)),
                                            ptr(y), ptr(stats), dropout, seed, site), "fira_add_layernorm_fwd")
    return y, x, stats


def linear_presum(x, w, bias, res, dropout=0.0, seed=0, site=0):
    """Pre-norm sum of a residual block: dropout(x @ w.T + bias) + res  (w [256, K])."""
    M, K = x.shape
    assert w.shape == (256, K) and x.stride(1) == 1
    s = torch.empty((M, 256), dtype=torch.float32, device=x.device)
    check(_lib.lib().fira_linear_presum_f32(cur_stream(), M, K, ptr(x), x.stride(0), ptr(_f32(w)), ptr(bias), ptr(_f32(res)),
                                            ptr(s), dropout, seed, site), "fira_linear_presum_f32")
    return s


def ln_linear(s, w, bias, gamma, beta, relu=False):
    """(LN(s) @ w.T + bias [relu], LN(s), stats[M,2]) in one launch: the LayerNorm runs in the product's prologue."""
    M = s.shape[0]
    N = w.shape[0]
    assert w.shape[1] == 256 and s.shape[1] == 256 and s.stride(1) == 1
    y = torch.empty((M, N), dtype=torch.float32, device=s.device)
    x = torch.empty((M, 256), dtype=torch.float32, device=s.device)
    stats = torch.empty((M, 2), dtype=torch.float32, device=s.device)
    check(_lib.lib().fira_ln_linear_f32(cur_stream(), M, N, ptr(s), s.stride(0), ptr(_f32(w)), ptr(bias), ptr(y), N, int(relu),
                                        ptr(_f32(gamma)), ptr(_f32(beta)), ptr(x), ptr(stats)), "fira_ln_linear_f32")
    return y, x, stats


def linear_layernorm_bf16_fwd(x, wb, bias, res, gamma, beta, dropout=0.0, seed=0, site=0):
    """bf16 twin of linear_layernorm_fwd: ``wb`` is the [256, 256] bf16 shadow (int16 tensor) of the weight."""
    M, K = x.shape
    assert K == 256 and wb.shape == (256, 256) and wb.dtype == torch.int16 and x.stride(1) == 1
    y = torch.empty((M, 256), dtype=torch.float32, device=x.device)
    s = torch.empty_like(y)
    stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
    check(_lib.lib().fira_linear_layernorm_bf16_fwd(cur_stream(), M, ptr(x), x.stride(0), ptr(wb), wb.stride(0), ptr(bias),
                                                    ptr(res), ptr(_f32(gamma)), ptr(_f32(beta)), ptr(s), ptr(y), ptr(stats),
                                                    dropout, seed, site), "fira_linear_layernorm_bf16_fwd")
    return y, s, stats


def add_layernorm_bwd(dy, s, stats, gamma, dropout=0.0, seed=0, site=0, want_dx_drop=False):
    M = dy.shape[0]
    ds = torch.empty_like(dy)
    dxd = torch.empty_like(dy) if want_dx_drop else None
    dg = torch.zeros(256, dtype=torch.float32, device=dy.device)
    db = torch.zeros(256, dtype=torch.float32, device=dy.device)
    check(_lib.lib().fira_add_layernorm_bwd(cur_stream(), M, ptr(_f32(dy)), ptr(_f32(s)), ptr(_f32(stats)),
                                            ptr(_f32(gamma)), ptr(ds), ptr(dxd), ptr(dg), ptr(db), dropout, seed, site),
          "fira_add_layernorm_bwd")
    return ds, dxd, dg, db


def ln_bwd_linear(dy, Wt, summ, stats, gamma, relu_mask=None, dropout=0.0, seed=0, site=0):
    """fira_ln_bwd_linear_f32: (dX, ds, dx_drop, dgamma, dbeta) -- LayerNorm backward in the prologue of dX = dx_drop . Wt."""
    M, N = dy.shape[0], Wt.shape[1]
    dX = torch.empty((M, N), dtype=torch.float32, device=dy.device)
    ds, dxd = torch.empty_like(dy), torch.empty_like(dy)
    dg = torch.zeros(256, dtype=torch.float32, device=dy.device)
    db = torch.zeros(256, dtype=torch.float32, device=dy.device)
    part = torch.empty(((M + 31) // 32) * 512, dtype=torch.float32, device=dy.device)
    check(_lib.lib().fira_ln_bwd_linear_f32(cur_stream(), M, N, ptr(_f32(dy)), ptr(_f32(Wt)), ptr(dX),
                                            ptr(None if relu_mask is None else _f32(relu_mask)), ptr(_f32(summ)),
                                            ptr(_f32(stats)), ptr(_f32(gamma)), ptr(ds), ptr(dxd), ptr(dg), ptr(db), ptr(part),
                                            dropout, seed, site), "fira_ln_bwd_linear_f32")
    return dX, ds, dxd, dg, db


def dropout_mask(seed, site, n, p, device="cuda"):
    """Scale factors (0 or 1/(1-p)) of dropout site ``site`` for element indices 0..n-1 under ``seed``."""
    out = torch.empty(n, dtype=torch.float32, device=device)
    check(_lib.lib().fira_dropout_mask(cur_stream(), seed, site, n, p, ptr(out)), "fira_dropout_mask")
    return out


def colsum(X):
    out = torch.zeros(X.shape[1], dtype=torch.float32, device=X.device)
    check(_lib.lib().fira_colsum_f32(cur_stream(), X.shape[0], X.shape[1], ptr(_f32(X)), X.stride(0), ptr(out)),
          "fira_colsum_f32")
    return out


def gcn_weight_planes(B):
    """fira_gcn_weight_planes: the three bf16 planes (fragment order) of n stacked [256, 256] fp32 matrices B[n][k] for the
    FIRA_F32X3 form of fira_gcn_layer_{fwd,bwd} (out = U B^T)."""
    B = _f32(B).contiguous()
    n = B.numel() // (256 * 256)
    planes = torch.empty(n * 3 * 256 * 256, dtype=torch.int16, device=B.device)
    check(_lib.lib().fira_gcn_weight_planes(cur_stream(), n, ptr(B), ptr(planes)), "fira_gcn_weight_planes")
    return planes


def linear_x3(x, W, bias=None, dtype=2, ldo=None):
    """fira_linear_x3: out = x W^T + bias, x [M, 256], W [N, 256] with N a multiple of 256, on the bf16 matrix cores -- dtype 2:
    three bf16 terms per operand (fp32-accurate), 3: one plane (the bf16 mode's rounding).  Returns out [M, N] (row pitch ldo)."""
    x = _f32(x)
    M, N = x.shape[0], W.shape[0]
    planes = gcn_weight_planes(W)
    ldo = N if ldo is None else ldo
    out = torch.zeros((M, ldo), dtype=torch.float32, device=x.device)
    check(_lib.lib().fira_linear_x3(cur_stream(), M, N, ptr(x), x.stride(0), ptr(planes), ptr(None if bias is None else _f32(bias)),
                                    ptr(out), ldo, dtype), "fira_linear_x3")
    return out[:, :N]


def linear_dgrad_x3(dy, W, dx=None, dtype=2):
    """fira_linear_dgrad_x3: dx (+)= dy W for W [K, 256] (K a multiple of 256), dy [M, K]; dx None: a fresh result."""
    assert dy.is_cuda and dy.dtype == torch.float32 and dy.stride(1) == 1          # (a column slice of wider rows is fine)
    M, K = dy.shape
    Wt = _f32(W).view(K // 256, 256, 256).transpose(1, 2).contiguous()
    planes = gcn_weight_planes(Wt)
    acc = dx is not None
    if dx is None:
        dx = torch.empty((M, 256), dtype=torch.float32, device=dy.device)
    check(_lib.lib().fira_linear_dgrad_x3(cur_stream(), M, K, ptr(dy), dy.stride(0), ptr(planes), ptr(dx), dx.stride(0), 1 if acc else 0,
                                          dtype), "fira_linear_dgrad_x3")
    return dx


def dgrad_x3_splitk(dy, W, dx, dtype=2):
    """fira_dgrad_x3_splitk: dx += dy W, dy [M, K] (row pitch a multiple of 4 floats), W [K, 256], K any size."""
    assert dy.is_cuda and dy.dtype == torch.float32 and dy.stride(1) == 1
    M, K = dy.shape
    ws = torch.empty(_lib.lib().fira_dgrad_x3_splitk_planes_bytes(K), dtype=torch.uint8, device=dy.device)
    check(_lib.lib().fira_dgrad_x3_splitk(cur_stream(), M, K, ptr(dy), dy.stride(0), ptr(_f32(W)), ptr(ws), ptr(dx), dx.stride(0),
                                          dtype), "fira_dgrad_x3_splitk")
    return dx


def gcn_layer_fwd(rowptr, col, val, X, W21t, bias, c21, gamma, beta, dropout=0.0, seed=0, site=0, dtype=0, want_rowsum=True):
    """fira_gcn_layer_fwd: (sum, y, stats, rowsum) of one folded GCN layer on the CSR adjacency (global column ids);
    W21t = W21^T contiguous.  dtype 2 / 3 (FIRA_F32X3 / FIRA_BF16X1): the planes of W21 are formed here."""
    n = X.shape[0]
    if dtype >= 2:
        W21t = gcn_weight_planes(_f32(W21t).t().contiguous())
    else:
        W21t = _f32(W21t)
    summ, y = torch.empty_like(X), torch.empty_like(X)
    stats = torch.empty((n, 2), dtype=torch.float32, device=X.device)
    rs = torch.empty(n, dtype=torch.float32, device=X.device) if want_rowsum else None
    check(_lib.lib().fira_gcn_layer_fwd(cur_stream(), n, ptr(_i32(rowptr)), ptr(_i32(col)), ptr(_f32(val)), ptr(_f32(X)),
                                        ptr(W21t), ptr(_f32(bias)), ptr(_f32(c21)), ptr(_f32(gamma)), ptr(_f32(beta)),
                                        ptr(summ), ptr(y), ptr(stats), ptr(rs), dropout, seed, site, dtype),
          "fira_gcn_layer_fwd")
    return summ, y, stats, rs


def combination_block_fwd(Xc, Wqk, bqk, Wo, bo, vtab, mark, gamma, beta, dropout=0.0, seed=0, site_gate=0, site_out=0, y=None,
                          y_rows=None, dtype=0):
    """fira_combination_block_fwd: (qk, c, sum, y, stats) of one Combination block on the code rows Xc [n,256]; Wqk [512,256]
    and Wo [256,256] as nn.Linear stores them (transposed here: the kernel streams k-major copies); vtab [4, >=256] rows of the
    projected mark table (row stride = vtab.stride(0)).  y / y_rows: optional node buffer and row map for the output rows."""
    n = Xc.shape[0]
    dev = Xc.device
    assert vtab.is_cuda and vtab.dtype == torch.float32 and vtab.stride(1) == 1 and vtab.shape[0] == 4, "vtab: fp32 rows"
    if dtype >= 2:          # FIRA_F32X3 / FIRA_BF16X1: planes of Wq | Wk | Wo as stored
        WqT = WkT = WoT = gcn_weight_planes(torch.cat([_f32(Wqk), _f32(Wo)], 0))
    else:
        WqT, WkT, WoT = (_f32(Wqk[:256]).t().contiguous(), _f32(Wqk[256:]).t().contiguous(), _f32(Wo).t().contiguous())
    qk = torch.empty((n, 512), dtype=torch.float32, device=dev)
    c, summ = torch.empty_like(Xc), torch.empty_like(Xc)
    if y is None:
        y = torch.empty_like(Xc)
    stats = torch.empty((n, 2), dtype=torch.float32, device=dev)
    yr = None if y_rows is None else _i32(y_rows)
    check(_lib.lib().fira_combination_block_fwd(cur_stream(), n, ptr(_f32(Xc)), ptr(WqT), ptr(WkT), ptr(WoT), ptr(_f32(bqk)),
                                                ptr(_f32(bo)), ptr(vtab), vtab.stride(0), ptr(_i32(mark)), ptr(qk), ptr(c),
                                                ptr(_f32(gamma)), ptr(_f32(beta)), ptr(summ), ptr(y), ptr(yr), ptr(stats),
                                                dropout, seed, site_gate, site_out, dtype), "fira_combination_block_fwd")
    return qk, c, summ, y, stats


def combination_block_bwd(dG, rows, summ, stats, gamma, Wo, Wqk, qk, vtab, mark, dropout=0.0, seed=0, site_gate=0, site_out=0,
                          dtype=0):
    """fira_combination_block_bwd: dG [N,256] is updated in place at rows[r]; returns (dYc, dqk, dgamma, dbeta, dvtab)."""
    n = summ.shape[0]
    dev = summ.device
    assert vtab.is_cuda and vtab.dtype == torch.float32 and vtab.stride(1) == 1 and vtab.shape[0] == 4, "vtab: fp32 rows"
    dYc = torch.empty((n, 256), dtype=torch.float32, device=dev)
    dqk = torch.empty((n, 512), dtype=torch.float32, device=dev)
    dgamma, dbeta = torch.zeros(256, device=dev), torch.zeros(256, device=dev)
    dvtab = torch.zeros((4, 256), device=dev)
    part = torch.empty(_lib.lib().fira_combination_block_bwd_part_floats(), dtype=torch.float32, device=dev)
    if dtype >= 2:          # FIRA_F32X3 / FIRA_BF16X1: planes of Wq^T | Wk^T | Wo^T
        Wo = gcn_weight_planes(torch.stack([_f32(Wqk[:256]).t(), _f32(Wqk[256:]).t(), _f32(Wo).t()]).contiguous())
    else:
        Wo = _f32(Wo)
    check(_lib.lib().fira_combination_block_bwd(cur_stream(), n, ptr(_f32(dG)), ptr(_i32(rows)), ptr(_f32(summ)), ptr(_f32(stats)),
                                                ptr(_f32(gamma)), ptr(Wo), ptr(_f32(Wqk)), ptr(_f32(qk)), ptr(vtab),
                                                vtab.stride(0), ptr(_i32(mark)), ptr(dYc), ptr(dqk), ptr(dgamma), ptr(dbeta),
                                                ptr(dvtab), 256, ptr(part), dropout, seed, site_gate, site_out, dtype),
          "fira_combination_block_bwd")
    return dYc, dqk, dgamma, dbeta, dvtab


def gcn_layer_bwd(rowptr, col, val, dY, W21, dX, dtype=0):
    """fira_gcn_layer_bwd: V = A_hat dY (returned), dX += V W21 in place."""
    V = torch.empty_like(dY)
    W = gcn_weight_planes(_f32(W21).t().contiguous()) if dtype >= 2 else _f32(W21)     # (FIRA_F32X3: out = V B^T with B = W21^T)
    check(_lib.lib().fira_gcn_layer_bwd(cur_stream(), dY.shape[0], ptr(_i32(rowptr)), ptr(_i32(col)), ptr(_f32(val)),
                                        ptr(_f32(dY)), ptr(W), ptr(V), ptr(_f32(dX)), dtype), "fira_gcn_layer_bwd")
    return V


def attention_ragged_fwd(q, k, v, key_valid, q_off, Tq, Tk, causal=False, self_kv=False, dtype=0, heads=8, k_off=None):
    """The engine's form (fira_attention_fwd_ex): q [R,256] compact query rows, commit b's are q_off[b] .. q_off[b+1]
    (<= Tq of them); k / v [B*Tk,256] dense, or the same compact rows with self_kv, or (k_off [B+1]) RAGGED key rows:
    commit b's keys are rows k_off[b] .. k_off[b+1] of k / v and key_valid is a flat mask over those rows;
    dtype 1 = bf16 MFMA."""
    B = q_off.numel() - 1
    o = torch.zeros_like(q)
    ko = None if k_off is None else _i32(k_off)
    check(_lib.lib().fira_attention_fwd_ex(cur_stream(), B, heads, Tq, Tk, ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v),
                                           v.stride(0), ptr(_i32(key_valid)), int(causal), 0, ptr(o), 256, ptr(_i32(q_off)),
                                           int(self_kv), dtype, ptr(ko)), "fira_attention_fwd_ex")
    return o


def attention_ragged_bwd(q, k, v, key_valid, o, do, q_off, Tq, Tk, causal=False, self_kv=False, dtype=0, heads=8, k_off=None,
                         fill=0.0):
    """fill: value the gradient buffers hold before the call (the kernel must overwrite every row it owns)."""
    B = q_off.numel() - 1
    dq, dk, dv = torch.full_like(q, fill), torch.full_like(k, fill), torch.full_like(v, fill)
    ko = None if k_off is None else _i32(k_off)
    check(_lib.lib().fira_attention_bwd_ex(cur_stream(), B, heads, Tq, Tk, ptr(q), q.stride(0), ptr(k), k.stride(0), ptr(v),
                                           v.stride(0), ptr(_i32(key_valid)), int(causal), 0, ptr(_f32(o)), 256,
                                           ptr(_f32(do)), 256, ptr(dq), dq.stride(0), ptr(dk), dk.stride(0), ptr(dv),
                                           dv.stride(0), ptr(_i32(q_off)), int(self_kv), dtype, ptr(ko)),
          "fira_attention_bwd_ex")
    return dq, dk, dv


def attention_fwd(q, k, v, key_valid, causal=False, q_pos0=0, heads=8):
    """q [B,Tq,256], k/v [B,Tk,256] (any row stride), key_valid int32 [B,Tk] -> o [B,Tq,256]."""
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    o = torch.empty((B, Tq, 256), dtype=torch.float32, device=q.device)
    check(_lib.lib().fira_attention_fwd(cur_stream(), B, heads, Tq, Tk, ptr(q), q.stride(1), ptr(k), k.stride(1),
                                        ptr(v), v.stride(1), ptr(_i32(key_valid)), int(causal), q_pos0, ptr(o), 256),
          "fira_attention_fwd")
    return o


def decode_attention(q, k, v, key_valid, tk=None, qpk=1, heads=8, knew=None, vnew=None, k_off=None):
    """One query per row: q [BR,256] (any row stride), k / v [BR/qpk, kb, 256] (any row stride), key_valid int32
    [BR/qpk, kvb] -> o [BR,256].  knew / vnew [BR,256] (row stride = their stride(0)): key tk-1 of every row comes from
    them and is appended to k / v in place.  k_off [BR/qpk + 1]: ragged key rows -- k / v are [rows, 256] (any row stride),
    entry e's keys are rows k_off[e] .. k_off[e+1], key_valid a flat mask over those rows (tk = the largest range)."""
    BR = q.shape[0]
    if k_off is not None:
        kb = kvb = tk
        ldk, ldv = k.stride(0), v.stride(0)
    else:
        kb, kvb = k.shape[1], key_valid.shape[1]
        ldk, ldv = k.stride(1), v.stride(1)
    tk = kb if tk is None else tk
    o = torch.empty((BR, 256), dtype=torch.float32, device=q.device)
    ko = None if k_off is None else _i32(k_off)
    check(_lib.lib().fira_decode_attention(cur_stream(), BR, heads, tk, ptr(q), q.stride(0), ptr(k), ldk, ptr(v),
                                           ldv, ptr(_i32(key_valid)), ptr(o), 256, kb, kvb, qpk, ptr(knew),
                                           ptr(vnew), knew.stride(0) if knew is not None else 0,
                                           ptr(k) if knew is not None else None, ptr(v) if knew is not None else None,
                                           ptr(ko)),
          "fira_decode_attention")
    return o


def attention_bwd(q, k, v, key_valid, o, do, causal=False, q_pos0=0, heads=8):
    B, Tq, _ = q.shape
    Tk = k.shape[1]
    dq = torch.empty((B, Tq, 256), dtype=torch.float32, device=q.device)
    dk = torch.empty((B, Tk, 256), dtype=torch.float32, device=q.device)
    dv = torch.empty((B, Tk, 256), dtype=torch.float32, device=q.device)
    check(_lib.lib().fira_attention_bwd(cur_stream(), B, heads, Tq, Tk, ptr(q), q.stride(1), ptr(k), k.stride(1),
                                        ptr(v), v.stride(1), ptr(_i32(key_valid)), int(causal), q_pos0, ptr(_f32(o)),
                                        256, ptr(_f32(do)), 256, ptr(dq), 256, ptr(dk), 256, ptr(dv), 256),
          "fira_attention_bwd")
    return dq, dk, dv


def copy_score_fwd(src, tgt, w, bias):
    B, S, _ = src.shape
    T = tgt.shape[1]
    score = torch.empty((B, T, S), dtype=torch.float32, device=src.device)
    check(_lib.lib().fira_copy_score_fwd(cur_stream(), B, T, S, ptr(_f32(src)), ptr(_f32(tgt)), ptr(_f32(w)),
                                         ptr(_f32(bias)), ptr(score)), "fira_copy_score_fwd")
    return score


def copy_score_bwd(src, tgt, w, dscore):
    B, S, _ = src.shape
    T = tgt.shape[1]
    dsrc = torch.empty_like(src)
    dtgt = torch.zeros_like(tgt)
    dw = torch.zeros(256, dtype=torch.float32, device=src.device)
    db = torch.zeros(1, dtype=torch.float32, device=src.device)
    check(_lib.lib().fira_copy_score_bwd(cur_stream(), B, T, S, ptr(_f32(src)), ptr(_f32(tgt)), ptr(_f32(w)),
                                         ptr(_f32(dscore)), ptr(dsrc), ptr(dtgt), ptr(dw), ptr(db)),
          "fira_copy_score_bwd")
    return dsrc, dtgt, dw, db


def head_loss(logits, score, mem_valid, gate_logits, tar_label, V, compact_row=None, want_grad=True, argmax=False):
    """In place: logits/score/gate_logits become their gradients when want_grad.  Returns (loss_sum, n_tok, ids)."""
    B, T = tar_label.shape
    S = score.shape[-1]
    loss = torch.zeros(1, dtype=torch.float32, device=logits.device)
    ntok = torch.zeros(1, dtype=torch.int32, device=logits.device)
    ids = torch.empty((B, T), dtype=torch.int32, device=logits.device) if argmax else None
    check(_lib.lib().fira_head_loss(cur_stream(), B * T, T, V, S, ptr(compact_row), ptr(_f32(logits)),
                                    logits.stride(0), ptr(_f32(score)), ptr(_i32(mem_valid)), ptr(_f32(gate_logits)),
                                    ptr(_i32(tar_label)), ptr(loss), ptr(ntok), ptr(ids), int(want_grad)),
          "fira_head_loss")
    return loss, ntok, ids


# ---- the forms the engine calls (fira_*_ex and the row kernels of the step's tail).  They allocate nothing: the caller owns
# every buffer, so that a test can pre-fill it with sentinels.
def copy_score_fwd_ex(src, tgt, w, bias, score, T, qpk=1, mem_valid=None, tar_label=None, V=0, t_off=None):
    """src [B/qpk, S, 256]; tgt / score: B*T rows, or (t_off [B+1]) the ragged rows t_off[b] .. t_off[b+1]; written in place."""
    S = src.shape[1]
    B = src.shape[0] * qpk
    opt = lambda t: None if t is None else _i32(t)
    check(_lib.lib().fira_copy_score_fwd_ex(cur_stream(), B, T, S, ptr(_f32(src)), ptr(_f32(tgt)), ptr(_f32(w)),
                                            ptr(_f32(bias)), ptr(_f32(score)), qpk, ptr(opt(mem_valid)), ptr(opt(tar_label)),
                                            V, ptr(opt(t_off))), "fira_copy_score_fwd_ex")
    return score


def copy_score_bwd_blocks(B, S):
    n = _lib.lib().fira_copy_score_bwd_blocks(B, S)
    if n < 0:
        check(n, "fira_copy_score_bwd_blocks")
    return n


def copy_part_stride():
    return _lib.lib().fira_copy_part_stride()


def copy_score_bwd_ex(src, tgt, w, dscore, dsrc, dtgt, dw, dbias, T, mem_valid=None, part=None, t_off=None):
    """dsrc is overwritten; dtgt (and dw / dbias, or with ``part`` the partial rows instead) are accumulated into."""
    B, S = src.shape[0], src.shape[1]
    opt = lambda t: None if t is None else _i32(t)
    optf = lambda t: None if t is None else _f32(t)
    check(_lib.lib().fira_copy_score_bwd_ex(cur_stream(), B, T, S, ptr(_f32(src)), ptr(_f32(tgt)), ptr(_f32(w)),
                                            ptr(_f32(dscore)), ptr(_f32(dsrc)), ptr(_f32(dtgt)), ptr(optf(dw)),
                                            ptr(optf(dbias)), ptr(opt(mem_valid)), ptr(optf(part)), ptr(opt(t_off))),
          "fira_copy_score_bwd_ex")


def head_loss_ex(logits, score, mem_valid, gate_logits, tar_label, V, compact_row=None, row_bt=None, want_grad=True,
                 argmax=False):
    """fira_head_loss on the rows of ``score`` (row r = flat position row_bt[r]; None: r itself).  In place as head_loss."""
    B, T = tar_label.shape
    R, S = score.shape
    loss = torch.zeros(1, dtype=torch.float32, device=logits.device)
    ntok = torch.zeros(1, dtype=torch.int32, device=logits.device)
    ids = torch.empty(R, dtype=torch.int32, device=logits.device) if argmax else None
    opt = lambda t: None if t is None else _i32(t)
    check(_lib.lib().fira_head_loss_ex(cur_stream(), R, T, V, S, ptr(opt(compact_row)), ptr(_f32(logits)), logits.stride(0),
                                       ptr(_f32(score)), ptr(_i32(mem_valid)), ptr(_f32(gate_logits)), ptr(_i32(tar_label)),
                                       ptr(loss), ptr(ntok), ptr(ids), int(want_grad), ptr(opt(row_bt))),
          "fira_head_loss_ex")
    return loss, ntok, ids


def deferred_reduce_max():
    return _lib.lib().fira_deferred_reduce_max()


def deferred_reduce(entries):
    """entries: (dst [width], src partial rows, width, n_part, stride) tuples; one launch: dst[c] += sum_p src[p*stride + c]."""
    arr = (_lib.RedEntry * max(len(entries), 1))()
    for i, (dst, src, width, n_part, stride) in enumerate(entries):       # (views allowed: src may start inside a wider row)
        assert dst.is_cuda and src.is_cuda and dst.dtype == src.dtype == torch.float32
        arr[i] = _lib.RedEntry(dst.data_ptr(), src.data_ptr(), width, n_part, stride)
    check(_lib.lib().fira_deferred_reduce(cur_stream(), len(entries), arr), "fira_deferred_reduce")


def rows_move(mode, R, W, out, ld_out, inp, ld_in, src=None, dst=None):
    """fira_rows_move on views: ``out`` / ``inp`` start at the first moved column of their (wider) matrices."""
    opt = lambda t: None if t is None else _i32(t)
    assert out.is_cuda and inp.is_cuda and out.dtype == inp.dtype == torch.float32
    check(_lib.lib().fira_rows_move(cur_stream(), mode, R, W, ptr(out), ld_out, ptr(inp), ld_in, ptr(opt(src)),
                                    ptr(opt(dst))), "fira_rows_move")


def rank2_rows(g, w):
    out = torch.empty((g.shape[0], 256), dtype=torch.float32, device=g.device)
    check(_lib.lib().fira_rank2_rows(cur_stream(), g.shape[0], ptr(_f32(g)), ptr(_f32(w)), ptr(out)), "fira_rank2_rows")
    return out


def colsum_weighted(X, N, out, row_weight=None):
    """out[:N] += sum_m row_weight[m] * X[m, :N]; X [M, ldx >= N]."""
    check(_lib.lib().fira_colsum_weighted(cur_stream(), X.shape[0], N, ptr(_f32(X)), X.stride(0), ptr(_f32(out)),
                                          ptr(None if row_weight is None else _f32(row_weight))), "fira_colsum_weighted")
    return out


def embed_rows_fwd(row_bt, idx, table, pos):
    R, T = row_bt.numel(), idx.shape[1]
    out = torch.empty((R, 256), dtype=torch.float32, device=table.device)
    check(_lib.lib().fira_embed_rows_fwd(cur_stream(), R, T, ptr(_i32(row_bt)), ptr(_i32(idx)), ptr(_f32(table)),
                                         ptr(_f32(pos)), ptr(out)), "fira_embed_rows_fwd")
    return out


def embed_rows_bwd(row_bt, idx, dtable, dout, padding_idx=0):
    check(_lib.lib().fira_embed_rows_bwd(cur_stream(), row_bt.numel(), ptr(_i32(row_bt)), ptr(_i32(idx)), ptr(_f32(dtable)),
                                         ptr(_f32(dout)), padding_idx), "fira_embed_rows_bwd")
    return dtable


def embed_grouped_bwd(item_tok, item_ptr, rows, dtable, dnode):
    check(_lib.lib().fira_embed_grouped_bwd(cur_stream(), item_tok.numel(), ptr(_i32(item_tok)), ptr(_i32(item_ptr)),
                                            ptr(_i32(rows)), ptr(_f32(dtable)), ptr(_f32(dnode))), "fira_embed_grouped_bwd")
    return dtable


def embed_list_bwd_small(rows, ids, dtable, dnode):
    check(_lib.lib().fira_embed_list_bwd_small(cur_stream(), rows.numel(), ptr(_i32(rows)), ptr(_i32(ids)), ptr(_f32(dtable)),
                                               ptr(_f32(dnode)), dtable.shape[0]), "fira_embed_list_bwd_small")
    return dtable


def embed_scatter_add_small(idx, dtable, dout, out_bstride, out_off, padding_idx):
    """embed_scatter_add through the LDS-table kernel (fira_embed_gather_bwd_small)."""
    B, L = idx.shape
    check(_lib.lib().fira_embed_gather_bwd_small(cur_stream(), B, L, ptr(_i32(idx)), ptr(_f32(dtable)), ptr(_f32(dout)),
                                                 out_bstride, out_off, padding_idx, dtable.shape[0]),
          "fira_embed_gather_bwd_small")
    return dtable


def adam_step(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, inv_scale=None):
    check(_lib.lib().fira_adam_step(cur_stream(), p.numel(), ptr(_f32(p)), ptr(_f32(g)), ptr(_f32(m)), ptr(_f32(v)),
                                    lr, beta1, beta2, eps, step, ptr(inv_scale)), "fira_adam_step")


def adam_step_count(p, g, m, v, lr, step, count, beta1=0.9, beta2=0.999, eps=1e-8):
    """Adam on g / max(count, 1): ``count`` is a device float (the all-reduced token count of a data-parallel step)."""
    check(_lib.lib().fira_adam_step_count(cur_stream(), p.numel(), ptr(_f32(p)), ptr(_f32(g)), ptr(_f32(m)), ptr(_f32(v)),
                                          lr, beta1, beta2, eps, step, ptr(_f32(count))), "fira_adam_step_count")


def pack_stats(loss_sum, n_tok, out2):
    """out2 = [loss_sum, float(n_tok)] on the device: what a rank contributes to the step's 2-scalar all-reduce."""
    check(_lib.lib().fira_pack_stats(cur_stream(), ptr(_f32(loss_sum)), ptr(_i32(n_tok)), ptr(_f32(out2))), "fira_pack_stats")
    return out2


ACCUM_MAX = 64


def accum_check(k):
    """Validates a number of micro-batches per optimizer step, ``1 <= K <= ACCUM_MAX`` (``None`` = 1); raises ``ValueError``."""
    if k is None:
        return 1
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= ACCUM_MAX:
        raise ValueError("accum steps %r: must be an integer in [1, %d]" % (k, ACCUM_MAX))
    return int(k)


def accum_split(lo: int, hi: int, k: int):
    """The K micro-batches of a rank's shard ``[lo, hi)`` of the global batch: K ranges of ``ceil((hi - lo) / K)`` commits in
    order.  A short shard leaves the last ones smaller or empty (``(hi, hi)``): every rank still makes K entries.  Host only."""
    k = accum_check(k)
    n = max(hi - lo, 0)
    size = -(-n // k)
    return [(min(lo + i * size, hi), min(lo + (i + 1) * size, hi)) for i in range(k)]


def accum_stats(loss_sum, n_tok, stats, n_tok_total, first: bool):
    """``stats = [loss_sum, float(n_tok)]`` summed over an optimizer step's micro-batches (fira_accum_stats; ``pack_stats``'
    layout), the exact token total in the int32 ``n_tok_total``; ``first`` starts a new sum whatever the buffers hold."""
    check(_lib.lib().fira_accum_stats(cur_stream(), ptr(_f32(loss_sum)), ptr(_i32(n_tok)), ptr(_f32(stats)),
                                      ptr(_i32(n_tok_total)), 1 if first else 0), "fira_accum_stats")
    return stats


def adam_step_mb(p, g0, g1, m, v, lr, step, n_tok0, n_tok1=None, beta1=0.9, beta2=0.999, eps=1e-8):
    """Adam on g0 (+ g1) / max(n_tok0 (+ n_tok1), 1): one launch, normaliser formed on the device."""
    check(_lib.lib().fira_adam_step_mb(cur_stream(), p.numel(), ptr(_f32(p)), ptr(_f32(g0)), ptr(g1), ptr(_f32(m)),
                                       ptr(_f32(v)), lr, beta1, beta2, eps, step, ptr(_i32(n_tok0)), ptr(n_tok1)),
          "fira_adam_step_mb")


def ema_check(decay, every):
    """Validates a per-step decay ``0 < D < 1`` and a cadence ``K >= 1`` of the weight average; raises ``ValueError``."""
    try:
        ok = 0.0 < float(decay) < 1.0                          # (also refuses nan)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("ema decay %r: must be a number in (0, 1)" % (decay,))
    if isinstance(every, bool) or not isinstance(every, int) or every < 1:
        raise ValueError("ema cadence %r: must be an integer >= 1" % (every,))
    return float(decay), int(every)


def ema_weight(decay: float, every: int = 1) -> float:
    """``w = float32(1 - D**K)``: the weight of one update of an average with per-step decay ``D`` that runs every ``K``
    steps.  Formed in double, rounded once to fp32 -- the float the update kernels are given.  Host only, no GPU."""
    import numpy as np
    decay, every = ema_check(decay, every)
    return float(np.float32(1.0 - decay ** every))


def ema_update(ema, p, w: float):
    """``ema += w * (p - ema)`` element by element (fira_ema_update): the subtraction, the multiply and the add each rounded to
    fp32 on its own, so a numpy float32 loop is the bit-exact reference.  Any length >= 1, any 4-byte alignment; ``ema`` must
    not overlap ``p``."""
    assert ema.numel() == p.numel(), "ema and p differ in length"
    check(_lib.lib().fira_ema_update(cur_stream(), ema.numel(), ptr(_f32(ema)), ptr(_f32(p)), float(w)), "fira_ema_update")
    return ema


LR_KINDS = ("constant", "inv_sqrt", "cosine", "linear")          # fira_lr_schedule.kind = the index


@dataclasses.dataclass(frozen=True)
class LrSchedule:
    """A learning-rate schedule, the mirror of ``fira_lr_schedule`` (include/fira_hip.h has the formulas; the library's
    ``fira_lr_at`` is their only implementation -- :func:`lr_at` calls it).  ``kind``: one of :data:`LR_KINDS`; ``base_lr``:
    the peak; ``warmup_steps`` W >= 0; ``decay_steps`` N > W: the step at which cosine / linear reach ``min_lr``."""
    kind: str = "constant"
    base_lr: float = 1e-4
    warmup_steps: int = 0
    decay_steps: int = 0
    min_lr: float = 0.0

    @staticmethod
    def make(obj) -> "LrSchedule":
        """From an ``LrSchedule``, or a dict with its field names (``kind`` as a name -- ``inv-sqrt`` allowed -- or its number)."""
        if isinstance(obj, LrSchedule):
            s = obj
        else:
            d = dict(obj)
            unknown = set(d) - {f.name for f in dataclasses.fields(LrSchedule)}
            if unknown:
                raise ValueError("lr_schedule: unknown field(s) %s" % sorted(unknown))
            s = LrSchedule(**d)
        kind = s.kind
        if isinstance(kind, int) and not isinstance(kind, bool) and 0 <= kind < len(LR_KINDS):
            kind = LR_KINDS[kind]
        kind = str(kind).replace("-", "_")
        if kind not in LR_KINDS:
            raise ValueError("lr_schedule: kind %r is not one of %s" % (s.kind, ", ".join(LR_KINDS)))
        s = LrSchedule(kind, float(s.base_lr), int(s.warmup_steps), int(s.decay_steps), float(s.min_lr))
        lr_schedule_check(s)
        return s

    def struct(self) -> "_lib.LrSchedule":
        return _lib.LrSchedule(LR_KINDS.index(self.kind), self.base_lr, self.warmup_steps, self.decay_steps, self.min_lr)

    def as_dict(self) -> dict:
        return dataclasses.asdict(self)


def _sched_struct(sched):
    return sched if isinstance(sched, _lib.LrSchedule) else sched.struct()


def lr_at(sched, step: int) -> float:
    """The rate of step ``step`` (counting from 1) under ``sched`` (an :class:`LrSchedule` or an ``_lib.LrSchedule``):
    ``fira_lr_at``, the float every update kernel of that step is given.  Host only, no GPU."""
    import ctypes as C
    return float(_lib.lib().fira_lr_at(C.byref(_sched_struct(sched)), int(step)))


def lr_schedule_check(sched):
    """Raises ``ValueError`` with the library's message when ``sched`` is not a valid schedule (``fira_lr_schedule_check``)."""
    import ctypes as C
    lib = _lib.lib()
    if lib.fira_lr_schedule_check(C.byref(_sched_struct(sched))) != 0:
        raise ValueError(lib.fira_last_error().decode())


def clip_state(device="cuda"):
    """A zeroed fira_clip_state on the device (16 int32 = 64 bytes) and the scratch fira_grad_sqsum sums through."""
    state = torch.zeros(16, dtype=torch.int32, device=device)
    scratch = torch.zeros(_lib.lib().fira_grad_sqsum_scratch_bytes() // 8, dtype=torch.float64, device=device)
    return state, scratch


def read_clip_state(state):
    """The fields of a device fira_clip_state as a dict (synchronises)."""
    st = _lib.ClipState.from_buffer_copy(state.cpu().numpy().tobytes())
    return {"sq": list(st.sq), "norm": st.norm, "coef": st.coef, "zero_flag": st.zero_flag, "n_clipped": st.n_clipped,
            "n_nonfinite": st.n_nonfinite}


def grad_sqsum_depth(n: int) -> int:
    """D of fira_grad_sqsum for a range of n floats: the fp32 roundings one value can pass through (csrc/gradnorm.hip); the
    result is within (D + 1) * 2^-24 relative of the exact sum of squares."""
    n4 = n // 4
    slice4 = -(-(-(-n4 // 1024)) // 1024) * 1024
    return slice4 // 1024 + 12


def grad_sqsum(g, state, slot, scratch):
    """state.sq[slot] = sum of g^2 over the contiguous fp32 tensor g (fira_grad_sqsum)."""
    assert g.dtype == torch.float32 and g.is_contiguous()
    check(_lib.lib().fira_grad_sqsum(cur_stream(), g.numel(), ptr(g), ptr(state), slot, ptr(scratch)), "fira_grad_sqsum")


def clip_finish(state, n_slots, max_norm, n_tok=None, count=None):
    """norm / coef / zero_flag / counters from state.sq[0 .. n_slots) (fira_clip_finish); normaliser from n_tok or count."""
    check(_lib.lib().fira_clip_finish(cur_stream(), ptr(state), n_slots, ptr(n_tok), ptr(count), max_norm), "fira_clip_finish")


def adam_step_clip(p, g, m, v, lr, step, state, n_tok=None, count=None, beta1=0.9, beta2=0.999, eps=1e-8):
    """adam_step_mb (n_tok) / adam_step_count (count) on g * inv * coef of the clip state, or on zeros under its zero flag."""
    check(_lib.lib().fira_adam_step_clip(cur_stream(), p.numel(), ptr(_f32(p)), ptr(_f32(g)), ptr(_f32(m)), ptr(_f32(v)), lr,
                                         beta1, beta2, eps, step, ptr(n_tok), ptr(count), ptr(state)), "fira_adam_step_clip")


def inv_count(n_tok, out):
    check(_lib.lib().fira_inv_count(cur_stream(), ptr(_i32(n_tok)), ptr(_f32(out))), "fira_inv_count")
    return out


def f32_to_bf16(src, dst):
    """dst (torch.bfloat16, same numel) = bf16(src) on the current stream: the gradient wire format (fira_f32_to_bf16)."""
    n = src.numel()
    assert dst.numel() == n and dst.dtype == torch.bfloat16 and src.dtype == torch.float32 and n % 4 == 0
    check(_lib.lib().fira_f32_to_bf16(cur_stream(), n, ptr(src), ptr(dst)), "fira_f32_to_bf16")
    return dst


def bf16_to_f32(src, dst):
    n = src.numel()
    assert dst.numel() == n and src.dtype == torch.bfloat16 and dst.dtype == torch.float32 and n % 4 == 0
    check(_lib.lib().fira_bf16_to_f32(cur_stream(), n, ptr(src), ptr(dst)), "fira_bf16_to_f32")
    return dst


def ffn_fwd(x, w1, b1, w2, b2, gamma, beta, dropout=0.0, seed=0, site=0, dtype=0):
    """fira_ffn_fwd: (h, sum, y, stats) of the FeedForward block LN(dropout(relu(x W1^T + b1) W2^T + b2) + x)."""
    M, F = x.shape[0], w1.shape[0]
    h = torch.empty((M, F), dtype=torch.float32, device=x.device)
    summ, y = torch.empty_like(x), torch.empty_like(x)
    stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
    check(_lib.lib().fira_ffn_fwd(cur_stream(), M, F, ptr(_f32(x)), ptr(_f32(w1)), ptr(_f32(b1)), ptr(_f32(w2)), ptr(_f32(b2)),
                                  ptr(_f32(gamma)), ptr(_f32(beta)), ptr(h), ptr(summ), ptr(y), ptr(stats), dropout, seed, site,
                                  dtype), "fira_ffn_fwd")
    return h, summ, y, stats


def ffn_bwd(dy, x, h, summ, stats, w1, w2, gamma, dropout=0.0, seed=0, site=0, dtype=0):
    """fira_ffn_bwd: (dx, dw1, db1, dw2, db2, dgamma, dbeta) -- the parameter gradients start from zero here."""
    M, F = x.shape[0], w1.shape[0]
    dev = x.device
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    dx, dyf, dh = torch.empty_like(x), torch.empty_like(x), torch.empty((M, F), dtype=torch.float32, device=dev)
    dw1, db1, dw2, db2, dg, db = z(F, 256), z(F), z(256, F), z(256), z(256), z(256)
    check(_lib.lib().fira_ffn_bwd(cur_stream(), M, F, ptr(_f32(dy)), ptr(_f32(x)), ptr(_f32(h)), ptr(_f32(summ)), ptr(_f32(stats)),
                                  ptr(_f32(w1)), ptr(_f32(w2)), ptr(_f32(gamma)), ptr(dx), ptr(dyf), ptr(dh), ptr(dw1), ptr(db1),
                                  ptr(dw2), ptr(db2), ptr(dg), ptr(db), dropout, seed, site, dtype), "fira_ffn_bwd")
    return dx, dw1, db1, dw2, db2, dg, db


def head_topk(x, wout, bout, k, dtype=0):
    """fira_head_topk: (ids [R,k] int32, vals [R,k], logits [R,V]) of the generator head x Wout^T + bout."""
    R, V = x.shape[0], wout.shape[0]
    ldl = (V + 63) // 64 * 64
    logits = torch.empty((R, ldl), dtype=torch.float32, device=x.device)
    ids = torch.empty((R, k), dtype=torch.int32, device=x.device)
    vals = torch.empty((R, k), dtype=torch.float32, device=x.device)
    check(_lib.lib().fira_head_topk(cur_stream(), R, V, k, ptr(_f32(x)), ptr(_f32(wout)), ptr(_f32(bout)), ptr(logits), ldl,
                                    ptr(ids), ptr(vals), dtype), "fira_head_topk")
    return ids, vals, logits[:, :V]


def head_logits_x3(x, wout, bout):
    """fira_head_logits_x3: logits [R, V] = x Wout^T + bout on the bf16 matrix cores at fp32 accuracy (three bf16 terms)."""
    R, V = x.shape[0], wout.shape[0]
    ldl = (V + 63) // 64 * 64
    logits = torch.empty((R, ldl), dtype=torch.float32, device=x.device)
    scratch = torch.empty(_lib.lib().fira_head_logits_x3_scratch_bytes(R), dtype=torch.uint8, device=x.device)
    x = _f32(x)
    check(_lib.lib().fira_head_logits_x3(cur_stream(), R, V, ptr(x), x.stride(0), ptr(_f32(wout)), ptr(_f32(bout)), ptr(logits), ldl,
                                         ptr(scratch)), "fira_head_logits_x3")
    return logits[:, :V]


_panel_scratch = {}


def gemm_wgrad_panel(A, B, out, colsum=None, dtype=0, split=True):
    """fira_gemm_wgrad_panel: out[M,N] += A^T B (A [K, >=M], B [K, N] row-major, row pitches = their strides), optional
    colsum[M] += column sums of A.  dtype 0: fp32-accurate three-term bf16 split, 1: bf16-rounded operands.  ``split``: hand
    the library a 64 MB scratch buffer so that it may cut K into slabs over the chip."""
    K, M, N = A.shape[0], out.shape[0], out.shape[1]
    assert B.shape[0] == K and B.shape[1] == N and A.stride(1) == 1 and B.stride(1) == 1 and out.stride(1) == 1
    scratch = None
    if split:
        scratch = _panel_scratch.get(A.device)
        if scratch is None:
            scratch = _panel_scratch[A.device] = torch.empty(256 * 65536, dtype=torch.float32, device=A.device)
    check(_lib.lib().fira_gemm_wgrad_panel(cur_stream(), dtype, M, N, K, ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(out),
                                           out.stride(0), ptr(colsum), ptr(scratch), scratch.numel() if split else 0),
          "fira_gemm_wgrad_panel")
    return out


def dev_bleu_stats(ids, sou, sub_token, tar, V, hyp=None, stats=None):
    """fira_dev_bleu_stats: per commit the sentence-BLEU statistics of ``Run.dev`` on token ids.  ids [B,T] are output indices
    of ``forward_dev``, sou [B,L], sub_token [B,S], tar [B,T], all int32.  Returns (hyp [B,T]: the hypothesis' vocabulary ids,
    compacted, -1 behind its length; stats [B,12]: num[4], cnt[4], hyp_len, ref_len, 0, 0) -- into ``hyp`` / ``stats`` when
    given (slices of a pass-wide buffer).  ``metrics.bleu_method2_from_stats`` turns a stats row into the score."""
    B, T = ids.shape
    L, S = sou.shape[1], sub_token.shape[1]
    assert sou.shape[0] == B and sub_token.shape[0] == B and tuple(tar.shape) == (B, T)
    if hyp is None:
        hyp = torch.empty((B, T), dtype=torch.int32, device=ids.device)
    if stats is None:
        stats = torch.empty((B, 12), dtype=torch.int32, device=ids.device)
    assert tuple(hyp.shape) == (B, T) and tuple(stats.shape) == (B, 12)
    check(_lib.lib().fira_dev_bleu_stats(cur_stream(), B, T, int(V), L, S, ptr(_i32(ids)), ptr(_i32(sou)), ptr(_i32(sub_token)),
                                         ptr(_i32(tar)), ptr(_i32(hyp)), ptr(_i32(stats))), "fira_dev_bleu_stats")
    return hyp, stats


def mbr_bleu_stats(tokens, length, stats=None):
    """fira_mbr_bleu_stats: the sentence-BLEU statistics of every ordered pair of a commit's candidate messages.  tokens
    [B,n,T] vocabulary ids, length [B,n], int32 (n <= 32, T <= 64); the message of a candidate is its ids at positions
    1 .. length - 1 without <pad> / <eos> / <start>.  Returns stats [B,n,n,12] int32 -- row [b,i,j]: num[4], cnt[4], hyp_len,
    ref_len, 0, 0 with candidate i as the hypothesis and j as the reference -- into ``stats`` when given.
    ``metrics.mbr_utilities`` turns it into expected-BLEU utilities."""
    B, n, T = tokens.shape
    assert tuple(length.shape) == (B, n)
    if stats is None:
        stats = torch.empty((B, n, n, 12), dtype=torch.int32, device=tokens.device)
    assert tuple(stats.shape) == (B, n, n, 12)
    check(_lib.lib().fira_mbr_bleu_stats(cur_stream(), B, n, T, ptr(_i32(tokens)), ptr(_i32(length)), ptr(_i32(stats))),
          "fira_mbr_bleu_stats")
    return stats


def dev_rouge_l_stats(ids, sou, sub_token, tar, V, stats=None):
    """fira_dev_rouge_l_stats: per commit the ROUGE-L statistics of the dev pass on token ids; hypothesis and reference are
    ``dev_bleu_stats``'s.  ids [B,T], sou [B,L], sub_token [B,S], tar [B,T], all int32.  Returns stats [B,4] int32: lcs (length
    of the longest common subsequence), hyp_len, ref_len, 0 -- into ``stats`` when given.  ``metrics.rouge_l_from_stats`` turns
    a row into the score."""
    B, T = ids.shape
    L, S = sou.shape[1], sub_token.shape[1]
    assert sou.shape[0] == B and sub_token.shape[0] == B and tuple(tar.shape) == (B, T)
    if stats is None:
        stats = torch.empty((B, 4), dtype=torch.int32, device=ids.device)
    assert tuple(stats.shape) == (B, 4)
    check(_lib.lib().fira_dev_rouge_l_stats(cur_stream(), B, T, int(V), L, S, ptr(_i32(ids)), ptr(_i32(sou)), ptr(_i32(sub_token)),
                                            ptr(_i32(tar)), ptr(_i32(stats))), "fira_dev_rouge_l_stats")
    return stats


def mbr_rouge_l_stats(tokens, length, stats=None):
    """fira_mbr_rouge_l_stats: the ROUGE-L statistics of every ordered pair of a commit's candidate messages (the messages are
    ``mbr_bleu_stats``'s).  tokens [B,n,T] vocabulary ids, length [B,n], int32 (n <= 32, T <= 64).  Returns stats [B,n,n,4]
    int32 -- row [b,i,j]: lcs, hyp_len, ref_len, 0 with candidate i as the hypothesis and j as the reference -- into ``stats``
    when given.  ``metrics.mbr_utilities(stats, "rouge_l")`` turns it into expected-ROUGE-L utilities."""
    B, n, T = tokens.shape
    assert tuple(length.shape) == (B, n)
    if stats is None:
        stats = torch.empty((B, n, n, 4), dtype=torch.int32, device=tokens.device)
    assert tuple(stats.shape) == (B, n, n, 4)
    check(_lib.lib().fira_mbr_rouge_l_stats(cur_stream(), B, n, T, ptr(_i32(tokens)), ptr(_i32(length)), ptr(_i32(stats))),
          "fira_mbr_rouge_l_stats")
    return stats


def dev_meteor_stats(ids, sou, sub_token, tar, V, classes=None, stats=None):
    """fira_dev_meteor_stats: per commit the METEOR alignment statistics of the dev pass on token ids; hypothesis and reference
    are ``dev_bleu_stats``'s.  ids [B,T], sou [B,L], sub_token [B,S], tar [B,T], all int32; ``classes`` int32 [V] or None (exact
    matches only).  Returns stats [B,4] int32: m (matched pairs), chunks, hyp_len, ref_len -- into ``stats`` when given.
    ``metrics.meteor_exact_from_stats`` turns a row into the score."""
    B, T = ids.shape
    L, S = sou.shape[1], sub_token.shape[1]
    assert sou.shape[0] == B and sub_token.shape[0] == B and tuple(tar.shape) == (B, T)
    assert classes is None or tuple(classes.shape) == (int(V),)
    if stats is None:
        stats = torch.empty((B, 4), dtype=torch.int32, device=ids.device)
    assert tuple(stats.shape) == (B, 4)
    check(_lib.lib().fira_dev_meteor_stats(cur_stream(), B, T, int(V), L, S, ptr(_i32(ids)), ptr(_i32(sou)), ptr(_i32(sub_token)),
                                           ptr(_i32(tar)), None if classes is None else ptr(_i32(classes)), ptr(_i32(stats))),
          "fira_dev_meteor_stats")
    return stats


def mbr_meteor_stats(tokens, length, classes=None, stats=None):
    """fira_mbr_meteor_stats: the METEOR alignment statistics of every ordered pair of a commit's candidate messages (the
    messages are ``mbr_bleu_stats``'s).  tokens [B,n,T] vocabulary ids, length [B,n], int32 (n <= 32, T <= 64); ``classes``
    int32 [V] or None (exact matches only).  Returns stats [B,n,n,4] int32 -- row [b,i,j]: m, chunks, hyp_len, ref_len with
    candidate i as the hypothesis and j as the reference -- into ``stats`` when given.
    ``metrics.mbr_utilities(stats, "meteor_exact")`` turns it into expected-METEOR utilities."""
    B, n, T = tokens.shape
    assert tuple(length.shape) == (B, n)
    assert classes is None or classes.dim() == 1
    if stats is None:
        stats = torch.empty((B, n, n, 4), dtype=torch.int32, device=tokens.device)
    assert tuple(stats.shape) == (B, n, n, 4)
    check(_lib.lib().fira_mbr_meteor_stats(cur_stream(), B, n, T, ptr(_i32(tokens)), ptr(_i32(length)),
                                           0 if classes is None else classes.shape[0],
                                           None if classes is None else ptr(_i32(classes)), ptr(_i32(stats))),
          "fira_mbr_meteor_stats")
    return stats


def pool_memory(dims, mem, mem_valid, out=None):
    """fira_pool_memory: the unit vector of every commit -- the mean of its valid encoder-memory rows, L2-normalised.  mem
    [B, sou_len + sub_len, 256] fp32 and mem_valid [B, sou_len + sub_len] int32 (a decode workspace's views).  Returns out
    [B, 256]."""
    B = mem.shape[0]
    assert mem.dim() == 3 and tuple(mem_valid.shape) == tuple(mem.shape[:2]) and mem.shape[2] == 256
    assert mem.shape[1] == dims.sou_len + dims.sub_len
    if out is None:
        out = torch.empty((B, 256), dtype=torch.float32, device=mem.device)
    assert tuple(out.shape) == (B, 256)
    import ctypes as C
    check(_lib.lib().fira_pool_memory(cur_stream(), C.byref(dims), B, ptr(_f32(mem)), ptr(_i32(mem_valid)), ptr(_f32(out))),
          "fira_pool_memory")
    return out


def nn_search(Q, store, exclude=None, scratch=None):
    """fira_nn_search: per query row of Q [B <= 64, 256] the store row (store [N, 256]) with the largest dot product, not
    counting row exclude[b] (int32 [B], -1 = none).  Returns (best_idx [B] int32, best_sim [B] fp32 clamped to [0, 1]); ties
    go to the lowest index, NaN never wins."""
    B, N = Q.shape[0], store.shape[0]
    assert Q.dim() == 2 and store.dim() == 2 and Q.shape[1] == 256 and store.shape[1] == 256
    assert exclude is None or tuple(exclude.shape) == (B,)
    lib = _lib.lib()
    need = lib.fira_nn_search_scratch_bytes(B, N)
    if scratch is None:
        scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=Q.device)
    idx = torch.empty(B, dtype=torch.int32, device=Q.device)
    sim = torch.empty(B, dtype=torch.float32, device=Q.device)
    check(lib.fira_nn_search(cur_stream(), ptr(_f32(Q)), B, ptr(_f32(store)), N, None if exclude is None else ptr(_i32(exclude)),
                             ptr(idx), ptr(sim), ptr(scratch), scratch.numel()), "fira_nn_search")
    return idx, sim


def mix_neighbour(dims, rows_per_commit, coef, q, dist, best=False):
    """fira_mix_neighbour: dist [R, W] <- a * dist (+ c * q below the vocabulary), (a, c) = coef[r // rows_per_commit], in place.
    ``best``: also return (best_id [R] int32, best_p [R]) of the rows as stored."""
    R = dist.shape[0]
    assert tuple(q.shape) == tuple(dist.shape) and coef.numel() == 2 * (R // max(rows_per_commit, 1))
    import ctypes as C
    bid = torch.empty(R, dtype=torch.int32, device=dist.device) if best else None
    bp = torch.empty(R, dtype=torch.float32, device=dist.device) if best else None
    check(_lib.lib().fira_mix_neighbour(cur_stream(), C.byref(dims), R, rows_per_commit, ptr(_f32(coef)), ptr(q), ptr(dist),
                                        ptr(bid), ptr(bp)), "fira_mix_neighbour")
    return (bid, bp) if best else dist
