"""Fixtures and plain torch statements for tests/test_tail_gpu.py and tests/test_host_items.py: the copy head, the loss and the
row scatters of the training step's tail, written once with the dtype as a parameter.  In float64 they are the references
of the GPU tests; the same statements in float32 give the fp32-vs-fp64 figures behind the worst-row bounds
(``python tests/tail_ref.py`` prints them and checks the clamp-margin condition of the loss fixtures; no GPU needed).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

D = 256


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def worst_row(a, ref):
    """max over rows of |row - ref| / max(|ref row|, floor), rows = the last dimension; floor = the median norm of the
    reference's non-zero rows (its typical row), so that rows that are (nearly) zero do not dominate."""
    a, ref = a.double().reshape(-1, a.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    rn = ref.norm(dim=1)
    floor = float(rn[rn > 0].median()) if bool((rn > 0).any()) else 1.0
    return float(((a - ref).norm(dim=1) / rn.clamp_min(floor)).max())


# ------------------------------------------------------------------------------------------------ copy score
def copy_inputs(Bm, R, S, seed):
    """src [Bm, S, 256] memory rows, tgt [R, 256] target rows, w [256], bias [1] (fp32, CPU)."""
    return (randn(Bm, S, D, seed=seed), randn(R, D, seed=seed + 1), randn(D, seed=seed + 2, scale=0.1),
            randn(1, seed=seed + 3))


def copy_valid(Bm, S, seed, tile=16):
    """Key mask [Bm, S] (int32): ~60 % valid at random; in every commit the second tile of 16 slots is fully masked and the
    third fully valid (whole forward chunks of 8 and backward tiles of 16 without / with every slot)."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand(Bm, S, generator=g) > 0.4).to(torch.int32)
    if S > 3 * tile:
        v[:, tile:2 * tile] = 0
        v[:, 2 * tile:3 * tile] = 1
    v[:, 0] = 1
    return v


def copy_score(src, tgt, w, bias, row_b, dtype):
    """score[r, j] = w . tanh(src[row_b[r], j] + tgt[r]) + bias  (Model.py:15-18) for target row r of commit row_b[r]."""
    src, tgt, w, bias = (x.to(dtype) for x in (src, tgt, w, bias))
    return (torch.tanh(src[row_b] + tgt[:, None, :]) * w).sum(-1) + bias


def copy_backward(src, tgt, w, bias, row_b, valid, dscore, dtype):
    """Gradients of sum(masked_fill(score, valid == 0, -1e9) * dscore): (dsrc, dtgt, dw, dbias)."""
    src, tgt, w, bias = (x.detach().to(dtype).requires_grad_(True) for x in (src, tgt, w, bias))
    sc = (torch.tanh(src[row_b] + tgt[:, None, :]) * w).sum(-1) + bias
    if valid is not None:
        sc = sc.masked_fill(valid[row_b] == 0, -1e9)
    sc.backward(dscore.to(dtype))
    return src.grad, tgt.grad, w.grad, bias.grad


# ------------------------------------------------------------------------------------------------ head + loss
def head_loss(logits, score, gate, valid_rows, label, dtype):
    """Model.py:54-82 on R rows: logits [R, V], score [R, S], gate [R, 2], valid_rows [R, S] the key mask of each row's
    commit, label [R] the shifted label (0 = ignore).  Returns loss_sum, n_tok, the three gradients, the probability of
    every row's label and the arg-max id of every row."""
    logits, score, gate = (x.detach().to(dtype).requires_grad_(True) for x in (logits, score, gate))
    V = logits.shape[1]
    p_gen = torch.softmax(logits, -1)
    p_copy = torch.softmax(score.masked_fill(valid_rows == 0, -1e9), -1)
    gt = torch.softmax(gate, -1)
    p = torch.cat([gt[:, :1] * p_gen, gt[:, 1:] * p_copy], -1)
    logp = torch.log(p.clamp(min=1e-10, max=1))
    nll = F.nll_loss(logp, label, reduction="none").masked_fill(label == 0, 0)
    nll.sum().backward()
    p_label = p.detach().gather(1, label[:, None])[:, 0]
    return (nll.sum().detach(), int((label != 0).sum()), logits.grad, score.grad, gate.grad, p_label,
            p.detach().argmax(-1))


def clamp_margin_ok(p_label, label):
    """The fixtures' condition: no live label has a reference probability within a factor 100 of the 1e-10 clamp."""
    p = p_label[label != 0].double()
    return not bool(((p > 1e-12) & (p < 1e-8)).any())


def ragged_rows(lens, T):
    """t_off [B+1], row_bt [R] (flat b*T + t of every computed row) and row_b [R] for per-commit prefix lengths."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    row_bt = np.concatenate([b * T + np.arange(n) for b, n in enumerate(lens)]).astype(np.int32)
    return torch.from_numpy(off), torch.from_numpy(row_bt), torch.from_numpy(row_bt // T).long()


def loss_fixture(V, S, T, seed, lens=None, B=4):
    """Inputs of one loss case on the computed rows of B commits (every row when lens is None).  Planted rows:
      commit 0   labels up to the last position (row T-2 carries tar_label[0, T-1], row T-1 the implicit 0), a label 0 in
                 mid-sequence, a copy label at position T-2 (the last the forward's guard admits), the generator label V-1
      commit 1   generator labels only (no copy label: the forward's mask == 0 exit), among them
                   a label 40 below its row's maximum (p < 1e-10: clamped, zero gradient)
                   a label 17 below a dominant maximum (the train kernel's one-exponential term far from the maximum; 20
                   below would put p = 2e-9 inside the clamp margin)
      commit 2   a copy label on a masked slot (p = 0), copy labels with the gate saturated both ways (logits +-60): on
                 the vanished branch (p underflows: clamped) and on the live one; a generator label on the vanished branch
      commit 3   copy and generator labels at random
    """
    g = torch.Generator().manual_seed(seed)
    lens = [T] * B if lens is None else list(lens)
    t_off, row_bt, row_b = ragged_rows(lens, T)
    R = int(t_off[-1])
    valid = copy_valid(B, S, seed + 5)
    lab = torch.zeros(B, T, dtype=torch.int64)
    lab[:, 0] = 2
    vslots = [valid[b].nonzero().view(-1) for b in range(B)]
    mslots = [(valid[b] == 0).nonzero().view(-1) for b in range(B)]
    pick = lambda s: int(s[int(torch.randint(0, len(s), (1,), generator=g))])
    n0 = lens[0]
    lab[0, 1:n0] = torch.randint(4, V, (n0 - 1,), generator=g)
    lab[0, 5] = 0
    lab[0, 3] = V + pick(vslots[0])
    lab[0, 7] = V - 1
    if n0 >= T - 1:
        lab[0, T - 1] = V + pick(vslots[0])
    n1 = min(lens[1], 10)
    lab[1, 1:n1 + 1] = torch.randint(4, V, (n1,), generator=g)
    n2 = min(lens[2], 12)
    lab[2, 1:n2 + 1] = torch.randint(4, V, (n2,), generator=g)
    lab[2, 2] = V + pick(mslots[2])
    lab[2, 3] = V + pick(vslots[2])
    lab[2, 4] = V + pick(vslots[2])
    n3 = lens[3]
    lab[3, 1:n3] = torch.randint(4, V, (n3 - 1,), generator=g)
    for t in range(2, n3, 3):
        lab[3, t] = V + pick(vslots[3])
    label = torch.cat([lab[:, 1:], torch.zeros_like(lab[:, :1])], 1).view(-1)[row_bt.long()]
    logits = randn(R, V, seed=seed + 1, scale=2.0)
    score = randn(R, S, seed=seed + 2, scale=2.0)
    gate = randn(R, 2, seed=seed + 3)
    row = lambda b, t: int(t_off[b]) + t                    # computed row of (b, t): its label is lab[b, t + 1]
    r = row(1, 1)
    logits[r, int(lab[1, 2])] = float(logits[r].max()) - 40.0
    r = row(1, 3)
    y = int(lab[1, 4])
    logits[r, (y + 501) % V] = 30.0
    logits[r, y] = 13.0
    gate[r] = torch.tensor([3.0, 0.0])
    gate[row(2, 2)] = torch.tensor([60.0, -60.0])            # copy label, gate on the generator
    gate[row(2, 3)] = torch.tensor([-60.0, 60.0])            # copy label, gate on the copy branch
    gate[row(2, 4)] = torch.tensor([-60.0, 60.0])            # generator label, gate on the copy branch
    return dict(B=B, T=T, V=V, S=S, R=R, lens=lens, t_off=t_off, row_bt=row_bt, row_b=row_b, valid=valid,
                tar_label=lab.to(torch.int32), label=label, logits=logits, score=score, gate=gate,
                clamped_rows=[row(1, 1), row(2, 1), row(2, 2), row(2, 4)])


# (V, S, prefix lengths of the computed rows or None = all 30); the seed was chosen on the CPU so that clamp_margin_ok holds on
# the float64 reference of every case, with and without plant_argmax_ties (seed 3 puts a random generator label of the
# V = 24650 case at p = 5e-9)
RAGGED = [30, 12, 17, 29]
LOSS_CASES = [(1000, 37, None), (1000, 370, RAGGED), (1001, 37, RAGGED), (1001, 370, None), (24650, 37, RAGGED)]
LOSS_SEED = 4


def plant_argmax_ties(fx):
    """The row maximum duplicated (exactly) at indices owned by different threads and waves of both loss kernels (register
    path: thread (i / 2) % 256; streaming path: i % 256), listed with the FIRST occurrence last; and two copy-score ties.
    Rows 0..5 of commit 3."""
    lg, sc, gt, S = fx["logits"], fx["score"], fx["gate"], fx["S"]
    base = int(fx["t_off"][3])
    fx["tar_label"][3, 1:7] = 0                 # the re-gated rows carry no label (the clamp-margin condition stays true)
    fx["label"][base:base + 6] = 0
    for k, idx in enumerate([(600, 901, 5), (522, 10), (901, 600), (131, 130)]):
        r = base + k
        lg[r, list(idx)] = float(lg[r].max()) + 1.0
        gt[r] = torch.tensor([4.0, -4.0])
    for k, idx in enumerate([(S - 1, 3), (S // 2 + 1, S // 2)]):
        r = base + 4 + k
        fx["valid"][3, list(idx)] = 1
        sc[r, list(idx)] = float(sc[r].max()) + 1.0
        gt[r] = torch.tensor([-6.0, 6.0])
    return fx


# ------------------------------------------------------------------------------------------------ embedding items
GROUP_COUNTS = {1: 33, 2: 1, 3: 31, 4: 32, 5: 64, 6: 65, 7: 1000, 150: 40, 299: 65}
GROUP_TABLE_ROWS = 300


def grouped_ids_batch(cfg, seed=0, B=4):
    """A HostBatch whose code / sub-token ids hold words occurring 1, 31, 32, 33, 64, 65 and 1000 times, placed at random
    (the rest is padding, id 0).  The smallest id (1) and the largest (299) both need more than one item of 32 rows, so
    the first and the last item of the list are shared with a neighbour."""
    from fira_icse_amd import data
    L, S, N = cfg.sou_len, cfg.sub_token_len, cfg.graph_len
    ids = np.zeros(B * (L + S), dtype=np.int64)
    flat = np.concatenate([np.full(n, w, dtype=np.int64) for w, n in GROUP_COUNTS.items()])
    assert flat.size <= ids.size
    ids[:flat.size] = flat
    ids = np.random.RandomState(seed).permutation(ids).reshape(B, L + S)
    z = lambda n: np.zeros((B, n), dtype=np.int64)
    return data.HostBatch(np.ascontiguousarray(ids[:, :L]), z(cfg.tar_len), z(L), z(N - L - S), z(cfg.tar_len),
                          np.ascontiguousarray(ids[:, L:]), np.arange(B * N + 1, dtype=np.int32),
                          np.arange(B * N, dtype=np.int32), np.ones(B * N, dtype=np.float32))


def scatter_add(table0, ids, rows, dtype):
    """table0 + index_add_ of `rows` at `ids` (ids == 0, the padding index, excluded)."""
    keep = ids != 0
    return table0.to(dtype).clone().index_add_(0, ids[keep].long(), rows.to(dtype)[keep])


# ------------------------------------------------------------------------------------------------ measurement
def copy_bwd_case(S, T, seed=20):
    """Backward fixture: commits with 8, 9, 16, 17 and min(30, T) target rows carrying gradient in the same slot tiles
    (the chunk loop of 8 active rows), and a commit whose single active row is non-zero in one tile of 16 slots only.
    dscore holds 1e30 on every masked slot."""
    counts = [8, 9, 16, 17, min(30, T), 1]
    B = len(counts)
    src, tgt, w, bias = copy_inputs(B, B * T, S, seed)
    valid = copy_valid(B, S, seed + 7)
    ds = torch.zeros(B, T, S)
    g = torch.Generator().manual_seed(seed + 9)
    for b, n in enumerate(counts):
        rows = torch.randperm(T, generator=g)[:n]
        ds[b, rows] = torch.randn(n, S, generator=g)
    one = int(ds[5].abs().sum(-1).nonzero()[0])
    keep = ds[5, one, 32:48].clone() if S > 48 else ds[5, one, 16:32].clone()
    ds[5, one] = 0
    if S > 48:
        ds[5, one, 32:48] = keep                                 # (the fully valid tile of copy_valid)
    else:
        ds[5, one, 16:32] = keep
        valid[5, 16:32] = 1
    ds = torch.where(valid[:, None, :] == 0, torch.full_like(ds, 1e30), ds)
    row_b = torch.arange(B).repeat_interleave(T)
    return dict(B=B, T=T, S=S, src=src, tgt=tgt, w=w, bias=bias, valid=valid, dscore=ds.view(B * T, S), row_b=row_b)


def measure():
    """fp32 torch against fp64 torch, same statements, same inputs: the figures the worst-row bounds are 4 x of."""
    out = {}

    def put(name, a, ref):
        out[name] = max(out.get(name, 0.0), worst_row(a, ref))

    for S in (37, 370):
        for T in (30, 32, 1):
            src, tgt, w, bias = copy_inputs(3, 3 * T, S, 11)
            row_b = torch.arange(3).repeat_interleave(T)
            put("score", copy_score(src, tgt, w, bias, row_b, torch.float32), copy_score(src, tgt, w, bias, row_b, torch.float64))
        for T in (30, 32):
            c = copy_bwd_case(S, T)
            a = copy_backward(c["src"], c["tgt"], c["w"], c["bias"], c["row_b"], c["valid"], c["dscore"], torch.float32)
            r = copy_backward(c["src"], c["tgt"], c["w"], c["bias"], c["row_b"], c["valid"], c["dscore"], torch.float64)
            put("dsrc", a[0], r[0])
            put("dtgt", a[1], r[1])
    for V, S, lens in LOSS_CASES:
        fx = loss_fixture(V, S, 30, LOSS_SEED, lens)
        vr = fx["valid"][fx["row_b"]]
        a = head_loss(fx["logits"], fx["score"], fx["gate"], vr, fx["label"], torch.float32)
        r = head_loss(fx["logits"], fx["score"], fx["gate"], vr, fx["label"], torch.float64)
        assert clamp_margin_ok(r[5], fx["label"]), (V, S)
        tie = plant_argmax_ties(loss_fixture(V, S, 30, LOSS_SEED, lens))
        assert clamp_margin_ok(head_loss(tie["logits"], tie["score"], tie["gate"], tie["valid"][tie["row_b"]], tie["label"],
                                         torch.float64)[5], tie["label"]), ("ties", V, S)
        put("dlogits", a[2], r[2])
        put("dscore", a[3], r[3])
        put("dgate", a[4], r[4])
        out["loss"] = max(out.get("loss", 0.0), abs(float(a[0]) - float(r[0])) / float(r[0]))
    for S, lens in ((37, None), (37, RAGGED), (370, None), (370, RAGGED)):     # copy score -> loss, as the forward composes them
        fx = loss_fixture(1000, S, 30, LOSS_SEED, lens)
        src, tgt, w, bias = copy_inputs(fx["B"], fx["R"], S, 17)
        vr, res = fx["valid"][fx["row_b"]], []
        for dt in (torch.float32, torch.float64):
            res.append(head_loss(fx["logits"], copy_score(src, tgt, w, bias, fx["row_b"], dt), fx["gate"], vr, fx["label"], dt))
        assert clamp_margin_ok(res[1][5], fx["label"]), ("composed", S)
        put("dscore_composed", res[0][3], res[1][3])
    g = torch.Generator().manual_seed(5)
    for n, hot in ((1021, True), (1021, False), (3000, False)):
        ids = torch.randint(1, 71, (n,), generator=g)
        if hot:
            ids[torch.rand(n, generator=g) < 0.98] = 7
        rows, t0 = randn(n, D, seed=n), randn(71, D, seed=n + 1)
        put("scatter", scatter_add(t0, ids, rows, torch.float32), scatter_add(t0, ids, rows, torch.float64))
    return out


if __name__ == "__main__":
    for k, v in measure().items():
        print("%-8s fp32 vs fp64 worst row %.3e   bound (4 x) %.3e" % (k, v, 4 * v))
