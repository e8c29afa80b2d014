"""The aggregation A_hat X on adversarial CSR rows, row by row, through every kernel that computes it.

Each kernel cuts a row at its own places: the 16-entry head and 64-entry chunks of the row-batch and fused-GCN gathers, the
64-entry staging passes of the LDS kernel, the three 64-entry slots and the tail loop of densify_rows (spmm_dense.hip).
The graphs below put runs of equal columns, row lengths and graph sizes on those cuts.  Every check is per row:
||Y_r - ref_r|| / ||(|A| |X|)_r||, where |A| adds up the MAGNITUDES of a row's entries, so a run that cancels (v, -v) is
still measured against its entries.  Rows without a non-zero entry must come out exactly zero.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 256
SPMM_LDS_AT, SPMM_DENSE_AT_F32, SPMM_DENSE_AT_BF16 = 0.02, 0.27, 0.025   # spmm.hip: the documented auto thresholds


# ------------------------------------------------------------------------------------------------ builder
class Case:
    """B graphs of N rows: host CSR (global column ids g*N + c), the fp64 dense [B,N,N] with equal neighbours summed, |A|,
    and the bf16 tile densify_rows must build: each run summed in fp32 from its last entry back to its first, then rounded."""

    def __init__(self, name, N, graphs):
        self.name, self.N, self.B = name, N, len(graphs)
        rowptr, col, val = [0], [], []
        dense = np.zeros((self.B, N, N))
        absA = np.zeros((self.B, N, N))
        tile = np.zeros((self.B, N, N), dtype=np.float32)
        for g, rows in enumerate(graphs):
            assert len(rows) == N
            for r, (cs, vs) in enumerate(rows):
                cs, vs = np.asarray(cs, dtype=np.int64), np.asarray(vs, dtype=np.float32)
                assert cs.shape == vs.shape and np.all(np.diff(cs) >= 0) and np.all((cs >= 0) & (cs < N))
                np.add.at(dense[g, r], cs, vs.astype(np.float64))
                np.add.at(absA[g, r], cs, np.abs(vs).astype(np.float64))
                i = len(cs)
                while i > 0:                                        # runs, last entry first
                    j, s = i - 1, vs[i - 1]
                    while j > 0 and cs[j - 1] == cs[i - 1]:
                        j -= 1
                        s = np.float32(s + vs[j])
                    tile[g, r, cs[i - 1]] = s
                    i = j
                col.extend((g * N + cs).tolist())
                val.extend(vs.tolist())
                rowptr.append(len(col))
        self.n = self.B * N
        self.nnz = len(col)
        self.row_len = np.diff(np.asarray(rowptr))
        self.rowptr = torch.tensor(np.asarray(rowptr, dtype=np.int32), device=DEV)
        self.col = torch.tensor(np.asarray(col, dtype=np.int32), device=DEV)
        self.val = torch.tensor(np.asarray(val, dtype=np.float32), device=DEV)
        self.dense = torch.tensor(dense, device=DEV)
        self.absA = torch.tensor(absA, device=DEV)
        self.tile_b = torch.from_numpy(tile).bfloat16().double().to(DEV)
        self.X = randn(self.n, D, seed=N + 3 * self.B)

    def product(self, A, X):                                   # fp64 block-diagonal A [B,N,N] times X [n,256]
        return torch.bmm(A, X.double().view(self.B, self.N, D)).view(self.n, D)

    def __repr__(self):
        return self.name


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def signed_vals(rng, n):
    """Signed values of magnitude 0.05..1, about one in ten an explicit zero."""
    v = rng.uniform(0.05, 1.0, n) * rng.choice([-1.0, 1.0], n)
    v[rng.random(n) < 0.1] = 0.0
    return v.astype(np.float32).tolist()


def distinct(rng, N, n):
    return sorted(rng.choice(N, size=n, replace=False).tolist())


def row(rng, cs):
    return cs, signed_vals(rng, len(cs))


def lone_run(rng, N, length, first, count=2):
    """`length` entries, all columns distinct except entries first .. first + count - 1 (one run)."""
    cs = distinct(rng, N, length - count + 1)
    return cs[:first + 1] + [cs[first]] * (count - 1) + cs[first + 1:]


def short_rows(rng, N, k, most=6):
    rows = []
    for _ in range(k):
        n = int(rng.integers(0, min(N, most) + 1))
        rows.append(row(rng, distinct(rng, N, n)))
    return rows


def scatter(rng, N, special):
    """N rows: the special rows at random positions, short rows (0..6 entries) elsewhere."""
    rows = short_rows(rng, N, N)
    for r, sp in zip(rng.choice(N, size=len(special), replace=False).tolist(), special):
        rows[r] = sp
    return rows


def slot_run_graph(rng, N):
    """Family 1: rows of 65..330 entries whose ONLY run of equal columns sits on a slot edge of densify_rows."""
    sp = []
    for first, lengths in ((63, (65, 80, 151, 192, 193, 257, 330)), (127, (129, 151, 192, 193, 330)),
                           (191, (193, 208, 257, 330)), (192, (194, 209, 330)), (255, (257, 272, 330))):
        for L in lengths:                                       # the pair (first, first + 1)
            sp.append(row(rng, lone_run(rng, N, L, first)))
    sp.append(row(rng, lone_run(rng, N, 100, 62, 3)))           # a run of three ending at lane 0 of slot 1: 62, 63, 64
    sp.append(row(rng, lone_run(rng, N, 151, 126, 3)))          # ... of slot 2: 126, 127, 128
    sp.append(row(rng, lone_run(rng, N, 100, 64)))              # a run starting at lane 0: 64, 65
    sp.append(row(rng, lone_run(rng, N, 100, 62)))              # inside slot 0: 62, 63
    sp.append(row(rng, [int(rng.integers(N))] * 200))           # one run of 200 entries: every slot and the tail
    for first in (63, 127):                                     # a run that sums to zero: (v, -v) across the edge
        cs = lone_run(rng, N, 151, first)
        vs = signed_vals(rng, len(cs))
        vs[first], vs[first + 1] = 0.625, -0.625
        sp.append((cs, vs))
    sp.append(row(rng, list(range(N))))                         # a full row (columns 0 and N - 1)
    return scatter(rng, N, sp)


def make_slot_runs():
    rng = np.random.default_rng(101)
    N = 512
    return Case("slot_runs", N, [slot_run_graph(rng, N) for _ in range(2)])


ROW_LENGTHS_SHORT = (0, 1, 15, 16, 17)
ROW_LENGTHS_LONG = (63, 64, 65, 79, 80, 81, 128, 129, 191, 192, 193, 256, 257, None)   # None: a full row


def make_row_lengths():
    """Family 2: a row at every cut point of length; each 4-row group holds one long row among short and empty ones, at a
    position that moves from group to group.  The batch's last row is empty."""
    rng = np.random.default_rng(102)
    N, B = 301, 3
    graphs, k = [], 0
    for _ in range(B):
        rows = []
        for r in range(N):
            grp = r // 4
            if r % 4 == grp % 4 and grp % 5 != 4:               # (every fifth group: short rows only)
                L = ROW_LENGTHS_LONG[k % len(ROW_LENGTHS_LONG)]
                k += 1
            else:
                L = ROW_LENGTHS_SHORT[(r * 7 + grp) % len(ROW_LENGTHS_SHORT)]
            L = N if L is None else L
            rows.append(row(rng, distinct(rng, N, L)))
        graphs.append(rows)
    graphs[-1][-1] = ([], [])
    return Case("row_lengths", N, graphs)


def sized_graph(rng, N):
    """Rows of 0..12 distinct columns, some with a run of two (a quarter of them cancelling), one full row (columns 0 and
    N - 1 of the graph), and the last row holding column N - 1."""
    rows = []
    for _ in range(N):
        cs = distinct(rng, N, int(rng.integers(0, min(N, 12) + 1)))
        vs = signed_vals(rng, len(cs))
        if cs and rng.random() < 0.3:
            i = int(rng.integers(len(cs)))
            cs.insert(i + 1, cs[i])
            vs.insert(i + 1, -vs[i] if rng.random() < 0.25 else signed_vals(rng, 1)[0])
        rows.append((cs, vs))
    rows[int(rng.integers(N))] = row(rng, list(range(N)))
    if N > 1 and (not rows[-1][0] or rows[-1][0][-1] != N - 1):
        rows[-1] = (rows[-1][0] + [N - 1], rows[-1][1] + signed_vals(rng, 1))
    return rows


GRAPH_SIZES = ((1, 3), (31, 3), (32, 3), (33, 3), (63, 3), (64, 3), (65, 3), (127, 3), (128, 2), (129, 3), (511, 2), (512, 2))


def make_sized(N, B):
    """Family 3: graph sizes around the tile and shape switches (n_rows not a multiple of 4 or 16 where N allows)."""
    rng = np.random.default_rng(200 + N)
    if N == 1:                                                  # one-node graphs: a run of three, one entry, nothing
        v = signed_vals(rng, 4)
        return Case("graph_rows_1", 1, [[([0, 0, 0], v[:3])], [([0], v[3:])], [([], [])]])
    return Case("graph_rows_%d" % N, N, [sized_graph(rng, N) for _ in range(B)])


def make_empty_graph():
    """Family 5: a graph without entries in the middle of the batch; the batch's last row empty."""
    rng = np.random.default_rng(103)
    N = 65
    graphs = [sized_graph(rng, N), [([], [])] * N, sized_graph(rng, N)]
    graphs[-1][-1] = ([], [])
    return Case("empty_middle_graph", N, graphs)


def make_one_row():
    return Case("one_row", 1, [[([0, 0], [0.75, -0.3125])]])


def make_threshold(nnz):
    """Auto dispatch: 2 graphs of 64 rows (8192 places) holding exactly nnz entries."""
    rng = np.random.default_rng(nnz)
    N, B = 64, 2
    flat = np.sort(rng.choice(B * N * N, size=nnz, replace=False))
    graphs = [[([], []) for _ in range(N)] for _ in range(B)]
    for f in flat.tolist():
        g, r, c = f // (N * N), (f // N) % N, f % N
        graphs[g][r][0].append(c)
    for g in range(B):
        for r in range(N):
            graphs[g][r] = row(rng, graphs[g][r][0])
    return Case("density_%d_of_8192" % nnz, N, graphs)


# just below / just above each threshold (x 8192 places): 0.02 -> 163.84, 0.025 -> 204.8, 0.27 -> 2211.84
THRESHOLD_NNZ = (163, 164, 204, 205, 2211, 2212)

CASES = ["slot_runs", "row_lengths"] + ["graph_rows_%d" % N for N, _ in GRAPH_SIZES] + ["empty_middle_graph", "one_row"]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "slot_runs":
        return make_slot_runs()
    if name == "row_lengths":
        return make_row_lengths()
    if name == "empty_middle_graph":
        return make_empty_graph()
    if name == "one_row":
        return make_one_row()
    if name.startswith("graph_rows_"):
        N = int(name[len("graph_rows_"):])
        return make_sized(N, dict(GRAPH_SIZES)[N])
    return make_threshold(int(name[len("density_"):].split("_")[0]))


# ------------------------------------------------------------------------------------------------ checks
def assert_rows(c, Y, ref, den, tol, what):
    """max over rows of ||Y_r - ref_r|| / ||den_r|| <= tol; rows whose den is zero (no non-zero entry) exactly zero."""
    Y = Y.double()
    assert torch.isfinite(Y).all(), "%s / %s: non-finite output" % (c, what)
    d = den.norm(dim=1)
    zero = d == 0
    bad = torch.nonzero(zero & (Y != 0).any(1)).flatten().tolist()
    assert not bad, "%s / %s: rows without entries are not zero: %s" % (c, what, bad[:8])
    err = torch.where(zero, torch.zeros_like(d), (Y - ref).norm(dim=1) / d.clamp_min(1e-300))
    r = int(err.argmax())
    assert float(err[r]) <= tol, "%s / %s: row %d (graph %d, row %d, %d entries): error %.3g > %.1g" % (
        c, what, r, r // c.N, r % c.N, int(c.row_len[r]), float(err[r]), tol)


def spmm_into_nan_buffer(c, **kw):
    """csr_spmm into columns 0..255 of a NaN-filled [n, 320] buffer: every row written, columns 256.. untouched."""
    from fira_icse_amd import ops
    buf = torch.full((c.n, 320), float("nan"), device=DEV)
    Y = ops.csr_spmm(c.rowptr, c.col, c.val, c.X, graph_rows=c.N, out=buf[:, :D], **kw)
    assert Y.data_ptr() == buf.data_ptr()
    torch.cuda.synchronize()
    left = torch.nonzero(torch.isnan(buf[:, :D]).any(1)).flatten().tolist()
    assert not left, "%s / %s: rows never written: %s" % (c, kw, left[:8])
    assert torch.isnan(buf[:, D:]).all(), "%s / %s: wrote past column 255" % (c, kw)
    return buf[:, :D]


def check_spmm(c, Y, bf16, what):
    den = c.product(c.absA, c.X.abs())
    if bf16:
        # exact products of the rounded operands, fp32 accumulation: the only error left is the accumulation's
        ref = c.product(c.tile_b, c.X.bfloat16())
        assert_rows(c, Y, ref, den, 1e-6, what)
    else:
        assert_rows(c, Y, c.product(c.dense, c.X), den, 1e-6, what)


def auto_variant(c, dtype):
    """The variant fira_csr_spmm's variant 0 must pick (spmm.hip, from the thresholds above)."""
    if not (0 < c.N <= 512 and c.n % c.N == 0):
        return 1
    density = c.nnz / (c.n * c.N)
    if dtype == 1 and density >= SPMM_DENSE_AT_BF16:
        return 4
    if density >= SPMM_DENSE_AT_F32:
        return 3
    if density >= SPMM_LDS_AT:
        return 2
    return 1


# ------------------------------------------------------------------------------------------------ SpMM
@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", CASES)
def test_csr_spmm_rows_on_every_cut(name, variant):
    """Variants 1 (row batch), 2 (LDS slab; every graph here has <= 512 rows), 3 / 4 (block-dense fp32 / bf16 via
    densify_rows) and 5 (row per wave): per-row error against the fp64 product (variant 4: of the bf16-rounded operands,
    with the run-sum tile); every output row written, nothing past column 255."""
    c = case(name)
    Y = spmm_into_nan_buffer(c, variant=variant)
    check_spmm(c, Y, variant == 4, "variant %d" % variant)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("name", CASES + ["density_%d_of_8192" % k for k in THRESHOLD_NNZ])
def test_csr_spmm_auto_dispatch_is_pinned(name, dtype):
    """Variant 0 with auto: the choice follows the documented density thresholds (cases just below and just above each),
    and the result is bit-equal to an explicit call of that variant (no variant uses atomics)."""
    from fira_icse_amd import ops
    c = case(name)
    v = auto_variant(c, dtype)
    if name.startswith("density_"):
        k = c.nnz
        want = {163: (1, 1), 164: (2, 2), 204: (2, 2), 205: (2, 4), 2211: (2, 4), 2212: (3, 4)}[k][dtype]
        assert v == want, (k, dtype, v)
    Ya = spmm_into_nan_buffer(c, variant=0, auto=True, dtype=dtype)
    Yv = ops.csr_spmm(c.rowptr, c.col, c.val, c.X, graph_rows=c.N, variant=v)
    assert torch.equal(Ya, Yv), "%s: auto (dtype %d) differs from variant %d" % (c, dtype, v)
    check_spmm(c, Ya, v == 4, "auto dtype %d -> variant %d" % (dtype, v))


# ------------------------------------------------------------------------------------------------ fused GCN layer
@pytest.mark.parametrize("dtype", [0, 1, 2, 3])
@pytest.mark.parametrize("name", CASES)
def test_gcn_layer_rows_on_every_cut(name, dtype):
    """fira_gcn_layer_{fwd,bwd} (gcn_fused.hip) against the folded formula of test_ops_gpu.test_gcn_layer_fused_fwd_bwd,
    per row.  The aggregations -- V = A_hat dY of the backward and rowsum = A_hat 1 -- against fp64 (1e-6 of |A| |dY|, zero
    on rows without entries).  dtypes 1 / 3 round the fp32 aggregate to bf16: an element whose fp64 value sits next to a
    bf16 rounding boundary may round the other way, a bf16 ulp that one row cannot hide under a per-row bound, so their
    reference rounds the kernel's own aggregate -- the gather of the backward launch (the same code) applied to X, itself
    checked against fp64 to 1e-6."""
    from fira_icse_amd import ops
    c = case(name)
    n, X = c.n, c.X
    W21, b2, c21 = randn(D, D, seed=2, scale=0.06), randn(D, seed=3, scale=0.1), randn(D, seed=4, scale=0.1)
    gamma, beta = 1 + randn(D, seed=5, scale=0.1), randn(D, seed=6, scale=0.1)
    p, seed, site = 0.1, 4321, 7
    bf = dtype in (1, 3)
    tol = 3e-5 if bf else 2e-6                                  # test_gcn_layer_fused_fwd_bwd's, here per row
    r16 = (lambda t: t.float().bfloat16().double()) if bf else (lambda t: t.double())
    absrow = c.absA.sum(2).view(n)
    # backward first: its gather on X is the aggregate the bf16 forward rounds
    dY, dX0 = randn(n, D, seed=7), randn(n, D, seed=8)
    dX = dX0.clone()
    V = ops.gcn_layer_bwd(c.rowptr, c.col, c.val, dY, W21, dX, dtype=dtype)
    refV = c.product(c.dense, dY)
    assert_rows(c, V, refV, c.product(c.absA, dY.abs()), 1e-6, "bwd V")
    ref_dX = dX0.double() + r16(V if bf else refV) @ r16(W21)
    assert_rows(c, dX, ref_dX, ref_dX, tol, "bwd dX")
    U = c.product(c.dense, X)
    if bf:
        UX = ops.gcn_layer_bwd(c.rowptr, c.col, c.val, X, W21, torch.zeros_like(X), dtype=dtype)
        assert_rows(c, UX, U, c.product(c.absA, X.abs()), 1e-6, "gather of X")
        U = UX.double()
    summ, y, stats, rs = ops.gcn_layer_fwd(c.rowptr, c.col, c.val, X, W21.t().contiguous(), b2, c21, gamma, beta, dropout=p,
                                           seed=seed, site=site, dtype=dtype)
    rowsum = c.dense.sum(2).view(n)
    assert_rows(c, rs.view(n, 1), rowsum.view(n, 1), absrow.view(n, 1), 1e-6, "rowsum")
    pre = r16(U) @ r16(W21).t() + b2.double() + rowsum[:, None] * c21.double()
    mask = ops.dropout_mask(seed, site, n * D, p).view(n, D).double()
    ref_sum = pre * mask + X.double()
    ref_y = F.layer_norm(ref_sum, (D,), gamma.double(), beta.double(), 1e-5)
    assert_rows(c, summ, ref_sum, ref_sum, tol, "fwd sum")
    assert_rows(c, y, ref_y, ref_y, 5 * tol, "fwd y")
    mean, rstd = ref_sum.mean(1), 1.0 / torch.sqrt(ref_sum.var(1, unbiased=False) + 1e-5)
    assert_rows(c, stats[:, 1:], rstd[:, None], rstd[:, None], 1e-5, "fwd rstd")
    assert float((stats[:, 0] - mean).norm() / mean.norm()) < 1e-4
