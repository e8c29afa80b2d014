"""The training step's tail in the forms the engine calls: copy head (key mask, copy-label row mask, ragged rows, partial
dw | dbias rows, the decode step's shared memory), the loss kernels on computed rows, the embedding scatters, the row movers
and the deferred column reductions -- each against a plain float64 torch statement of the same operation (tests/tail_ref.py).

Whole-tensor relative error: the bounds the suite already states for these kernels (tests/test_ops_gpu.py): 2e-6 forward,
5e-6 gradients, 1e-5 dw / db, 1e-6 scatters and column sums.

Worst row (tail_ref.worst_row: max over rows of |row - ref| / max(|ref row|, median reference row norm)): a whole-tensor norm
cannot see one wrong row.  Bound = 4 x the worst row of the SAME statement evaluated by torch in float32 against float64 on
the same inputs (4 x for the kernels' other summation order), measured on the CPU by ``python tests/tail_ref.py``:

    quantity   fp32 vs fp64   bound            quantity   fp32 vs fp64   bound
    score      1.198e-07      4.794e-07        dscore     1.021e-07      4.085e-07
    dsrc       2.379e-07      9.516e-07        dgate      1.513e-07      6.052e-07
    dtgt       1.890e-07      7.558e-07        scatter    5.376e-07      2.150e-06
    dlogits    1.180e-07      4.718e-07        dscore through the forward (composition test)  1.422e-07  5.686e-07

Buffers start as NaN / sentinels wherever a kernel has to write (or must not): those are data, every index is in range.
"""
import numpy as np
import pytest
import torch

import util  # noqa: F401
import tail_ref as R
from tail_ref import rel_err, worst_row

pytestmark = pytest.mark.gpu

DEV = "cuda"
WORST = {"score": 4.794e-07, "dsrc": 9.516e-07, "dtgt": 7.558e-07, "dlogits": 4.718e-07, "dscore": 4.085e-07,
         "dgate": 6.052e-07, "scatter": 2.150e-06, "dscore_composed": 5.686e-07}
NAN = float("nan")


def close(name, got, ref, tol):
    """whole-tensor bound `tol` and the worst-row bound of quantity `name`; the figures are printed before they are asserted."""
    e, wr = rel_err(got, ref), worst_row(got, ref)
    print("%s: rel %.3e (< %.0e)  worst row %.3e (< %.3e)" % (name, e, tol, wr, WORST[name]))
    assert e < tol, (name, e)
    assert wr < WORST[name], (name, wr)


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def ref_score_dev(src, tgt, w, bias, row_b):
    return R.copy_score(*dev(src, tgt, w, bias, row_b), torch.float64)


# ------------------------------------------------------------------------------------------------ copy score, forward
@pytest.mark.parametrize("T", [30, 32, 1])
@pytest.mark.parametrize("S", [37, 370])
def test_copy_fwd_key_mask(S, T):
    """Unmasked slots equal the reference; masked slots hold exactly 0; nothing of the NaN-filled buffer is left (S = 37:
    the last chunk of 8 slots has 5)."""
    from fira_icse_amd import ops
    B = 3
    src, tgt, w, bias = R.copy_inputs(B, B * T, S, 11)
    row_b = torch.arange(B).repeat_interleave(T)
    valid = R.copy_valid(B, S, 12)
    ref = ref_score_dev(src, tgt, w, bias, row_b)
    src, tgt, w, bias, valid = dev(src, tgt, w, bias, valid)
    score = torch.full((B * T, S), NAN, device=DEV)
    ops.copy_score_fwd_ex(src, tgt, w, bias, score, T, mem_valid=valid)
    vr = valid[row_b.to(DEV)] != 0
    assert bool(torch.isfinite(score).all())
    assert float(score[~vr].abs().max()) == 0.0
    close("score", score, torch.where(vr, ref, torch.zeros_like(ref)), 2e-6)
    plain = torch.full((B * T, S), NAN, device=DEV)
    ops.copy_score_fwd_ex(src, tgt, w, bias, plain, T)
    close("score", plain, ref, 2e-6)


@pytest.mark.parametrize("S", [37, 370])
def test_copy_fwd_decode_rows_share_their_commits_memory(S):
    """The decode step: T = 1, qpk = 3 hypothesis rows per commit read one memory / key mask."""
    from fira_icse_amd import ops
    B, qpk = 6, 3
    src, tgt, w, bias = R.copy_inputs(B // qpk, B, S, 13)
    valid = R.copy_valid(B // qpk, S, 14)
    row_b = torch.arange(B) // qpk
    ref = ref_score_dev(src, tgt, w, bias, row_b)
    src, tgt, w, bias, valid = dev(src, tgt, w, bias, valid)
    score = torch.full((B, S), NAN, device=DEV)
    ops.copy_score_fwd_ex(src, tgt, w, bias, score, 1, qpk=qpk, mem_valid=valid)
    vr = valid[row_b.to(DEV)] != 0
    assert float(score[~vr].abs().max()) == 0.0
    close("score", score, torch.where(vr, ref, torch.zeros_like(ref)), 2e-6)


LENS = [30, 1, 17, 29, 8]


@pytest.mark.parametrize("S", [37, 370])
def test_copy_fwd_ragged_target_rows(S):
    """t_off: the rows that exist equal the dense computation; the rows of `score` past t_off[B] keep their sentinel."""
    from fira_icse_amd import ops
    T, B = 30, len(LENS)
    t_off, row_bt, row_b = R.ragged_rows(LENS, T)
    n = int(t_off[-1])
    src, tgt_dense, w, bias = R.copy_inputs(B, B * T, S, 15)
    valid = R.copy_valid(B, S, 16)
    ref = ref_score_dev(src, tgt_dense, w, bias, torch.arange(B).repeat_interleave(T))[row_bt.long().to(DEV)]
    tgt = torch.cat([tgt_dense[row_bt.long()], torch.full((3, 256), NAN)])
    src, tgt, w, bias, valid, t_off = dev(src, tgt, w, bias, valid, t_off)
    score = torch.full((n + 3, S), 12345.0, device=DEV)
    ops.copy_score_fwd_ex(src, tgt, w, bias, score, T, mem_valid=valid, t_off=t_off)
    vr = valid[row_b.to(DEV)] != 0
    assert bool((score[n:] == 12345.0).all())
    assert float(score[:n][~vr].abs().max()) == 0.0
    close("score", score[:n], torch.where(vr, ref, torch.zeros_like(ref)), 2e-6)


# ------------------------------------------------------------------------------------------------ forward + loss
def run_loss_reference(fx):
    lg, sc, gt, vr, lab = dev(fx["logits"], fx["score"], fx["gate"], fx["valid"][fx["row_b"]], fx["label"])
    out = R.head_loss(lg, sc, gt, vr, lab, torch.float64)
    assert R.clamp_margin_ok(out[5], lab), "a live label of the fixture sits within a factor 100 of the 1e-10 clamp"
    return out


def logits_buffer(fx, ldl, rows=None):
    lg = torch.zeros(fx["R"], ldl)
    lg[:, :fx["V"]] = fx["logits"]
    lg = lg.to(DEV)
    return lg if rows is None else lg[rows].contiguous()


def check_loss(fx, ref, loss, ntok, lg, sc, gl, rows=None, dscore="dscore"):
    """loss / n_tok / the three in-place gradients against the reference; the rows planted under the clamp are exactly 0."""
    loss_ref, ntok_ref, dlg, dsc, dgt = ref[:5]
    V = fx["V"]
    assert int(ntok) == ntok_ref
    e = abs(float(loss) - float(loss_ref)) / float(loss_ref)
    print("loss: rel %.3e" % e)
    assert e < 2e-6
    close("dlogits", lg[:, :V], dlg if rows is None else dlg[rows], 5e-6)
    close(dscore, sc, dsc, 5e-6)
    close("dgate", gl, dgt, 5e-6)
    assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(lg[:, :V]).all())
    for r in fx["clamped_rows"]:
        assert float(sc[r].abs().max()) == 0.0 and float(gl[r].abs().max()) == 0.0, r
        k = r if rows is None else int((rows == r).nonzero()[0]) if bool((rows == r).any()) else None
        if k is not None:
            assert float(lg[k, :V].abs().max()) == 0.0, r
    dead = (fx["label"] == 0).to(DEV)
    assert float(sc[dead].abs().max()) == 0.0 and float(gl[dead].abs().max()) == 0.0


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("S", [37, 370])
def test_copy_fwd_label_mask_composed_with_head_loss(S, ragged):
    """The contract of the forward's tar_label form is a composition: "head_loss neither reads nor propagates the unwritten
    rows".  score starts as NaN; copy_score_fwd_ex(tar_label) then head_loss_ex on the same buffers give the reference's loss,
    n_tok, gate and logit gradients, and the WHOLE score buffer ends finite and equal to the reference dscore (zero on rows
    with a generator label, zero on masked slots).  Fixture (tail_ref.loss_fixture): a commit without any copy label (the
    forward's mask == 0 return), a copy label at position T-2 (the last one `t0 < T - 1` admits), one on a masked slot."""
    from fira_icse_amd import ops
    T, V = 30, 1000
    fx = R.loss_fixture(V, S, T, R.LOSS_SEED, R.RAGGED if ragged else None)
    B, n = fx["B"], fx["R"]
    assert int(fx["tar_label"][0, T - 1]) >= V and not bool((fx["tar_label"][1] >= V).any())
    src, tgt, w, bias = R.copy_inputs(B, n, S, 17)
    fx["score"] = R.copy_score(src, tgt, w, bias, fx["row_b"], torch.float64)            # the head sees the copy head's scores
    ref = run_loss_reference(fx)
    src, tgt, w, bias, valid, lab, t_off, row_bt = dev(src, tgt, w, bias, fx["valid"], fx["tar_label"], fx["t_off"], fx["row_bt"])
    score = torch.full((n, S), NAN, device=DEV)
    ops.copy_score_fwd_ex(src, tgt, w, bias, score, T, mem_valid=valid, tar_label=lab, V=V, t_off=t_off if ragged else None)
    copy_rows = (fx["label"] >= V).to(DEV)
    vr = valid[fx["row_b"].to(DEV)] != 0
    full = ref_score_dev(src, tgt, w, bias, fx["row_b"])
    assert bool(torch.isfinite(score[copy_rows]).all()) and float(score[copy_rows][~vr[copy_rows]].abs().max()) == 0.0
    close("score", score[copy_rows], torch.where(vr, full, torch.zeros_like(full))[copy_rows], 2e-6)
    r1 = int(fx["t_off"][1]), int(fx["t_off"][2])
    assert bool(torch.isnan(score[r1[0]:r1[1]]).all())                 # the commit without a copy label was not touched
    lg, gl = logits_buffer(fx, V), fx["gate"].clone().to(DEV)
    loss, ntok, _ = ops.head_loss_ex(lg, score, valid, gl, lab, V, row_bt=row_bt if ragged else None)
    check_loss(fx, ref, loss, ntok, lg, score, gl, dscore="dscore_composed")


# ------------------------------------------------------------------------------------------------ copy score, backward
def run_copy_bwd(c, T, part=False, t_off=None, n_extra=0):
    """Launch the backward on NaN / non-zero start values; returns what the kernel left and the start values."""
    from fira_icse_amd import ops
    B, S = c["B"], c["S"]
    src, tgt, w, valid, ds = dev(c["src"], c["tgt"], c["w"], c["valid"], c["dscore"])
    n = tgt.shape[0]
    dsrc = torch.full((B, S, 256), NAN, device=DEV)
    dtgt0 = torch.cat([R.randn(n - n_extra, 256, seed=31, scale=0.5), torch.full((n_extra, 256), 777.0)]).to(DEV)
    dw0, db0 = R.randn(256, seed=32, scale=0.5).to(DEV), R.randn(1, seed=33, scale=0.5).to(DEV)
    dtgt, dw, db = dtgt0.clone(), dw0.clone(), db0.clone()
    pt = None
    if part:
        nb, st = ops.copy_score_bwd_blocks(B, S), ops.copy_part_stride()
        assert nb == B * ((S + 15) // 16) and st >= 257
        pt = torch.full((nb, st), NAN, device=DEV)
    ops.copy_score_bwd_ex(src, tgt, w, ds, dsrc, dtgt, dw, db, T, mem_valid=valid, part=pt,
                          t_off=None if t_off is None else t_off.to(DEV))
    return dsrc, dtgt, dw, db, pt, dtgt0, dw0, db0


def check_copy_bwd(c, got, ref, n_rows):
    dsrc, dtgt, dw, db, pt, dtgt0, dw0, db0 = got
    rsrc, rtgt, rw, rb = ref
    valid = c["valid"].to(DEV)
    assert bool(torch.isfinite(dsrc).all()), "a memory row of dsrc was not written"
    assert float(dsrc[valid == 0].abs().max()) == 0.0
    close("dsrc", dsrc, rsrc, 5e-6)
    close("dtgt", dtgt[:n_rows], dtgt0[:n_rows].double() + rtgt[:n_rows], 5e-6)          # dtgt accumulates
    assert torch.equal(dtgt[n_rows:], dtgt0[n_rows:])
    rwb = torch.cat([rw, rb])
    live = torch.where(valid[c["row_b"].to(DEV)] != 0, c["dscore"].to(DEV), torch.zeros((), device=DEV))
    db_scale = float(live.double().abs().sum())                                           # condition of the sum that dbias is
    if pt is None:
        e = rel_err(torch.cat([dw, db]), torch.cat([dw0, db0]).double() + rwb)
        print("dw|db: rel %.3e" % e)
        assert e < 1e-5
        assert abs(float(db) - float(db0) - float(rb)) < 1e-5 * db_scale
        return
    assert torch.equal(dw, dw0) and torch.equal(db, db0), "dw / dbias were touched although partial rows were asked for"
    assert bool(torch.isfinite(pt[:, :257]).all()), "a workgroup left its partial row unwritten"
    s = pt[:, :257].double().sum(0)
    e = rel_err(s, rwb)
    print("partial rows: rel %.3e" % e)
    assert e < 1e-5 and abs(float(s[256]) - float(rb)) < 1e-5 * db_scale
    from fira_icse_amd import ops
    dst = torch.cat([dw0, db0, torch.full((3,), 555.0, device=DEV)])
    ops.deferred_reduce([(dst, pt, 256, pt.shape[0], pt.shape[1]), (dst[256:], pt[:, 256:], 1, pt.shape[0], pt.shape[1])])
    assert rel_err(dst[:257], torch.cat([dw0, db0]).double() + rwb) < 1e-5 and bool((dst[257:] == 555.0).all())


@pytest.mark.parametrize("part", [False, True])
@pytest.mark.parametrize("T", [30, 32])
@pytest.mark.parametrize("S", [37, 370])
def test_copy_bwd_key_mask_chunks_and_partial_rows(S, T, part):
    """tail_ref.copy_bwd_case: commits with 8, 9, 16, 17 and 30 rows carrying gradient in the same slot tiles (chunks of
    COPY_KA = 8 active rows), one whose single active row is non-zero in one tile only, fully masked tiles (the mask == 0 exit,
    which must still zero its dsrc rows and write its partial row), 1e30 in dscore on every masked slot; S = 37: the last tile
    has 5 slots, waves 1..3 of it have fewer live slots than wave 0.  All four gradients equal the masked_fill reference; dsrc
    (NaN before) is finite everywhere and exactly 0 on masked slots; dtgt, dw, dbias add to their start values; with `part`
    every partial row is written, their sum -- in float64 and through fira_deferred_reduce onto a non-zero destination -- is
    dw | dbias, and the dw / dbias pointers are left alone."""
    c = R.copy_bwd_case(S, T)
    ref = R.copy_backward(*dev(c["src"], c["tgt"], c["w"], c["bias"], c["row_b"], c["valid"], c["dscore"]), torch.float64)
    got = run_copy_bwd(c, T, part)
    check_copy_bwd(c, got, ref, c["B"] * T)


@pytest.mark.parametrize("part", [False, True])
@pytest.mark.parametrize("S", [37, 370])
def test_copy_bwd_ragged_target_rows(S, part):
    """t_off as in the forward: lens 30, 1, 17, 29, 8; rows of dtgt past t_off[B] keep their sentinel."""
    T, B = 30, len(LENS)
    t_off, row_bt, row_b = R.ragged_rows(LENS, T)
    n = int(t_off[-1])
    src, tgt, w, bias = R.copy_inputs(B, n, S, 40)
    valid = R.copy_valid(B, S, 41)
    g = torch.Generator().manual_seed(42)
    ds = torch.zeros(n, S)
    act = torch.rand(n, generator=g) < 0.4
    act[int(t_off[1])] = True                                           # the commit with a single row has a gradient
    ds[act] = torch.randn(int(act.sum()), S, generator=g)
    ds = torch.where(valid[row_b] == 0, torch.full_like(ds, 1e30), ds)
    ref = R.copy_backward(*dev(src, tgt, w, bias, row_b, valid, ds), torch.float64)
    c = dict(B=B, S=S, src=src, tgt=torch.cat([tgt, torch.full((3, 256), NAN)]), w=w, valid=valid,
             dscore=torch.cat([ds, torch.full((3, S), NAN)]), row_b=torch.cat([row_b, torch.zeros(3, dtype=torch.long)]))
    got = run_copy_bwd(c, T, part, t_off=t_off, n_extra=3)
    c["dscore"], c["row_b"] = ds, row_b
    check_copy_bwd(c, got, ref, n)


# ------------------------------------------------------------------------------------------------ head loss
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("argmax", [False, True])
@pytest.mark.parametrize("V,S,lens", R.LOSS_CASES)
def test_head_loss_on_computed_rows(V, S, lens, argmax, compact):
    """head_loss_train_kernel (even V, no arg-max), head_loss_kernel<true> (even V, arg-max), head_loss_kernel<false>
    (V = 1001); V = 24650 / ldl = 24704: the register path's last pairs (a label on V - 1).  row_bt on ragged rows, with and
    without compact_row (logits only for the rows with a generator label).  Fixture rows (tail_ref.loss_fixture): the row at
    t = T-1 and a mid-sequence row with label 0; a generator label 40 below the maximum (p < 1e-10: loss -log(1e-10), every
    gradient of the row exactly 0, gate included); the gate saturated both ways with a label on the vanished branch; a label
    17 below a dominant maximum through the train kernel's one-exponential term.
    Clamp margin (asserted on the reference): no live label within a factor 100 of 1e-10, so that the fp32 kernel and the
    float64 reference stand on the same side of the clamp."""
    from fira_icse_amd import ops
    T = 30
    fx = R.loss_fixture(V, S, T, R.LOSS_SEED, lens)
    ref = run_loss_reference(fx)
    ldl = 24704 if V == 24650 else V
    valid, lab = dev(fx["valid"], fx["tar_label"])
    row_bt = None if lens is None else fx["row_bt"].to(DEV)
    rows, compact_row = None, None
    if compact:
        rows = ((fx["label"] > 0) & (fx["label"] < V)).nonzero().view(-1).to(DEV)
        compact_row = torch.full((fx["R"],), -1, dtype=torch.int32, device=DEV)
        compact_row[rows] = torch.arange(rows.numel(), dtype=torch.int32, device=DEV)
    lg, sc, gl = logits_buffer(fx, ldl, rows), fx["score"].clone().to(DEV), fx["gate"].clone().to(DEV)
    loss, ntok, ids = ops.head_loss_ex(lg, sc, valid, gl, lab, V, compact_row=compact_row, row_bt=row_bt, argmax=argmax)
    check_loss(fx, ref, loss, ntok, lg, sc, gl, rows)
    if argmax and not compact:
        assert torch.equal(ids.long(), ref[6])
    # the clamped rows each add exactly -log(1e-10); forward only (want_grad = 0) leaves the inputs alone
    lg2, sc2, gl2 = logits_buffer(fx, ldl, rows), fx["score"].clone().to(DEV), fx["gate"].clone().to(DEV)
    keep = (lg2.clone(), sc2.clone(), gl2.clone())
    loss2, ntok2, _ = ops.head_loss_ex(lg2, sc2, valid, gl2, lab, V, compact_row=compact_row, row_bt=row_bt, want_grad=False,
                                       argmax=argmax)
    assert abs(float(loss2) - float(loss)) < 1e-6 * float(loss) and int(ntok2) == int(ntok)     # (float atomics: any order)
    assert torch.equal(lg2, keep[0]) and torch.equal(sc2, keep[1]) and torch.equal(gl2, keep[2])


@pytest.mark.parametrize("V,S,lens", R.LOSS_CASES[:4])
def test_head_loss_argmax_ties_take_the_first_occurrence(V, S, lens):
    """The row maximum duplicated at indices owned by different threads and waves (and by one thread twice), in the generator
    and in the copy part: the first occurrence wins, as torch.argmax on the float64 reference."""
    from fira_icse_amd import ops
    fx = R.plant_argmax_ties(R.loss_fixture(V, S, 30, R.LOSS_SEED, lens))
    ref = run_loss_reference(fx)
    base = int(fx["t_off"][3])
    want = [5, 10, 600, 130, V + 3, V + S // 2]
    assert ref[6][base:base + 6].tolist() == want
    valid, lab = dev(fx["valid"], fx["tar_label"])
    row_bt = None if lens is None else fx["row_bt"].to(DEV)
    _, _, ids = ops.head_loss_ex(logits_buffer(fx, V), fx["score"].clone().to(DEV), valid, fx["gate"].clone().to(DEV), lab, V,
                                 row_bt=row_bt, want_grad=False, argmax=True)
    assert ids[base:base + 6].tolist() == want
    assert torch.equal(ids.long(), ref[6])


# ------------------------------------------------------------------------------------------------ embedding scatters
def scatter_close(got, ref):
    close("scatter", got, ref, 1e-6)


@pytest.mark.parametrize("n,hot", [(1, False), (5, False), (1021, False), (1021, True)])
def test_embed_rows_fwd_bwd(n, hot):
    """The decoder's token embedding on ragged computed rows: R = 1, 5, 1021 (not a multiple of the 4 rows per workgroup), ids
    equal to the padding index, one id on ~1000 rows (serialised atomics).  The gradient table starts non-zero."""
    from fira_icse_amd import ops
    T, B, rows_tab = 30, 80, 500
    g = torch.Generator().manual_seed(50 + n)
    lens, left = [], n
    while left > 0:
        k = min(left, int(torch.randint(1, T + 1, (1,), generator=g)))
        lens.append(k)
        left -= k
    assert len(lens) <= B
    lens += [0] * (B - len(lens))
    row_bt = torch.from_numpy(np.concatenate([b * T + np.arange(k) for b, k in enumerate(lens)]).astype(np.int32))
    idx = torch.randint(1, rows_tab, (B, T), generator=g)
    if hot:
        idx[torch.rand(B, T, generator=g) < 0.98] = 7
    idx[torch.rand(B, T, generator=g) < 0.1] = 0
    idx.view(-1)[row_bt[0].long()] = 0 if n > 1 else 3
    table, pos, dout, dt0 = (R.randn(rows_tab, 256, seed=51), R.randn(T, 256, seed=52), R.randn(n, 256, seed=53),
                             R.randn(rows_tab, 256, seed=54))
    ids = idx.view(-1)[row_bt.long()]
    out = ops.embed_rows_fwd(*dev(row_bt, idx.to(torch.int32), table, pos))
    assert torch.equal(out.cpu(), table[ids] + pos[row_bt.long() % T])
    dtab = ops.embed_rows_bwd(*dev(row_bt, idx.to(torch.int32), dt0.clone(), dout), padding_idx=0)
    scatter_close(dtab.cpu(), R.scatter_add(dt0, ids, dout, torch.float64))
    assert torch.equal(dtab[0].cpu(), dt0[0])
    untouched = torch.ones(rows_tab, dtype=torch.bool)
    untouched[ids] = False
    assert torch.equal(dtab.cpu()[untouched], dt0[untouched])


def test_embed_grouped_bwd_items_of_32_and_33_rows():
    """Lists from the project's own model.embedding_items on tail_ref.grouped_ids_batch: words occurring 1, 31, 32 (ONE item:
    the plain read-modify-write), 33 (TWO adjacent items: the atomic path), 64, 65 and 1000 times; the smallest and the largest
    id both span several items, so the first and the last item of the list are shared with a neighbour."""
    from fira_icse_amd import model as M, ops
    from fira_icse_amd.config import FiraConfig
    cfg = FiraConfig()
    hb = R.grouped_ids_batch(cfg)
    tok, ptr, rows = M.embedding_items(hb, cfg)
    per = {w: int((tok == w).sum()) for w in R.GROUP_COUNTS}
    assert per[4] == 1 and per[1] == 2 and per[299] == 3 and tok[0] == tok[1] == 1 and tok[-1] == tok[-2] == 299
    n_nodes = len(hb) * cfg.graph_len
    dnode, dt0 = R.randn(n_nodes, 256, seed=60), R.randn(R.GROUP_TABLE_ROWS, 256, seed=61)
    dtab = ops.embed_grouped_bwd(*dev(torch.from_numpy(tok), torch.from_numpy(ptr), torch.from_numpy(rows), dt0.clone(), dnode))
    ids = torch.from_numpy(np.repeat(tok.astype(np.int64), np.diff(ptr)))
    ref = R.scatter_add(dt0, ids, dnode[torch.from_numpy(rows).long()], torch.float64)
    scatter_close(dtab.cpu(), ref)
    assert torch.equal(dtab[0].cpu(), dt0[0])
    # the same sums from the id arrays themselves (what the lists stand for)
    all_ids = torch.from_numpy(np.concatenate([hb.sou, hb.sub_token], axis=1)).view(-1)
    L = cfg.sou_len + cfg.sub_token_len
    node = (torch.arange(len(hb))[:, None] * cfg.graph_len + torch.arange(L)[None, :]).view(-1)
    assert rel_err(ref, R.scatter_add(dt0, all_ids, dnode[node], torch.float64)) < 1e-12


@pytest.mark.parametrize("n", [1, 255, 256, 257, 3000])
def test_embed_list_bwd_small(n):
    """(row, id) pairs into the 71-row table: n around the slice of 256 items per workgroup; id 13 occurs in no slice; id 5
    fills 20 consecutive items of one wave (more than the eight row loads a wave has in flight)."""
    from fira_icse_amd import ops
    g = torch.Generator().manual_seed(70 + n)
    ids = torch.randint(1, 71, (n,), generator=g)
    ids[ids == 13] = 14
    if n >= 255:
        ids[70:90] = 5
    n_rows = n + 37
    rows = torch.randperm(n_rows, generator=g)[:n]
    dnode, dt0 = R.randn(n_rows, 256, seed=71), R.randn(71, 256, seed=72)
    dtab = ops.embed_list_bwd_small(*dev(rows.to(torch.int32), ids.to(torch.int32), dt0.clone(), dnode))
    scatter_close(dtab.cpu(), R.scatter_add(dt0, ids, dnode[rows], torch.float64))
    assert torch.equal(dtab[13].cpu(), dt0[13]) and torch.equal(dtab[0].cpu(), dt0[0])


def test_embed_gather_bwd_small_equals_the_plain_scatter():
    """The LDS-table form against fira_embed_gather_bwd and the reference; 141 rows are no multiple of the 64 per workgroup;
    the gradient rows sit at an offset inside a wider node buffer."""
    from fira_icse_amd import ops
    B, L, stride, off = 3, 47, 60, 5
    g = torch.Generator().manual_seed(80)
    idx = torch.randint(0, 71, (B, L), generator=g)
    dout, dt0 = R.randn(B * stride, 256, seed=81), R.randn(71, 256, seed=82)
    idx_d, dout_d = dev(idx.to(torch.int32), dout)
    small = ops.embed_scatter_add_small(idx_d, dt0.clone().to(DEV), dout_d, stride, off, 0)
    plain = ops.embed_scatter_add(idx_d, dt0.clone().to(DEV), dout_d, stride, off, 0)
    node = (torch.arange(B)[:, None] * stride + off + torch.arange(L)[None, :]).view(-1)
    ref = R.scatter_add(dt0, idx.view(-1), dout[node], torch.float64)
    scatter_close(small.cpu(), ref)
    scatter_close(plain.cpu(), ref)
    assert torch.equal(small[0].cpu(), dt0[0])


# ------------------------------------------------------------------------------------------------ row movers, reductions
@pytest.mark.parametrize("W", [256, 512])
@pytest.mark.parametrize("n", [1, 5, 1021])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_rows_move_on_a_column_block(mode, n, W):
    """All four modes on a column block of a wider matrix (ld = 3136): the columns on both sides and the rows nobody addresses
    keep their sentinel.  dst lists hold no duplicates (the kernel's precondition for modes 1-3); moves are exact."""
    from fira_icse_amd import ops
    ld, co, ci = 3136, 256, 512
    g = torch.Generator().manual_seed(90 + n)
    n_in, n_out = (n + 9, n) if mode in (0, 3) else (n, n + 9)
    if mode == 3:
        n_out = n + 9
    inp = R.randn(n_in, ld, seed=91).to(DEV)
    out0 = torch.full((n_out, ld), 4321.0)
    out0[:, co:co + W] = R.randn(n_out, W, seed=92)
    out = out0.clone().to(DEV)
    src = torch.randint(0, n_in, (n,), generator=g) if mode in (0, 3) else None
    dst = torch.randperm(n_out, generator=g)[:n] if mode != 0 else None
    ops.rows_move(mode, n, W, out[:, co:], ld, inp[:, ci:], ld, None if src is None else src.to(torch.int32).to(DEV),
                  None if dst is None else dst.to(torch.int32).to(DEV))
    blk = inp.cpu()[:, ci:ci + W]
    want = out0.clone()
    if mode == 0:
        want[:, co:co + W] = blk[src]
    elif mode == 1:
        want[dst, co:co + W] = blk
    elif mode == 2:
        want[dst, co:co + W] = out0[dst, co:co + W] + blk
    else:
        want[dst, co:co + W] = blk[src]
    assert torch.equal(out.cpu(), want)
    if mode == 0:                                        # src == NULL: the identity list
        ops.rows_move(0, n, W, out[:, co:], ld, inp[:, ci:], ld)
        assert torch.equal(out.cpu()[:, co:co + W], blk[:n]) and bool((out[:, :co] == 4321.0).all())


@pytest.mark.parametrize("M", [1, 5, 1021])
def test_rank2_rows(M):
    from fira_icse_amd import ops
    gt, w = R.randn(M, 2, seed=100), R.randn(2, 256, seed=101)
    out = ops.rank2_rows(*dev(gt, w))
    ref = gt.double() @ w.double()
    assert rel_err(out.cpu(), ref) < 2e-6
    fp32 = worst_row(gt @ w, ref)                         # the same statement in float32: the worst-row figure, 4 x allowed
    print("rank2 worst row %.3e (fp32 torch %.3e)" % (worst_row(out.cpu(), ref), fp32))
    assert worst_row(out.cpu(), ref) <= 4 * max(fp32, 2.0 ** -24)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("N", [2, 70, 256])
@pytest.mark.parametrize("M", [1, 257, 5000])
def test_colsum_weighted(M, N, weighted):
    """out[:N] += sum_m w[m] X[m, :N] with ldx > N onto a non-zero destination; what lies past N is not touched."""
    from fira_icse_amd import ops
    X, wt, o0 = R.randn(M, N + 6, seed=110), R.randn(M, seed=111), R.randn(N + 4, seed=112)
    out = ops.colsum_weighted(X.to(DEV), N, o0.clone().to(DEV), wt.to(DEV) if weighted else None).cpu()
    xs = X[:, :N].double() * (wt.double()[:, None] if weighted else 1.0)
    assert rel_err(out[:N], o0[:N].double() + xs.sum(0)) < 1e-6
    assert torch.equal(out[N:], o0[N:])


@pytest.mark.parametrize("case", [((1, 1536), (70, 63), (257, 65)), ((257, 1), (1, 64), (70, 65)),
                                  ((70, 1536), (257, 64), (1, 63)), ((257, 1536), (70, 1), (1, 65))])
def test_deferred_reduce_three_entries_in_one_launch(case):
    """(width, n_part) per entry: widths 1, 70, 257 (257 = the copy head's dw | dbias row: five column blocks, the last with one
    column), n_part around the 64 partial rows a workgroup sums; stride > width with NaN between the rows; non-zero
    destinations with a sentinel behind them."""
    from fira_icse_amd import ops
    assert ops.deferred_reduce_max() >= 3
    entries, want, dsts = [], [], []
    for k, (width, n_part) in enumerate(case):
        stride = width + 7
        src = torch.full((n_part, stride), NAN)
        src[:, :width] = R.randn(n_part, width, seed=120 + k)
        d0 = torch.cat([R.randn(width, seed=130 + k), torch.full((2,), 999.0)])
        dst = d0.clone().to(DEV)
        entries.append((dst, src.to(DEV), width, n_part, stride))
        want.append(d0[:width].double() + src[:, :width].double().sum(0))
        dsts.append(dst)
    ops.deferred_reduce(entries)
    for dst, ref in zip(dsts, want):
        got = dst.cpu()
        assert rel_err(got[:-2], ref) < 1e-6 and bool((got[-2:] == 999.0).all())
