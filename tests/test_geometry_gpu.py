"""The engine at the corners of the geometry box ``get_layout`` accepts, against the CPU oracle (tests/geometry_ref.py).

Every whole-model test elsewhere runs at 210 / 160 / 280 / 30, six layers, 24650 words; the engine's choices among kernels
are keyed on geometry (layers 8+ of the encoder, the plane tables that stop at 8 / 10 / 12 layers, the grouped weight-gradient
table, the head loss's register path, zero-width arrays, full and ragged key tiles).  Each case of ``geometry_ref.CASES``
is the smallest shape that reaches one of those branches.  Per case:

  (a) fp32 loss, token count and every gradient tensor against oracle autograd, in both node layouts -- the assertions and
      tolerances of tests/test_model_gpu.py::test_full_gradient_vs_oracle;
  (b) teacher-forced arg-max ids against the oracle's wherever its top-2 margin exceeds 100 x its own fp32 rounding error;
  (c) three Adam steps against torch.optim.Adam on the oracle's gradients (2e-4 of the largest loss per token, the bound of
      test_adam_loss_curve_matches_reference_golden), and one Trainer.step with the row-sparse Adam against the dense update
      (the comparison of tests/test_adam_rows_gpu.py::test_rows_trainer_equals_dense_trainer: distance between two dense runs);
  (d) bf16 mode within the bounds of tests/test_bf16_gpu.py;
  (e) greedy and beam-3 search on peaked weights against ``O.beam_decode``: every hypothesis and length identical,
      probabilities to 2e-4 (test_beam3_all_hypotheses_and_probabilities_vs_oracle), eager launches == graph capture == replay.
      ``big_vocab`` (25602 words, more than the search's row kernels hold) must be refused before any launch, and train on.
"""
import os

import numpy as np
import pytest
import torch

import geometry_ref as G

pytestmark = pytest.mark.gpu

CASES = list(G.CASES.values())


@pytest.fixture(scope="module", params=CASES, ids=[c.name for c in CASES])
def setup(request):
    """Weights, batch and the oracle's fp32 loss / gradients of one case (computed once per case, never modified)."""
    from fira_icse_amd.model import DeviceBatch, TransModel
    case = request.param
    cfg, hb, sd = case.cfg, G.case_batch(case), G.case_weights(case)
    model = TransModel(cfg, init=False)
    model.load_state_dict(sd)
    model.eval()
    ref = G.oracle_loss_and_grads(cfg, sd, hb)
    return case, model, hb, sd, DeviceBatch(hb, cfg), ref


def _check_gradient(model, grads, what):
    gv = model.grad_views()
    floor = 1e-6 * max(float(g.double().norm()) for g in grads.values() if g is not None)
    for k, g in grads.items():
        if g is None:
            assert float(gv[k].abs().max()) == 0, (what, k)
            continue
        ref = g.double()
        err = float((gv[k].cpu().double() - ref).norm())
        # (the named exemption of test_full_gradient_vs_oracle: a ReLU tie moves the FFN's fc1 gradient by ~2e-4 of its norm)
        tol = 3e-4 if ("feed_forward_list" in k and ".fc1." in k) else 1e-4
        print("%s %-60s err %.3g of norm %.3g" % (what, k, err, float(ref.norm())))
        assert err <= tol * float(ref.norm()) + floor, (what, k, err, float(ref.norm()))


@pytest.mark.parametrize("layout", ["computed", "dense"])
def test_fp32_loss_and_every_gradient_vs_oracle(setup, layout):
    from fira_icse_amd.model import DeviceBatch
    case, model, hb, sd, db, (ls, nt, grads) = setup
    if layout == "dense":
        db = DeviceBatch(hb, case.cfg, skip_padding=False)
        assert db.n_nodes == case.B * case.cfg.graph_len
    model.compute_dtype = "f32"
    loss, ntok = model.train_fwd_bwd(db)
    print(case.name, layout, "loss", float(loss), "oracle", ls, "n_tok", int(ntok), nt)
    assert int(ntok) == nt
    assert abs(float(loss) - ls) / ls < 1e-5, (float(loss), ls)
    _check_gradient(model, grads, "%s/%s" % (case.name, layout))


def test_teacher_forced_argmax_vs_oracle(setup):
    case, model, hb, sd, db, _ = setup
    want, margin = G.oracle_argmax_and_margins(case.cfg, sd, hb)
    sure = G.labelled(hb) & (margin > case.threshold)
    assert sure.sum() >= (1 - G.ARGMAX_MAX_EXCLUDED) * G.labelled(hb).sum()      # (tests/test_geometry.py asserts it on the CPU)
    model.compute_dtype = "f32"
    ids = model.forward_dev(db).cpu().numpy()
    assert ids.shape == want.shape
    assert np.array_equal(ids[sure], want[sure]), (case.name, np.argwhere(sure & (ids != want)).tolist())


def test_three_adam_steps_vs_oracle(setup):
    from fira_icse_amd import ops
    case, model, hb, sd, db, _ = setup
    cfg = case.cfg
    ref = np.array(G.oracle_adam_curve(cfg, sd, hb, 3))
    model.compute_dtype = "f32"
    model.load_state_dict(sd)
    try:
        m, v = torch.zeros_like(model.gbuf), torch.zeros_like(model.gbuf)
        inv = torch.zeros(1, device="cuda")
        curve = []
        for step in range(1, 4):
            loss, ntok = model.train_fwd_bwd(db)
            curve.append(float(loss) / float(ntok))
            ops.inv_count(ntok, inv)
            ops.adam_step(model.flat.data, model.gbuf, m, v, cfg.lr, step, inv_scale=inv)
        loss, ntok = model.train_fwd_bwd(db)
        curve.append(float(loss) / float(ntok))
    finally:
        model.load_state_dict(sd)
    print(case.name, "curve", curve, "oracle", ref.tolist())
    assert np.abs(np.array(curve) - ref).max() / ref.max() < 2e-4, (curve, ref.tolist())


def test_row_sparse_trainer_step_equals_dense(setup):
    """One Trainer.step on fresh weights: fira_train_step_rows against fira_train_step (FIRA_ADAM_ROWS=0), dropout on with
    the same masks.  The step's split-K sums are not bit-reproducible, so the yardstick is the distance between two dense
    runs, with the floors of test_rows_trainer_equals_dense_trainer."""
    from fira_icse_amd.model import DeviceBatch, TransModel
    from fira_icse_amd.train import Trainer
    case, _, hb, sd, _, _ = setup
    cfg = case.cfg
    out = {}
    for run, rows in (("rows", "1"), ("dense", "0"), ("dense2", "0")):
        os.environ["FIRA_ADAM_ROWS"] = rows
        try:
            model = TransModel(cfg, init=False)
            model.load_state_dict(sd)
            model.train()
            model.set_dropout_stream(3, 0)
            tr = Trainer(model)
        finally:
            os.environ.pop("FIRA_ADAM_ROWS", None)
        assert (tr.row_step is not None) == (rows == "1")
        tr.step(DeviceBatch(hb, cfg, model.device_))
        loss = tr.last_loss()
        new = model.state_dict()                                  # (syncs the rows the batch did not touch)
        if rows == "1":
            assert int(tr.row_step.min()) == 1
        out[run] = (model.flat.data.clone(), tr.m.clone(), tr.v.clone(), new["encoder.embedding.weight"].clone(),
                    new["decoder.embedding.weight"].clone(), loss)
    live = model.layout.live

    def dist(x, y):
        return float((x - y).norm() / y.norm())
    for k, name in enumerate(("params", "m", "v")):
        a, b, b2 = (out[r][k][:live] for r in ("rows", "dense", "dense2"))
        floor = {"params": 1e-4, "m": 1e-2, "v": 1e-3}[name]
        print(case.name, name, "rows-dense", dist(a, b), "dense-dense", dist(b2, b))
        assert dist(a, b) < 6 * dist(b2, b) + floor, (name, dist(a, b), dist(b2, b))
    # No row of the two word tables was left behind.  After ONE step every element of a touched row has moved by about lr
    # (Adam's first update is lr * g / (|g| + eps)), so a row the sparse update forgot is a whole row update away from the dense
    # run: per touched row, the distance to the dense run is held against the length of the dense update itself.  A forgotten
    # row scores 1; the dense pair's own noise (an element whose gradient is of the size of eps takes another step in each
    # run, up to 2 lr on one of 256 elements: 0.125 of a row update) stays below the 0.25 allowed beside 6 x what that pair shows.
    for k, name in ((3, "encoder.embedding.weight"), (4, "decoder.embedding.weight")):
        a, b, b2 = (out[r][k] for r in ("rows", "dense", "dense2"))
        before = sd[name].to(b.device)
        step = (b - before).norm(dim=1)
        moved = step > 0
        assert int(moved.sum()) > 0
        assert not (a - before)[~moved].any(), name                   # rows without a gradient stay where they were
        rel = (a - b).norm(dim=1)[moved] / step[moved]
        noise = (b2 - b).norm(dim=1)[moved] / step[moved]
        print(case.name, name, "rows moved", int(moved.sum()), "worst", float(rel.max()), "dense pair", float(noise.max()))
        assert float(rel.max()) < 6 * float(noise.max()) + 0.25, (name, float(rel.max()), float(noise.max()))
    assert np.allclose(out["rows"][5], out["dense"][5], rtol=5e-3), (out["rows"][5], out["dense"][5])


def test_bf16_mode_vs_fp32_and_oracle(setup):
    case, model, hb, sd, db, (ls, nt, grads) = setup
    model.compute_dtype = "f32"
    l32, _ = model.train_fwd_bwd(db)
    l32, g32 = float(l32), model.gbuf.clone()
    model.compute_dtype = "bf16"
    try:
        l16, n16 = model.train_fwd_bwd(db)
        l16, n16, g16 = float(l16), int(n16), model.gbuf.clone()
    finally:
        model.compute_dtype = "f32"
    print(case.name, "bf16 loss", l16, "fp32", l32, "oracle", ls)
    assert n16 == nt
    assert abs(l16 - ls) / ls < 1e-2 and l16 != l32, (l16, l32, ls)
    if nt == 1:               # `min`: a single token -- the loss check only
        return
    live = model.layout.live
    cos = float(torch.nn.functional.cosine_similarity(g16[:live].double(), g32[:live].double(), dim=0))
    ratio = float(g16[:live].norm() / g32[:live].norm())
    print(case.name, "bf16 gradient cosine", cos, "norm ratio", ratio)
    if not (cos > 0.999 and abs(ratio - 1) < 2e-2):               # name the first tensor where the direction is lost
        for k, (off, shp) in model.layout.entries.items():
            n = int(np.prod(shp))
            a, b = g16[off:off + n].double(), g32[off:off + n].double()
            if float(b.norm()) > 0:
                print("    %-60s cos %.5f ratio %.4f" % (k, float(torch.nn.functional.cosine_similarity(a, b, dim=0)),
                                                          float(a.norm() / b.norm())))
    assert cos > 0.999, cos
    assert abs(ratio - 1) < 2e-2, ratio


# ------------------------------------------------------------------------------------------------------------- (e) search
@pytest.fixture(scope="module")
def search_setup(setup):
    """The case's model with its peaked weights (geometry_ref.peaked_weights) and a Searcher; the weights go back afterwards."""
    from fira_icse_amd.decode import Searcher
    case, model, hb, sd, db, _ = setup
    model.load_state_dict(G.peaked_weights(case))
    model.compute_dtype = "f32"
    yield case, model, db, Searcher(model)
    model.load_state_dict(sd)


def _same_search(a, b):
    (gen, length, _), (gen2, length2, _) = a, b
    live = torch.arange(gen.shape[-1], device=gen.device).expand_as(gen) < length.unsqueeze(-1)
    return torch.equal(length, length2) and torch.equal(gen * live, gen2 * live)


def test_greedy_and_beam3_vs_oracle_search(search_setup):
    """Every case the search takes; ``big_vocab`` must be refused instead (the issue's table: "the search must refuse")."""
    case, model, db, search = search_setup
    if case.cfg.vocab_size > 25600:
        return _refused_and_training_goes_on(case, model, db, search)
    B = case.B
    for beam in (1, 3):
        hyp, prob, _ = G.oracle_search(case, beam)
        run = (lambda **kw: search.greedy(db, **kw)) if beam == 1 else (lambda **kw: search.beam(db, 3, **kw))
        eager = run(use_graphs=False)
        first, replay = run(), run()                              # graph capture, then replay
        assert _same_search(eager, first) and _same_search(eager, replay), (case.name, beam)
        gen, length, p = (t.cpu().reshape(B, beam, -1) for t in first)
        for i in range(B):
            for j in range(beam):
                n = int(length[i, j, 0])
                print(case.name, beam, i, j, gen[i, j, :n].tolist(), float(p[i, j, 0]), prob[i][j])
                assert gen[i, j, :n].tolist() == hyp[i][j], (case.name, beam, i, j, hyp[i][j])
                assert abs(float(p[i, j, 0]) - prob[i][j]) <= 2e-4 * abs(prob[i][j]) + 1e-30, (case.name, beam, i, j)


def _refused_and_training_goes_on(case, model, db, search):
    from fira_icse_amd._lib import FiraError
    for run in (lambda: search.greedy(db), lambda: search.greedy(db, use_graphs=False), lambda: search.beam(db, 3)):
        with pytest.raises(FiraError, match=r"vocabulary 25602 .* outside 4\.\.25600"):
            run()
    sd = G.case_weights(case)
    model.load_state_dict(sd)
    ls, nt, _ = G.oracle_loss_and_grads(case.cfg, sd, G.case_batch(case))
    loss, ntok = model.train_fwd_bwd(db)
    assert int(ntok) == nt and abs(float(loss) - ls) / ls < 1e-5
