"""Edge cases of the hot path against the CPU oracle: single commit, a commit without sub-tokens / AST / edits, a
message made only of copied tokens (no row needs the vocabulary head), a maximum-length message, an over-long diff."""
import numpy as np
import pytest
import torch

import util
from fira_icse_amd import data, synth
from fira_icse_amd.config import FiraConfig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model_sd():
    from fira_icse_amd.model import TransModel, reference_init_state_dict
    cfg = FiraConfig()
    torch.manual_seed(0)
    sd = util.perturb_state_dict(reference_init_state_dict(cfg), seed=1)
    model = TransModel(cfg, init=False)
    model.load_state_dict(sd)
    model.eval()
    return cfg, model, sd


@pytest.mark.parametrize("sel", [[0], [1], [2], [3], [0, 1, 2, 3]])
def test_loss_grad_and_ids_vs_oracle(model_sd, sel):
    from oracle import fira_oracle as O
    from fira_icse_amd.model import DeviceBatch
    cfg, model, sd = model_sd
    store = data.process_raw(cfg, util.edge_case_raw())
    hb = store.batch(sel)
    db = DeviceBatch(hb, cfg)
    if sel == [1]:
        assert db.n_head_rows <= 1                      # only the <eos> row can still need the generator
    tb = util.to_torch_batch(hb, cfg)
    P = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ls, nt = O.forward(P, cfg, tb["sou"], tb["tar"], tb["mark"], tb["ast_change"], tb["edge"], tb["tar_label"],
                       tb["sub_token"], "train")
    ls.backward()
    loss, ntok = model.train_fwd_bwd(db)
    assert int(ntok) == int(nt)
    assert abs(float(loss) - float(ls.detach())) <= 1e-5 * float(ls.detach())
    gv = model.grad_views()
    num = sum(float((gv[k].cpu().double() - p.grad.double()).norm() ** 2) for k, p in P.items() if p.grad is not None)
    den = sum(float(p.grad.double().norm() ** 2) for p in P.values() if p.grad is not None)
    assert (num / den) ** 0.5 < 1e-4
    with torch.no_grad():
        ids = O.forward(sd, cfg, tb["sou"], tb["tar"], tb["mark"], tb["ast_change"], tb["edge"], tb["tar_label"],
                        tb["sub_token"], "dev")
    real = tb["tar"] != 0                                # positions past the message are never read by dev()
    assert torch.equal(model.forward_dev(db).cpu().long()[real], ids[real])


def test_greedy_early_stop_and_single_commit(model_sd):
    """A batch whose every hypothesis ends immediately stops the chunked graph replay early; batch of one works."""
    from fira_icse_amd.model import DeviceBatch, TransModel
    from fira_icse_amd.decode import Searcher
    cfg, model, sd = model_sd
    sd2 = {k: v.clone() for k, v in sd.items()}
    sd2["out_fc.bias"][1] += 1e4                         # <eos> wins every step
    sd2["copy_net.LinearProb.bias"][0] += 50.0           # generator branch only
    m2 = TransModel(cfg, init=False)
    m2.load_state_dict(sd2)
    m2.eval()
    store = data.process_raw(cfg, util.edge_case_raw())
    for sel in ([2], [0, 1, 2, 3]):
        out, length, prob = Searcher(m2).greedy(DeviceBatch(store.batch(sel), cfg))
        assert length.tolist() == [2] * len(sel) and out[:, 1].tolist() == [1] * len(sel)
        assert float(prob.min()) > 0.99


_dense = {}


def _dense_host_batch(cfg):
    """Three synthetic commits with thousands of random AST-AST and AST-code edges added (~70 entries per computed row);
    built once per module."""
    if "hb" not in _dense:
        raw = synth.generate_dataset(3, seed=31)
        rng = np.random.default_rng(5)
        for i in range(3):
            n_a, n_d = len(raw["ast"][i]), len(raw["difftoken"][i])
            pairs = rng.integers(0, n_a, size=(9000, 2))
            raw["edge_ast"][i] = raw["edge_ast"][i] + [[int(a), int(b)] for a, b in pairs if a != b]
            ac = np.stack([rng.integers(0, n_a, 3000), rng.integers(0, n_d, 3000)], 1)
            raw["edge_ast_code"][i] = raw["edge_ast_code"][i] + [[int(a), int(b)] for a, b in ac]
        _dense["hb"] = data.process_raw(cfg, raw).batch([0, 1, 2])
    return _dense["hb"]


def test_dense_graphs_take_the_unfused_gcn_path_and_match_the_oracle():
    """Graphs far denser than FIRA's (BASELINE config 5's regime: here ~70 entries per computed row from thousands of random
    AST-AST and AST-code edges) make the engine run the GCN layers as aggregation + product + row kernel instead of the fused
    launch (engine.hip: graphs_dense).  Loss and every gradient tensor against the oracle on the dense float64
    adjacency, as for the sparse fixtures."""
    from oracle import fira_oracle as O
    from fira_icse_amd.model import TransModel, DeviceBatch, reference_init_state_dict
    cfg = FiraConfig()
    hb = _dense_host_batch(cfg)
    db = DeviceBatch(hb, cfg)
    assert db.nnz > 48 * db.n_nodes, (db.nnz, db.n_nodes)          # beyond the fused kernels' density limit
    torch.manual_seed(0)
    sd = util.perturb_state_dict(reference_init_state_dict(cfg), seed=1)
    model = TransModel(cfg, init=False)
    model.load_state_dict(sd)
    model.eval()
    tb = util.to_torch_batch(hb, cfg)
    P = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ls, nt = O.forward(P, cfg, tb["sou"], tb["tar"], tb["mark"], tb["ast_change"], tb["edge"], tb["tar_label"],
                       tb["sub_token"], "train")
    ls.backward()
    loss, ntok = model.train_fwd_bwd(db)
    assert int(ntok) == int(nt)
    assert abs(float(loss) - float(ls.detach())) / float(ls.detach()) < 1e-5
    gv = model.grad_views()
    floor = 1e-6 * max(float(p.grad.double().norm()) for p in P.values() if p.grad is not None)
    for k, p in P.items():
        if p.grad is None:
            continue
        ref = p.grad.double()
        err = float((gv[k].cpu().double() - ref).norm())
        tol = 3e-4 if ("feed_forward_list" in k and ".fc1." in k) else 1e-4
        assert err <= tol * float(ref.norm()) + floor, (k, err, float(ref.norm()))
    ids = model.forward_dev(db).cpu()
    with torch.no_grad():
        want = O.forward(sd, cfg, tb["sou"], tb["tar"], tb["mark"], tb["ast_change"], tb["edge"], tb["tar_label"],
                         tb["sub_token"], "dev")
    assert torch.equal(ids.long(), want.long())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_pending_step_owns_its_state(model_sd, dtype):
    """A step pending between train_step_begin and train_step_end keeps its own mode (engine.hip: Ctx::call): other library
    calls on the thread in between must not change its second half.  The step is begun on a sparse batch (fused GCN kernels);
    a dense batch evaluated in between (another model, its own workspaces) once switched the pending encoder backward to the
    unfused branch, which reads an aggregation the fused forward never wrote -- wrong gcn_list fc1 / fc2 gradients, no error;
    fira_ffn_bwd in between once reset the pending step's deferred column reductions.  The weight-gradient queue and its panel
    scratch travel with the step too (engine.h: WgradQueue): fira_gemm_wgrad_panel in between once left the pending encoder
    backward without scratch (its panel products silently unsplit), a training call on another workspace once pointed its
    partial tiles at that workspace.
    Bounds: those of test_encoder_wgrad_schedules_give_the_same_gradient (f32) and test_two_commit_lanes_equal_one (bf16)."""
    from fira_icse_amd import ops
    from fira_icse_amd.model import TransModel, DeviceBatch
    cfg, _, sd = model_sd
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = data.split_index(*util.GOLDEN_SPLIT, seed=0)
    db_sparse = DeviceBatch(store.batch(idx["train"][:util.GOLDEN_B]), cfg)
    db_dense = DeviceBatch(_dense_host_batch(cfg), cfg)
    assert db_dense.nnz > 48 * db_dense.n_nodes, (db_dense.nnz, db_dense.n_nodes)
    assert db_sparse.nnz < 48 * db_sparse.n_nodes, (db_sparse.nnz, db_sparse.n_nodes)
    models = []
    for _ in range(2):
        m = TransModel(cfg, init=False)
        m.load_state_dict(sd)
        m.eval()
        m.compute_dtype = dtype
        models.append(m)
    model, other = models
    ev = torch.cuda.Event()
    ev.record()

    def ffn_bwd_call():
        g = torch.Generator().manual_seed(7)
        r = lambda *s: (0.1 * torch.randn(*s, generator=g)).cuda()
        M, F = 64, 1024
        x, w1, b1, w2, b2, gamma, beta = r(M, 256), r(F, 256), r(F), r(256, F), r(256), 1.0 + r(256), r(256)
        h, summ, y, stats = ops.ffn_fwd(x, w1, b1, w2, b2, gamma, beta)
        ops.ffn_bwd(r(M, 256), x, h, summ, stats, w1, w2, gamma)

    def step(between):
        model.train_step_begin(db_sparse, ev)
        if between is not None:
            between()
        model.train_step_end(None, None, 0.0, 1, update=False)
        return model.gbuf[:model.layout.live].cpu().double()

    def wgrad_panel_call():                  # a taken shape (M = 32, N = 256, K = 512), with and without the split scratch
        g = torch.Generator().manual_seed(11)
        r = lambda *s: (0.1 * torch.randn(*s, generator=g)).cuda()
        A, B = r(512, 32), r(512, 256)
        for split in (True, False):
            ops.gemm_wgrad_panel(A, B, torch.zeros(32, 256, device="cuda"), dtype=int(dtype == "bf16"), split=split)

    want = step(None)
    cases = {"dense forward_dev": lambda: other.forward_dev(db_dense),
             "gemm_wgrad_panel": wgrad_panel_call,
             "train_fwd_bwd on another workspace": lambda: other.train_fwd_bwd(db_sparse)}
    if dtype == "f32":
        cases["ffn_bwd"] = ffn_bwd_call
    tol, tol_gcn = (1e-5, 2e-5) if dtype == "f32" else (3e-3, 3e-3)
    base = model.gbuf.data_ptr()
    for name, between in cases.items():
        got = step(between)
        rel = float((got - want).norm() / want.norm())
        worst = ("", 0.0)
        bad = []
        for k, v in model.grad_views().items():
            if "gcn_list" not in k:
                continue
            o = (v.data_ptr() - base) // 4
            a, b = got[o:o + v.numel()], want[o:o + v.numel()]
            err, ref = float((a - b).norm()), float(b.norm())
            if ref > 0 and err / ref > worst[1]:
                worst = (k, err / ref)
            if err > tol_gcn * ref + 1e-12:
                bad.append((k, err, ref))
        print("%s [%s]: whole gradient rel %.3g, worst gcn_list tensor %s rel %.3g" % (name, dtype, rel, worst[0], worst[1]))
        assert rel < tol, (name, rel)
        assert not bad, (name, bad[:4])
