"""Learning-rate schedules on the device (include/fira_hip.h: fira_lr_schedule, fira_adam_opts.sched).

The claim that matters is the row-sparse one: a row that lags k steps owes k updates that each ran at a DIFFERENT rate, and the
lazy replay (in the update kernels, the catch-up / sync kernel and the forward gathers) must use each step's own rate -- so
after fira_adam_rows_sync the tables and both moments are EQUAL (torch.equal) to a dense update that was handed
fira_lr_at(step) step by step.  Then: torch.optim.Adam + LambdaLR, a constant schedule against no schedule, the reference's own
scheduled runs (tests/golden/sched_ref.json), two ranks against one process, resume, and the command line."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import util
from fira_icse_amd import data
from fira_icse_amd.config import FiraConfig

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")

# rates that change at every one of the 70 steps (constant: through its warmup only)
SCHEDULES = {
    "constant": dict(kind="constant", base_lr=1e-3, warmup_steps=5),
    "inv_sqrt": dict(kind="inv_sqrt", base_lr=1e-3, warmup_steps=10),
    "cosine": dict(kind="cosine", base_lr=1e-3, warmup_steps=8, decay_steps=60, min_lr=1e-5),
    "linear": dict(kind="linear", base_lr=2e-3, warmup_steps=3, decay_steps=50, min_lr=0.0),
}
T = 70                                                       # more than two rings of 32; crosses the every-row steps 32 and 64


def _tables(model, cfg):
    v = model.named_views()
    base = model.flat.data.data_ptr()
    out = []
    for name in ("decoder.embedding.weight", "encoder.embedding.weight"):
        off = (v[name].data_ptr() - base) // 4
        out.append((off, off + cfg.vocab_size * 256))
    return out


class _Rows:
    """Flat p / m / v buffers of the model's geometry with a dense side (driven with fira_lr_at(step) per step) and a row-sparse
    side (driven with the schedule), fed the same gradients."""

    def __init__(self, schedule, seed=5):
        from fira_icse_amd import _lib, ops
        from fira_icse_amd.model import TransModel
        self.L, self.ops = _lib, ops
        self.lib = _lib.lib()
        self.cfg = FiraConfig()
        self.model = TransModel(self.cfg, device=DEV)
        self.V = self.cfg.vocab_size
        self.tabs = _tables(self.model, self.cfg)
        self.total = self.model.flat.data.numel()
        self.gen = torch.Generator(device=DEV).manual_seed(seed)
        p0 = torch.randn(self.total, device=DEV, generator=self.gen) * 0.05
        self.dense = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
        self.rows = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
        self.last = torch.zeros(2 * self.V, dtype=torch.int32, device=DEV)
        self.g = torch.zeros(self.total, device=DEV)
        self.n_tok = torch.tensor([37], dtype=torch.int32, device=DEV)
        self.betas_eps = (0.9, 0.999, 1e-8)
        self.sched = ops.LrSchedule.make(schedule).struct()

    def lr(self, step):
        return self.ops.lr_at(self.sched, step)

    def opts(self, step):
        b1, b2, eps = self.betas_eps
        # lr = nan: with a schedule the field must not be read
        return self.L.AdamOpts(float("nan"), b1, b2, eps, step, self.L.ptr(self.rows[1]), self.L.ptr(self.rows[2]),
                               self.L.sched_ptr(self.sched))

    def gradient(self, step):
        """Rows 1..3 of each table at every step, row 1000 + step at that step only, a random 1 % of the rows below 20000; rows
        from 20000 on are never touched."""
        self.g.zero_()
        touched = []
        for a, b in self.tabs:
            rnd = torch.nonzero(torch.rand(20000, device=DEV, generator=self.gen) < 0.01).flatten()
            rows = torch.unique(torch.cat([torch.tensor([1, 2, 3, 1000 + step], device=DEV), rnd]))
            self.g[a:b].view(self.V, 256)[rows] = torch.randn(rows.numel(), 256, device=DEV, generator=self.gen)
            touched.append(rows.to(torch.int32))
        return touched

    def dense_step(self, step, state=None):
        b1, b2, eps = self.betas_eps
        p, m, v = self.dense
        for a, b in self.tabs:
            if state is None:
                self.ops.adam_step_mb(p[a:b], self.g[a:b], None, m[a:b], v[a:b], self.lr(step), step, self.n_tok, None, b1, b2, eps)
            else:
                self.ops.adam_step_clip(p[a:b], self.g[a:b], m[a:b], v[a:b], self.lr(step), step, state, n_tok=self.n_tok,
                                        beta1=b1, beta2=b2, eps=eps)

    def catchup(self, step, table, ids):
        ad = self.opts(step)
        self.L.check(self.lib.fira_adam_rows_catchup(self.L.cur_stream(), C.byref(self.model.dims), self.L.ptr(self.rows[0]),
                                                     C.byref(ad), self.L.ptr(self.last), table, self.L.ptr(ids), ids.numel()))

    def rows_step(self, step, state=None):
        ad = self.opts(step)
        s, d = self.L.cur_stream(), C.byref(self.model.dims)
        if state is None:
            self.L.check(self.lib.fira_adam_rows_step(s, d, self.L.ptr(self.rows[0]), self.L.ptr(self.g), C.byref(ad),
                                                      self.L.ptr(self.last), self.L.ptr(self.n_tok), None, 3))
        else:
            self.L.check(self.lib.fira_adam_rows_step_clip(s, d, self.L.ptr(self.rows[0]), self.L.ptr(self.g), C.byref(ad),
                                                           self.L.ptr(self.last), self.L.ptr(self.n_tok), None, 3,
                                                           self.L.ptr(state)))

    def sync_and_compare(self, step):
        ad = self.opts(step)
        self.L.check(self.lib.fira_adam_rows_sync(self.L.cur_stream(), C.byref(self.model.dims), self.L.ptr(self.rows[0]),
                                                  C.byref(ad), self.L.ptr(self.last)))
        for a, b in self.tabs:
            for name, x, y in zip("pmv", self.dense, self.rows):
                assert torch.equal(x[a:b], y[a:b]), (step, name)
        assert int(self.last.min()) == step == int(self.last.max())


# ------------------------------------------------------------------------------- 1. row-sparse == dense under a changing rate
@pytest.mark.parametrize("kind", list(SCHEDULES))
def test_rows_update_equals_dense_update_under_a_changing_rate(kind):
    r = _Rows(SCHEDULES[kind])
    rates = [r.lr(t) for t in range(1, T + 1)]
    assert len(set(rates)) >= (5 if kind == "constant" else 40)              # the rate really moves
    for step in range(1, T + 1):
        touched = r.gradient(step)
        r.dense_step(step)
        if step > 1 and step % 5 == 0:
            # what a forward pass does ahead of the step: rows it gathers -- lagging ones among them (the once-touched rows of
            # earlier steps), duplicates, never-touched rows, ids out of range -- brought up to step - 1
            for t in (0, 1):
                ids = torch.cat([touched[t], touched[t][:9],
                                 torch.tensor([1000 + step - 3, 1000 + step - 30, 21000 + step, r.V + 3, -1], dtype=torch.int32,
                                              device=DEV)])
                r.catchup(step - 1, t, ids)
        r.rows_step(step)
        for t, (a, b) in enumerate(r.tabs):                                # the touched rows are current after the step
            rows = touched[t].long()
            assert torch.equal(r.dense[0][a:b].view(r.V, 256)[rows], r.rows[0][a:b].view(r.V, 256)[rows]), (step, t)
        if step in (31, 47, 64, T):                # a full window of lag, mid-window, on an every-row step, at the end
            if step != 64:
                assert int(r.last.min()) < step                            # rows do lag (never-touched: since the last forced step)
            r.sync_and_compare(step)


@pytest.mark.parametrize("kind", list(SCHEDULES))
def test_clipped_rows_update_equals_clipped_dense_update_under_a_changing_rate(kind):
    """The _clip kernels with a binding threshold, and with a non-finite gradient injected at steps 31, 32 (a forced step) and 40:
    those steps are applied as zero-gradient steps at their own rate."""
    r = _Rows(SCHEDULES[kind], seed=7)
    state, scratch = r.ops.clip_state(DEV)
    n_bad = 0
    for step in range(1, T + 1):
        r.gradient(step)
        if step in (31, 32, 40):
            a, _ = r.tabs[step % 2]
            r.g[a + 256 * 2 + 7] = INF if step != 40 else float("nan")
            n_bad += 1
        r.ops.grad_sqsum(r.g, state, 0, scratch)
        r.ops.clip_finish(state, 1, 0.5, n_tok=r.n_tok)
        r.dense_step(step, state)
        r.rows_step(step, state)
        if step in (20, 31, 32, 41, T):
            st = r.ops.read_clip_state(state)
            assert st["zero_flag"] == (1 if step in (31, 32) else 0) and (st["coef"] < 1.0 or st["zero_flag"])
            r.sync_and_compare(step)
    st = r.ops.read_clip_state(state)
    assert st["n_nonfinite"] == n_bad == 3 and st["n_clipped"] == T - 3
    assert all(bool(torch.isfinite(x).all()) for x in r.rows)


def test_a_schedule_in_the_opts_is_validated_by_every_rows_entry():
    from fira_icse_amd import _lib
    r = _Rows(SCHEDULES["cosine"])
    r.sched = _lib.LrSchedule(2, 1e-3, 8, 8, 0.0)                          # decay_steps == warmup_steps
    for call in (lambda: r.rows_step(1), lambda: r.catchup(1, 0, torch.zeros(4, dtype=torch.int32, device=DEV)),
                 lambda: r.sync_and_compare(1)):
        with pytest.raises(_lib.FiraError, match="cosine needs decay_steps > warmup_steps"):
            call()


# ------------------------------------------------------------------------------- golden-batch helpers
def _golden_model():
    from fira_icse_amd.model import TransModel, reference_init_state_dict
    cfg = FiraConfig()
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = data.split_index(*util.GOLDEN_SPLIT, seed=0)["train"]
    torch.manual_seed(0)
    sd = util.perturb_state_dict(reference_init_state_dict(cfg), seed=1)
    model = TransModel(cfg, init=False)
    model.load_state_dict(sd)
    model.eval()
    return cfg, store, idx, model, sd


# ------------------------------------------------------------------------------- 2. lazy forward reads
def test_forward_reads_of_lagging_rows_replay_each_step_at_its_own_rate():
    """Step 1 on batch B, steps 2..4 on batch A: the words only B uses lag three steps, each owed at another rate.  Step 5 on B
    gathers them lazily (in registers); the same step from the same state after sync() reads them from memory.  The two forward
    passes must give the same loss, bit for bit.  (The loss is a sum of per-token terms added by atomics, in any order: for
    step 5 all labels of B but one are padded out, so that the sum has ONE term and its bits are a function of the forward
    pass alone -- every encoder row and the decoder rows up to that token still feed it.)"""
    from fira_icse_amd.config import PAD
    from fira_icse_amd.model import DeviceBatch
    from fira_icse_amd.train import Trainer
    cfg, store, idx, model, _ = _golden_model()
    hb_b, hb_5 = store.batch(idx[4:8]), store.batch(idx[4:8])
    lab = hb_5.tar_label.copy()
    keep = tuple(np.argwhere(lab != PAD)[3])                               # the fourth labelled token of the first commit
    lab[:] = PAD
    lab[keep] = hb_5.tar_label[keep]
    hb_5.tar_label = lab
    A, B, B5 = DeviceBatch(store.batch(idx[0:4]), cfg), DeviceBatch(hb_b, cfg), DeviceBatch(hb_5, cfg)
    tr = Trainer(model, lr_schedule=dict(kind="cosine", base_lr=1e-3, warmup_steps=3, decay_steps=6, min_lr=1e-4))
    assert tr.row_step is not None
    for db in (B, A, A, A):
        tr.step(db)
    torch.cuda.synchronize()
    rates = [tr._rate_of(t) for t in (2, 3, 4)]
    assert len(set(rates)) == 3                                            # the owed steps ran at three different rates
    V = cfg.vocab_size
    words = torch.as_tensor(np.unique(np.concatenate([hb_b.sou.reshape(-1), hb_b.sub_token.reshape(-1)])), device=DEV).long()
    assert int((tr.row_step[V + words] < 4).sum()) > 0                     # encoder-table rows B gathers do lag
    saved = [x.clone() for x in (model.flat.data, tr.m, tr.v, tr.row_step)]
    saved_dropout = model.dropout_step

    def step5(sync_first):
        for dst, src in zip((model.flat.data, tr.m, tr.v, tr.row_step), saved):
            dst.copy_(src)
        tr.t, tr._rows_dirty, model.dropout_step = 4, True, saved_dropout
        if sync_first:
            tr.sync()
            assert int(tr.row_step.min()) == 4
        else:
            assert int(tr.row_step.min()) < 4
        tr.step(B5)
        torch.cuda.synchronize()
        return model.loss_sum.clone(), int(model.n_tok.item())

    lazy, n1 = step5(False)
    synced, n2 = step5(True)
    lazy2, _ = step5(False)
    assert n1 == n2 == 1 and float(lazy) > 0
    assert torch.equal(lazy, lazy2)                                        # (the forward pass is reproducible at all)
    assert torch.equal(lazy, synced), (float(lazy), float(synced))


# ------------------------------------------------------------------------------- 3. torch.optim.Adam + LambdaLR
@pytest.mark.parametrize("kind", ["inv_sqrt", "cosine", "linear", "constant"])
def test_scheduled_adam_matches_torch_lambda_lr(kind):
    from fira_icse_amd import ops
    base = 1e-4
    s = ops.LrSchedule.make({"constant": dict(kind=kind, base_lr=base, warmup_steps=3),
                             "inv_sqrt": dict(kind=kind, base_lr=base, warmup_steps=2),
                             "cosine": dict(kind=kind, base_lr=base, warmup_steps=2, decay_steps=6, min_lr=1e-5),
                             "linear": dict(kind=kind, base_lr=base, warmup_steps=1, decay_steps=5)}[kind])
    n = 100003
    gen = torch.Generator(device=DEV).manual_seed(1)
    p0 = torch.randn(n, device=DEV, generator=gen)
    grads = [torch.randn(n, device=DEV, generator=gen) * 0.01 for _ in range(6)]
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=base)
    lrs = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: ops.lr_at(s, e + 1) / base)
    p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ntok = torch.tensor([8], dtype=torch.int32, device=DEV)
    inv = ops.inv_count(ntok, torch.zeros(1, device=DEV))
    for i, gr in enumerate(grads):
        ref.grad = gr / 8
        opt.step()
        lrs.step()
        ops.adam_step(p, gr, m, v, ops.lr_at(s, i + 1), i + 1, inv_scale=inv)
        assert float((p - ref.data).abs().max()) < 2e-7                    # (tests/test_ops_gpu.py::test_adam_matches_torch)


# ------------------------------------------------------------------------------- 4. a constant schedule changes nothing
@pytest.mark.parametrize("clip", [None, 1.0])
def test_a_constant_schedule_is_the_unscheduled_trainer(clip):
    """Trainer(lr_schedule=constant, W = 0) against Trainer() from the same state, five steps on the golden batch: the kernels
    divide the same float by the same bias correction.  torch.equal is asserted where it can hold -- on the update kernels fed
    the SAME gradient (here the dense one; the row kernels in the next test): the training step around them sums by atomics
    and is not bit-reproducible run to run (tests/test_adam_rows_gpu.py), so two runs of even the same Trainer differ in the
    last bits; the two Trainers are held to the tolerance two orders of summation get in tests/test_dp_gpu.py."""
    from fira_icse_amd.model import DeviceBatch
    from fira_icse_amd.train import Trainer
    cfg, store, idx, model, sd = _golden_model()
    db = DeviceBatch(store.batch(idx[0:4]), cfg)
    out = {}
    for name, schedule in (("plain", None), ("constant", dict(kind="constant", base_lr=cfg.lr, warmup_steps=0))):
        model.load_state_dict(sd)
        model.eval()
        tr = Trainer(model, clip_grad_norm=clip, lr_schedule=schedule)
        assert tr.row_step is not None
        losses = []
        for i in range(5):
            tr.step(db)
            assert tr.last_lr() == (cfg.lr if schedule is None else float(np.float32(cfg.lr)))
            losses.append(tr.last_loss())
        out[name] = (model.flat.data.clone(), tr.m.clone(), tr.v.clone(), losses)
    # the forward + backward pass of step 1 starts from the same bits; from step 2 on the runs may differ by atomics' noise, so
    # the bit-for-bit claim is made where it can hold: on the optimizer, fed the same gradient
    from fira_icse_amd import _lib, ops
    live = model.layout.live
    gen = torch.Generator(device=DEV).manual_seed(3)
    g = torch.randn(live, device=DEV, generator=gen)
    n_tok = torch.tensor([11], dtype=torch.int32, device=DEV)
    sched = ops.LrSchedule.make(dict(kind="constant", base_lr=cfg.lr, warmup_steps=0)).struct()
    sides = []
    for use in (None, sched):
        p = out["plain"][0][:live].clone()
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        for step in range(1, 6):
            lr = cfg.lr if use is None else ops.lr_at(use, step)
            ops.adam_step_mb(p, g, None, m, v, lr, step, n_tok, None)
        sides.append((p, m, v))
    for x, y in zip(*sides):
        assert torch.equal(x, y)
    # and the trainers themselves stay on one trajectory (the tolerance two runs of the SAME trainer need)
    assert np.allclose(out["plain"][3], out["constant"][3], rtol=1e-5), (out["plain"][3], out["constant"][3])
    d = (out["plain"][0][:live] - out["constant"][0][:live]).abs()
    assert float((d > 0.05 * cfg.lr).float().mean()) < 2e-4, float(d.max())


def test_constant_schedule_rows_kernels_are_bit_identical_to_the_plain_ones():
    """The row-sparse kernels with sched = constant (W = 0) against the same kernels with sched = NULL and lr: EQUAL after
    every step -- the ring then holds the caller's float in every entry."""
    from fira_icse_amd import _lib
    r = _Rows(dict(kind="constant", base_lr=1e-3, warmup_steps=0))
    plain = [x.clone() for x in r.rows]
    last_b = r.last.clone()
    b1, b2, eps = r.betas_eps
    for step in range(1, 40):
        r.gradient(step)
        r.rows_step(step)
        ad = _lib.AdamOpts(1e-3, b1, b2, eps, step, _lib.ptr(plain[1]), _lib.ptr(plain[2]))
        _lib.check(r.lib.fira_adam_rows_step(_lib.cur_stream(), C.byref(r.model.dims), _lib.ptr(plain[0]), _lib.ptr(r.g), C.byref(ad),
                                             _lib.ptr(last_b), _lib.ptr(r.n_tok), None, 3))
        if step % 8 == 0 or step >= 31:
            for x, y in zip(plain, r.rows):
                assert torch.equal(x, y), step
            assert torch.equal(r.last, last_b)


# ------------------------------------------------------------------------------- 5. the reference fixture
@pytest.mark.parametrize("rows", ["1", "0"])
def test_scheduled_training_matches_the_reference_runs(tmp_path, rows):
    """Both scheduled runs of tests/golden/sched_ref.json (the reference under torch.optim.Adam + LambdaLR): the 9-point loss
    curves within 2e-4 in fp32 -- the one-call path and the fwd_bwd + update path -- and 2e-2 in bf16, with the row-sparse
    tables on and off (a child process: the switch is read once); last_lr() equals the recorded rate exactly."""
    with open(os.path.join(util.GOLDEN, "sched_ref.json")) as f:
        ref = json.load(f)
    out = str(tmp_path / "sched.json")
    env = dict(os.environ, FIRA_ADAM_ROWS=rows, PYTHONPATH=util.REPO)
    r = subprocess.run([sys.executable, os.path.join(util.HERE, "sched_run.py"), out], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out) as f:
        got = json.load(f)
    assert got["rows"] == (rows == "1")
    assert set(ref["runs"]) == {"inv_sqrt", "cosine"}
    for name, run in ref["runs"].items():
        curve_ref = np.array(run["loss_curve"])
        for path, tol in (("f32/fused", 2e-4), ("f32/two_call", 2e-4), ("bf16/fused", 2e-2)):
            q = got["%s/%s" % (name, path)]
            cerr = float(np.abs(np.array(q["curve"]) - curve_ref).max() / curve_ref.max())
            print(name, path, "curve error %.3e" % cerr)
            assert q["lr"] == run["lr"], (name, path, q["lr"], run["lr"])
            assert cerr < tol, (name, path, q["curve"], run["loss_curve"])


# ------------------------------------------------------------------------------- 6. data parallel
DP_SCHEDULE = dict(kind="cosine", base_lr=FiraConfig().lr, warmup_steps=2, decay_steps=4, min_lr=0.0)   # base/2, base, base/2


def _dp_run(rank, world, port, out, zero1=False, wire="f32"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, util.REPO)
    from fira_icse_amd import ops
    from fira_icse_amd.model import TransModel, DeviceBatch, reference_init_state_dict
    from fira_icse_amd.train import Trainer
    from fira_icse_amd.parallel import shard_indices
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = FiraConfig()
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = data.split_index(*util.GOLDEN_SPLIT, seed=0)["train"]
    torch.manual_seed(0)
    model = TransModel(cfg, init=False)
    model.load_state_dict(util.perturb_state_dict(reference_init_state_dict(cfg), seed=1))
    model.eval()                                        # dropout off: the comparison must be deterministic
    trainer = Trainer(model, distributed=world > 1, zero1=zero1, grad_wire=wire, lr_schedule=DP_SCHEDULE)
    if world > 1 and not zero1:
        assert trainer.fused_dp and trainer.row_step is not None
    losses, lrs = [], []
    for step in range(3):
        # the last global batch holds ONE commit: with two ranks, rank 1's shard is empty -- it must apply the same update at
        # the same rate, and its rows must not be brought past the last completed step on the way
        gidx = idx[4 * step:4 * step + 4] if step < 2 else idx[8:9]
        mine = shard_indices(gidx, rank, world)
        trainer.step(DeviceBatch(store.batch(mine), cfg) if mine else None)
        losses.append(trainer.last_loss())
        lrs.append(trainer.last_lr())
    assert lrs == [ops.lr_at(trainer.lr_schedule, t) for t in (1, 2, 3)] and len(set(lrs[:2])) == 2
    torch.cuda.synchronize()
    opt = trainer.state_dict()                              # (syncs the lazy rows; collective with zero1)
    torch.save({"flat": model.flat.data.cpu(), "losses": losses, "lr": lrs, "m": opt["m"].cpu(), "v": opt["v"].cpu(),
                "schedule": opt["lr_schedule"]}, "%s.%d" % (out, rank))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _dp_pair(tmp_path, port, **kw):
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    mp.spawn(_dp_run, args=(1, port, one), nprocs=1, join=True)
    mp.spawn(_dp_run, args=(2, port + 1, two, kw.get("zero1", False), kw.get("wire", "f32")), nprocs=2, join=True)
    a = torch.load(one + ".0", weights_only=False)
    b = [torch.load("%s.%d" % (two, r), weights_only=False) for r in (0, 1)]
    assert a["lr"] == b[0]["lr"] == b[1]["lr"] and a["schedule"] == b[0]["schedule"] == DP_SCHEDULE
    assert torch.equal(b[0]["flat"], b[1]["flat"])          # the replicas stay identical (the empty-shard step included)
    return a, b[0]


def test_two_ranks_follow_the_schedule_like_a_single_process(tmp_path):
    # (the tolerances of tests/test_dp_gpu.py::test_two_rank_training_equals_single_process)
    a, b = _dp_pair(tmp_path, 30200 + (os.getpid() % 150))
    for x, y in zip(a["losses"], b["losses"]):
        assert abs(x - y) / x < 1e-5, (a["losses"], b["losses"])
    lr = FiraConfig().lr
    diff = (a["flat"] - b["flat"]).abs()
    assert float((diff > 0.05 * lr).float().mean()) < 2e-4, float(diff.max())
    assert float(diff.mean()) < 1e-3 * lr


def test_two_ranks_follow_the_schedule_with_the_bf16_gradient_wire(tmp_path):
    # (the tolerances of tests/test_dp_gpu.py::test_two_ranks_with_bf16_gradient_wire_track_single_process)
    a, b = _dp_pair(tmp_path, 30400 + (os.getpid() % 150), wire="bf16")
    assert abs(a["losses"][0] - b["losses"][0]) / a["losses"][0] < 1e-5
    for x, y in zip(a["losses"], b["losses"]):
        assert abs(x - y) / x < 1e-3, (a["losses"], b["losses"])
    diff = (a["flat"] - b["flat"]).abs()
    assert float(diff.mean()) < 0.05 * FiraConfig().lr, float(diff.mean())


def test_two_rank_zero1_follows_the_schedule_like_a_single_process(tmp_path):
    # (the tolerances of tests/test_dp_gpu.py::test_two_rank_zero1_equals_single_process)
    a, b = _dp_pair(tmp_path, 30600 + (os.getpid() % 150), zero1=True)
    for x, y in zip(a["losses"], b["losses"]):
        assert abs(x - y) / x < 1e-5, (a["losses"], b["losses"])
    lr = FiraConfig().lr
    diff = (a["flat"] - b["flat"]).abs()
    assert float((diff > 0.05 * lr).float().mean()) < 2e-4, float(diff.max())
    assert float(diff.mean()) < 1e-3 * lr


# ------------------------------------------------------------------------------- 7. / 8. command line
def _cli(args, cwd, ok=True):
    env = dict(os.environ, PYTHONPATH=util.REPO)
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "run_model.py")] + args, cwd=cwd, env=env, capture_output=True,
                       text=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def _log(path):
    with open(path) as f:
        return [json.loads(l) for l in f.read().splitlines()]


def test_resume_continues_the_saved_schedule(tmp_path):
    """train --lr-schedule cosine for 2 steps + --resume for 2 more == 4 uninterrupted steps (compared as
    tests/test_cli_gpu.py::test_resume_continues_from_the_saved_adam_state compares); the lr values of the two loss logs
    concatenate to the uninterrupted sequence; a resume under another schedule is refused."""
    from fira_icse_amd import ops, synth
    sched = ["--lr", "1e-3", "--lr-schedule", "cosine", "--warmup-steps", "1", "--lr-decay-steps", "4", "--lr-min", "1e-4"]
    common = ["--splits", "16,4,4", "--batch-size", "16", "--dev-from-epoch", "99", "--no-dropout", "--save-optimizer"]
    roots = {}
    for name in ("full", "split", "bare"):
        roots[name] = str(tmp_path / name)
        os.makedirs(roots[name])
        synth.write_dataset(roots[name], util.load_golden_raw())
    log = {k: os.path.join(r, "loss.jsonl") for k, r in roots.items()}
    _cli(["train", "--max-steps", "4", "--loss-log", log["full"]] + common + sched, roots["full"])
    _cli(["train", "--max-steps", "2", "--loss-log", log["split"]] + common + sched, roots["split"])
    st = torch.load(os.path.join(roots["split"], "fira_train_state.pt"), map_location="cpu")
    assert int(st["t"]) == 2 and st["lr_schedule"]["kind"] == "cosine" and st["lr_schedule"]["decay_steps"] == 4
    # a conflicting schedule is refused, and nothing is overwritten
    r = _cli(["train", "--max-steps", "2", "--resume"] + common + sched[:-1] + ["5e-4"], roots["split"], ok=False)
    assert r.returncode != 0 and "saved under the learning-rate schedule" in r.stderr
    assert int(torch.load(os.path.join(roots["split"], "fira_train_state.pt"), map_location="cpu")["t"]) == 2
    _cli(["train", "--max-steps", "2", "--resume", "--loss-log", log["split"]] + common + sched, roots["split"])
    st = torch.load(os.path.join(roots["split"], "fira_train_state.pt"), map_location="cpu")
    assert int(st["t"]) == 4
    s = ops.LrSchedule.make(st["lr_schedule"])
    want = [ops.lr_at(s, t) for t in (1, 2, 3, 4)]
    assert len(set(want)) == 4
    assert [rec["lr"] for rec in _log(log["full"])] == want
    assert [rec["lr"] for rec in _log(log["split"])] == want          # (2 lines of the first run + 2 of the resumed one)
    # --resume without any schedule option continues the saved one
    _cli(["train", "--max-steps", "2", "--loss-log", log["bare"]] + common + sched, roots["bare"])
    _cli(["train", "--max-steps", "2", "--resume", "--loss-log", log["bare"], "--lr", "1e-3"] + common, roots["bare"])
    assert [rec["lr"] for rec in _log(log["bare"])] == want
    w = {k: torch.load(os.path.join(r, "best_model.pt"), map_location="cpu") for k, r in roots.items()}
    key = "decoder.feed_forward_list.0.fc1.weight"
    for name in ("split", "bare"):
        d = float((w[name][key] - w["full"][key]).abs().mean())
        # (test_resume_*: 2e-7 at lr 1e-4 = 2e-3 of a step; the same fraction of this run's peak rate)
        assert d < 2e-3 * 1e-3, (name, d)


def test_cli_writes_lr_only_with_a_schedule(tmp_path):
    from fira_icse_amd import ops, synth
    recs = {}
    for name, extra in (("sched", ["--lr", "1e-3", "--lr-schedule", "inv-sqrt", "--warmup-steps", "2"]), ("plain", [])):
        root = str(tmp_path / name)
        os.makedirs(root)
        synth.write_dataset(root, util.load_golden_raw())
        log = os.path.join(root, "loss.jsonl")
        r = _cli(["train", "--splits", "16,4,4", "--batch-size", "4", "--dev-from-epoch", "99", "--max-steps", "5", "--loss-log",
                  log] + extra, root)
        recs[name] = _log(log)
        assert ("learning rate:" in r.stdout) == bool(extra) and ("learning-rate schedule:" in r.stdout) == bool(extra)
    assert len(recs["sched"]) == 5 and len(recs["plain"]) == 5
    s = ops.LrSchedule.make(dict(kind="inv_sqrt", base_lr=1e-3, warmup_steps=2))
    for step, rec in enumerate(recs["sched"], 1):
        assert rec["lr"] == ops.lr_at(s, step)
        assert sorted(rec) == ["batch", "epoch", "index", "loss", "lr"]
    assert recs["sched"][1]["lr"] == float(np.float32(1e-3)) > recs["sched"][0]["lr"] and recs["sched"][4]["lr"] < recs["sched"][1]["lr"]
    for rec in recs["plain"]:
        assert sorted(rec) == ["batch", "epoch", "index", "loss"]        # key for key what the log held before schedules existed
