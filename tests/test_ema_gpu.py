"""Exponential moving average of the weights on the device (csrc/ema.hip, Trainer(ema_decay=...), run_model.py --ema-decay).

The definition is bit-exact -- diff = p - e; e = e + w * diff, every operation rounded to fp32 on its own -- so a numpy float32
loop is the reference and the comparisons are ``==``.  The central claim: under the row-sparse Adam the average is taken over
the parameters as a forward pass sees them (rows that lag read with the zero-gradient updates they owe applied in registers),
which makes it EQUAL to the average a dense Adam gives, without a sync.  As in tests/test_adam_rows_gpu.py the kernels are
compared in isolation on synthetic gradients (the training step around them is not bit-reproducible run to run); the trainer
is then held to the recurrence over its own parameter snapshots."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import util
from fira_icse_amd import data, ops, synth
from fira_icse_amd.config import FiraConfig

pytestmark = pytest.mark.gpu


def ema_ref(e, p, w):
    """The definition, in numpy float32 (every operation rounds to fp32)."""
    w = np.float32(w)
    diff = (p - e).astype(np.float32)
    t = (w * diff).astype(np.float32)
    return (e + t).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. the plain kernel
WEIGHTS = [ops.ema_weight(0.999, 1), ops.ema_weight(0.5, 4), 0.0]


@pytest.mark.parametrize("p_start", [1, 3])                   # p in ema's 16-byte phase (one 16-byte load) / out of it
@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("n", [1, 3, 255, 1029])
def test_plain_kernel_equals_the_numpy_loop(n, w, p_start):
    gen = torch.Generator(device="cuda").manual_seed(1000 * n + p_start)
    ebuf = torch.randn(n + 6, device="cuda", generator=gen)
    pbuf = torch.randn(n + 6, device="cuda", generator=gen)
    e, p = ebuf[1:1 + n], pbuf[p_start:p_start + n]            # 4-byte aligned pointers, guard elements on both sides
    assert e.data_ptr() % 16 == 4 and p.data_ptr() % 16 == 4 * p_start
    e0, p0, eb0, pb0 = e.cpu().numpy().copy(), p.cpu().numpy().copy(), ebuf.clone(), pbuf.clone()
    ops.ema_update(e, p, w)
    assert np.array_equal(e.cpu().numpy().view(np.uint32), ema_ref(e0, p0, w).view(np.uint32))
    assert torch.equal(ebuf[:1], eb0[:1]) and torch.equal(ebuf[1 + n:], eb0[1 + n:])        # the guards
    assert torch.equal(pbuf, pb0)                                                           # p is read only
    if w != 0.0 and n > 1:
        assert not np.array_equal(e.cpu().numpy(), e0)


@pytest.mark.parametrize("n", [1, 255, 1029])
def test_plain_kernel_keeps_the_bits_where_ema_equals_p(n):
    p = torch.randn(n + 2, device="cuda")[1:1 + n]
    e = p.clone()
    e[n // 2:] += 1.0                                           # one half equal, one half not
    e0 = e.clone()
    ops.ema_update(e, p, ops.ema_weight(0.999, 1))
    assert torch.equal(e[:n // 2].view(torch.int32), e0[:n // 2].view(torch.int32))
    assert n < 2 or not torch.equal(e[n // 2:], e0[n // 2:])


def test_plain_kernel_refuses_aliasing_and_bad_weights():
    from fira_icse_amd import _lib
    buf = torch.randn(64, device="cuda")
    b0 = buf.clone()
    for e, p in ((buf[:32], buf[:32]), (buf[:32], buf[16:48]), (buf[16:48], buf[:32])):
        with pytest.raises(_lib.FiraError, match="overlaps"):
            ops.ema_update(e, p, 0.5)
    for w in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(_lib.FiraError, match="outside"):
            ops.ema_update(buf[:32], buf[32:], w)
    torch.cuda.synchronize()
    assert torch.equal(buf, b0)                                 # nothing was launched
    ops.ema_update(buf[:32], buf[32:], 1.0)                     # adjacent ranges are fine; w = 1 copies up to rounding
    assert torch.allclose(buf[:32], buf[32:], rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------------------------ 2. lazy rows
def _tables(model, cfg):
    v = model.named_views()
    base = model.flat.data.data_ptr()
    out = []
    for name in ("decoder.embedding.weight", "encoder.embedding.weight"):
        off = (v[name].data_ptr() - base) // 4
        out.append((off, off + cfg.vocab_size * 256))
    return out


@pytest.mark.parametrize("schedule", ["constant", "inv-sqrt"])
def test_rows_average_equals_dense_average_bit_for_bit(schedule):
    """Dense side: fira_adam_step_mb on both tables, then fira_ema_update.  Row-sparse side: fira_adam_rows_step, then
    fira_ema_update_rows with NO sync and no catch-up in between: rows owe up to 31 steps when the average reads them."""
    from fira_icse_amd import _lib
    from fira_icse_amd.model import TransModel
    cfg = FiraConfig()
    model = TransModel(cfg, device="cuda")
    lib, dims, V = _lib.lib(), model.dims, cfg.vocab_size
    dev = model.flat.data.device
    gen = torch.Generator(device="cuda").manual_seed(7)
    tabs = _tables(model, cfg)
    total = model.flat.data.numel()
    p0 = torch.randn(total, device=dev, generator=gen) * 0.05
    e0 = torch.randn(total, device=dev, generator=gen) * 0.05     # not the parameters: every element of the average moves
    pd, md, vd, ed = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), e0.clone()          # dense side
    pr, mr, vr, er = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), e0.clone()          # row-sparse side
    last = torch.zeros(2 * V, dtype=torch.int32, device=dev)
    g = torch.zeros(total, device=dev)
    n_tok = torch.tensor([37], dtype=torch.int32, device=dev)
    base_lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    sched = None if schedule == "constant" else ops.LrSchedule.make({"kind": "inv-sqrt", "base_lr": base_lr, "warmup_steps": 5}).struct()
    w = ops.ema_weight(0.9, 1)
    s = _lib.cur_stream()
    rates = set()
    for step in range(1, 41):                                    # crosses the every-row step 32
        g.zero_()
        for a, b in tabs:
            rows = torch.nonzero(torch.rand(V, device=dev, generator=gen) < 0.02).flatten()
            g[a:b].view(V, 256)[rows] = torch.randn(rows.numel(), 256, device=dev, generator=gen)
        lr = base_lr if sched is None else ops.lr_at(sched, step)          # the float a dense launch of this step is given
        rates.add(lr)
        for a, b in tabs:
            _lib.check(lib.fira_adam_step_mb(s, b - a, _lib.ptr(pd[a:]), _lib.ptr(g[a:]), None, _lib.ptr(md[a:]), _lib.ptr(vd[a:]),
                                             lr, b1, b2, eps, step, _lib.ptr(n_tok), None))
        ops.ema_update(ed, pd, w)
        ad = _lib.AdamOpts(base_lr, b1, b2, eps, step, _lib.ptr(mr), _lib.ptr(vr), _lib.sched_ptr(sched))
        _lib.check(lib.fira_adam_rows_step(s, C.byref(dims), _lib.ptr(pr), _lib.ptr(g), C.byref(ad), _lib.ptr(last), _lib.ptr(n_tok),
                                           None, 3), "fira_adam_rows_step")
        before = [t.clone() for t in (pr, mr, vr, last)] if step == 31 else None
        _lib.check(lib.fira_ema_update_rows(s, C.byref(dims), _lib.ptr(er), _lib.ptr(pr), C.byref(ad), _lib.ptr(last), w),
                   "fira_ema_update_rows")
        if step == 31:                                           # the kernel writes the average only
            assert int(last.min()) == 0 and int(last.max()) == 31        # rows that owe everything, rows that owe nothing
            for x, y in zip(before, (pr, mr, vr, last)):
                assert torch.equal(x, y)
            for a, b in tabs:                                    # (and the lazy side really is behind the dense one)
                assert not torch.equal(pd[a:b], pr[a:b])
        if step in (1, 2, 31, 32, 33, 40):
            assert torch.equal(ed, er), (step, int((ed != er).sum()))
    assert len(rates) == 1 if sched is None else len(rates) > 30         # the schedule's rates differ step to step: the ring is used
    assert not torch.equal(er, e0)


# ------------------------------------------------------------------------------------------------ 3. the trainer
N_STEPS = 8


def _store_and_batches(cfg, model):
    from fira_icse_amd.model import DeviceBatch
    store = data.process_raw(cfg, synth.generate_dataset(32, seed=11))
    return [DeviceBatch(store.batch(list(range(4 * i, 4 * i + 4))), cfg, model.device_) for i in range(2)]


def _trainer(rows, **kw):
    from fira_icse_amd.model import TransModel
    from fira_icse_amd.train import Trainer
    cfg = FiraConfig()
    os.environ["FIRA_ADAM_ROWS"] = "1" if rows else "0"
    try:
        torch.manual_seed(0)
        model = TransModel(cfg, device="cuda")
        model.eval()                                             # dropout off
        tr = Trainer(model, **kw)
    finally:
        os.environ.pop("FIRA_ADAM_ROWS", None)
    assert (tr.row_step is not None) == rows
    return cfg, model, tr


def _recurrence(e, snaps, w, every):
    """numpy float32 recurrence over the parameter snapshots taken after steps 1, 2, ..."""
    for t, p in enumerate(snaps, start=1):
        if t % every == 0:
            e = ema_ref(e, p, w)
    return e


@pytest.fixture(scope="module")
def dense_tables():
    """The weight average of a DENSE trainer (FIRA_ADAM_ROWS=0, no ema option: the average is formed here, in torch), for both
    cadences, run twice: the distance between the two runs is the yardstick of tests/test_adam_rows_gpu.py."""
    out = []
    for _ in range(2):
        cfg, model, tr = _trainer(False)
        batches = _store_and_batches(cfg, model)
        tabs = _tables(model, cfg)
        emas = {k: model.flat.data.clone() for k in (1, 4)}
        for i in range(N_STEPS):
            tr.step(batches[i % 2])
            for k, e in emas.items():
                if (i + 1) % k == 0:
                    diff = model.flat.data - e
                    e += diff * ops.ema_weight(0.9, k)
        out.append({k: [e[a:b].clone() for a, b in tabs] for k, e in emas.items()})
        del model, tr, emas
    return out


@pytest.mark.parametrize("every", [1, 4])
def test_trainer_average_obeys_the_recurrence(every, dense_tables):
    w = ops.ema_weight(0.9, every)
    # run A: a snapshot of the synced parameters after every step.  The average was updated inside step(), BEFORE the sync, from
    # rows that still owed updates: it must equal the recurrence over what the sync then wrote.
    cfg, model, tr = _trainer(True, ema_decay=0.9, ema_every=every)
    batches = _store_and_batches(cfg, model)
    e_start = tr.ema.cpu().numpy().copy()
    assert np.array_equal(e_start, model.flat.data.cpu().numpy())
    snaps, lagged = [], False
    for i in range(N_STEPS):
        tr.step(batches[i % 2])
        lagged = lagged or int(tr.row_step.min()) < tr.t
        tr.sync()
        snaps.append(model.flat.data.cpu().numpy().copy())
    assert lagged and tr.ema_updates == N_STEPS // every
    want = _recurrence(e_start, snaps, w, every)
    got = tr.ema.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    live = model.layout.live
    assert np.array_equal(got[live:], e_start[live:]) and not np.array_equal(got[:live], e_start[:live])
    del model, tr, snaps

    # run B: no sync between the steps, the rows stay lazy throughout (raw copies of the flat buffer: its non-table part is
    # always current).  Non-table part: the same recurrence, ==.  Table part: the average of a dense trainer on the same batches.
    cfg, model, tr = _trainer(True, ema_decay=0.9, ema_every=every)
    batches = _store_and_batches(cfg, model)
    tabs = _tables(model, cfg)
    e_start = tr.ema.cpu().numpy().copy()
    snaps = []
    for i in range(N_STEPS):
        tr.step(batches[i % 2])
        snaps.append(model.flat.data.clone())                    # (no sync_params: the raw buffer)
    assert int(tr.row_step.min()) < N_STEPS                      # rows no batch touched are still behind
    want = _recurrence(e_start, [x.cpu().numpy() for x in snaps], w, every)
    got = tr.ema.cpu().numpy()
    mask = np.ones(got.size, dtype=bool)
    for a, b in tabs:
        mask[a:b] = False
    assert np.array_equal(got[mask].view(np.uint32), want[mask].view(np.uint32))
    for k, (a, b) in enumerate(tabs):
        d1, d2 = dense_tables[0][every][k], dense_tables[1][every][k]
        diff = float((tr.ema[a:b] - d1).abs().max())
        noise = float((d2 - d1).abs().max())
        print("every %d table %d: |rows - dense| %.3g  |dense2 - dense| %.3g" % (every, k, diff, noise))
        assert diff < 6 * noise + 2 * cfg.lr, (k, diff, noise)


def test_averaged_context_and_state_round_trip():
    from fira_icse_amd.train import Trainer
    cfg, model, tr = _trainer(True, ema_decay=0.9, ema_every=1)
    batches = _store_and_batches(cfg, model)
    for i in range(3):
        tr.step(batches[i % 2])
    tr.sync()
    raw = model.flat.data.clone()
    assert not torch.equal(raw, tr.ema)
    with tr.averaged() as m:
        assert m is model
        views = model.layout.views(tr.ema)
        sd = model.state_dict()
        assert list(sd) == list(views)
        for name, t in sd.items():
            assert torch.equal(t, views[name]), name
        assert torch.equal(model.flat.data, tr.ema)
        with pytest.raises(RuntimeError, match="nest"):
            with tr.averaged():
                pass
        with pytest.raises(RuntimeError, match="averaged"):
            tr.step(batches[0])
        inside = tr.state_dict()                                 # "params" are the RAW parameters also in here
        assert torch.equal(inside["params"], raw) and torch.equal(inside["ema"], tr.ema)
        model.forward_dev(batches[0])                            # a dev pass on the averaged weights runs
    assert torch.equal(model.flat.data.view(torch.int32), raw.view(torch.int32))          # the raw bits are back
    state = dict(tr.state_dict())
    state["m"], state["v"] = state["m"].clone(), state["v"].clone()         # (the moments are handed out by reference)
    assert state["ema_cfg"] == {"decay": 0.9, "every": 1} and int(state["t"]) == 3
    assert torch.equal(state["params"], raw) and torch.equal(state["ema"], tr.ema)
    ema3 = tr.ema.clone()
    tr.step(batches[1])                                          # a further step works, and moves the average
    assert tr.t == 4 and not torch.equal(tr.ema, ema3)
    # round trip into a fresh trainer of a fresh model
    cfg2, model2, tr2 = _trainer(True, ema_decay=0.9, ema_every=1)
    tr2.load_state_dict(state)
    assert tr2.t == 3 and tr2.ema_updates == 3
    assert torch.equal(tr2.ema, ema3) and torch.equal(model2.flat.data, raw) and torch.equal(tr2.m, state["m"])
    tr2.step(batches[1])
    assert tr2.t == 4
    # another (decay, every) is refused, by decay and by cadence
    for kw in ({"ema_decay": 0.8, "ema_every": 1}, {"ema_decay": 0.9, "ema_every": 4}):
        tr3 = Trainer(model2, **kw)
        with pytest.raises(ValueError, match="decay, every"):
            tr3.load_state_dict(state)
    # a state without the keys: the average starts from the (loaded) parameters; a trainer without the option ignores the keys
    plain = {k: v for k, v in state.items() if k not in ("ema", "ema_cfg", "params")}
    tr4 = Trainer(model2, ema_decay=0.9, ema_every=4)
    tr4.ema.zero_()
    tr4.load_state_dict(plain)
    model2.sync_params()
    assert torch.equal(tr4.ema, model2.flat.data) and tr4.ema_updates == 0
    tr5 = Trainer(model2)
    assert tr5.ema is None
    tr5.load_state_dict(state)
    assert tr5.t == 3 and "ema" not in tr5.state_dict()
    with pytest.raises(RuntimeError, match="without ema_decay"):
        with tr5.averaged():
            pass
    for kw in ({"ema_decay": 0.0}, {"ema_decay": 1.0}, {"ema_decay": 0.9, "ema_every": 0}):
        with pytest.raises(ValueError):
            Trainer(model2, **kw)


# ------------------------------------------------------------------------------------------------ 4. replicas
def _rank(rank, world, port, out, zero1):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, util.REPO)
    from fira_icse_amd.model import TransModel, DeviceBatch, reference_init_state_dict
    from fira_icse_amd.train import Trainer
    from fira_icse_amd.parallel import shard_indices
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = FiraConfig()
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = data.split_index(*util.GOLDEN_SPLIT, seed=0)["train"]
    torch.manual_seed(0)
    model = TransModel(cfg, init=False)
    model.load_state_dict(util.perturb_state_dict(reference_init_state_dict(cfg), seed=1))
    model.eval()
    trainer = Trainer(model, distributed=True, zero1=zero1, ema_decay=0.9, ema_every=1)
    assert (trainer.row_step is None) == zero1
    e = trainer.ema.cpu().numpy().copy()
    w = ops.ema_weight(0.9, 1)
    for i in range(3):
        mine = shard_indices(idx[4 * i:4 * i + 4], rank, world)
        trainer.step(DeviceBatch(store.batch(mine), cfg))
        trainer.sync()                                           # (after the average was updated from the lazy rows)
        e = ema_ref(e, model.flat.data.cpu().numpy(), w)         # this rank's own parameter snapshot
    got = trainer.ema.cpu().numpy()
    ok = bool(np.array_equal(got.view(np.uint32), e.view(np.uint32)))
    torch.save({"ema": trainer.ema.cpu(), "flat": model.flat.data.cpu(), "ok": ok, "updates": trainer.ema_updates},
               "%s.%d" % (out, rank))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("zero1", [False, True])
def test_two_ranks_keep_identical_averages(tmp_path, zero1):
    out = str(tmp_path / "ema.pt")
    port = 30200 + (os.getpid() % 150) + (200 if zero1 else 0)
    mp.spawn(_rank, args=(2, port, out, zero1), nprocs=2, join=True)
    r = [torch.load("%s.%d" % (out, k), weights_only=False) for k in (0, 1)]
    assert r[0]["ok"] and r[1]["ok"]                             # each rank: the recurrence over its own snapshots, ==
    assert r[0]["updates"] == r[1]["updates"] == 3
    assert torch.equal(r[0]["flat"], r[1]["flat"])
    assert torch.equal(r[0]["ema"], r[1]["ema"])
    assert not torch.equal(r[0]["ema"], r[0]["flat"])


# ------------------------------------------------------------------------------------------------ 5. the command line
def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=util.REPO)
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "run_model.py")] + args, cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_cli_saves_the_averaged_model_and_resumes_from_the_raw_one(tmp_path):
    from fira_icse_amd.model import ParamLayout
    common = ["--splits", "16,4,4", "--batch-size", "4", "--dev-from-epoch", "99", "--no-dropout", "--save-optimizer"]
    ema = ["--ema-decay", "0.5", "--ema-every", "1"]
    root = str(tmp_path / "ema")
    os.makedirs(root)
    synth.write_dataset(root, util.load_golden_raw())
    out = _cli(["train", "--max-steps", "3"] + ema + common, root)
    assert "weight-average (EMA) updates so far: 3" in out
    entries = ParamLayout(FiraConfig()).entries

    def check_files(t):
        sd = torch.load(os.path.join(root, "best_model.pt"), map_location="cpu")
        st = torch.load(os.path.join(root, "fira_train_state.pt"), map_location="cpu")
        assert int(st["t"]) == t and st["ema_cfg"] == {"decay": 0.5, "every": 1}
        assert len(sd) == len(entries) == 338
        differs = False
        for name, (off, shape) in entries.items():
            n = int(np.prod(shape))
            assert torch.equal(sd[name], st["ema"][off:off + n].view(shape)), name         # the file holds the averaged model
            differs = differs or not torch.equal(sd[name], st["params"][off:off + n].view(shape))
        assert differs                                           # ... which is not the raw one
        return st

    st3 = check_files(3)
    _cli(["train", "--max-steps", "2", "--resume"] + ema + common, root)
    st5 = check_files(5)
    assert not torch.equal(st5["ema"], st3["ema"]) and not torch.equal(st5["params"], st3["params"])
    _cli(["test", "--splits", "16,4,4", "--test-batch-size", "3", "--beam", "1"], root)
    lines = open(os.path.join(root, "OUTPUT", "output_fira")).read().split("\n")
    assert len(lines) == 5 and lines[-1] == ""
    # without the option: no new key in the state
    root2 = str(tmp_path / "plain")
    os.makedirs(root2)
    synth.write_dataset(root2, util.load_golden_raw())
    out = _cli(["train", "--max-steps", "3"] + common, root2)
    assert "EMA" not in out
    st = torch.load(os.path.join(root2, "fira_train_state.pt"), map_location="cpu")
    assert int(st["t"]) == 3 and not {"ema", "ema_cfg", "params"} & set(st)
