"""What the training entries of the engine refuse (csrc/engine.hip: check_step; the table of step forms in DESIGN.md).

A table of calls through ``_lib.lib()`` on the golden batch, every one with ONE thing wrong.  Each must raise ``_lib.FiraError``
before anything is launched -- the model's scalars, gradient buffer, parameters, moments, row stamps and clip state keep the
sentinels they were given -- and, where the library's message names the entry, it names the entry that was called.  After the
whole table ``Trainer.step`` on the same model still returns a finite loss.

The stream and parameter-buffer checks of fira_train_step_end are not driven here: a test of them would leave a half-run step on
the library's streams.  fira_train_accum_last with a NULL clip state is its unclipped form, not an error, so "state NULL" is a
case of fira_train_step_clip only."""
import ctypes as C
import math
import re

import pytest
import torch

import util
from fira_icse_amd import data
from fira_icse_amd.config import FiraConfig

pytestmark = pytest.mark.gpu

SCHEDULE_TEXT = "cosine needs decay_steps > warmup_steps"        # fira_lr_schedule_check's own message: it names no entry


def test_every_malformed_training_call_is_refused_before_a_launch():
    from fira_icse_amd import _lib, ops
    from fira_icse_amd.model import DeviceBatch, TransModel, reference_init_state_dict
    from fira_icse_amd.train import Trainer
    cfg = FiraConfig()
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = list(data.split_index(*util.GOLDEN_SPLIT, seed=0)["train"][:util.GOLDEN_B])
    torch.manual_seed(0)
    model = TransModel(cfg, init=False)
    model.load_state_dict(util.perturb_state_dict(reference_init_state_dict(cfg), seed=1))
    model.eval()
    db = DeviceBatch(store.batch(idx), cfg)
    model.sync_params()
    db.wait_ready()
    lib, ptr, dev = _lib.lib(), _lib.ptr, model.gbuf.device
    ws = model.workspace(db.B, 1)
    flat = model.flat.data
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    row_step = torch.zeros(2 * cfg.vocab_size, dtype=torch.int32, device=dev)
    state, scratch = ops.clip_state(dev)
    stats = torch.zeros(2, dtype=torch.float32, device=dev)
    total = torch.zeros(1, dtype=torch.int32, device=dev)
    event = torch.cuda.Event()
    event.record()
    ev = C.c_void_p(event.cuda_event)
    stream = _lib.cur_stream()
    # sentinels: the prep launch of a training call zeroes the scalars, opts.zero_grads the gradient buffer
    model.loss_sum.fill_(12345.0)
    model.n_tok.fill_(-7)
    model.gbuf.fill_(1.0)
    state.fill_(3)
    params0 = flat.clone()

    def opts(zero_grads=1):
        return _lib.TrainOpts(0.0, 0.0, 1, 1 if model.compact_head else 0, 0, 1 if model.compact_dec else 0, zero_grads)

    bad_sched = _lib.LrSchedule(2, 1e-3, 8, 8, 0.0)              # cosine with decay_steps == warmup_steps

    def adam(m_=m, v_=v, step=1, sched=None):
        return C.byref(_lib.AdamOpts(1e-3, 0.9, 0.999, 1e-8, step, ptr(m_), ptr(v_), _lib.sched_ptr(sched)))

    def head(o, loss_sum=model.loss_sum, n_tok=model.n_tok):
        return (stream, C.byref(model.dims), C.byref(db.struct), ptr(flat), ptr(model.gbuf), ptr(ws), ws.numel(), C.byref(o),
                ptr(loss_sum), ptr(n_tok))

    off4 = C.c_void_p(scratch.data_ptr() + 4)
    nan = float("nan")
    # every one-call entry that takes Adam options, as a function of (adam, opts): otherwise well-formed
    one_call = {
        "fira_train_step": lambda a, o: lib.fira_train_step(*head(o), a),
        "fira_train_step_rows": lambda a, o: lib.fira_train_step_rows(*head(o), a, ptr(row_step)),
        "fira_train_step_clip": lambda a, o: lib.fira_train_step_clip(*head(o), a, None, 1.0, ptr(state), ptr(scratch)),
        "fira_train_accum_micro": lambda a, o: lib.fira_train_accum_micro(*head(o), a, ptr(row_step)),
        "fira_train_accum_last": lambda a, o: lib.fira_train_accum_last(*head(o), a, None, ptr(stats), ptr(total), 0.0, None, None),
    }
    table = []                                                    # (what is wrong, entry, call, message must match)
    for name, call in one_call.items():
        table += [("moments NULL", name, lambda call=call: call(adam(m_=None, v_=None), opts()), name + ":"),
                  ("step == 0", name, lambda call=call: call(adam(step=0), opts()), name + ":"),
                  ("invalid schedule", name, lambda call=call: call(adam(sched=bad_sched), opts()), SCHEDULE_TEXT)]

    def clip(o, row=None, max_norm=1.0, st=state, sc=ptr(scratch)):
        return lib.fira_train_step_clip(*head(o), adam(), ptr(row), max_norm, ptr(st), sc)

    def last(max_norm=1.0, sc=ptr(scratch), st_=stats, tot=total, **kw):
        return lib.fira_train_accum_last(*head(opts(0), **kw), adam(), None, ptr(st_), ptr(tot), max_norm, ptr(state), sc)

    rows, clp, mic, lst = "fira_train_step_rows", "fira_train_step_clip", "fira_train_accum_micro", "fira_train_accum_last"
    table += [
        ("without zero_grads", rows, lambda: lib.fira_train_step_rows(*head(opts(0)), adam(), ptr(row_step)), rows + ":"),
        ("row_step NULL", rows, lambda: lib.fira_train_step_rows(*head(opts()), adam(), None), rows + ":"),
        ("max_norm 0", clp, lambda: clip(opts(), max_norm=0.0), clp + ":"),
        ("max_norm NaN", clp, lambda: clip(opts(), max_norm=nan), clp + ":"),
        ("state NULL", clp, lambda: clip(opts(), st=None), clp + ":"),
        ("scratch NULL", clp, lambda: clip(opts(), sc=None), clp + ":"),
        ("scratch misaligned by 4 bytes", clp, lambda: clip(opts(), sc=off4), clp + ":"),
        ("row_step without zero_grads", clp, lambda: clip(opts(0), row=row_step), clp + ":"),
        ("adam without row_step", mic, lambda: lib.fira_train_accum_micro(*head(opts()), adam(), None), mic + ":"),
        ("row_step without adam", mic, lambda: lib.fira_train_accum_micro(*head(opts()), None, ptr(row_step)), mic + ":"),
        ("totals NULL", lst, lambda: last(st_=None, tot=None), lst + ":"),
        ("stats aliasing loss_sum", lst, lambda: last(loss_sum=stats), lst + ":"),
        ("total aliasing n_tok", lst, lambda: last(n_tok=total), lst + ":"),
        ("max_norm 0", lst, lambda: last(max_norm=0.0), lst + ":"),
        ("max_norm NaN", lst, lambda: last(max_norm=nan), lst + ":"),
        ("scratch NULL", lst, lambda: last(sc=None), lst + ":"),
        ("scratch misaligned by 4 bytes", lst, lambda: last(sc=off4), lst + ":"),
        ("without mid_event", "fira_train_step_begin", lambda: lib.fira_train_step_begin(*head(opts()), None),
         "fira_train_step_begin:"),
        ("without mid_event", "fira_train_step_begin_rows",
         lambda: lib.fira_train_step_begin_rows(*head(opts()), None, adam(), ptr(row_step)), "fira_train_step_begin_rows:"),
        ("row_step NULL", "fira_train_step_begin_rows",
         lambda: lib.fira_train_step_begin_rows(*head(opts()), ev, adam(), None), "fira_train_step_begin_rows:"),
        ("no step begun", "fira_train_step_end", lambda: lib.fira_train_step_end(stream, ptr(flat), adam(), None, None),
         "fira_train_step_end:"),
        ("adam NULL", "fira_train_step_end_rows",
         lambda: lib.fira_train_step_end_rows(stream, ptr(flat), None, None, None, ptr(row_step)), "fira_train_step_end_rows:"),
    ]
    assert len(table) == 5 * 3 + 22
    wrong = []
    for what, entry, call, pattern in table:
        try:
            _lib.check(call())
        except _lib.FiraError as e:
            if not re.search(re.escape(pattern), str(e)):
                wrong.append("%s, %s: message %r does not contain %r" % (entry, what, str(e), pattern))
        else:
            wrong.append("%s, %s: accepted" % (entry, what))
    assert not wrong, "\n".join(wrong)
    # nothing was launched: every buffer a training call writes first still holds what it held
    torch.cuda.synchronize()
    assert float(model.loss_sum.item()) == 12345.0 and int(model.n_tok.item()) == -7
    assert bool((model.gbuf == 1.0).all()) and torch.equal(flat, params0)
    assert not bool(m.any()) and not bool(v.any()) and not bool(row_step.any())
    assert bool((state == 3).all()) and not bool(stats.any()) and int(total.item()) == 0
    # ... and the library is none the worse for it
    tr = Trainer(model)
    tr.step(db)
    assert math.isfinite(tr.last_loss())
