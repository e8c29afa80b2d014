"""Native training step (reference run_model.py:101-112) on the HIP engine: no autograd, no per-tensor optimizer.

    fwd+bwd (one C call, whole step enqueued on the stream)  ->  [RCCL all-reduce]  ->  fused Adam over the flat buffer

The 1/n_tok normaliser stays on the device (no ``loss.item()`` sync per step; the reference syncs every step at
run_model.py:112); ``last_loss()`` reads it back only when asked.
"""
from __future__ import annotations

import contextlib
import os
from typing import Optional

import torch

from . import _lib, ops
from .model import DeviceBatch, TransModel
from .parallel import GradReducer, ShardedOptimizerComm


class Trainer:
    def __init__(self, model: TransModel, lr: Optional[float] = None, betas=(0.9, 0.999), eps: float = 1e-8,
                 distributed: bool = False, zero1: bool = False, grad_wire: str = "f32",
                 clip_grad_norm: Optional[float] = None, lr_schedule=None, ema_decay: Optional[float] = None,
                 ema_every: int = 32, accum_steps: Optional[int] = None):
        """``zero1`` (with ``distributed``): reduce-scatter + Adam on the owned 1/world shard + all-gather instead of
        all-reduce + replicated Adam; Adam moments exist only for the owned shard (parallel.ShardedOptimizerComm).
        ``grad_wire`` (with ``distributed``, all-reduce path): "f32", or "bf16" = the two gradient buckets travel as bf16
        (half the bytes on xGMI; parallel.GradReducer).
        ``clip_grad_norm`` (``None`` = off: the code path of every release so far): the gradient is clipped to this global norm
        on the device (``torch.nn.utils.clip_grad_norm_``; ``inf`` = observe and guard only) and a step whose gradient holds
        an ``inf`` / ``nan`` is applied as a zero-gradient step instead of destroying the weights; see :meth:`last_grad_norm`.
        ``lr_schedule`` (``None`` = the constant ``lr``: the code path of every release so far): an ``ops.LrSchedule`` or a
        dict of its fields -- warmup and decay as a function of the step number (``ops.lr_at``).  ``lr`` is then not used.
        The row-sparse update stays lazy under it: the rate of every step a row still owes travels with the launch.
        ``ema_decay`` (``None`` = off: no buffer, no launch, the code path of every release so far): a per-step decay
        ``0 < D < 1`` of an exponential moving average of the weights, ``self.ema`` (flat, like ``model.flat``; one full copy
        on every rank, also with ``zero1``).  It starts as a copy of the parameters -- no warm-up of the decay and no bias
        correction -- and after every ``ema_every``-th step (K, default 32: the cadence at which the row-sparse update has
        just written every row) moves toward them by ``w = ops.ema_weight(D, K) = float32(1 - D**K)``:
        ``e += w * (p - e)``, each operation rounded to fp32 on its own.  Embedding rows the row-sparse Adam still owes updates
        are read as the forward pass reads them (fira_ema_update_rows): nothing is synced.  See :meth:`averaged`.
        ``accum_steps`` (``None`` = 1): how many micro-batches the command line cuts a rank's shard of the global batch into
        (``ops.accum_check``); kept for the caller only -- :meth:`step_many` takes a sequence of any length and :meth:`step`
        never looks at it."""
        self.accum_steps = ops.accum_check(accum_steps)
        self._acc_last = False                                   # the last step was accumulated: last_loss reads self.stats
        self.ema = None
        self.ema_cfg = None
        self.ema_updates = 0                                     # updates behind self.ema (a loaded state: t // K)
        self._raw = None                                         # the raw parameters while averaged() holds the model
        if ema_decay is not None:
            self.ema_cfg = ops.ema_check(ema_decay, ema_every)
            self._ema_w = ops.ema_weight(*self.ema_cfg)
        self.lr_schedule = None if lr_schedule is None else ops.LrSchedule.make(lr_schedule)
        self._last_lr = None
        self._sched_cache = (None, None)
        self.clip = None
        if clip_grad_norm is not None:
            self.clip = float(clip_grad_norm)
            if not self.clip > 0:                                # (also refuses nan)
                raise ValueError("clip_grad_norm must be > 0 (inf allowed), not %r" % (clip_grad_norm,))
            self.clip_state, self.clip_scratch = ops.clip_state(model.gbuf.device)
        self.model = model
        self.lr = model.cfg.lr if lr is None else lr
        self.betas, self.eps = betas, eps
        self.zero = ShardedOptimizerComm(model.layout.split, model.layout.live, model.layout.total) \
            if (distributed and zero1) else None
        if self.zero is None:
            self.m = torch.zeros_like(model.gbuf)
            self.v = torch.zeros_like(model.gbuf)
        else:
            dev = model.gbuf.device
            chunks = [q["chunk"] for q in self.zero.buckets]
            self.m_sh = [torch.zeros(c, dtype=torch.float32, device=dev) for c in chunks]
            self.v_sh = [torch.zeros(c, dtype=torch.float32, device=dev) for c in chunks]
            self.g_sh = [torch.zeros(c, dtype=torch.float32, device=dev) for c in chunks]
            self.zstream = torch.cuda.Stream()
            self.end_event = torch.cuda.Event()
        # one library call per step (fira_train_step: the head + decoder slice of the update beside the last weight gradients;
        # round 5: +0.9 % against fira_train_fwd_bwd + one Adam launch over [0, live), identical results)
        self.fused_step = not distributed
        # data parallel (round 6): the same schedule as two calls with the collectives in between (fira_train_step_begin / _end:
        # Adam of [0, split) inside the library, beside its last weight gradients, behind the early bucket's event).  ZeRO-1
        # keeps fira_train_fwd_bwd: its optimizer runs on the owned shards after the reduce-scatter.
        self.fused_dp = distributed and not zero1
        self.t = 0
        # row-sparse Adam of the two vocabulary-sized embedding tables (fira_train_step_rows, round 6): the rows a batch did
        # not touch are updated lazily, bit for bit (include/fira_hip.h); FIRA_ADAM_ROWS=0 = every row every step (A/B switch).
        # The model calls self.sync before anything but this trainer's step reads the parameters.
        self.row_step = None
        self._rows_dirty = False
        self._rows_hyper = None
        if (self.fused_step or self.fused_dp) and os.environ.get("FIRA_ADAM_ROWS", "1") != "0" \
                and model.cfg.embedding_dim == 256:
            model.sync_params()                                  # (an earlier trainer of this model may still owe rows)
            self.row_step = torch.zeros(2 * model.cfg.vocab_size, dtype=torch.int32, device=model.gbuf.device)
            model._rows_sync = self.sync
        if self.ema_cfg is not None:
            model.sync_params()
            self.ema = model.flat.data.clone()
        self.inv = torch.zeros(1, dtype=torch.float32, device=model.gbuf.device)
        self.stats = torch.zeros(2, dtype=torch.float32, device=model.gbuf.device)
        self.n_tok_total = torch.zeros(1, dtype=torch.int32, device=model.gbuf.device)   # step_many: the exact int32 behind stats[1]
        self.reducer = GradReducer(model.layout.split, model.layout.live, wire=grad_wire) if distributed else None
        self.mid_event = None
        if distributed:
            # fires inside the backward pass when the gradients of [0, split) (head + decoder) are final: their all-reduce
            # then runs beside the encoder's backward pass
            self.mid_event = torch.cuda.Event()
            self.mid_event.record()            # torch creates the hipEvent lazily: force it so its handle can be passed

    def step(self, db: Optional[DeviceBatch]):
        """One optimisation step (:meth:`_step`), then -- with ``ema_decay`` -- the update of the weight average, on every path
        that advanced ``self.t`` (also on a rank with an empty shard that took part in the collectives; not where nothing was
        applied).  Every branch of ``_step`` returns with all parameters final on the caller's stream."""
        if self._raw is not None:
            raise RuntimeError("Trainer.step inside Trainer.averaged(): the model holds the averaged weights")
        t = self.t
        self._step(db)
        if self.ema is not None and self.t != t:
            self._ema_update()

    def step_many(self, dbs):
        """ONE optimisation step over the micro-batches ``dbs`` (a non-empty sequence of ``DeviceBatch`` or ``None``): the
        gradient of the loss SUM is accumulated over them on the device and the update is normalised by the sum of their token
        counts -- the step of their concatenation, in the memory of the largest of them.  ``self.t``, the learning-rate
        schedule, the EMA cadence, the clip counters and the ``row_step`` stamps advance by one; the dropout masks are drawn per
        micro-batch (``model.dropout_step`` advances with every pass).  ``None`` entries (empty micro-batches) are skipped;
        with one entry left this IS :meth:`step` -- the same library calls -- and with none it is ``step(None)``.  On the
        data-parallel paths only the last micro-batch meets the collectives, which carry the accumulated gradient and stats."""
        dbs = list(dbs)
        if not dbs:
            raise ValueError("Trainer.step_many: needs at least one micro-batch (None = an empty one)")
        live = [db for db in dbs if db is not None]
        if len(live) <= 1:
            return self.step(live[0] if live else None)
        if self._raw is not None:
            raise RuntimeError("Trainer.step_many inside Trainer.averaged(): the model holds the averaged weights")
        self._step_accum(live)
        if self.ema is not None:
            self._ema_update()

    def _step_accum(self, live):
        """:meth:`step_many` with two or more non-empty micro-batches: K - 1 passes that only add to ``model.gbuf`` and to the
        stats pair (fira_train_accum_micro / fira_accum_stats, no collective), then the last one on the schedule :meth:`_step`
        runs its only one on."""
        m = self.model
        dp = self.reducer is not None and self.reducer.world > 1
        zero_dp = self.zero is not None and self.zero.world > 1
        self._rows_check_hyper()
        sched = self._sched_struct()
        b1, b2 = self.betas
        step = self.t + 1
        one_call = self.fused_step and self.reducer is None and self.zero is None
        fused_dp = dp and self.fused_dp and self.zero is None
        rows = None
        if self.row_step is not None and (one_call or fused_dp):
            rows = (self.m, self.v, self._rate_of(step), step, b1, b2, self.eps, self.row_step)
        for k, db in enumerate(live[:-1]):
            if one_call or fused_dp:
                loss_sum, n_tok = m.train_accum_micro(db, zero_grad=(k == 0), rows=rows, sched=sched)
            else:
                loss_sum, n_tok = m.train_fwd_bwd(db, zero_grad=(k == 0))
            ops.accum_stats(loss_sum, n_tok, self.stats, self.n_tok_total, k == 0)
        db = live[-1]
        self._acc_last = True
        if one_call:
            self.t += 1
            clip = None if self.clip is None else (self.clip, self.clip_state, self.clip_scratch)
            m.train_accum_last(db, self.m, self.v, self._rate(), self.t, self.stats, self.n_tok_total, beta1=b1, beta2=b2,
                               eps=self.eps, row_step=self.row_step, clip=clip, sched=sched)
            self._rows_dirty = self.row_step is not None
            return
        if fused_dp:
            loss_sum, n_tok = m.train_step_begin(db, self.mid_event, rows=rows, sched=sched, zero_grad=False)
        else:
            loss_sum, n_tok = m.train_fwd_bwd(db, zero_grad=False, mid_event=self.mid_event)
            if zero_dp or not dp:                                # (all-reduce data parallel: the reducer adds it on its stream)
                ops.accum_stats(loss_sum, n_tok, self.stats, self.n_tok_total, False)
        self._apply(loss_sum, n_tok, dp, fused_dp, acc=True)

    def _ema_update(self):
        """``self.ema`` toward the parameters as they stand after step ``self.t``, if that step is on the cadence.  One launch on
        the caller's stream, no synchronisation: with rows still owed, the rows entry applies what they owe in registers, under
        the hyper-parameters the updates were deferred under (``_rows_check_hyper`` settles the rows before those change)."""
        if self.t % self.ema_cfg[1]:
            return
        m = self.model
        if self.row_step is not None and self._rows_dirty:
            import ctypes as C
            schedule, lr, b1, b2, eps = self._rows_hyper
            adam = _lib.AdamOpts(lr if schedule is None else schedule.base_lr, b1, b2, eps, int(self.t), _lib.ptr(self.m),
                                 _lib.ptr(self.v), _lib.sched_ptr(self._sched_struct()))
            _lib.check(_lib.lib().fira_ema_update_rows(_lib.cur_stream(), C.byref(m.dims), _lib.ptr(self.ema),
                                                       _lib.ptr(m.flat.data), C.byref(adam), _lib.ptr(self.row_step),
                                                       self._ema_w), "fira_ema_update_rows")
        else:
            ops.ema_update(self.ema, m.flat.data, self._ema_w)
        self.ema_updates += 1

    @contextlib.contextmanager
    def averaged(self):
        """Inside the context the model holds the averaged weights (dev pass, checkpoint, search); on exit the raw parameters
        are back bit for bit.  A phase change, not a per-step call: it syncs the rows (:meth:`sync`) and copies the flat buffer
        twice.  The averaged weights are written INTO ``model.flat`` -- the address every captured search graph has baked in --
        and the library forms its derived weights (folded GCN weights, planes, bf16 shadows) from the parameters inside every
        call, so nothing is left to invalidate.  Not re-entrant; :meth:`step` and :meth:`load_state_dict` inside it raise."""
        if self.ema is None:
            raise RuntimeError("Trainer.averaged: this Trainer was built without ema_decay")
        if self._raw is not None:
            raise RuntimeError("Trainer.averaged: already inside the context (it does not nest)")
        self.sync()
        flat = self.model.flat.data
        self._raw = flat.clone()
        flat.copy_(self.ema)
        try:
            yield self.model
        finally:
            flat.copy_(self._raw)
            self._raw = None

    def _step(self, db: Optional[DeviceBatch]):
        """One optimisation step on this rank's shard of the global batch.

        ``db is None`` = this rank's shard of the global batch is empty (``shard_range`` chunks like
        ``DataParallel.scatter``: the tail batch of an epoch can leave trailing ranks without commits).  Such a rank
        still joins every collective of the step with a zero gradient and zero (loss_sum, n_tok) and applies the same
        Adam update as the others, so the replicas stay identical and nobody waits for a peer that never arrives."""
        m = self.model
        dp = self.reducer is not None and self.reducer.world > 1
        fused_dp = False
        self._acc_last = False
        # once per step, before t advances -- also on a rank whose shard is empty: a sync that a changed hyper-parameter forces
        # brings the rows up to the LAST completed step
        self._rows_check_hyper()
        sched = self._sched_struct()
        if db is None:
            if not dp and not (self.zero is not None and self.zero.world > 1):
                return                                           # nothing to learn from, nobody to keep in step
            m.gbuf[:m.layout.live].zero_()
            m.loss_sum.zero_()
            m.n_tok.zero_()
            self.mid_event.record()
            loss_sum, n_tok = m.loss_sum, m.n_tok
        elif self.fused_step and self.reducer is None and self.zero is None:
            self.t += 1
            clip = None if self.clip is None else (self.clip, self.clip_state, self.clip_scratch)
            m.train_step(db, self.m, self.v, self._rate(), self.t, self.betas[0], self.betas[1], self.eps,
                         row_step=self.row_step, clip=clip, sched=sched)
            self._rows_dirty = self.row_step is not None
            return
        elif dp and self.fused_dp and self.zero is None:
            fused_dp = True
            rows = None if self.row_step is None else \
                (self.m, self.v, self._rate_of(self.t + 1), self.t + 1, self.betas[0], self.betas[1], self.eps, self.row_step)
            loss_sum, n_tok = m.train_step_begin(db, self.mid_event, rows=rows, sched=sched)
        else:
            loss_sum, n_tok = m.train_fwd_bwd(db, zero_grad=True, mid_event=self.mid_event)
        self._apply(loss_sum, n_tok, dp, fused_dp)

    def _apply(self, loss_sum, n_tok, dp: bool, fused_dp: bool, acc: bool = False):
        """The collectives and the update behind a backward pass that left the (rank's) loss-sum gradient in ``model.gbuf``.
        ``acc`` (:meth:`step_many`): ``loss_sum`` / ``n_tok`` are the LAST micro-batch's and ``self.stats`` /
        ``self.n_tok_total`` hold the pair accumulated over the ones before it -- every micro-batch's on the paths whose last
        one ran through ``train_fwd_bwd`` (ZeRO-1, one device without the one-call step)."""
        m = self.model
        b1, b2 = self.betas
        sched = self._sched_struct()
        if self.zero is not None and self.zero.world > 1:
            self._step_zero1(loss_sum, n_tok, packed=acc)
            return
        if dp:
            red, split, live = self.reducer, m.layout.split, m.layout.live
            # stats pair + head/decoder bucket on the communication stream behind the mid-backward event (beside the encoder's
            # backward pass).  One launch packs {loss_sum, float(n_tok)} (exact below 2^24 tokens); the update kernels form
            # 1 / max(count, 1) from the all-reduced pair themselves: no torch arithmetic between the collective and Adam
            # (accumulating: the same launch slot adds the last micro-batch to the pair of the earlier ones instead)
            pack = (lambda: ops.accum_stats(loss_sum, n_tok, self.stats, self.n_tok_total, False)) if acc else \
                (lambda: ops.pack_stats(loss_sum, n_tok, self.stats))
            ev = red.reduce_early(m.gbuf, self.stats, self.mid_event, pack=pack)
            self.t += 1
            lr = self._rate()
            count = self.stats[1:2]
            if self.clip is not None:
                # clipped: every update waits for the norm of the ALL-REDUCED gradient (every rank sums the same numbers, bf16
                # wire included, and takes the same decision).  The encoder's backward pass runs without an update; the sum
                # of squares of each bucket follows its all-reduce, the closing step uses the global token count.
                if fused_dp:
                    m.train_step_end(self.m, self.v, lr, self.t, update=False)
                red.wait_early()
                ops.grad_sqsum(m.gbuf[:split], self.clip_state, 0, self.clip_scratch)
                red.start_late(m.gbuf)
                red.wait_late(m.gbuf)
                ops.grad_sqsum(m.gbuf[split:live], self.clip_state, 1, self.clip_scratch)
                ops.clip_finish(self.clip_state, 2, self.clip, count=count)
                self._adam_slice(0, split, count, table=0)
                self._adam_slice(split, live, count, table=1)
                self._rows_dirty = self.row_step is not None
                return
            if fused_dp:
                # encoder backward; Adam of [0, split) inside the library as soon as the caller's stream has passed the
                # encoder's chain and `ev`, beside the last weight gradients; the join
                m.train_step_end(self.m, self.v, lr, self.t, early_event=ev, count=count, beta1=b1, beta2=b2, eps=self.eps,
                                 row_step=self.row_step, sched=sched)
            else:
                red.wait_early()
                self._adam_slice(0, split, count, table=0)
            red.start_late(m.gbuf)
            red.wait_late(m.gbuf)
            self._adam_slice(split, live, count, table=1)
            self._rows_dirty = self.row_step is not None
            return
        self.t += 1
        # [live, total) holds the tensors no kernel touches (encoder.lstm, combination_list1, gate_fc): their gradient is
        # None in the reference, so torch.optim.Adam skips them too.  1 / n_tok (run_model.py:105) is formed inside the
        # Adam kernel from the device counter (no separate launch, no host sync).
        # One launch over [0, live).  (Running the head+decoder slice on its own stream beside the encoder's backward pass
        # was measured on one box: 8 497 vs 8 553 commits/s -- the HBM-bound update only slows the backward kernels it
        # overlaps; profiles/r2_probes.md.)
        n = m.layout.live
        lr = self._rate()
        if acc:
            count = self.stats[1:2]                              # (every micro-batch is in the pair: _step_accum)
            if self.clip is not None:
                ops.grad_sqsum(m.gbuf[:n], self.clip_state, 0, self.clip_scratch)
                ops.clip_finish(self.clip_state, 1, self.clip, count=count)
                ops.adam_step_clip(m.flat.data[:n], m.gbuf[:n], self.m[:n], self.v[:n], lr, self.t, self.clip_state,
                                   count=count, beta1=b1, beta2=b2, eps=self.eps)
                return
            ops.adam_step_count(m.flat.data[:n], m.gbuf[:n], self.m[:n], self.v[:n], lr, self.t, count, b1, b2, self.eps)
            return
        if self.clip is not None:
            ops.grad_sqsum(m.gbuf[:n], self.clip_state, 0, self.clip_scratch)
            ops.clip_finish(self.clip_state, 1, self.clip, n_tok=n_tok)
            ops.adam_step_clip(m.flat.data[:n], m.gbuf[:n], self.m[:n], self.v[:n], lr, self.t, self.clip_state,
                               n_tok=n_tok, beta1=b1, beta2=b2, eps=self.eps)
            return
        ops.adam_step_mb(m.flat.data[:n], m.gbuf[:n], None, self.m[:n], self.v[:n], lr, self.t, n_tok, None, b1, b2,
                         self.eps)

    def _step_zero1(self, loss_sum, n_tok, packed: bool = False):
        """reduce-scatter -> Adam on the owned shard -> all-gather, per readiness bucket, on a side stream: the head+decoder
        bucket's reduce-scatter starts at the mid-backward event, beside the encoder's backward pass.  ``packed``:
        ``self.stats`` already holds this rank's pair (accumulated over the step's micro-batches)."""
        m, z, zs = self.model, self.zero, self.zstream
        b1, b2 = self.betas
        main = torch.cuda.current_stream()
        zs.wait_event(self.mid_event)
        with torch.cuda.stream(zs):
            z.reduce_scatter(0, m.gbuf, self.g_sh[0])
        if not packed:
            ops.pack_stats(loss_sum, n_tok, self.stats)       # {loss_sum, float(n_tok)}: exact below 2^24 tokens
        torch.distributed.all_reduce(self.stats, op=torch.distributed.ReduceOp.SUM, group=z.group)
        self.end_event.record(main)                            # backward pass done, global token count known
        self.t += 1
        lr = self._rate()
        zs.wait_event(self.end_event)
        if self.clip is not None:
            # clipped: each rank sums the squares of its owned shards, one extra all-reduce of the two scalars gives every
            # rank the same global sums (a rank with an empty shard contributes zeros), then the clipped update on the shards
            with torch.cuda.stream(zs):
                for b in (0, 1):
                    if b == 1:
                        z.reduce_scatter(1, m.gbuf, self.g_sh[1])
                    lo, hi = z.owned(b)
                    ops.grad_sqsum(self.g_sh[b][:hi - lo], self.clip_state, b, self.clip_scratch)
                sq = self.clip_state.view(torch.float32)[0:2]
                torch.distributed.all_reduce(sq, op=torch.distributed.ReduceOp.SUM, group=z.group)
                ops.clip_finish(self.clip_state, 2, self.clip, count=self.stats[1:2])
                for b in (0, 1):
                    lo, hi = z.owned(b)
                    if hi > lo:
                        n = hi - lo
                        ops.adam_step_clip(m.flat.data[lo:hi], self.g_sh[b][:n], self.m_sh[b][:n], self.v_sh[b][:n], lr,
                                           self.t, self.clip_state, count=self.stats[1:2], beta1=b1, beta2=b2, eps=self.eps)
                    z.all_gather(b, m.flat.data)
            main.wait_stream(zs)
            return
        with torch.cuda.stream(zs):
            for b in (0, 1):
                if b == 1:
                    z.reduce_scatter(1, m.gbuf, self.g_sh[1])
                lo, hi = z.owned(b)
                if hi > lo:
                    n = hi - lo
                    ops.adam_step_count(m.flat.data[lo:hi], self.g_sh[b][:n], self.m_sh[b][:n], self.v_sh[b][:n], lr,
                                        self.t, self.stats[1:2], b1, b2, self.eps)
                z.all_gather(b, m.flat.data)
        main.wait_stream(zs)                                   # the next forward pass reads every parameter

    def _rows_check_hyper(self):
        # lazily applied updates use each step's own rate (the schedule's, or the constant lr) and the beta / eps in force: a
        # change of the schedule, of beta or eps -- or, without a schedule, of lr -- first settles what the rows owe
        hyper = (self.lr_schedule, None if self.lr_schedule is not None else self.lr, self.betas[0], self.betas[1], self.eps)
        if self._rows_hyper != hyper:
            self.sync()
            self._rows_hyper = hyper

    def _sched_struct(self):
        """The ``fira_lr_schedule`` of this trainer's schedule (``None`` without one), built once per schedule."""
        if self.lr_schedule is None:
            return None
        if self._sched_cache[0] is not self.lr_schedule:
            self._sched_cache = (self.lr_schedule, self.lr_schedule.struct())
        return self._sched_cache[1]

    def _rate_of(self, t: int) -> float:
        return self.lr if self.lr_schedule is None else ops.lr_at(self._sched_struct(), t)

    def _rate(self) -> float:
        """The rate of step ``self.t`` (already advanced): what every update launch of this step is given."""
        self._last_lr = self._rate_of(self.t)
        return self._last_lr

    def last_lr(self) -> Optional[float]:
        """The learning rate the last step used (``None`` before the first step).  No synchronisation."""
        return self._last_lr

    def _adam_slice(self, lo: int, hi: int, count, table: int):
        """Adam on ``[lo, hi)`` of the flat buffers, scaled by ``1 / count`` (data-parallel step).  On the row-sparse path the
        vocabulary-sized table at the head of the slice (``table`` 0: decoder.embedding at 0, 1: encoder.embedding at
        ``split``) is updated on the rows of the all-reduced gradient that are not zero (fira_adam_rows_step)."""
        m = self.model
        b1, b2 = self.betas
        lr = self._rate()
        if self.row_step is not None:
            import ctypes as C
            adam = _lib.AdamOpts(lr, b1, b2, self.eps, int(self.t), _lib.ptr(self.m), _lib.ptr(self.v),
                                 _lib.sched_ptr(self._sched_struct()))
            if self.clip is not None:
                _lib.check(_lib.lib().fira_adam_rows_step_clip(_lib.cur_stream(), C.byref(m.dims), _lib.ptr(m.flat.data),
                                                               _lib.ptr(m.gbuf), C.byref(adam), _lib.ptr(self.row_step), None,
                                                               _lib.ptr(count), 1 << table, _lib.ptr(self.clip_state)),
                           "fira_adam_rows_step_clip")
            else:
                _lib.check(_lib.lib().fira_adam_rows_step(_lib.cur_stream(), C.byref(m.dims), _lib.ptr(m.flat.data),
                                                          _lib.ptr(m.gbuf), C.byref(adam), _lib.ptr(self.row_step), None,
                                                          _lib.ptr(count), 1 << table), "fira_adam_rows_step")
            lo += m.cfg.vocab_size * 256
        if self.clip is not None:
            ops.adam_step_clip(m.flat.data[lo:hi], m.gbuf[lo:hi], self.m[lo:hi], self.v[lo:hi], lr, self.t, self.clip_state,
                               count=count, beta1=b1, beta2=b2, eps=self.eps)
            return
        ops.adam_step_count(m.flat.data[lo:hi], m.gbuf[lo:hi], self.m[lo:hi], self.v[lo:hi], lr, self.t, count, b1, b2,
                            self.eps)

    def sync(self):
        """Apply the embedding-row updates the row-sparse path still owes (fira_adam_rows_sync): afterwards ``model.flat``,
        ``self.m`` and ``self.v`` are what the dense update leaves after ``self.t`` steps, bit for bit.  Cheap when nothing
        is owed.  Synchronises the stream (a phase change -- checkpoint, dev pass, search -- not a per-step call)."""
        if self.row_step is None or not self._rows_dirty:
            return
        self._rows_dirty = False
        schedule, lr, b1, b2, eps = self._rows_hyper           # (the values the owed updates were deferred under)
        import ctypes as C
        sched = None if schedule is None else schedule.struct()
        adam = _lib.AdamOpts(lr if schedule is None else schedule.base_lr, b1, b2, eps, int(self.t), _lib.ptr(self.m),
                             _lib.ptr(self.v), _lib.sched_ptr(sched))
        _lib.check(_lib.lib().fira_adam_rows_sync(_lib.cur_stream(), C.byref(self.model.dims), _lib.ptr(self.model.flat.data),
                                                  C.byref(adam), _lib.ptr(self.row_step)), "fira_adam_rows_sync")
        torch.cuda.current_stream().synchronize()

    def last_loss(self) -> float:
        """Mean token loss of the last (global) batch; synchronises."""
        if (self.reducer is not None and self.reducer.world > 1) or self._acc_last:
            s = self.stats.tolist()                              # (all-reduced, or accumulated over a step's micro-batches)
        else:
            s = [float(self.model.loss_sum.item()), float(self.model.n_tok.item())]
        return s[0] / max(s[1], 1.0)

    def last_grad_norm(self):
        """``(norm, coef, n_clipped, n_nonfinite)`` of the last step with ``clip_grad_norm``: the global norm of the (global)
        batch's mean-token-loss gradient before clipping, the factor the update applied, and how many steps so far were
        clipped / were applied as zero-gradient steps because the norm was not finite.  Synchronises, like :meth:`last_loss`."""
        if self.clip is None:
            raise RuntimeError("last_grad_norm: this Trainer was built without clip_grad_norm")
        st = ops.read_clip_state(self.clip_state)
        return st["norm"], st["coef"], st["n_clipped"], st["n_nonfinite"]

    def state_dict(self):
        """Everything a restart needs besides the weights: Adam moments, Adam step and the dropout step counter (so
        that a resumed run continues the mask sequence instead of replaying it from step 1)."""
        if self.zero is not None:                              # collective: every rank calls it, any rank may save it
            total = self.model.layout.total
            return self._ema_state({"m": self.zero.gather_full(self.m_sh, total), "v": self.zero.gather_full(self.v_sh, total),
                                    "t": self.t, "dropout_step": self.model.dropout_step,
                                    "lr_schedule": self._schedule_state()})
        self.sync()
        return self._ema_state({"m": self.m, "v": self.v, "t": self.t, "dropout_step": self.model.dropout_step,
                                "lr_schedule": self._schedule_state()})

    def _ema_state(self, sd):
        """With ``ema_decay``: the average, its configuration and the RAW parameters (inside :meth:`averaged` the model -- and
        so the checkpoint written from it -- holds the averaged ones; a restart needs both).  Copies, not views."""
        if self.ema is not None:
            raw = self.model.flat.data if self._raw is None else self._raw
            sd.update(ema=self.ema.clone(), ema_cfg={"decay": self.ema_cfg[0], "every": self.ema_cfg[1]}, params=raw.clone())
        return sd

    def _schedule_state(self):
        return None if self.lr_schedule is None else self.lr_schedule.as_dict()

    def load_state_dict(self, sd):
        """Restores what :meth:`state_dict` holds.  The learning-rate schedule: a Trainer built without one takes the saved
        one (a state without the key was saved by a constant-rate run: nothing to take); a Trainer built WITH one refuses a
        state saved under a different schedule -- the run would silently continue on another curve.  The weight average: a
        Trainer built with ``ema_decay`` takes ``"ema"`` and the raw ``"params"`` from a state that has them and refuses one
        saved under another ``(decay, every)``; from a state without them the average starts at the model's (loaded)
        parameters.  A Trainer built without it ignores the keys."""
        if self._raw is not None:
            raise RuntimeError("Trainer.load_state_dict inside Trainer.averaged()")
        if self.ema is not None and "ema" in sd:
            cfg = sd.get("ema_cfg") or {}
            if (cfg.get("decay"), cfg.get("every")) != self.ema_cfg:
                raise ValueError("load_state_dict: the state's weight average was kept with (decay, every) = (%r, %r), this "
                                 "Trainer was built with (%r, %r)" % ((cfg.get("decay"), cfg.get("every")) + self.ema_cfg))
        saved = sd.get("lr_schedule")
        saved = None if saved is None else ops.LrSchedule.make(saved)
        if self.lr_schedule is not None and saved != self.lr_schedule:
            raise ValueError("load_state_dict: the state was saved under the learning-rate schedule %s, this Trainer was built "
                             "with %s" % ("none (a constant rate)" if saved is None else saved, self.lr_schedule))
        if self.zero is not None:                              # the checkpoint holds full moments: keep the owned shards
            for b in (0, 1):
                lo, hi = self.zero.owned(b)
                self.m_sh[b][:hi - lo].copy_(sd["m"][lo:hi]); self.v_sh[b][:hi - lo].copy_(sd["v"][lo:hi])
        else:
            self.sync()
            self.m.copy_(sd["m"]); self.v.copy_(sd["v"])
        self.lr_schedule = saved
        self.t = int(sd["t"])
        if self.row_step is not None:
            self.row_step.fill_(self.t)                          # a checkpoint holds synced tables
        self.model.dropout_step = int(sd.get("dropout_step", self.t))
        if self.ema is not None:
            if "ema" in sd:
                if "params" in sd:
                    self.model.flat.data.copy_(sd["params"])
                self.ema.copy_(sd["ema"])
                self.ema_updates = self.t // self.ema_cfg[1]
            else:
                self.ema.copy_(self.model.flat.data)
                self.ema_updates = 0
