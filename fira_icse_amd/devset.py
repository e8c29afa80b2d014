"""Dev-set model selection (reference run_model.py:118-184): a teacher-forced pass over the valid split and NLTK
sentence-BLEU (method 2) per commit, as the host loop the driver has always run (``host_pass``) and on the device
(``device_pass``: resident batches, ``fira_dev_bleu_stats`` on token ids, one copy back per pass).

Both passes return ``(total, lines)``: this rank's plain running sum of the per-commit scores over its shard, in shard order,
and a callable that builds this rank's ``dev_output`` lines.  The two are interchangeable: the totals are ``==`` and the lines
the same strings (DESIGN.md 6i has the argument; tests/test_dev_bleu_gpu.py holds them to it).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import metrics, text
from .config import EOS, PAD, UNK, FiraConfig
from .parallel import shard_indices

_STAT_COLS = 12
_ROUGE_COLS = 4
_METEOR_COLS = 4


def check_vocabulary(r_vocab: Dict[int, str], vocab_size: int) -> None:
    """Raises ValueError unless comparing vocabulary ids is the same as comparing the words the host pass compares.

    The host joins the hypothesis' words with blanks, deletes ``<pad>``, writes ``<unkm>`` as the emoji, and splits at white
    space.  That round trip gives back exactly the non-pad words, one per id, iff every id has a word, no word is empty or
    contains white space, no word other than the two tokens themselves contains ``<pad>`` / ``<unkm>``, and no word IS the
    emoji (a hypothesis ``<unkm>`` would then equal that word in a reference).  Distinct ids always carry distinct words:
    ``r_vocab`` inverts a word -> id dictionary."""
    if r_vocab.get(PAD) != "<pad>" or r_vocab.get(UNK) != "<unkm>":
        raise ValueError("device dev pass: ids %d / %d must be '<pad>' / '<unkm>', not %r / %r"
                         % (PAD, UNK, r_vocab.get(PAD), r_vocab.get(UNK)))
    for i in range(vocab_size):
        if i not in r_vocab:
            raise ValueError("device dev pass: vocabulary id %d has no word" % i)
    for i, w in r_vocab.items():
        if w.split() != [w]:
            raise ValueError("device dev pass: the word of id %d (%r) is empty or contains white space" % (i, w))
        if w == text.UNK_EMOJI:
            raise ValueError("device dev pass: the word of id %d is the emoji the host writes for <unkm>" % i)
        for tok in ("<pad>", "<unkm>"):
            if tok in w and w != tok:
                raise ValueError("device dev pass: the word of id %d (%r) contains %s" % (i, w, tok))


class DevEvaluator:
    """The valid split of one rank, scored on the host or on the device.

    ``model`` supplies ``forward_dev`` and the device (None: a CPU evaluator for ``host_pass`` with an injected ``ids_fn``);
    ``store`` is the valid ``GraphStore``; ``var_maps`` / ``valid_index`` map a commit to its ``variable.json`` entry.
    ``ids_fn(db) -> int32 [B, T]`` replaces ``model.forward_dev`` in BOTH passes; every batch carries the store positions of
    its commits as ``db.commits``.  Sharding and batch boundaries are the driver's: ``shard_indices`` over the split, batches of
    ``batch_size // world`` commits, tail batch included.

    Resident set of ``device_pass``.  A ``DeviceBatch`` owns its device arena (the pinned ring is only the staging side of its
    one copy), so the batches built at the first call stay valid whatever is collated later.  An arena holds the id arrays,
    the node lists and the CSR adjacency: on ``synth.py`` commits 18.4 kB per commit (18.0 to 18.8 kB over four batches of 170: 3.06 to 3.20 MB
    per arena), i.e. about 148 MB for the reference's 8 000 valid commits on one rank -- 0.05 % of 288 GB -- plus
    4 * (12 + tar_len) = 168 bytes per commit (1.3 MB) for the two pass-wide result buffers.  ``resident_bytes`` has the
    actual figure of a built set.

    ``rouge_l=True``: both passes also score every commit by sentence-level ROUGE-L (``metrics.rouge_l`` on the same words;
    on the device ``fira_dev_rouge_l_stats`` on the same ids, 16 more bytes per commit in the pass-wide buffer and the same one
    copy back) and leave the values in ``last_rouge_l``, per commit in shard order.  A second reported figure only: model
    selection, the ``dev_output`` lines and the return values are the BLEU ones either way.

    ``meteor_exact=True``: the same for ``metrics.meteor_exact`` (NLTK's METEOR alignment and score without its stem and WordNet
    stages -- not the paper's METEOR): ``fira_dev_meteor_stats`` on the device, 16 more bytes per commit behind the ROUGE-L
    block, the values in ``last_meteor_exact``.  ``meteor_classes`` (needs ``meteor_exact=True``): integers, one per vocabulary
    id; words of equal class match in a second stage on both passes (the host looks the class of a word up through
    ``r_vocab``; a hypothesis ``<unkm>`` has none).  A third reported figure only.
    """

    def __init__(self, model, store, cfg: FiraConfig, r_vocab: Dict[int, str], var_maps: Sequence[Dict[str, str]],
                 valid_index: Sequence[int], rank: int = 0, world: int = 1,
                 ids_fn: Optional[Callable] = None, device=None, rouge_l: bool = False, meteor_exact: bool = False,
                 meteor_classes=None):
        self.model, self.store, self.cfg = model, store, cfg
        self.r_vocab, self.var_maps, self.valid_index = r_vocab, var_maps, valid_index
        self.rank, self.world = rank, world
        self.device = torch.device(device if device is not None else (model.device_ if model is not None else "cpu"))
        if ids_fn is None:
            if model is None:
                raise ValueError("DevEvaluator needs a model or an ids_fn")
            ids_fn = model.forward_dev
        self.ids_fn = ids_fn
        self.mine: List[int] = shard_indices(list(range(len(store))), rank, world)
        self.bs = max(1, cfg.batch_size // world)
        self.last_scores: List[float] = []       # per-commit scores of the latest pass, in shard order
        self.rouge_l = bool(rouge_l)
        self.last_rouge_l: List[float] = []      # per-commit ROUGE-L of the latest pass (rouge_l=True), in shard order
        self.meteor_exact = bool(meteor_exact)
        self.last_meteor_exact: List[float] = []     # per-commit meteor_exact of the latest pass (meteor_exact=True)
        self.meteor_classes = None               # int32 [vocab_size] on the host, or None
        if meteor_classes is not None:
            if not self.meteor_exact:
                raise ValueError("meteor_classes: needs meteor_exact=True")
            table = torch.as_tensor(meteor_classes)
            if table.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
                raise ValueError("meteor_classes: expected integers, got %s" % table.dtype)
            if tuple(table.shape) != (cfg.vocab_size,):
                raise ValueError("meteor_classes: shape %s, expected (%d,)" % (tuple(table.shape), cfg.vocab_size))
            table = table.detach().cpu().long()
            if table.numel() and (int(table.min()) < -(1 << 31) or int(table.max()) >= 1 << 31):
                raise ValueError("meteor_classes: class outside the int32 range")
            self.meteor_classes = table.to(torch.int32)
        self._batches = None                     # resident DeviceBatches (device_pass)
        self._out = None                         # [n_mine, 12 + T (+ 4) (+ 4)] int32: stats | hyp (| ROUGE-L) (| METEOR) of one pass
        self._classes_dev = None                 # meteor_classes on the device (device_pass)

    def _batch(self, idx):
        from .model import DeviceBatch
        db = DeviceBatch(self.store.batch(idx), self.cfg, self.device)
        db.commits = list(idx)
        return db

    def _line(self, i: int, words: List[str], b: float) -> str:
        back = {v: k for k, v in self.var_maps[self.valid_index[i]].items()}
        return " ".join(back.get(t, t) for t in words) + "," + str(b)

    # ------------------------------------------------------------------------------ the host loop (run_model.py:118-184)
    @torch.no_grad()
    def host_pass(self):
        cfg, store = self.cfg, self.store
        lines, total, scores, rouge, meteor = [], 0.0, [], [], []
        word_class = None
        if self.meteor_classes is not None:      # the class of a WORD; the emoji a hypothesis <unkm> is written as has none
            word_class = {self.r_vocab[i]: c for i, c in enumerate(self.meteor_classes.tolist()) if i in self.r_vocab}
        for lo in range(0, len(self.mine), self.bs):
            idx = self.mine[lo:lo + self.bs]
            ids = self.ids_fn(self._batch(idx)).cpu().tolist()
            for k, i in enumerate(idx):
                sen = text.dev_sentence(ids[k], store.sou[i], store.sub_token[i], cfg.vocab_size, cfg.sou_len, EOS)
                s = " ".join(self.r_vocab[t] for t in sen).replace("<pad>", "").replace("<unkm>", text.UNK_EMOJI).strip()
                hyp = s.split()
                ref_ids = store.tar[i].tolist()
                ref = [self.r_vocab[t] for t in ref_ids[1:ref_ids.index(EOS)]]
                b = metrics.sentence_bleu_method2([ref], hyp)
                total += b
                scores.append(b)
                if self.rouge_l:
                    rouge.append(metrics.rouge_l(ref, hyp))
                if self.meteor_exact:
                    meteor.append(metrics.meteor_exact(ref, hyp, word_class))
                lines.append(self._line(i, hyp, b))
        self.last_scores = scores
        self.last_rouge_l = rouge
        self.last_meteor_exact = meteor
        return total, lambda: lines

    # ------------------------------------------------------------------------------ the device pass
    def _build_resident(self):
        check_vocabulary(self.r_vocab, self.cfg.vocab_size)
        tar = np.asarray(self.store.tar)[self.mine] if self.mine else np.zeros((0, self.cfg.tar_len), np.int64)
        no_eos = np.nonzero(~(tar == EOS).any(axis=1))[0]
        if no_eos.size:                          # (the host pass raises ValueError from list.index on such a commit)
            raise ValueError("device dev pass: valid commit %d has no <eos> in its target" % self.mine[int(no_eos[0])])
        self._batches = [self._batch(self.mine[lo:lo + self.bs]) for lo in range(0, len(self.mine), self.bs)]
        cols = (_STAT_COLS + self.cfg.tar_len + (_ROUGE_COLS if self.rouge_l else 0)
                + (_METEOR_COLS if self.meteor_exact else 0))
        self._out = torch.empty((len(self.mine) * cols,), dtype=torch.int32, device=self.device)
        if self.meteor_classes is not None:
            self._classes_dev = self.meteor_classes.to(self.device)

    @property
    def resident_bytes(self) -> int:
        """Device bytes the resident set holds (0 before the first ``device_pass``)."""
        if self._batches is None:
            return 0
        return sum(db.arena.numel() for db in self._batches) + self._out.numel() * 4

    @torch.no_grad()
    def device_pass(self):
        from . import ops
        cfg, n, T = self.cfg, len(self.mine), self.cfg.tar_len
        if self._batches is None:
            self._build_resident()
        stats = self._out[:n * _STAT_COLS].view(n, _STAT_COLS)
        hyp = self._out[n * _STAT_COLS:n * (_STAT_COLS + T)].view(n, T)
        r_end = n * (_STAT_COLS + T + (_ROUGE_COLS if self.rouge_l else 0))
        rouge = self._out[n * (_STAT_COLS + T):r_end].view(n, _ROUGE_COLS) if self.rouge_l else None
        meteor = self._out[r_end:].view(n, _METEOR_COLS) if self.meteor_exact else None
        off = 0
        for db in self._batches:
            ids = self.ids_fn(db)
            db.wait_ready()
            ops.dev_bleu_stats(ids, db.sou, db.sub_token, db.tar, cfg.vocab_size, hyp=hyp[off:off + db.B],
                               stats=stats[off:off + db.B])
            if self.rouge_l:
                ops.dev_rouge_l_stats(ids, db.sou, db.sub_token, db.tar, cfg.vocab_size, stats=rouge[off:off + db.B])
            if self.meteor_exact:
                ops.dev_meteor_stats(ids, db.sou, db.sub_token, db.tar, cfg.vocab_size, classes=self._classes_dev,
                                     stats=meteor[off:off + db.B])
            off += db.B
        host = self._out.cpu()                   # the pass's one copy back and its one synchronisation
        st = host[:n * _STAT_COLS].view(n, _STAT_COLS).tolist()
        total, scores = 0.0, []
        for row in st:
            b = metrics.bleu_method2_from_stats(row[0:4], row[4:8], row[8], row[9])
            total += b
            scores.append(b)
        self.last_scores = scores
        self.last_rouge_l = ([metrics.rouge_l_from_stats(r[0], r[1], r[2])
                              for r in host[n * (_STAT_COLS + T):r_end].view(n, _ROUGE_COLS).tolist()] if self.rouge_l else [])
        self.last_meteor_exact = ([metrics.meteor_exact_from_stats(r[0], r[1], r[2], r[3])
                                   for r in host[r_end:].view(n, _METEOR_COLS).tolist()] if self.meteor_exact else [])
        hyp_host = host[n * _STAT_COLS:n * (_STAT_COLS + T)].view(n, T)

        def lines():
            out = []
            for k, (i, row) in enumerate(zip(self.mine, hyp_host.tolist())):
                words = [text.UNK_EMOJI if t == UNK else self.r_vocab[t] for t in row[:st[k][8]]]
                out.append(self._line(i, words, scores[k]))
            return out

        return total, lines
