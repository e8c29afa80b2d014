"""Retrieval for retrieval-augmented search: the store of training-commit vectors and the
nearest-neighbour query.

A commit's vector is the mean of its valid encoder-memory rows, L2-normalised (``fira_pool_memory``); the neighbour of a
commit is the stored vector with the largest dot product (``fira_nn_search``: one pass over the store for up to 64 queries).
``decode.Neighbour`` carries the result into ``Searcher.greedy`` / ``greedy_many`` / ``beam``.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import warnings
from typing import Optional, Sequence

import torch

from . import _lib, ops

MAX_QUERIES = 64                                 # fira_nn_search: B <= 64 per call


def model_checksum(model) -> str:
    """A checksum of the model's flat parameters (sha256 of the fp32 bytes): vectors pooled under other weights do not
    belong to this model."""
    flat = model.flat.data.detach().to("cpu", torch.float32).contiguous()
    return hashlib.sha256(flat.numpy().tobytes()).hexdigest()


def pooled_vectors(searcher, db) -> torch.Tensor:
    """u [B, 256]: the encoder pass of ``db`` (``Searcher._begin(db, 1)``) and ``fira_pool_memory`` over its workspace."""
    ws = searcher._begin(db, 1)
    dims, lib, B = searcher.model.dims, _lib.lib(), db.B
    mem_p = lib.fira_decode_memory(C.byref(dims), _lib.ptr(ws), B, 1)
    val_p = lib.fira_decode_mem_valid(C.byref(dims), _lib.ptr(ws), B, 1)
    out = torch.empty((B, 256), dtype=torch.float32, device=searcher.model.device_)
    _lib.check(lib.fira_pool_memory(_lib.cur_stream(), C.byref(dims), B, C.c_void_p(mem_p), C.c_void_p(val_p), _lib.ptr(out)),
               "fira_pool_memory")
    return out


class Datastore:
    """The unit vectors of a set of commits on the device (``vectors`` [N, 256] fp32) and the commit index each belongs to
    (``index`` [N] int64 on the host, e.g. the row in the train ``GraphStore``)."""

    def __init__(self, vectors: torch.Tensor, index, checksum: str = ""):
        index = torch.as_tensor(index, dtype=torch.int64).reshape(-1).cpu()
        if vectors.dim() != 2 or vectors.shape[1] != 256 or vectors.shape[0] != index.numel():
            raise ValueError("Datastore: vectors %s do not match %d commit indices (expected [N, 256])"
                             % (tuple(vectors.shape), index.numel()))
        self.vectors, self.index, self.checksum = vectors.to(torch.float32).contiguous(), index, checksum

    def __len__(self):
        return self.vectors.shape[0]

    @classmethod
    def build(cls, model, batches, searcher=None) -> "Datastore":
        """``batches``: an iterable of (commit indices, DeviceBatch).  One encoder pass and one pooling launch per batch."""
        from .decode import Searcher
        searcher = Searcher(model) if searcher is None else searcher
        vecs, index = [], []
        with torch.no_grad():
            for idx, db in batches:
                vecs.append(pooled_vectors(searcher, db).clone())
                index.extend(int(i) for i in idx)
        if not vecs:
            raise ValueError("Datastore.build: no batches")
        return cls(torch.cat(vecs, 0), index, model_checksum(model))

    def save(self, path: str) -> None:
        torch.save({"vectors": self.vectors.cpu(), "index": self.index, "checksum": self.checksum, "format": 1}, path)

    @classmethod
    def load(cls, path: str, model=None, device=None) -> "Datastore":
        """Reads what ``save`` wrote; with ``model`` the vectors go to its device and a ``UserWarning`` is raised when its
        parameters are not the ones the vectors were pooled under."""
        blob = torch.load(path, map_location="cpu")
        if not isinstance(blob, dict) or blob.get("format") != 1 or "vectors" not in blob or "index" not in blob:
            raise ValueError("Datastore.load: %s is not a datastore file" % path)
        if model is not None:
            device = model.device_ if device is None else device
            if blob.get("checksum") != model_checksum(model):
                warnings.warn("Datastore.load: %s was built with other model parameters (checksum mismatch); its neighbours "
                              "are not this model's" % path)
        vectors = blob["vectors"] if device is None else blob["vectors"].to(device)
        return cls(vectors, blob["index"], blob.get("checksum", ""))

    @torch.no_grad()
    def query(self, searcher, db, exclude: Optional[Sequence[int]] = None):
        """(idx [B] int64: the neighbour's commit index (``self.index`` applied), sim [B] float32 in [0, 1]), both on the host.
        ``exclude``: per commit a commit index that must not be returned (-1 or None entries: nothing), e.g. the commit
        itself when it is in the store.  Batches above 64 commits are searched in chunks of 64."""
        B = db.B
        rows = None
        if exclude is not None:
            ex = [-1 if e is None else int(e) for e in exclude]
            if len(ex) != B:
                raise ValueError("Datastore.query: %d exclude values for a batch of %d commits" % (len(ex), B))
            if len(self) < 2:
                raise ValueError("Datastore.query: exclude with a store of %d vectors leaves nothing to return" % len(self))
            pos = {int(c): j for j, c in enumerate(self.index.tolist())}
            rows = torch.tensor([pos.get(e, -1) for e in ex], dtype=torch.int32, device=self.vectors.device)
        u = pooled_vectors(searcher, db)
        idx, sim = [], []
        for lo in range(0, B, MAX_QUERIES):
            hi = min(lo + MAX_QUERIES, B)
            i, s = ops.nn_search(u[lo:hi].contiguous(), self.vectors, None if rows is None else rows[lo:hi].contiguous())
            idx.append(i)
            sim.append(s)
        idx = torch.cat(idx).long().cpu()
        sim = torch.cat(sim).cpu()
        if bool((idx < 0).any()):
            raise ValueError("Datastore.query: a query has no admissible neighbour (non-finite vectors)")
        return self.index[idx], sim


# ------------------------------------------------------------------------------------------------ token-level store (kNN-MT)
KEY_WIDTH = 256                                  # fira_knn_search: keys [N, 256]
MAX_TOKEN_ROWS = 8388608                         # fira_knn_search: N <= 8 388 608


def sum_sq_rows(x: torch.Tensor) -> torch.Tensor:
    """[N] sums of squares of the rows of x [N, C] in ascending column order, every multiply and add its own fp32 operation
    (one elementwise multiply and one add per column: no fused multiply-add, no tree)."""
    ss = torch.zeros(x.shape[0], dtype=torch.float32, device=x.device)
    for c in range(x.shape[1]):
        col = x[:, c]
        ss = ss + col * col
    return ss


def resolve_labels(tar_label, sou, sub_token, vocab: int):
    """The vocabulary id every label of ``tar_label`` [B, T] stands for (numpy int64): itself below ``vocab``, else the id of
    the diff slot or sub-token slot it addresses, the way ``fira_merge_dist`` resolves an entry."""
    import numpy as np
    lab, sou, sub = (np.asarray(a, dtype=np.int64) for a in (tar_label, sou, sub_token))
    L, S = sou.shape[1], sub.shape[1]
    out = lab.copy()
    if L:
        in_sou = (lab >= vocab) & (lab < vocab + L)
        out = np.where(in_sou, np.take_along_axis(sou, np.clip(lab - vocab, 0, L - 1), 1), out)
    if S:
        in_sub = lab >= vocab + L
        out = np.where(in_sub, np.take_along_axis(sub, np.clip(lab - vocab - L, 0, S - 1), 1), out)
    return out


class TokenStore:
    """One row per training token: ``keys`` [N, 256] fp32 (the decoder's last hidden state,
    ``fira_decode_hidden``, after the message's words 0..t), ``key_sq`` [N] (``sum_sq_rows``), ``values`` [N] int32 (the word at
    t + 1 as a vocabulary id, copy labels resolved), ``owner`` [N] int32 (the commit index the row comes from), all on the
    device; ``N`` rows.  ``decode.KnnMT`` carries it into the searches."""

    def __init__(self, keys: torch.Tensor, values, owner, key_sq: Optional[torch.Tensor] = None, checksum: str = ""):
        if keys.dim() != 2:
            raise ValueError("TokenStore: keys %s are not [N, width]" % (tuple(keys.shape),))
        dev = keys.device
        self.keys = keys.to(torch.float32).contiguous()
        self.values = torch.as_tensor(values).reshape(-1).to(dev, torch.int32).contiguous()
        self.owner = torch.as_tensor(owner).reshape(-1).to(dev, torch.int32).contiguous()
        self.N = int(self.keys.shape[0])
        if self.values.numel() != self.N or self.owner.numel() != self.N:
            raise ValueError("TokenStore: %d keys, %d values, %d owners" % (self.N, self.values.numel(), self.owner.numel()))
        if self.N > MAX_TOKEN_ROWS:
            raise ValueError("TokenStore: %d rows, more than %d" % (self.N, MAX_TOKEN_ROWS))
        self.key_sq = sum_sq_rows(self.keys) if key_sq is None else key_sq.reshape(-1).to(dev, torch.float32).contiguous()
        if self.key_sq.numel() != self.N:
            raise ValueError("TokenStore: %d keys, %d sums of squares" % (self.N, self.key_sq.numel()))
        self.checksum = checksum

    def __len__(self):
        return self.N

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.keys, self.key_sq, self.values, self.owner))

    @classmethod
    @torch.no_grad()
    def build(cls, searcher, batches) -> "TokenStore":
        """``batches``: an iterable of (commit indices, DeviceBatch with ``tar_label``).  Per batch one encoder pass and the
        teacher-forced step loop: step t feeds word t of every reference message (word 0 is <start>, copy labels resolved to
        vocabulary ids -- what the searches feed back), ``fira_decode_hidden`` hands over the hidden rows, and the rows of the
        commits that have a word at t + 1 are appended on the device, step by step, commit by commit."""
        from .decode import START
        searcher._no_ensemble("TokenStore.build")
        model, cfg = searcher.model, searcher.cfg
        if cfg.embedding_dim != KEY_WIDTH:
            raise ValueError("TokenStore.build: the model's width is %d, the keys' %d" % (cfg.embedding_dim, KEY_WIDTH))
        lib, dims, dev, T = _lib.lib(), model.dims, model.device_, cfg.tar_len
        keys, values, owner = [], [], []
        for idx, db in batches:
            if db.tar_label is None:
                raise ValueError("TokenStore.build: a batch without tar_label")
            B = db.B
            commits = torch.as_tensor([int(i) for i in idx], dtype=torch.int32)
            if commits.numel() != B:
                raise ValueError("TokenStore.build: %d commit indices for a batch of %d" % (commits.numel(), B))
            ws = searcher._begin(db, 1)
            lab = db.tar_label.cpu().numpy()
            words = torch.from_numpy(resolve_labels(lab, db.sou.cpu().numpy(), db.sub_token.cpu().numpy(), cfg.vocab_size))
            has = torch.from_numpy(lab != 0).long().cumprod(1).bool()          # [B, T]: positions 0..p all hold words
            words[:, 0] = START
            words_d = words.to(dev, torch.int32)
            commits_d = commits.to(dev)
            hid = torch.empty((B, KEY_WIDTH), dtype=torch.float32, device=dev)
            best_id = torch.empty(B, dtype=torch.int32, device=dev)
            best_p = torch.empty(B, dtype=torch.float32, device=dev)
            for t in range(T - 1):
                rows = torch.nonzero(has[:, t + 1]).reshape(-1)
                if rows.numel() == 0:
                    break
                tok = words_d[:, t].contiguous()
                searcher._step_model(model, ws, B, 1, t, tok, None, None, best_id, best_p)
                _lib.check(lib.fira_decode_hidden(_lib.cur_stream(), C.byref(dims), _lib.ptr(ws), ws.numel(), B, 1, searcher.flags,
                                                  _lib.ptr(hid)), "fira_decode_hidden")
                rows_d = rows.to(dev)
                keys.append(hid.index_select(0, rows_d))
                values.append(words_d[:, t + 1].index_select(0, rows_d))
                owner.append(commits_d.index_select(0, rows_d))
        if not keys:
            raise ValueError("TokenStore.build: no rows (no batches, or no message with a word after <start>)")
        return cls(torch.cat(keys, 0), torch.cat(values), torch.cat(owner), checksum=model_checksum(model))

    def save(self, path: str) -> None:
        torch.save({"keys": self.keys.cpu(), "key_sq": self.key_sq.cpu(), "values": self.values.cpu(), "owner": self.owner.cpu(),
                    "checksum": self.checksum, "format": "tokens-1"}, path)

    @classmethod
    def load(cls, path: str, model=None, device=None) -> "TokenStore":
        """Reads what ``save`` wrote; with ``model`` the rows go to its device and a ``UserWarning`` is raised when its
        parameters are not the ones the keys were formed under."""
        blob = torch.load(path, map_location="cpu")
        if not isinstance(blob, dict) or blob.get("format") != "tokens-1" or any(
                k not in blob for k in ("keys", "key_sq", "values", "owner")):
            raise ValueError("TokenStore.load: %s is not a token store file" % path)
        if model is not None:
            device = model.device_ if device is None else device
            if blob.get("checksum") != model_checksum(model):
                warnings.warn("TokenStore.load: %s was built with other model parameters (checksum mismatch); its keys are "
                              "not this model's hidden states" % path)
        keys = blob["keys"] if device is None else blob["keys"].to(device)
        return cls(keys, blob["values"], blob["owner"], blob["key_sq"], blob.get("checksum", ""))
