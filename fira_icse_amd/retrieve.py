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
