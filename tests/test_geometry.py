"""The box of model geometries the library accepts, and the fixtures of tests/test_geometry_gpu.py, without a GPU.

* every bound of ``get_layout`` (csrc/layout.cpp): the value at the bound is accepted, the value one past it is refused with
  a message that names the field -- checked through ``fira_param_count``, as tests/test_abi.py does;
* the batches of ``geometry_ref.build_batch`` are well-formed at every case (prefixes, label kinds, the normalised graph);
* what the GPU comparisons assume about the oracle holds for the oracle alone: the recorded fp32-against-fp64 distance covers
  the measured one, at most 2 % of a case's labelled positions have a top-2 margin below the arg-max threshold, and the
  oracle's search on the peaked weights ends hypotheses at two lengths or more without a near-tie at any step;
* a geometry the search's row kernels refuse (more than 25600 words) is refused by ``fira_decode_begin``, ahead of any launch.
"""
import ctypes as C

import numpy as np
import pytest

import geometry_ref as G
from fira_icse_amd import _lib
from fira_icse_amd.config import FiraConfig
from fira_icse_amd.model import batch_lists

CASES = list(G.CASES.values())
ids = [c.name for c in CASES]


def _count(lib, **fields):
    d = _lib.make_dims(FiraConfig())
    for k, v in fields.items():
        assert hasattr(d, k)
        setattr(d, k, v)
    return lib.fira_param_count(C.byref(d)), lib.fira_last_error().decode()


# field(s) at the bound, field(s) one past it, what the refusal names
BOUNDS = [
    (dict(tar_len=2), dict(tar_len=1), "tar_len = 1"),
    (dict(tar_len=32), dict(tar_len=33), "tar_len = 33"),
    (dict(sou_len=1), dict(sou_len=0), "sou_len = 0"),
    (dict(sub_len=0), dict(sub_len=-1), "sub_len = -1"),
    (dict(sou_len=224, sub_len=160), dict(sou_len=225, sub_len=160), "sou_len + sub_len = 385"),
    (dict(sou_len=384, sub_len=0), dict(sou_len=385, sub_len=0), "sou_len + sub_len = 385"),
    (dict(ast_len=0), dict(ast_len=-1), "ast_len = -1"),
    (dict(ast_len=400), dict(ast_len=401), "ast_len = 401"),
    (dict(n_layer=1), dict(n_layer=0), "n_layer = 0"),
    (dict(n_layer=16), dict(n_layer=17), "n_layer = 17"),
    (dict(vocab=4), dict(vocab=3), "vocab = 3"),
    (dict(ast_vocab=1), dict(ast_vocab=0), "ast_vocab = 0"),
    (dict(d_ff=64), dict(d_ff=0), "d_ff = 0"),
    (dict(d_ff=1088), dict(d_ff=1056), "d_ff = 1056"),
]


@pytest.mark.parametrize("at, past, names", BOUNDS, ids=[b[2] for b in BOUNDS])
def test_every_bound_of_get_layout(lib, at, past, names):
    n, _ = _count(lib, **at)
    assert n > 0, at
    n, msg = _count(lib, **past)
    assert n == -1 and names in msg and "unsupported geometry" in msg, (past, msg)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_every_case_is_inside_the_box(lib, case):
    d = _lib.make_dims(case.cfg)
    # 338 tensors at six layers: 52 per layer, 26 besides (four tables, the dead LSTM's 12, the head's 10)
    assert lib.fira_param_count(C.byref(d)) == 26 + 52 * case.cfg.num_layers, lib.fira_last_error()
    assert lib.fira_workspace_bytes(C.byref(d), case.B, 1) > lib.fira_workspace_bytes(C.byref(d), case.B, 0) > 0


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_batches_are_well_formed(case):
    cfg, hb = case.cfg, G.case_batch(case)
    B, L, S, A, T, V, N = case.B, cfg.sou_len, cfg.sub_token_len, cfg.ast_change_len, cfg.tar_len, cfg.vocab_size, cfg.graph_len
    assert hb.sou.shape == (B, L) and hb.sub_token.shape == (B, S) and hb.ast_change.shape == (B, A)
    assert hb.tar.shape == hb.tar_label.shape == (B, T) and hb.mark.shape == (B, L)
    assert all(a.dtype == np.int64 for a in (hb.sou, hb.sub_token, hb.ast_change, hb.tar, hb.tar_label, hb.mark))
    assert hb.rowptr.dtype == np.int32 and hb.col.dtype == np.int32 and hb.val.dtype == np.float32
    for a, hi in ((hb.sou, V), (hb.sub_token, V), (hb.ast_change, cfg.ast_change_vocab_size), (hb.tar, V), (hb.mark, 4)):
        n = (a != 0).sum(1)
        assert a.min(initial=0) >= 0 and a.max(initial=0) < hi
        assert all(not a[b, n[b]:].any() and a[b, :n[b]].all() for b in range(B))          # a prefix, then zero padding
    n_sou, n_sub, n_tar = (hb.sou != 0).sum(1), (hb.sub_token != 0).sum(1), (hb.tar != 0).sum(1)
    assert n_sou[0] == L and n_tar[0] == T and (hb.mark != 0).sum(1).tolist() == n_sou.tolist()
    for b in range(B):
        assert hb.sou[b, 0] == hb.tar[b, 0] == 2 and hb.sou[b, n_sou[b] - 1] == hb.tar[b, n_tar[b] - 1] == 1
        assert ((hb.sou[b, 1:n_sou[b] - 1] >= 4).all() and (hb.sub_token[b, :n_sub[b]] >= 4).all())
    if B > 1:
        assert n_sou[1] == 2 and n_tar[1] == 2 and n_sub[1] == 0
    if S:
        assert n_sub[0] == S
    # labels: 0 exactly on padding; a copy label points at a live slot that holds the word
    assert ((hb.tar_label != 0) == (hb.tar != 0)).all() and hb.tar_label.max() < cfg.out_len
    for b, t in zip(*np.nonzero(hb.tar_label)):
        lab, w = hb.tar_label[b, t], hb.tar[b, t]
        if lab >= V + L:
            assert lab - V - L < n_sub[b] and hb.sub_token[b, lab - V - L] == w
        elif lab >= V:
            assert lab - V < n_sou[b] and hb.sou[b, lab - V] == w
        else:
            assert lab == w
    words, code, sub = G.label_kinds(cfg, hb)
    assert words > 0 and (code > 0) == (T > 2) and (sub > 0) == (T > 3 and S > 0)
    # graph: symmetric, a self-loop on every node, padding nodes nothing else, D^-1/2 (A) D^-1/2 values, sorted unique columns
    assert hb.rowptr.shape == (B * N + 1,) and hb.rowptr[0] == 0 and hb.rowptr[-1] == hb.col.shape[0] == hb.val.shape[0]
    E = hb.dense_edge(N)
    assert (E == E.transpose(0, 2, 1)).all() and (np.diagonal(E, axis1=1, axis2=2) > 0).all()
    deg = (E != 0).sum(2)
    ids_all = np.concatenate([hb.sou, hb.sub_token, hb.ast_change], 1)
    assert (deg[ids_all == 0] == 1).all() and (deg[ids_all != 0] > 1).all()
    want = (E != 0) / np.sqrt(deg[:, :, None]) / np.sqrt(deg[:, None, :])
    assert np.abs(E - want).max() < 1e-7                                   # fp32 roundings of the float64 values
    d = np.diff(hb.rowptr)
    assert d.sum() == (E != 0).sum()
    rows = np.repeat(np.arange(B * N), d)
    assert ((np.diff(hb.col) > 0) | (np.diff(rows) > 0)).all() and (hb.col // N == rows // N).all()
    if n_sou[0] + n_sub[0] + (hb.ast_change[0] != 0).sum() > 66:
        assert d.max() > 64                                                # the hub row: the gather's tail path
    # the engine's host lists take the batch in both layouts (zero-width arrays included)
    for skip in (True, False):
        lists = batch_lists(hb, cfg, skip)
        assert lists[0].shape[0] == (int((ids_all != 0).sum()) if skip else B * N)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_recorded_oracle_error_covers_the_measured_one(case):
    eps = G.oracle_fp32_error(case.cfg, G.case_weights(case), G.case_batch(case))
    assert 0.25 * case.oracle_eps <= eps <= case.oracle_eps, (case.name, eps)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_argmax_margins_leave_at_most_two_percent_out(case):
    hb = G.case_batch(case)
    ids_, margin = G.oracle_argmax_and_margins(case.cfg, G.case_weights(case), hb)
    lab = G.labelled(hb)
    assert lab.sum() >= 1 and ids_.shape == lab.shape
    assert (margin[lab] <= case.threshold).mean() <= G.ARGMAX_MAX_EXCLUDED, (case.name, np.sort(margin[lab])[:4], case.threshold)


def test_builder_is_deterministic_and_seeded():
    c = G.CASES["off_by_one"]
    a, b, other = G.build_batch(c.cfg, c.B, 3), G.build_batch(c.cfg, c.B, 3), G.build_batch(c.cfg, c.B, 4)
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("sou", "tar", "tar_label", "sub_token", "col", "val"))
    assert not np.array_equal(a.sou, other.sou)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_oracle_search_fixture(case):
    """What tests/test_geometry_gpu.py compares the device searches with, from the oracle alone: with the peaked weights no step
    of greedy or beam-3 search has two neighbouring candidates (the taken ones and the best one not taken) closer than the
    arg-max threshold, so every hypothesis is decided by the model and needs no exclusion; and the beam's hypotheses end at two
    lengths or more wherever the geometry has room for that (``tar_len`` 2 leaves one step)."""
    for beam in (1, 3):
        hyp, prob, gap = G.oracle_search(case, beam)
        assert len(hyp) == case.B and all(len(row) == beam for row in hyp)
        assert all(h[0] == 2 and 2 <= len(h) <= case.cfg.tar_len for row in hyp for h in row)
        assert all(p > 0 for row in prob for p in row), (case.name, beam, prob)        # no underflow: nothing ties at zero
        assert gap > case.threshold, (case.name, beam, gap, case.threshold)
    lengths = {len(h) for row in G.oracle_search(case, 3)[0] for h in row}
    assert len(lengths) >= 2 or case.cfg.tar_len == 2, (case.name, lengths)


def test_search_refuses_a_vocabulary_its_row_kernels_cannot_hold(lib):
    """fira_decode_begin is the first library call of every search (Searcher._begin): the refusal comes before the encoder
    pass, with the message of the row kernels' own check."""
    big, ok = _lib.make_dims(G.CASES["big_vocab"].cfg), _lib.make_dims(FiraConfig(vocab_size=25600))
    assert lib.fira_decode_begin_ex(None, C.byref(big), None, None, None, 0, 3, 0) != 0
    msg = lib.fira_last_error().decode()
    assert "fira_decode_begin" in msg and "vocabulary 25602" in msg and "outside 4..25600" in msg, msg
    assert lib.fira_decode_begin_ex(None, C.byref(ok), None, None, None, 0, 3, 0) != 0       # (no batch: refused further on)
    assert "vocabulary" not in lib.fira_last_error().decode()
