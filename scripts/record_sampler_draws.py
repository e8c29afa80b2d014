"""Record tests/golden/sampler_draws.npz: what fira_sample_dist draws, bit for bit, on fixed rows under fixed settings.

    FIRA_HIP_LIB=PATH/libfira_hip.so python scripts/record_sampler_draws.py [--out tests/golden/sampler_draws.npz]

The fixture pins the sampler body's draws across refactors of its code: tests/test_sample_search_gpu.py replays it (``replay``
below, the one definition of the call) and asserts equal ids and equal probability bits.  It was recorded from the library of
the commit before the sampler body became shared code (FIRA_HIP_LIB selects the library; needs a GPU).  The one legitimate
reason to record it again is a toolchain change that moves the bits of logf / exp2f / log2f / expf on the device -- then every
draw that sits within an ulp of a threshold or of its runner-up may move.  A change of the sampler's code is not a reason: it
has to reproduce these draws.

Rows (``pinned_rows``: an integer formula, every value an integer below 2^24 times 2^-36, so the float32 bits do not depend
on numpy's version or its random streams): one all positive, the same with about 60 % of the entries zero and the former
maximum gone, one with a single positive entry, one all zero.  Geometries (vocab, sou, sub) = (7, 3, 0), (1025, 5, 4) and
(25600, 370, 654), the register-resident maximum; the rows of the two small ones are stored, the large one is rebuilt from the
formula.  Every row is drawn under 8 noise streams and at buffer offsets 0..3 (floats), i.e. at every 4-byte alignment.
Settings: plain, temperature alone, top-k, top-p, top-k + top-p, min_p, epsilon, eta, typical_p with top-k."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

GEOMETRIES = [(7, 3, 0), (1025, 5, 4), (25600, 370, 654)]
STORED = GEOMETRIES[:2]                                              # their input rows are in the fixture
FIELDS = ("temperature", "top_k", "top_p", "min_p", "epsilon", "eta", "typical_p")
DEFAULTS = dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, epsilon=0.0, eta=0.0, typical_p=1.0)
SETTINGS = [dict(), dict(temperature=1.3), dict(temperature=1.3, top_k=5), dict(temperature=0.8, top_p=0.9),
            dict(temperature=1.5, top_k=50, top_p=0.9), dict(min_p=0.02), dict(temperature=1.7, epsilon=0.002), dict(eta=0.003),
            dict(top_k=40, typical_p=0.8)]
RPC, STEP, SEED = 2, 3, 0x0BADC0FFEE123457
KEYS = [5, 40, 77, 1000003, 6, 41, 78, 1000004, 7, 42, 79, 1000005, 8, 43, 80, 1000006]   # 32 rows: row r is kind r % 4
OFFSETS = 4
PAD = 8


def _mix(i, salt):
    """A 32-bit integer hash of the uint64 array i (every product stays below 2^64)."""
    m = np.uint64(0xFFFFFFFF)
    x = (i * np.uint64(0x9E3779B1) + np.uint64(salt) * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & m
    x ^= x >> np.uint64(12)
    x = (x * np.uint64(0x297A2D39)) & m
    x ^= x >> np.uint64(15)
    return x


def pinned_rows(W):
    """[4, W] float32: positive (24-bit integers shifted right by 0..19 bits: a long tail under a few large entries), holed,
    one entry, empty."""
    i = np.arange(W, dtype=np.uint64)
    h = _mix(i, W)
    v = (((h & np.uint64(0xFFFFFF)) | np.uint64(1)) >> ((h >> np.uint64(24)) % np.uint64(20))) + np.uint64(1)
    full = v.astype(np.float32) * np.float32(2.0 ** -36)             # exact: v < 2^24 + 1
    holed = full.copy()
    holed[_mix(i, W + 1) % np.uint64(5) < 3] = 0.0
    holed[int(np.argmax(full))] = 0.0
    assert (holed > 0).sum() >= 2 and holed.max() < full.max()
    one = np.zeros(W, np.float32)
    one[(5 * W) // 7] = 0.25
    return np.stack([full, holed, one, np.zeros(W, np.float32)])


def setting_table(W):
    """[len(SETTINGS), len(FIELDS)] float64: every setting in full, top_k capped at the row's width."""
    full = [dict(DEFAULTS, **kw) for kw in SETTINGS]
    return np.array([[min(s[f], W) if f == "top_k" else s[f] for f in FIELDS] for s in full], np.float64)


def replay(geometry, rows, table, rpc, step, seed, keys):
    """fira_sample_dist on ``rows`` (the four kinds, tiled to rpc x len(keys) rows) under every setting of ``table`` at every
    offset: (best_id [OFFSETS, settings, R] int32, the bits of best_p, same shape)."""
    import torch
    from fira_icse_amd import _lib
    from fira_icse_amd.config import FiraConfig
    V, L, S = geometry
    rows = np.tile(rows, (rpc * len(keys) // len(rows), 1))
    R, W = rows.shape
    assert W == V + L + S and R == rpc * len(keys)
    d = _lib.make_dims(FiraConfig())
    d.vocab, d.sou_len, d.sub_len = V, L, S
    key = torch.tensor(keys, dtype=torch.int32, device="cuda")
    seed &= (1 << 64) - 1
    seed_dev = torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device="cuda")
    ids = np.zeros((OFFSETS, len(table), R), np.int32)
    p_bits = np.zeros_like(ids)
    for offset in range(OFFSETS):
        buf = torch.zeros(R * W + offset + PAD, dtype=torch.float32, device="cuda")
        view = buf[offset:offset + R * W].view(R, W)
        view.copy_(torch.from_numpy(rows))
        for k, s in enumerate(table):
            kw = dict(zip(FIELDS, s))
            bid = torch.full((R,), -7, dtype=torch.int32, device="cuda")
            bp = torch.full((R,), -7.0, dtype=torch.float32, device="cuda")
            _lib.check(_lib.lib().fira_sample_dist(_lib.cur_stream(), C.byref(d), R, rpc, step, _lib.ptr(view), _lib.ptr(key),
                                                   _lib.ptr(seed_dev), float(kw["temperature"]), int(kw["top_k"]), float(kw["top_p"]),
                                                   float(kw["min_p"]), float(kw["epsilon"]), float(kw["eta"]), float(kw["typical_p"]),
                                                   _lib.ptr(bid), _lib.ptr(bp)), "fira_sample_dist")
            torch.cuda.synchronize()
            ids[offset, k] = bid.cpu().numpy()
            p_bits[offset, k] = bp.cpu().numpy().view(np.int32)
    return ids, p_bits


def name(geometry):
    return "%d_%d_%d" % geometry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "sampler_draws.npz"))
    a = ap.parse_args()
    import torch
    from fira_icse_amd import _lib
    assert torch.cuda.is_available(), "record_sampler_draws.py needs a GPU"
    out = dict(rpc=np.int64(RPC), step=np.int64(STEP), seed=np.uint64(SEED), keys=np.array(KEYS, np.int32),
               fields=np.array(FIELDS), geometries=np.array(GEOMETRIES, np.int32))
    for g in GEOMETRIES:
        rows, table = pinned_rows(sum(g)), setting_table(sum(g))
        ids, p_bits = replay(g, rows, table, RPC, STEP, SEED, KEYS)
        out.update({"settings_" + name(g): table, "best_id_" + name(g): ids, "best_p_bits_" + name(g): p_bits})
        if g in STORED:
            out["rows_" + name(g)] = rows
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("recorded %d draws from %s to %s (%d bytes)" % (sum(out["best_id_" + name(g)].size for g in GEOMETRIES), _lib.LIB_PATH,
                                                          a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
