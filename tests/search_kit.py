"""Shared helpers of the search tests (tests/test_*_gpu.py and their CPU-side companions): the golden model setup, the kernel
launch scaffolding and the comparisons every search is held to.  One definition each; util.py holds the training side's.  A
plain module: it registers nothing with pytest, and every fixture that uses it stays in its own test module."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

import util
from fira_icse_amd import _lib
from fira_icse_amd.config import FiraConfig


# ------------------------------------------------------------------------------------------------ the golden setup
def spread_state_dict(cfg, seed=2):
    """Weights whose step distributions have real spread (the peaked fixture weights put ~all mass on one entry)."""
    from fira_icse_amd.model import reference_init_state_dict
    torch.manual_seed(0)
    sd = util.perturb_state_dict(reference_init_state_dict(cfg), seed=seed)
    sd["out_fc.weight"] = sd["out_fc.weight"] * 10.0
    sd["copy_net.LinearRes.weight"] = sd["copy_net.LinearRes.weight"] * 6.0
    return sd


def golden_search(tar_len=None, weights="init", searchers=1, batch=util.GOLDEN_B, **weight_kwargs):
    """The golden synthetic commits (the first ``batch`` of the test split) under one freshly built model.  ``weights``: "init"
    (the seeded initialisation under torch seed 0), "perturb" / "peaked" / "tie" (util.py's functions of it, ``weight_kwargs``
    = their seed) or "spread".  Returns cfg, store, ids, idx, state_dict, model, host_batch, db and ``searchers`` fresh
    Searchers of the model.  Call it from a module-scoped fixture: the tests read the Searchers' private caches."""
    from fira_icse_amd import data
    from fira_icse_amd.decode import Searcher
    from fira_icse_amd.model import DeviceBatch, TransModel, reference_init_state_dict
    cfg = FiraConfig() if tar_len is None else FiraConfig(tar_len=tar_len)
    store = data.process_raw(cfg, util.load_golden_raw())
    idx = data.split_index(*util.GOLDEN_SPLIT, seed=0)
    ids = idx["test"][:batch]
    torch.manual_seed(0)
    if weights == "spread":
        sd = spread_state_dict(cfg, **weight_kwargs)
    else:
        sd = reference_init_state_dict(cfg)
        if weights != "init":
            sd = {"perturb": util.perturb_state_dict, "peaked": util.peaked_state_dict, "tie": util.tie_state_dict}[weights](
                sd, **weight_kwargs)
    model = TransModel(cfg, init=False)
    model.load_state_dict(sd)
    model.eval()
    hb = store.batch(ids)
    return types.SimpleNamespace(cfg=cfg, store=store, ids=ids, idx=idx, state_dict=sd, model=model, host_batch=hb,
                                 db=DeviceBatch(hb, cfg), searchers=[Searcher(model) for _ in range(searchers)])


def dims_of(cfg):
    return cfg.vocab_size, cfg.sou_len, cfg.sub_token_len


def device_dims(vocab=None, sou_len=None, sub_len=None, tar_len=None):
    """The library's dims of ``FiraConfig()`` with the given fields overwritten (None: the configuration's own)."""
    d = _lib.make_dims(FiraConfig())
    for k, v in dict(vocab=vocab, sou_len=sou_len, sub_len=sub_len, tar_len=tar_len).items():
        if v is not None:
            setattr(d, k, v)
    return d


# ------------------------------------------------------------------------------------------------ comparisons
def bits(x):
    """The int32 view of a floating tensor or array, for bit-for-bit comparison (integers compare exactly as they are)."""
    x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return x.contiguous().view(torch.int32) if x.is_floating_point() else x


def same_search(got, want):
    """The equality test_decode_gpu.py holds ``beam`` to against ``beam_torch``: lengths and probabilities equal (as values
    and as bits), ids equal inside the lengths."""
    (gen, length, p), (gen_t, len_t, p_t) = [tuple(t.cpu() for t in x[:3]) for x in (got, want)]
    assert torch.equal(length, len_t)
    assert torch.equal(p, p_t) and torch.equal(bits(p), bits(p_t))
    live = torch.arange(gen.shape[-1])[(None,) * (gen.dim() - 1)] < length[..., None]
    assert torch.equal(gen * live, gen_t * live)


def messages(gen, length):
    gen, length = gen.cpu().reshape(-1, gen.shape[-1]).tolist(), length.cpu().reshape(-1).tolist()
    return [row[1:n] for row, n in zip(gen, length)]


def seed_tensor(seed):
    seed &= (1 << 64) - 1
    return torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device="cuda")


def last_error():
    return _lib.lib().fira_last_error().decode()


# ------------------------------------------------------------------------------------------------ rows at every alignment
PAD_FLOATS = 8


def offset_rows(values, offset, fill=0.0, device="cuda"):
    """``values`` [R, W] ``offset`` floats into a buffer of ``fill`` with PAD_FLOATS behind (rows then begin at every
    alignment); returns (buffer, view)."""
    n = values.size
    buf = torch.full((n + offset + PAD_FLOATS,), fill, dtype=torch.float32, device=device)
    view = buf[offset:offset + n].view(values.shape)
    view.copy_(torch.from_numpy(values))
    return buf, view


def outside_untouched(buf, offset, n, fill=0.0):
    """Asserts that nothing outside the ``n`` floats of the rows was written."""
    assert bool((buf[:offset] == fill).all()) and bool((buf[offset + n:] == fill).all())
    return True


def best_pair(n_rows, want=True):
    """The two outputs of a row arg-max, filled with -7, or (None, None)."""
    if not want:
        return None, None
    return (torch.full((n_rows,), -7, dtype=torch.int32, device="cuda"),
            torch.full((n_rows,), -7.0, dtype=torch.float32, device="cuda"))


# ------------------------------------------------------------------------------------------------ library calls
class CountingLib:
    """Stands in for the loaded library: counts the calls of every entry by name."""

    def __init__(self, real):
        self.real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def count_calls(monkeypatch, run):
    lib = CountingLib(_lib.lib())
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "_lib", lib)
        run()
    torch.cuda.synchronize()
    return lib.calls


# ------------------------------------------------------------------------------------------------ command line
def run_cli(args, cwd, timeout=600):
    """run_model.py in a fresh process; asserts that it succeeded and returns the finished process (stdout, stderr)."""
    env = dict(os.environ, PYTHONPATH=util.REPO)
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "run_model.py")] + args, cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r
