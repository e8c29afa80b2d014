"""Learning-rate schedules without a GPU: fira_lr_at against the float64 formula of include/fira_hip.h bit for bit, the shape
of each schedule, fira_lr_schedule_check, the ABI surface, and the command-line validation of run_model.py train
--lr-schedule / --warmup-steps / --lr-decay-steps / --lr-min (in the pattern of tests/test_clip_cli.py)."""
import argparse
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import util
from fira_icse_amd import _lib, ops
from run_model import check_lr_schedule_args, lr_schedule_from_args, parse_args

KINDS = ("constant", "inv_sqrt", "cosine", "linear")
BASE = 1e-3
# (W, N, min_lr)
PARAMS = [(0, 100, 0.0), (1, 2, 0.0), (4, 8, 0.1 * BASE), (4000, 100000, 1e-6), (7, 1000, 2.5e-4)]


def formula(kind, base, W, N, mn, t):
    """The definition, in float64 (Python floats), rounded to float32 once.  base / mn: the float32 values the struct holds."""
    base, mn = float(np.float32(base)), float(np.float32(mn))
    w = min(1.0, t / W) if W > 0 else 1.0
    if kind == "constant":
        r = base * w
    elif kind == "inv_sqrt":
        r = base * min(t / W, math.sqrt(W / t))
    elif t <= W:
        r = base * w
    else:
        q = min(max((t - W) / (N - W), 0.0), 1.0)
        r = mn + (base - mn) * 0.5 * (1.0 + math.cos(math.pi * q)) if kind == "cosine" else mn + (base - mn) * (1.0 - q)
    return np.float32(r)


def steps_of(W, N):
    return sorted({t for t in (1, W - 1, W, W + 1, N - 1, N, N + 1, 10 * N, 2, 3, 17) if t >= 1})


def cases(params):
    # (inv_sqrt is defined for W >= 1 only: fira_lr_schedule_check refuses W = 0)
    return [(k,) + p for k in KINDS for p in params if not (k == "inv_sqrt" and p[0] < 1)]


@pytest.mark.parametrize("kind,W,N,mn", cases(PARAMS))
def test_lr_at_equals_the_float64_formula_bit_for_bit(lib, kind, W, N, mn):
    s = _lib.LrSchedule(KINDS.index(kind), BASE, W, N, mn)
    assert lib.fira_lr_schedule_check(C.byref(s)) == 0, lib.fira_last_error()
    for t in steps_of(W, N):
        got = np.float32(lib.fira_lr_at(C.byref(s), t))
        want = formula(kind, BASE, W, N, mn, t)
        assert got.tobytes() == want.tobytes(), (kind, W, N, mn, t, float(got), float(want))
        assert ops.lr_at(s, t) == float(got)
    sched = ops.LrSchedule(kind, BASE, W, N, mn)
    assert ops.lr_at(sched, 5) == float(np.float32(lib.fira_lr_at(C.byref(s), 5)))       # the dataclass reaches the same function


@pytest.mark.parametrize("kind,W,N,mn", cases([(0, 100, 0.0), (1, 2, 0.0), (4, 8, 0.1 * BASE), (40, 300, 1e-6), (7, 1000, 2.5e-4)]))
def test_shape_of_each_schedule(lib, kind, W, N, mn):
    s = _lib.LrSchedule(KINDS.index(kind), BASE, W, N, mn)
    base32, mn32 = float(np.float32(BASE)), float(np.float32(mn))
    r = [lib.fira_lr_at(C.byref(s), t) for t in range(1, 2 * N + 50)]
    for t in range(1, len(r)):                                  # r[t - 1] = the rate of step t
        if t + 1 <= W:
            assert r[t] >= r[t - 1], (t, r[t - 1], r[t])        # non-decreasing on [1, W]
        if t >= max(W, 1):
            assert r[t] <= r[t - 1], (t, r[t - 1], r[t])        # non-increasing after
    assert all(0.0 <= x <= base32 for x in r)
    if W >= 1:
        assert r[W - 1] == base32                               # the peak, exactly, at t = W
        assert r[0] < base32 or W == 1
    if kind in ("cosine", "linear"):
        assert all(x == mn32 for x in r[N - 1:])                # min_lr, exactly, from N on
        assert r[N - 2] > mn32 or N - 1 <= W
    if kind == "constant":
        assert all(x == base32 for x in r[max(W, 1) - 1:])
    if kind == "inv_sqrt":
        assert r[4 * W - 1] == pytest.approx(base32 / 2, rel=1e-6)


def test_step_below_one_counts_as_one_and_null_gives_zero(lib):
    s = _lib.LrSchedule(2, BASE, 4, 8, 0.0)
    assert lib.fira_lr_at(C.byref(s), 0) == lib.fira_lr_at(C.byref(s), -3) == lib.fira_lr_at(C.byref(s), 1)
    assert lib.fira_lr_at(None, 5) == 0.0


@pytest.mark.parametrize("fields,msg", [
    ((4, BASE, 0, 10, 0.0), "kind 4"),
    ((-1, BASE, 0, 10, 0.0), "kind -1"),
    ((0, 0.0, 0, 0, 0.0), "base_lr must be finite and > 0"),
    ((0, -1e-3, 0, 0, 0.0), "base_lr must be finite and > 0"),
    ((0, float("nan"), 0, 0, 0.0), "base_lr must be finite and > 0"),
    ((0, float("inf"), 0, 0, 0.0), "base_lr must be finite and > 0"),
    ((0, BASE, -1, 0, 0.0), "warmup_steps must be >= 0"),
    ((1, BASE, 0, 0, 0.0), "inv_sqrt needs warmup_steps >= 1"),
    ((2, BASE, 8, 8, 0.0), "cosine needs decay_steps > warmup_steps"),
    ((3, BASE, 8, 4, 0.0), "linear needs decay_steps > warmup_steps"),
    ((2, BASE, 0, 0, 0.0), "cosine needs decay_steps > warmup_steps"),
    ((2, BASE, 2, 8, -1e-6), "min_lr must be in [0, base_lr]"),
    ((3, BASE, 2, 8, 2 * BASE), "min_lr must be in [0, base_lr]"),
    ((0, BASE, 0, 0, float("nan")), "min_lr must be in [0, base_lr]"),
])
def test_schedule_check_refuses_each_invalid_combination(lib, fields, msg):
    s = _lib.LrSchedule(*fields)
    assert lib.fira_lr_schedule_check(C.byref(s)) != 0
    assert msg in lib.fira_last_error().decode()
    with pytest.raises(ValueError, match=re.escape(msg)):
        ops.lr_schedule_check(s)


def test_schedule_check_accepts_the_valid_ones_and_null_is_refused(lib):
    for fields in ((0, BASE, 0, 0, 0.0), (0, BASE, 10, 0, 0.0), (1, BASE, 1, 0, 0.0), (2, BASE, 0, 1, 0.0), (3, BASE, 3, 4, BASE)):
        assert lib.fira_lr_schedule_check(C.byref(_lib.LrSchedule(*fields))) == 0, fields
    assert lib.fira_lr_schedule_check(None) != 0 and b"null" in lib.fira_last_error()


def test_the_dataclass_mirrors_the_struct():
    s = ops.LrSchedule.make({"kind": "inv-sqrt", "base_lr": 1e-3, "warmup_steps": 4})
    assert s == ops.LrSchedule("inv_sqrt", 1e-3, 4, 0, 0.0) and s == ops.LrSchedule.make(s) == ops.LrSchedule.make(s.as_dict())
    st = s.struct()
    assert (st.kind, st.warmup_steps, st.decay_steps, st.min_lr) == (1, 4, 0, 0.0) and st.base_lr == float(np.float32(1e-3))
    assert ops.LrSchedule.make({"kind": 2, "base_lr": 1e-3, "decay_steps": 5}).kind == "cosine"
    for bad in ({"kind": "step", "base_lr": 1e-3}, {"kind": "cosine", "base_lr": 1e-3, "decay_steps": 0},
                {"kind": "constant", "base_lr": 1e-3, "gamma": 0.5}, {"kind": "linear", "base_lr": 1e-3, "decay_steps": 4, "min_lr": 1.0}):
        with pytest.raises(ValueError):
            ops.LrSchedule.make(bad)


# ---------------------------------------------------------------------------------------------------- ABI surface
def test_header_exports_and_ctypes_table_agree_on_the_new_symbols(lib):
    header = open(os.path.join(util.REPO, "include", "fira_hip.h")).read()
    assert int(re.search(r"#define FIRA_ABI_VERSION (\d+)", header).group(1)) == 11 == lib.fira_abi_version()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("fira_lr_at", "fira_lr_schedule_check"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["fira_lr_at"][0] is C.c_float
    # the struct: five 4-byte fields in the header's order
    body = re.search(r"typedef struct fira_lr_schedule \{(.*?)\} fira_lr_schedule;", code, flags=re.S).group(1)
    names = re.findall(r"\b(?:int32_t|float)\s+(\w+)\s*;", body)
    assert names == [f[0] for f in _lib.LrSchedule._fields_] == ["kind", "base_lr", "warmup_steps", "decay_steps", "min_lr"]
    assert C.sizeof(_lib.LrSchedule) == 20
    # fira_adam_opts: one trailing pointer field; a positional AdamOpts that stops at v leaves it NULL
    body = re.search(r"typedef struct fira_adam_opts \{(.*?)\} fira_adam_opts;", code, flags=re.S).group(1)
    assert re.search(r"const\s+fira_lr_schedule\s*\*\s*sched\s*;\s*$", body.strip())
    assert [f[0] for f in _lib.AdamOpts._fields_] == ["lr", "beta1", "beta2", "eps", "step", "m", "v", "sched"]
    ad = _lib.AdamOpts(1e-3, 0.9, 0.999, 1e-8, 1, None, None)
    assert not ad.sched
    assert C.sizeof(_lib.AdamOpts) == 48 and _lib.AdamOpts.sched.offset == 40


# ---------------------------------------------------------------------------------------------------- command line
def test_default_is_no_schedule_and_values_are_parsed():
    a = parse_args(["train"])
    assert (a.lr_schedule, a.warmup_steps, a.lr_decay_steps, a.lr_min) == (None, None, None, None)
    assert lr_schedule_from_args(a, 1000) is None
    a = parse_args(["train", "--lr", "1e-3", "--lr-schedule", "cosine", "--warmup-steps", "10", "--lr-decay-steps", "200",
                    "--lr-min", "1e-5"])
    assert lr_schedule_from_args(a, 1000) == {"kind": "cosine", "base_lr": 1e-3, "warmup_steps": 10, "decay_steps": 200,
                                              "min_lr": 1e-5}
    # --lr-decay-steps defaults to the steps the run plans, counted from where a resumed state stands
    a = parse_args(["train", "--lr-schedule", "linear", "--warmup-steps", "3"])
    assert lr_schedule_from_args(a, 40)["decay_steps"] == 40 and lr_schedule_from_args(a, 40, 25)["decay_steps"] == 65
    assert lr_schedule_from_args(a, 40)["min_lr"] == 0.0
    with pytest.raises(ValueError, match="give --lr-decay-steps"):
        lr_schedule_from_args(a, 3)
    a = parse_args(["train", "--lr-schedule", "inv-sqrt", "--warmup-steps", "4000"])
    assert lr_schedule_from_args(a, 10) == {"kind": "inv_sqrt", "base_lr": 1e-4, "warmup_steps": 4000, "decay_steps": 0, "min_lr": 0.0}
    a = parse_args(["train", "--lr-schedule", "constant"])
    assert lr_schedule_from_args(a, 10)["warmup_steps"] == 0
    for d in (lr_schedule_from_args(a, 10), lr_schedule_from_args(parse_args(["train", "--lr-schedule", "cosine"]), 10)):
        ops.LrSchedule.make(d)                                   # what the driver hands the Trainer is a valid schedule


BAD_ARGV = [
    (["train", "--warmup-steps", "10"], "--warmup-steps needs --lr-schedule"),
    (["train", "--lr-decay-steps", "10"], "--lr-decay-steps needs --lr-schedule"),
    (["train", "--lr-min", "1e-5"], "--lr-min needs --lr-schedule"),
    (["train", "--lr-schedule", "constant", "--lr-decay-steps", "10"], "--lr-decay-steps has no meaning with --lr-schedule constant"),
    (["train", "--lr-schedule", "constant", "--lr-min", "1e-5"], "--lr-min has no meaning with --lr-schedule constant"),
    (["train", "--lr-schedule", "inv-sqrt", "--warmup-steps", "4", "--lr-min", "1e-5"], "--lr-min has no meaning with --lr-schedule inv-sqrt"),
    (["train", "--lr-schedule", "inv-sqrt", "--warmup-steps", "4", "--lr-decay-steps", "9"], "--lr-decay-steps has no meaning"),
    (["train", "--lr-schedule", "inv-sqrt"], "inv-sqrt needs --warmup-steps W >= 1"),
    (["train", "--lr-schedule", "inv-sqrt", "--warmup-steps", "0"], "inv-sqrt needs --warmup-steps W >= 1"),
    (["train", "--lr-schedule", "cosine", "--warmup-steps", "-1"], "--warmup-steps -1: must be >= 0"),
    (["train", "--lr-schedule", "cosine", "--warmup-steps", "8", "--lr-decay-steps", "8"], "needs N > W"),
    (["train", "--lr-schedule", "linear", "--warmup-steps", "8", "--lr-decay-steps", "4"], "needs N > W"),
    (["train", "--lr-schedule", "linear", "--lr-decay-steps", "0"], "needs N > W"),
    (["train", "--lr-schedule", "cosine", "--lr-min=-1e-6"], "--lr-min -1e-06: must be in [0, --lr"),
    (["train", "--lr", "1e-4", "--lr-schedule", "cosine", "--lr-min", "1e-3"], "--lr-min 0.001: must be in [0, --lr"),
    (["train", "--lr-schedule", "linear", "--lr-min", "nan"], "--lr-min nan: must be in [0, --lr"),
    (["train", "--lr", "0", "--lr-schedule", "constant"], "a schedule needs a finite peak rate > 0"),
    (["test", "--lr-schedule", "cosine"], "--lr-schedule only applies to the train stage"),
]


@pytest.mark.parametrize("argv,msg", BAD_ARGV)
def test_each_invalid_combination_is_refused(argv, msg, capsys):
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "error" in err and msg in err


def test_validation_function_raises_value_error():
    ns = dict(stage="train", lr=1e-4, lr_schedule=None, warmup_steps=None, lr_decay_steps=None, lr_min=None)
    check_lr_schedule_args(argparse.Namespace(**ns))
    check_lr_schedule_args(argparse.Namespace(**dict(ns, stage="test")))
    check_lr_schedule_args(argparse.Namespace(**dict(ns, lr_schedule="cosine", warmup_steps=2, lr_decay_steps=8, lr_min=1e-5)))
    for bad in (dict(warmup_steps=3), dict(lr_schedule="inv-sqrt"), dict(lr_schedule="linear", warmup_steps=5, lr_decay_steps=5),
                dict(lr_schedule="cosine", lr_min=1.0), dict(lr_schedule="constant", stage="test")):
        with pytest.raises(ValueError):
            check_lr_schedule_args(argparse.Namespace(**dict(ns, **bad)))


@pytest.mark.parametrize("argv", [["train", "--warmup-steps", "5"], ["train", "--lr-schedule", "inv-sqrt"],
                                  ["train", "--lr-schedule", "cosine", "--warmup-steps", "9", "--lr-decay-steps", "9"],
                                  ["train", "--lr-schedule", "linear", "--lr-min", "1"]])
def test_the_driver_exits_before_anything_touches_the_gpu(argv, tmp_path):
    """The whole program: a one-line error and exit status 2 from an empty directory (no DataSet, no model, no device needed)."""
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "run_model.py")] + argv, capture_output=True, text=True,
                       cwd=str(tmp_path), timeout=300)
    assert r.returncode == 2
    last = r.stderr.splitlines()[-1]
    assert ("--lr-" in last or "--warmup-steps" in last) and "Traceback" not in r.stderr


def test_help_names_the_options():
    r = subprocess.run([sys.executable, os.path.join(util.REPO, "run_model.py"), "--help"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0
    for opt in ("--lr-schedule", "--warmup-steps", "--lr-decay-steps", "--lr-min"):
        assert opt in r.stdout


def test_the_reference_fixture_records_the_library_rates(lib):
    """tests/golden/sched_ref.json was written by a Python transcription of the formula: its per-step rates are fira_lr_at's."""
    import json
    ref = json.load(open(os.path.join(util.REPO, "tests", "golden", "sched_ref.json")))
    for name, run in ref["runs"].items():
        s = ops.LrSchedule.make(run["schedule"])
        assert [ops.lr_at(s, t) for t in range(1, ref["steps"] + 1)] == run["lr"], name
        assert run["separation"] >= 2e-3 and len(run["loss_curve"]) == ref["steps"] + 1
