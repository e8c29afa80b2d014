"""The library calls of ONE search step, in order, with which of their pointer arguments are NULL: ``_greedy_steps``, ``_beam_steps``
and ``_sbs_steps`` at step 1 (so ``parent`` is in play) for every combination of merge_copies / prefix / constraints, a
``BeamScoring`` and a two-member ensemble.  The expected sequences are written out below: the edit order is merge, prefix,
constraints; in greedy exactly the last edit call carries best_id / best_p, in the beam family none does."""
import pytest
import torch

import util
from search_kit import CountingLib, golden_search
from fira_icse_amd import _lib
from fira_icse_amd.config import UNK
from fira_icse_amd.decode import BeamScoring, Constraints, Searcher

pytestmark = pytest.mark.gpu

B = 3
CON = Constraints(2, 3, (UNK,))
PREFIX = [[5, 6], [], [7]]
SCORING = BeamScoring(1.0, groups=2, diversity=0.5)
TEMPERATURE = 1.25

# the pointer arguments of an entry that may be NULL, by position
NULLABLE = {"fira_decode_step_ex": {9: "parent", 10: "dist", 11: "best_id", 12: "best_p"},
            "fira_mix_dist": {7: "best_id", 8: "best_p"},
            "fira_merge_dist": {7: "best_id", 8: "best_p"},
            "fira_force_dist": {11: "best_id", 12: "best_p"},
            "fira_constrain_dist": {13: "best_id", 14: "best_p"}}


class RecordingLib(CountingLib):
    """``CountingLib`` that also keeps, per call and in order, (entry name, names of the arguments that are NULL)."""

    def __init__(self, real):
        super().__init__(real)
        self.log = []

    def __getattr__(self, name):
        counted = super().__getattr__(name)

        def recorded(*args):
            names = NULLABLE.get(name, {})
            self.log.append((name, tuple(names.get(i, "arg%d" % i) for i, a in enumerate(args) if a is None)))
            return counted(*args)
        return recorded


def one_step(monkeypatch, run):
    lib = RecordingLib(_lib.lib())
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "_lib", lib)
        run()
    torch.cuda.synchronize()
    assert sum(lib.calls.values()) == len(lib.log)
    return lib.log


@pytest.fixture(scope="module")
def setup():
    """The model of test_merge_gpu.py's setup (the perturbed seeded initialisation) and the first three of its commits; a second
    model (seed 2) for the ensemble."""
    from fira_icse_amd.model import TransModel, reference_init_state_dict
    g = golden_search(weights="perturb", searchers=0, batch=B, seed=1)
    torch.manual_seed(0)
    second = TransModel(g.cfg, init=False)
    second.load_state_dict(util.perturb_state_dict(reference_init_state_dict(g.cfg), seed=2))
    second.eval()
    return dict(db=g.db, single=Searcher(g.model), ens=Searcher(g.model, members=(second,)))


def options(flags):
    return dict(merge_copies="m" in flags, prefix=PREFIX if "p" in flags else None, constraints=CON if "c" in flags else None)


def greedy_step(monkeypatch, search, db, flags):
    """The state of a real eager ``greedy`` call, reset, step 0 unrecorded, step 1 recorded."""
    search.greedy(db, use_graphs=False, **options(flags))
    st = search._ws[Searcher._key(("greedy", B), "m" in flags, CON if "c" in flags else None, forced="p" in flags)]
    ws = search._ws[("members", B, 1) if search.members else (B, 1)]
    search._greedy_reset(st)
    search._greedy_steps(st, ws, B, 0, 1)
    return one_step(monkeypatch, lambda: search._greedy_steps(st, ws, B, 1, 2))


def beam_step(monkeypatch, search, db, beam, flags, scoring=None):
    search.beam(db, beam, use_graphs=False, scoring=scoring, **options(flags))
    st = search._ws[Searcher._key(("beam", B, beam), "m" in flags, CON if "c" in flags else None, scoring, "p" in flags)]
    ws = search._ws[("members", B, beam) if search.members else (B, beam)]
    search._beam_reset(st, B, beam)
    search._beam_steps(st, ws, B, beam, 0, 1)
    return one_step(monkeypatch, lambda: search._beam_steps(st, ws, B, beam, 1, 2))


def sbs_step(monkeypatch, search, db, n, flags):
    search.sample_distinct(db, n, temperature=TEMPERATURE, merge_copies="m" in flags, constraints=CON if "c" in flags else None,
                           use_graphs=False)
    st = search._ws[("sbs", B, n, "m" in flags, CON if "c" in flags else None, TEMPERATURE)]
    ws = search._ws[(B, n)]
    search._sbs_reset(st, B, n)
    search._sbs_steps(st, ws, B, n, 0, 1, TEMPERATURE)
    return one_step(monkeypatch, lambda: search._sbs_steps(st, ws, B, n, 1, 2, TEMPERATURE))


NO_BEST = ("best_id", "best_p")
# greedy never passes a parent; the beam family does from step 1 on
G_STEP_FUSED = ("fira_decode_step_ex", ("parent", "dist"))                 # no distribution: the step's own arg-max
G_STEP_DIST = ("fira_decode_step_ex", ("parent",) + NO_BEST)               # the distribution, no arg-max
B_STEP = ("fira_decode_step_ex", NO_BEST)
MERGE, MERGE_BEST = ("fira_merge_dist", NO_BEST), ("fira_merge_dist", ())
FORCE, FORCE_BEST = ("fira_force_dist", NO_BEST), ("fira_force_dist", ())
CONSTRAIN, CONSTRAIN_BEST = ("fira_constrain_dist", NO_BEST), ("fira_constrain_dist", ())
MIX, MIX_BEST = ("fira_mix_dist", NO_BEST), ("fira_mix_dist", ())
ADVANCE, PREPARE = ("fira_greedy_advance", ()), ("fira_beam_prepare", ())
SELECT, SELECT_SCORED, SELECT_GUMBEL = ("fira_beam_select", ()), ("fira_beam_select_scored", ()), ("fira_beam_select_gumbel", ())

GREEDY = {"": [G_STEP_FUSED, ADVANCE],
          "m": [G_STEP_DIST, MERGE_BEST, ADVANCE],
          "p": [G_STEP_DIST, FORCE_BEST, ADVANCE],
          "c": [G_STEP_DIST, CONSTRAIN_BEST, ADVANCE],
          "mp": [G_STEP_DIST, MERGE, FORCE_BEST, ADVANCE],
          "mc": [G_STEP_DIST, MERGE, CONSTRAIN_BEST, ADVANCE],
          "pc": [G_STEP_DIST, FORCE, CONSTRAIN_BEST, ADVANCE],
          "mpc": [G_STEP_DIST, MERGE, FORCE, CONSTRAIN_BEST, ADVANCE]}

BEAM = {"": [PREPARE, B_STEP, SELECT],
        "m": [PREPARE, B_STEP, MERGE, SELECT],
        "p": [PREPARE, B_STEP, FORCE, SELECT],
        "c": [PREPARE, B_STEP, CONSTRAIN, SELECT],
        "mpc": [PREPARE, B_STEP, MERGE, FORCE, CONSTRAIN, SELECT]}

BEAM_SCORED = {"": [PREPARE, B_STEP, SELECT_SCORED],
               "mpc": [PREPARE, B_STEP, MERGE, FORCE, CONSTRAIN, SELECT_SCORED]}

SBS = {"": [PREPARE, B_STEP, SELECT_GUMBEL],
       "m": [PREPARE, B_STEP, MERGE, SELECT_GUMBEL],
       "c": [PREPARE, B_STEP, CONSTRAIN, SELECT_GUMBEL],
       "mc": [PREPARE, B_STEP, MERGE, CONSTRAIN, SELECT_GUMBEL]}

# two members: every step becomes two (no arg-max from either), one mix follows; the mix reports the arg-max in plain greedy only
ENSEMBLE_GREEDY = {"": [G_STEP_DIST, G_STEP_DIST, MIX_BEST, ADVANCE],
                   "mpc": [G_STEP_DIST, G_STEP_DIST, MIX, MERGE, FORCE, CONSTRAIN_BEST, ADVANCE]}
ENSEMBLE_BEAM = {"mpc": [PREPARE, B_STEP, B_STEP, MIX, MERGE, FORCE, CONSTRAIN, SELECT]}


@pytest.mark.parametrize("flags", list(GREEDY), ids=[f or "plain" for f in GREEDY])
def test_greedy_step(setup, monkeypatch, flags):
    got = greedy_step(monkeypatch, setup["single"], setup["db"], flags)
    print(flags or "plain", got)
    assert got == GREEDY[flags]


@pytest.mark.parametrize("flags", list(BEAM), ids=[f or "plain" for f in BEAM])
def test_beam_step(setup, monkeypatch, flags):
    got = beam_step(monkeypatch, setup["single"], setup["db"], 3, flags)
    print(flags or "plain", got)
    assert got == BEAM[flags]


@pytest.mark.parametrize("flags", list(BEAM_SCORED), ids=[f or "plain" for f in BEAM_SCORED])
def test_scored_beam_step(setup, monkeypatch, flags):
    got = beam_step(monkeypatch, setup["single"], setup["db"], 4, flags, SCORING)
    print(flags or "plain", got)
    assert got == BEAM_SCORED[flags]


@pytest.mark.parametrize("flags", list(SBS), ids=[f or "plain" for f in SBS])
def test_sample_distinct_step(setup, monkeypatch, flags):
    got = sbs_step(monkeypatch, setup["single"], setup["db"], 2, flags)
    print(flags or "plain", got)
    assert got == SBS[flags]
    assert all(name != "fira_force_dist" for name, _ in got)


def test_ensemble_steps(setup, monkeypatch):
    ens, db = setup["ens"], setup["db"]
    for flags, want in ENSEMBLE_GREEDY.items():
        got = greedy_step(monkeypatch, ens, db, flags)
        print("greedy", flags or "plain", got)
        assert got == want
    for flags, want in ENSEMBLE_BEAM.items():
        got = beam_step(monkeypatch, ens, db, 3, flags)
        print("beam3", flags or "plain", got)
        assert got == want
