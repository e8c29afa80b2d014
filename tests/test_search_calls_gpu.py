"""The library calls of ONE search step, in order, with which of their pointer arguments are NULL: ``_greedy_steps``, ``_beam_steps``
and ``_sbs_steps`` at step 1 (so ``parent`` is in play) for every combination of merge_copies / prefix / constraints, a
``BeamScoring`` and a two-member ensemble.  The expected sequences are written out below: the edit order is merge, prefix,
constraints; in greedy exactly the last edit call carries best_id / best_p, in the beam family none does.  Below them the full
chain -- merge, prefix, constraints, banned phrases, template, word sets, penalties -- in ``greedy``, ``beam`` and
``sample_search``, each of the four later links alone, and ``greedy`` with a neighbour and with ``knn=``, whose mix carries the
pair only where the chain is empty."""
import pytest
import torch

import util
from search_kit import CountingLib, golden_search
from fira_icse_amd import _lib
from fira_icse_amd.config import UNK
from fira_icse_amd import retrieve
from fira_icse_amd.decode import BeamScoring, Constraints, KnnMT, Neighbour, Penalties, Phrases, Searcher, Template, WordSets

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
            "fira_constrain_dist": {13: "best_id", 14: "best_p"},
            "fira_ban_phrases_dist": {12: "best_id", 13: "best_p"},
            "fira_template_dist": {13: "best_id", 14: "best_p"},
            "fira_wordset_dist": {8: "allow", 9: "deny", 10: "boost", 11: "ground", 12: "slot_valid", 13: "boost_factor",
                                  15: "best_id", 16: "best_p"},
            "fira_penalise_dist": {13: "best_id", 14: "best_p"},
            "fira_mix_neighbour": {7: "best_id", 8: "best_p"},
            "fira_mix_knn": {10: "best_id", 11: "best_p"}}


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
    store = retrieve.TokenStore.build(Searcher(g.model), [(list(g.ids), g.db)])
    return dict(db=g.db, single=Searcher(g.model), ens=Searcher(g.model, members=(second,)), knn=KnnMT(store, k=4),
                neighbour=Neighbour(g.db, [0.5, 1.0, 0.25]))


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


# ------------------------------------------------------------------------------------------------ the full chain
BAN = Phrases(banned=[(8, 9)])                        # not in PREFIX
TEMPLATE = Template(word_class={12: 1}, next=[[0, -1]], accept=[0])       # one state, word 12 never: PREFIX is a path of it
DENY = WordSets(deny=[13])                            # no word of PREFIX
ALLOW = WordSets(allow=range(UNK, 200))               # every word of PREFIX
PENALTIES = Penalties(presence=0.5, frequency=0.25, bias={10: 1.0})
LINKS = dict(phrases=BAN, template=TEMPLATE, wordsets=DENY, penalties=PENALTIES)
ALL = dict(merge_copies=True, prefix=PREFIX, constraints=CON, **LINKS)
# the key components of the options above, as ``_key`` orders them
ALL_KEY = ("merge", "prefix", "penalties", "ban-phrases", "template", ("wordsets", ("deny",)), CON)
LINK_KEY = dict(phrases=("ban-phrases",), template=("template",), wordsets=(("wordsets", ("deny",)),), penalties=("penalties",))

ONLY_DENY = ("allow", "boost", "ground", "slot_valid", "boost_factor")
ONLY_ALLOW = ("deny", "boost", "ground", "slot_valid", "boost_factor")
BAN_PHRASES, BAN_PHRASES_BEST = ("fira_ban_phrases_dist", NO_BEST), ("fira_ban_phrases_dist", ())
TEMPLATE_DIST, TEMPLATE_BEST = ("fira_template_dist", NO_BEST), ("fira_template_dist", ())
WORDSET_DENY, WORDSET_DENY_BEST = ("fira_wordset_dist", ONLY_DENY + NO_BEST), ("fira_wordset_dist", ONLY_DENY)
WORDSET_ALLOW_BEST = ("fira_wordset_dist", ONLY_ALLOW)
PENALISE, PENALISE_BEST = ("fira_penalise_dist", NO_BEST), ("fira_penalise_dist", ())
MIX_NEIGHBOUR, MIX_NEIGHBOUR_BEST = ("fira_mix_neighbour", NO_BEST), ("fira_mix_neighbour", ())
MIX_KNN, MIX_KNN_BEST = ("fira_mix_knn", NO_BEST), ("fira_mix_knn", ())
HIDDEN, KNN_SEARCH = ("fira_decode_hidden", ()), ("fira_knn_search", ())
SAMPLE_DIST, SAMPLE_ADVANCE = ("fira_sample_dist", ()), ("fira_sample_advance", ())

GREEDY_ALL = [G_STEP_DIST, MERGE, FORCE, CONSTRAIN, BAN_PHRASES, TEMPLATE_DIST, WORDSET_DENY, PENALISE_BEST, ADVANCE]
GREEDY_LINK = {"phrases": [G_STEP_DIST, BAN_PHRASES_BEST, ADVANCE],
               "template": [G_STEP_DIST, TEMPLATE_BEST, ADVANCE],
               "wordsets": [G_STEP_DIST, WORDSET_DENY_BEST, ADVANCE],
               "penalties": [G_STEP_DIST, PENALISE_BEST, ADVANCE]}
GREEDY_ALLOW = [G_STEP_DIST, WORDSET_ALLOW_BEST, ADVANCE]
BEAM_ALL = [PREPARE, B_STEP, MERGE, FORCE, CONSTRAIN, BAN_PHRASES, TEMPLATE_DIST, WORDSET_DENY, PENALISE, SELECT]
SAMPLE_SEARCH_ALL = [G_STEP_DIST, MERGE, FORCE, CONSTRAIN, BAN_PHRASES, TEMPLATE_DIST, WORDSET_DENY, PENALISE, SAMPLE_DIST,
                     SAMPLE_ADVANCE]
# a neighbour: the input's step, the neighbour's, the neighbour's row folded into words, the mix; knn=: the step, the hidden rows,
# the look-up, the mix.  The mix carries the arg-max only where no edit follows.
NEIGHBOUR_GREEDY = {"": [G_STEP_DIST, G_STEP_DIST, MERGE, MIX_NEIGHBOUR_BEST, ADVANCE],
                    "c": [G_STEP_DIST, G_STEP_DIST, MERGE, MIX_NEIGHBOUR, CONSTRAIN_BEST, ADVANCE]}
KNN_GREEDY = {"": [G_STEP_DIST, HIDDEN, KNN_SEARCH, MIX_KNN_BEST, ADVANCE],
              "c": [G_STEP_DIST, HIDDEN, KNN_SEARCH, MIX_KNN, CONSTRAIN_BEST, ADVANCE]}


def greedy_step_of(monkeypatch, search, db, key, ws_key=(B, 1), **kw):
    """``greedy_step`` for any options: ``key`` is the state's key after ("greedy", B), ``ws_key`` what ``_begin`` returned."""
    search.greedy(db, use_graphs=False, **kw)
    st, ws = search._ws[("greedy", B) + key], search._ws[ws_key]
    search._greedy_reset(st)
    search._greedy_steps(st, ws, B, 0, 1)
    return one_step(monkeypatch, lambda: search._greedy_steps(st, ws, B, 1, 2))


def test_greedy_full_chain_step(setup, monkeypatch):
    got = greedy_step_of(monkeypatch, setup["single"], setup["db"], ALL_KEY, **ALL)
    print(got)
    assert got == GREEDY_ALL


@pytest.mark.parametrize("link", list(GREEDY_LINK))
def test_greedy_one_link_step(setup, monkeypatch, link):
    got = greedy_step_of(monkeypatch, setup["single"], setup["db"], LINK_KEY[link], **{link: LINKS[link]})
    print(link, got)
    assert got == GREEDY_LINK[link]


def test_greedy_allow_alone_gets_null_for_the_other_sets(setup, monkeypatch):
    got = greedy_step_of(monkeypatch, setup["single"], setup["db"], (("wordsets", ("allow",)),), wordsets=ALLOW)
    print(got)
    assert got == GREEDY_ALLOW


def test_beam_full_chain_step(setup, monkeypatch):
    search, db, beam = setup["single"], setup["db"], 3
    search.beam(db, beam, use_graphs=False, **ALL)
    st, ws = search._ws[("beam", B, beam) + ALL_KEY], search._ws[(B, beam)]
    search._beam_reset(st, B, beam)
    search._beam_steps(st, ws, B, beam, 0, 1)
    got = one_step(monkeypatch, lambda: search._beam_steps(st, ws, B, beam, 1, 2))
    print(got)
    assert got == BEAM_ALL


def test_sample_search_full_chain_step(setup, monkeypatch):
    search, db, n = setup["single"], setup["db"], 2
    search.sample_search(db, n, seed=3, use_graphs=False, **ALL)
    st, ws = search._ws[("sample_search", B, n, 1.0, 0, 1.0) + Searcher.CUTS_OFF + ALL_KEY], search._ws[(B, n)]
    steps = lambda lo, hi: search._sample_search_steps(st, ws, B, n, lo, hi, 1.0, 0, 1.0, Searcher.CUTS_OFF)
    search._sample_reset(st)
    steps(0, 1)
    got = one_step(monkeypatch, lambda: steps(1, 2))
    print(got)
    assert got == SAMPLE_SEARCH_ALL


@pytest.mark.parametrize("flags", list(NEIGHBOUR_GREEDY), ids=[f or "bare" for f in NEIGHBOUR_GREEDY])
def test_greedy_neighbour_step(setup, monkeypatch, flags):
    key = ("neighbour",) + ((CON,) if flags else ())
    got = greedy_step_of(monkeypatch, setup["single"], setup["db"], key, ("neighbours", B, 1), neighbour=setup["neighbour"],
                         constraints=CON if flags else None)
    print(flags or "bare", got)
    assert got == NEIGHBOUR_GREEDY[flags]


@pytest.mark.parametrize("flags", list(KNN_GREEDY), ids=[f or "bare" for f in KNN_GREEDY])
def test_greedy_knn_step(setup, monkeypatch, flags):
    kn = setup["knn"]
    key = (("knn", kn.k, id(kn.store)),) + ((CON,) if flags else ())
    got = greedy_step_of(monkeypatch, setup["single"], setup["db"], key, ("knn", B, 1, kn.k, id(kn.store)), knn=kn,
                         constraints=CON if flags else None)
    print(flags or "bare", got)
    assert got == KNN_GREEDY[flags]
