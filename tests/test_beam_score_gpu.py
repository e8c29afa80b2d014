"""fira_beam_select_scored alone on synthetic states, against fira_beam_select (bit identity at alpha = 0 in one group) and against
the numpy statement beamscore_ref.py: exact order on inputs whose keys are separated, validity without exclusions on random
inputs, a penalty that dominates the key range, and the argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import beamscore_ref as R
from search_kit import device_dims
from fira_icse_amd import _lib
from fira_icse_amd.config import EOS, START

pytestmark = pytest.mark.gpu

SMALL = dict(vocab=37, sou_len=6, sub_len=5, tar_len=8)            # W = 48
MODEL = {}                                                          # the reference geometry (FiraConfig's own dims)


def geometry(geo):
    d = device_dims(**geo)
    return d.vocab, d.sou_len, d.sub_len, d.tar_len


def make_state(rng, geo, B, beam, finished=0.35, inactive_slot=None, max_len=None, zero_prob=0.15):
    """A consistent search state: hypotheses <start> w .. [<eos>], finished = last id is <eos>; active[j] = some commit still runs
    in slot j (active[8] = their number), as fira_beam_prepare leaves it."""
    V, L, S, T = geometry(geo)
    max_len = max_len or T - 2
    gen = np.zeros((B, beam, T), dtype=np.int32)
    length = rng.randint(1, max_len + 1, size=(B, beam)).astype(np.int32)
    fin = np.zeros((B, beam), dtype=np.int32)
    for b in range(B):
        for j in range(beam):
            n = length[b, j]
            gen[b, j, 0] = START
            gen[b, j, 1:n] = rng.randint(3, V, size=n - 1)
            if n >= 2 and (rng.rand() < finished or j == inactive_slot):
                gen[b, j, n - 1] = EOS
                fin[b, j] = 1
            elif j == inactive_slot:                               # (a one-id hypothesis cannot be finished: make it two)
                length[b, j] = 2
                gen[b, j, 1] = EOS
                fin[b, j] = 1
    prob = rng.uniform(0.05, 1.0, size=(B, beam)).astype(np.float32)
    prob[rng.rand(B, beam) < zero_prob] = 0.0
    active = np.zeros(9, dtype=np.int32)
    active[:beam] = (fin == 0).any(0)
    active[8] = active[:beam].sum()
    sou = rng.randint(3, V, size=(B, L)).astype(np.int32)
    sub = rng.randint(3, V, size=(B, S)).astype(np.int32)
    return dict(geo=geo, B=B, beam=beam, gen=gen, length=length, fin=fin, prob=prob, active=active, sou=sou, sub=sub, done=0)


def launch(st, dist, scored, inv_lp=None, groups=1, lam=0.0, want_key=True):
    dev = "cuda"
    B, beam = st["B"], st["beam"]
    V, L, S, T = geometry(st["geo"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gen, length, prob, fin, active = t(st["gen"].reshape(B * beam, T)), t(st["length"].reshape(-1)), t(st["prob"].reshape(-1)), \
        t(st["fin"].reshape(-1)), t(st["active"])
    done = torch.tensor([st["done"]], dtype=torch.int32, device=dev)
    sou, sub, dist_d = t(st["sou"]), t(st["sub"]), t(dist.reshape(B * beam, -1))
    g_out = torch.full_like(gen, -7)
    l_out, p_out, parent = torch.full_like(length, -7), torch.full_like(prob, -7.0), torch.full_like(length, -7)
    key = torch.full_like(prob, -7.0) if scored and want_key else None
    dd = device_dims(**st["geo"])
    args = (_lib.cur_stream(), C.byref(dd), B, beam, _lib.ptr(dist_d), _lib.ptr(fin), _lib.ptr(active), _lib.ptr(done), _lib.ptr(sou),
            _lib.ptr(sub), _lib.ptr(gen), _lib.ptr(length), _lib.ptr(prob), _lib.ptr(g_out), _lib.ptr(l_out), _lib.ptr(p_out),
            _lib.ptr(parent))
    if scored:
        inv_d = t(np.asarray(inv_lp, dtype=np.float32))
        _lib.check(_lib.lib().fira_beam_select_scored(*args, _lib.ptr(inv_d), groups, float(lam), _lib.ptr(key)), "fira_beam_select_scored")
    else:
        _lib.check(_lib.lib().fira_beam_select(*args), "fira_beam_select")
    torch.cuda.synchronize()
    return g_out.cpu(), l_out.cpu(), p_out.cpu(), parent.cpu(), None if key is None else key.cpu()


def per_commit(st, out, b):
    """The outputs of commit b as check_step / apply name them (parent as a slot of the commit)."""
    beam = st["beam"]
    g, l, p, parent, key = out
    rows = slice(b * beam, (b + 1) * beam)
    return (g[rows].numpy().astype(np.int64), l[rows].numpy().astype(np.int64), p[rows].numpy(), parent[rows].numpy() - b * beam,
            None if key is None else key[rows].numpy())


def words_of(st, b):
    return R.words_of(st["sou"][b], st["sub"][b], geometry(st["geo"])[0])


# ------------------------------------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("geo, beam", [(SMALL, 2), (SMALL, 3), (SMALL, 5), (SMALL, 8), (MODEL, 3), (MODEL, 8)],
                         ids=["small-2", "small-3", "small-5", "small-8", "model-3", "model-8"])
def test_alpha_zero_one_group_is_beam_select_bit_for_bit(geo, beam):
    rng = np.random.RandomState(beam)
    V, L, S, T = geometry(geo)
    ones = np.ones(T + 1, dtype=np.float32)
    for case in ("mixed", "inactive", "done", "start"):
        st = make_state(rng, geo, 3, beam, inactive_slot=1 if case == "inactive" else None)
        if case == "start":                                        # the reset state: slot 0 at 1, the others at 0
            st = make_state(rng, geo, 3, beam, finished=0.0, max_len=1, zero_prob=0.0)
            st["prob"][:] = 0
            st["prob"][:, 0] = 1
        st["done"] = int(case == "done")
        assert case != "inactive" or st["active"][1] == 0
        assert case != "mixed" or (st["fin"].any() and not st["fin"].all())
        dist = rng.uniform(1e-6, 1.0, size=(3, beam, V + L + S)).astype(np.float32)
        dist[:, :, ::7] = dist[:, :, 3:4]                          # equal values: the index decides
        want = launch(st, dist, scored=False)
        got = launch(st, dist, scored=True, inv_lp=ones, groups=1, lam=0.0)
        for a, b, name in zip(got[:4], want[:4], ("gen", "len", "prob", "parent")):
            assert torch.equal(a, b), (case, name)
        got_nokey = launch(st, dist, scored=True, inv_lp=ones, want_key=False)
        assert all(torch.equal(a, b) for a, b in zip(got_nokey[:4], want[:4])), case
        # key_out = ln(prob_out): -inf at 0
        p = got[2].double()
        ref = torch.where(p > 0, torch.log(p.clamp(min=1e-300)), torch.full_like(p, float("-inf")))
        assert torch.equal(torch.isinf(got[4]), torch.isinf(ref)) and float((got[4].double() - ref).nan_to_num(0, 0, 0).abs().max()) <= R.TOL


# ------------------------------------------------------------------------------------------------ exact order, separated keys
POOL = list(range(20, 30))                                         # the words the spikes resolve to: few, so groups collide
W0 = 20                                                            # group 0's best word; later groups meet it in a copy slot only
GAP = 0.05
STEP_GROUPED = 0.45                                                # key levels of a grouped case: -0.3 - 0.45 n, n = 0, 1, ...
LAM_SEPARATED = STEP_GROUPED * (1 + 1 / 8)                         # c penalties move a key by 0.45 (c + c / 8): for c, c' in 0..7 two
                                                                   # penalised keys differ by a multiple of 0.45 or by >= 0.45 / 8 > GAP


def separated_case(beam, groups, alpha, seed):
    """Rows of 1e-30 with twelve spikes each, laid out on distinct key levels (one group: 0.3 apart and jittered; groups: on the
    grid of STEP_GROUPED, see LAM_SEPARATED), slot probabilities and lengths mixed in, so that the float64 penalised keys of a
    group's candidates differ by >= GAP (asserted by the caller on the reference).
    Group 0's best candidate is generator entry W0; in the rows of every later group W0 has NO generator spike, but the copy slot
    V + 2 (sou id W0) carries the group's best unpenalised key."""
    geo = SMALL
    V, L, S, T = geometry(geo)
    rng = np.random.RandomState(seed)
    B, k = 2, beam // groups
    st = make_state(rng, geo, B, beam, finished=0.3, max_len=5, zero_prob=0.0)
    st["sou"][:] = rng.choice(POOL[1:], size=(B, L))
    st["sub"][:] = rng.choice(POOL[1:], size=(B, S))
    st["sou"][:, 2] = W0
    inv = R.inv_lp_table(alpha, T)
    dist = np.full((B, beam, V + L + S), 1e-30, dtype=np.float32)
    for b in range(B):
        for g in range(groups):
            slots = [j for j in range(g * k, g * k + k)]
            running = [j for j in slots if not st["fin"][b, j] and st["active"][j]]
            n_cand = 12 * len(running) + (k - len(running))
            if groups == 1:
                levels = -0.3 - 0.3 * rng.permutation(np.arange(1, n_cand + 1)) - rng.uniform(0, 0.1, size=n_cand)
            else:
                levels = -0.3 - STEP_GROUPED * rng.permutation(np.arange(1, n_cand + 1))
            levels = list(levels)
            for j in slots:                                        # the carried hypotheses take a level too
                if st["fin"][b, j]:
                    st["prob"][b, j] = np.float32(np.exp(levels.pop() / inv[st["length"][b, j] - 1]))
            for n, j in enumerate(running):
                m = st["length"][b, j]
                top = V + 2 if g > 0 else W0
                gens = [w for w in rng.choice(POOL[1:], size=7, replace=False)]
                slots_ = [V + s for s in rng.choice([s for s in range(L + S) if s != 2], size=4, replace=False)]
                entries = ([top] if n == 0 else [int(rng.choice([w for w in POOL[1:] if w not in gens]))]) + gens + slots_
                for i, e in enumerate(entries):
                    key = -0.3 if (n == 0 and i == 0) else levels.pop()
                    dist[b, j, e] = np.float32(np.exp(key / inv[m]) / st["prob"][b, j])
    return st, dist, inv


def reference_step(st, dist, inv, groups, lam):
    out = []
    for b in range(st["B"]):
        picks = R.select(dist[b], st["fin"][b], st["active"], st["prob"][b], st["length"][b], words_of(st, b), inv, groups, lam)
        out.append((picks, R.apply(picks, st["gen"][b].astype(np.int64), st["length"][b].astype(np.int64), inv)))
    return out


def assert_separated(st, dist, inv, groups, lam):
    """On the float64 reference alone: within every group the penalised keys of all candidates above the 1e-30 floor differ
    pairwise by >= GAP, and there are at least k of them."""
    beam = st["beam"]
    k = beam // groups
    for b in range(st["B"]):
        counts = {}
        picks = R.select(dist[b], st["fin"][b], st["active"], st["prob"][b], st["length"][b], words_of(st, b), inv, groups, lam)
        for g in range(groups):
            c = R.group_candidates(dist[b], st["fin"][b], st["active"], st["prob"][b], st["length"][b], words_of(st, b), inv, g, k,
                                   lam, counts)
            real = ~c["void"] & (c["p"] > 1e-25)
            keys = np.sort(c["pkey"][real])[::-1]
            if len(keys) < k or not (np.diff(keys) <= -GAP).all():
                return False
            assert all(pk["p"] > 1e-25 for pk in picks[g * k:g * k + k])
            for pk in picks[g * k:g * k + k]:
                if not pk["carry"]:
                    counts[pk["word"]] = counts.get(pk["word"], 0) + 1
    return True


@pytest.mark.parametrize("alpha", [0.6, 1.0, 2.0])
@pytest.mark.parametrize("beam, groups", [(4, 2), (6, 3), (8, 8), (3, 3), (4, 1)])
def test_separated_keys_give_exactly_the_reference(beam, groups, alpha):
    lam = LAM_SEPARATED if groups > 1 else 0.0
    def penalty_matters(want, plain):
        """In some commit group 0 appends W0 through its generator entry, a later group would append it through the copy slot
        V + 2 without the penalty, and with the penalty the picks differ."""
        for (picks, _), (picks0, _) in zip(want, plain):
            if (picks0[0]["entry"] == W0 and any(p["entry"] == SMALL["vocab"] + 2 and p["word"] == W0 for p in picks0[beam // groups:])
                    and [p["entry"] for p in picks] != [p["entry"] for p in picks0]):
                return True
        return False

    for seed in range(200):                                        # the first layout that qualifies (decided on the reference only)
        st, dist, inv = separated_case(beam, groups, alpha, 1000 * beam + seed)
        if not assert_separated(st, dist, inv, groups, lam):
            continue
        want = reference_step(st, dist, inv, groups, lam)
        if groups == 1 or penalty_matters(want, reference_step(st, dist, inv, groups, 0.0)):
            break
    else:
        pytest.fail("no separated layout found")
    assert assert_separated(st, dist, inv, groups, lam)            # the gap, on the float64 reference, before the launch
    got = launch(st, dist, scored=True, inv_lp=inv, groups=groups, lam=lam)
    for b, (picks, (g_w, l_w, p_w, parent_w, key_w)) in enumerate(want):
        g, l, p, parent, key = per_commit(st, got, b)
        assert parent.tolist() == parent_w.tolist(), (b, parent, parent_w)
        assert l.tolist() == l_w.tolist() and (g == g_w).all(), b
        assert p.tobytes() == p_w.tobytes(), b
        assert np.abs(key.astype(np.float64) - key_w).max() <= R.TOL


# ------------------------------------------------------------------------------------------------ validity, random inputs
def random_rows(rng, shape):
    """Dirichlet-like rows with exact zeros and runs of equal values."""
    x = rng.gamma(0.3, size=shape)
    x /= x.sum(-1, keepdims=True)
    x = x.astype(np.float32)
    x[rng.rand(*shape) < 0.1] = 0.0
    q = rng.rand(*shape) < 0.2
    x[q] = np.round(x[q] * 64) / 64                                # many equal values, many zeros
    return x


@pytest.mark.parametrize("beam, groups, alpha, lam", [(4, 2, 0.7, 0.5), (6, 3, 1.0, 2.0), (8, 8, 0.0, 1.0), (8, 2, 2.0, 0.5),
                                                      (3, 3, 0.6, 2.0), (5, 1, 1.5, 0.0), (8, 4, 4.0, 0.25), (2, 2, 1.0, 1.0)])
def test_random_inputs_every_pick_is_valid(beam, groups, alpha, lam):
    rng = np.random.RandomState(100 * beam + groups)
    V, L, S, T = geometry(SMALL)
    inv = R.inv_lp_table(alpha, T)
    for rep in range(3):
        st = make_state(rng, SMALL, 3, beam, inactive_slot=1 if rep == 2 else None)
        st["sou"][:] = rng.randint(3, 12, size=st["sou"].shape)     # copy slots collide with each other and with generator ids
        st["sub"][:] = rng.randint(3, 12, size=st["sub"].shape)
        dist = random_rows(rng, (3, beam, V + L + S))
        got = launch(st, dist, scored=True, inv_lp=inv, groups=groups, lam=lam)
        for b in range(3):
            R.check_step(dist[b], st["fin"][b], st["active"], st["prob"][b], st["length"][b], st["gen"][b].astype(np.int64),
                         words_of(st, b), inv, groups, lam, per_commit(st, got, b))


def test_random_inputs_reference_geometry():
    rng = np.random.RandomState(7)
    V, L, S, T = geometry(MODEL)
    beam, groups, alpha, lam = 8, 4, 1.0, 0.5
    inv = R.inv_lp_table(alpha, T)
    st = make_state(rng, MODEL, 2, beam)
    st["sou"][:] = rng.randint(3, 40, size=st["sou"].shape)
    st["sub"][:] = rng.randint(3, 40, size=st["sub"].shape)
    dist = random_rows(rng, (2, beam, V + L + S))
    got = launch(st, dist, scored=True, inv_lp=inv, groups=groups, lam=lam)
    for b in range(2):
        R.check_step(dist[b], st["fin"][b], st["active"], st["prob"][b], st["length"][b], st["gen"][b].astype(np.int64),
                     words_of(st, b), inv, groups, lam, per_commit(st, got, b))


# ------------------------------------------------------------------------------------------------ a penalty above the key range
def test_dominating_penalty_gives_pairwise_distinct_words():
    """Four groups of one slot at step 0 (every slot seeded at 1, all rows equal), lam = 512 > 104 = the whole key range of fp32.
    The four largest entries -- generator 9 and three copy slots with id 9 -- are one word: each later group must leave it."""
    V, L, S, T = geometry(SMALL)
    rng = np.random.RandomState(5)
    st = make_state(rng, SMALL, 2, 4, finished=0.0, max_len=1, zero_prob=0.0)
    st["prob"][:] = 1.0
    st["sou"][:] = rng.randint(10, V, size=st["sou"].shape)
    st["sub"][:] = rng.randint(10, V, size=st["sub"].shape)
    st["sou"][:, 1] = st["sou"][:, 4] = st["sub"][:, 3] = 9
    row = rng.uniform(1e-4, 0.05, size=(2, 1, V + L + S)).astype(np.float32)
    row[:, :, V + 1], row[:, :, 9], row[:, :, V + 4], row[:, :, V + L + 3] = 0.4, 0.3, 0.25, 0.2
    dist = np.repeat(row, 4, axis=1)
    inv = R.inv_lp_table(1.0, T)
    got = launch(st, dist, scored=True, inv_lp=inv, groups=4, lam=512.0)
    for b in range(2):
        g, l, p, parent, key = per_commit(st, got, b)
        words = g[:, 1].tolist()
        assert words[0] == 9 and p[0] == np.float32(0.4) and len(set(words)) == 4, words
        assert parent.tolist() == [0, 1, 2, 3] and l.tolist() == [2, 2, 2, 2]
        R.check_step(dist[b], st["fin"][b], st["active"], st["prob"][b], st["length"][b], st["gen"][b].astype(np.int64),
                     words_of(st, b), inv, 4, 512.0, (g, l, p, parent, key))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw, word", [
    (dict(beam=1, groups=1), "n_beam"), (dict(beam=4, groups=3), "n_groups"), (dict(lam=-1.0), "diversity"),
    (dict(lam=float("nan")), "diversity"), (dict(lam=float("inf")), "diversity"), (dict(geo=dict(SMALL, tar_len=65)), "tar_len"),
])
def test_refusals_return_non_zero_with_a_message(kw, word):
    rng = np.random.RandomState(0)
    geo = kw.get("geo", SMALL)
    beam = kw.get("beam", 4)
    st = make_state(rng, geo, 1, beam)
    V, L, S, T = geometry(geo)
    dist = np.ones((1, beam, V + L + S), dtype=np.float32)
    with pytest.raises(Exception) as e:
        launch(st, dist, scored=True, inv_lp=np.ones(T + 1, dtype=np.float32), groups=kw.get("groups", 2), lam=kw.get("lam", 0.5))
    assert "fira_beam_select_scored" in str(e.value) and word in str(e.value), str(e.value)
