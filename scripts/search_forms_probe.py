"""Every form of the device searches on a fixed seeded model and batch, written to a file, so that two trees (a refactor of
``decode.py`` and its parent commit) can be compared bit for bit.

    python scripts/search_forms_probe.py --out this.pt [--tree DIR]       # run the forms of the tree DIR (default: this one)
    python scripts/search_forms_probe.py --compare parent.pt this.pt      # torch.equal on every tensor; exit 1 on a difference

The forms: ``greedy`` with every combination of merge_copies / prefix / constraints, ``beam`` 3 plain, with each flag alone and
with all three, ``beam`` 4 under a ``BeamScoring`` (alone and with all three), ``sample_distinct`` n = 2 with and without
merge_copies and constraints, a two-member ensemble's ``greedy`` and ``beam`` 3 (plain and with all three) -- each with captured
graphs (twice: capture, then replay) and eager -- then ``sample``, ``score`` and ``greedy_many`` over three batches with two in
flight.  Two weight sets: the seeded initialisation (mass spread over the entries, so merge and constraints change the messages;
short messages) and the same with a sharpened generator (every search runs its tar_len - 1 steps).  Then the later controls
(``control_forms``): ``greedy``, ``beam`` 3 and ``sample_search`` n = 2 with penalties, banned phrases, a template and word sets
(allow, boost and ground), each alone and all of them with merge, prefix and constraints; ``beam`` 4 with ``require=`` and with
required items; ``greedy`` and ``beam`` 3 with a ``Neighbour`` and with a ``KnnMT`` over a token store built from the probe's own
batches, bare and with merge and constraints; ``greedy_many`` with per-batch word sets and prefixes.  The controls' values are
derived from the plain greedy messages, so that they bite; the output says how many of these forms differ from their plain
form.  Only public methods are called, so the file runs unchanged against an older tree.  Float tensors are compared through
their bits."""
import argparse
import itertools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
B = 4


def forms(search, ens, db, prefix, con, scoring):
    """(name, call) of every form; a call takes use_graphs and returns a tuple of tensors."""
    out = []
    for merge, forced, c in itertools.product((False, True), repeat=3):
        kw = dict(merge_copies=merge, prefix=prefix if forced else None, constraints=con if c else None)
        tag = "".join(f for f, on in zip("mpc", (merge, forced, c)) if on) or "plain"
        out.append(("greedy/" + tag, lambda g, kw=kw: search.greedy(db, use_graphs=g, **kw)))
        if merge + forced + c in (0, 1, 3):
            out.append(("beam3/" + tag, lambda g, kw=kw: search.beam(db, 3, use_graphs=g, **kw)))
        if merge + forced + c in (0, 3):
            out.append(("beam4-scored/" + tag, lambda g, kw=kw: search.beam(db, 4, use_graphs=g, scoring=scoring, **kw)))
            out.append(("ensemble-greedy/" + tag, lambda g, kw=kw: ens.greedy(db, use_graphs=g, **kw)))
            out.append(("ensemble-beam3/" + tag, lambda g, kw=kw: ens.beam(db, 3, use_graphs=g, **kw)))
        if not forced:
            out.append(("sbs2/" + tag, lambda g, m=merge, c=c: search.sample_distinct(
                db, 2, seed=7, temperature=1.25, merge_copies=m, constraints=con if c else None, use_graphs=g)))
    out.append(("sample3", lambda g: search.sample(db, 3, temperature=0.9, top_k=50, top_p=0.95, seed=(1 << 63) + 5, use_graphs=g)))
    return out


def control_forms(decode, search, db, dbs, prefix, con, knn, w, pair):
    """(name, plain form it is counted against, call) of the forms with the later controls.  ``w``: a word the plain greedy
    search writes, in no prefix: the hard controls take it away, the soft ones make it unlikely; ``pair``: two words it writes
    one after the other, the banned phrase."""
    V = search.cfg.vocab_size
    taken = {x for row in prefix for x in row}
    alone = dict(
        penalties=decode.Penalties(presence=2.0, frequency=0.5, bias={w: -8.0}),
        phrases=decode.Phrases(banned=[pair, (20, 21)]),
        template=decode.Template(word_class={w: 1}, next=[[0, -1]], accept=[0]),
        wordsets=decode.WordSets(allow=[x for x in range(3, V) if x != w], boost=[30, 31, 32], boost_bias=2.0,
                                 ground=[x for x in range(4, V) if x % 7 == 0 and x not in taken]))
    every = dict(merge_copies=True, prefix=prefix, constraints=con, **alone)
    mc = dict(merge_copies=True, constraints=con)
    nb = decode.Neighbour(dbs[1], [0.9, 0.5, 0.0, 1.0], lam=1.0)
    searches = (("greedy", "greedy/plain", lambda g, **kw: search.greedy(db, use_graphs=g, **kw)),
                ("beam3", "beam3/plain", lambda g, **kw: search.beam(db, 3, use_graphs=g, **kw)),
                ("sample_search2", "sample_search2/plain",
                 lambda g, **kw: search.sample_search(db, 2, temperature=0.9, top_k=50, seed=11, use_graphs=g, **kw)))
    out = [("sample_search2/plain", None, lambda g: searches[2][2](g)),
           ("beam4/plain", None, lambda g: search.beam(db, 4, use_graphs=g))]
    for tag, plain, call in searches:
        for name, kw in [(k, {k: v}) for k, v in alone.items()] + [("every", every)]:
            out.append(("%s/%s" % (tag, name), plain, lambda g, call=call, kw=kw: call(g, **kw)))
    out.append(("beam4/require", "beam4/plain", lambda g: search.beam(db, 4, use_graphs=g, require=[[20, 21], [], [22], []])))
    out.append(("beam4/require-phrases", "beam4/plain", lambda g: search.beam(
        db, 4, use_graphs=g, phrases=decode.Phrases(required=[[(20, 21)], [], [(22,)], []]))))
    for tag, plain, call in searches[:2]:
        for name, kw in (("neighbour", dict(neighbour=nb)), ("knn", dict(knn=knn))):
            out.append(("%s/%s" % (tag, name), plain, lambda g, call=call, kw=kw: call(g, **kw)))
            out.append(("%s/%s-mc" % (tag, name), plain, lambda g, call=call, kw=kw: call(g, **kw, **mc)))
    return out, alone["wordsets"]


def run(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from fira_icse_amd import data, decode, retrieve, synth
    from fira_icse_amd.config import EOS, START, UNK, FiraConfig
    from fira_icse_amd.decode import BeamScoring, Constraints, Searcher
    from fira_icse_amd.model import DeviceBatch, TransModel
    assert os.path.abspath(decode.__file__).startswith(os.path.abspath(a.tree) + os.sep), decode.__file__
    cfg = FiraConfig()
    store = data.process_raw(cfg, synth.generate_dataset(3 * B, seed=5))
    dbs = [DeviceBatch(store.batch(list(range(k * B, (k + 1) * B))), cfg) for k in range(3)]
    db = dbs[0]
    con, scoring = Constraints(2, 3, (UNK,)), BeamScoring(1.0, groups=2, diversity=0.5)
    prefix = [[5, 6], [], [7], [9, 11, 5]]
    cand = torch.tensor([[[START, 5 + b, 9, 11, EOS, 0], [START, 7, 6 + b, EOS, 0, 0]] for b in range(B)])
    cpu = lambda ts: [t.detach().cpu().clone() for t in ts]
    res, differ, counted = {}, [], 0
    for weights in ("init", "sharp"):
        models = []
        for seed in (0, 1):
            torch.manual_seed(seed)
            m = TransModel(cfg)
            if weights == "sharp":
                with torch.no_grad():
                    sd = m.state_dict()
                    sd["out_fc.weight"] = sd["out_fc.weight"] * 10.0
                    m.load_state_dict(sd)
            m.eval()
            models.append(m)
        search, ens = Searcher(models[0]), Searcher(models[0], members=(models[1],), weights=(0.75, 0.25))
        for name, call in forms(search, ens, db, prefix, con, scoring):
            for mode, g in (("capture", True), ("replay", True), ("eager", False)):
                res["%s/%s/%s" % (weights, name, mode)] = cpu(call(g))
        for mode, g in (("capture", True), ("replay", True), ("eager", False)):
            sc = search.score(db, cand, use_graphs=g)
            res["%s/score/%s" % (weights, mode)] = cpu(sc[k] for k in sorted(sc))
        for tag, kw in (("plain", {}), ("mpc", dict(merge_copies=True, constraints=con, prefix=[prefix, None, prefix]))):
            many = search.greedy_many(dbs, in_flight=2, **kw)
            torch.cuda.synchronize()
            res["%s/greedy_many/%s" % (weights, tag)] = cpu(t for r in many for t in r)
        # the later controls, on values that bite: w is the first word plain greedy writes that no prefix holds
        taken = {x for row in prefix for x in row}
        msgs = res["%s/greedy/plain/eager" % weights][0].tolist()
        w = next((x for row in msgs for x in row[1:] if x > UNK and x not in taken), 12)
        pair = next(((x, y) for row in msgs for x, y in zip(row[1:], row[2:]) if x > UNK and y > UNK and x not in taken), (w, w))
        store_ = retrieve.TokenStore.build(Searcher(models[0]), [(list(range(k * B, (k + 1) * B)), d) for k, d in enumerate(dbs)])
        knn = decode.KnnMT(store_, k=4, lam=0.5, temperature=10.0)
        more, wst = control_forms(decode, search, db, dbs, prefix, con, knn, w, pair)
        for name, plain, call in more:
            for mode, g in (("capture", True), ("replay", True), ("eager", False)):
                res["%s/%s/%s" % (weights, name, mode)] = cpu(call(g))
            if plain is not None:
                counted += 1
                one, two = res["%s/%s/eager" % (weights, name)], res["%s/%s/eager" % (weights, plain)]
                if not torch.equal(one[0], two[0]):
                    differ.append("%s/%s" % (weights, name))
        many = search.greedy_many(dbs, in_flight=2, wordsets=[wst, None, decode.WordSets(deny=[w])],
                                  prefix=[prefix, None, prefix])
        torch.cuda.synchronize()
        name = "%s/greedy_many/wordsets-prefix" % weights
        res[name] = cpu(t for r in many for t in r)
        counted += 1
        if not all(torch.equal(x, y) for x, y in zip(res[name], res["%s/greedy_many/plain" % weights])):
            differ.append(name)
        print("%s: %d forms so far (w = %d, pair = %r)" % (weights, len(res), w, pair), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    torch.save(res, a.out)
    print("wrote %d forms, %d tensors to %s" % (len(res), sum(len(v) for v in res.values()), a.out))
    print("%d of the %d forms with the later controls differ from their plain form" % (len(differ), counted))


def same(x, y):
    import torch
    if x.dtype != y.dtype or x.shape != y.shape:
        return False
    if x.is_floating_point():
        ints = {4: torch.int32, 8: torch.int64}[x.element_size()]
        x, y = x.contiguous().view(ints), y.contiguous().view(ints)
    return torch.equal(x, y)


def compare(a):
    import torch
    one, two = (torch.load(p) for p in a.compare)
    bad = sorted(set(one) ^ set(two))
    n = 0
    for name in sorted(set(one) & set(two)):
        n += len(one[name])
        if len(one[name]) != len(two[name]) or not all(same(x, y) for x, y in zip(one[name], two[name])):
            bad.append(name)
    print("%d forms, %d tensors compared; %d forms differ%s" % (len(set(one) & set(two)), n, len(bad), ": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="where the returned tensors of every form go (torch.save)")
    ap.add_argument("--tree", default=REPO, help="the checkout whose package is probed (its library built)")
    ap.add_argument("--compare", nargs=2, metavar="FILE", help="compare two files written with --out")
    a = ap.parse_args()
    if a.compare:
        return compare(a)
    assert a.out, "--out FILE"
    return run(a)


if __name__ == "__main__":
    sys.exit(main())
