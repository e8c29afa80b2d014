"""Seconds per batch of MBR selection by expected sentence BLEU: `Searcher.mbr` against the host string loop, same process,
interleaved, on the same sampled candidates.

    python scripts/mbr_probe.py [--batch 64] [--reps 7] [--out profiles/mbr_probe.md]

The commits are synthetic (synth.py) and the weights the seeded initialisation with a sharpened generator, so the candidates
are what an untrained model draws: mostly full-length messages without <eos> -- the string work per pair is then at its LONGEST.
Two sizes: n = 8 (one `sample` call, what `run_model.py test --sample 8 --rerank mbr_bleu` does per batch) and n = 32 (four
`sample` calls with different seeds pooled along n, the kernel's limit).  Per repetition, in this order: the `sample` call(s)
that produce the candidates, `Searcher.mbr` as a whole, its three parts apart (the kernel over `--launches` back-to-back
launches between two synchronisations, the copy of the statistics, forming utilities and pick on the host), and the host loop
(`text.detokenize` -> `split` -> `metrics.sentence_bleu_method2` for all ordered pairs, `math.fsum` mean, `metrics.mbr_pick`).
Two warm-up repetitions are thrown away.  Medians, min and max over the rest."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from fira_icse_amd import data, metrics, ops, synth, text   # noqa: E402
from fira_icse_amd.config import FiraConfig                 # noqa: E402
from fira_icse_amd.decode import Searcher                   # noqa: E402
from fira_icse_amd.model import DeviceBatch, TransModel     # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def host_loop(toks, lens, logp, r_vocab, var_maps):
    """What the selection costs without the kernel: every candidate to text and back to words, all ordered pairs scored."""
    toks, lens, logp = toks.tolist(), lens.tolist(), logp.tolist()
    util = []
    for b, var_map in enumerate(var_maps):
        ws = [text.detokenize(row[:n], r_vocab, var_map).split() for row, n in zip(toks[b], lens[b])]
        n = len(ws)
        util.append([math.fsum(metrics.sentence_bleu_method2([ws[j]], ws[i]) for j in range(n) if j != i) / (n - 1)
                     if n > 1 else 0.0 for i in range(n)])
    return metrics.mbr_pick(util, logp), util


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50, help="kernel launches inside one timed window")
    ap.add_argument("--temperature", type=float, default=1.2)
    ap.add_argument("--top-k", type=int, default=30)
    ap.add_argument("--out", default=None, help="append the result as markdown to this file")
    a = ap.parse_args()
    assert a.reps >= 5
    B = a.batch
    cfg = FiraConfig()
    raw = synth.generate_dataset(B, seed=5)
    store = data.process_raw(cfg, raw)
    r_vocab = {i: w for w, i in raw["word_vocab"].items()}
    var_maps = [raw["variable"][i] for i in range(B)]
    torch.manual_seed(0)
    model = TransModel(cfg)
    with torch.no_grad():                                    # candidates that share words: a sharper generator
        sd = model.state_dict()
        sd["out_fc.weight"] = sd["out_fc.weight"] * 10.0
        model.load_state_dict(sd)
    model.eval()
    search = Searcher(model)
    db = DeviceBatch(store.batch(list(range(B))), cfg)
    blocks = []
    for n, draws in ((8, 1), (32, 4)):
        def sample_all():
            parts = [search.sample(db, 8, temperature=a.temperature, top_k=a.top_k, seed=11 + d) for d in range(draws)]
            return tuple(torch.cat([p[k] for p in parts], 1) for k in (0, 1, 3))

        t = {k: [] for k in ("sample", "mbr", "kernel", "copy", "form", "host")}
        same = True
        for rep in range(a.reps + 2):
            dt_sample, (toks, lens, logp) = timed(sample_all)
            dt_mbr, (pick, util) = timed(lambda: search.mbr(toks, lens, logp))
            t32, l32 = toks.to(torch.int32).contiguous(), lens.to(torch.int32).contiguous()
            stats = ops.mbr_bleu_stats(t32, l32)

            def launches():
                for _ in range(a.launches):
                    ops.mbr_bleu_stats(t32, l32, stats)

            dt_kernel, _ = timed(launches)
            dt_copy, host_stats = timed(stats.cpu)
            t0 = time.perf_counter()
            util2 = metrics.mbr_utilities(host_stats)
            pick2 = metrics.mbr_pick(util2, logp.cpu())
            dt_form = time.perf_counter() - t0
            t0 = time.perf_counter()
            h_pick, h_util = host_loop(toks, lens, logp, r_vocab, var_maps)
            dt_host = time.perf_counter() - t0
            same &= h_pick == pick == pick2 and h_util == util.tolist() == util2
            if rep >= 2:
                for k, v in (("sample", dt_sample), ("mbr", dt_mbr), ("kernel", dt_kernel / a.launches), ("copy", dt_copy),
                             ("form", dt_form), ("host", dt_host)):
                    t[k].append(v)
        med = {k: statistics.median(v) for k, v in t.items()}
        words = [len(text.detokenize(row[:k], r_vocab, var_maps[b]).split())
                 for b in range(B) for row, k in zip(toks[b].tolist(), lens[b].tolist())]
        n_zero = sum(u == 0.0 for row in util.tolist() for u in row)
        names = (("sample", "`Searcher.sample`, %d call%s of 8" % (draws, "" if draws == 1 else "s")),
                 ("mbr", "`Searcher.mbr` (launch + copy + host forming)"),
                 ("kernel", "  kernel alone (mean of %d back-to-back launches)" % a.launches),
                 ("copy", "  copy of the statistics to the host (%.1f kB)" % (B * n * n * 48 / 1e3)),
                 ("form", "  utilities and pick on the host (`mbr_utilities`, `mbr_pick`)"),
                 ("host", "host loop: detokenize, split, %d x `sentence_bleu_method2`" % (B * n * (n - 1))))
        rows = ["| part | median ms | min ms | max ms |", "|---|---|---|---|"]
        for k, name in names:
            rows.append("| %s | %.3f | %.3f | %.3f |" % (name, 1e3 * med[k], 1e3 * min(t[k]), 1e3 * max(t[k])))
        blocks += [
            "### B = %d commits, n = %d candidates (T = %d), %d repetitions after 2 warm-ups, %s" % (
                B, n, cfg.tar_len, a.reps, torch.cuda.get_device_name(0)),
            "",
            "candidates: %.1f words on average (max %d); utilities equal to 0: %d of %d; picks and utilities identical (`==`) "
            "between `Searcher.mbr` and the host loop in every repetition: %s" % (
                sum(words) / len(words), max(words), n_zero, B * n, same),
            "",
        ] + rows + [
            "",
            "host loop / `Searcher.mbr`: %.1fx; `Searcher.mbr` is %.2f %% and the host loop %.1f %% of the time of the `sample` "
            "call%s beside it" % (med["host"] / med["mbr"], 100.0 * med["mbr"] / med["sample"],
                                  100.0 * med["host"] / med["sample"], "" if draws == 1 else "s"),
            "",
        ]
    out = "\n".join(blocks)
    print(out, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
