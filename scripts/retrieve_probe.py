"""Times of retrieval-augmented search, one JSON line each:

  nn_search   fira_nn_search over N = 75 000 unit vectors at B = 20 and B = 64 against ``(Q @ store.T).max(1)`` in torch on the
              same box, interleaved, with min / median over the repetitions and the share of the 77 MB pass in the HBM peak;
  beam_step   a beam-3 search per step at batch 20 with and without a neighbour (synthetic commits, untrained weights).

``python scripts/retrieve_probe.py [--reps 30] [--n 75000]``.  There is no pass / fail figure."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

HBM_PEAK = 8.0e12                                  # bytes / s, the data sheet's figure


def timed(fn, reps):
    """Device times of ``fn`` in microseconds, one event pair per repetition."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def summary(ts):
    return {"min_us": round(min(ts), 2), "median_us": round(statistics.median(ts), 2), "max_us": round(max(ts), 2)}


def probe_search(N, reps):
    from fira_icse_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    store = torch.nn.functional.normalize(torch.randn((N, 256), device="cuda", generator=g), dim=1).contiguous()
    for B in (20, 64):
        Q = torch.nn.functional.normalize(store[:B] + 0.01 * torch.randn((B, 256), device="cuda", generator=g), dim=1).contiguous()
        kernel = lambda: ops.nn_search(Q, store)
        stmt = lambda: (Q @ store.T).max(1)
        for f in (kernel, stmt):
            f()
        torch.cuda.synchronize()
        tk, tt = [], []
        for _ in range(reps):                      # interleaved: both see the same clocks and cache state
            tk += timed(kernel, 1)
            tt += timed(stmt, 1)
        idx, _ = kernel()
        agree = bool((idx.long() == stmt().indices).all())
        nbytes = N * 256 * 4
        print(json.dumps({"probe": "nn_search", "N": N, "B": B, "store_MB": round(nbytes / 1e6, 1), "kernel": summary(tk),
                          "torch": summary(tt), "same_argmax": agree,
                          "kernel_share_of_hbm_peak": round(nbytes / (min(tk) * 1e-6) / HBM_PEAK, 3),
                          "torch_share_of_hbm_peak": round(nbytes / (min(tt) * 1e-6) / HBM_PEAK, 3)}), flush=True)


def probe_beam(reps):
    from fira_icse_amd import data, synth
    from fira_icse_amd.config import FiraConfig
    from fira_icse_amd.decode import Neighbour, Searcher
    from fira_icse_amd.model import DeviceBatch, TransModel, reference_init_state_dict
    cfg = FiraConfig()
    store = data.process_raw(cfg, synth.generate_dataset(40, seed=5))
    torch.manual_seed(0)
    model = TransModel(cfg, init=False)
    model.load_state_dict(reference_init_state_dict(cfg))
    model.eval()
    db, nb_db = DeviceBatch(store.batch(list(range(20))), cfg), DeviceBatch(store.batch(list(range(20, 40))), cfg)
    search = Searcher(model)
    nb = Neighbour(nb_db, [0.8] * 20, lam=1.0)
    steps = cfg.tar_len - 1
    plain = lambda: search.beam(db, 3)
    mixed = lambda: search.beam(db, 3, neighbour=nb)
    for f in (plain, mixed):
        f()
    torch.cuda.synchronize()
    tp, tm = [], []
    for _ in range(reps):
        tp += timed(plain, 1)
        tm += timed(mixed, 1)
    # (the whole call: encoder pass(es), reset and the chunks the search runs before every hypothesis has ended)
    print(json.dumps({"probe": "beam_step", "batch": 20, "beam": 3, "steps_at_most": steps, "plain_call": summary(tp),
                      "neighbour_call": summary(tm), "ratio_of_medians": round(statistics.median(tm) / statistics.median(tp), 3)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--n", type=int, default=75000)
    a = ap.parse_args()
    probe_search(a.n, a.reps)
    probe_beam(max(3, a.reps // 3))


if __name__ == "__main__":
    main()
