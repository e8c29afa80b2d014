#!/usr/bin/env python
"""Drop-in for the reference driver: ``python run_model.py train`` / ``python run_model.py test``
(reference run_model.py:417-425), running on the MI355X engine.

Kept from the reference: the positional ``train|test`` stage, every path relative to the working directory
(``DataSet/*.json``, ``VOCAB_UPPER_CASE``, ``all_index``, ``best_model.pt`` = ``torch.save(state_dict)`` with the
reference's 338 keys, ``OUTPUT/train_process``, ``OUTPUT/dev_output``, ``OUTPUT/output_fira``), the hyper-parameters of
its ``args`` dict as defaults, seed 0, the order in which the global RNGs are consumed (split shuffle, weight
initialisation, per-epoch DataLoader permutation), dev-BLEU checkpoint selection from epoch 15 every 10 batches, and
beam search with the reference's scoring quirks at test time.

New (all optional): overrides for what the reference hard-codes (``--batch-size``, ``--splits``, ``--epochs``,
``--beam``, ...), and multi-GPU through one process per GPU (``torchrun --nproc-per-node N run_model.py train``):
commits of the global batch are sharded over ranks and gradients all-reduced over RCCL, instead of the reference's
single-process ``nn.DataParallel``.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import random
import sys
import time

# The search keeps several batches in flight, each on its own HIP stream (decode.Searcher.greedy_many); HIP multiplexes streams
# onto GPU_MAX_HW_QUEUES hardware queues (default 4), and two lanes that land on one queue run one after the other: four lanes
# took 0.38 ms per batch-step on 4 queues and 0.14 on 8 (profiles/r6_probes.md).  Read by the HIP runtime when it initialises,
# so it is set before torch is imported; training is unaffected (same-box triple).  An exported value wins.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from fira_icse_amd import data, text                               # noqa: E402
from fira_icse_amd.config import EOS, PAD, START, UNK, FiraConfig                 # noqa: E402
from fira_icse_amd.parallel import gather_lines, init_from_env, shard_indices   # noqa: E402
from fira_icse_amd.prefetch import prefetch                        # noqa: E402


def seed_everything(seed=0):
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def parse_args(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("stage", choices=["train", "test"])
    ap.add_argument("--root", default=".", help="directory holding DataSet/, VOCAB_UPPER_CASE, all_index (default: cwd)")
    ap.add_argument("--splits", default=None, help="train,valid,test sizes (reference hard-codes 75000,8000,7661)")
    ap.add_argument("--batch-size", type=int, default=None, help="GLOBAL train batch (reference: 170 x n_gpu)")
    ap.add_argument("--test-batch-size", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=150)
    ap.add_argument("--beam", type=int, default=None, help="beam size of the test-time search (default 3; 1 with --sample)")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--dev-from-epoch", type=int, default=15)
    ap.add_argument("--dev-every", type=int, default=10)
    ap.add_argument("--dev-on-device", action="store_true", help="train: score the dev passes on the device -- the valid split "
                    "stays resident in HBM, sentence-BLEU statistics come from a kernel on token ids, one copy back per pass, and "
                    "the dev_output text is only built for a new best; train_process, dev_output and the chosen checkpoint are "
                    "identical to a run without it")
    ap.add_argument("--max-steps", type=int, default=0, help="stop after this many optimisation steps (0 = no limit)")
    ap.add_argument("--no-dropout", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--loss-log", default=None, help="write one JSON line per optimisation step: the train-split positions "
                    "of the global batch and its mean token loss (synchronises every step, like run_model.py:112 does)")
    ap.add_argument("--save-optimizer", action="store_true", help="also write fira_train_state.pt (Adam moments, step)")
    ap.add_argument("--resume", action="store_true", help="start from best_model.pt (+ fira_train_state.pt if present)")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32", help="arithmetic of the nn.Linear products: f32 = "
                    "the reference's (fp32 MFMA, default); bf16 = BASELINE configs[2] (bf16 MFMA, fp32 accumulate; master "
                    "weights, LayerNorm, soft-max, loss and Adam stay fp32).  Applies to train and dev (teacher-forced BLEU); the test-time "
                    "SEARCH always runs the reference's fp32 arithmetic (decode.Searcher / fira_decode_step), whatever --dtype says")
    ap.add_argument("--grad-wire", choices=["auto", "f32", "bf16"], default="auto", help="multi-GPU, all-reduce path: wire format "
                    "of the gradient buckets; auto = bf16 with --dtype bf16 (half the bytes on xGMI; Adam, master weights and the "
                    "token normaliser stay fp32), else f32")
    ap.add_argument("--zero1", action="store_true", help="multi-GPU: reduce-scatter + Adam on the owned shard + all-gather "
                    "(Adam moments sharded over the ranks) instead of all-reduce + replicated Adam")
    ap.add_argument("--sample", type=int, default=None, metavar="N", help="test: draw N (1-8) candidate messages per commit "
                    "on the device instead of searching; writes OUTPUT/output_fira (the candidate of highest log-probability) "
                    "and OUTPUT/output_fira_samples (one JSON line per commit: the N candidates and their log-probabilities)")
    ap.add_argument("--temperature", type=float, default=None, help="with --sample: temperature > 0 (default 1)")
    ap.add_argument("--top-k", type=int, default=None, help="with --sample: keep the k most probable entries (default 0 = off)")
    ap.add_argument("--top-p", type=float, default=None, help="with --sample: nucleus mass in (0, 1] (default 1 = off)")
    ap.add_argument("--sample-seed", type=int, default=None, help="with --sample: seed of the sampling noise (default 0)")
    ap.add_argument("--min-p", type=float, default=None, metavar="X", help="with --sample: keep the entries at least X times as "
                    "probable as the most probable one, 0 <= X < 1 (default 0 = off); like the three options below a cut of "
                    "the tempered distribution that --top-k and --top-p left, renormalised; every cut keeps the maximum")
    ap.add_argument("--epsilon-cutoff", type=float, default=None, metavar="E", help="with --sample: epsilon sampling -- keep "
                    "the entries of probability >= E, 0 <= E < 1 (default 0 = off); the candidate generator to pair with "
                    "--rerank mbr_bleu")
    ap.add_argument("--eta-cutoff", type=float, default=None, metavar="E", help="with --sample: eta sampling -- keep the "
                    "entries of probability >= min(E, sqrt(E) * exp(-entropy)), 0 <= E < 1 (default 0 = off)")
    ap.add_argument("--typical-p", type=float, default=None, metavar="P", help="with --sample: locally typical sampling -- keep "
                    "the entries whose surprise is nearest the entropy until they hold P of the mass, 0 < P <= 1 (default 1 = "
                    "off); combines with --temperature and --top-k, not with --top-p, --min-p, --epsilon-cutoff, --eta-cutoff")
    ap.add_argument("--without-replacement", action="store_true", help="with --sample: draw the N candidates WITHOUT "
                    "replacement by stochastic beam search on the device -- N distinct messages for the cost of one beam "
                    "search, the first an ordinary sample; implies --merge-copies; combines with --temperature, --sample-seed, "
                    "--no-repeat-ngram, --min-length, --ban-words, --ensemble and --rerank, not with --top-k / --top-p; every "
                    "line of OUTPUT/output_fira_samples then carries the candidates' keys under \"key\", best first")
    ap.add_argument("--score", default=None, metavar="refs|PATH", help="test: instead of searching, score given messages "
                    "teacher-forced on the device: 'refs' = the test split's own messages, PATH = a file with one line per test "
                    "commit in all_index['test'] order (plain text as in OUTPUT/output_fira, or the JSON lines of "
                    "OUTPUT/output_fira_samples with up to 8 candidates); writes OUTPUT/output_fira_scores and prints the "
                    "corpus perplexity")
    ap.add_argument("--rerank", default=None, choices=RERANK_KEYS, help="with --sample: score the drawn candidates in the same "
                    "run and write the best one under this key to OUTPUT/output_fira (default: the candidate of highest "
                    "log-probability of the drawn entries).  logp_word / mean_logp_word: teacher-forced word probability; "
                    "mbr_bleu: minimum-Bayes-risk -- the candidate of highest mean sentence BLEU against the other N - 1, "
                    "computed on the device on token ids, ties to the higher log-probability (no scoring pass); every line of "
                    "OUTPUT/output_fira_samples then carries the N values under the key")
    ap.add_argument("--no-repeat-ngram", type=int, default=None, metavar="N", help="test: the search (any --beam) emits no "
                    "N-gram of words twice in a message (1: no word twice); a word is blocked through its generator id and "
                    "through every copy slot of the commit that carries it")
    ap.add_argument("--min-length", type=int, default=None, metavar="M", help="test: the search does not end a message before "
                    "M words (at most tar_len - 2)")
    ap.add_argument("--ban-words", default=None, metavar="W[,W...]", help="test: up to 32 vocabulary words the search never "
                    "emits, generator or copied (<unkm> may be given by name; <pad>, <eos> and <start> may not)")
    ap.add_argument("--merge-copies", action="store_true", help="test: the search (any --beam) ranks WORDS, not entries: the "
                    "copy entries of a step's distribution are folded into the generator entry of the word they resolve to, so "
                    "a word counts once with its whole probability and the beam holds distinct messages; combines with "
                    "--no-repeat-ngram, --min-length and --ban-words")
    ap.add_argument("--nbest", action="store_true", help="test, beam above 1: also write OUTPUT/output_fira_nbest, one JSON "
                    "line per commit with the beam's messages and their probabilities, best first (OUTPUT/output_fira is "
                    "unchanged: its line is the first message); without --merge-copies the list may repeat a message")
    ap.add_argument("--length-penalty", type=float, default=None, metavar="A", help="test, beam above 1: rank hypotheses by "
                    "ln(prob) / ((5 + m) / 6)^A, m = words emitted (GNMT's length penalty, 0 <= A <= 4) instead of the raw "
                    "probability, under which a message that ends early wins; combines with the constraint options, "
                    "--merge-copies and --nbest")
    ap.add_argument("--beam-groups", type=int, default=None, metavar="G", help="test, beam above 1: diverse beam search -- the "
                    "beam is G groups (G divides --beam) that --diversity-penalty keeps apart; needs --diversity-penalty")
    ap.add_argument("--diversity-penalty", type=float, default=None, metavar="L", help="test, with --beam-groups: a group ranks "
                    "a continuation L lower (in log-probability) for every earlier group that has just appended the same word, "
                    "generator or copied (0 < L <= 1024)")
    ap.add_argument("--ensemble", default=None, metavar="PATH[,PATH...]", help="test: search (any --beam) under the weighted "
                    "mean of several checkpoints' step distributions, mixed on the device: each PATH is a further state-dict "
                    "file in the layout of best_model.pt, which stays member 0 (up to 8 models in all)")
    ap.add_argument("--ensemble-weights", default=None, metavar="W0,W1,...", help="with --ensemble: one weight >= 0 per model, "
                    "best_model.pt first; normalised to sum 1 (default: uniform)")
    ap.add_argument("--prefix", default=None, metavar="WORDS", help="test: every message of the search (any --beam) begins "
                    "with these words; a word is forced through its generator id or a copy slot that carries it, identifiers go "
                    "through the commit's variable map, a word the vocabulary lacks is forced as <unkm>; at most tar_len - 2 "
                    "words; --merge-copies is recommended with it")
    ap.add_argument("--prefix-file", default=None, metavar="PATH", help="test: as --prefix, with one line per test commit in "
                    "all_index['test'] order (an empty line: no prefix for that commit)")
    ap.add_argument("--require-words", default=None, metavar="W[,W...]", help="test, beam above 1: every message of the search "
                    "contains these words (up to 4; lexically constrained decoding with dynamic beam allocation): the beam is "
                    "divided into banks by the number of required words a hypothesis holds, and no message ends before it holds "
                    "them all; a word counts through its generator id or a copy slot that carries it, identifiers go through "
                    "the commit's variable map, a word the vocabulary lacks is dropped with a warning; needs --beam above the "
                    "number of words; --merge-copies is recommended with it")
    ap.add_argument("--require-file", default=None, metavar="PATH", help="test: as --require-words, with one line per test "
                    "commit in all_index['test'] order, words separated by white space (an empty line: none for that commit)")
    ap.add_argument("--retrieve", action="store_true", help="test: retrieval-augmented search (any --beam) -- every test commit "
                    "looks up the train commit with the nearest encoder representation, and at every step the distribution the "
                    "model predicts for that neighbour is mixed into its own, weighted by the similarity; also writes "
                    "OUTPUT/output_fira_neighbours (one JSON line per commit: train_index, sim, message).  Not with --sample, "
                    "--score or --ensemble")
    ap.add_argument("--retrieve-lambda", type=float, default=None, metavar="L", help="with --retrieve: the neighbour's weight is "
                    "L x similarity (default 1; 0 = the plain search)")
    ap.add_argument("--retrieve-min-sim", type=float, default=None, metavar="X", help="with --retrieve: commits whose neighbour "
                    "is less similar than X are searched without it (default 0)")
    ap.add_argument("--retrieve-store", default=None, metavar="PATH", help="with --retrieve: the file of the train split's "
                    "vectors; built and written on first use, loaded afterwards (default OUTPUT/retrieve_store.pt)")
    ap.add_argument("--retrieve-only", action="store_true", help="with --retrieve: write the neighbour's message to "
                    "OUTPUT/output_fira without decoding (the retrieval baseline)")
    ap.add_argument("--clip-grad-norm", type=float, default=None, metavar="C", help="train: clip the gradient to the global "
                    "norm C > 0 on the device (torch.nn.utils.clip_grad_norm_; inf = observe and guard only) and apply a step "
                    "whose gradient holds an inf / nan as a zero-gradient step instead of destroying the weights; every "
                    "--loss-log line then carries grad_norm and clip_coef")
    ap.add_argument("--lr-schedule", default=None, choices=LR_SCHEDULES, help="train: warmup and decay of the learning rate "
                    "as a function of the optimisation step (--lr is the peak): constant = --lr behind a linear warmup; "
                    "inv-sqrt = linear warmup, then lr * sqrt(W / step); cosine / linear = linear warmup, then down to --lr-min at "
                    "step --lr-decay-steps.  Every --loss-log line then carries lr.  Default: none (--lr at every step)")
    ap.add_argument("--warmup-steps", type=int, default=None, metavar="W", help="with --lr-schedule: steps of linear warmup "
                    "(default 0; inv-sqrt needs W >= 1)")
    ap.add_argument("--lr-decay-steps", type=int, default=None, metavar="N", help="with --lr-schedule cosine|linear: the step "
                    "at which the rate reaches --lr-min, N > W (default: the optimisation steps the run plans -- --max-steps if "
                    "given, else epochs x steps per epoch -- counted from the step a --resume starts at)")
    ap.add_argument("--lr-min", type=float, default=None, metavar="X", help="with --lr-schedule cosine|linear: the rate from "
                    "step N on, 0 <= X <= --lr (default 0)")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D", help="train: keep an exponential moving average of "
                    "the weights on the device, per-step decay 0 < D < 1 (for example 0.999); the dev passes run on it and "
                    "best_model.pt holds it (the raw weights travel in fira_train_state.pt with --save-optimizer)")
    ap.add_argument("--ema-every", type=int, default=None, metavar="K", help="with --ema-decay: update the average every K-th "
                    "step by the weight 1 - D^K (default 32, the cadence at which the row-sparse Adam has just written every "
                    "row; 1 = the per-step average)")
    ap.add_argument("--accum-steps", type=int, default=None, metavar="K", help="train: gradient accumulation -- every "
                    "optimisation step runs each rank's shard of the GLOBAL --batch-size as K micro-batches of ceil(shard / K) "
                    "commits (1 <= K <= 64) and updates once, normalised by their total token count: the step of the whole "
                    "batch in the memory of one micro-batch.  --max-steps, --warmup-steps, --lr-decay-steps and --ema-every "
                    "count optimisation steps; every --loss-log line then carries micro = K.  Default: off (one pass per step)")
    a = ap.parse_args(argv)
    try:
        check_accum_args(a)
        check_clip_args(a)
        check_ema_args(a)
        check_lr_schedule_args(a)
        check_without_replacement_args(a)
        check_score_args(a)
        check_constraint_args(a)
        check_merge_args(a)
        check_scoring_args(a)
        check_prefix_args(a)
        check_require_args(a)
        check_ensemble_args(a)
        check_sample_args(a)
        check_cut_args(a)
        check_retrieve_args(a)
    except ValueError as e:
        ap.error(str(e))
    return a


RERANK_KEYS = ("logp_word", "mean_logp_word", "mbr_bleu")
LR_SCHEDULES = ("constant", "inv-sqrt", "cosine", "linear")


def check_accum_args(a):
    """Validates --accum-steps (no GPU, no DataSet needed); raises ValueError on a conflict or an out-of-range value."""
    if a.accum_steps is None:
        return a
    if a.stage != "train":
        raise ValueError("--accum-steps only applies to the train stage")
    from fira_icse_amd import ops
    try:
        ops.accum_check(a.accum_steps)
    except ValueError as e:
        raise ValueError("--accum-steps: %s" % e)
    return a


def micro_batches(mine, k):
    """A rank's shard ``mine`` (a list of train-split positions) of one global batch as the K micro-batches of --accum-steps:
    ceil(len / K) positions each, in order; a short shard leaves the last ones smaller or empty -- always K lists."""
    from fira_icse_amd import ops
    return [list(mine[lo:hi]) for lo, hi in ops.accum_split(0, len(mine), k)]


def loss_log_record(epoch, batch, gidx, loss, micro=None, grad=None, lr=None):
    """One --loss-log line (a dict): the positions of the whole global batch and its mean token loss; ``grad`` =
    ``(grad_norm, clip_coef)`` with --clip-grad-norm, ``lr`` with --lr-schedule, ``micro`` = K with --accum-steps (the loss is
    then the one accumulated over the K micro-batches).  Keys a run did not ask for are absent."""
    rec = {"epoch": epoch, "batch": batch, "index": [int(i) for i in gidx], "loss": loss}
    if grad is not None:
        rec["grad_norm"], rec["clip_coef"] = grad
    if lr is not None:
        rec["lr"] = lr
    if micro is not None:
        rec["micro"] = int(micro)
    return rec


def check_clip_args(a):
    """Validates --clip-grad-norm (no GPU, no DataSet needed); raises ValueError on a conflict or an out-of-range value."""
    c = a.clip_grad_norm
    if c is None:
        return a
    if a.stage != "train":
        raise ValueError("--clip-grad-norm only applies to the train stage")
    if not c > 0:                                            # (also refuses nan)
        raise ValueError("--clip-grad-norm %g: must be > 0 (inf = observe and guard only)" % c)
    return a


def check_ema_args(a):
    """Validates --ema-decay / --ema-every (no GPU, no DataSet needed); raises ValueError on a conflict or an out-of-range
    value.  Fills in the default cadence."""
    if a.ema_decay is None:
        if a.ema_every is not None:
            raise ValueError("--ema-every needs --ema-decay")
        return a
    if a.stage != "train":
        raise ValueError("--ema-decay only applies to the train stage")
    from fira_icse_amd import ops
    try:
        ops.ema_check(a.ema_decay, 32 if a.ema_every is None else a.ema_every)
    except ValueError as e:
        raise ValueError("--ema-decay / --ema-every: %s" % e)
    if a.ema_every is None:
        a.ema_every = 32
    return a


def check_lr_schedule_args(a):
    """Validates --lr-schedule / --warmup-steps / --lr-decay-steps / --lr-min (no GPU, no DataSet needed); raises ValueError on
    a conflict or an out-of-range value.  The formulas themselves live in the library (fira_lr_at)."""
    kind, W, N, mn = a.lr_schedule, a.warmup_steps, a.lr_decay_steps, a.lr_min
    given = [n for n, v in (("--warmup-steps", W), ("--lr-decay-steps", N), ("--lr-min", mn)) if v is not None]
    if kind is None:
        if given:
            raise ValueError("%s needs --lr-schedule" % ", ".join(given))
        return a
    if a.stage != "train":
        raise ValueError("--lr-schedule only applies to the train stage")
    if not (a.lr > 0 and a.lr < float("inf")):                 # (also refuses nan)
        raise ValueError("--lr %g: a schedule needs a finite peak rate > 0" % a.lr)
    if kind in ("constant", "inv-sqrt"):
        for name, v in (("--lr-decay-steps", N), ("--lr-min", mn)):
            if v is not None:
                raise ValueError("%s has no meaning with --lr-schedule %s (it never reaches a floor)" % (name, kind))
    if W is not None and W < 0:
        raise ValueError("--warmup-steps %d: must be >= 0" % W)
    if kind == "inv-sqrt" and (W is None or W < 1):
        raise ValueError("--lr-schedule inv-sqrt needs --warmup-steps W >= 1")
    if kind in ("cosine", "linear"):
        if N is not None and N <= (W or 0):
            raise ValueError("--lr-decay-steps %d: --lr-schedule %s needs N > W (--warmup-steps %d)" % (N, kind, W or 0))
        if mn is not None and not (0 <= mn <= a.lr):           # (also refuses nan)
            raise ValueError("--lr-min %g: must be in [0, --lr %g]" % (mn, a.lr))
    return a


def lr_schedule_from_args(a, planned_steps: int, done_steps: int = 0):
    """The ops.LrSchedule fields the options describe (None without --lr-schedule).  planned_steps: the optimisation steps
    this run plans; done_steps: the steps a resumed state has behind it -- the default of --lr-decay-steps is their sum."""
    if a.lr_schedule is None:
        return None
    W = a.warmup_steps or 0
    decays = a.lr_schedule in ("cosine", "linear")
    N = (a.lr_decay_steps if a.lr_decay_steps is not None else done_steps + planned_steps) if decays else 0
    if decays and N <= W:
        raise ValueError("--lr-schedule %s: the run plans %d steps, not more than --warmup-steps %d; give --lr-decay-steps"
                         % (a.lr_schedule, N, W))
    return {"kind": a.lr_schedule.replace("-", "_"), "base_lr": a.lr, "warmup_steps": W, "decay_steps": N,
            "min_lr": (a.lr_min or 0.0) if decays else 0.0}


def check_without_replacement_args(a):
    """Validates --without-replacement against the other options (no GPU, no DataSet needed); raises ValueError naming the
    option on a conflict.  The options it combines with pass their own checks (they let --sample through when it is given)."""
    if not getattr(a, "without_replacement", False):
        return a
    wr = "--without-replacement"
    if a.stage != "test":
        raise ValueError("%s only applies to the test stage" % wr)
    if a.sample is None:
        raise ValueError("%s draws the candidates of --sample without replacement: it needs --sample" % wr)
    for name, flag in (("top_k", "--top-k"), ("top_p", "--top-p")):
        if getattr(a, name, None) is not None:
            raise ValueError("%s samples from the whole tempered distribution: it does not combine with %s" % (wr, flag))
    if a.beam is not None and a.beam > 1:
        raise ValueError("%s is a search of its own over --sample slots: it does not combine with --beam %d" % (wr, a.beam))
    if getattr(a, "score", None) is not None:
        raise ValueError("%s draws messages: it does not combine with --score" % wr)
    for name, flag in (("prefix", "--prefix"), ("prefix_file", "--prefix-file"), ("length_penalty", "--length-penalty"),
                       ("beam_groups", "--beam-groups"), ("diversity_penalty", "--diversity-penalty")):
        if getattr(a, name, None) is not None:
            raise ValueError("%s ranks by a random key of the whole message: it does not combine with %s" % (wr, flag))
    if getattr(a, "nbest", False):
        raise ValueError("%s writes its candidates to output_fira_samples: it does not combine with --nbest" % wr)
    if getattr(a, "ensemble", None) is not None and a.rerank in ("logp_word", "mean_logp_word"):
        raise ValueError("%s with --ensemble: --rerank %s scores with one model and does not combine with an ensemble "
                         "(--rerank mbr_bleu does)" % (wr, a.rerank))
    return a


def check_score_args(a):
    """Validates --score / --rerank against the other options (no GPU, no DataSet needed); raises ValueError on a conflict."""
    if a.rerank is not None and a.sample is None:
        raise ValueError("--rerank %s ranks sampled candidates: it needs --sample" % a.rerank)
    if a.score is None:
        return a
    if a.stage != "test":
        raise ValueError("--score only applies to the test stage")
    if a.sample is not None:
        raise ValueError("--score scores given messages instead of producing them: it does not combine with --sample")
    if a.beam is not None and a.beam > 1:
        raise ValueError("--score scores given messages instead of searching: it does not combine with --beam %d" % a.beam)
    if a.score != "refs" and not os.path.isfile(a.score):
        raise ValueError("--score %s: not 'refs' and no such file" % a.score)
    a.beam = 1
    return a


def read_score_lines(path, n_commits):
    """The candidate lines of ``--score PATH``: per test commit (1..8 message strings, whether the line was JSON).  A line is plain text (the
    format of OUTPUT/output_fira) or the JSON of OUTPUT/output_fira_samples ({"candidates": [...]}).  Raises ValueError on
    a wrong line count or candidate count."""
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if len(lines) != n_commits:
        raise ValueError("--score %s: %d lines for %d test commits" % (path, len(lines), n_commits))
    out = []
    for k, line in enumerate(lines):
        cands, is_json = [line], False
        if line.lstrip().startswith("{"):
            try:
                rec = json.loads(line)
                if isinstance(rec, dict) and isinstance(rec.get("candidates"), list):
                    cands, is_json = [str(c) for c in rec["candidates"]], True
            except ValueError:
                pass                                          # not JSON: a message that starts with a brace
        if not 1 <= len(cands) <= 8:
            raise ValueError("--score %s: line %d holds %d candidates, outside 1..8" % (path, k + 1, len(cands)))
        out.append((cands, is_json))
    return out


CONSTRAINT_OPTIONS = (("no_repeat_ngram", "--no-repeat-ngram"), ("min_length", "--min-length"), ("ban_words", "--ban-words"))


def check_constraint_args(a):
    """Validates --no-repeat-ngram / --min-length / --ban-words against the other options (no GPU, no DataSet needed); raises
    ValueError on a conflict or an out-of-range value.  The words are looked up later (constraints_from_args)."""
    given = [flag for name, flag in CONSTRAINT_OPTIONS if getattr(a, name) is not None]
    if not given:
        return a
    if a.stage != "test":
        raise ValueError("%s only apply to the test stage" % ", ".join(given))
    if a.sample is not None and not getattr(a, "without_replacement", False):
        raise ValueError("%s constrain a search: they do not combine with --sample" % ", ".join(given))
    if a.score is not None:
        raise ValueError("%s constrain a search: they do not combine with --score" % ", ".join(given))
    if a.no_repeat_ngram is not None and a.no_repeat_ngram < 0:
        raise ValueError("--no-repeat-ngram %d: must be >= 0 (0 = off)" % a.no_repeat_ngram)
    if a.min_length is not None and a.min_length < 0:
        raise ValueError("--min-length %d: must be >= 0 (0 = off)" % a.min_length)
    if a.ban_words is not None and not [w for w in a.ban_words.split(",") if w.strip()]:
        raise ValueError("--ban-words: no word given")
    return a


def constraints_from_args(a, vocab, cfg=None):
    """The decode.Constraints of the command line (None without the options): --ban-words looked up in ``vocab`` (word -> id).
    Raises ValueError naming an unknown word, a word that cannot be banned, or a value outside the model's limits."""
    from fira_icse_amd.decode import Constraints
    if all(getattr(a, name, None) is None for name, _ in CONSTRAINT_OPTIONS):
        return None
    ids = []
    for w in (a.ban_words or "").split(","):
        w = w.strip()
        if not w:
            continue
        if w not in vocab:
            raise ValueError("--ban-words: %r is not in the vocabulary" % w)
        if vocab[w] < UNK:
            raise ValueError("--ban-words: %s cannot be banned" % w)
        ids.append(int(vocab[w]))
    c = Constraints(no_repeat_ngram=a.no_repeat_ngram or 0, min_length=a.min_length or 0, banned=tuple(ids))
    return c.check(cfg) if cfg is not None else c


def check_merge_args(a):
    """Validates --merge-copies / --nbest against the other options (no GPU, no DataSet needed); raises ValueError on a
    conflict."""
    merge, nbest = getattr(a, "merge_copies", False), getattr(a, "nbest", False)
    given = [flag for on, flag in ((merge, "--merge-copies"), (nbest, "--nbest")) if on]
    if not given:
        return a
    if a.stage != "test":
        raise ValueError("%s only apply to the test stage" % ", ".join(given))
    if a.sample is not None and not (getattr(a, "without_replacement", False) and not nbest):
        raise ValueError("%s belong to a search: they do not combine with --sample" % ", ".join(given))
    if a.score is not None:
        raise ValueError("%s belong to a search: they do not combine with --score" % ", ".join(given))
    if nbest and a.beam is not None and a.beam <= 1:
        raise ValueError("--nbest lists the hypotheses of a beam: it does not combine with --beam %d" % a.beam)
    return a


SCORING_OPTIONS = (("length_penalty", "--length-penalty"), ("beam_groups", "--beam-groups"),
                   ("diversity_penalty", "--diversity-penalty"))


def check_scoring_args(a):
    """Validates --length-penalty / --beam-groups / --diversity-penalty against the other options (no GPU, no DataSet needed);
    raises ValueError naming the flags on a conflict or an out-of-range value (the ranges are decode.BeamScoring's)."""
    given = [flag for name, flag in SCORING_OPTIONS if getattr(a, name, None) is not None]
    if not given:
        return a
    if a.stage != "test":
        raise ValueError("%s only apply to the test stage" % ", ".join(given))
    if a.sample is not None:
        raise ValueError("%s rank the hypotheses of a beam: they do not combine with --sample" % ", ".join(given))
    if a.score is not None:
        raise ValueError("%s rank the hypotheses of a beam: they do not combine with --score" % ", ".join(given))
    if a.beam is not None and a.beam <= 1:
        raise ValueError("%s rank the hypotheses of a beam: they do not combine with --beam %d" % (", ".join(given), a.beam))
    A, G, lam = a.length_penalty, a.beam_groups, a.diversity_penalty
    if A is not None and not 0 <= A <= 4:                      # (also refuses nan)
        raise ValueError("--length-penalty %g: must be in [0, 4] (0 = off)" % A)
    if G is not None and not 1 <= G <= 8:
        raise ValueError("--beam-groups %d: must be in 1..8 (1 = off)" % G)
    if lam is not None and not 0 <= lam <= 1024:
        raise ValueError("--diversity-penalty %g: must be in [0, 1024] (0 = off)" % lam)
    if (lam or 0) > 0 and (G or 1) == 1:
        raise ValueError("--diversity-penalty %g acts between beam groups: it needs --beam-groups above 1" % lam)
    if (G or 1) > 1 and not (lam or 0) > 0:
        raise ValueError("--beam-groups %d needs --diversity-penalty above 0 (else every group searches the same)" % G)
    beam = a.beam if a.beam is not None else 3
    if beam % (G or 1):
        raise ValueError("--beam-groups %d does not divide --beam %d" % (G, beam))
    return a


def scoring_from_args(a):
    """The decode.BeamScoring of the command line; None without the options or when they are all at their off values."""
    from fira_icse_amd.decode import BeamScoring
    if all(getattr(a, name, None) is None for name, _ in SCORING_OPTIONS):
        return None
    sc = BeamScoring(length_alpha=a.length_penalty or 0.0, groups=a.beam_groups or 1, diversity=a.diversity_penalty or 0.0)
    return sc.check(a.beam) if sc.active() else None


def check_prefix_args(a):
    """Validates --prefix / --prefix-file against the other options and the file system (no GPU, no DataSet needed); raises
    ValueError on a conflict.  The words are looked up later (prefixes_from_args)."""
    words, path = getattr(a, "prefix", None), getattr(a, "prefix_file", None)
    given = [flag for v, flag in ((words, "--prefix"), (path, "--prefix-file")) if v is not None]
    if not given:
        return a
    if len(given) == 2:
        raise ValueError("--prefix and --prefix-file are mutually exclusive")
    if a.stage != "test":
        raise ValueError("%s only apply to the test stage" % ", ".join(given))
    if a.sample is not None:
        raise ValueError("%s begin the messages of a search: they do not combine with --sample" % ", ".join(given))
    if a.score is not None:
        raise ValueError("%s begin the messages of a search: they do not combine with --score" % ", ".join(given))
    if words is not None and not words.split():
        raise ValueError("--prefix: no word given")
    if path is not None and not os.path.isfile(path):
        raise ValueError("--prefix-file %s: no such file" % path)
    return a


def read_prefix_lines(path, n_commits):
    """The lines of ``--prefix-file PATH``, one per test commit (an empty line: no prefix).  Raises ValueError on a wrong line
    count."""
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if len(lines) != n_commits:
        raise ValueError("--prefix-file %s: %d lines for %d test commits" % (path, len(lines), n_commits))
    return lines


def prefixes_from_args(a, vocab, var_maps, tar_len):
    """The forced message starts of the command line: (None, 0) without the options, else (one list of vocabulary ids per test
    commit, the number of words that became <unkm> because the vocabulary lacks them).  ``var_maps``: the commits' variable
    maps in test order; its length is the number of test commits.  Lines are tokenised with text.tokenize_message (the
    commit's identifiers to their placeholders), <start> / <eos> stripped.  Raises ValueError on a wrong line count or a
    prefix of more than tar_len - 2 words, naming the line."""
    words, path = getattr(a, "prefix", None), getattr(a, "prefix_file", None)
    if words is None and path is None:
        return None, 0
    n = len(var_maps)
    lines = [words] * n if words is not None else read_prefix_lines(path, n)
    out, n_unk = [], 0
    for k, (line, var_map) in enumerate(zip(lines, var_maps)):
        toks = line.split()
        if len(toks) > tar_len - 2:
            where = "--prefix" if words is not None else "--prefix-file %s: line %d" % (path, k + 1)
            raise ValueError("%s: %d words, more than tar_len - 2 = %d" % (where, len(toks), tar_len - 2))
        ids = text.tokenize_message(line, vocab, var_map, len(toks) + 2)[1:-1]
        n_unk += sum(1 for w in toks if w != text.UNK_EMOJI and var_map.get(w, w) not in vocab)
        out.append(ids)
    return out, n_unk


MAX_REQUIRED = 4                                 # decode.MAX_REQUIRED (not imported here: parsing needs no torch)


def check_require_args(a):
    """Validates --require-words / --require-file against the other options and the file system (no GPU, no DataSet needed);
    raises ValueError on a conflict.  The words are looked up later (required_from_args): how many are left for a commit, and
    the beam they need, is known only then."""
    words, path = getattr(a, "require_words", None), getattr(a, "require_file", None)
    given = [flag for v, flag in ((words, "--require-words"), (path, "--require-file")) if v is not None]
    if not given:
        return a
    if len(given) == 2:
        raise ValueError("--require-words and --require-file are mutually exclusive")
    what = given[0]
    if a.stage != "test":
        raise ValueError("%s only applies to the test stage" % what)
    if a.sample is not None:
        raise ValueError("%s names the words of a beam search's messages: it does not combine with --sample" % what)
    if a.score is not None:
        raise ValueError("%s names the words of a beam search's messages: it does not combine with --score" % what)
    beam = a.beam if a.beam is not None else 3
    if beam <= 1:
        raise ValueError("%s divides a beam into banks: it does not combine with --beam %d" % (what, beam))
    for name, flag in SCORING_OPTIONS:
        if getattr(a, name, None) is not None:
            raise ValueError("%s ranks its banks by raw probability: it does not combine with %s" % (what, flag))
    if words is not None:
        toks = [w for w in words.split(",") if w.strip()]
        if not toks:
            raise ValueError("--require-words: no word given")
        if any(len(w.split()) != 1 for w in toks):
            raise ValueError("--require-words: words are separated by commas, and a phrase is not one word")
    if path is not None and not os.path.isfile(path):
        raise ValueError("--require-file %s: no such file" % path)
    return a


def read_require_lines(path, n_commits):
    """The lines of ``--require-file PATH``, one per test commit (an empty line: no word).  Raises ValueError on a wrong line
    count."""
    with open(path) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if len(lines) != n_commits:
        raise ValueError("--require-file %s: %d lines for %d test commits" % (path, len(lines), n_commits))
    return lines


def required_from_args(a, vocab, var_maps, tar_len):
    """The required words of the command line: (None, 0) without the options, else (one list of vocabulary ids per test commit,
    the number of words dropped because the vocabulary lacks them for that commit).  ``var_maps``: the commits' variable maps
    in test order; its length is the number of test commits.  A word goes through the commit's variable map (the commit's
    identifiers to their placeholders) as a prefix word does; duplicates after mapping collapse to the first occurrence.
    Raises ValueError on a wrong line count, on more than 4 words left for a commit, on more than tar_len - 2, or on a
    --beam smaller than the longest list plus one, naming the line or the beam that is needed."""
    words, path = getattr(a, "require_words", None), getattr(a, "require_file", None)
    if words is None and path is None:
        return None, 0
    n = len(var_maps)
    unk = vocab["<unkm>"]
    lines = [words.replace(",", " ")] * n if words is not None else read_require_lines(path, n)
    out, n_dropped = [], 0
    for k, (line, var_map) in enumerate(zip(lines, var_maps)):
        ids = []
        for w in line.split():
            i = vocab.get(var_map.get(w, w))
            if i is None or i <= unk:                           # unknown here, or <pad> / <eos> / <start> / <unkm>
                n_dropped += 1
            elif i not in ids:
                ids.append(i)
        where = "--require-words" if words is not None else "--require-file %s: line %d" % (path, k + 1)
        if len(ids) > MAX_REQUIRED:
            raise ValueError("%s: %d words, more than %d" % (where, len(ids), MAX_REQUIRED))
        if len(ids) > tar_len - 2:
            raise ValueError("%s: %d words, more than tar_len - 2 = %d" % (where, len(ids), tar_len - 2))
        out.append(ids)
    longest = max((len(ids) for ids in out), default=0)
    beam = getattr(a, "beam", None)
    beam = 3 if beam is None else beam
    if longest and beam < longest + 1:
        k = next(k for k, ids in enumerate(out) if len(ids) == longest)
        where = "--require-words" if words is not None else "--require-file %s: line %d" % (path, k + 1)
        raise ValueError("%s: %d words need --beam %d or more (one bank per count of words met), not --beam %d"
                         % (where, longest, longest + 1, beam))
    return out, n_dropped


def required_summary(messages, required):
    """(commits with required words, those whose written message -- a list of ids -- contains all of them)."""
    with_words = [(m, r) for m, r in zip(messages, required) if r]
    return len(with_words), sum(1 for m, r in with_words if set(r) <= set(m[1:]))


def check_ensemble_args(a):
    """Validates --ensemble / --ensemble-weights against the other options and the file system (no GPU, no DataSet needed, no
    model loaded); raises ValueError on a conflict, a missing file, a wrong weight count or a bad weight.  Leaves
    ``a.ensemble`` as the list of paths (or None) and ``a.ensemble_weights`` as the list of weights as given (or None)."""
    from fira_icse_amd.decode import MAX_MODELS, ensemble_weights
    paths, weights = getattr(a, "ensemble", None), getattr(a, "ensemble_weights", None)
    if paths is None:
        if weights is not None:
            raise ValueError("--ensemble-weights only applies with --ensemble")
        return a
    if a.stage != "test":
        raise ValueError("--ensemble only applies to the test stage")
    if a.sample is not None and not getattr(a, "without_replacement", False):
        raise ValueError("--ensemble mixes the distributions of a search: it does not combine with --sample")
    if a.score is not None:
        raise ValueError("--ensemble mixes the distributions of a search: it does not combine with --score")
    if isinstance(paths, str):
        paths = [p for p in paths.split(",")]
    if not paths or any(not p for p in paths):
        raise ValueError("--ensemble: an empty path")
    if 1 + len(paths) > MAX_MODELS:
        raise ValueError("--ensemble: %d models in all, more than %d" % (1 + len(paths), MAX_MODELS))
    for p in paths:
        if not os.path.isfile(p):
            raise ValueError("--ensemble: no such file: %s" % p)
    if isinstance(weights, str):
        try:
            weights = [float(x) for x in weights.split(",")]
        except ValueError:
            raise ValueError("--ensemble-weights %s: not a list of numbers" % weights) from None
    if weights is not None:
        if len(weights) != 1 + len(paths):
            raise ValueError("--ensemble-weights: %d weights for %d models (best_model.pt first, then one per --ensemble path)"
                             % (len(weights), 1 + len(paths)))
        try:
            ensemble_weights(weights, 1 + len(paths))        # (checked here, normalised by the Searcher)
        except ValueError as e:
            raise ValueError("--ensemble-weights: %s" % e) from None
    a.ensemble, a.ensemble_weights = paths, weights
    return a


RETRIEVE_SUBOPTIONS = (("retrieve_lambda", "--retrieve-lambda"), ("retrieve_min_sim", "--retrieve-min-sim"),
                       ("retrieve_store", "--retrieve-store"), ("retrieve_only", "--retrieve-only"))


def check_retrieve_args(a):
    """Validates --retrieve and its sub-options against the other options (no GPU, no DataSet needed); raises ValueError on a
    conflict."""
    on = bool(getattr(a, "retrieve", False))
    for name, flag in RETRIEVE_SUBOPTIONS:
        v = getattr(a, name, None)
        if v is not None and v is not False and not on:
            raise ValueError("%s needs --retrieve" % flag)
    if not on:
        return a
    if a.stage != "test":
        raise ValueError("--retrieve only applies to the test stage")
    for name, flag in (("sample", "--sample"), ("score", "--score"), ("ensemble", "--ensemble")):
        if getattr(a, name, None) is not None:
            raise ValueError("--retrieve mixes a neighbour into the greedy and beam searches: it does not combine with %s" % flag)
    lam, ms = getattr(a, "retrieve_lambda", None), getattr(a, "retrieve_min_sim", None)
    if lam is not None and not 0 <= lam <= 1024:             # (also refuses nan)
        raise ValueError("--retrieve-lambda %r: must be in [0, 1024]" % lam)
    if ms is not None and not 0 <= ms < float("inf"):
        raise ValueError("--retrieve-min-sim %r: must be >= 0" % ms)
    if getattr(a, "retrieve_only", False):
        for name, flag in (("retrieve_lambda", "--retrieve-lambda"), ("retrieve_min_sim", "--retrieve-min-sim"), ("nbest", "--nbest")):
            v = getattr(a, name, None)
            if v is not None and v is not False:
                raise ValueError("--retrieve-only writes the neighbours' messages without decoding: it does not combine with %s"
                                 % flag)
    return a


def neighbour_record(train_index, sim, message):
    """One line of OUTPUT/output_fira_neighbours."""
    return json.dumps({"train_index": int(train_index), "sim": float(sim), "message": message}, ensure_ascii=False)


def nbest_record(messages, probs, keys=None, met=None):
    """One line of OUTPUT/output_fira_nbest: the beam's messages of positive probability (the -1 padding and zero-probability
    candidates are left out), ordered by probability descending, then slot ascending.  With ``keys`` (a search under
    --length-penalty / --beam-groups): ordered by key descending, then slot ascending, and the line carries the keys too.
    With ``met`` (a search under --require-words / --require-file): ordered by words met descending first, and the line
    carries the counts under "met"."""
    rank = probs if keys is None else keys
    order = sorted((j for j in range(len(probs)) if probs[j] > 0), key=lambda j: (0 if met is None else -met[j], -rank[j], j))
    rec = {"messages": [messages[j] for j in order], "prob": [probs[j] for j in order]}
    if keys is not None:
        rec["key"] = [keys[j] for j in order]
    if met is not None:
        rec["met"] = [met[j] for j in order]
    return json.dumps(rec)


SAMPLE_OPTIONS = (("temperature", "--temperature", 1.0), ("top_k", "--top-k", 0), ("top_p", "--top-p", 1.0),
                  ("sample_seed", "--sample-seed", 0))


def check_sample_args(a, vocab_size: int = None):
    """Validates the sampling options of ``a`` in place (no GPU, no DataSet needed) and fills in their defaults; raises
    ValueError on a conflict or an out-of-range value.  Without --sample the namespace is left as the search uses it."""
    if a.sample is None:
        given = [flag for name, flag, _ in SAMPLE_OPTIONS if getattr(a, name) is not None]
        if given:
            raise ValueError("%s only apply with --sample" % ", ".join(given))
        if a.beam is None:
            a.beam = 3
        return a
    if not 1 <= a.sample <= 8:
        raise ValueError("--sample %d: between 1 and 8 candidates per commit" % a.sample)
    if a.beam is not None and a.beam > 1:
        raise ValueError("--sample draws candidates instead of searching: it does not combine with --beam %d" % a.beam)
    a.beam = 1
    for name, _, default in SAMPLE_OPTIONS:
        if getattr(a, name) is None:
            setattr(a, name, default)
    if not (a.temperature > 0 and a.temperature < float("inf")):
        raise ValueError("--temperature %g: must be finite and > 0" % a.temperature)
    if a.top_k < 0 or (vocab_size is not None and a.top_k > vocab_size):
        raise ValueError("--top-k %d: must be >= 0 (0 = off)" % a.top_k)
    if not 0 < a.top_p <= 1:
        raise ValueError("--top-p %g: must be in (0, 1] (1 = off)" % a.top_p)
    if not 0 <= a.sample_seed < 1 << 64:
        raise ValueError("--sample-seed %d: must be in [0, 2^64)" % a.sample_seed)
    return a


CUT_OPTIONS = (("min_p", "--min-p"), ("epsilon_cutoff", "--epsilon-cutoff"), ("eta_cutoff", "--eta-cutoff"),
               ("typical_p", "--typical-p"))


def check_cut_args(a):
    """Validates the truncation cuts of --sample (--min-p, --epsilon-cutoff, --eta-cutoff, --typical-p; no GPU, no DataSet
    needed) after check_sample_args has passed what --sample itself refuses; raises ValueError naming the option on a conflict
    or an out-of-range value.  An option not given stays None (off)."""
    given = [(name, flag) for name, flag in CUT_OPTIONS if getattr(a, name, None) is not None]
    if not given:
        return a
    flags = ", ".join(flag for _, flag in given)
    if a.stage != "test":
        raise ValueError("%s only apply to the test stage" % flags)
    if a.sample is None:
        raise ValueError("%s only apply with --sample" % flags)
    if getattr(a, "without_replacement", False):
        raise ValueError("--without-replacement samples from the whole tempered distribution: it does not combine with %s"
                         % flags)
    for name, flag in given:
        v = getattr(a, name)
        if name == "typical_p":
            if not 0 < v <= 1:                               # (also refuses nan)
                raise ValueError("%s %g: must be in (0, 1] (1 = off)" % (flag, v))
        elif not 0 <= v < 1:
            raise ValueError("%s %g: must be in [0, 1) (0 = off)" % (flag, v))
    if given[-1][0] == "typical_p" and a.typical_p < 1:
        others = (["--top-p"] if a.top_p != 1.0 else []) + [flag for name, flag in given[:-1] if getattr(a, name) > 0]
        if others:
            raise ValueError("--typical-p keeps a band of the distribution, not its head: it does not combine with %s"
                             % ", ".join(others))
    return a


class Run:
    def __init__(self, a):
        self.a = a
        self.rank, self.world, self.local = init_from_env()
        torch.cuda.set_device(self.local)
        self.root = a.root
        with open(os.path.join(self.root, "DataSet", "word_vocab.json")) as f:
            self.vocab = json.load(f)
        with open(os.path.join(self.root, "DataSet", "ast_change_vocab.json")) as f:
            ast_vocab = json.load(f)
        self.r_vocab = {v: k for k, v in self.vocab.items()}
        # the kernels and the search loop use the special ids as constants (config.PAD/EOS/START/UNK); the reference looks
        # them up in word_vocab.json (run_model.py:205-222): refuse a vocabulary that numbers them differently
        for tok, want in (("<pad>", PAD), ("<eos>", EOS), ("<start>", START), ("<unkm>", UNK)):
            if self.vocab.get(tok) != want:
                raise ValueError("word_vocab.json maps %r to %r; this engine requires %d" % (tok, self.vocab.get(tok), want))
        with open(os.path.join(self.root, "DataSet", "variable.json")) as f:
            self.var_maps = json.load(f)
        bs = a.batch_size if a.batch_size else 170 * self.world
        self.cfg = FiraConfig(lr=a.lr, batch_size=bs, test_batch_size=a.test_batch_size, epoches=a.epochs,
                              beam_size=a.beam, vocab_size=len(self.vocab), ast_change_vocab_size=len(ast_vocab))
        splits = tuple(int(x) for x in a.splits.split(",")) if a.splits else None
        # rank 0 builds the caches (first run only: minutes of pure Python); the others poll the file system for the
        # finished, matching cache -- no collective, so no process-group timeout can fire during the build
        self.sets = {n: data.TransDataset(self.cfg, n, root=self.root, splits=splits, seed=a.seed, build=self.rank == 0)
                     for n in ("train", "valid", "test")}
        with open(os.path.join(self.root, "all_index")) as f:
            self.all_index = json.load(f)
        os.makedirs(os.path.join(self.root, "OUTPUT"), exist_ok=True)

    def out(self, name):
        return os.path.join(self.root, "OUTPUT", name)

    def device_batch(self, store, idx):
        from fira_icse_amd.model import DeviceBatch
        return DeviceBatch(store.batch(idx), self.cfg, self.model.device_)

    # ------------------------------------------------------------------------------ dev (run_model.py:118-184)
    @torch.no_grad()
    def dev(self, epoch):
        """(mean sentence-BLEU over the valid split, callable -> the text of OUTPUT/dev_output).  The pass itself lives in
        fira_icse_amd.devset: the host loop, or with --dev-on-device the resident valid set and the BLEU kernel; there the
        lines are only built (and gathered: a collective every rank enters, all ranks compare the same all-reduced number)
        when the caller asks for them."""
        store = self.sets["valid"].store
        if getattr(self, "dev_eval", None) is None or self.dev_eval.model is not self.model:
            from fira_icse_amd.devset import DevEvaluator
            self.dev_eval = DevEvaluator(self.model, store, self.cfg, self.r_vocab, self.var_maps, self.all_index["valid"],
                                         self.rank, self.world)
        on_device = getattr(self.a, "dev_on_device", False)
        self.model.eval()
        total, lines = self.dev_eval.device_pass() if on_device else self.dev_eval.host_pass()
        if self.world > 1:
            t = torch.tensor([total], dtype=torch.float64, device=self.model.device_)
            torch.distributed.all_reduce(t)
            total = float(t.item())

        def output():
            out = lines()
            if self.world > 1:
                out = gather_lines(out)
            return "\n".join(out) + "\n"

        if not on_device:                            # as ever: the lines are built and gathered in every pass
            done = output()
            output = lambda: done
        self.model.train()
        return total / max(1, len(store)), output

    # ------------------------------------------------------------------------------ train (run_model.py:83-117,382-399)
    def train(self):
        from fira_icse_amd.model import TransModel
        from fira_icse_amd.train import Trainer
        a, cfg = self.a, self.cfg
        store = self.sets["train"].store
        self.model = TransModel(cfg, device="cuda:%d" % self.local)       # consumes the torch RNG like the reference
        if a.resume and os.path.exists(os.path.join(self.root, "best_model.pt")):
            self.model.load_state_dict(torch.load(os.path.join(self.root, "best_model.pt"), map_location="cpu"))
        self.model.compute_dtype = a.dtype
        self.model.set_dropout_stream(a.seed, self.rank)           # masks depend on (--seed, rank, step)
        wire = a.grad_wire if a.grad_wire != "auto" else ("bf16" if a.dtype == "bf16" else "f32")
        state_path = os.path.join(self.root, "fira_train_state.pt")
        state = torch.load(state_path, map_location=self.model.device_) if a.resume and os.path.exists(state_path) else None
        if state is not None and "params" in state:
            # a run with --ema-decay wrote the AVERAGED weights to best_model.pt; training continues from the raw ones
            self.model.flat.data.copy_(state["params"])
        n_batches = -(-len(store) // cfg.batch_size)
        accum = getattr(a, "accum_steps", None)                    # None: the one-pass step; K is not optimizer state (a resume may change it)
        # (no --lr-schedule: no schedule object, the constant-rate path; a resumed state then brings its own, if it has one)
        schedule = lr_schedule_from_args(a, a.max_steps if a.max_steps else cfg.epoches * n_batches,
                                         int(state["t"]) if state is not None else 0)
        trainer = Trainer(self.model, lr=cfg.lr, distributed=self.world > 1, zero1=a.zero1, grad_wire=wire,
                          clip_grad_norm=a.clip_grad_norm, lr_schedule=schedule, accum_steps=accum,
                          **({} if a.ema_decay is None else {"ema_decay": a.ema_decay, "ema_every": a.ema_every}))
        # with --ema-decay the dev passes and every best_model.pt are taken on the averaged weights
        averaged = contextlib.nullcontext if a.ema_decay is None else trainer.averaged
        if state is not None:
            trainer.load_state_dict(state)                   # (refuses a state saved under another schedule)
            del state
        scheduled = trainer.lr_schedule is not None
        if scheduled and self.rank == 0:
            print("learning-rate schedule: %s" % (trainer.lr_schedule,), flush=True)
        self.model.train(not a.no_dropout)
        best_bleu, steps = -1.0, 0
        for epoch in range(cfg.epoches):
            total_data, t0 = 0, time.time()
            def prepare(gidx):                                     # worker thread: collate + H2D of this rank's shard
                mine = shard_indices(gidx, self.rank, self.world)   # DataParallel.scatter's contiguous chunks
                if accum is not None:                              # --accum-steps: K micro-batches, empty ones as None
                    return gidx, [self.device_batch(store, mb) if mb else None for mb in micro_batches(mine, accum)]
                return gidx, (self.device_batch(store, mine) if mine else None)

            batches = prefetch(data.iterate_batches(len(store), cfg.batch_size, shuffle=True), prepare, depth=2,
                               device=self.model.device_)
            for idx_b, (gidx, db) in enumerate(batches):
                if epoch >= a.dev_from_epoch and idx_b % a.dev_every == 0:
                    with averaged():
                        cur_bleu, dev_text = self.dev(epoch)
                        if self.rank == 0:
                            with open(self.out("train_process"), "a") as f:
                                f.write("epoch: {} batch: {} dev bleu: {} is better: {}\n".format(
                                    epoch, idx_b, cur_bleu, cur_bleu > best_bleu))
                        if cur_bleu > best_bleu:
                            best_bleu = cur_bleu
                            output_str = dev_text()          # (--dev-on-device: builds the lines now; collective when world > 1)
                            opt_state = trainer.state_dict() if a.save_optimizer else None     # collective with --zero1
                            if self.rank == 0:
                                torch.save(self.model.state_dict(), os.path.join(self.root, "best_model.pt"))
                                if a.save_optimizer:
                                    torch.save(opt_state, state_path)
                                with open(self.out("dev_output"), "w") as f:
                                    f.write(output_str)
                    self.model.train(not a.no_dropout)
                if accum is not None:
                    trainer.step_many(db)            # one update over this rank's K micro-batches (all None: as step(None))
                else:
                    trainer.step(db)                 # db None (empty shard of a short tail batch): still joins the collectives
                total_data += len(gidx)
                steps += 1
                if a.loss_log and self.rank == 0:
                    rec = loss_log_record(epoch, idx_b, gidx, trainer.last_loss(), micro=accum,
                                          grad=trainer.last_grad_norm()[:2] if a.clip_grad_norm is not None else None,
                                          lr=trainer.last_lr() if scheduled else None)
                    with open(a.loss_log, "a") as f:
                        f.write(json.dumps(rec) + "\n")
                if idx_b % 10 == 0 and self.rank == 0:
                    print("epoch: %d batch: %d/%d  data: %d/%d loss: %.4f  (%.1f commits/s)" % (
                        epoch, idx_b, n_batches, total_data, len(store), trainer.last_loss(),
                        total_data / max(time.time() - t0, 1e-9)), flush=True)
                if a.max_steps and steps >= a.max_steps:
                    break
            batches.close()                          # stops the worker thread and drops its prepared batches
            if a.clip_grad_norm is not None and self.rank == 0:
                _, _, n_clipped, n_nonfinite = trainer.last_grad_norm()      # running counts since the start of the run
                print("epoch: %d  clipped steps so far: %d  non-finite (zero-gradient) steps so far: %d of %d" % (
                    epoch, n_clipped, n_nonfinite, steps), flush=True)
            if trainer.ema is not None and self.rank == 0:
                print("epoch: %d  weight-average (EMA) updates so far: %d (step %d)" % (epoch, trainer.ema_updates, trainer.t),
                      flush=True)
            if scheduled and self.rank == 0:
                print("epoch: %d  learning rate: %.6g (step %d)" % (epoch, trainer.last_lr() or 0.0, trainer.t), flush=True)
            if a.max_steps and steps >= a.max_steps:
                break
        if best_bleu < 0:                               # never reached a dev point (short runs): keep the last weights
            with averaged():
                opt_state = trainer.state_dict() if a.save_optimizer else None             # collective with --zero1
                if self.rank == 0:
                    torch.save(self.model.state_dict(), os.path.join(self.root, "best_model.pt"))
                    if a.save_optimizer:                 # ... and the optimizer state that belongs to them (--resume)
                        torch.save(opt_state, state_path)
        return best_bleu

    # ------------------------------------------------------------------------------ test (run_model.py:187-380,401-415)
    @torch.no_grad()
    def test(self):
        from fira_icse_amd.model import TransModel
        from fira_icse_amd.decode import Searcher
        cfg, store = self.cfg, self.sets["test"].store
        test_index = self.all_index["test"]
        if self.a.sample is not None:
            check_sample_args(self.a, cfg.out_len)           # top-k against this vocabulary, before the model loads
        given = None
        if self.a.score is not None and self.a.score != "refs":
            given = read_score_lines(self.a.score, len(store))   # a wrong line count is an error before the model loads
        constraints = constraints_from_args(self.a, self.vocab, cfg)       # an unknown word too
        prefixes, n_unk = prefixes_from_args(self.a, self.vocab, [self.var_maps[i] for i in test_index], cfg.tar_len)
        if n_unk and self.rank == 0:                         # (a wrong line count or a line too long: an error before the model loads)
            print("warning: %d prefix words are not in the vocabulary and are forced as <unkm>" % n_unk, file=sys.stderr, flush=True)
        scoring = scoring_from_args(self.a)
        required, n_dropped = required_from_args(self.a, self.vocab, [self.var_maps[i] for i in test_index], cfg.tar_len)
        if n_dropped and self.rank == 0:                     # (a wrong line count or too many words: an error before the model loads)
            print("warning: %d required words are not in the vocabulary and are dropped" % n_dropped, file=sys.stderr, flush=True)
        self.model = TransModel(cfg, device="cuda:%d" % self.local, init=False)
        self.model.load_state_dict(torch.load(os.path.join(self.root, "best_model.pt"), map_location="cpu"))
        self.model.compute_dtype = self.a.dtype
        self.model.eval()
        members = []
        for path in getattr(self.a, "ensemble", None) or ():   # further checkpoints, loaded the way the primary is
            m = TransModel(cfg, device="cuda:%d" % self.local, init=False)
            m.load_state_dict(torch.load(path, map_location="cpu"))
            m.compute_dtype = self.a.dtype
            m.eval()
            members.append(m)
        search = Searcher(self.model, members=members, weights=getattr(self.a, "ensemble_weights", None))
        mine = shard_indices(list(range(len(store))), self.rank, self.world)
        retrieve = bool(getattr(self.a, "retrieve", False))
        datastore = self.retrieve_store(search) if retrieve else None
        nb_lines = []
        if self.a.sample is not None and getattr(self.a, "without_replacement", False):
            return self.test_sample_distinct(search, store, mine, constraints)
        if self.a.sample is not None:
            return self.test_sample(search, store, mine)
        if self.a.score is not None:
            return self.test_score(search, store, mine, given)
        merge, want_nbest = bool(getattr(self.a, "merge_copies", False)), bool(getattr(self.a, "nbest", False))
        lines, nbest, n_tok, t0 = [], [], 0, time.time()
        n_with, n_all = 0, 0                                 # --require-*: commits with words; messages that hold all of theirs
        # greedy: groups of `in_flight` batches share the GPU (independent launch chains: decode.Searcher.greedy_many; four lanes
        # on eight hardware queues: 0.14 ms per batch-step against 0.33 one at a time); the output order stays
        # all_index['test'] order (run_model.py:372)
        group = int(os.environ.get("FIRA_DECODE_IN_FLIGHT", "4")) if cfg.beam_size == 1 else 1
        starts = list(range(0, len(mine), cfg.test_batch_size))
        for g0 in range(0, len(starts), group):
            idxs = [mine[lo:lo + cfg.test_batch_size] for lo in starts[g0:g0 + group]]
            dbs = [self.device_batch(store, idx) for idx in idxs]
            # (--prefix / --prefix-file: the commits' forced message starts, batch by batch; without them no argument at all)
            forced = {} if prefixes is None else {"prefix": [[prefixes[i] for i in idx] for idx in idxs]}
            if retrieve:                                     # (--retrieve: the batches' neighbours; without it no argument at all)
                nbs = [self.neighbours(search, datastore, db, nb_lines) for db in dbs]
                if getattr(self.a, "retrieve_only", False):
                    continue
                forced["neighbour"] = nbs
            if cfg.beam_size == 1:
                outs = [search.best(*r) for r in search.greedy_many(dbs, in_flight=group, constraints=constraints,
                                                                    merge_copies=merge, **forced)]
            else:
                keys = met = None
                forced = {k: v[0] for k, v in forced.items()}
                if required is not None:                     # banks by words met: best_required's pick
                    words = [required[i] for i in idxs[0]]
                    res = search.beam(dbs[0], cfg.beam_size, constraints=constraints, merge_copies=merge, require=words, **forced)
                    gen, length, prob = res[:3]
                    met = res[3] if len(res) == 4 else torch.zeros_like(length)    # (a batch without words: three tensors)
                    outs = [search.best_required(gen, length, prob, met)]
                    w, h = required_summary(outs[0], words)
                    n_with, n_all = n_with + w, n_all + h
                    met = met.tolist()
                elif scoring is None:
                    gen, length, prob = search.beam(dbs[0], cfg.beam_size, constraints=constraints, merge_copies=merge, **forced)
                    outs = [search.best(gen, length, prob)]
                else:                                        # ranked by key: the best slot of positive probability, lowest on ties
                    gen, length, prob, keys = search.beam(dbs[0], cfg.beam_size, constraints=constraints, merge_copies=merge,
                                                          scoring=scoring, **forced)
                    outs = [search.best(gen, length, keys)]
                    keys = keys.tolist()
                if want_nbest:                               # the whole beam of every commit, best first
                    gen, length, prob = gen.tolist(), length.tolist(), prob.tolist()
                    for k, i in enumerate(idxs[0]):
                        msgs = [text.detokenize(g[:n], self.r_vocab, self.var_maps[test_index[i]])
                                for g, n in zip(gen[k], length[k])]
                        nbest.append(nbest_record(msgs, prob[k], None if keys is None else keys[k],
                                                  None if met is None else met[k]))
            for idx, hyps in zip(idxs, outs):
                for h, i in zip(hyps, idx):
                    lines.append(text.detokenize(h, self.r_vocab, self.var_maps[test_index[i]]))
                    n_tok += max(len(h) - 1, 0)
            if self.rank == 0:
                done = min(len(mine), starts[min(g0 + group, len(starts)) - 1] + cfg.test_batch_size)
                print("data: %d/%d  (%.1f tokens/s)" % (done, len(mine), n_tok / max(time.time() - t0, 1e-9)), flush=True)
        if retrieve and getattr(self.a, "retrieve_only", False):
            lines = [json.loads(l)["message"] for l in nb_lines]
        lines = gather_lines(lines)
        if retrieve:
            nb_lines = gather_lines(nb_lines)
            if self.rank == 0:
                with open(self.out("output_fira_neighbours"), "w") as f:
                    f.write("".join(l + "\n" for l in nb_lines))
        if want_nbest:
            nbest = gather_lines(nbest)
        if required is not None:
            counts = [l.split() for l in gather_lines(["%d %d" % (n_all, n_with)])]
            if self.rank == 0:
                print("required words: %d of the %d commits with words have a message that contains all of them"
                      % (sum(int(c[0]) for c in counts), sum(int(c[1]) for c in counts)), flush=True)
        if self.rank == 0:
            with open(self.out("output_fira"), "w") as f:
                f.write("".join(l + "\n" for l in lines))
            if want_nbest:
                with open(self.out("output_fira_nbest"), "w") as f:
                    f.write("".join(l + "\n" for l in nbest))
        return lines

    def retrieve_store(self, search):
        """--retrieve: the train split's vectors -- loaded from --retrieve-store, or built (one encoder pass per train batch) and
        written there by rank 0 on first use; the other ranks build their own copy in memory."""
        from fira_icse_amd.retrieve import Datastore
        path = getattr(self.a, "retrieve_store", None) or self.out("retrieve_store.pt")
        if os.path.isfile(path):
            ds = Datastore.load(path, self.model)
            if self.rank == 0:
                print("retrieve: loaded %d vectors from %s" % (len(ds), path), flush=True)
            return ds
        train = self.sets["train"].store
        bs = max(1, min(64, len(train)))
        batches = ((list(range(lo, min(lo + bs, len(train)))), self.device_batch(train, list(range(lo, min(lo + bs, len(train))))))
                   for lo in range(0, len(train), bs))
        ds = Datastore.build(self.model, batches, searcher=search)
        if self.rank == 0:
            ds.save(path)
            print("retrieve: built %d vectors, written to %s" % (len(ds), path), flush=True)
        return ds

    def neighbours(self, search, datastore, db, nb_lines):
        """The ``decode.Neighbour`` of one test batch: the nearest train commits, collated from the train store; appends the
        batch's lines of OUTPUT/output_fira_neighbours to ``nb_lines``."""
        from fira_icse_amd.decode import Neighbour
        train = self.sets["train"].store
        idx, sim = datastore.query(search, db)
        idx, sim = idx.tolist(), sim.tolist()
        train_index = self.all_index["train"]
        for i, s_ in zip(idx, sim):
            nb_lines.append(neighbour_record(i, s_, text.detokenize(train.tar[i], self.r_vocab, self.var_maps[train_index[i]])))
        a = self.a
        return Neighbour(self.device_batch(train, idx), sim, lam=1.0 if a.retrieve_lambda is None else a.retrieve_lambda,
                         min_sim=0.0 if a.retrieve_min_sim is None else a.retrieve_min_sim)

    def test_sample(self, search, store, mine):
        """--sample: N candidates per commit drawn on the device (decode.Searcher.sample); the noise of a commit is keyed by
        its index in the test split, so its candidates do not depend on how the commits are grouped into batches."""
        a, cfg = self.a, self.cfg
        test_index = self.all_index["test"]
        lines, samples, n_tok, t0 = [], [], 0, time.time()
        cuts = {kw: getattr(a, name) for (name, _), kw in zip(CUT_OPTIONS, ("min_p", "epsilon", "eta", "typical_p"))
                if getattr(a, name, None) is not None}
        for lo in range(0, len(mine), cfg.test_batch_size):
            idx = mine[lo:lo + cfg.test_batch_size]
            db = self.device_batch(store, idx)
            toks, lens, _, logp = search.sample(db, a.sample, temperature=a.temperature,
                                                top_k=a.top_k, top_p=a.top_p, seed=a.sample_seed, keys=idx, **cuts)
            best = search.best_sample(toks, lens, logp)
            values = None
            if a.rerank == "mbr_bleu":                       # expected BLEU among the candidates themselves: no scoring pass
                pick, util = search.mbr(toks, lens, logp)
                best = [toks[k, j, :int(lens[k, j])].tolist() for k, j in enumerate(pick)]
                values = util.tolist()
            elif a.rerank is not None:                       # score the drawn candidates; pick by the word marginal
                best, values = self.rerank(search, db, toks, lens)
            toks, lens, logp = toks.tolist(), lens.tolist(), logp.tolist()
            for k, i in enumerate(idx):
                var_map = self.var_maps[test_index[i]]
                lines.append(text.detokenize(best[k], self.r_vocab, var_map))
                cands = [text.detokenize(toks[k][j][:lens[k][j]], self.r_vocab, var_map) for j in range(a.sample)]
                rec = {"candidates": cands, "logp": logp[k]}
                if values is not None:
                    rec[a.rerank] = values[k]
                samples.append(json.dumps(rec))
                n_tok += sum(max(n - 1, 0) for n in lens[k])
            if self.rank == 0:
                print("data: %d/%d  (%.1f tokens/s)" % (min(len(mine), lo + cfg.test_batch_size), len(mine),
                                                        n_tok / max(time.time() - t0, 1e-9)), flush=True)
        lines, samples = gather_lines(lines), gather_lines(samples)
        if self.rank == 0:
            with open(self.out("output_fira"), "w") as f:
                f.write("".join(l + "\n" for l in lines))
            with open(self.out("output_fira_samples"), "w") as f:
                f.write("".join(l + "\n" for l in samples))
        return lines

    def test_sample_distinct(self, search, store, mine, constraints):
        """--sample N --without-replacement: N distinct messages per commit by stochastic beam search on the device
        (decode.Searcher.sample_distinct, over words); the noise of a commit is keyed by its index in the test split.  The
        files are --sample's; a line of output_fira_samples also carries the candidates' keys, best first, and leaves out the
        void slots of a commit that has fewer than N possible messages."""
        a, cfg = self.a, self.cfg
        test_index = self.all_index["test"]
        ninf = float("-inf")
        lines, samples, n_tok, t0 = [], [], 0, time.time()
        for lo in range(0, len(mine), cfg.test_batch_size):
            idx = mine[lo:lo + cfg.test_batch_size]
            db = self.device_batch(store, idx)
            toks, lens, logp, _, key = search.sample_distinct(db, a.sample, temperature=a.temperature, seed=a.sample_seed,
                                                              keys=idx, merge_copies=True, constraints=constraints)
            live = key > ninf                                # void slots come last: they are never picked, never written
            best = search.best_sample(toks, lens, logp)      # (a void slot's logp is -inf)
            values = None
            if a.rerank == "mbr_bleu":                       # a void slot is an empty message: it lowers every mean alike
                _, util = search.mbr(toks, lens, logp)
                masked = torch.where(live.cpu(), util, torch.full_like(util, ninf))
                top = masked.max(1, keepdim=True).values
                tie = torch.where(masked == top, logp.cpu().double(), torch.full_like(util, ninf))
                pick = torch.argmax(tie, dim=1).tolist()     # the utility, then the log-probability, then the lower slot
                best = [toks[k, j, :int(lens[k, j])].tolist() for k, j in enumerate(pick)]
                values = util.tolist()
            elif a.rerank is not None:
                best, values = self.rerank(search, db, toks, lens, live)
            toks, lens, logp, key, live = toks.tolist(), lens.tolist(), logp.tolist(), key.tolist(), live.tolist()
            for k, i in enumerate(idx):
                var_map = self.var_maps[test_index[i]]
                lines.append(text.detokenize(best[k], self.r_vocab, var_map))
                slots = [j for j in range(a.sample) if live[k][j]]
                rec = {"candidates": [text.detokenize(toks[k][j][:lens[k][j]], self.r_vocab, var_map) for j in slots],
                       "logp": [logp[k][j] for j in slots], "key": [key[k][j] for j in slots]}
                if values is not None:
                    rec[a.rerank] = [values[k][j] for j in slots]
                samples.append(json.dumps(rec))
                n_tok += sum(max(lens[k][j] - 1, 0) for j in slots)
            if self.rank == 0:
                print("data: %d/%d  (%.1f tokens/s)" % (min(len(mine), lo + cfg.test_batch_size), len(mine),
                                                        n_tok / max(time.time() - t0, 1e-9)), flush=True)
        lines, samples = gather_lines(lines), gather_lines(samples)
        if self.rank == 0:
            with open(self.out("output_fira"), "w") as f:
                f.write("".join(l + "\n" for l in lines))
            with open(self.out("output_fira_samples"), "w") as f:
                f.write("".join(l + "\n" for l in samples))
        return lines

    def rerank(self, search, db, toks, lens, live=None):
        """--rerank: the drawn candidates scored teacher-forced (decode.Searcher.score) and the best one per commit under the
        key.  A candidate in which <pad> or <start> was drawn mid-message cannot be scored (its text drops that id): it is
        scored up to there, reported as null and never preferred to a candidate that can."""
        from fira_icse_amd.decode import rank_values
        T = toks.shape[2]
        inner = (toks[:, :, 1:] == PAD) | (toks[:, :, 1:] == START)
        first = torch.where(inner.any(2), inner.long().argmax(2) + 1, torch.full_like(lens, T))
        cut = torch.minimum(lens, first)
        sc = search.score(db, toks, lengths=cut)
        vals = rank_values(sc, self.a.rerank).cpu()
        vals = torch.where(cut.cpu() < lens.cpu(), torch.full_like(vals, float("-inf")), vals)
        if live is not None:                                 # (--without-replacement: a void slot is never preferred)
            vals = torch.where(live.cpu(), vals, torch.full_like(vals, float("-inf")))
        pick = torch.argmax(vals, dim=1).tolist()
        best = [toks[k, j, :int(lens[k, j])].tolist() for k, j in enumerate(pick)]
        return best, [[v if v != float("-inf") else None for v in row] for row in vals.tolist()]

    def test_score(self, search, store, mine, given):
        """--score: teacher-forced scores of given messages (decode.Searcher.score), one JSON line per test commit in
        OUTPUT/output_fira_scores, and the corpus perplexity exp(-sum logp_word / sum n_tokens)."""
        cfg = self.cfg
        test_index = self.all_index["test"]
        V, L, T = cfg.vocab_size, cfg.sou_len, cfg.tar_len
        recs, t0 = [], time.time()

        def record(sc, k, j, ids, sou_row, sub_row):
            n_tok = int(sc["length"][k][j]) - 1
            src = []
            for e in sc["entry"][k][j][:n_tok]:
                src.append("none" if e < 0 else "gen" if e < V else "diff:%d" % (e - V) if e < V + L else "sub:%d" % (e - V - L))
            rec = {"logp_word": sc["logp_word"][k][j], "n_tokens": n_tok, "tokens": ids[1:n_tok + 1],
                   "p_word": sc["p_word"][k][j][:n_tok], "copy_share": sc["copy_share"][k][j][:n_tok], "source": src,
                   "top": [text.resolve_copy(t, sou_row, sub_row, V, L) for t in sc["top_id"][k][j][:n_tok]]}
            if "logp_label" in sc:
                rec["logp_label"] = sc["logp_label"][k][j]
            return rec

        for lo in range(0, len(mine), cfg.test_batch_size):
            idx = mine[lo:lo + cfg.test_batch_size]
            if given is None:
                counts = [1] * len(idx)
                cand, labels = store.tar[idx][:, None, :], store.tar_label[idx][:, None, :]
            else:
                msgs = [[text.tokenize_message(m, self.vocab, self.var_maps[test_index[i]], T) for m in given[i][0]] for i in idx]
                counts = [len(m) for m in msgs]
                n = max(counts)                                # commits with fewer candidates repeat their first one
                cand = np.zeros((len(idx), n, T), dtype=np.int64)
                for k, m in enumerate(msgs):
                    for j in range(n):
                        ids = m[j] if j < len(m) else m[0]
                        cand[k, j, :len(ids)] = ids
                labels = None
            sc = search.score(self.device_batch(store, idx), cand, labels=labels)
            sc = {k: v.tolist() for k, v in sc.items()}
            cand = np.asarray(cand).tolist()
            for k, i in enumerate(idx):
                rows = [record(sc, k, j, cand[k][j], store.sou[i], store.sub_token[i]) for j in range(counts[k])]
                recs.append(json.dumps(rows[0] if given is None or not given[i][1] else {"candidates": rows}))
            if self.rank == 0:
                print("data: %d/%d  (%.1f commits/s)" % (min(len(mine), lo + cfg.test_batch_size), len(mine),
                                                        len(recs) / max(time.time() - t0, 1e-9)), flush=True)
        recs = gather_lines(recs)
        if self.rank == 0:
            with open(self.out("output_fira_scores"), "w") as f:
                f.write("".join(l + "\n" for l in recs))
            import math
            flat = []
            for l in recs:
                r = json.loads(l)
                flat.extend(r["candidates"] if "candidates" in r else [r])
            n_tok = sum(r["n_tokens"] for r in flat)
            line = "scored %d messages, %d tokens: perplexity %.4f" % (
                len(flat), n_tok, math.exp(-sum(r["logp_word"] for r in flat) / max(n_tok, 1)))
            if flat and "logp_label" in flat[0]:
                line += " (label entries only: %.4f)" % math.exp(-sum(r["logp_label"] for r in flat) / max(n_tok, 1))
            print(line, flush=True)
        return recs


def main(argv=None):
    a = parse_args(sys.argv[1:] if argv is None else argv)
    seed_everything(a.seed)
    run = Run(a)
    if a.stage == "train":
        run.train()
    else:
        run.test()
    if run.world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
