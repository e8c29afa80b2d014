"""Test-only statement of the template control (include/fira_hip.h: fira_template_dist) in plain numpy /
Python, written from its definition.  Not part of the product.

The tables are the device's: word_class [V] (the low five bits), next [32 * 32] with pitch 32 (-1, or a value of 32 or more: no
transition), need [32], start (one state; outside 0 .. 31: none).  For an unfinished row with the words h_1 .. h_m,
len = clamp(length, 1, T), m = len - 1:
    s = start, then s = next[s][class(h_p)] for p = 1 .. m, and -1 stays -1;   left = T - 1 - len
    w is blocked  iff  s == -1,  or  w == <eos> and need[s] != 0,  or  w != <eos> and (s' = next[s][class(w)]) == -1 or need[s'] > left
and every entry whose word is blocked becomes 0.0f, everything else keeps its bits.  A word outside [0, V) has class 0."""
import numpy as np

from constrain_ref import argmax_ref, entry_words, is_finished  # noqa: F401  (argmax_ref: the arg-max the kernel reports)

EOS = 1
N = 32
NEVER = 1 << 20


def class_of(word_class, w) -> int:
    w = int(w)
    return int(word_class[w]) & (N - 1) if 0 <= w < len(word_class) else 0


def step(nxt, s: int, c: int) -> int:
    if not 0 <= s < N:
        return -1
    t = int(nxt[s * N + c])
    return t if 0 <= t < N else -1


def walk(words, word_class, nxt, start) -> int:
    """The state after the words from ``start``; -1 once there is no transition (and for a start outside 0 .. 31)."""
    s = int(start) if 0 <= int(start) < N else -1
    for w in words:
        s = step(nxt, s, class_of(word_class, w))
    return s


def need_of(nxt, accept) -> np.ndarray:
    """need [32]: the fewest words from every state to a state of ``accept`` (NEVER if there is none), breadth first."""
    need = np.full(N, NEVER, dtype=np.int32)
    need[list(accept)] = 0
    for d in range(1, N + 1):
        for s in range(N):
            if need[s] == NEVER and any(step(nxt, s, c) >= 0 and need[step(nxt, s, c)] == d - 1 for c in range(N)):
                need[s] = d
    return need


def blocked(w, s, left, word_class, nxt, need) -> bool:
    if s < 0:
        return True
    if int(w) == EOS:
        return int(need[s]) != 0
    t = step(nxt, s, class_of(word_class, w))
    return t < 0 or int(need[t]) > left


def template_mask(gen_row, length, sou_row, sub_row, dims, word_class, nxt, need, start) -> np.ndarray:
    """bool[W]: the entries fira_template_dist sets to 0 for this row."""
    words = entry_words(sou_row, sub_row, dims)
    T = len(gen_row)
    n = min(max(int(length), 1), T)
    if is_finished(gen_row, n):
        return np.zeros(words.shape, dtype=bool)
    s = walk(gen_row[1:n], word_class, nxt, start)
    return np.array([blocked(w, s, T - 1 - n, word_class, nxt, need) for w in words], dtype=bool)
