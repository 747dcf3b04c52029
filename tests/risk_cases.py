"""The token batches of the risk tests (host program and GPU kernel see the same ones): three images per batch, built
so that every corner the rules name occurs -- an empty draw (END first), a draw without END, a draw equal to the gold
formula, a PAD sampled before END, an empty gold formula with an empty draw beside it (both empty: reward 1), a gold row
that fills all T places, and an image whose draws are all equal (every advantage 0 up to the rounding of the double sum of the other rewards)."""
import numpy as np

PAD, START, END = 0, 1, 2
LOW, HIGH = 3, 9          # body tokens: few, so that draws and gold share many of them


def _row(body, T, fill):
    body = list(body)[:T]
    return body + ([END] if len(body) < T else []) + [fill] * max(0, T - len(body) - 1)


def batch(N, T, seed):
    """-> formulas (3, T + 1) int32, draws (3, N, T) int32 (-1 behind END)."""
    rng = np.random.default_rng(seed)
    body = lambda n: rng.integers(LOW, HIGH, int(n)).tolist()
    formulas = np.zeros((3, T + 1), dtype=np.int32)
    draws = np.zeros((3, N, T), dtype=np.int32)
    # image 0: a gold formula of random length (every fourth seed: all T places, no END) and the corner draws, rotated by
    # the seed so that N = 2 meets all of them over a few batches; the rest are edits of the gold formula
    gold0 = body(T if seed % 4 == 3 else rng.integers(1, T + 1))
    formulas[0] = [START] + _row(gold0, T, PAD)
    near = list(gold0)
    for _ in range(max(1, len(near) // 4)):
        at = int(rng.integers(0, len(near)))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            near[at] = int(rng.integers(LOW, HIGH))
        elif kind == 1 and len(near) > 1:
            del near[at]
        else:
            near.insert(at, int(rng.integers(LOW, HIGH)))
    with_pad = list(gold0[:max(1, len(gold0) // 2)])
    with_pad[len(with_pad) // 2] = PAD                                   # the model sampled PAD before its END
    corners = [[], body(T), list(gold0), with_pad, near, body(rng.integers(1, T + 1))]
    for n in range(N):
        pick = corners[(n + seed) % len(corners)] if n < len(corners) else body(rng.integers(0, T + 1))
        draws[0, n] = _row(pick, T, -1)
    # image 1: an empty gold formula; draw 0 empty too, the others random
    formulas[1] = [START] + _row([], T, PAD)
    for n in range(N):
        draws[1, n] = _row([] if n == 0 else body(rng.integers(0, min(T, 6) + 1)), T, -1)
    # image 2: all draws equal
    formulas[2] = [START] + _row(body(rng.integers(1, T + 1)), T, PAD)
    same = _row(body(rng.integers(0, T + 1)), T, -1)
    for n in range(N):
        draws[2, n] = same
    return formulas, draws
