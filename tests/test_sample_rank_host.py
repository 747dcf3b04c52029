"""The consensus decode on the host (no GPU).

csrc/sample_rank_rules.inc.h -- the cut, the distance, the risk, the keys and the order of the samples of an image -- as a
stand-alone program (csrc/sample_rank_host_main.cpp), a process of its own under the host sanitizers, compared with the
Python restatement (sample_rank_ref.py): ``order``, ``risk``, ``len``, ``finished`` and ``dist`` exactly, ``key`` bit for
bit.  Exhaustively over every image of up to 3 samples of up to 3 tokens over {a, b, END}, and on random and crafted
images up to 16 samples of 130 tokens (``image_kinds``: the GPU test feeds the same ones to i2l_sample_rank).
``boundary_images`` are the GPU test's images on the 64-token block boundaries up to 1024 steps; here their pairings are
checked and the restatement's numpy distance is held to the plain table at those sizes.

Also here: the header / library / ``_lib`` agreement on the three entries, the scratch-size query, the refusals of
i2l_sample_decode_multi and i2l_sample_rank (they answer before the first HIP call), and the Python and CLI refusals."""
import ctypes
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import png_cases
import sample_rank_ref as R
from img2latex_amd import _lib

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FAKE = 0x1000          # a non-null pointer that a refusing call never follows
END = 2
A, B = 5, 9


# ------------------------------------------------------------------------------------------------ the cases
def _scores(rng, S):
    """Multiples of 1/4 in [-3, 0]: exact in fp64 and tied often."""
    return rng.integers(-12, 1, size=S).astype(np.float64) / 4


def _random_rows(rng, S, T, p_end):
    ids = rng.choice(np.array([A, B, 7], dtype=np.int32), size=(S, T))
    for s in range(S):
        if rng.random() < p_end:
            at = int(rng.integers(0, T))
            ids[s, at] = END
            ids[s, at + 1:] = -1                         # the sticky stop's rows
    return ids.astype(np.int32)


def image_kinds(rng, S, T):
    """{kind: (ids (S, T) int32, score (S,) float64)}: the crafted images of one shape."""
    out = {}
    out["random"] = (_random_rows(rng, S, T, 0.7), _scores(rng, S))
    out["no end"] = (_random_rows(rng, S, T, 0.0), _scores(rng, S))
    ids = _random_rows(rng, S, T, 0.5)
    ids[::2, 0] = END                                    # END at step 0: the empty sequence, len 1
    ids[::2, 1:] = A                                     # tokens behind END are not the sequence's
    out["end at step 0"] = (ids, _scores(rng, S))
    one = _random_rows(rng, 1, T, 0.8)
    out["all equal, scores differ"] = (np.repeat(one, S, axis=0), -np.arange(S, dtype=np.float64)[::-1].copy())
    out["all equal, scores tie"] = (np.repeat(one, S, axis=0), np.full(S, -1.5))
    ids = _random_rows(rng, S, T, 1.0)
    ids[S // 2:] = ids[:S - S // 2]                      # pairs of equal samples: their risks tie, the score decides
    sc = _scores(rng, S)
    sc[S // 2:] = sc[:S - S // 2][::-1]
    out["risk ties"] = (ids, sc)
    ids = np.full((S, T), A, dtype=np.int32)             # lengths 0 .. T: END walks through the row
    for s in range(S):
        at = (s * max(T, 1)) // max(S, 1)
        if s % 3 != 2:
            ids[s, at] = END
            ids[s, at + 1:] = -1
    out["lengths"] = (ids, np.zeros(S))
    return out


def norm_table(T):
    return [1.0] + [float(n) ** 0.7 for n in range(1, T + 1)]


# ------------------------------------------------------------------------------------------------ the block boundaries
BOUNDARY_STEPS = [64, 128, 192, 193, 256, 257, 512, 513, 1023, 1024]    # sample_distance_kernel<W>: W = 1 2 3 4 4 8 8 16 16 16
ALPHABETS = (2, 5, 400)                                                 # dense .. sparse match masks
SAMPLES = 16


def alphabet(alpha):
    """The first ``alpha`` token ids that are not END; 0 is among them, so the kernel's zero padding is a real token."""
    return np.array([t for t in range(alpha + 1) if t != END], dtype=np.int32)


def boundary_lengths(T, image):
    """The cut length (the place of the first END; >= T: the row has none) of each of the 16 rows of image ``image``
    (0, 1 or 2).  Rows in pairs: 0-1 identical, 2-3 no token in common and no END, 4-5 one the other shifted by half its
    length, 6-7 / 8-9 / 10-11 equal but for their last token at R = 64, 128, T; rows 12-15 are random rows.  Over the
    three images the lengths are {0, 1, 63, 64, 65, 127, 128, 129, T / 2, T - 1, T, no END}, each clipped to T."""
    same, shifted, free = [(T - 1, T, (0, 1, 63, 65)), (T // 2, 127, (0, 1, 127, 129)), (129, T - 1, (0, 65, T // 2, T - 1))][image]
    return [same, same, T, T, shifted, shifted, 64, 64, 128, 128, T, T] + list(free)


def boundary_image(rng, T, alpha, image):
    """ids (16, T) int32 and the rows' cut lengths, each clipped to T.  Behind its END a row holds random tokens, further
    ENDs and zeros among them: the cut ignores them."""
    abc = alphabet(alpha)
    low, high = abc[:alpha // 2], abc[alpha // 2:]
    cut = [min(n, T) for n in boundary_lengths(T, image)]
    ids = rng.choice(abc, size=(SAMPLES, T)).astype(np.int32)
    ids[rng.random(ids.shape) < 0.1] = 0                 # the sparse alphabet too meets the padding's token
    ids[1] = ids[0]
    ids[2], ids[3] = rng.choice(low, size=T), rng.choice(high, size=T)
    n = cut[4]
    ids[5, :n // 2] = ids[4, n - n // 2:n]
    for s in (6, 8, 10):
        ids[s + 1] = ids[s]
        if cut[s]:
            ids[s + 1, cut[s] - 1] = abc[(list(abc).index(ids[s, cut[s] - 1]) + 1) % alpha]
    behind = np.concatenate([abc, [END, END, 0, 0]]).astype(np.int32)
    for s in range(SAMPLES):
        if cut[s] < T:
            ids[s, cut[s]] = END
            ids[s, cut[s] + 1:] = rng.choice(behind, size=T - cut[s] - 1)
    return ids, cut


def boundary_images(T, images=3):
    """[(ids, cut)] of ``images`` images of ``T`` steps; image k draws from alphabet k, the steps taking turns in which
    image comes first, so that a call of two images still meets every alphabet at every kernel width."""
    rng = np.random.default_rng(7000 + T)
    turn = BOUNDARY_STEPS.index(T) if T in BOUNDARY_STEPS else 0
    return [boundary_image(rng, T, ALPHABETS[(k + turn) % 3], (k + turn) % 3) for k in range(images)]


def boundary_scores(T, images=3):
    rng = np.random.default_rng(7100 + T)
    return np.stack([_scores(rng, SAMPLES) for _ in range(images)])


@pytest.mark.parametrize("T", BOUNDARY_STEPS)
def test_boundary_images_hold_the_pairings(T):
    """What test_sample_rank_gpu.test_distance_block_boundaries relies on, of every image: the restatement's cut is the
    intended one; two lengths that are multiples of 64; a row in block 0 beside one in the last block; an empty row
    beside a non-empty one; two rows without END; the crafted pairs are at distance 0, their length, and 1."""
    seen = set()
    for ids, cut in boundary_images(T):
        got = [R.cut(row, END) for row in ids]
        assert [len(g[0]) for g in got] == cut and [g[2] for g in got] == [int(n < T) for n in cut]
        seen |= set(cut)
        assert sum(n > 0 and n % 64 == 0 for n in cut) >= 2
        assert any(1 <= n <= 64 for n in cut) and any((n - 1) >> 6 == (T - 1) >> 6 for n in cut if n)
        assert 0 in cut and sum(n == T and END not in row for n, row in zip(cut, ids.tolist())) >= 2
        seq = [g[0] for g in got]
        assert sum(0 in q for q in seq) >= 4                                 # token 0 is in play
        assert seq[0] == seq[1] and not set(seq[2]) & set(seq[3]) and R.distance(seq[2], seq[3]) == T
        assert seq[5][:cut[4] // 2] == seq[4][cut[4] - cut[4] // 2:]
        for s in (6, 8, 10):
            assert cut[s] == cut[s + 1] and seq[s][:-1] == seq[s + 1][:-1] and seq[s][-1] != seq[s + 1][-1]
            assert (cut[s] - 1) & 63 == 63 or cut[s] == T
        for s in range(SAMPLES):                                             # something lies behind every END
            assert T - cut[s] <= 8 or len(set(ids[s, cut[s] + 1:].tolist())) > 1
    assert seen == {min(n, T) for n in (0, 1, 63, 64, 65, 127, 128, 129, T // 2, T - 1, T)}


def test_the_numpy_distance_at_the_block_boundaries():
    """sample_rank_ref.distance (a table row per numpy operation: the device tests' reference) against the plain table
    ``levenshtein`` at lengths on and around the 64-token block boundaries, each against each (the alphabets -- dense and
    sparse matches -- take turns over the pairs), a pair equal but for its last token, a pair one the other's shift, and
    one 1024 x 1023 pair."""
    rng = np.random.default_rng(64)
    lens = (63, 64, 65, 127, 128, 129, 255, 256, 257)
    for i, na in enumerate(lens):
        for j, nb in enumerate(lens):
            abc = alphabet(ALPHABETS[(i + j) % 3])
            a, b = rng.choice(abc, size=na).tolist(), rng.choice(abc, size=nb).tolist()
            want = R.levenshtein(a, b)
            assert 0 < want and R.distance(a, b) == want == R.distance(b, a), (na, nb)
    a = rng.choice(alphabet(5), size=257).tolist()
    assert R.distance(a, a[:256] + [a[256] + 7]) == 1 == R.levenshtein(a, a[:256] + [a[256] + 7])
    assert R.distance(a, a[128:] + a[:128]) == R.levenshtein(a, a[128:] + a[:128]) > 0
    a, b = rng.choice(alphabet(5), size=1024).tolist(), rng.choice(alphabet(5), size=1023).tolist()
    assert R.distance(a, b) == R.levenshtein(a, b) > 0


def make_cases():
    """[(what, ids, score, rank, norm or None)]"""
    rng = np.random.default_rng(20241020)
    out = []
    rows = {T: [np.array(r, dtype=np.int32) for r in itertools.product((A, B, END), repeat=T)] for T in (1, 2, 3)}
    for T in (1, 2, 3):                                  # every image of <= 3 samples of <= 3 tokens
        for S in (1, 2, 3):
            for k, pick in enumerate(itertools.product(range(len(rows[T])), repeat=S)):
                ids = np.stack([rows[T][i] for i in pick])
                sc = np.array([-((k + 3 * s) % 3) / 2 for s in range(S)])
                out.append((f"all {S}x{T} #{k}", ids, sc, k % 2, norm_table(T) if k % 4 >= 2 else None))
    for S, T in ((16, 130), (16, 65), (5, 129), (2, 64), (7, 7), (16, 1), (1, 130), (3, 66), (11, 40)):
        for kind, (ids, sc) in image_kinds(rng, S, T).items():
            for rank in (R.CONSENSUS, R.LOGPROB):
                for norm in (None, norm_table(T)):
                    out.append((f"{kind} {S}x{T} rank {rank} norm {norm is not None}", ids, sc, rank, norm))
    return out


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(b"SRNK" + struct.pack("<i", len(cases)))
        for _, ids, sc, rank, norm in cases:
            S, T = ids.shape
            f.write(struct.pack("<5i", S, T, END, rank, norm is not None))
            if norm is not None:
                f.write(struct.pack(f"<{T + 1}d", *norm))
            f.write(np.ascontiguousarray(ids, dtype="<i4").tobytes())
            f.write(np.ascontiguousarray(sc, dtype="<f8").tobytes())


def read_results(path, cases):
    data, pos, out = open(path, "rb").read(), 0, []
    for _, ids, _, _, _ in cases:
        S = ids.shape[0]
        take = lambda dt, n: np.frombuffer(data, dtype=dt, count=n, offset=pos)      # noqa: E731
        rec = {}
        for name, dt, n in (("len", "<i4", S), ("finished", "<i4", S), ("risk", "<i4", S), ("key", "<f8", S),
                            ("order", "<i4", S), ("dist", "<i4", S * S)):
            rec[name] = take(dt, n)
            pos += rec[name].nbytes
        out.append(rec)
    assert pos == len(data)
    return out


def check_against_restatement(got, ids, sc, rank, norm, where):
    want = R.rank_image(ids, END, sc, rank, norm)
    for name in ("len", "finished", "risk", "order"):
        assert list(got[name]) == list(want[name]), (where, name, list(got[name]), want[name])
    assert np.array_equal(np.asarray(got["dist"]).reshape(len(ids), len(ids)), np.array(want["dist"])), (where, "dist")
    assert np.asarray(got["key"], dtype=np.float64).tobytes() == want["key"].tobytes(), (where, "key", got["key"], want["key"])


def test_host_program_against_the_restatement(tmp_path):
    exe, sanitized = png_cases.build_host_program(str(tmp_path), "sample_rank_host_main")
    print("sample_rank_host_main built", "with -fsanitize=address,undefined" if sanitized else "PLAIN: the sanitizer build did not link")
    assert sanitized or os.environ.get("I2L_PNG_HOST_PLAIN") == "1", \
        "the sanitized build of sample_rank_host_main failed; set I2L_PNG_HOST_PLAIN=1 to accept a plain build on a machine without the runtime"
    cases = make_cases()
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    write_cases(src, cases)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    results = read_results(dst, cases)
    assert len(cases) > 20000
    for (what, ids, sc, rank, norm), got in zip(cases, results):
        check_against_restatement(got, ids, sc, rank, norm, what)


def test_the_restatement_on_known_answers():
    rng = np.random.default_rng(3)
    for _ in range(200):                                   # the numpy rows against the textbook table
        a, b = (rng.integers(0, 3, size=int(rng.integers(0, 40))).tolist() for _ in range(2))
        assert R.distance(a, b) == R.levenshtein(a, b) == R.distance(b, a), (a, b)
    assert R.levenshtein([1, 2, 3], [1, 3]) == 1 and R.levenshtein([], [4, 4]) == 2 and R.levenshtein([1, 2], [2, 1]) == 2
    assert R.cut([A, END, B], END) == ([A], 2, 1) and R.cut([A, B, B], END) == ([A, B, B], 3, 0) and R.cut([END], END) == ([], 1, 1)
    ids = [[A, B, END], [A, B, END], [B, B, B], [A, END, -1]]
    got = R.rank_image(ids, END, [-3.0, -1.0, -0.5, -2.0], R.CONSENSUS)
    assert got["dist"][0] == [0, 0, 2, 1] and got["risk"] == [3, 3, 7, 5]
    assert got["order"] == [1, 0, 3, 2] and list(got["key"]) == [3.0, 3.0, 7.0, 5.0]      # the tie at risk 3: the higher score
    got = R.rank_image(ids, END, [-3.0, -3.0, -0.5, -2.0], R.LOGPROB, [1.0, 1.0, 2.0, 3.0])
    assert list(got["key"]) == [-1.0, -1.0, -0.5 / 3.0, -1.0] and got["order"] == [2, 0, 1, 3]   # ties: the lower index


# ------------------------------------------------------------------------------------------------ the C entries
def test_header_library_and_binding_agree():
    header = open(os.path.join(REPO, "include", "img2latex_hip.h")).read()
    assert re.search(r"^size_t\s+i2l_sample_multi_scratch_bytes\s*\(", header, flags=re.M)
    assert re.search(r"^int\s+i2l_sample_decode_multi\s*\(", header, flags=re.M)
    assert re.search(r"^int\s+i2l_sample_rank\s*\(", header, flags=re.M)
    assert re.search(r"^#define\s+I2L_RANK_CONSENSUS\s+0\b", header, flags=re.M) and _lib.RANK_CONSENSUS == 0
    assert re.search(r"^#define\s+I2L_RANK_LOGPROB\s+1\b", header, flags=re.M) and _lib.RANK_LOGPROB == 1
    assert re.search(r"^#define\s+I2L_MAX_RANK_STEPS\s+1024\b", header, flags=re.M) and _lib.MAX_RANK_STEPS == 1024
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("i2l_sample_multi_scratch_bytes", "i2l_sample_decode_multi", "i2l_sample_rank"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(raw, name)
    L = _lib.lib()
    assert len(L.i2l_sample_multi_scratch_bytes.argtypes) == 7
    assert len(L.i2l_sample_decode_multi.argtypes) == 26
    assert len(L.i2l_sample_rank.argtypes) == 15
    assert L.i2l_version() >= 115 and _lib.ABI_VERSION >= 115       # moved in api.hip and in the binding's check
    api = open(os.path.join(REPO, "hmer-img2latex_amd", "csrc", "api.hip")).read()
    assert int(re.search(r"i2l_version\(void\)\s*\{\s*return\s+(\d+);", api).group(1)) == L.i2l_version()


def test_scratch_size_query():
    q, loop = _lib.lib().i2l_sample_multi_scratch_bytes, _lib.lib().i2l_decode_batched_scratch_bytes
    V, H, L = 500, 512, 2
    for what, args in {"samples 0": (4, 0, V, H, L, 150, 0), "samples 17": (4, 17, V, H, L, 150, 0),
                       "steps 1025": (4, 5, V, H, L, 1025, 0), "steps 0": (4, 5, V, H, L, 0, 0),
                       "images 0": (0, 5, V, H, L, 150, 0), "V 2049": (4, 5, 2049, H, L, 150, 0),
                       "H 96": (4, 5, V, 96, L, 150, 0), "L 5": (4, 5, V, H, 5, 150, 0), "kind 3": (4, 5, V, H, L, 150, 3),
                       "kind -1": (4, 5, V, H, L, 150, -1)}.items():
        assert q(*args) == 0, what
    for n, s in ((1, 1), (16, 16), (64, 4), (7, 5)):
        plain, brackets, arguments = (q(n, s, V, H, L, 150, k) for k in (0, 1, 2))
        assert plain >= loop(n * s, V, H, L) > 0                      # the loop's scratch for images * samples rows
        assert brackets >= plain + 16 * n * s and arguments >= plain + 32 * n * s          # the rows' states, 16 or 32 bytes
        assert arguments >= brackets > plain and (n * s < 16 or arguments > brackets)
    assert q(1, 1, 37, 64, 1, 1, 0) > 0 and q(3, 16, 500, 512, 2, 1024, 2) > 0


def _weights(V=500, E=512, H=512, L=2):
    arrs = [(ctypes.c_void_p * max(L, 1))(*([FAKE] * max(L, 1))) for _ in range(4)]
    w = _lib.DecoderWeights()
    w.embedding, w.w_out, w.b_out = FAKE, FAKE, FAKE
    w.w_ih, w.w_hh, w.b_ih, w.b_hh = arrs
    w.vocab, w.embed, w.hidden, w.layers = V, E, H, L
    return w, arrs


OUTS = ("ids", "ln", "fin", "score", "risk", "key", "order")


def _multi(w, images=4, samples=5, steps=6, tok0=FAKE, temperature=1.0, top_k=5, top_p=0.9, end_id=2, kind=0, cls=None,
           rank=0, norm=None, workspace=FAKE, scratch=FAKE, scratch_bytes=1 << 40, **outs):
    o = [outs.get(k, FAKE) for k in OUTS]
    return _lib.lib().i2l_sample_decode_multi(ctypes.byref(w) if w is not None else None, workspace, images, samples, steps,
                                              tok0, temperature, top_k, top_p, 7, end_id, kind, cls, rank, norm, scratch,
                                              scratch_bytes, *o, 0, None)


MULTI_REFUSALS = [
    ("weights null", dict(w=None), _lib.ERR_ARG), ("workspace null", dict(workspace=None), _lib.ERR_ARG),
    ("tok0 null", dict(tok0=None), _lib.ERR_ARG),
] + [(f"{k}_out null", {k: None}, _lib.ERR_ARG) for k in OUTS] + [
    ("images 0", dict(images=0), _lib.ERR_ARG), ("steps 0", dict(steps=0), _lib.ERR_ARG),
    ("samples 0", dict(samples=0), _lib.ERR_ARG), ("samples 17", dict(samples=17), _lib.ERR_UNSUPPORTED),
    ("steps 1025", dict(steps=1025), _lib.ERR_UNSUPPORTED),
    ("rank 2", dict(rank=2), _lib.ERR_ARG), ("rank -1", dict(rank=-1), _lib.ERR_ARG),
    ("kind 3", dict(kind=3, cls=FAKE), _lib.ERR_ARG), ("kind -1", dict(kind=-1, cls=FAKE), _lib.ERR_ARG),
    ("brackets without cls", dict(kind=1), _lib.ERR_ARG), ("arguments without cls", dict(kind=2), _lib.ERR_ARG),
    ("brackets: end_id -1", dict(kind=1, cls=FAKE, end_id=-1), _lib.ERR_ARG),
    ("arguments: end_id == vocab", dict(kind=2, cls=FAKE, end_id=500), _lib.ERR_ARG),
    ("temperature 0", dict(temperature=0.0), _lib.ERR_ARG), ("temperature nan", dict(temperature=float("nan")), _lib.ERR_ARG),
    ("top_k and top_p zero", dict(top_k=0, top_p=0.0), _lib.ERR_ARG), ("top_k -1", dict(top_k=-1), _lib.ERR_ARG),
    ("top_p nan", dict(top_p=float("nan")), _lib.ERR_ARG),
    ("V 2049", dict(V=2049), _lib.ERR_UNSUPPORTED), ("H 96", dict(H=96), _lib.ERR_UNSUPPORTED),
    ("L 5", dict(L=5), _lib.ERR_UNSUPPORTED),
    ("scratch null", dict(scratch=None), _lib.ERR_WORKSPACE), ("scratch 0 bytes", dict(scratch_bytes=0), _lib.ERR_WORKSPACE),
    ("scratch one byte short", dict(short=0), _lib.ERR_WORKSPACE),
    ("brackets: the plain scratch size", dict(short=1, kind=1, cls=FAKE), _lib.ERR_WORKSPACE),
    ("arguments: the brackets' scratch size", dict(short=2, kind=2, cls=FAKE), _lib.ERR_WORKSPACE),
]


@pytest.mark.parametrize("what,kw,code", MULTI_REFUSALS, ids=[r[0] for r in MULTI_REFUSALS])
def test_decode_multi_refusals_need_no_device(what, kw, code):
    """Every pointer is null or fake: a call that touched the device, or followed one of them, would not return a code."""
    kw = dict(kw)
    w, keep = _weights(**{k: kw.pop(k) for k in ("V", "H", "L") if k in kw})
    if "w" in kw:
        w = kw.pop("w")
    short = kw.pop("short", None)
    if short is not None:
        q = _lib.lib().i2l_sample_multi_scratch_bytes
        kw["scratch_bytes"] = q(4, 5, 500, 512, 2, 6, 0) - 1 if short == 0 else q(4, 5, 500, 512, 2, 6, short - 1)
        assert kw["scratch_bytes"] > 0
    assert _multi(w, **kw) == code, what
    del keep


def _rank(ids=FAKE, images=3, samples=5, steps=7, score=FAKE, rank=0, norm=None, dist=None, **outs):
    o = [outs.get(k, FAKE) for k in ("ln", "fin", "risk", "key", "order")]
    return _lib.lib().i2l_sample_rank(ids, images, samples, steps, END, score, rank, norm, *o, dist, None)


RANK_REFUSALS = [
    ("ids null", dict(ids=None), _lib.ERR_ARG), ("score null", dict(score=None), _lib.ERR_ARG),
] + [(f"{k}_out null", {k: None}, _lib.ERR_ARG) for k in ("ln", "fin", "risk", "key", "order")] + [
    ("images 0", dict(images=0), _lib.ERR_ARG), ("samples 0", dict(samples=0), _lib.ERR_ARG),
    ("steps 0", dict(steps=0), _lib.ERR_ARG), ("samples 17", dict(samples=17), _lib.ERR_UNSUPPORTED),
    ("steps 1025", dict(steps=1025), _lib.ERR_UNSUPPORTED), ("rank 2", dict(rank=2), _lib.ERR_ARG),
]


@pytest.mark.parametrize("what,kw,code", RANK_REFUSALS, ids=[r[0] for r in RANK_REFUSALS])
def test_rank_refusals_need_no_device(what, kw, code):
    assert _rank(**kw) == code, what


# ------------------------------------------------------------------------------------------------ the Python surface
def _tiny_model():
    from img2latex_amd import synth
    from img2latex_amd.model import Seq2SeqModel
    cfg = synth.model_config(vocab_size=10, embedding_dim=8, hidden_dim=64, lstm_layers=1, attention=False, channels=1,
                             img_height=16, img_width=32, conv_filters=(4, 8, 16))
    return cfg, Seq2SeqModel("cnn_lstm", 10, synth.encoder_params(cfg), synth.decoder_params(cfg))


def test_sample_nbest_refuses_before_any_launch():
    from img2latex_amd.model import SampleHypothesis
    assert SampleHypothesis._fields == ("tokens", "score", "key", "risk", "finished", "sample")
    _, m = _tiny_model()
    enc = torch.zeros(2, 8)                                # on the host: anything that got as far as prepare() would raise
    with pytest.raises(ValueError, match="unknown rank"):
        m.sample_nbest(enc, 1, 2, 8, 4, top_k=5, rank="mbr")
    for n in (0, 17):
        with pytest.raises(ValueError, match="1 .. 16"):
            m.sample_nbest(enc, 1, 2, 8, n, top_k=5)
    with pytest.raises(ValueError, match="length_norm needs"):
        m.sample_nbest(enc, 1, 2, 8, 4, top_k=5, rank="logprob", length_norm=[1.0, 2.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.sample_nbest(enc, 1, 2, 8, 4, top_k=5)


def test_ensemble_refuses_the_consensus_decode():
    from img2latex_amd.model import EnsembleModel
    from img2latex_amd.training import Predictor
    models = [_tiny_model()[1] for _ in range(2)]
    ens = EnsembleModel(models)
    with pytest.raises(RuntimeError, match="sample_nbest over an ensemble"):
        ens.sample_nbest(None, 1, 2, 8, 4)
    p = Predictor.__new__(Predictor)                       # the constructor wants a device; the refusal reads the model alone
    p.model = ens
    with pytest.raises(RuntimeError, match="predict_samples is single-model"):
        p.predict_samples(torch.zeros(1, 16, 32), samples=4, top_k=5)
    with pytest.raises(RuntimeError, match="predict_batch_samples is single-model"):
        p.predict_batch_samples([torch.zeros(1, 16, 32)], samples=4, top_k=5)


def test_cli_option_rules(monkeypatch, capsys):
    from img2latex_amd import cli
    base = ["predict", "ck.pt", "x.png"]
    for argv, said in ((["--samples", "4", "--top-k", "5", "--beam-size", "3"], "--samples with --beam-size"),
                       (["--samples", "4", "--top-k", "5", "--nbest", "2"], "--samples with --nbest"),
                       (["--samples", "4", "--top-k", "5", "--ensemble", "b.pt"], "--samples with --ensemble"),
                       (["--samples", "17", "--top-k", "5"], "--samples must be 1 .. 16"),
                       (["--samples", "-1", "--top-k", "5"], "--samples must be 1 .. 16"),
                       (["--samples", "4"], "--samples needs --top-k or --top-p"),
                       (["--samples", "4", "--top-k", "5", "--rank", "mbr"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + argv)
        assert e.value.code == 2, argv
        assert said in capsys.readouterr().err, argv
    seen = []

    def fake(checkpoint_path, image_path, samples, rank, max_length, temperature, top_k, top_p, seed, *args, **kw):
        seen.append((samples, rank, top_k, top_p, seed, kw.get("well_formed")))
        return [("x ^ { 2 }", -1.0, 3.0), ("x ^ 2", -2.0, 5.0)]
    monkeypatch.setattr(cli, "predict_samples", fake)
    assert cli.main(base + ["--samples", "2", "--top-k", "5", "--seed", "11"]) == 0
    assert cli.main(base + ["--samples", "16", "--top-p", "0.9", "--rank", "logprob", "--well-formed"]) == 0
    assert cli.main(base + ["--samples", "1", "--top-k", "3", "--complete-arguments"]) == 0
    assert seen == [(2, "consensus", 5, 0.0, 11, False), (16, "logprob", 0, 0.9, 0, True), (1, "consensus", 3, 0.0, 0, "arguments")]
    assert capsys.readouterr().out == "3.0\tx ^ { 2 }\n5.0\tx ^ 2\n" * 3
