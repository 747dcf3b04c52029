"""The beam search's serial rules (csrc/beam_rules.inc.h: retirement, the ranking of the K x K candidates, the step's
ending, the results) as a stand-alone host program (csrc/beam_rules_host_main.cpp), a process of its own under the host
sanitizers, against a Python restatement built on ``sorted(..., reverse=True)`` and Python floats: the loop of
nbest_ref.search with the decoder step replaced by a table of (log-prob, token) pairs per (step, slot), then
nbest_ref.rank.  The log-probs come from four dyadic values, so candidates of different slots, candidates inside one slot
and keys of the N-best list tie EXACTLY -- what these rules decide and real logits almost never produce.  Both sides add
the same doubles in the same order: tokens, lengths, finished flags, counts and the bits of scores and keys are equal."""
import os
import random
import struct
import subprocess

import nbest_ref
import png_cases
from img2latex_amd import _lib

LOGPS = (-0.25, -0.5, -0.75, -1.0)
START, END = 0, 1


def make_case(seed, K, T, N, norm=False, p_end=0.15, start=START, all_end_at=None, end_at_last=False):
    """table[t][s]: the K (logp, token) pairs of slot s at step t, descending; tokens of a slot distinct."""
    rng = random.Random(seed)
    other = [v for v in range(K + 4) if v != END]
    table = []
    for t in range(T):
        row = []
        for s in range(K):
            lps = sorted((rng.choice(LOGPS) for _ in range(K)), reverse=True)
            toks = rng.sample(other, K)
            if all_end_at == t:
                toks = [END] * K                                                # every new beam ends
            elif end_at_last:
                if t == T - 1 and s == 0:
                    lps[0], toks[0] = LOGPS[0], END                             # slot 0's best candidate: always selected
            elif rng.random() < p_end:
                toks[rng.randrange(K)] = END
            row.append(list(zip(lps, toks)))
        table.append(row)
    table_norm = [1.0] + [float(n) ** 0.7 for n in range(1, T + 1)] if norm else None
    return dict(K=K, T=T, N=N, start=start, end=END, norm=table_norm, table=table)


def cases():
    out = []
    seed = 0
    for K in (1, 2, 5, 8):
        for N in (1, 3, _lib.MAX_NBEST):
            for norm in (False, True):
                for T, p_end in ((12, 0.15), (7, 0.5), (3, 0.0)):
                    seed += 1
                    out.append(make_case(seed, K, T, N, norm, p_end))
                out.append(make_case(1000 + seed, K, 9, N, norm, all_end_at=2))
                out.append(make_case(2000 + seed, K, 6, N, norm, end_at_last=True))
                out.append(make_case(3000 + seed, K, 5, N, norm, start=END))    # START == END: no beam is ever live
    return out


def search(c) -> nbest_ref.Search:
    """nbest_ref.search, the decoder step replaced by the table."""
    K, end = c["K"], c["end"]
    beams, completed, ran_out = [([c["start"]], 0.0)], [], True
    for t in range(c["T"]):
        cands = []
        for s, (tokens, score) in enumerate(beams):
            if tokens[-1] == end:
                completed.append((tokens, score))
                continue
            for lp, ix in c["table"][t][s]:
                cands.append((tokens + [ix], score + lp))
        if not cands:
            ran_out = False
            break
        beams = sorted(cands, key=lambda b: b[1], reverse=True)[:K]
        if all(b[0][-1] == end for b in beams):
            completed.extend(beams)
            ran_out = False
            break
    return nbest_ref.Search(completed, beams, ran_out, float("inf"))


def write_cases(path, cs):
    with open(path, "wb") as f:
        f.write(b"BEAM" + struct.pack("<i", len(cs)))
        for c in cs:
            f.write(struct.pack("<6i", c["K"], c["T"], c["N"], c["start"], c["end"], c["norm"] is not None))
            if c["norm"] is not None:
                f.write(struct.pack(f"<{c['T'] + 1}d", *c["norm"]))
            for row in c["table"]:
                for slot in row:
                    for lp, tok in slot:
                        f.write(struct.pack("<fi", lp, tok))


def read_results(path, cs):
    """[(best: (len, score bytes, seq), count, rows: [(len, finished, score bytes, key bytes, seq)])]"""
    data, pos, out = open(path, "rb").read(), 0, []

    def take(fmt):
        nonlocal pos
        v = struct.unpack_from(fmt, data, pos)
        pos += struct.calcsize(fmt)
        return v

    for c in cs:
        seq = f"<{c['T'] + 1}i"
        (ln,), sc = take("<i"), take("<8s")[0]
        best = (ln, sc, list(take(seq)))
        (count,) = take("<i")
        rows = []
        for _ in range(c["N"]):
            ln, fin, sc, key = take("<ii8s8s")
            rows.append((ln, fin, sc, key, list(take(seq))))
        out.append((best, count, rows))
    assert pos == len(data)
    return out


def bits(x):
    return struct.pack("<d", x)


def padded(tokens, T):
    return tokens + [-1] * (T + 1 - len(tokens))


def test_the_rules_as_a_sanitized_host_program(tmp_path):
    cs = cases()
    exe, sanitized = png_cases.build_host_program(str(tmp_path), "beam_rules_host_main")
    print("beam_rules_host_main built", "with -fsanitize=address,undefined" if sanitized else "PLAIN: the sanitizer build did not link")
    assert sanitized or os.environ.get("I2L_PNG_HOST_PLAIN") == "1", \
        "the sanitized build of beam_rules_host_main failed; set I2L_PNG_HOST_PLAIN=1 to accept a plain build on a machine without the runtime"
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    write_cases(src, cs)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])

    seen = set()
    for i, (c, (best, count, rows)) in enumerate(zip(cs, read_results(dst, cs))):
        K, T, N, end = c["K"], c["T"], c["N"], c["end"]
        s = search(c)
        # the best-completed result: max(completed), first on ties, else beams[0] (seq2seq.py:286-297)
        tokens, score = max(s.completed, key=lambda b: b[1]) if s.completed else s.beams[0]
        tokens = nbest_ref._strip(tokens, c["start"], end)
        assert best == (len(tokens), bits(score), padded(tokens, T)), i
        # the N-best rows
        want = nbest_ref.rank(s, c["start"], end, T, N, c["norm"])
        assert count == len(want), i
        for j, row in enumerate(rows):
            if j < count:
                w = want[j]
                assert row == (len(w.tokens), int(w.finished), bits(w.score), bits(w.key), padded(w.tokens, T)), (i, j)
            else:
                assert row == (-1, 0, bits(float("-inf")), bits(float("-inf")), [-1] * (T + 1)), (i, j)

        # what this case exercised
        seen.add(("K", K))
        seen.add(("N", N))
        seen.add("norm" if c["norm"] else "no norm")
        seen.add("more completed than N" if len(s.completed) > N else "fewer completed than N" if len(s.completed) < N else "N completed")
        if c["start"] == end:
            assert s.completed == [([end], 0.0)] and not s.ran_out and count == 1 and rows[0][0] == 0
            seen.add("START == END")
        if s.ran_out and any(w.finished for w in want[min(N, len(s.completed)):]):
            seen.add("a beam ends at the very last step")               # a leftover row, finished all the same
        if not s.ran_out and s.completed and all(b[0][-1] == end for b in s.beams) and c["start"] != end:
            seen.add("every new beam ends")
        keys = [w.key for w in want if w.finished]
        if any(a == b for a, b in zip(keys[:-1], keys[1:])):
            seen.add("equal keys in the list")
        # exact ties between the candidates of a step: different slots, and inside one slot
        beams = [([c["start"]], 0.0)]
        for t in range(min(T, 3)):
            sc = [(slot, score + lp) for slot, (tk, score) in enumerate(beams) if tk[-1] != end for lp, _ in c["table"][t][slot]]
            for a in range(len(sc)):
                for b in range(a + 1, len(sc)):
                    if sc[a][1] == sc[b][1]:
                        seen.add("tie inside a slot" if sc[a][0] == sc[b][0] else "tie between slots")
            if not sc:
                break
            order = sorted(((slot, lp, ix) for slot, (tk, score) in enumerate(beams) if tk[-1] != end
                            for lp, ix in c["table"][t][slot]), key=lambda e: beams[e[0]][1] + e[1], reverse=True)[:K]
            beams = [(beams[slot][0] + [ix], beams[slot][1] + lp) for slot, lp, ix in order]
    need = {("K", 1), ("K", 2), ("K", 5), ("K", 8), ("N", 1), ("N", 3), ("N", _lib.MAX_NBEST), "norm", "no norm",
            "more completed than N", "fewer completed than N", "START == END", "a beam ends at the very last step",
            "every new beam ends", "equal keys in the list", "tie inside a slot", "tie between slots"}
    assert need <= seen, need - seen
