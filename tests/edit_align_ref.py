"""Python restatement of the error analysis' rules (csrc/edit_align_rules.inc.h): the full Levenshtein table, the
canonical backtrace and the confusion update, written from the rules' text and not from the C++."""
import struct

import numpy as np

MATCH, SUB, DEL, INS = 0, 1, 2, 3


def table(r, p):
    """D[i][j]: the Levenshtein table of the target r[0, i) against the prediction p[0, j)."""
    m, n = len(r), len(p)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        D[i][0] = i
    for j in range(n + 1):
        D[0][j] = j
    for i in range(1, m + 1):
        ri, Di, Dp = r[i - 1], D[i], D[i - 1]
        for j in range(1, n + 1):
            if ri == p[j - 1]:
                Di[j] = Dp[j - 1]
            else:
                Di[j] = 1 + min(Dp[j - 1], Dp[j], Di[j - 1])
    return D


def table_fast(r, p):
    """The same table a row at a time in numpy, for the long pairs of the GPU test (the host test holds it to ``table``):
    t[j] = min(diagonal + (tokens differ), up + 1) needs no left neighbour, and D[i][j] = min(t[j], D[i][j-1] + 1)
    unrolls to min over k <= j of t[k] + (j - k), a running minimum of t[k] - k."""
    m, n = len(r), len(p)
    pa = np.asarray(p, dtype=np.int64).reshape(n)
    D = np.zeros((m + 1, n + 1), dtype=np.int64)
    D[0] = np.arange(n + 1)
    ar = np.arange(n + 1)
    for i in range(1, m + 1):
        t = np.empty(n + 1, dtype=np.int64)
        t[0] = i
        t[1:] = np.minimum(D[i - 1, :-1] + (pa != r[i - 1]), D[i - 1, 1:] + 1)
        D[i] = np.minimum.accumulate(t - ar) + ar
    return D


def script(r, p, table=table):
    """The canonical script in forward order, one operation code per step."""
    D = table(r, p)
    i, j, rev = len(r), len(p), []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and r[i - 1] == p[j - 1] and D[i][j] == D[i - 1][j - 1]:
            rev.append(MATCH)
            i, j = i - 1, j - 1
        elif i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + 1:
            rev.append(SUB)
            i, j = i - 1, j - 1
        elif i > 0 and D[i][j] == D[i - 1][j] + 1:
            rev.append(DEL)
            i -= 1
        else:
            rev.append(INS)
            j -= 1
    return rev[::-1]


def counts(ops):
    return [ops.count(k) for k in (MATCH, SUB, DEL, INS)]


def confusion_update(C, r, p, ops, V):
    """Adds one pair's script to the (V+1, V+1) matrix C in place."""
    i = j = 0
    for op in ops:
        if op in (MATCH, SUB):
            a, b = r[i], p[j]
            if 0 <= a < V and 0 <= b < V:
                C[a, b] += 1
            i, j = i + 1, j + 1
        elif op == DEL:
            if 0 <= r[i] < V:
                C[r[i], V] += 1
            i += 1
        else:
            if 0 <= p[j] < V:
                C[V, p[j]] += 1
            j += 1
    assert i == len(r) and j == len(p)


def replay(r, p, ops):
    """The prediction that the script makes of the target (substitutions and insertions take their token from p)."""
    i = j = 0
    out = []
    for op in ops:
        if op == MATCH:
            out.append(r[i])
            i, j = i + 1, j + 1
        elif op == SUB:
            out.append(p[j])
            i, j = i + 1, j + 1
        elif op == DEL:
            i += 1
        else:
            out.append(p[j])
            j += 1
    assert i == len(r)
    return out


def align_batch(p_ids, p_len, t_ids, t_len, V, table=table):
    """What i2l_edit_alignment returns for id matrices: ops (P, 4), scripts (list of lists), C (V+1, V+1) uint32.
    Lengths are clamped to [0, width]."""
    P = len(p_len)
    ops_all = np.zeros((P, 4), dtype=np.int32)
    C = np.zeros((V + 1, V + 1), dtype=np.int64)
    scripts = []
    for k in range(P):
        n = min(max(int(p_len[k]), 0), p_ids.shape[1])
        m = min(max(int(t_len[k]), 0), t_ids.shape[1])
        r, p = [int(v) for v in t_ids[k, :m]], [int(v) for v in p_ids[k, :n]]
        s = script(r, p, table)
        scripts.append(s)
        ops_all[k] = counts(s)
        confusion_update(C, r, p, s, V)
    return ops_all, scripts, C.astype(np.uint32)


# ---- the case file of csrc/edit_align_host_main.cpp

def write_cases(path, cases):
    """cases: [(r, p, V)]."""
    with open(path, "wb") as f:
        f.write(b"EALN" + struct.pack("<i", len(cases)))
        for r, p, V in cases:
            f.write(struct.pack("<3i", len(r), len(p), V))
            f.write(np.asarray(r, dtype="<i4").tobytes() + np.asarray(p, dtype="<i4").tobytes())


def read_results(path, cases):
    """-> per case [(ops[4], script, C)] x 2: from the table, from the bit vectors."""
    buf = open(path, "rb").read()
    pos, out = 0, []
    for r, p, V in cases:
        both = []
        for _ in range(2):
            head = struct.unpack_from("<5i", buf, pos)
            pos += 20
            s = list(buf[pos:pos + head[0]])
            pos += head[0]
            cells = (V + 1) * (V + 1)
            C = np.frombuffer(buf, dtype="<u4", count=cells, offset=pos).reshape(V + 1, V + 1)
            pos += 4 * cells
            both.append((list(head[1:]), s, C))
        out.append(both)
    assert pos == len(buf)
    return out
