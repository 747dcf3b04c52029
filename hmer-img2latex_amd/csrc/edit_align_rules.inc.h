// The rules of the error analysis (i2l_edit_alignment), stated once: which edit script of a (target, prediction) pair is
// THE script, and what it adds to the token confusion matrix.  Shared by edit_align.hip (the device kernels) and a
// stand-alone host program (edit_align_host_main.cpp) that a host test compares with the Python restatement
// (tests/edit_align_ref.py).
//
// Plain C++, no HIP: BR_HD is `__host__ __device__` under hipcc and empty elsewhere.  Every function is called by ONE
// thread; the arrays it gets are the caller's.
//
//   table     for a target r[0, m) and a prediction p[0, n), D[i][j] is the Levenshtein table of r[0, i) against p[0, j):
//             D[i][0] = i, D[0][j] = j, equal tokens copy the diagonal, otherwise 1 + min(up, left, diagonal) -- the
//             recurrence of the reference's training/metrics.py:73-81, so D[m][n] is i2l_sequence_metrics' integer.
//   script    the backtrace from (m, n) to (0, 0); at (i, j) the FIRST of these that applies (ea_op):
//               1. i > 0, j > 0, r[i-1] == p[j-1] and D[i][j] == D[i-1][j-1]      match          -> (i-1, j-1)
//               2. i > 0, j > 0 and D[i][j] == D[i-1][j-1] + 1                    substitution   -> (i-1, j-1)
//               3. i > 0 and D[i][j] == D[i-1][j] + 1                             deletion of r[i-1]  -> (i-1, j)
//               4. otherwise                                                      insertion of p[j-1] -> (i, j-1)
//             reported in forward order, one byte per operation (EA_MATCH .. EA_INS), at most m + n of them.
//   confusion C is (V+1) x (V+1) uint32, row = target id or V for "nothing", column = predicted id or V: a match or a
//             substitution of a by b adds 1 to C[a][b], a deletion of a to C[a][V], an insertion of b to C[V][b]; C[V][V]
//             stays 0.  An operation with an id outside [0, V) is part of the script and of the counts (ids are only
//             compared for equality) and adds nothing to C.
//
// The device does not keep the table.  It keeps, per column j >= 1 and per block of 64 rows, two bit vectors of Myers'
// column pass (J. ACM 46(3) 1999, block formulation; Hyyro 2003 for the diagonal vector): bit i-1 of
//   pv  is set iff D[i][j] == D[i-1][j] + 1          (rule 3's test)
//   d0  is set iff D[i][j] == D[i-1][j-1]            (a diagonal step is 0 or 1: rules 1 and 2's tests)
// which is all the backtrace asks of the table (ea_block_step computes them, EaBitCells reads them).  The host program
// runs both the full table and the bit vectors through the same walk.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BR_HD __host__ __device__ inline
#else
#define BR_HD inline
#endif

#define EA_MATCH 0
#define EA_SUB 1
#define EA_DEL 2
#define EA_INS 3
#define EA_MAX_STRIDE 1024       // the decode's own step limit
#define EA_MAX_VOCAB 2048

typedef unsigned long long ea_u64;

// The operation at (i, j), (i, j) != (0, 0).  eq: r[i-1] == p[j-1]; d, d_diag, d_up: D[i][j], D[i-1][j-1], D[i-1][j]; only
// their differences matter, and a neighbour that does not exist (i == 0 or j == 0) is not looked at.
BR_HD int ea_op(int i, int j, bool eq, int d, int d_diag, int d_up) {
    if (i > 0 && j > 0 && eq && d == d_diag) return EA_MATCH;
    if (i > 0 && j > 0 && d == d_diag + 1) return EA_SUB;
    if (i > 0 && d == d_up + 1) return EA_DEL;
    return EA_INS;
}

BR_HD void ea_add(uint32_t* cell) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(cell, 1u);
#else
    ++*cell;
#endif
}

// What one operation adds to C (null: nothing).  a = r[i-1] (not read for an insertion), b = p[j-1] (not for a deletion).
BR_HD void ea_count(uint32_t* C, int V, int op, int a, int b) {
    if (!C) return;
    if (op != EA_INS && (a < 0 || a >= V)) return;
    if (op != EA_DEL && (b < 0 || b >= V)) return;
    const size_t row = op == EA_INS ? (size_t)V : (size_t)a, col = op == EA_DEL ? (size_t)V : (size_t)b;
    ea_add(C + row * ((size_t)V + 1) + col);
}

// The full table, (m + 1) x (n + 1) ints of the caller, row-major.
BR_HD void ea_table(const int32_t* r, int m, const int32_t* p, int n, int* D) {
    const size_t ld = (size_t)n + 1;
    for (int j = 0; j <= n; ++j) D[j] = j;
    for (int i = 1; i <= m; ++i) {
        D[i * ld] = i;
        for (int j = 1; j <= n; ++j) {
            int v;
            if (r[i - 1] == p[j - 1]) v = D[(i - 1) * ld + j - 1];
            else {
                v = D[(i - 1) * ld + j - 1];
                if (D[(i - 1) * ld + j] < v) v = D[(i - 1) * ld + j];
                if (D[i * ld + j - 1] < v) v = D[i * ld + j - 1];
                v += 1;
            }
            D[i * ld + j] = v;
        }
    }
}

struct EaTableCells {
    const int* D;
    size_t ld;
    BR_HD void at(int i, int j, int& d, int& d_diag, int& d_up) const {
        d = D[i * ld + j];
        d_diag = i > 0 && j > 0 ? D[(i - 1) * ld + j - 1] : 0;
        d_up = i > 0 ? D[(i - 1) * ld + j] : 0;
    }
};

// One block of 64 rows of one column.  eq: bit k set iff the block's k-th target token equals the column's prediction
// token; pv / mv: the block's vertical +1 / -1 vectors of the previous column on entry (column 0: all ones / zero), of
// this column on return; hin: D[top][j] - D[top][j-1] of the row above the block (+1 above block 0); d0: this column's
// diagonal vector.  Returns the same difference for the block's last row, the next block's hin.
BR_HD int ea_block_step(ea_u64 eq, ea_u64& pv, ea_u64& mv, int hin, ea_u64& d0) {
    const ea_u64 xv = eq | mv;
    if (hin < 0) eq |= 1ull;
    const ea_u64 xh = (((eq & pv) + pv) ^ pv) | eq;
    d0 = xh | mv;
    ea_u64 ph = mv | ~(xh | pv);
    ea_u64 mh = pv & xh;
    const int hout = (ph >> 63) ? 1 : ((mh >> 63) ? -1 : 0);
    ph <<= 1;
    mh <<= 1;
    if (hin < 0) mh |= 1ull;
    else if (hin > 0) ph |= 1ull;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
    return hout;
}

// The vectors of every column: vec[((j - 1) * W + w) * 2] = pv, [.. + 1] = d0 of column j's block w.
struct EaBitCells {
    const ea_u64* vec;
    int W;
    BR_HD void at(int i, int j, int& d, int& d_diag, int& d_up) const {
        d = 0; d_diag = 0; d_up = i > 0 ? -1 : 0;             // column 0: D[i][0] = D[i-1][0] + 1
        if (i > 0 && j > 0) {
            const ea_u64* b = vec + ((size_t)(j - 1) * W + ((i - 1) >> 6)) * 2;
            const int k = (i - 1) & 63;
            d_up = ((b[0] >> k) & 1ull) ? -1 : 0;
            d_diag = ((b[1] >> k) & 1ull) ? 0 : -1;
        }
    }
};

// The column pass on the host (the device builds eq with a ballot): W >= ceil(m / 64) blocks, vec of n * W * 2 words.
BR_HD void ea_fill_columns(const int32_t* r, int m, const int32_t* p, int n, int W, ea_u64* vec, ea_u64* pv, ea_u64* mv) {
    for (int w = 0; w < W; ++w) { pv[w] = ~0ull; mv[w] = 0ull; }
    for (int j = 1; j <= n; ++j) {
        int hin = 1;
        for (int w = 0; w < W; ++w) {
            ea_u64 eq = 0, d0;
            for (int k = 0; k < 64; ++k)
                if (64 * w + k < m && r[64 * w + k] == p[j - 1]) eq |= 1ull << k;
            hin = ea_block_step(eq, pv[w], mv[w], hin, d0);
            vec[((size_t)(j - 1) * W + w) * 2] = pv[w];
            vec[((size_t)(j - 1) * W + w) * 2 + 1] = d0;
        }
    }
}

// The backtrace.  rev[0, m + n): the operations LAST first (the script is rev reversed); ops[4]: the number of matches,
// substitutions, deletions, insertions; C: see ea_count.  Returns the script's length.
template <class Cells>
BR_HD int ea_walk(const int32_t* r, int m, const int32_t* p, int n, const Cells& cells, int V, uint8_t* rev, int32_t* ops,
                  uint32_t* C) {
    int i = m, j = n, len = 0;
    int n_match = 0, n_sub = 0, n_del = 0;                 // in registers: a step is one round of independent loads
    while (i > 0 || j > 0) {
        const int a = i > 0 ? r[i - 1] : 0, b = j > 0 ? p[j - 1] : 0;
        int d, d_diag, d_up;
        cells.at(i, j, d, d_diag, d_up);
        const int op = ea_op(i, j, i > 0 && j > 0 && a == b, d, d_diag, d_up);
        ea_count(C, V, op, a, b);
        rev[len++] = (uint8_t)op;
        n_match += op == EA_MATCH ? 1 : 0;
        n_sub += op == EA_SUB ? 1 : 0;
        n_del += op == EA_DEL ? 1 : 0;
        if (op != EA_INS) --i;
        if (op != EA_DEL) --j;
    }
    ops[EA_MATCH] = n_match;
    ops[EA_SUB] = n_sub;
    ops[EA_DEL] = n_del;
    ops[EA_INS] = len - n_match - n_sub - n_del;
    return len;
}
