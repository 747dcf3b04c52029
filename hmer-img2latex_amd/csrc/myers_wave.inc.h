// The Levenshtein distance of two token rows by ONE wave (included inside an anonymous namespace by decode.hip, through
// sample_rank.inc.h, and by train_risk.hip): Myers' bit-vector algorithm in blocks of 64 tokens, as metrics.hip's
// sequence_metrics_bp_kernel walks it (J. ACM 46(3) 1999; global-distance boundary as in Hyyro 2003).
//
// Row a's tokens sit in registers, lane = place within a block, W blocks; per token of row b a ballot yields the match
// mask of a block and ~20 scalar bit operations its new vertical deltas and the carry into the next block.  Row b's tokens
// sit in registers too and are read lane by lane, so the walk touches no memory at all.  Exact: integers throughout.
// Every loop is bounded by 64 W.
//
//   pa[w], tb[w]   lane l holds token 64 w + l of row a / row b (anything where that place is outside the row)
//   R, C           the rows' lengths after the cut, 0 <= R, C <= 64 W; wave-uniform
// Every lane of the wave calls it and every lane returns d(a[0, R), b[0, C)).
#pragma once

template <int W>
__device__ inline int wave_edit_distance(const int (&pa)[W], int R, const int (&tb)[W], int C, int lane) {
    typedef unsigned long long u64;
    int d = R;
    if (R == 0) d = C;
    else if (C > 0) {
        bool ok[W];
        u64 Pv[W], Mv[W];
#pragma unroll
        for (int w = 0; w < W; ++w) { ok[w] = 64 * w + lane < R; Pv[w] = ~0ull; Mv[w] = 0ull; }
        const int last = (R - 1) >> 6;
        const u64 high = 1ull << ((R - 1) & 63);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int nk = min(64, C - 64 * k);          // tokens of row b in its block k
            for (int jj = 0; jj < nk; ++jj) {
                const int t = __builtin_amdgcn_readlane(tb[k], jj);
                int hin = 1;                             // D[0][j] - D[0][j-1] = +1: global distance
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    if (w <= last) {
                        u64 Eq = __ballot(ok[w] && pa[w] == t);
                        const u64 pv = Pv[w], mv = Mv[w];
                        const u64 Xv = Eq | mv;
                        if (hin < 0) Eq |= 1ull;
                        const u64 Xh = (((Eq & pv) + pv) ^ pv) | Eq;
                        u64 Ph = mv | ~(Xh | pv);
                        u64 Mh = pv & Xh;
                        const u64 hb = w == last ? high : (1ull << 63);
                        const int hout = (Ph & hb) ? 1 : ((Mh & hb) ? -1 : 0);
                        Ph <<= 1;
                        Mh <<= 1;
                        if (hin < 0) Mh |= 1ull;
                        else if (hin > 0) Ph |= 1ull;
                        Pv[w] = Mh | ~(Xv | Ph);
                        Mv[w] = Ph & Xv;
                        hin = hout;
                    }
                }
                d += hin;                                // D[R][j+1] - D[R][j]
            }
        }
    }
    return d;
}
