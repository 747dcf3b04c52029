// The argument rules of the constrained decode, stated once: bracket_rules.inc.h's nesting rules plus arity -- every
// column that demands arguments (\frac's two groups, the operand of ^) gets them.  Which vocabulary columns a row may
// emit at a step, what the pick does to the row's state, and what is picked when a malformed table leaves nothing.
// Shared by the selection kernels' pick policy (decode_constrained.inc.h) and a stand-alone host program
// (argument_rules_host_main.cpp) that a host test compares with the Python restatement (training/constraint.py
// ArgumentTable) step by step and with an independent recogniser over every short sequence.
//
// Plain C++, no HIP: BR_HD is `__host__ __device__` under hipcc and empty elsewhere.  Every function is called by ONE
// thread (ar_rule / ar_allowed by any number of threads on their own copy of the row's scalars).
//
// Table: one byte per column.  Bits 0..3: the bracket class of bracket_rules.inc.h (0 neutral, 1..4 opens a group of
// kind 0..3, 5..8 closes one).  Bits 4..5: the number of arguments the column demands, 0..3.  Bit 6 "loose": each of
// them may be a brace group or ONE plain token; without it each must be a brace group.  A byte is valid iff its low
// nibble is <= 8, bit 7 is clear, loose comes with a count > 0 and a closer demands nothing; every other byte (255
// among them) is never emitted.  END is named by the call (end_id); its byte is ignored.  A column may open a group
// AND demand arguments (\begin{array}: kind 2, one strict argument inside the environment).  A byte without argument
// bits is bracket_rules.inc.h's class byte and means what it means there.
//   argument opener: class 1 ({), count 0.      plain token: class 0, count 0, not END.
//
// State: the open groups as in BracketState, and per level 0..31 the arguments still owed there (2 bits) and whether
// they are loose (1 bit).  owed = sum over levels of pending * (loose ? 1 : 2): the fewest tokens that discharge every
// argument ({ and } for a strict one, a plain token for a loose one).  need(s) = owed + depth + 1 is the fewest
// emissions that finish the row: the arguments, the closers, END.
//
// With rem = steps - t - 1 emissions left after this one, d = depth, p = pending[d] (0 at d = 32) and
// room = rem - need(s), a row that has not ended may emit a column iff the first matching line says so:
//   p > 0   argument opener      iff it fits: always for a strict argument (need falls by 1), room >= 0 for a loose one
//           plain token          iff the argument is loose (need falls by 1)
//           anything else, END   never: argument expected
//   p == 0  END                  iff d == 0
//           close kind g         iff d > 0 and the innermost open group is of kind g (need falls by 1)
//           neutral, count n     iff n * w <= room, and d < 32 when n > 0        (w = 1 loose, 2 strict)
//           open,    count n     iff d < 32, 1 + n * w <= room, and d + 1 < 32 when n > 0
// which is "structurally possible and need(state after it) <= rem": a demanding column lands on level d, or d + 1 when
// it opens, and level 32 holds no pending arguments.
//
// Liveness.  need(s) <= steps - t holds at t = 0 (need = 1, steps >= 1) and every allowed pick keeps it, so room >= -1.
// A pick that lowers need by one is never refused for budget, and there always is one: the argument opener when a
// strict argument is owed, a plain token when a loose one is, else the innermost closer (d > 0) or END (d == 0).  So
// every row ends on END at depth 0 with nothing owed within `steps` steps -- provided the table has {, } and a plain
// token wherever it demands strict / loose arguments, and a closer for every open kind; ArgumentTable (constraint.py)
// builds no other.  A table that breaks this can leave NO column allowed; the pick is then end_id (constraint_fallback) --
// defined, though such a row is not complete.  With no demanding column owed is 0 throughout and the lines above are
// bracket_rules.inc.h's: neutral iff d + 1 <= rem, open iff d < 32 and d + 2 <= rem.
//
// Which rule id is reported when several apply: never emitted first; then, p > 0, "argument expected" before the
// budget; then, p == 0, the structural refusal (END inside, closer, open depth, argument depth -- open depth before
// argument depth) before the budget; a budget refusal is AR_ARG_BUDGET for a demanding column or an argument opener,
// BR_OPEN_BUDGET / BR_NEUTRAL_BUDGET otherwise.
#pragma once
#include "bracket_rules.inc.h"

constexpr int AR_STATE_BYTES = 32;

struct ArgumentState {   // 32 bytes per row; all-zero bytes are the initial state
    uint64_t stack;      // 2 bits per open group, the outermost group in the low bits
    uint64_t pending;    // 2 bits per level 0..31: the arguments still owed at that level
    uint32_t loose;      // 1 bit per level: the owed arguments are loose (as last demanded; stale once pending is 0)
    int32_t depth;       // 0 .. 32
    int32_t owed;        // sum over levels of pending * (loose ? 1 : 2)
    int32_t ended;
};
static_assert(sizeof(ArgumentState) == AR_STATE_BYTES, "32 bytes of state per row");

// ids 0..6 are BracketRuleId's, with their meanings
enum ArgumentRuleId {
    AR_ARG_EXPECTED = 7,   // an argument is owed here and the column cannot be one
    AR_ARG_BUDGET = 8,     // a demanding column, or a column that starts an argument, whose completion would not fit
    AR_ARG_DEPTH = 9,      // a demanding column that would land on level 32
};

BR_HD bool ar_valid(uint8_t c) {
    const int lo = c & 15, n = (c >> 4) & 3;
    return !(c & 0x80) && lo <= 2 * BR_KINDS && (!(c & 0x40) || n > 0) && (lo <= BR_KINDS || n == 0);
}
BR_HD int ar_count(uint8_t c) { return (c >> 4) & 3; }
BR_HD int ar_weight(uint8_t c) { return (c & 0x40) ? 1 : 2; }   // tokens that discharge one argument

// What the predicate needs of a row's state at one step -- derived once, not per column.
struct ArgumentRow {
    int d, p, loose, top, room, ended;   // top: the innermost group's kind, -1 at depth 0
};

BR_HD ArgumentRow ar_row(const ArgumentState& s, int rem) {
    ArgumentRow r;
    r.d = s.depth;
    r.p = r.d < BR_MAX_DEPTH ? (int)((s.pending >> (2 * r.d)) & 3u) : 0;
    r.loose = r.d < BR_MAX_DEPTH ? (int)((s.loose >> r.d) & 1u) : 0;
    r.top = r.d > 0 ? (int)((s.stack >> (2 * (r.d - 1))) & 3u) : -1;
    r.room = rem - (s.owed + s.depth + 1);
    r.ended = s.ended;
    return r;
}

// the rule that forbids the column of byte `c` (0: allowed)
BR_HD int ar_rule(const ArgumentRow& r, bool is_end, uint8_t c) {
    if (r.ended) return BR_OK;
    if (is_end) return r.p > 0 ? AR_ARG_EXPECTED : r.d == 0 ? BR_OK : BR_END_INSIDE;
    if (!ar_valid(c)) return BR_NEVER_EMITTED;
    const int k = c & 15, n = ar_count(c);
    if (r.p > 0) {
        if (n == 0 && k == 1) return r.loose && r.room < 0 ? AR_ARG_BUDGET : BR_OK;
        return n == 0 && k == 0 && r.loose ? BR_OK : AR_ARG_EXPECTED;
    }
    const int cost = n * ar_weight(c);
    if (k == 0) {
        if (n == 0) return r.room >= 0 ? BR_OK : BR_NEUTRAL_BUDGET;
        return r.d >= BR_MAX_DEPTH ? AR_ARG_DEPTH : cost <= r.room ? BR_OK : AR_ARG_BUDGET;
    }
    if (k <= BR_KINDS) {
        if (r.d >= BR_MAX_DEPTH) return BR_OPEN_DEPTH;
        if (n == 0) return r.room >= 1 ? BR_OK : BR_OPEN_BUDGET;
        return r.d + 1 >= BR_MAX_DEPTH ? AR_ARG_DEPTH : 1 + cost <= r.room ? BR_OK : AR_ARG_BUDGET;
    }
    return r.top == k - BR_KINDS - 1 ? BR_OK : BR_CLOSER;
}

BR_HD bool ar_allowed(const ArgumentRow& r, bool is_end, uint8_t c) { return ar_rule(r, is_end, c) == BR_OK; }

// After the pick: the argument it was (if one was owed), push or pop, then its own demand on the level it landed on --
// whose pending is 0 at that point.  A pick the rules would not have allowed (only the fallback's END) ends the row as is.
BR_HD void ar_advance(ArgumentState& s, bool is_end, uint8_t c) {
    if (s.ended) return;
    if (is_end) { s.ended = 1; return; }
    if (!ar_valid(c)) return;
    const int k = c & 15, n = ar_count(c);
    if (s.depth < BR_MAX_DEPTH && ((s.pending >> (2 * s.depth)) & 3u)) {
        s.pending -= (uint64_t)1 << (2 * s.depth);
        s.owed -= ((s.loose >> s.depth) & 1u) ? 1 : 2;
    }
    if (k >= 1 && k <= BR_KINDS && s.depth < BR_MAX_DEPTH) {
        s.stack |= (uint64_t)(k - 1) << (2 * s.depth);
        ++s.depth;
    } else if (k > BR_KINDS && s.depth > 0) {
        --s.depth;
        s.stack &= ~((uint64_t)3 << (2 * s.depth));
    }
    if (n > 0 && s.depth < BR_MAX_DEPTH) {
        s.pending = (s.pending & ~((uint64_t)3 << (2 * s.depth))) | (uint64_t)n << (2 * s.depth);
        s.loose = (s.loose & ~(1u << s.depth)) | (uint32_t)((c >> 6) & 1) << s.depth;
        s.owed += n * ar_weight(c);
    }
}

// The rule model (bracket_rules.inc.h); the fallback pick is constraint_fallback<ArgumentModel>.
struct ArgumentModel {
    using State = ArgumentState;
    using Row = ArgumentRow;
    BR_HD static Row row(const State& s, int rem) { return ar_row(s, rem); }
    BR_HD static bool allowed(const Row& r, bool is_end, uint8_t c) { return ar_allowed(r, is_end, c); }
    BR_HD static void advance(State& s, bool is_end, uint8_t c) { ar_advance(s, is_end, c); }
};
