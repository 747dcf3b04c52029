// The nesting rules of the bracket-constrained decode, stated once: which vocabulary columns a row may emit at a step,
// what the pick does to the row's state, and what is picked when a malformed table leaves nothing.  Shared by the
// constrained selection kernels (decode_constrained.inc.h) and a stand-alone host program (bracket_rules_host_main.cpp)
// that a host test compares with the Python restatement (training/constraint.py) step by step.
//
// Plain C++, no HIP: BR_HD is `__host__ __device__` under hipcc and empty elsewhere.  Every function is called by ONE
// thread (br_rule / br_allowed by any number of threads on their own copy of the state).
//
// Class table: one byte per column -- 0 neutral, 1..4 opens a group of kind 0..3, 5..8 closes one, anything else is
// never emitted.  END is named by the call (end_id), not by the table; its entry is ignored.
//
// With rem = steps - t - 1 emissions left after this one and d = depth, a row that has not ended may emit
//   END          iff d == 0
//   neutral      iff d + 1 <= rem          (d closers and END still fit behind it)
//   open kind g  iff d < 32 and d + 2 <= rem
//   close kind g iff d > 0 and the innermost open group is of kind g
// d + 1 <= steps - t holds at t = 0 for steps >= 1 and every allowed pick keeps it, so the closer of the innermost
// kind (d > 0) or END (d == 0) is always allowed: every row emits END at depth 0 within `steps` steps.  A row that has
// ended is not constrained any more.  A table without the closer of an open kind can leave NO column allowed; the pick
// is then end_id (constraint_fallback) -- defined, though such a row is not well formed.  BracketTable (constraint.py)
// never builds such a table: an open without a closer becomes "never".
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BR_HD __host__ __device__ inline
#else
#define BR_HD inline
#endif

constexpr int BR_KINDS = 4;
constexpr int BR_MAX_DEPTH = 32;
constexpr int BR_NEVER = 255;

struct BracketState {    // 16 bytes per row; all-zero bytes are the initial state
    uint64_t stack;      // 2 bits per open group, the outermost group in the low bits
    int32_t depth;       // 0 .. 32
    int32_t ended;
};
static_assert(sizeof(BracketState) == 16, "16 bytes of state per row");

// the rule that forbids a column (0: allowed); the restatement reports which one overrode the unconstrained arg max
enum BracketRuleId {
    BR_OK = 0,
    BR_END_INSIDE = 1,       // END at depth > 0
    BR_NEUTRAL_BUDGET = 2,   // neutral, but the closers and END would not fit behind it
    BR_OPEN_BUDGET = 3,      // open, but its closer would not fit
    BR_OPEN_DEPTH = 4,       // open at depth 32
    BR_CLOSER = 5,           // closer of another kind than the innermost group's, or no group open
    BR_NEVER_EMITTED = 6,
};

BR_HD int br_class(uint8_t c) { return c <= 2 * BR_KINDS ? (int)c : BR_NEVER; }

BR_HD int br_top(const BracketState& s) { return (int)((s.stack >> (2 * (s.depth - 1))) & 3u); }   // depth > 0

// column `v` of class byte `c` at `rem` emissions left after this one
BR_HD int br_rule(const BracketState& s, bool is_end, uint8_t c, int rem) {
    if (s.ended) return BR_OK;
    const int d = s.depth;
    if (is_end) return d == 0 ? BR_OK : BR_END_INSIDE;
    const int k = br_class(c);
    if (k == 0) return d + 1 <= rem ? BR_OK : BR_NEUTRAL_BUDGET;
    if (k <= BR_KINDS) return d >= BR_MAX_DEPTH ? BR_OPEN_DEPTH : d + 2 <= rem ? BR_OK : BR_OPEN_BUDGET;
    if (k <= 2 * BR_KINDS) return d > 0 && br_top(s) == k - BR_KINDS - 1 ? BR_OK : BR_CLOSER;
    return BR_NEVER_EMITTED;
}

BR_HD bool br_allowed(const BracketState& s, bool is_end, uint8_t c, int rem) { return br_rule(s, is_end, c, rem) == BR_OK; }

// after the pick: push, pop or end.  A pick the rules would not have allowed (only the fallback's END) ends the row as is.
BR_HD void br_advance(BracketState& s, bool is_end, uint8_t c) {
    if (s.ended) return;
    if (is_end) { s.ended = 1; return; }
    const int k = br_class(c);
    if (k >= 1 && k <= BR_KINDS && s.depth < BR_MAX_DEPTH) {
        s.stack |= (uint64_t)(k - 1) << (2 * s.depth);
        ++s.depth;
    } else if (k > BR_KINDS && k <= 2 * BR_KINDS && s.depth > 0) {
        --s.depth;
        s.stack &= ~((uint64_t)3 << (2 * s.depth));
    }
}

// The rules as a RULE MODEL: the five names under which the selection kernels' pick policy (decode_constrained.inc.h),
// constraint_fallback and the host programs' walk (rules_walk_host.inc.h) take a rule set -- the per-row State, the
// per-step Row derived from it once, row(state, rem), allowed(row, is_end, c), advance(state&, is_end, c).
struct BracketModel {
    using State = BracketState;
    struct Row { BracketState st; int rem; };
    BR_HD static Row row(const State& s, int rem) { return {s, rem}; }
    BR_HD static bool allowed(const Row& r, bool is_end, uint8_t c) { return br_allowed(r.st, is_end, c, r.rem); }
    BR_HD static void advance(State& s, bool is_end, uint8_t c) { br_advance(s, is_end, c); }
};

// The pick when the selection found none among the allowed columns (no column allowed, or every allowed logit -inf /
// NaN), under any model: the first allowed column, else end_id.
template <class Model>
BR_HD int constraint_fallback(const typename Model::Row& r, const uint8_t* cls, int V, int end_id) {
    for (int v = 0; v < V; ++v)
        if (Model::allowed(r, v == end_id, cls[v])) return v;
    return end_id;
}
