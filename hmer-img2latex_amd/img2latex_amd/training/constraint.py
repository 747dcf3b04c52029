"""Well-formed LaTeX out of the decoder: the bracket constraint of the step-batched greedy and sampling decode and of
the N-best beam search.

``BracketTable`` holds one class byte per vocabulary column (csrc/bracket_rules.inc.h): 0 neutral, 1..4 opens a group of
kind 0..3, 5..8 closes one, 255 never emitted.  ``from_tokenizer`` classifies token strings -- ``{ }`` kind 0,
``\\left… \\right…`` kind 1, ``\\begin{…} \\end{…}`` kind 2 -- ``device`` uploads the bytes once per device, and
``allowed`` / ``advance`` / ``candidates`` / ``replay`` / ``well_formed`` restate the rules on the host, which is what the
tests hold the kernels and the stand-alone host programs to.

What a constrained decode guarantees: every row emits END within ``steps`` steps, at depth 0, and every group it opened
is closed, innermost first, by a closer of its own kind.  What it does not: arity (``\\frac`` still needs its two
groups), operands of ``^`` / ``_``, or that a ``\\begin{array}`` is closed by ``\\end{array}`` and not by another
environment's ``\\end`` -- the kinds are three, not one per environment -- or anything about meaning.

``ArgumentTable`` is the stronger rule set of the greedy and sampling decode (csrc/argument_rules.inc.h;
``well_formed="arguments"``): the same byte carries, beside the bracket class, how many arguments the column demands and
whether they are loose.  On top of the above it guarantees that every demanded argument is present -- a brace group where
strict (``\\frac { a } { b }``), a brace group or one plain token where loose (``x ^ 2``, ``\\sqrt [ 3 ] { x }``).  It does
not guarantee: no double scripts (``x ^ a ^ b``), that a loose single-token argument is a sensible one (``^ &``),
delimiter tokens after a bare ``\\left``, environment names matching, or meaning.  The N-best beam search has no argument
form."""
from __future__ import annotations

import weakref
from typing import Dict, List, Optional, Sequence

import numpy as np

from .. import _lib

NEUTRAL, NEVER = 0, 255
KINDS, MAX_DEPTH = 4, 32
KIND_BRACE, KIND_LEFT_RIGHT, KIND_ENVIRONMENT = 0, 1, 2
STATE_BYTES = 16
# the rule that forbids a column (bracket_rules.inc.h BracketRuleId); 0: allowed
RULE_OK, RULE_END_INSIDE, RULE_NEUTRAL_BUDGET, RULE_OPEN_BUDGET, RULE_OPEN_DEPTH, RULE_CLOSER, RULE_NEVER = range(7)
RULE_NAMES = ("allowed", "END at depth > 0", "neutral out of budget", "open out of budget", "open at depth 32",
              "wrong or absent closer", "never")


def open_class(kind: int) -> int:
    return 1 + int(kind)


def close_class(kind: int) -> int:
    return 1 + KINDS + int(kind)


class BracketState:
    """The 16 bytes of one row: uint64 stack (2 bits per open group, the outermost in the low bits), int32 depth, int32
    ended."""
    __slots__ = ("stack", "depth", "ended")

    def __init__(self, stack: int = 0, depth: int = 0, ended: int = 0):
        self.stack, self.depth, self.ended = int(stack), int(depth), int(ended)

    def top(self) -> int:
        return (self.stack >> (2 * (self.depth - 1))) & 3

    def to_bytes(self) -> bytes:
        return np.array([self.stack], dtype="<u8").tobytes() + np.array([self.depth, self.ended], dtype="<i4").tobytes()

    @classmethod
    def from_bytes(cls, b: bytes) -> "BracketState":
        return cls(int(np.frombuffer(b[:8], dtype="<u8")[0]), *np.frombuffer(b[8:16], dtype="<i4").tolist())

    def copy(self) -> "BracketState":
        return BracketState(self.stack, self.depth, self.ended)

    def __eq__(self, other):
        return (self.stack, self.depth, self.ended) == (other.stack, other.depth, other.ended)

    def __repr__(self):
        return f"BracketState(stack={self.stack:#x}, depth={self.depth}, ended={self.ended})"


def _starts_command(token: str, command: str) -> bool:
    """``token`` is ``command`` or ``command`` followed by a non-letter: ``\\left(`` and ``\\left`` are, ``\\leftarrow``
    is not."""
    return token.startswith(command) and (len(token) == len(command) or not token[len(command)].isalpha())


def classify_token(token: str) -> int:
    """The class byte of one token string (special tokens are the caller's)."""
    if token == "{":
        return open_class(KIND_BRACE)
    if token == "}":
        return close_class(KIND_BRACE)
    if _starts_command(token, "\\left"):
        return open_class(KIND_LEFT_RIGHT)
    if _starts_command(token, "\\right"):
        return close_class(KIND_LEFT_RIGHT)
    if token.startswith("\\begin{"):
        return open_class(KIND_ENVIRONMENT)
    if token.startswith("\\end{"):
        return close_class(KIND_ENVIRONMENT)
    return NEUTRAL


class ConstraintTable:
    """What the rule sets' tables share: the bytes on the device and the replay of the constrained greedy rule.  A table
    names ``kind`` (I2L_CONSTRAIN_*), ``state_class`` and ``STATE_BYTES`` (the state of one row), ``table_bytes`` (uint8,
    one per column: what the kernels read), the library's ``greedy_entry`` / ``sample_entry`` / ``pick_entry``, and restates
    its rule set as ``rules`` and ``advance`` -- which the host tests compare with the C++."""
    _unit = "byte"                                                    # what the END column's message calls a table entry

    @property
    def vocab(self) -> int:
        return int(self.table_bytes.size)

    def state_bytes(self, rows: int) -> int:
        """The size of the rows' state buffer of a constrained call (i2l_bracket_state_bytes / i2l_argument_state_bytes)."""
        return max(int(rows), 0) * self.STATE_BYTES

    def device(self, dev):
        """The table bytes on ``dev`` (uint8, V), uploaded once per device."""
        import torch
        dev = torch.device(dev)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._device:
            self._device[dev] = torch.from_numpy(self.table_bytes.copy()).to(dev)
        return self._device[dev]

    def _end(self, end_id: Optional[int]) -> int:
        end = self.end_id if end_id is None else int(end_id)
        if end is None or not 0 <= end < self.vocab:
            raise ValueError("img2latex_amd: the constraint needs an end_id inside the table")
        if self.table_bytes[end] != NEUTRAL:
            raise ValueError(f"img2latex_amd: the END column's {self._unit} must be 0: END is named by the call, not the table")
        return end

    def allowed(self, state, end_id: int, rem: int) -> np.ndarray:
        return (self.rules(state, end_id, rem) == RULE_OK).astype(np.uint8)

    def pick(self, logits: np.ndarray, mask: np.ndarray, end_id: int) -> int:
        """The first-index arg max of ``logits`` over the columns ``mask`` allows; without one above -inf the first
        allowed column, else ``end_id``."""
        x = np.asarray(logits, dtype=np.float32)
        x = np.where(mask.astype(bool) & ~np.isnan(x), x, -np.inf)   # the kernel's `a > best` is false for a NaN
        if (x > -np.inf).any():
            return int(np.argmax(x))
        on = np.flatnonzero(mask)
        return int(on[0]) if on.size else int(end_id)

    def replay(self, logits_per_step, end_id: Optional[int] = None, steps: Optional[int] = None, state=None,
               first_step: int = 0) -> List[dict]:
        """The constrained greedy rule (temperature 1, arg max of the logits) over one row's logits, step by step:
        ``logits_per_step`` is (n, V).  Returns per step ``{"id", "allowed" (V uint8), "state" (the table's state class,
        after the pick), "free" (the unconstrained arg max), "rule" (the rule that forbade ``free``, 0 when it was
        allowed)}``.  ``steps`` is the decode's length (default n); ``state`` / ``first_step`` continue an earlier replay."""
        x = np.asarray(logits_per_step, dtype=np.float32)
        end = self._end(end_id)
        steps = x.shape[0] + first_step if steps is None else int(steps)
        st = self.state_class() if state is None else state.copy()
        out = []
        for i in range(x.shape[0]):
            rem = steps - (first_step + i) - 1
            rules = self.rules(st, end, rem)
            mask = (rules == RULE_OK).astype(np.uint8)
            free = int(np.argmax(x[i]))
            pick = self.pick(x[i], mask, end)
            self.advance(st, pick, end)
            out.append({"id": pick, "allowed": mask, "state": st.copy(), "free": free, "rule": int(rules[free])})
        return out


class BracketTable(ConstraintTable):
    """``classes``: one value per vocabulary column, 0..8 or 255 (anything else is stored as 255)."""
    kind, state_class, STATE_BYTES, _unit = _lib.CONSTRAIN_BRACKETS, BracketState, STATE_BYTES, "class"
    greedy_entry, sample_entry, pick_entry = "greedy_decode_constrained", "sample_decode_constrained", "constrained_pick_logits"
    table_bytes = property(lambda self: self.classes)

    def __init__(self, classes: Sequence[int], end_id: Optional[int] = None, unclosable: Sequence[str] = ()):
        cls = np.asarray(classes, dtype=np.int64).reshape(-1)
        if cls.size == 0:
            raise ValueError("img2latex_amd: a BracketTable needs at least one column")
        self.classes = np.where((cls >= 0) & (cls <= 2 * KINDS), cls, NEVER).astype(np.uint8)
        if end_id is not None:
            if not 0 <= int(end_id) < self.classes.size:
                raise ValueError(f"img2latex_amd: end_id {end_id} outside the table's {self.classes.size} columns")
            if self.classes[int(end_id)] != NEUTRAL:
                raise ValueError("img2latex_amd: the END column's class must be 0: END is named by the call, not the table")
        self.end_id = None if end_id is None else int(end_id)
        self.unclosable = list(unclosable)
        self._device: Dict = {}

    @classmethod
    def from_tokenizer(cls, tokenizer) -> "BracketTable":
        """Classifies ``tokenizer.id_to_token`` (module docstring).  PAD, START and UNK -- and any id gap, which decodes as
        UNK -- are never emitted; END is neutral in the table.  An open whose kind has no closer in the vocabulary could
        never be closed: it becomes never and its string is listed in ``unclosable``."""
        special = tokenizer.special_tokens
        to_id = tokenizer.token_to_id
        end = int(to_id[special["END"]])
        V = max(int(i) for i in tokenizer.id_to_token) + 1
        classes = np.full(V, NEVER, dtype=np.int64)
        special_ids = {int(to_id[t]) for t in special.values()}
        for i, tok in tokenizer.id_to_token.items():
            i = int(i)
            if i >= 0 and i not in special_ids:
                classes[i] = classify_token(tok)
        classes[end] = NEUTRAL
        unclosable = []
        for kind in range(KINDS):
            if not (classes == close_class(kind)).any():
                for i in np.flatnonzero(classes == open_class(kind)).tolist():
                    unclosable.append(tokenizer.id_to_token[i])
                    classes[i] = NEVER
        return cls(classes, end, unclosable)

    # ------------------------------------------------------------------ the host restatement of bracket_rules.inc.h
    def rules(self, state: BracketState, end_id: int, rem: int) -> np.ndarray:
        """(V) uint8: per column the rule that forbids it at ``rem`` emissions left after this one, 0 = allowed."""
        V, c, d = self.vocab, self.classes, state.depth
        out = np.zeros(V, dtype=np.uint8)
        if state.ended:
            return out
        is_open = (c >= 1) & (c <= KINDS)
        is_close = (c > KINDS) & (c <= 2 * KINDS)
        out[c == NEVER] = RULE_NEVER
        if d + 1 > rem:
            out[c == NEUTRAL] = RULE_NEUTRAL_BUDGET
        if d >= MAX_DEPTH:
            out[is_open] = RULE_OPEN_DEPTH
        elif d + 2 > rem:
            out[is_open] = RULE_OPEN_BUDGET
        if d > 0:
            out[is_close & (c != close_class(state.top()))] = RULE_CLOSER
        else:
            out[is_close] = RULE_CLOSER
        out[end_id] = RULE_OK if d == 0 else RULE_END_INSIDE
        return out

    def advance(self, state: BracketState, pick: int, end_id: int) -> None:
        if state.ended:
            return
        if pick == end_id:
            state.ended = 1
            return
        k = int(self.classes[pick])
        if 1 <= k <= KINDS and state.depth < MAX_DEPTH:
            state.stack |= (k - 1) << (2 * state.depth)
            state.depth += 1
        elif KINDS < k <= 2 * KINDS and state.depth > 0:
            state.depth -= 1
            state.stack &= ~(3 << (2 * state.depth))

    def candidates(self, state: BracketState, row, end_id: int, rem: int, beam: int, logits: bool = False):
        """The slot policy of the well-formed beam search (csrc/beam_bracket_rules.inc.h): the candidates of a live slot
        in ``state`` at ``rem`` emissions left after this one, as ``[(column, log-prob)]`` -- its top ``min(beam,
        #allowed)`` allowed columns of ``row``, descending, the lower index first on ties; the list stops at the first
        column without a value above -inf, and an empty list becomes ``[(end_id, 0.0)]`` (defined, not well formed).
        ``logits=True``: ``row`` holds logits and the log-probs are its log-softmax over the allowed columns only, in the
        row's dtype (the device's phase (c)); otherwise ``row`` holds log-probs that are taken as they are."""
        x = np.asarray(row)
        x = x if x.dtype in (np.float32, np.float64) else x.astype(np.float64)
        mask = self.allowed(state, end_id, rem).astype(bool)
        sel = np.where(mask & ~np.isnan(x), x, -np.inf)                # the kernel's `x > best` is false for a NaN
        lp = sel
        if logits:
            masked = np.where(mask, x, -np.inf).astype(x.dtype)
            m = masked.max() if mask.any() else -np.inf
            with np.errstate(invalid="ignore"):
                lp = (masked - m) - np.log(np.exp(masked - m).sum(dtype=x.dtype))
        order = np.argsort(-sel, kind="stable")[:int(beam)]
        out = [(int(v), float(lp[v])) for v in order if sel[v] > -np.inf]
        return out if out else [(int(end_id), 0.0)]

    def well_formed(self, ids: Sequence[int], end_id: Optional[int] = None) -> bool:
        """``ids`` (START not included) reach END -- ids behind it, and the sticky stop's -1 filler, are not looked at --
        with every group closed by a closer of its own kind, innermost first, none deeper than 32, no never column."""
        end = self._end(end_id)
        stack: List[int] = []
        for i in ids:
            i = int(i)
            if i == end:
                return not stack
            if not 0 <= i < self.vocab:
                return False
            k = int(self.classes[i])
            if k == NEVER:
                return False
            if 1 <= k <= KINDS:
                if len(stack) >= MAX_DEPTH:
                    return False
                stack.append(k - 1)
            elif k > KINDS:
                if not stack or stack.pop() != k - KINDS - 1:
                    return False
        return False


# ---------------------------------------------------------------------------------------------------------------------
# The argument rules (csrc/argument_rules.inc.h): the bracket rules plus arity
# ---------------------------------------------------------------------------------------------------------------------
ARGUMENT_STATE_BYTES = 32
RULE_ARG_EXPECTED, RULE_ARG_BUDGET, RULE_ARG_DEPTH = 7, 8, 9
ARGUMENT_RULE_NAMES = RULE_NAMES + ("argument expected", "argument out of budget", "argument at level 32")
LOOSE_BIT = 0x40

_FONTS_AND_ACCENTS = ("\\mathrm", "\\mathbf", "\\mathcal", "\\mathbb", "\\text", "\\operatorname", "\\hat", "\\bar", "\\vec",
                      "\\tilde", "\\overline", "\\underline", "\\widehat", "\\widetilde", "\\dot", "\\ddot", "\\overbrace",
                      "\\underbrace")
# token string -> (count, loose).  \sqrt is loose so that ``\sqrt [ 3 ] { x }`` stays reachable ([ is a plain token).
DEFAULT_ARGUMENTS: Dict[str, tuple] = {
    "^": (1, True), "_": (1, True), "\\sqrt": (1, True),
    **{t: (2, False) for t in ("\\frac", "\\dfrac", "\\tfrac", "\\cfrac", "\\binom", "\\stackrel", "\\overset",
                               "\\underset")},
    "\\begin{array}": (1, False), "\\begin{tabular}": (1, False),
    **{t: (1, True) for t in _FONTS_AND_ACCENTS},
}


def argument_byte(cls: int, count: int = 0, loose: bool = False) -> int:
    """The table byte of a column: bracket class in bits 0..3, argument count in bits 4..5, loose in bit 6."""
    return int(cls) | int(count) << 4 | (LOOSE_BIT if loose else 0)


def _valid_bytes(b: np.ndarray) -> np.ndarray:
    lo, n, loose = b & 15, (b >> 4) & 3, (b & LOOSE_BIT) != 0
    return ((b & 0x80) == 0) & (lo <= 2 * KINDS) & (~loose | (n > 0)) & ((lo <= KINDS) | (n == 0))


class ArgumentState:
    """The 32 bytes of one row: uint64 stack, uint64 pending (2 bits per level: arguments owed there), uint32 loose (1 bit
    per level), int32 depth, int32 owed (sum of pending * (1 if loose else 2)), int32 ended."""
    __slots__ = ("stack", "pending", "loose", "depth", "owed", "ended")

    def __init__(self, stack: int = 0, pending: int = 0, loose: int = 0, depth: int = 0, owed: int = 0, ended: int = 0):
        self.stack, self.pending, self.loose = int(stack), int(pending), int(loose)
        self.depth, self.owed, self.ended = int(depth), int(owed), int(ended)

    def top(self) -> int:
        return (self.stack >> (2 * (self.depth - 1))) & 3

    def pending_here(self) -> int:
        return (self.pending >> (2 * self.depth)) & 3 if self.depth < MAX_DEPTH else 0

    def loose_here(self) -> bool:
        return bool((self.loose >> self.depth) & 1) if self.depth < MAX_DEPTH else False

    def _fields(self):
        return (self.stack, self.pending, self.loose, self.depth, self.owed, self.ended)

    def to_bytes(self) -> bytes:
        return (np.array([self.stack, self.pending], dtype="<u8").tobytes() + np.array([self.loose], dtype="<u4").tobytes()
                + np.array([self.depth, self.owed, self.ended], dtype="<i4").tobytes())

    @classmethod
    def from_bytes(cls, b: bytes) -> "ArgumentState":
        b = bytes(b)
        stack, pending = np.frombuffer(b[:16], dtype="<u8").tolist()
        return cls(stack, pending, int(np.frombuffer(b[16:20], dtype="<u4")[0]), *np.frombuffer(b[20:32], dtype="<i4").tolist())

    def copy(self) -> "ArgumentState":
        return ArgumentState(*self._fields())

    def __eq__(self, other):
        return self._fields() == other._fields()

    def __repr__(self):
        return (f"ArgumentState(stack={self.stack:#x}, pending={self.pending:#x}, loose={self.loose:#x}, "
                f"depth={self.depth}, owed={self.owed}, ended={self.ended})")


class ArgumentTable(ConstraintTable):
    """``table``: one byte per vocabulary column -- bits 0..3 the bracket class (0..8), bits 4..5 the number of arguments
    the column demands, bit 6 loose (each argument a brace group or one plain token; without it a brace group).  A byte
    that is not valid (csrc/argument_rules.inc.h) is stored as 255, never emitted.  The table must be able to discharge
    what it demands: ``{`` and ``}`` for a strict demand, a plain token for a loose one -- ``from_tokenizer`` and
    ``from_brackets`` see to it, the constructor refuses a table that cannot.  (An open kind without a closer is the
    caller's to avoid, as with a BracketTable.)

    What an argument-constrained decode guarantees: nesting and END as the bracket constraint, and every demanded argument
    present -- a brace group where strict, a group or one plain token where loose.  What it does not: double scripts
    (``x ^ a ^ b``), that a loose single-token argument is a sensible one (``^ &``), delimiter tokens after a bare
    ``\\left``, environment names matching, or anything about meaning."""

    kind, state_class, STATE_BYTES = _lib.CONSTRAIN_ARGUMENTS, ArgumentState, ARGUMENT_STATE_BYTES
    greedy_entry, sample_entry, pick_entry = "greedy_decode_arguments", "sample_decode_arguments", "arguments_pick_logits"
    table_bytes = property(lambda self: self.table)

    def __init__(self, table: Sequence[int], end_id: Optional[int] = None, unclosable: Sequence[str] = (),
                 unsatisfiable: Sequence[str] = ()):
        b = np.asarray(table, dtype=np.int64).reshape(-1)
        if b.size == 0:
            raise ValueError("img2latex_amd: an ArgumentTable needs at least one column")
        b = np.where((b >= 0) & (b <= 255), b, NEVER)
        self.table = np.where(_valid_bytes(b), b, NEVER).astype(np.uint8)
        if end_id is not None:
            if not 0 <= int(end_id) < self.table.size:
                raise ValueError(f"img2latex_amd: end_id {end_id} outside the table's {self.table.size} columns")
            if self.table[int(end_id)] != NEUTRAL:
                raise ValueError("img2latex_amd: the END column's byte must be 0: END is named by the call, not the table")
        self.end_id = None if end_id is None else int(end_id)
        self.unclosable, self.unsatisfiable = list(unclosable), list(unsatisfiable)
        self._device: Dict = {}
        valid = self.table != NEVER
        self.classes = np.where(valid, self.table & 15, NEVER).astype(np.uint8)          # the bracket class per column
        self.counts = np.where(valid, (self.table >> 4) & 3, 0).astype(np.int64)
        self.loose = valid & ((self.table & LOOSE_BIT) != 0)
        self.weights = np.where(self.loose, 1, 2).astype(np.int64) * self.counts          # tokens the demand costs
        self.openers = valid & (self.table == open_class(KIND_BRACE))                     # argument openers
        self.plain = valid & (self.table == NEUTRAL)
        if end_id is not None:
            self.plain[int(end_id)] = False
        missing = self.missing()
        if missing:
            raise ValueError("img2latex_amd: the table cannot discharge what it demands: " + "; ".join(missing))

    def missing(self) -> List[str]:
        """What the liveness of the rules needs and the table lacks (empty: nothing)."""
        out = []
        strict = (self.counts > 0) & ~self.loose
        if strict.any() and not (self.openers.any() and (self.classes == close_class(KIND_BRACE)).any()):
            out.append("a strict argument needs { and } columns")
        if ((self.counts > 0) & self.loose).any() and not self.plain.any():
            out.append("a loose argument needs a plain token")
        return out

    @classmethod
    def from_brackets(cls, bracket_table: BracketTable, arguments_by_column: Dict[int, tuple],
                      names: Optional[Dict[int, str]] = None) -> "ArgumentTable":
        """``bracket_table``'s classes with ``arguments_by_column[column] = (count, loose)`` on top.  A demand that could
        not be met -- a strict one without ``{`` and ``}`` in the table, a loose one without a plain token, any on a
        closer or a never column -- is stored as count 0 and listed in ``unsatisfiable`` (by ``names[column]``, else the
        column number as a string)."""
        c = bracket_table.classes.astype(np.int64)
        end = bracket_table.end_id
        demands = {int(k): (int(v[0]), bool(v[1])) for k, v in arguments_by_column.items() if int(v[0]) > 0}
        for k, (n, _) in demands.items():
            if not 0 <= k < c.size or not 0 < n <= 3:
                raise ValueError(f"img2latex_amd: column {k} demanding {n} arguments: outside the table or the 0..3 range")
        braces = bool((c == open_class(KIND_BRACE)).any() and (c == close_class(KIND_BRACE)).any())
        plain = (c == NEUTRAL)
        if end is not None:
            plain[end] = False
        for k in demands:
            plain[k] = False
        has_plain = bool(plain.any())
        table, unsatisfiable = c.copy(), []
        for k, (n, loose) in sorted(demands.items()):
            ok = c[k] <= KINDS and k != end and (has_plain if loose else braces)
            if ok:
                table[k] = argument_byte(c[k], n, loose)
            else:
                unsatisfiable.append(names[k] if names and k in names else str(k))
        return cls(table, end, bracket_table.unclosable, unsatisfiable)

    @classmethod
    def from_tokenizer(cls, tokenizer, arguments: Optional[Dict[str, tuple]] = None) -> "ArgumentTable":
        """``BracketTable.from_tokenizer``'s classes, and the demand ``arguments[token] = (count, loose)`` on every token
        of the vocabulary that the mapping names (default ``DEFAULT_ARGUMENTS``; a caller's mapping replaces it)."""
        arguments = DEFAULT_ARGUMENTS if arguments is None else arguments
        brackets = BracketTable.from_tokenizer(tokenizer)
        special = {int(tokenizer.token_to_id[t]) for t in tokenizer.special_tokens.values()}
        names = {int(i): tok for i, tok in tokenizer.id_to_token.items()}
        by_column = {i: arguments[tok] for i, tok in names.items() if i >= 0 and i not in special and tok in arguments}
        return cls.from_brackets(brackets, by_column, names)

    # ------------------------------------------------------------------ the host restatement of argument_rules.inc.h
    def rules(self, state: ArgumentState, end_id: int, rem: int) -> np.ndarray:
        """(V) uint8: per column the rule that forbids it at ``rem`` emissions left after this one, 0 = allowed."""
        V, c, n, d = self.vocab, self.classes, self.counts, state.depth
        out = np.zeros(V, dtype=np.uint8)
        if state.ended:
            return out
        room = rem - (state.owed + d + 1)
        plain = self.plain.copy()
        plain[end_id] = False
        never = c == NEVER
        if state.pending_here() > 0:
            out[:] = RULE_ARG_EXPECTED
            out[self.openers] = RULE_ARG_BUDGET if state.loose_here() and room < 0 else RULE_OK
            if state.loose_here():
                out[plain] = RULE_OK
            out[never] = RULE_NEVER
            out[end_id] = RULE_ARG_EXPECTED
            return out
        is_open = (c >= 1) & (c <= KINDS)
        is_close = (c > KINDS) & (c <= 2 * KINDS)
        neutral = c == NEUTRAL
        demanding = n > 0
        out[neutral & ~demanding] = RULE_OK if room >= 0 else RULE_NEUTRAL_BUDGET
        out[neutral & demanding] = RULE_ARG_DEPTH if d >= MAX_DEPTH else RULE_OK
        out[neutral & demanding & (out == RULE_OK) & (self.weights > room)] = RULE_ARG_BUDGET
        if d >= MAX_DEPTH:
            out[is_open] = RULE_OPEN_DEPTH
        else:
            out[is_open & ~demanding] = RULE_OK if room >= 1 else RULE_OPEN_BUDGET
            if d + 1 >= MAX_DEPTH:
                out[is_open & demanding] = RULE_ARG_DEPTH
            else:
                out[is_open & demanding & (1 + self.weights > room)] = RULE_ARG_BUDGET
        if d > 0:
            out[is_close & (c != close_class(state.top()))] = RULE_CLOSER
        else:
            out[is_close] = RULE_CLOSER
        out[never] = RULE_NEVER
        out[end_id] = RULE_OK if d == 0 else RULE_END_INSIDE
        return out

    def advance(self, state: ArgumentState, pick: int, end_id: int) -> None:
        if state.ended:
            return
        if pick == end_id:
            state.ended = 1
            return
        if self.table[pick] == NEVER:
            return
        k, n = int(self.classes[pick]), int(self.counts[pick])
        if state.pending_here() > 0:
            state.owed -= 1 if state.loose_here() else 2
            state.pending -= 1 << (2 * state.depth)
        if 1 <= k <= KINDS and state.depth < MAX_DEPTH:
            state.stack |= (k - 1) << (2 * state.depth)
            state.depth += 1
        elif k > KINDS and state.depth > 0:
            state.depth -= 1
            state.stack &= ~(3 << (2 * state.depth))
        if n > 0 and state.depth < MAX_DEPTH:
            d = state.depth
            state.pending = (state.pending & ~(3 << (2 * d))) | n << (2 * d)
            state.loose = (state.loose & ~(1 << d)) | int(self.loose[pick]) << d
            state.owed += int(self.weights[pick])

    def enumerate(self, steps: int, end_id: Optional[int] = None) -> List[tuple]:
        """Every sequence (END last) the rules allow within ``steps``, in lexicographic order of the ids -- what the host
        program's ``--enumerate`` writes.  For small tables only."""
        end = self._end(end_id)
        out: List[tuple] = []

        def go(st, t, ids):
            if t == steps:
                return
            for v in np.flatnonzero(self.allowed(st, end, steps - t - 1)).tolist():
                if v == end:
                    out.append(tuple(ids + [v]))
                else:
                    nxt = st.copy()
                    self.advance(nxt, v, end)
                    go(nxt, t + 1, ids + [v])
        go(ArgumentState(), 0, [])
        return out

    def complete(self, ids: Sequence[int], end_id: Optional[int] = None) -> bool:
        """``ids`` (START not included) reach END -- what follows it is not looked at -- with every group closed by a
        closer of its own kind, innermost first, none deeper than 32, no never column, and every demanded argument
        present: a brace group where strict, a brace group or one plain token where loose.  Written as a walk over the
        groups, not as the state machine above."""
        end = self._end(end_id)
        stack: List[int] = []                 # the open groups' kinds
        owed: List[List] = [[0, False]]       # per level: [arguments still owed, loose]
        for i in ids:
            i = int(i)
            if i == end:
                return not stack and owed[0][0] == 0
            if not 0 <= i < self.vocab or self.table[i] == NEVER:
                return False
            k, n = int(self.classes[i]), int(self.counts[i])
            here = owed[-1]
            if here[0] > 0:
                if not (self.openers[i] or (here[1] and self.plain[i])):
                    return False
                here[0] -= 1
            elif k > KINDS:
                if not stack or stack.pop() != k - KINDS - 1:
                    return False
                owed.pop()
            if 1 <= k <= KINDS:
                if len(stack) >= MAX_DEPTH:
                    return False
                stack.append(k - 1)
                owed.append([0, False])
            if n > 0:
                if len(stack) >= MAX_DEPTH:
                    return False
                owed[-1] = [n, bool(self.loose[i])]
        return False

    def well_formed(self, ids: Sequence[int], end_id: Optional[int] = None) -> bool:
        """The bracket property alone (``BracketTable.well_formed`` on this table's classes)."""
        return BracketTable(self.classes, self.end_id).well_formed(ids, end_id)


_TABLES: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
_ARGUMENT_TABLES: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _cached(cache, tokenizer, build):
    try:
        table = cache.get(tokenizer)
        if table is None:
            table = cache[tokenizer] = build(tokenizer)
    except TypeError:                                                # not hashable / not weakly referenceable: no cache
        table = build(tokenizer)
    return table


def as_table(constraint, tokenizer=None):
    """None / False -> None; True -> the tokenizer's BracketTable, "arguments" -> its ArgumentTable (each built once; the
    cache dies with the tokenizer, and a tokenizer refitted afterwards needs ``from_tokenizer`` anew); a BracketTable or
    an ArgumentTable -> itself."""
    if constraint is None or constraint is False:
        return None
    if isinstance(constraint, ConstraintTable):
        return constraint
    if constraint is True and tokenizer is not None:
        return _cached(_TABLES, tokenizer, BracketTable.from_tokenizer)
    if isinstance(constraint, str) and constraint == "arguments" and tokenizer is not None:
        return _cached(_ARGUMENT_TABLES, tokenizer, ArgumentTable.from_tokenizer)
    raise TypeError('img2latex_amd: constraint must be a BracketTable, an ArgumentTable, True or "arguments"')
