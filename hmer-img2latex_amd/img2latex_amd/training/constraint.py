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
environment's ``\\end`` -- the kinds are three, not one per environment -- or anything about meaning."""
from __future__ import annotations

import weakref
from typing import Dict, List, Optional, Sequence

import numpy as np

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


class BracketTable:
    """``classes``: one value per vocabulary column, 0..8 or 255 (anything else is stored as 255)."""

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

    @property
    def vocab(self) -> int:
        return int(self.classes.size)

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

    def device(self, dev):
        """The class bytes on ``dev`` (uint8, V), uploaded once per device."""
        import torch
        dev = torch.device(dev)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._device:
            self._device[dev] = torch.from_numpy(self.classes.copy()).to(dev)
        return self._device[dev]

    def _end(self, end_id: Optional[int]) -> int:
        end = self.end_id if end_id is None else int(end_id)
        if end is None or not 0 <= end < self.vocab:
            raise ValueError("img2latex_amd: the constraint needs an end_id inside the table")
        if self.classes[end] != NEUTRAL:
            raise ValueError("img2latex_amd: the END column's class must be 0: END is named by the call, not the table")
        return end

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

    def allowed(self, state: BracketState, end_id: int, rem: int) -> np.ndarray:
        return (self.rules(state, end_id, rem) == RULE_OK).astype(np.uint8)

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

    def pick(self, logits: np.ndarray, mask: np.ndarray, end_id: int) -> int:
        """The first-index arg max of ``logits`` over the columns ``mask`` allows; without one above -inf the first
        allowed column, else ``end_id``."""
        x = np.asarray(logits, dtype=np.float32)
        x = np.where(mask.astype(bool) & ~np.isnan(x), x, -np.inf)   # the kernel's `a > best` is false for a NaN
        if (x > -np.inf).any():
            return int(np.argmax(x))
        on = np.flatnonzero(mask)
        return int(on[0]) if on.size else int(end_id)

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

    def replay(self, logits_per_step, end_id: Optional[int] = None, steps: Optional[int] = None,
               state: Optional[BracketState] = None, first_step: int = 0) -> List[dict]:
        """The constrained greedy rule (temperature 1, arg max of the logits) over one row's logits, step by step:
        ``logits_per_step`` is (n, V).  Returns per step ``{"id", "allowed" (V uint8), "state" (BracketState after the
        pick), "free" (the unconstrained arg max), "rule" (the rule that forbade ``free``, 0 when it was allowed)}``.
        ``steps`` is the decode's length (default n); ``state`` / ``first_step`` continue an earlier replay."""
        x = np.asarray(logits_per_step, dtype=np.float32)
        end = self._end(end_id)
        steps = x.shape[0] + first_step if steps is None else int(steps)
        st = BracketState() if state is None else state.copy()
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


_TABLES: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def as_table(constraint, tokenizer=None) -> Optional[BracketTable]:
    """None / False -> None; True -> the tokenizer's table (built once; the cache dies with the tokenizer, and a
    tokenizer refitted afterwards needs ``BracketTable.from_tokenizer`` anew); a BracketTable -> itself."""
    if constraint is None or constraint is False:
        return None
    if isinstance(constraint, BracketTable):
        return constraint
    if constraint is True and tokenizer is not None:
        try:
            table = _TABLES.get(tokenizer)
            if table is None:
                table = _TABLES[tokenizer] = BracketTable.from_tokenizer(tokenizer)
        except TypeError:                                            # not hashable / not weakly referenceable: no cache
            table = BracketTable.from_tokenizer(tokenizer)
        return table
    raise TypeError("img2latex_amd: constraint must be a BracketTable")
