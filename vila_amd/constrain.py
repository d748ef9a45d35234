"""Structured output: compile a choice list, a regular expression or a JSON schema into a token-level automaton for the constrained decode steps
(`vila_llm_decode_step[_batch]_constrained`, csrc/constrain.hip).  Pure Python + numpy; nothing here touches the GPU.

    front-end (`choice`, `regex`, `json_schema`)  ->  regex AST  ->  byte NFA  ->  byte DFA (subset construction, Moore minimisation)
    ->  lifted over a vocabulary (`compile_automaton`): dst[state][token], EOS -> DONE from accepting states, trimmed at TOKEN level
    ->  `Automaton`(cls uint16 [V], next int16 [S][C], start, n_classes): token classes are the distinct columns of dst.

The regex subset: literals, escapes (\\d \\w \\s \\D \\W \\S \\t \\n \\r \\f \\v \\xHH and escaped metacharacters), `.`, classes with ranges and negation,
groups `(...)` and `(?:...)`, `|`, `* + ? {m} {m,} {m,n}` (lazy forms are accepted as their greedy language).  Semantics are FULL match with ASCII
classes (`re.fullmatch(p, s, re.ASCII)`); `.` (anything but a newline) and negated classes admit every well-formed UTF-8 sequence outside their set.
The automaton runs on BYTES, so a token may end inside a character.  Anchors, backreferences and lookaround raise ValueError naming the construct.

`json_schema(schema, indent=None)` serves: object with properties (every declared property is emitted, in declaration order; nested objects), array with
items / minItems / maxItems, string (enum, minLength / maxLength, pattern), integer, number, boolean, null, enum / const of scalars, anyOf, and a list
of types.  indent=None gives the layout of `json.dumps(obj)`, indent=k that of `json.dumps(obj, indent=k)`.  `$ref` / recursion, additionalProperties and
free-form JSON (`{"type": "json_object"}`) need a stack and are not served: each raises ValueError saying so.

`max_new_tokens` can cut a reply before the automaton accepts: the text is then a prefix of a member of the language, not a member."""
from __future__ import annotations

import json
from collections import OrderedDict
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

MAX_STATES = 32767            # next[] is int16
MAX_CLASSES = 4096            # = VILA_CONSTRAIN_MAX_CLASSES: one state's table row sits in LDS
MAX_LIFT = 1 << 28            # byte states x vocabulary entries the lift may hold (int16: 512 MB, plus a byte per entry while it trims)

# ------------------------------------------------------------------------------------------------------------------------------------------------------
# regex AST: ("set", frozenset of byte values) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None) ; the empty string is ("cat", [])
# ------------------------------------------------------------------------------------------------------------------------------------------------------
EPS = ("cat", [])
_DIGIT = frozenset(range(0x30, 0x3A))
_WORD = frozenset(list(range(0x30, 0x3A)) + list(range(0x41, 0x5B)) + list(range(0x61, 0x7B)) + [0x5F])
_SPACE = frozenset(b" \t\n\r\f\v")
_ASCII = frozenset(range(0x80))
_META = set("\\.[]()|*+?{}^$")


def _bset(lo: int, hi: int):
    return ("set", frozenset(range(lo, hi + 1)))


def _lit(data: bytes):
    return ("cat", [("set", frozenset([b])) for b in data])


def _not_ascii(excluded) -> tuple:
    """Every well-formed UTF-8 sequence (RFC 3629: no overlongs, no surrogates, up to U+10FFFF) except the ASCII bytes in `excluded`."""
    c = _bset(0x80, 0xBF)
    alts = [("set", _ASCII - frozenset(excluded)),
            ("cat", [_bset(0xC2, 0xDF), c]),
            ("cat", [_bset(0xE0, 0xE0), _bset(0xA0, 0xBF), c]), ("cat", [_bset(0xE1, 0xEC), c, c]),
            ("cat", [_bset(0xED, 0xED), _bset(0x80, 0x9F), c]), ("cat", [_bset(0xEE, 0xEF), c, c]),
            ("cat", [_bset(0xF0, 0xF0), _bset(0x90, 0xBF), c, c]), ("cat", [_bset(0xF1, 0xF3), c, c, c]),
            ("cat", [_bset(0xF4, 0xF4), _bset(0x80, 0x8F), c, c])]
    return ("alt", [a for a in alts if a[0] != "set" or a[1]])


class _Parser:
    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError("regex: the pattern must be a str")
        self.p, self.i = pattern, 0

    def fail(self, what: str):
        raise ValueError(f"regex: {what} (at offset {self.i} of {self.p!r})")

    def peek(self) -> str:
        return self.p[self.i] if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced `)`")
        return node

    def alt(self):
        alts = [self.seq()]
        while self.peek() == "|":
            self.i += 1
            alts.append(self.seq())
        return alts[0] if len(alts) == 1 else ("alt", alts)

    def seq(self):
        items = []
        while self.i < len(self.p) and self.peek() not in "|)":
            items.append(self.quant(self.atom()))
        return items[0] if len(items) == 1 else ("cat", items)

    def quant(self, node):
        while True:
            ch = self.peek()
            if ch and ch in "*+?":
                m, n = {"*": (0, None), "+": (1, None), "?": (0, 1)}[ch]
                self.i += 1
            elif ch == "{":
                got = self.braces()             # (stops behind `}`)
                if got is None:
                    return node
                m, n = got
            else:
                return node
            if self.peek() == "?":              # a lazy form: the same language
                self.i += 1
            node = ("rep", node, m, n)

    def braces(self):
        """`{m}`, `{m,}`, `{m,n}` at the cursor -> (m, n) with the cursor behind `}`; anything else is a literal `{` (as in `re`): None."""
        j = self.p.find("}", self.i)
        body = self.p[self.i + 1:j] if j > 0 else ""
        parts = body.split(",")
        if j < 0 or len(parts) > 2 or any(q and not (q.isdigit() and q.isascii()) for q in parts) or (len(parts) == 1 and not parts[0]):
            return None
        m = int(parts[0] or 0)                  # (`{,n}` = `{0,n}`, as in `re`)
        n = m if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
        if n is not None and n < m:
            self.fail("a repeat with max below min")
        if m > 1000 or (n or 0) > 1000:
            self.fail("a repeat count above 1000")
        self.i = j + 1
        return m, n

    def atom(self):
        ch = self.peek()
        self.i += 1
        if ch == "(":
            if self.peek() == "?":
                nxt = self.p[self.i + 1:self.i + 3]
                if nxt[:1] == ":":
                    self.i += 2
                elif nxt[:1] in ("=", "!") or nxt in ("<=", "<!"):
                    self.fail("lookaround `(?" + (nxt if nxt[:1] == "<" else nxt[:1]) + "...)` is not served")
                elif nxt[:2] == "P=":
                    self.fail("backreference `(?P=...)` is not served")
                else:
                    self.fail("group extension `(?" + nxt + "` is not served")
            node = self.alt()
            if self.peek() != ")":
                self.fail("missing `)`")
            self.i += 1
            return node
        if ch == "[":
            return self.klass()
        if ch == ".":
            return _not_ascii(b"\n")
        if ch in "^$":
            self.i -= 1
            self.fail(f"anchor `{ch}` is not served (the match is a full match already)")
        if ch in "*+?":
            self.i -= 1
            self.fail("nothing to repeat")
        if ch == "{":
            self.i -= 1
            if self.braces() is not None:
                self.fail("nothing to repeat")
            self.i += 1
            return _lit(b"{")
        if ch == "\\":
            kind, val = self.escape(False)
            return val if kind == "node" else _lit(chr(val).encode("utf-8"))
        return _lit(ch.encode("utf-8"))

    def escape(self, in_class: bool):
        """Behind a backslash -> ("node", AST) for a class escape or ("chr", code point) for a single character."""
        ch = self.peek()
        if not ch:
            self.fail("a trailing backslash")
        self.i += 1
        sets = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
        if ch in sets:
            return ("node", ("set", sets[ch]))
        if ch.lower() in sets and ch.isupper():
            return ("node", _not_ascii(sets[ch.lower()]))
        simple = {"t": 9, "n": 10, "r": 13, "f": 12, "v": 11, "a": 7, "0": 0}
        if ch in simple:
            return ("chr", simple[ch])
        if ch == "b" and in_class:
            return ("chr", 8)
        if ch == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(c not in "0123456789abcdefABCDEF" for c in h):
                self.fail("a bad \\x escape")
            self.i += 2
            if int(h, 16) > 0x7F:
                self.fail("\\x escapes above 7F are not served (write the character itself)")
            return ("chr", int(h, 16))
        if ch in "bBAZ":
            self.i -= 2
            self.fail(f"anchor `\\{ch}` is not served")
        if ch.isdigit():
            self.i -= 2
            self.fail(f"backreference `\\{ch}` is not served")
        if ch.isalnum() and ch.isascii():
            self.i -= 2
            self.fail(f"escape `\\{ch}` is not served")
        return ("chr", ord(ch))

    def klass(self):
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        members = set()
        first = True
        while True:
            ch = self.peek()
            if not ch:
                self.fail("missing `]`")
            self.i += 1
            if ch == "]" and not first:
                break
            first = False
            if ch == "\\":
                kind, val = self.escape(True)
                if kind == "node":
                    if val[0] != "set":
                        self.fail("a negated escape inside a class is not served")
                    members |= val[1]
                    continue
                lo = val
            else:
                lo = ord(ch)
            hi = lo
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                ch2 = self.peek()
                self.i += 1
                if ch2 == "\\":
                    kind, val = self.escape(True)
                    if kind == "node":
                        self.fail("a bad character range")
                    hi = val
                else:
                    hi = ord(ch2)
                if hi < lo:
                    self.fail("a bad character range")
            if hi > 0x7F:
                self.fail("classes hold ASCII members only (a negated class admits every other character)")
            members |= set(range(lo, hi + 1))
        return _not_ascii(members) if neg else ("set", frozenset(members))


def regex(pattern: str):
    """The AST of a pattern in the subset above (full-match semantics, ASCII classes)."""
    return _Parser(pattern).parse()


def choice(strings: Iterable[str]):
    """One of the given strings (str or bytes), exactly."""
    opts = [s if isinstance(s, bytes) else str(s).encode("utf-8") for s in strings]
    if not opts or any(len(o) == 0 for o in opts):
        raise ValueError("choice: a non-empty list of non-empty strings is required")
    return ("alt", [_lit(o) for o in dict.fromkeys(opts)])


# ---- JSON schema --------------------------------------------------------------------------------------------------------------------------------------
_INT = ("alt", [_lit(b"0"), ("cat", [("rep", _lit(b"-"), 0, 1), _bset(0x31, 0x39), ("rep", ("set", _DIGIT), 0, None)])])      # (no "-0": json.dumps never writes it)
_NUMBER = ("cat", [("rep", _lit(b"-"), 0, 1), ("alt", [_lit(b"0"), ("cat", [_bset(0x31, 0x39), ("rep", ("set", _DIGIT), 0, None)])]), ("rep", ("cat", [_lit(b"."), ("rep", ("set", _DIGIT), 1, None)]), 0, 1),
                   ("rep", ("cat", [("set", frozenset(b"eE")), ("rep", ("set", frozenset(b"+-")), 0, 1), ("rep", ("set", _DIGIT), 1, None)]), 0, 1)])
_HEX = ("set", frozenset(b"0123456789abcdefABCDEF"))
_STR_CHAR = ("alt", [_not_ascii(list(range(0x20)) + [0x22, 0x5C, 0x7F]),
                     ("cat", [_lit(b"\\"), ("alt", [("set", frozenset(b'"\\/bfnrt')), ("cat", [_lit(b"u"), ("rep", _HEX, 4, 4)])])])])
_ANNOTATIONS = {"title", "description", "default", "examples", "$schema", "$id", "required", "format"}
_NOT_SERVED = {"$ref": "`$ref` and recursive schemas are not served (they need a stack)", "$defs": "`$defs` / `$ref` are not served (they need a stack)",
               "definitions": "`definitions` / `$ref` are not served (they need a stack)",
               "additionalProperties": "`additionalProperties` is not served: exactly the declared properties are emitted",
               "patternProperties": "`patternProperties` is not served"}
_KEYS = {"object": {"properties"}, "array": {"items", "minItems", "maxItems"}, "string": {"enum", "minLength", "maxLength", "pattern"},
         "integer": set(), "number": set(), "boolean": set(), "null": set()}


def _scalar(v):
    if v is None or isinstance(v, (bool, int, float, str)):
        return _lit(json.dumps(v).encode("ascii"))
    raise ValueError(f"json_schema: enum / const serve scalars only (got {v!r})")


def _schema(s, indent, level: int):
    if not isinstance(s, dict):
        raise ValueError(f"json_schema: a schema must be an object (got {s!r})")
    for k, why in _NOT_SERVED.items():
        if k in s:
            raise ValueError("json_schema: " + why)
    keys = set(s) - _ANNOTATIONS
    if "const" in s or ("enum" in s and "type" not in s):
        if keys - {"const", "enum", "type"}:
            raise ValueError(f"json_schema: keywords {sorted(keys - {'const', 'enum', 'type'})} are not served beside enum / const")
        vals = [s["const"]] if "const" in s else list(s["enum"])
        if not vals:
            raise ValueError("json_schema: an empty enum")
        return ("alt", [_scalar(v) for v in vals])
    if "anyOf" in s:
        if keys - {"anyOf"}:
            raise ValueError(f"json_schema: keywords {sorted(keys - {'anyOf'})} are not served beside anyOf")
        if not s["anyOf"]:
            raise ValueError("json_schema: an empty anyOf")
        return ("alt", [_schema(a, indent, level) for a in s["anyOf"]])
    t = s.get("type")
    if isinstance(t, list):
        return ("alt", [_schema(dict(s, type=x), indent, level) for x in t])
    if t == "json_object" or t is None:
        raise ValueError("json_schema: free-form JSON (a schema without `type`, {\"type\": \"json_object\"}) is not served: it needs a stack")
    if t not in _KEYS:
        raise ValueError(f"json_schema: type {t!r} is not served")
    extra = keys - {"type"} - _KEYS[t] - ({"enum"} if t != "string" else set())
    # (keywords of other types are errors too: a schema that says more than is enforced must not pass silently)
    if extra:
        raise ValueError(f"json_schema: keywords {sorted(extra)} are not served for type {t!r}")
    if "enum" in s and t != "string":
        return ("alt", [_scalar(v) for v in s["enum"]])
    nl = (lambda lv: b"") if indent is None else (lambda lv: b"\n" + b" " * (int(indent) * lv))
    comma = b", " if indent is None else b","
    if t == "object":
        props = s.get("properties") or {}
        if not props:
            return _lit(b"{}")
        items = [_lit(b"{" + nl(level + 1))]
        for j, (k, v) in enumerate(props.items()):
            if j:
                items.append(_lit(comma + nl(level + 1)))
            items += [_lit(json.dumps(str(k)).encode("ascii") + b": "), _schema(v, indent, level + 1)]
        return ("cat", items + [_lit(nl(level) + b"}")])
    if t == "array":
        if "items" not in s:
            raise ValueError("json_schema: an array needs `items` (free-form elements are not served)")
        lo, hi = int(s.get("minItems", 0)), s.get("maxItems")
        hi = None if hi is None else int(hi)
        if lo < 0 or (hi is not None and hi < lo) or max(lo, hi or 0) > 1000:
            raise ValueError(f"json_schema: bad minItems / maxItems ({lo}, {hi})")
        item = _schema(s["items"], indent, level + 1)
        if hi == 0:
            return _lit(b"[]")
        body = ("cat", [_lit(b"[" + nl(level + 1)), item, ("rep", ("cat", [_lit(comma + nl(level + 1)), item]), max(lo - 1, 0), None if hi is None else hi - 1),
                        _lit(nl(level) + b"]")])
        return body if lo > 0 else ("alt", [_lit(b"[]"), body])
    if t == "string":
        if "enum" in s:
            if not s["enum"] or any(not isinstance(v, str) for v in s["enum"]):
                raise ValueError("json_schema: a string enum needs strings")
            return ("alt", [_scalar(v) for v in s["enum"]])
        if "pattern" in s:
            if "maxLength" in s or "minLength" in s:
                raise ValueError("json_schema: `pattern` is not served together with minLength / maxLength")
            return ("cat", [_lit(b'"'), regex(s["pattern"]), _lit(b'"')])
        lo, hi = int(s.get("minLength", 0)), s.get("maxLength")
        if lo < 0 or (hi is not None and int(hi) < lo) or max(lo, int(hi or 0)) > 1000:
            raise ValueError(f"json_schema: bad minLength / maxLength ({lo}, {hi})")
        return ("cat", [_lit(b'"'), ("rep", _STR_CHAR, lo, None if hi is None else int(hi)), _lit(b'"')])
    return {"integer": _INT, "number": _NUMBER, "boolean": ("alt", [_lit(b"true"), _lit(b"false")]), "null": _lit(b"null")}[t]


def json_schema(schema, indent: Optional[int] = None):
    """The AST of the JSON texts that satisfy `schema` (the subset in the module docstring), laid out as `json.dumps(obj, indent=indent)` lays them out."""
    if isinstance(schema, str):
        schema = json.loads(schema)
    if indent is not None and (isinstance(indent, bool) or not isinstance(indent, int) or indent < 0):
        raise ValueError(f"json_schema: indent has to be None or a non-negative integer, but is {indent!r}")
    return _schema(schema, indent, 0)


def response_format_spec(response_format):
    """The reference's `ResponseFormat` shape (`type` plus `json_schema.schema`, as an object or a dict) -> ("json_schema", schema), or None for
    `type: "text"` / None.  `json_object` raises: free-form JSON is not served."""
    if response_format is None:
        return None
    get = (lambda o, k: o.get(k)) if isinstance(response_format, dict) else (lambda o, k: getattr(o, k, None))
    t = get(response_format, "type")
    if t in (None, "text"):
        return None
    if t == "json_object":
        raise ValueError("response_format: {\"type\": \"json_object\"} (free-form JSON) is not served: it needs a stack; give a json_schema")
    if t != "json_schema":
        raise ValueError(f"response_format: type {t!r} is not served")
    js = get(response_format, "json_schema")
    if js is None:
        raise ValueError("response_format: type json_schema needs `json_schema`")
    schema = js.get("schema") if isinstance(js, dict) else getattr(js, "schema", None)
    if schema is None and hasattr(js, "schema_"):
        schema = js.schema_
    if schema is None:
        raise ValueError("response_format: `json_schema.schema` is missing")
    return ("json_schema", schema)


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# AST -> NFA -> DFA
# ------------------------------------------------------------------------------------------------------------------------------------------------------
class _Nfa:
    def __init__(self):
        self.eps: List[List[int]] = []
        self.edges: List[List[Tuple[int, int]]] = []        # (256-bit mask, target)

    def new(self) -> int:
        self.eps.append([])
        self.edges.append([])
        if len(self.eps) > 400000:
            raise ValueError("constraint: the pattern expands to more than 400000 NFA states")
        return len(self.eps) - 1

    def build(self, node, a: int) -> int:
        """Thread `node` from state a; returns its end state."""
        kind = node[0]
        if kind == "set":
            b = self.new()
            mask = 0
            for v in node[1]:
                mask |= 1 << v
            if mask:
                self.edges[a].append((mask, b))
            return b
        if kind == "cat":
            for ch in node[1]:
                a = self.build(ch, a)
            return a
        if kind == "alt":
            end = self.new()
            for ch in node[1]:
                s = self.new()
                self.eps[a].append(s)
                self.eps[self.build(ch, s)].append(end)
            return end
        if kind == "rep":
            _, inner, m, n = node
            for _ in range(m):
                a = self.build(inner, a)
            if n is None:
                s, end = self.new(), self.new()
                self.eps[a] += [s, end]
                e = self.build(inner, s)
                self.eps[e] += [s, end]
                return end
            end = self.new()
            self.eps[a].append(end)
            for _ in range(n - m):
                a = self.build(inner, a)
                self.eps[a].append(end)
            return end
        raise ValueError(f"constraint: unknown AST node {kind!r}")


def byte_dfa(ast) -> Tuple[np.ndarray, np.ndarray, int]:
    """AST -> the minimal byte DFA of its language: (trans int32 [S][256] with -1 = dead, accept bool [S], start).  Every state can reach acceptance."""
    nfa = _Nfa()
    s0 = nfa.new()
    end = nfa.build(ast, s0)
    n = len(nfa.eps)
    # bytes that no edge tells apart move together: work on one representative per group
    masks = sorted({m for es in nfa.edges for m, _ in es})
    sig = {}
    for b in range(256):
        sig.setdefault(tuple(i for i, m in enumerate(masks) if (m >> b) & 1), []).append(b)
    groups = [g for k, g in sig.items() if k]

    closure_cache = {}

    def closure(states) -> frozenset:
        out, stack = set(states), list(states)
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in out:
                    out.add(t)
                    stack.append(t)
        return frozenset(out)

    start = closure([s0])
    index, order, rows = {start: 0}, [start], []
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        row = np.full(256, -1, dtype=np.int32)
        edges = [e for s in cur for e in nfa.edges[s]]
        for g in groups:
            b = g[0]
            tg = frozenset(t for m, t in edges if (m >> b) & 1)
            if not tg:
                continue
            nxt = closure_cache.get(tg)
            if nxt is None:
                nxt = closure_cache[tg] = closure(tg)
            j = index.get(nxt)
            if j is None:
                j = index[nxt] = len(order)
                order.append(nxt)
                if j > 2 * MAX_STATES:          # (minimisation rarely halves an automaton, and its passes grow with the automaton's depth)
                    raise ValueError(f"constraint: the byte automaton has more than {2 * MAX_STATES} states before minimisation; the table holds {MAX_STATES}")
            row[g] = j
        rows.append(row)
    trans = np.stack(rows)
    accept = np.array([end in st for st in order], dtype=bool)
    del n
    return _minimise(trans, accept, 0)


def _minimise(trans: np.ndarray, accept: np.ndarray, start: int):
    S = trans.shape[0]
    # drop states that cannot reach acceptance
    live = accept.copy()
    while True:
        ext = np.concatenate([live, [False]])
        new = live | ext[trans].any(axis=1)
        if (new == live).all():
            break
        live = new
    if not live[start]:
        raise ValueError("constraint: the language is empty")
    trans = np.where(np.concatenate([live, [False]])[trans], trans, -1)
    keep = np.flatnonzero(live)
    remap = np.full(S + 1, -1, dtype=np.int32)
    remap[keep] = np.arange(keep.size, dtype=np.int32)
    trans, accept, start = remap[trans[keep]], accept[keep], int(remap[start])
    # Moore refinement on the distinct byte columns
    cols = np.unique(trans, axis=1)
    label = accept.astype(np.int64)
    count = len(np.unique(label))
    while True:
        ext = np.concatenate([label, [-1]])
        sigm = np.concatenate([label[:, None], ext[cols]], axis=1)
        _, label = np.unique(sigm, axis=0, return_inverse=True)
        label = label.reshape(-1)
        c = int(label.max()) + 1
        if c == count:
            break
        count = c
    rep = np.full(count, -1, dtype=np.int64)
    rep[label[::-1]] = np.arange(trans.shape[0])[::-1]         # the first state of every block
    ext = np.concatenate([label, [-1]]).astype(np.int32)
    return ext[trans[rep]], accept[rep], int(label[start])


def dfa_accepts(dfa, data: bytes) -> bool:
    s = dfa_run(dfa, data)
    return s >= 0 and bool(dfa[1][s])


def dfa_run(dfa, data: bytes, state: Optional[int] = None) -> int:
    """The state behind `data` from `state` (default: the start), -1 once no member of the language continues the text."""
    trans, _, start = dfa
    s = start if state is None else int(state)
    for b in data:
        if s < 0:
            break
        s = int(trans[s, b])
    return s


# ------------------------------------------------------------------------------------------------------------------------------------------------------
# lift to tokens
# ------------------------------------------------------------------------------------------------------------------------------------------------------
class Automaton:
    """A compiled constraint over one vocabulary.  cls uint16 [V]: the class of every token id; next int16 [S][C]: the table (< 0 = not allowed);
    start; n_classes = C.  The last state is DONE: it is entered by an EOS id from an accepting state and allows only EOS."""

    def __init__(self, cls: np.ndarray, nxt: np.ndarray, start: int, eos_ids: Sequence[int]):
        self.cls = np.ascontiguousarray(cls, dtype=np.uint16)
        self.next = np.ascontiguousarray(nxt, dtype=np.int16)
        self.start = int(start)
        self.n_states, self.n_classes = int(nxt.shape[0]), int(nxt.shape[1])
        self.eos_ids = tuple(int(e) for e in eos_ids)

    @property
    def vocab(self) -> int:
        return int(self.cls.shape[0])

    def step(self, state: int, token: int) -> int:
        """The operator's advance: the next state, or `state` itself where the token is out of range or not allowed."""
        if state < 0 or not 0 <= int(token) < self.vocab:
            return int(state)
        s2 = int(self.next[state, self.cls[int(token)]])
        return s2 if s2 >= 0 else int(state)

    def walk(self, ids, state: Optional[int] = None) -> int:
        """The state behind `ids` from `state` (default: the start); -1 if one of them is not allowed where it stands."""
        s = self.start if state is None else int(state)
        for t in ids:
            if s < 0 or not 0 <= int(t) < self.vocab:
                return -1
            s = int(self.next[s, self.cls[int(t)]])
        return s

    def allowed(self, state: int) -> np.ndarray:
        """bool [V]: the tokens allowed in `state` (none in -1, the state `walk` returns for a text outside the language)."""
        if not 0 <= int(state) < self.n_states:
            return np.zeros(self.vocab, dtype=bool)
        return self.next[int(state)][self.cls] >= 0

    def accepting(self, state: int) -> bool:
        """Whether the text so far is a member of the language (EOS is allowed)."""
        return bool(self.eos_ids) and bool(self.allowed(state)[self.eos_ids[0]])


def compile_automaton(ast, token_bytes: Sequence[Optional[bytes]], eos_ids: Iterable[int], max_states: int = MAX_STATES,
                      max_classes: int = MAX_CLASSES, max_table: Optional[int] = None) -> Automaton:
    """Lift the byte DFA of `ast` over a vocabulary.  token_bytes[id] = the bytes of a token, or None for a special / unusable one (never allowed); an
    empty token is never allowed either.  eos_ids: the ids that end a reply: allowed exactly in accepting states.
    dst[s][t] is computed for all tokens at once, one byte position at a time.  States that cannot reach acceptance through TOKEN transitions are
    dropped (a viable byte prefix may be unspellable in this vocabulary); a start state that goes raises "the vocabulary cannot spell this constraint".
    max_states / max_classes / max_table (entries of the table, n_states x n_classes): the caps of the session that will hold the automaton."""
    dfa = ast if isinstance(ast, tuple) and len(ast) == 3 and isinstance(ast[0], np.ndarray) else byte_dfa(ast)
    trans, accept, start = dfa
    S, V = trans.shape[0], len(token_bytes)
    eos = sorted({int(e) for e in eos_ids})
    if not eos or any(not 0 <= e < V for e in eos):
        raise ValueError(f"constraint: the EOS ids {eos} must be a non-empty set of ids inside the vocabulary of {V}")
    if S + 1 > MAX_STATES:
        raise ValueError(f"constraint: the byte automaton has {S} states; the table holds at most {MAX_STATES}")
    if (S + 1) * V > MAX_LIFT:                                   # refused before anything of that size is allocated
        raise ValueError(f"constraint: {S} byte states x {V} tokens is beyond what the lift holds ({MAX_LIFT} entries): the constraint is too large "
                         "for this vocabulary (shorten its bounded repeats, maxLength / maxItems)")
    lens = np.array([0 if (b is None or i in eos) else len(b) for i, b in enumerate(token_bytes)], dtype=np.int64)
    order = np.argsort(-lens, kind="stable")                     # longest first: the tokens still running at byte j are a prefix of this order
    L = int(lens.max()) if V else 0
    tokb = np.zeros((V, max(L, 1)), dtype=np.uint8)
    for r, i in enumerate(order):
        n = int(lens[i])
        if n == 0:
            break
        tokb[r, :n] = np.frombuffer(token_bytes[i], dtype=np.uint8)
    T = np.concatenate([np.where(trans < 0, S, trans), np.full((1, 256), S, dtype=trans.dtype)]).astype(np.int32)     # row S: dead
    n_live = int((lens > 0).sum())
    dst = np.full((S + 1, V), -1, dtype=np.int16)                # (row S = DONE; S < 32767)
    sorted_lens = lens[order]
    longer = [int(np.searchsorted(-sorted_lens, -j, side="left")) for j in range(L)]       # tokens longer than j: a prefix of the order
    for s0 in range(0, S, 128):                                  # (a block of states at a time bounds the working set)
        s1 = min(s0 + 128, S)
        cur = np.broadcast_to(np.arange(s0, s1, dtype=np.int32)[:, None], (s1 - s0, n_live)).copy()
        for j in range(L):
            k = longer[j]
            cur[:, :k] = T[cur[:, :k], tokb[:k, j][None, :]]
        cur[cur == S] = -1
        dst[s0:s1, order[:n_live]] = cur
    DONE = S
    for e in eos:
        dst[:S, e] = np.where(accept, DONE, -1)
        dst[DONE, e] = DONE
    # token-level trim: the states that reach DONE
    good = np.zeros(S + 1, dtype=bool)
    good[DONE] = True
    while True:
        ext = np.concatenate([good, [False]])
        new = good | np.concatenate([ext[dst[s0:s0 + 128]].any(axis=1) for s0 in range(0, S + 1, 128)])
        if (new == good).all():
            break
        good = new
    if not good[start]:
        raise ValueError("constraint: the vocabulary cannot spell this constraint")
    ext = np.concatenate([good, [False]])
    for s0 in range(0, S + 1, 128):                              # (in place, a block of states at a time)
        blk = dst[s0:s0 + 128]
        blk[~ext[blk]] = -1
    # reachable from the start through what is left
    reach = np.zeros(S + 1, dtype=bool)
    reach[start] = True
    frontier = np.array([start])
    while frontier.size:
        nxt = np.unique(dst[frontier])
        nxt = nxt[nxt >= 0]
        nxt = nxt[~reach[nxt]]
        reach[nxt] = True
        frontier = nxt
    keep = np.flatnonzero(reach)                                 # (DONE is reachable: the start is good)
    remap = np.full(S + 2, -1, dtype=np.int16)
    remap[keep] = np.arange(keep.size, dtype=np.int16)
    dst = remap[dst[keep]]
    n_states = int(keep.size)
    if n_states > min(int(max_states), MAX_STATES):
        raise ValueError(f"constraint: the automaton has {n_states} states; the cap is {min(int(max_states), MAX_STATES)} (max_states)")
    # token classes: the distinct columns
    colsT = np.ascontiguousarray(dst.T)
    void = colsT.view(np.dtype((np.void, colsT.shape[1] * 2))).reshape(-1)
    _, first, inv = np.unique(void, return_index=True, return_inverse=True)
    C = int(first.size)
    if C > min(int(max_classes), MAX_CLASSES):
        raise ValueError(f"constraint: the automaton has {C} token classes; the cap is {min(int(max_classes), MAX_CLASSES)} (max_classes)")
    if max_table is not None and n_states * C > int(max_table):
        raise ValueError(f"constraint: the table of {n_states} states x {C} classes does not fit the session's {int(max_table)} entries "
                         "(batch_open(max_states=, max_classes=))")
    return Automaton(inv.reshape(-1).astype(np.uint16), colsT[first].T, int(remap[start]), eos)


def _gpt2_byte_table():
    """GPT-2's printable stand-ins for the 256 byte values (byte-level BPE): character -> byte."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


def token_bytes_from_tokenizer(tokenizer, vocab_size: Optional[int] = None) -> List[Optional[bytes]]:
    """token_bytes for an HF byte-level BPE tokenizer (Qwen2, GPT-2): `convert_ids_to_tokens` through the GPT-2 byte table.  Added / special tokens
    and pieces the table cannot decode map to None.  vocab_size (the model's, which may exceed the tokenizer's): the ids beyond map to None."""
    table = _gpt2_byte_table()
    n = len(tokenizer)
    special = set(getattr(tokenizer, "all_special_ids", None) or [])
    added = getattr(tokenizer, "get_added_vocab", None)
    special |= set((added() or {}).values()) if callable(added) else set()
    out: List[Optional[bytes]] = []
    for i, tok in enumerate(tokenizer.convert_ids_to_tokens(list(range(n)))):
        if i in special or not isinstance(tok, str) or any(ch not in table for ch in tok):
            out.append(None)
        else:
            out.append(bytes(table[ch] for ch in tok))
    V = n if vocab_size is None else int(vocab_size)
    return out[:V] + [None] * max(0, V - n)


class ConstraintCompiler:
    """Compiles and caches (LRU) automata for ONE vocabulary, keyed by (kind, spec, indent).  kind: "choice" (a list of strings), "regex" (a pattern),
    "json_schema" (a schema; indent as `json_schema`)."""

    def __init__(self, token_bytes: Sequence[Optional[bytes]], eos_ids: Iterable[int], max_states: int = MAX_STATES, max_classes: int = MAX_CLASSES,
                 max_table: Optional[int] = None, cache_size: int = 32):
        self.token_bytes, self.eos_ids = list(token_bytes), sorted({int(e) for e in eos_ids})
        self.caps = dict(max_states=max_states, max_classes=max_classes, max_table=max_table)
        self.cache_size = int(cache_size)
        self._lru: "OrderedDict[tuple, Automaton]" = OrderedDict()
        self.hits = self.misses = 0

    @staticmethod
    def ast(kind: str, spec, indent: Optional[int] = None):
        if kind == "choice":
            return choice(spec)
        if kind == "regex":
            return regex(spec)
        if kind == "json_schema":
            return json_schema(spec, indent)
        raise ValueError(f"constraint: unknown kind {kind!r} (choice, regex, json_schema)")

    def compile(self, kind: str, spec, indent: Optional[int] = None) -> Automaton:
        key = (kind, json.dumps(spec) if not isinstance(spec, str) else spec, indent)
        got = self._lru.get(key)
        if got is not None:
            self._lru.move_to_end(key)
            self.hits += 1
            return got
        self.misses += 1
        got = compile_automaton(self.ast(kind, spec, indent), self.token_bytes, self.eos_ids, **self.caps)
        self._lru[key] = got
        while len(self._lru) > self.cache_size:
            self._lru.popitem(last=False)
        return got

    def choice(self, strings) -> Automaton:
        return self.compile("choice", list(strings))

    def regex(self, pattern: str) -> Automaton:
        return self.compile("regex", pattern)

    def json_schema(self, schema, indent: Optional[int] = None) -> Automaton:
        return self.compile("json_schema", schema, indent)
