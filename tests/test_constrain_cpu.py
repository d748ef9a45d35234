"""The host side of structured output (vila_amd/constrain.py): the regex compiler against `re` and `regex`, the token lift against brute force on
finite languages, the token-level trim, json_schema by random walks, the caps and refusals, and the byte table of byte-level BPE
tokenizers.  Everything is exact; nothing here needs a GPU."""
import itertools
import json
import re

import numpy as np
import pytest

from tests.constrain_ref import EOS_IDS, SPLIT_ID, brute_allowed, constrain_ref, pairs_ref, synthetic_vocab
from vila_amd import constrain as cn
from vila_amd import serving

PATTERNS = [r"abc", r"a|b", r"(ab|a)*c?", r"a{2,3}b", r"[a-c]+", r"[^a]b", r"\d+\.\d*", r"a.c", r"(?:ab)+?c", r"a{2}", r"a{1,}b?", r"[\w-]+", r"\s*a",
            r"[]a]b", r"a\|b", r"x{,2}", r"(a|)b", r"a*?b", r"a??b", r"[^\d\s]+", r"\w\W", r"(a(b|c))+", r"a{0}b", r"[a\]]+", r"\.\*", r"a{1,2}?b", r"\S\D",
            r"(ab){2,}", r"a|bc|", r"[-a]b", r"\x41b", r"a{b"]
ALPHABET = "abc1. |-\n"
# `regex`'s partial matching over-approximates under a LAZY quantifier (fullmatch("a*?b", "ac", partial=True) matches, though no member of a*b starts
# with "ac"): the prefix oracle of a lazy pattern is its greedy twin, which has the same language; `re.fullmatch` is asked the pattern itself
GREEDY_TWIN = {r"(?:ab)+?c": r"(?:ab)+c", r"a*?b": r"a*b", r"a??b": r"a?b", r"a{1,2}?b": r"a{1,2}b"}
HAND = ["", "é", "aéc", "a\nc", "ab" * 10 + "c", "a" * 7 + "b", "12.50", "a-b_c9", " \t\na", "a]b", "]b", "a|b", "Ab", "a{b", "ééb", "\U0001F600b", "é1"]


@pytest.mark.parametrize("p", PATTERNS)
def test_regex_compiler_agrees_with_re_and_regex(p):
    regex_mod = pytest.importorskip("regex")                          # (the prefix oracle; nothing else in this file needs it)
    dfa = cn.byte_dfa(cn.regex(p))
    strings = ["".join(t) for n in range(5) for t in itertools.product(ALPHABET, repeat=n)] + HAND
    for s in strings:
        want = re.fullmatch(p, s, re.ASCII) is not None
        assert cn.dfa_accepts(dfa, s.encode()) == want, (p, s, want)
        live = regex_mod.fullmatch(GREEDY_TWIN.get(p, p), s, partial=True, flags=regex_mod.ASCII) is not None
        assert (cn.dfa_run(dfa, s.encode()) >= 0) == live, (p, s, live)
    # minimal: no two states with the same behaviour, every state reaches acceptance
    trans, accept, _ = dfa
    assert len({(bool(accept[i]), trans[i].tobytes()) for i in range(len(accept))}) == len(accept)
    live = accept.copy()
    for _ in range(len(accept)):
        live = live | np.array([bool(live[row[row >= 0]].any()) for row in trans])
    assert live.all(), "a state that cannot reach acceptance survived"


def test_bytes_inside_a_character_keep_a_live_state():
    dfa = cn.byte_dfa(cn.regex(r"a.c"))
    e = "é".encode()
    assert cn.dfa_run(dfa, b"a" + e[:1]) >= 0 and cn.dfa_run(dfa, b"a" + e[1:]) < 0 and cn.dfa_accepts(dfa, b"a" + e + b"c")
    assert cn.dfa_run(dfa, b"a\xc0") < 0 and cn.dfa_run(dfa, b"a\xed\xa0") < 0, "overlongs and surrogates are no characters"


@pytest.mark.parametrize("p, construct", [(r"^a", "anchor"), (r"a$", "anchor"), (r"a\b", "anchor"), (r"\Aa", "anchor"), (r"(a)\1", "backreference"),
                                          (r"(?P<x>a)(?P=x)", "group extension|backreference"), (r"(?=a)a", "lookaround"), (r"(?<!a)b", "lookaround"),
                                          (r"a(?!b)", "lookaround")])
def test_unsupported_constructs_are_named(p, construct):
    with pytest.raises(ValueError, match=construct):
        cn.regex(p)


# ---- the token lift -------------------------------------------------------------------------------------------------------------------------------------
TB = synthetic_vocab()
FINITE = {
    "choice": (cn.choice(["yes", "no", "no!", "abc", "true", "né"]), [b"yes", b"no", b"no!", b"abc", b"true", "né".encode()]),
    "regex": (cn.regex(r"(ab|bc){1,2}1?"), [x + y + z for x in (b"ab", b"bc") for y in (b"", b"ab", b"bc") for z in (b"", b"1")]),
    "json": (cn.json_schema({"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"enum": [12, None, "é"]}}}),
             [json.dumps({"ok": o, "n": n}).encode() for o in (True, False) for n in (12, None, "é")]),
}


def test_synthetic_vocabulary_has_the_stated_shape():
    assert len(TB) == 1000 and all(TB[i] == bytes([i]) for i in range(256)) and TB[EOS_IDS[0]] is None and TB[EOS_IDS[1]] is None
    assert TB[SPLIT_ID] == b'"\xc3' and sum(b is None for b in TB) > 10 and {b'{"', b'": ', b'true', b'12'} <= set(TB)


@pytest.mark.parametrize("name", sorted(FINITE))
def test_token_lift_equals_brute_force_on_a_finite_language(name):
    ast, members = FINITE[name]
    members = sorted(set(members))
    a = cn.compile_automaton(ast, TB, EOS_IDS)
    assert a.cls.dtype == np.uint16 and a.next.dtype == np.int16 and a.vocab == 1000 and a.next.shape == (a.n_states, a.n_classes)
    seen, stack, visited = 0, [(b"", a.start)], set()
    while stack:
        text, s = stack.pop()
        if (text, s) in visited:
            continue
        visited.add((text, s))
        want, member = brute_allowed(members, text, TB)
        got = set(np.flatnonzero(a.allowed(s)).tolist())
        assert got - set(EOS_IDS) == want, (name, text, sorted(got ^ want)[:8])
        assert (set(EOS_IDS) <= got) == member and (not (set(EOS_IDS) & got) or member), (name, text)
        assert a.accepting(s) == member
        seen += 1
        for t in want:
            s2 = a.step(s, t)
            assert s2 >= 0 and a.walk([t], s) == s2
            stack.append((text + TB[t], s2))
    assert seen > len(members)
    done = a.step(a.walk([i for i in members[0]]), EOS_IDS[1])          # the single-byte spelling of a member, then EOS
    assert done == a.n_states - 1 and set(np.flatnonzero(a.allowed(done)).tolist()) == set(EOS_IDS) and a.step(done, EOS_IDS[0]) == done
    assert a.walk([ord("q")]) == -1 and a.step(a.start, ord("q")) == a.start and a.step(a.start, 5000) == a.start


def test_a_token_may_end_inside_a_character():
    a = cn.compile_automaton(cn.json_schema({"type": "object", "properties": {"s": {"type": "string", "maxLength": 2}}}), TB, EOS_IDS)
    s = a.walk(list(b'{"s": '))
    assert a.allowed(s)[SPLIT_ID], "'\"' + the first byte of 'é' keeps the text a prefix of a member"
    s = a.step(s, SPLIT_ID)
    rest = TB.index("é".encode()[1:] + b'"')
    assert set(np.flatnonzero(a.allowed(s)).tolist()) <= set(range(0x80, 0xC0)) | {rest}, "only a continuation byte may follow"
    assert a.accepting(a.walk([rest, ord("}")], s)) and not a.accepting(a.walk([rest], s))


def test_token_level_trim():
    drop = [ord("e")]                                                 # no token can spell an 'e': "yes" and "true" go, the others stay
    tb = synthetic_vocab(drop=drop)
    assert all(b is None or b"e" not in b for b in tb)
    a = cn.compile_automaton(cn.choice(["yes", "no", "abc", "true"]), tb, EOS_IDS)
    members = [b"no", b"abc"]
    stack, visited = [(b"", a.start)], set()
    while stack:
        text, s = stack.pop()
        if text in visited:
            continue
        visited.add(text)
        want, member = brute_allowed(members, text, tb)
        got = set(np.flatnonzero(a.allowed(s)).tolist())
        assert got - set(EOS_IDS) == want and a.accepting(s) == member, (text, got ^ want)
        stack += [(text + tb[t], a.step(s, t)) for t in want]
    assert not a.allowed(a.start)[ord("y")] and not a.allowed(a.start)[ord("t")], "a viable byte prefix that cannot be finished is not offered"
    with pytest.raises(ValueError, match="the vocabulary cannot spell this constraint"):
        cn.compile_automaton(cn.choice(["yes", "true"]), tb, EOS_IDS)
    for ast in (cn.choice(["yes", "no", "abc", "true"]), cn.regex(r"(no|abc|e)+"), FINITE["json"][0]):
        try:
            b = cn.compile_automaton(ast, tb, EOS_IDS)
        except ValueError:
            continue
        assert all(b.allowed(s).any() for s in range(b.n_states)), "a reachable state with nothing allowed"


# ---- json_schema ----------------------------------------------------------------------------------------------------------------------------------------
SCHEMAS = {
    "flat": {"type": "object", "properties": {"name": {"type": "string", "maxLength": 6}, "age": {"type": "integer"}, "ok": {"type": "boolean"}, "x": {"type": "null"}}},
    "nested": {"type": "object", "properties": {"id": {"type": "integer"}, "who": {"type": "object", "properties": {"name": {"type": "string", "maxLength": 4},
                                                                                                                    "tags": {"type": "array", "items": {"type": "boolean"}, "maxItems": 2}}}}},
    "array": {"type": "array", "items": {"type": "integer"}, "minItems": 1, "maxItems": 4},
    "enum": {"type": "object", "properties": {"colour": {"enum": ["red", "green", 12, None, True]}, "size": {"type": "string", "enum": ["S", "M"]}, "k": {"const": "v"}}},
    "anyOf": {"anyOf": [{"type": "integer"}, {"type": "array", "items": {"type": ["boolean", "null"]}, "maxItems": 3}, {"type": "object", "properties": {"a": {"type": "boolean"}}}]},
    "number": {"type": "object", "properties": {"v": {"type": "number"}, "s": {"type": "string", "maxLength": 5}, "p": {"type": "string", "pattern": "[a-c]{1,3}-\\d"}}},
}
TEXT_EXACT = {"flat": False, "nested": False, "array": True, "enum": True, "anyOf": True, "number": False}    # (no floats, no string escapes)


def _valid(schema, v) -> bool:
    """A small validator of the served subset."""
    if "const" in schema:
        return v == schema["const"] and type(v) is type(schema["const"])
    if "anyOf" in schema:
        return any(_valid(s, v) for s in schema["anyOf"])
    if "enum" in schema:
        return any(v == e and type(v) is type(e) for e in schema["enum"])
    t = schema["type"]
    if isinstance(t, list):
        return any(_valid(dict(schema, type=x), v) for x in t)
    if t == "object":
        return isinstance(v, dict) and list(v) == list(schema.get("properties", {})) and all(_valid(s, v[k]) for k, s in schema["properties"].items())
    if t == "array":
        return (isinstance(v, list) and schema.get("minItems", 0) <= len(v) <= schema.get("maxItems", 10 ** 9) and all(_valid(schema["items"], x) for x in v))
    if t == "string":
        return (isinstance(v, str) and len(v) <= schema.get("maxLength", 10 ** 9) and
                ("pattern" not in schema or re.fullmatch(schema["pattern"], v, re.ASCII) is not None))
    return {"integer": type(v) is int, "number": type(v) in (int, float), "boolean": type(v) is bool, "null": v is None}[t]


def _skeleton(text: str) -> str:
    """A JSON text with every string literal and every number blanked: what is left is the layout — brackets, separators, newlines, indentation —
    and the literals true / false / null."""
    text = re.sub(r'"(?:[^"\\]|\\.)*"', '"S"', text)
    return re.sub(r"-?\d+(?:\.\d+)?(?:[eE][+-]?\d+)?|-?Infinity", "0", text)      # (json.dumps writes a float that overflowed as Infinity)


@pytest.mark.parametrize("indent", [None, 2], ids=["compact", "indent2"])
@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_json_schema_random_walks_parse_and_validate(name, indent):
    schema = SCHEMAS[name]
    a = cn.compile_automaton(cn.json_schema(schema, indent=indent), TB, EOS_IDS)
    rng = np.random.default_rng(hash((name, indent is None)) % 2 ** 31)
    skipped, texts = 0, set()
    for _ in range(200):
        s, out = a.start, []
        while len(out) <= 256:
            ok = np.flatnonzero(a.allowed(s))
            assert ok.size, "a reachable state with nothing allowed"
            t = int(rng.choice(ok))
            if t in EOS_IDS:
                break
            out.append(t)
            s = a.step(s, t)
        else:
            skipped += 1
            continue
        text = b"".join(TB[t] for t in out).decode("utf-8")
        obj = json.loads(text)
        assert _valid(schema, obj), (name, text)
        if TEXT_EXACT[name]:
            assert json.dumps(obj, indent=indent) == text, (name, text)
        else:                                                         # the layout, whatever spelling the scalars took: strings and numbers blanked
            assert _skeleton(json.dumps(obj, indent=indent)) == _skeleton(text), (name, text)
        texts.add(text)
    assert skipped <= 10, f"{skipped} of 200 walks passed 256 tokens"
    assert len(texts) > 20 or name in ("enum",)


def test_json_layouts_are_those_of_json_dumps():
    obj = {"a": [1, 2], "b": {"c": True, "d": []}, "e": "x"}
    schema = {"type": "object", "properties": {"a": {"type": "array", "items": {"type": "integer"}}, "b": {"type": "object", "properties": {
        "c": {"type": "boolean"}, "d": {"type": "array", "items": {"type": "null"}}}}, "e": {"type": "string"}}}
    for indent in (None, 2, 4):
        dfa = cn.byte_dfa(cn.json_schema(schema, indent=indent))
        assert cn.dfa_accepts(dfa, json.dumps(obj, indent=indent).encode())
        assert not cn.dfa_accepts(dfa, json.dumps(obj, indent=3).encode()) and not cn.dfa_accepts(dfa, json.dumps(obj, separators=(",", ":")).encode())
    assert cn.dfa_accepts(cn.byte_dfa(cn.json_schema({"type": "object", "properties": {}})), b"{}")


@pytest.mark.parametrize("schema, match", [({"$ref": "#/x"}, r"\$ref"), ({"type": "object", "properties": {}, "additionalProperties": False}, "additionalProperties"),
                                           ({"type": "json_object"}, "free-form JSON"), ({}, "free-form JSON"), ({"type": "array"}, "items"),
                                           ({"type": "string", "minimum": 3}, "minimum"), ({"type": "integer", "maximum": 3}, "maximum"),
                                           ({"type": "object", "patternProperties": {}}, "patternProperties"), ({"enum": [[1]]}, "scalars"),
                                           ({"type": "string", "pattern": "^a"}, "anchor"), ({"allOf": []}, "free-form|allOf")])
def test_unsupported_schemas_raise(schema, match):
    with pytest.raises(ValueError, match=match):
        cn.json_schema(schema)


def test_response_format_shapes():
    from types import SimpleNamespace as NS
    schema = {"type": "boolean"}
    assert cn.response_format_spec({"type": "json_schema", "json_schema": {"name": "x", "schema": schema}}) == ("json_schema", schema)
    assert cn.response_format_spec(NS(type="json_schema", json_schema=NS(name="x", schema=schema))) == ("json_schema", schema)
    assert cn.response_format_spec(None) is None and cn.response_format_spec({"type": "text"}) is None
    with pytest.raises(ValueError, match="json_object"):
        cn.response_format_spec({"type": "json_object"})
    with pytest.raises(ValueError, match="json_schema"):
        cn.response_format_spec({"type": "json_schema"})


def test_caps_and_the_compiler_cache():
    ast = cn.json_schema(SCHEMAS["flat"])
    full = cn.compile_automaton(ast, TB, EOS_IDS)
    with pytest.raises(ValueError, match=r"states; the cap is 8 \(max_states\)"):
        cn.compile_automaton(ast, TB, EOS_IDS, max_states=8)
    with pytest.raises(ValueError, match=r"token classes; the cap is 4 \(max_classes\)"):
        cn.compile_automaton(ast, TB, EOS_IDS, max_classes=4)
    with pytest.raises(ValueError, match="does not fit the session"):
        cn.compile_automaton(ast, TB, EOS_IDS, max_table=full.n_states * full.n_classes - 1)
    assert cn.compile_automaton(ast, TB, EOS_IDS, max_table=full.n_states * full.n_classes).n_states == full.n_states
    with pytest.raises(ValueError, match="32767"):
        cn.compile_automaton(cn.regex(r"[ab]*a[ab]{14}"), TB, EOS_IDS)        # (2^15 states, all distinct)
    with pytest.raises(ValueError, match="EOS"):
        cn.compile_automaton(ast, TB, [])
    comp = cn.ConstraintCompiler(TB, EOS_IDS, cache_size=2)
    a = comp.choice(["yes", "no"])
    assert comp.choice(["yes", "no"]) is a and (comp.hits, comp.misses) == (1, 1)
    b, c = comp.regex(r"ab+"), comp.json_schema(SCHEMAS["array"], indent=2)
    assert comp.json_schema(SCHEMAS["array"], indent=2) is c and comp.json_schema(SCHEMAS["array"]) is not c      # indent is part of the key
    assert comp.choice(["yes", "no"]) is not a, "the least recently used entry was kept beyond the cache size"
    assert b.n_states >= 3


def test_numpy_reference_of_the_operator():
    a = cn.compile_automaton(cn.choice(["yes", "no"]), TB, EOS_IDS)
    x = np.linspace(-3, 3, 1000, dtype=np.float32)[None].repeat(2, 0)
    nxt = np.stack([a.next.reshape(-1)] * 2)
    y, s = constrain_ref(x, [a.start, -1], np.stack([a.cls] * 2), nxt, [a.n_classes] * 2, token=[ord("y"), 5])
    assert s.tolist() == [a.step(a.start, ord("y")), -1] and np.array_equal(y[1], x[1])
    assert np.array_equal(np.isfinite(y[0]), a.allowed(s[0])) and np.array_equal(y[0][np.isfinite(y[0])], x[0][a.allowed(s[0])])
    pv, pi = pairs_ref(y, 32)
    # x rises with the index: the merged pick of the constrained row is its LAST allowed id, that of the free row the last id; no slice is empty
    assert pi[0][pv[0] == pv[0].max()].min() == np.flatnonzero(a.allowed(s[0]))[-1] and pi[1][pv[1] == pv[1].max()].min() == 999
    assert pi.max() < 1000 and pairs_ref(y[:, :8], 32)[1][0, 2:].min() == 0x7FFFFFFF, "an empty slice reports an index beyond every real one"
    y0, s0 = constrain_ref(x, [a.start, 3], np.stack([a.cls] * 2), nxt, [a.n_classes] * 2, token=[ord("q"), 1000])
    assert s0.tolist() == [a.start, 3], "a disallowed or out-of-range token leaves the state"


def test_token_bytes_from_a_byte_level_tokenizer():
    table = {b: c for c, b in cn._gpt2_byte_table().items()}
    assert len(table) == 256 and table[ord("a")] == "a" and table[ord(" ")] == "Ġ" and table[ord("\n")] == "Ċ"
    enc = lambda data: "".join(table[b] for b in data)
    vocab = [enc(b"a"), enc(b" the"), enc("é".encode()), enc("é".encode()[:1]), enc(b'{"'), "<|im_end|>", "<|endoftext|>", enc(b"\n\n")]

    class Tok:
        all_special_ids = [6]

        def __len__(self):
            return len(vocab)

        def convert_ids_to_tokens(self, ids):
            return [vocab[i] for i in ids]

        def get_added_vocab(self):
            return {"<|im_end|>": 5, "<|endoftext|>": 6}

    tb = cn.token_bytes_from_tokenizer(Tok(), vocab_size=10)
    assert tb == [b"a", b" the", "é".encode(), b"\xc3", b'{"', None, None, b"\n\n", None, None]
    a = cn.compile_automaton(cn.regex(r"a( the)?é"), tb, [5, 6])
    assert a.accepting(a.walk([0, 1, 3])) is False and a.accepting(a.walk([0, 1, 2])) and a.accepting(a.walk([0, 2]))
    assert a.walk([0, 3]) == -1, "no token of this vocabulary finishes the character: the split is trimmed"


# ---- serving ---------------------------------------------------------------------------------------------------------------------------------------------
from tests.test_serving_cpu import _Model, _StubEngine, _Tok, _want      # noqa: E402


class _BpeTok(_Tok):
    """`_Tok` with the face of a byte-level BPE tokenizer: its words are their own GPT-2 spellings (ASCII), id 1 is the special EOS."""
    all_special_ids = [1]

    def __len__(self):
        return max(self.inv) + 1

    def convert_ids_to_tokens(self, ids):
        return [self.inv.get(i) for i in ids]


def test_serving_compiles_what_a_request_asks_for():
    from types import SimpleNamespace as NS
    comp = cn.ConstraintCompiler(TB, EOS_IDS)
    schema = {"type": "object", "properties": {"ok": {"type": "boolean"}}}
    fmt = {"type": "json_schema", "json_schema": {"name": "r", "schema": schema}}
    a = serving.constraint_of(dict(response_format=fmt), comp)
    assert a is serving.constraint_of(dict(response_format=NS(type="json_schema", json_schema=NS(schema=schema))), comp) and a is comp.json_schema(schema, indent=2)
    assert a.accepting(a.walk(list(json.dumps({"ok": True}, indent=2).encode()))) and a.walk(list(json.dumps({"ok": True}).encode())) == -1
    assert serving.constraint_of(dict(guided_regex="ab+"), comp) is comp.regex("ab+") and serving.constraint_of(dict(temperature=0.2), comp) is None
    assert serving.constraint_of(dict(guided_choice=("yes", "no")), comp) is comp.choice(["yes", "no"])
    assert serving.constraint_of(dict(response_format={"type": "text"}), comp) is None
    with pytest.raises(ValueError, match="json_object"):
        serving.constraint_of(dict(response_format={"type": "json_object"}), comp)
    with pytest.raises(ValueError, match="cannot spell"):
        serving.constraint_of(dict(guided_choice=["yes"]), cn.ConstraintCompiler(synthetic_vocab(drop=[ord("e")]), EOS_IDS))
    assert serving.structured_of(dict(temperature=0.2, guided_regex=None, response_format={"type": "text"})) == {}
    assert serving.structured_of(dict(guided_regex="a", top_p=1.0)) == dict(guided_regex="a")
    with pytest.raises(ValueError, match="one of"):
        serving.structured_of(dict(guided_regex="a", guided_choice=["a"]))
    with pytest.raises(ValueError, match="stream"):
        serving.check_structured_request(dict(guided_regex="a"), True)
    assert serving.check_structured_request(dict(), True) == {} and serving.check_structured_request(dict(guided_regex="a"), False) == dict(guided_regex="a")


def test_compilers_are_kept_per_tokenizer_and_bounded():
    toks = [_BpeTok() for _ in range(serving._COMPILERS_KEPT + 2)]
    for t in toks:
        t("a red square")
    first = serving.constraint_compiler(toks[0], 1000)
    assert serving.constraint_compiler(toks[0], 1000) is first and first.choice(["a", "red"]) is first.choice(["a", "red"])
    for t in toks[1:]:
        serving.constraint_compiler(t, 1000)
    assert len(serving._COMPILERS) == serving._COMPILERS_KEPT and serving.constraint_compiler(toks[0], 1000) is not first, "the oldest entry was kept"


def test_generate_content_passes_the_automaton_on():
    tok = _BpeTok()
    m = _Model(tok)
    assert serving.generate_content(m, tok, "what is this ?") == "a red square" and m.sampling == {}, "a plain request makes the call it always made"
    words = tok("a red square").input_ids
    r = serving.generate_content(m, tok, "what is this ?", guided_choice=["ared", "red"], prompt_lookup_num_tokens=4)
    assert r == "a red square" and sorted(m.sampling) == ["constraint"], "the automaton is passed on, the speculation is dropped"
    a = m.sampling["constraint"]
    assert isinstance(a, cn.Automaton) and a.vocab == m.cfg.llm.vocab_size and a.eos_ids == (1,)
    assert set(np.flatnonzero(a.allowed(a.start)).tolist()) == {words[0], words[1]} and a.accepting(a.walk([words[1]])) and not a.accepting(a.walk([words[0]]))
    fmt = {"type": "json_schema", "json_schema": {"schema": {"enum": ["red", "square"]}}}
    with pytest.raises(ValueError, match="cannot spell"):               # this vocabulary has no quote: the error names the cause
        serving.generate_content(m, tok, "what is this ?", response_format=fmt)
    tok('"red" "square"')
    serving._COMPILERS.clear()                                          # (the vocabulary grew: the byte table is per tokenizer object)
    serving.generate_content(m, tok, "what is this ?", response_format=fmt, temperature=0.5, seed=3)
    assert sorted(m.sampling) == ["constraint", "do_sample", "seed", "temperature", "top_k", "top_p"]
    assert m.sampling["constraint"].accepting(m.sampling["constraint"].walk(tok('"red"').input_ids))
    assert serving.generate_content(m, tok, "what is this ?", response_format={"type": "text"}) == "a red square" and m.sampling == {}
    for bad, why in ((dict(response_format={"type": "json_object"}), "json_object"), (dict(guided_regex="^a"), "anchor"),
                     (dict(guided_regex="a", guided_choice=["a"]), "one of"), (dict(guided_regex="a", streamer=object()), "stream")):
        with pytest.raises(ValueError, match=why):
            serving.generate_content(m, tok, "what is this ?", **bad)


def test_request_schema_and_endpoint_carry_the_fields():
    pytest.importorskip("pydantic")
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    _, Req = serving._request_models()
    r = Req(model="m", messages=[{"role": "user", "content": "hi"}])
    assert r.response_format is None and r.guided_choice is None and r.guided_regex is None
    tok = _BpeTok()
    m = _Model(tok)
    client = TestClient(serving.create_app(m, tok, model_name="stub"))
    body = {"model": "stub", "max_tokens": 8, "temperature": 0.0, "messages": [{"role": "user", "content": "what is this ?"}]}
    r = client.post("/chat/completions", json=body)
    assert r.status_code == 200 and m.sampling == {}
    assert sorted(r.json()) == ["choices", "created", "id", "model", "object"] and list(r.json()["choices"][0]) == ["message"], "today's keys, nothing else"
    r = client.post("/chat/completions", json=dict(body, response_format={"type": "text"}))
    assert r.status_code == 200 and m.sampling == {}
    r = client.post("/chat/completions", json=dict(body, guided_choice=["a", "red"]))
    assert r.status_code == 200 and sorted(m.sampling) == ["constraint"] and r.json()["choices"][0]["message"]["content"][0]["text"] == "a red square"
    r = client.post("/chat/completions", json=dict(body, guided_regex="(a|red)+"))
    assert r.status_code == 200 and isinstance(m.sampling["constraint"], cn.Automaton)
    n_calls = len(m.calls)
    for bad, why in ((dict(guided_regex="a", stream=True), "stream"), (dict(response_format={"type": "json_object"}), "json_object"),
                     (dict(response_format={"type": "json_schema", "json_schema": {"schema": {"$ref": "#/x"}}}), "$ref"),
                     (dict(guided_regex="a", guided_choice=["a"]), "one of"), (dict(guided_choice=["zebra"]), "cannot spell")):
        r = client.post("/chat/completions", json=dict(body, **bad))
        assert r.status_code == 500 and why in r.json()["error"], (bad, r.json())
    assert len(m.calls) == n_calls, "a refused request reached the model"


class _ConEngine(_StubEngine):
    """The stub engine with `HipBatchEngine(constraints=...)`'s additions: the capability, `compile_constraint` (the real compiler, over the synthetic
    vocabulary) and `admit(..., constraint=)`."""
    def __init__(self, constraints, **kw):
        super().__init__(**kw)
        self.batches_constraints = constraints
        self.comp = cn.ConstraintCompiler(TB, EOS_IDS)
        self.admitted, self.solos = [], []

    def compile_constraint(self, asks):
        self._mark("compile")
        return serving.constraint_of(asks, self.comp)

    def admit(self, slot, e, constraint=None):
        self.admitted.append(constraint)
        return super().admit(slot, e)

    def solo(self, prompt, max_new_tokens, system, **gen):
        self.solos.append(gen)
        return super().solo(prompt, max_new_tokens, system, **gen)


def test_a_constrained_request_takes_a_row_only_with_the_flag():
    fmt = {"type": "json_schema", "json_schema": {"schema": {"enum": ["yes", "no"]}}}
    for flag in (True, False):
        eng = _ConEngine(flag, n_slots=4)
        b = serving.ContinuousBatcher(eng, max_batch=4, chunk=4, constraints=True)
        try:
            assert b.constraints == flag
            f1 = b.submit("A:6", 48)                                   # a plain request beside them: served as before
            f2 = b.submit("B:5", 48, response_format=fmt)
            f3 = b.submit("C:4", 48, guided_choice=["yes", "no"])
            f4 = b.submit("D:3", 48, response_format={"type": "text"})
            r1, r2, r3, r4 = (f.result(timeout=30) for f in (f1, f2, f3, f4))
            assert r1 == _want(6) and r4 == _want(3)
            solos = [ev for ev in b.events if ev[0] == "solo"]
            if flag:
                assert r2 == _want(5) and r3 == _want(4) and not solos and eng.solos == []
                assert eng.admitted == [None, eng.comp.json_schema({"enum": ["yes", "no"]}, indent=2), eng.comp.choice(["yes", "no"]), None]
                assert len(eng.threads) == 1, "the automaton is compiled on the worker thread"
            else:
                assert r2.startswith("solo B:5") and r3.startswith("solo C:4") and len(solos) == 2 and eng.admitted == [None, None]
                assert eng.solos == [dict(response_format=fmt), dict(guided_choice=["yes", "no"])], "the solo request carries its field"
                assert "compile" not in eng.calls
            # refused: with a stream, two fields at once; a compile error fails its request alone — the batcher lives
            stream = serving.TextStream(_Tok(), timeout=5)
            for kw, why in ((dict(guided_regex="a", stream=stream), "stream"), (dict(guided_regex="a", guided_choice=["a"]), "one of")):
                with pytest.raises(ValueError, match=why):
                    b.submit("E:3", 48, **kw).result(timeout=30)
            if flag:
                with pytest.raises(ValueError, match="json_object"):
                    b.submit("F:3", 48, response_format={"type": "json_object"}).result(timeout=30)
                with pytest.raises(ValueError, match="anchor"):
                    b.submit("G:3", 48, guided_regex="^a").result(timeout=30)
            assert b.submit("H:3", 48).result(timeout=30) == _want(3)
        finally:
            b.close()
    eng = _ConEngine(True, n_slots=2)                                   # without the batcher's flag an engine that could batch them is not asked to
    b = serving.ContinuousBatcher(eng, max_batch=2, chunk=4)
    try:
        assert not b.constraints and b.submit("I:3", 48, guided_regex="a").result(timeout=30).startswith("solo I:3") and eng.admitted == []
    finally:
        b.close()


def test_engine_and_app_pass_the_flag_only_when_asked(monkeypatch):
    from types import SimpleNamespace
    import torch
    from vila_amd import configs
    calls = []

    class _Llm:
        _bdecode = None

        def batch_open(self, n_slots, max_ctx, max_new_tokens, **kw):
            calls.append(("open", kw))
            self._bdecode = SimpleNamespace()
            return self._bdecode

        def batch_admit(self, st, slot, embeds, **kw):
            calls.append(("admit", slot, kw))
            return 5

    tok = _BpeTok()
    words = tok("a red square").input_ids
    model = SimpleNamespace(llm=_Llm(), cfg=configs.tiny(), device=torch.device("cpu"))
    eng = serving.HipBatchEngine(model, tok, n_slots=2, constraints=True, max_states=16, max_classes=8)
    a = eng.compile_constraint(dict(guided_choice=["a", "red"]))
    assert eng.batches_constraints and a is eng.compile_constraint(dict(guided_choice=["a", "red"])) and a.accepting(a.walk(words[:1]))
    with pytest.raises(ValueError, match="does not fit|cap is"):        # the session's table bounds what is compiled for it
        eng.compile_constraint(dict(guided_regex="(a|red|square){300}"))
    assert eng.admit(0, "e", constraint=a) == 5 and eng.admit(1, "e") == 5
    assert calls == [("open", dict(constraints=True, max_states=16, max_classes=8)), ("admit", 0, dict(constraint=a)), ("admit", 1, {})]
    given = cn.ConstraintCompiler(TB, EOS_IDS)
    assert serving.HipBatchEngine(model, tok, constraints=True, compiler=given).compile_constraint(dict(guided_regex="ab")) is given.regex("ab")
    del calls[:]
    model.llm._bdecode = None
    plain = serving.HipBatchEngine(model, tok, n_slots=2)
    assert not plain.batches_constraints and plain.admit(0, "e") == 5
    assert calls == [("open", {}), ("admit", 0, {})], "an engine without the flag makes the calls it always made"
    # create_app
    pytest.importorskip("fastapi")
    seen = []

    class _Engine:
        def __init__(self, model, tokenizer, n_slots, **kw):
            seen.append(("engine", kw))
            self.n_slots = n_slots

    class _Batcher:
        def __init__(self, engine, max_batch=8, batch_sampled=False, **kw):
            seen.append(("batcher", kw))

    monkeypatch.setattr(serving, "HipBatchEngine", _Engine)
    monkeypatch.setattr(serving, "ContinuousBatcher", _Batcher)
    monkeypatch.setattr(serving, "continuous_batching", lambda model: True)
    serving.create_app(SimpleNamespace(), _Tok(), batch_window_s=0.0)
    serving.create_app(SimpleNamespace(), _Tok(), batch_window_s=0.0, constraints=True)
    assert seen == [("engine", {}), ("batcher", {}), ("engine", dict(constraints=True)), ("batcher", dict(constraints=True))]
