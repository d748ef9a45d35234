"""Per-token logprobs, the parts that need no GPU: the new entry and its struct on both sides of the C ABI, the reference against torch, what
`generate` refuses and which session it selects, the request schema, the endpoint with a stub model, and the batcher's and engine's routing with
stubs."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests.logprob_ref import MAX_TOP, bound, check_rows, logprob_ref
from tests.test_serving_cpu import _Model, _StubEngine, _Tok, _want
from vila_amd import _lib, configs, ops, serving
from vila_amd.modules import HipQwen2ForCausalLM, Logprobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {"vila_logprobs_workspace_bytes": 1, "vila_logprobs_slice_width": 1, "vila_logprobs_f32": 11}


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_new_entries_and_the_struct_on_both_sides_of_the_abi():
    raw = open(os.path.join(ROOT, "include", "vila_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    flat = " ".join(hdr.split())
    for name, n_args in NEW.items():
        assert name in _lib.PROTOTYPES, name
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", flat)
        assert m, f"{name} is not declared in include/vila_hip.h"
        got = 0 if m.group(1).strip() in ("", "void") else m.group(1).count(",") + 1
        assert got == n_args == len(_lib.PROTOTYPES[name][1]), (name, got, len(_lib.PROTOTYPES[name][1]))
    assert "#define VILA_LOGPROBS_MAX_TOP 20" in flat and ops.LOGPROBS_MAX_TOP == 20 == serving.LOGPROBS_MAX_TOP == MAX_TOP
    # the struct: the header's members in the header's order, with the ctypes that lay them out as a C compiler does on this ABI
    m = re.search(r"typedef struct \{([^}]*)\} VilaLogprobOut;", flat)
    assert m, "VilaLogprobOut is not declared in include/vila_hip.h"
    members = [d.strip().rsplit(" ", 1) for d in m.group(1).split(";") if d.strip()]
    members = [(t.replace(" ", ""), n) for t, n in ((t + "*" * n.count("*"), n.lstrip("*")) for t, n in members)]
    assert members == [("float*", "token_logprob"), ("float*", "top_logprob"), ("int32_t*", "top_id"), ("int", "max_rec")], members
    ctype_of = {"float*": C.c_void_p, "int32_t*": C.c_void_p, "int": C.c_int}
    assert [(n, t) for n, t in _lib.VilaLogprobOut._fields_] == [(n, ctype_of[t]) for t, n in members]
    P = C.sizeof(C.c_void_p)
    assert [getattr(_lib.VilaLogprobOut, n).offset for _, n in members] == [0, P, 2 * P, 3 * P] and C.sizeof(_lib.VilaLogprobOut) == 4 * P
    # the header says where the operator goes and that the numbers are raw
    assert "rec_bias = -1" in raw and "RAW" in raw and "logprob.hip" in raw
    assert "logprob.hip" in open(os.path.join(ROOT, "vila_amd", "build.py")).read()


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def test_reference_agrees_with_torch_and_orders_ties_towards_the_lower_index():
    g = torch.Generator().manual_seed(0)
    x = 4 * torch.randn(6, 777, generator=g)
    lp, lse, top_id, top_lp = logprob_ref(x, 20)
    want = torch.log_softmax(x.double(), 1)
    assert torch.allclose(lp, want, rtol=0, atol=1e-12) and torch.allclose(lse, torch.logsumexp(x.double(), 1), rtol=0, atol=1e-12)
    tv, ti = torch.topk(x, 20, dim=1)                                   # no ties in random rows: topk's order is the only one
    assert torch.equal(top_id, ti) and torch.allclose(top_lp, torch.gather(want, 1, ti), rtol=0, atol=1e-12)
    # planted ties: equal values in index order, -0.0 and 0.0 equal
    y = torch.full((2, 50), -5.0)
    y[0, [40, 3, 17]] = 2.0
    y[0, [9, 30]] = 1.0
    y[1, 7], y[1, 5] = 0.0, -0.0
    _, _, ids, lps = logprob_ref(y, 6)
    assert ids[0].tolist() == [3, 17, 40, 9, 30, 0] and ids[1].tolist() == [5, 7, 0, 1, 2, 3]
    assert float(lps[0, 0]) == float(lps[0, 2]) > float(lps[0, 3])
    # a vocabulary below top_n, and -inf rows
    _, _, ids, lps = logprob_ref(torch.tensor([[0.5, -math.inf, 1.5]]), 5)
    assert ids[0].tolist() == [2, 0, 1, -1, -1] and lps[0, 2] == -math.inf and lps[0, 3] == -math.inf
    one = torch.full((1, 9), -math.inf); one[0, 4] = 3.0
    lp1, lse1, _, _ = logprob_ref(one, 0)
    assert float(lp1[0, 4]) == 0.0 and float(lse1) == 3.0
    # the bound and the checker: exact values pass, an error of 64 ulp of the row's scale does not, a wrong id does not, a bad token wants NaN
    b = bound(x, lse)
    assert torch.equal(b, 32 * 2.0 ** -23 * torch.maximum(x.abs().amax(1).double(), lse.abs()).clamp(min=1.0))
    tok = torch.tensor([0, 5, 776, 3, 2, 1])
    good = lp[torch.arange(6), tok].float()
    assert check_rows(x, tok, good, top_lp.float(), top_id, 20) < 1.0
    with pytest.raises(AssertionError, match="bound"):
        check_rows(x, tok, good + 2 * b.float(), top_lp.float(), top_id, 20)
    swapped = top_id.clone(); swapped[2, [3, 4]] = swapped[2, [4, 3]]
    with pytest.raises(AssertionError, match="ids differ"):
        check_rows(x, tok, good, top_lp.float(), swapped, 20)
    bad = tok.clone(); bad[1] = 777
    with pytest.raises(AssertionError, match="NaN"):
        check_rows(x, bad, good, top_lp.float(), top_id, 20)
    good[1] = math.nan
    check_rows(x, bad, good, top_lp.float(), top_id, 20)


# ---- generate's argument handling --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_llm():
    from vila_amd.vlm import HipLlavaLlamaModel
    return HipLlavaLlamaModel(configs.tiny("mlp_downsample"), device="cpu").llm


def test_generate_refuses_and_routes(cpu_llm, monkeypatch):
    H = cpu_llm.lcfg.hidden_size
    one = torch.zeros(1, 4, H, dtype=torch.bfloat16)
    for bad in (21, -1, 2.5, True, "3"):
        with pytest.raises(ValueError, match=r"`logprobs` has to be None or an integer in 0..20"):
            cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, logprobs=bad)
    with pytest.raises(ValueError, match="return_logits"):
        cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, logprobs=3, return_logits=True)
    for spec in (dict(prompt_lookup_num_tokens=3), dict(draft_ids=torch.tensor([1, 2, 3])),
                 dict(generation_config=SimpleNamespace(prompt_lookup_num_tokens=3))):
        with pytest.raises(ValueError, match="speculative decoding"):
            cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, logprobs=3, **spec)
    # logprobs=None makes the call generate always made — the same arguments, the same return value — and k travels as one keyword
    seen = []
    monkeypatch.setattr(cpu_llm, "_generate_solo", lambda *a, **k: seen.append((a, k)) or "out", raising=False)
    assert cpu_llm.generate(inputs_embeds=one, max_new_tokens=4) == "out" and cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, logprobs=None) == "out"
    (a0, k0), (a1, k1) = seen
    assert k0 == k1 == {} and len(a0) == len(a1) == 12 and all(x is y or x == y for x, y in zip(a0[1:], a1[1:])) and a0[0] is a1[0] is one
    del seen[:]
    cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, logprobs=0)
    cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, logprobs=20, repetition_penalty=1.1)
    assert [k for _, k in seen] == [dict(logprobs=0), dict(penalties=(1.1, 0.0, 0.0), logprobs=20)]
    # a padded batch: the batched driver gets the keyword only when asked
    calls = []
    monkeypatch.setattr(cpu_llm, "_can_batch_decode", lambda *a, **k: True, raising=False)
    monkeypatch.setattr(cpu_llm, "_generate_batch", lambda *a, **k: calls.append((len(a), k)) or "batch", raising=False)
    two = torch.zeros(2, 4, H, dtype=torch.bfloat16)
    assert cpu_llm.generate(inputs_embeds=two, max_new_tokens=4) == "batch" and cpu_llm.generate(inputs_embeds=two, max_new_tokens=4, logprobs=None) == "batch"
    assert calls == [(6, {})] * 2
    cpu_llm.generate(inputs_embeds=two, max_new_tokens=4, logprobs=7)
    assert calls[-1] == (8, dict(logprobs=7))


def test_the_flag_enters_the_session_key_only_when_set(cpu_llm, monkeypatch):
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: "stream")
    monkeypatch.setattr(_lib, "load", lambda: SimpleNamespace(vila_logprobs_workspace_bytes=lambda n: 8064 * n + 256,
                                                              vila_llm_decode_workspace_bytes=lambda s, c: 1024,
                                                              vila_llm_decode_penalized_workspace_bytes=lambda s, c: 2048))
    cache = SimpleNamespace(k=torch.zeros(4), max_ctx=256)
    try:
        plain = cpu_llm._decode_session(cache, 8)
        key = plain.key
        assert plain.lp is None and len(key) == 5 and "logprobs" not in key
        assert cpu_llm._decode_session(cache, 8, None, logprobs=False) is plain
        flagged = cpu_llm._decode_session(cache, 8, None, logprobs=True)
        assert flagged is not plain and flagged.key == key + ("logprobs",) and flagged.lp is not None
        assert flagged.lp_tok.shape == (1, 8) and flagged.lp_top.shape == (1, 8, 20) and flagged.lp_id.shape == (1, 8, 20) and flagged.lp_id.dtype == torch.int32
        assert flagged.lp.max_rec == 8 and flagged.lp.token_logprob == flagged.lp_tok.data_ptr() and flagged.lp.top_id == flagged.lp_id.data_ptr()
        assert flagged.ws.numel() == plain.ws.numel(), "the step's own workspace does not change"
        assert cpu_llm._decode_session(cache, 8, None, logprobs=True) is flagged
        both = cpu_llm._decode_session(cache, 8, None, penalties=True, logprobs=True)
        assert both.key == key + (True, "logprobs") and both.pen is not None and both.lp is not None
        assert cpu_llm._decode_session(cache, 8).key == key
    finally:
        cpu_llm._decode = None


def test_pack_logprobs_pads_behind_each_rows_end():
    t = torch.arange(1.0, 5.0); p = torch.arange(80.0).reshape(4, 20); i = torch.arange(80, dtype=torch.int32).reshape(4, 20)
    lp = HipQwen2ForCausalLM._pack_logprobs([(t, p, i), (t, p, i)], [4, 2], 4, 3, "cpu")
    assert isinstance(lp, Logprobs) and lp.token_logprobs.dtype == torch.float32 and lp.top_ids.dtype == torch.int64
    assert lp.token_logprobs.tolist() == [[1, 2, 3, 4], [1, 2, 0, 0]]
    assert lp.top_ids[1].tolist() == [[0, 1, 2], [20, 21, 22], [-1] * 3, [-1] * 3] and bool((lp.top_logprobs[1, 2:] == -math.inf).all())
    assert lp.top_logprobs[0, 3].tolist() == [60.0, 61.0, 62.0]
    assert HipQwen2ForCausalLM._pack_logprobs([(t, p, i)], [4], 4, 0, "cpu").top_ids.shape == (1, 4, 0)


def test_score_refuses_bad_shapes(cpu_llm):
    H = cpu_llm.lcfg.hidden_size
    # (the refusals come before anything touches the device: a stand-in that says it lives there is enough)
    fake = SimpleNamespace(is_cuda=True, dtype=torch.bfloat16, dim=lambda: 2, shape=(10, H), device="cpu")
    for ids, why in ((torch.zeros(0, dtype=torch.int64), "target ids"), (torch.zeros(513, dtype=torch.int64), "target ids"),
                     (torch.zeros(10, dtype=torch.int64), "LAST positions")):
        with pytest.raises(ValueError, match=why):
            cpu_llm.score(fake, ids)
    with pytest.raises(ValueError, match="top_n"):
        cpu_llm.score(fake, torch.zeros(3, dtype=torch.int64), top_n=21)


# ---- serving -----------------------------------------------------------------------------------------------------------------------------
def test_request_schema_carries_the_two_fields():
    pytest.importorskip("pydantic")
    _, Req = serving._request_models()
    r = Req(model="m", messages=[{"role": "user", "content": "hi"}])
    assert r.logprobs is False and r.top_logprobs is None
    r = Req(model="m", messages=[{"role": "user", "content": "hi"}], logprobs=True, top_logprobs=5)
    assert r.logprobs is True and r.top_logprobs == 5


def test_logprobs_of():
    f = serving._logprobs_of
    assert f(None, None) is None and f(False, None) is None and f(True, None) == 0 and f(True, 0) == 0 and f(True, 20) == 20
    for bad in ((False, 3), (None, 0), (True, 21), (True, -1), (True, 2.5)):
        with pytest.raises(ValueError, match="top_logprobs"):
            f(*bad)


class _LpModel(_Model):
    """`_Model` whose generate answers a `logprobs=k` call the way `llm.generate` does: (ids, Logprobs) with 20 alternatives' worth of records cut to
    k, for every returned position — the EOS and the token behind it included, which the shim must drop."""
    def generate(self, input_ids, media, max_new_tokens, eos_token_id, media_config=None, **sampling):
        out = super().generate(input_ids, media, max_new_tokens, eos_token_id, media_config, **sampling)
        if "logprobs" not in sampling:
            return out
        k, n = sampling["logprobs"], out.shape[1]
        words = self.tok("a red square").input_ids
        tl = -0.5 * torch.arange(1, n + 1, dtype=torch.float32)[None]
        pl = (tl[:, :, None] - torch.arange(k, dtype=torch.float32)).contiguous()
        pi = torch.tensor([[[words[(j + a) % len(words)] for a in range(k)] for j in range(n)]], dtype=torch.int64).reshape(1, n, k)
        return out, Logprobs(tl, pl, pi)


def test_generate_content_attaches_the_entries_cut_at_eos():
    tok = _Tok()
    m = _LpModel(tok)
    plain = serving.generate_content(m, tok, "what is this ?")
    assert type(plain) is str and plain == "a red square" and m.sampling == {}
    assert type(serving.generate_content(m, tok, "what is this ?", logprobs=False)) is str and m.sampling == {}
    r = serving.generate_content(m, tok, "what is this ?", logprobs=True, top_logprobs=2, prompt_lookup_num_tokens=4)
    assert isinstance(r, str) and r == "a red square" and m.sampling == dict(logprobs=2), "the speculation is dropped, k is passed on"
    assert [e["token"] for e in r.logprobs] == ["a", "red", "square"], "one entry per reply token: the EOS and what follows are dropped"
    assert [e["logprob"] for e in r.logprobs] == [-0.5, -1.0, -1.5]
    assert all(e["bytes"] == list(e["token"].encode("utf-8")) and len(e["top_logprobs"]) == 2 for e in r.logprobs)
    assert r.logprobs[1]["top_logprobs"] == [{"token": "red", "logprob": -1.0, "bytes": list(b"red")}, {"token": "square", "logprob": -2.0, "bytes": list(b"square")}]
    r0 = serving.generate_content(m, tok, "what is this ?", logprobs=True)
    assert m.sampling == dict(logprobs=0) and all(e["top_logprobs"] == [] for e in r0.logprobs) and len(r0.logprobs) == 3
    with pytest.raises(ValueError, match="top_logprobs"):
        serving.generate_content(m, tok, "what is this ?", top_logprobs=2)
    with pytest.raises(ValueError, match="top_logprobs"):
        serving.generate_content(m, tok, "what is this ?", logprobs=True, top_logprobs=21)
    # unused places (a vocabulary below k: id -1) give no entry
    ents = serving.logprob_entries(tok, tok("a red").input_ids, [-1.0, -2.0], [[-1.0, -math.inf]] * 2, [[tok.vocab["a"], -1]] * 2, 2)
    assert [len(e["top_logprobs"]) for e in ents] == [1, 1]


def test_endpoint_returns_logprobs_only_when_asked():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    tok = _Tok()
    m = _LpModel(tok)
    client = TestClient(serving.create_app(m, tok, model_name="stub"))
    body = {"model": "stub", "max_tokens": 8, "temperature": 0.0, "messages": [{"role": "user", "content": "what is this ?"}]}
    r = client.post("/chat/completions", json=body)
    assert r.status_code == 200 and m.sampling == {}
    j = r.json()
    assert sorted(j) == ["choices", "created", "id", "model", "object"] and list(j["choices"][0]) == ["message"], "today's keys, nothing else"
    assert j["choices"][0]["message"] == {"role": "assistant", "content": [{"type": "text", "text": "a red square"}]}
    r = client.post("/chat/completions", json=dict(body, logprobs=False))
    assert r.status_code == 200 and list(r.json()["choices"][0]) == ["message"] and m.sampling == {}
    r = client.post("/chat/completions", json=dict(body, logprobs=True, top_logprobs=3))
    assert r.status_code == 200 and m.sampling == dict(logprobs=3)
    ch = r.json()["choices"][0]
    assert ch["message"]["content"][0]["text"] == "a red square"
    content = ch["logprobs"]["content"]
    assert [e["token"] for e in content] == ["a", "red", "square"] and all(len(e["top_logprobs"]) == 3 for e in content)
    assert all(set(e) == {"token", "logprob", "bytes", "top_logprobs"} and set(e["top_logprobs"][0]) == {"token", "logprob", "bytes"} for e in content)
    for bad, why in ((dict(logprobs=True, stream=True), "stream"), (dict(top_logprobs=3), "top_logprobs"), (dict(logprobs=True, top_logprobs=21), "0..20")):
        r = client.post("/chat/completions", json=dict(body, **bad))
        assert r.status_code == 500 and why in r.json()["error"], (bad, r.json())


class _LpEngine(_StubEngine):
    """The stub engine with `HipBatchEngine(logprobs=...)`'s additions: the capability and `read_logprobs`, which must be asked while the row is
    still live (before its release)."""
    def __init__(self, logprobs, **kw):
        super().__init__(**kw)
        self.batches_logprobs = logprobs
        self.reads, self.solos = [], []

    def read_logprobs(self, slot, toks, k):
        assert self.script[slot] is not None and self.n_out[slot] + 1 >= len(toks), "the row was released before its records were read"
        self.reads.append((list(toks), k))
        return [{"token": str(t), "logprob": -float(j), "bytes": list(str(t).encode()), "top_logprobs": [None] * k} for j, t in enumerate(toks)]

    def solo(self, prompt, max_new_tokens, system, **gen):
        self.solos.append(gen)
        return super().solo(prompt, max_new_tokens, system, **gen)


def test_a_logprob_request_takes_a_row_only_with_the_flag():
    for flag in (True, False):
        eng = _LpEngine(flag, n_slots=4)
        b = serving.ContinuousBatcher(eng, max_batch=4, chunk=4, logprobs=True)
        try:
            assert b.logprobs == flag
            f1 = b.submit("A:6", 48)                                   # a plain request beside it: served as before
            f2 = b.submit("B:5", 48, logprobs=True, top_logprobs=2)
            f3 = b.submit("C:4", 48, logprobs=False)
            r1, r2, r3 = f1.result(timeout=30), f2.result(timeout=30), f3.result(timeout=30)
            assert r1 == _want(6) and type(r1) is str and r3 == _want(4) and type(r3) is str
            solos = [ev for ev in b.events if ev[0] == "solo"]
            if flag:
                assert r2 == _want(5) and not solos and eng.reads == [([100 + i for i in range(5)], 2)]
                assert [e["token"] for e in r2.logprobs] == _want(5).split() and all(len(e["top_logprobs"]) == 2 for e in r2.logprobs)
            else:
                assert r2.startswith("solo B:5") and len(solos) == 1 and eng.reads == []
                assert eng.solos == [dict(logprobs=True, top_logprobs=2)], "the solo request carries the two keywords"
            f = b.submit("D:3", 48, top_logprobs=2)                    # top_logprobs without logprobs: the request fails, the batcher lives
            with pytest.raises(ValueError, match="top_logprobs"):
                f.result(timeout=30)
            assert b.submit("E:3", 48).result(timeout=30) == _want(3)
        finally:
            b.close()
    # without the batcher's flag an engine that could batch them is not asked to
    eng = _LpEngine(True, n_slots=2)
    b = serving.ContinuousBatcher(eng, max_batch=2, chunk=4)
    try:
        assert not b.logprobs
        assert b.submit("F:3", 48, logprobs=True).result(timeout=30).startswith("solo F:3") and eng.reads == []
    finally:
        b.close()


def test_engine_opens_the_session_with_the_flag_and_reads_a_rows_records():
    calls = []
    tok = _Tok()
    words = tok("a red square").input_ids

    class _Llm:
        _bdecode = None

        def batch_open(self, n_slots, max_ctx, max_new_tokens, **kw):
            calls.append(("open", kw))
            self._bdecode = SimpleNamespace()
            return self._bdecode

        def batch_admit(self, st, slot, embeds, **kw):
            calls.append(("admit", slot, kw))
            return 5

        def batch_logprobs(self, st, slot):
            calls.append(("logprobs", slot))
            return Logprobs(torch.tensor([-1.0, -2.0, -3.0]), torch.zeros(3, 20), torch.tensor([[words[j]] * 20 for j in range(3)]))

    model = SimpleNamespace(llm=_Llm(), cfg=configs.tiny(), device=torch.device("cpu"))
    eng = serving.HipBatchEngine(model, tok, n_slots=2, logprobs=True)
    assert eng.batches_logprobs and eng.admit(0, "e") == 5
    ents = eng.read_logprobs(0, words[:2], 3)
    assert calls == [("open", dict(logprobs=True)), ("admit", 0, {}), ("logprobs", 0)]
    assert [e["token"] for e in ents] == ["a", "red"] and [e["logprob"] for e in ents] == [-1.0, -2.0] and all(len(e["top_logprobs"]) == 3 for e in ents)
    del calls[:]
    model.llm._bdecode = None
    plain = serving.HipBatchEngine(model, tok, n_slots=2)
    assert not plain.batches_logprobs and plain.admit(0, "e") == 5
    assert calls == [("open", {}), ("admit", 0, {})], "an engine without the flag makes the calls it always made"


def test_create_app_passes_the_flag_only_when_asked(monkeypatch):
    pytest.importorskip("fastapi")
    seen = []

    class _Engine:
        def __init__(self, model, tokenizer, n_slots):                  # the narrow constructor of a substituted engine class
            seen.append(("engine", n_slots))
            self.n_slots = n_slots

    class _Batcher:
        def __init__(self, engine, max_batch=8, batch_sampled=False, **kw):
            seen.append(("batcher", kw))

    monkeypatch.setattr(serving, "HipBatchEngine", _Engine)
    monkeypatch.setattr(serving, "ContinuousBatcher", _Batcher)
    monkeypatch.setattr(serving, "continuous_batching", lambda model: True)
    serving.create_app(SimpleNamespace(), _Tok(), batch_window_s=0.0)
    assert seen == [("engine", 8), ("batcher", {})]
    del seen[:]

    class _WideEngine(_Engine):
        def __init__(self, model, tokenizer, n_slots, **kw):
            seen.append(("engine", kw))
    monkeypatch.setattr(serving, "HipBatchEngine", _WideEngine)
    serving.create_app(SimpleNamespace(), _Tok(), batch_window_s=0.0, logprobs=True)
    assert seen == [("engine", dict(logprobs=True)), ("batcher", dict(logprobs=True))]
