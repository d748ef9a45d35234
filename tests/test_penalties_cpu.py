"""Repetition / presence / frequency penalties, the parts that need no GPU: the reference expression against transformers' processor, the new
entries on both sides of the C ABI and in the step table, what `generate` refuses and which session it selects, and the serving shim's routing with a
stub engine."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests.penalty_ref import counts_of, first_argmax, from_u16_bits, penalize_ref, u16_bits
from tests.test_serving_cpu import _Model, _StubEngine, _Tok, _want
from vila_amd import _lib, configs, serving
from vila_amd.modules import HipQwen2ForCausalLM, _step_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {"vila_logits_penalize_slices": 0, "vila_logits_penalize_f32": 11, "vila_llm_decode_penalized_workspace_bytes": 2,
       "vila_llm_decode_step_penalized": 9, "vila_llm_decode_batch_penalized_workspace_bytes": 4, "vila_llm_decode_step_batch_penalized": 10}


# ---- the reference expression ------------------------------------------------------------------------------------------------------------
def test_reference_equals_the_transformers_processor_bit_for_bit():
    transformers = pytest.importorskip("transformers")
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    g = torch.Generator().manual_seed(0)
    V, n = 257, 4
    x = torch.randn(n, V, generator=g) * 4
    x[:, 5], x[:, 6], x[:, 7] = -0.0, 0.0, -0.0
    # histories with duplicated ids, a -0.0 logit inside (5) and outside (7) of them
    hist = torch.tensor([[5, 6, 9, 9, 9, 200, 6, 0], [1, 1, 1, 1, 1, 1, 1, 1], [256, 5, 17, 33, 5, 17, 33, 256], [3, 4, 5, 6, 8, 10, 12, 14]])
    counts = torch.cat([counts_of(h.tolist(), V) for h in hist])
    for rep in (1.05, 1.3, 0.02):
        want = RepetitionPenaltyLogitsProcessor(penalty=rep)(hist, x.clone())
        got = penalize_ref(x, counts, rep, 0.0, 0.0)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), rep
    # neutral parameters return the input bits, -0.0 included
    assert torch.equal(penalize_ref(x, counts, 1.0, 0.0, 0.0).view(torch.int32), x.view(torch.int32))
    # presence and frequency: OpenAI's mu[j] - c[j] * freq - (c[j] > 0) * pres, frequency first
    y = penalize_ref(x, counts, 1.0, 0.5, 0.25)
    assert float(y[0, 9]) == float((x[0, 9] - torch.tensor(0.25) * 3) - 0.5) and float(y[0, 10]) == float(x[0, 10])
    assert first_argmax(torch.tensor([1.0, 3.0, 3.0, 2.0])) == 1
    assert from_u16_bits(u16_bits(torch.tensor([0, 1, 32767, 32768, 65535]))).tolist() == [0, 1, 32767, 32768, 65535]
    # a penalty that is not positive: generate's refusal is HF's, word for word
    with pytest.raises(ValueError) as hf:
        RepetitionPenaltyLogitsProcessor(penalty=0.0)
    with pytest.raises(ValueError) as ours:
        HipQwen2ForCausalLM._check_penalties(0.0, None, None)
    assert str(ours.value) == str(hf.value) == "`penalty` has to be a strictly positive float, but is 0.0"


# ---- the C ABI and the step table --------------------------------------------------------------------------------------------------------
def test_new_entries_on_both_sides_of_the_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vila_hip.h")).read(), flags=re.S)
    flat = " ".join(hdr.split())
    for name, n_args in NEW.items():
        assert name in _lib.PROTOTYPES, name
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", flat)
        assert m, f"{name} is not declared in include/vila_hip.h"
        got = 0 if m.group(1).strip() in ("", "void") else m.group(1).count(",") + 1
        assert got == n_args == len(_lib.PROTOTYPES[name][1]), (name, got, len(_lib.PROTOTYPES[name][1]))
    assert [f[0] for f in _lib.VilaPenalties._fields_] == ["repetition", "presence", "frequency", "counts", "ld_counts"]
    assert "int vila_abi_version" in flat and "uint16_t* counts" in flat


def test_step_table_returns_the_two_penalised_names_for_every_combination():
    solo = ("vila_llm_decode_step_penalized", "vila_llm_decode_penalized_workspace_bytes")
    batch = ("vila_llm_decode_step_batch_penalized", "vila_llm_decode_batch_penalized_workspace_bytes")
    for w4 in (False, True):
        for sampled in (False, True):
            assert _step_symbols(False, w4, sampled, penalized=True) == solo
            for prefix in (False, True):
                assert _step_symbols(True, w4, sampled, prefix=prefix, penalized=True) == batch
            with pytest.raises(ValueError):
                _step_symbols(False, w4, sampled, prefix=True, penalized=True)
        with pytest.raises(ValueError, match="no penalised form"):
            _step_symbols(True, w4, False, verify=True, penalized=True)
        with pytest.raises(ValueError, match="no penalised form"):
            _step_symbols(True, w4, True, verify_sample=True, penalized=True)
    for name in solo + batch:
        assert name in _lib.PROTOTYPES
    # the unpenalised table is what it was
    assert _step_symbols(True, True, True) == ("vila_llm_decode_step_batch_w4_sample", "vila_llm_decode_batch_w4_sample_workspace_bytes_ctx")
    assert _step_symbols(False, False, False) == ("vila_llm_decode_step", "vila_llm_decode_workspace_bytes")


# ---- generate's argument handling --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_llm():
    from vila_amd.vlm import HipLlavaLlamaModel
    return HipLlavaLlamaModel(configs.tiny("mlp_downsample"), device="cpu").llm


def test_check_penalties():
    chk = HipQwen2ForCausalLM._check_penalties
    assert chk(None, None, None) is None and chk(1.0, 0.0, 0.0) is None and chk(1, 0, 0) is None and chk(1.0, None, -0.0) is None
    assert chk(1.1, None, None) == (1.1, 0.0, 0.0) and chk(None, -3, None) == (1.0, -3.0, 0.0) and chk(None, None, -1e4) == (1.0, 0.0, -1e4)
    for bad in (0, 0.0, -1.5, float("nan"), "1.1"):
        with pytest.raises(ValueError, match=r"`penalty` has to be a strictly positive float, but is"):
            chk(bad, None, None)
    with pytest.raises(ValueError, match="finite"):
        chk(None, float("inf"), None)
    with pytest.raises(ValueError, match="finite"):
        chk(None, None, float("nan"))


def test_generate_refuses_and_routes(cpu_llm, monkeypatch):
    H = cpu_llm.lcfg.hidden_size
    one = torch.zeros(1, 4, H, dtype=torch.bfloat16)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match=r"`penalty` has to be a strictly positive float, but is"):
            cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, repetition_penalty=bad)
    with pytest.raises(ValueError, match="strictly positive"):        # read from generation_config under HF's field name
        cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, generation_config=SimpleNamespace(repetition_penalty=0.0))
    # the speculative combinations say so
    for spec in (dict(prompt_lookup_num_tokens=3), dict(draft_ids=torch.tensor([1, 2, 3])), dict(do_sample=True, spec_sample=True, prompt_lookup_num_tokens=3),
                 dict(do_sample=True, spec_sample=True)):
        for pen in (dict(repetition_penalty=1.1), dict(presence_penalty=0.5), dict(frequency_penalty=-1.0)):
            with pytest.raises(ValueError, match="speculative decoding"):
                cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, **spec, **pen)
    with pytest.raises(ValueError, match="speculative decoding"):
        cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, prompt_lookup_num_tokens=3, generation_config=SimpleNamespace(repetition_penalty=1.2))
    # which path a request takes: neutral values make the call generate always made, others carry the three floats
    seen = []
    monkeypatch.setattr(cpu_llm, "_generate_solo", lambda *a, **k: seen.append((len(a), k)) or "out", raising=False)
    for kw in ({}, dict(repetition_penalty=1.0), dict(repetition_penalty=1, presence_penalty=0.0, frequency_penalty=0),
               dict(generation_config=SimpleNamespace(repetition_penalty=1.0, max_new_tokens=4))):
        assert cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, **kw) == "out"
    assert seen == [(12, {})] * 4
    del seen[:]
    cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, repetition_penalty=1.1)
    cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, generation_config=SimpleNamespace(repetition_penalty=1.3, frequency_penalty=0.25), presence_penalty=0.5)
    assert seen == [(12, dict(penalties=(1.1, 0.0, 0.0))), (12, dict(penalties=(1.3, 0.5, 0.25)))]


def test_neutral_values_select_todays_session_key(cpu_llm, monkeypatch):
    """The solo session's key gains the flag only when it is set; the penalised session owns the count table, the parameter arrays and a workspace
    with room for the processed row."""
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: "stream")
    cache = SimpleNamespace(k=torch.zeros(4), max_ctx=256)
    V = cpu_llm.lcfg.vocab_size
    try:
        plain = cpu_llm._decode_session(cache, 8)
        key = plain.key
        assert plain.pen is None and len(key) == 5 and True not in key
        assert cpu_llm._decode_session(cache, 8, None) is plain
        pen = cpu_llm._decode_session(cache, 8, None, penalties=True)
        assert pen is not plain and pen.key == key + (True,) and pen.pen is not None
        assert pen.counts.shape == (1, V) and pen.counts.dtype == torch.int16 and int(pen.counts.abs().sum()) == 0
        assert pen.p_rep.tolist() == [1.0] and pen.p_pres.tolist() == [0.0] and pen.p_freq.tolist() == [0.0]
        assert pen.pen.counts == pen.counts.data_ptr() and pen.pen.ld_counts == V and pen.ws.numel() >= plain.ws.numel() + 4 * V
        assert cpu_llm._decode_session(cache, 8, None, penalties=True) is pen          # the values are not in the key
        pen.counts[0, 3] = 2
        HipQwen2ForCausalLM._set_penalties(pen, 0, (1.3, 0.5, 0.25))
        assert pen.p_rep.tolist() == [pytest.approx(1.3)] and pen.p_freq.tolist() == [0.25] and int(pen.counts.abs().sum()) == 0
        assert cpu_llm._decode_session(cache, 8, None, penalties=True) is pen
        assert cpu_llm._decode_session(cache, 8).key == key
    finally:
        cpu_llm._decode = None


# ---- serving -----------------------------------------------------------------------------------------------------------------------------
def test_request_schema_carries_the_three_fields():
    pytest.importorskip("pydantic")
    _, Req = serving._request_models()
    r = Req(model="m", messages=[{"role": "user", "content": "hi"}])
    assert (r.repetition_penalty, r.presence_penalty, r.frequency_penalty) == (1.0, 0.0, 0.0)
    r = Req(model="m", messages=[{"role": "user", "content": "hi"}], repetition_penalty=1.1, presence_penalty=-0.5, frequency_penalty=0.3)
    assert (r.repetition_penalty, r.presence_penalty, r.frequency_penalty) == (1.1, -0.5, 0.3)


def test_generate_content_passes_non_neutral_penalties_on():
    tok = _Tok()
    m = _Model(tok)
    serving.generate_content(m, tok, "what is this ?")
    assert m.sampling == {}
    serving.generate_content(m, tok, "what is this ?", repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)
    assert m.sampling == {}, "a neutral request makes the call it always made"
    serving.generate_content(m, tok, "what is this ?", repetition_penalty=1.1, frequency_penalty=0.25)
    assert m.sampling == dict(repetition_penalty=1.1, frequency_penalty=0.25)
    serving.generate_content(m, tok, "what is this ?", temperature=0.2, top_p=0.9, presence_penalty=0.5, prompt_lookup_num_tokens=4, spec_sample=True)
    assert m.sampling["presence_penalty"] == 0.5 and m.sampling["do_sample"] is True and "prompt_lookup_num_tokens" not in m.sampling
    # ChatSession.ask hands them to llm.generate, from the session's defaults and per turn
    seen = {}

    class _Llm:
        def new_cache(self, max_ctx):
            return SimpleNamespace(max_ctx=max_ctx)

        def generate(self, inputs_embeds, max_new_tokens, cache, **kw):
            seen.clear(); seen.update(kw)
            return torch.tensor([[7, 1]])

    model = SimpleNamespace(cfg=configs.tiny(), device=torch.device("cpu"), llm=_Llm(),
                            _embed=lambda ids, media, mc, a, b: (torch.zeros(1, ids.shape[1], 8), None, None))
    s = serving.ChatSession(model, tok, max_ctx=256, repetition_penalty=1.1)
    s.ask("what is this ?", max_new_tokens=2)
    assert seen["repetition_penalty"] == 1.1 and "frequency_penalty" not in seen
    s.ask("and this ?", max_new_tokens=2, frequency_penalty=0.3)
    assert seen["repetition_penalty"] == 1.1 and seen["frequency_penalty"] == 0.3 and seen["past_len"] > 0


def test_endpoint_passes_the_penalties_on():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    tok = _Tok()
    m = _Model(tok)
    client = TestClient(serving.create_app(m, tok, model_name="stub"))
    body = {"model": "stub", "max_tokens": 8, "temperature": 0.0, "messages": [{"role": "user", "content": "what is this ?"}]}
    assert client.post("/chat/completions", json=body).status_code == 200 and m.sampling == {}
    assert client.post("/chat/completions", json=dict(body, repetition_penalty=1.0, presence_penalty=0.0)).status_code == 200 and m.sampling == {}
    assert client.post("/chat/completions", json=dict(body, repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.25)).status_code == 200
    assert m.sampling == dict(repetition_penalty=1.1, presence_penalty=0.5, frequency_penalty=0.25)



class _PenEngine(_StubEngine):
    """The stub engine with `HipBatchEngine(penalties=...)`'s two additions: the capability and the admit keyword."""
    def __init__(self, penalties, **kw):
        super().__init__(**kw)
        self.batches_penalties = penalties
        self.admitted = []

    def admit(self, slot, e, **kw):
        self.admitted.append(kw)
        return super().admit(slot, e)


def test_a_penalised_request_takes_a_row_only_with_the_flag():
    for flag in (True, False):
        eng = _PenEngine(flag, n_slots=4)
        b = serving.ContinuousBatcher(eng, max_batch=4, chunk=4, penalties=True)
        try:
            assert b.penalties == flag
            f1 = b.submit("A:6", 48)                                   # neutral: a row, with the call it always took
            f2 = b.submit("B:5", 48, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=None)
            f3 = b.submit("C:4", 48, repetition_penalty=1.1, frequency_penalty=0.25)
            assert f1.result(timeout=30) == _want(6) and f2.result(timeout=30) == _want(5)
            r3 = f3.result(timeout=30)
            solos = [ev for ev in b.events if ev[0] == "solo"]
            if flag:
                assert r3 == _want(4) and not solos
                assert eng.admitted == [{}, {}, dict(penalties=(1.1, 0.0, 0.25))]
            else:
                assert r3.startswith("solo C:4") and len(solos) == 1
                assert eng.admitted == [{}, {}]
        finally:
            b.close()
    # without the batcher's flag an engine that could batch them is not asked to
    eng = _PenEngine(True, n_slots=2)
    b = serving.ContinuousBatcher(eng, max_batch=2, chunk=4)
    try:
        assert not b.penalties
        assert b.submit("D:3", 48, presence_penalty=0.5).result(timeout=30).startswith("solo D:3") and eng.admitted == []
        assert b.submit("E:3", 48).result(timeout=30) == _want(3) and eng.admitted == [{}]
    finally:
        b.close()


def test_engine_opens_the_session_with_the_flag_and_hands_the_row_its_penalties():
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

    model = SimpleNamespace(llm=_Llm(), cfg=configs.tiny(), device=torch.device("cpu"))
    eng = serving.HipBatchEngine(model, _Tok(), n_slots=2, penalties=True)
    assert eng.batches_penalties and eng.admit(0, "e", penalties=(1.1, 0.0, 0.0)) == 5 and eng.admit(1, "e") == 5
    assert calls == [("open", dict(penalties=True)), ("admit", 0, dict(penalties=(1.1, 0.0, 0.0))), ("admit", 1, {})]
    del calls[:]
    model.llm._bdecode = None
    plain = serving.HipBatchEngine(model, _Tok(), n_slots=2)
    assert not plain.batches_penalties and plain.admit(0, "e") == 5
    assert calls == [("open", {}), ("admit", 0, {})], "an engine without the flag makes the calls it always made"
