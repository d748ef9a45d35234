"""Speculative decoding for penalised, constrained and logprob requests, without a GPU: the closed forms the verify kernels implement against the
sequential application of the references (tests/spec_processed_ref.py), the C ABI's names, and which path a request takes with and without
`spec_processed`."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.constrain_ref import EOS_IDS, synthetic_vocab
from tests.penalty_ref import counts_of
from tests.spec_processed_ref import (chain_counts, chain_states, constrain_chain_ref, constrain_sequential_ref, penalize_chain_ref,
                                      penalize_sequential_ref)
from tests.test_constrain_cpu import _BpeTok
from tests.test_logprobs_cpu import _LpModel
from tests.test_serving_cpu import _Model, _Tok
from vila_amd import _lib, configs, serving
from vila_amd import constrain as cn
from vila_amd.modules import _step_symbols

V = 257
PARAMS = [(1.3, 0.5, 0.25), (0.02, 0.0, 0.0), (1.0, -3.0, -1e4), (1.0, 0.0, 0.0)]


def _bits(t):
    return torch.as_tensor(np.asarray(t)).contiguous().view(torch.int32)


# ---- the closed forms ------------------------------------------------------------------------------------------------------------------------
PEN_CASES = {
    "distinct": [3, 9, 200, 256, 0],
    "a draft repeats an id twice and three times": [5, 5, 7, 5, 7, 0],
    "counts at 65534 and 65535": [11, 11, 11, 12, 12],
    "ids out of range count nothing": [-1, V, 4, -7, V + 100, 4],
    "padding rows repeat token[0]": [8, 1, 8, 8, 8, 8, 8, 8],
}


@pytest.mark.parametrize("name", list(PEN_CASES))
def test_the_saturating_sum_equals_the_sequential_bumps(name):
    tokens = PEN_CASES[name]
    g = torch.Generator().manual_seed(len(name))
    n = len(tokens)
    x = torch.randn(n, V, generator=g) * 3
    x[:, 20], x[:, 21], x[:, 22] = -0.0, float("inf"), float("-inf")
    counts = torch.tensor([0, 1, 2, 65535])[torch.randint(0, 4, (V,), generator=g)]
    counts[11], counts[12], counts[5], counts[7] = 65534, 65535, 0, 65533
    for pen in PARAMS:
        y_seq, tables = penalize_sequential_ref(x, counts, tokens, *pen)
        y = penalize_chain_ref(x, counts, tokens, *pen)
        assert torch.equal(_bits(y), _bits(y_seq)), (name, pen)
        for i in range(n):
            assert torch.equal(chain_counts(counts, tokens, i), tables[i]), (name, i)
        if pen == (1.0, 0.0, 0.0):
            assert torch.equal(_bits(y), _bits(x)), "neutral values copy the bits"
    assert int(chain_counts(counts, PEN_CASES["counts at 65534 and 65535"], 2)[11]) == 65535
    assert int(chain_counts(torch.zeros(V), PEN_CASES["a draft repeats an id twice and three times"], 3)[5]) == 3
    # the commit's table: the histogram of the first m + 1 consumed ids
    for m in range(n):
        assert torch.equal(chain_counts(torch.zeros(V), tokens, m), counts_of(tokens[:m + 1], V)[0])


TB = synthetic_vocab()
COMP = cn.ConstraintCompiler(TB, EOS_IDS)
AUTOS = dict(choice=COMP.choice(["yes", "no!", "abc"]), loop=COMP.regex(r"(yes|no|ab|abc|bc|[ ,01]|12|100)+"))


def _ids(text: bytes):
    return [TB.index(bytes([b])) for b in text]


@pytest.mark.parametrize("kind", list(AUTOS))
def test_the_state_chain_equals_the_sequential_advance(kind):
    a = AUTOS[kind]
    Vv, C = a.vocab, a.n_classes
    g = torch.Generator().manual_seed(7)
    yes = TB.index(b"yes")
    cases = {
        "all allowed": _ids(b"yes") if kind == "choice" else _ids(b"yes01"),
        "a forbidden draft mid-chain": [_ids(b"y")[0], TB.index(b"~1~"), _ids(b"e")[0], _ids(b"s")[0]],
        "ids out of range": [-1, _ids(b"y")[0], Vv, _ids(b"e")[0]],
        "a multi-byte token, then padding": [yes, yes, yes, yes],
    }
    for name, tokens in cases.items():
        x = (torch.randn(len(tokens), Vv, generator=g) * 3).numpy()
        x[:, 3] = -0.0
        for start in (a.start, -1):
            y, states = constrain_chain_ref(x, start, a.cls, a.next, C, tokens)
            y_seq, states_seq = constrain_sequential_ref(x, start, a.cls, a.next, C, tokens)
            assert states == states_seq and np.array_equal(y.view(np.int32), y_seq.view(np.int32)), (kind, name, start)
            if start == -1:
                assert states == [-1] * len(tokens) and np.array_equal(y.view(np.int32), x.view(np.int32)), "an unconstrained row copies the bits"
            else:
                s = start
                for i, t in enumerate(tokens):
                    s = a.step(s, t)
                    assert states[i] == s
    # the forbidden draft: the row in front of it holds -inf at it, and the state stays where it was
    tokens = cases["a forbidden draft mid-chain"]
    y, states = constrain_chain_ref(np.zeros((4, Vv), dtype=np.float32), a.start, a.cls, a.next, C, tokens)
    assert y[0, tokens[1]] == -np.inf and states[1] == states[0]
    # a class beyond the table's class count leaves the state as well
    assert chain_states(a.start, [5], np.full(Vv, C), a.next.reshape(-1), C, Vv) == [a.start]


# ---- the C ABI's names -------------------------------------------------------------------------------------------------------------------
def test_step_symbols_name_the_processed_entry_and_keep_the_refusals():
    for kw in (dict(verify=True), dict(verify_sample=True), dict(verify_sample=True, any_k=True), dict(verify=True, penalized=True, constrained=True)):
        for w4 in (False, True):
            assert _step_symbols(True, w4, False, processed=True, **kw) == ("vila_llm_decode_step_verify_processed",
                                                                            "vila_llm_decode_verify_processed_workspace_bytes")
    with pytest.raises(ValueError, match="verify step"):
        _step_symbols(True, False, False, processed=True)
    n_args = {"vila_llm_decode_step_verify_processed": 12, "vila_llm_decode_verify_processed_workspace_bytes": 3, "vila_logits_penalize_verify_f32": 11,
              "vila_logits_constrain_verify_f32": 12, "vila_verify_commit": 8, "vila_logprobs_seq_f32": 10}
    for name, n in n_args.items():
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n, name
    # every spelling from before keeps its refusal
    with pytest.raises(ValueError, match="no penalised form"):
        _step_symbols(True, False, False, verify=True, penalized=True)
    with pytest.raises(ValueError, match="no constrained form"):
        _step_symbols(True, False, False, verify_sample=True, constrained=True)
    with pytest.raises(ValueError, match="no penalised, constrained or shared-prefix form"):
        _step_symbols(True, False, True, verify_sample=True, any_k=True, penalized=True)
    assert _step_symbols(True, False, False, verify=True) == ("vila_llm_decode_step_verify", "vila_llm_decode_verify_workspace_bytes")


# ---- generate's routing --------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def cpu_llm():
    from vila_amd.vlm import HipLlavaLlamaModel
    return HipLlavaLlamaModel(configs.tiny("mlp_downsample"), device="cpu").llm


def test_generate_reaches_the_verify_path_only_with_the_flag(cpu_llm, monkeypatch):
    H = cpu_llm.lcfg.hidden_size
    one = torch.zeros(1, 4, H, dtype=torch.bfloat16)
    auto = cn.ConstraintCompiler(synthetic_vocab() + [None] * (cpu_llm.lcfg.vocab_size - 1000), EOS_IDS).choice(["yes", "no"])
    seen = []
    monkeypatch.setattr(cpu_llm, "_generate_verify", lambda *a, **k: seen.append((len(a), k)) or "verify", raising=False)
    asks = [(dict(repetition_penalty=1.1), "no penalised form"), (dict(presence_penalty=0.5, frequency_penalty=0.25), "no penalised form"),
            (dict(constraint=auto), "no constrained form"), (dict(logprobs=5), "no logprob form")]
    for ask, why in asks:
        for spec in (dict(prompt_lookup_num_tokens=3), dict(draft_ids=torch.tensor([1, 2, 3]))):
            with pytest.raises(ValueError, match=why):
                cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, **spec, **ask)
            with pytest.raises(ValueError, match=why):
                cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, spec_processed=False, **spec, **ask)
    assert seen == []
    assert cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, prompt_lookup_num_tokens=3, spec_processed=True, repetition_penalty=1.1) == "verify"
    assert seen[-1] == (13, dict(penalties=(1.1, 0.0, 0.0)))
    cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, draft_ids=torch.tensor([1, 2]), spec_processed=True, constraint=auto, logprobs=5, presence_penalty=0.5)
    assert seen[-1] == (13, dict(penalties=(1.0, 0.5, 0.0), logprobs=5, constraint=auto))
    # read from generation_config; sampled with spec_sample and any_top_k
    cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, generation_config=SimpleNamespace(prompt_lookup_num_tokens=3, spec_processed=True), logprobs=0)
    assert seen[-1] == (13, dict(logprobs=0))
    cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, prompt_lookup_num_tokens=3, spec_processed=True, do_sample=True, spec_sample=True, any_top_k=True,
                     top_k=0, seed=1, frequency_penalty=0.25)
    assert seen[-1] == (13, dict(any_top_k=True, penalties=(1.0, 0.0, 0.25)))
    # the flag alone changes nothing: a plain speculative request makes the call it always made
    cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, prompt_lookup_num_tokens=3, spec_processed=True)
    cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, prompt_lookup_num_tokens=3)
    assert seen[-2] == seen[-1] == (13, {})
    # a sampled request still needs spec_sample
    with pytest.raises(ValueError, match="do_sample"):
        cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, prompt_lookup_num_tokens=3, spec_processed=True, do_sample=True, repetition_penalty=1.1)


# ---- serving ---------------------------------------------------------------------------------------------------------------------------------
def test_generate_content_keeps_or_drops_the_speculation_by_the_flag():
    tok = _Tok()
    m = _LpModel(tok)
    for ask in (dict(repetition_penalty=1.1), dict(logprobs=True, top_logprobs=2)):
        serving.generate_content(m, tok, "what is this ?", prompt_lookup_num_tokens=4, **ask)
        assert "prompt_lookup_num_tokens" not in m.sampling and "spec_processed" not in m.sampling, "without the flag the drafts are dropped"
        serving.generate_content(m, tok, "what is this ?", prompt_lookup_num_tokens=4, spec_processed=True, **ask)
        assert m.sampling["prompt_lookup_num_tokens"] == 4 and m.sampling["spec_processed"] is True
    serving.generate_content(m, tok, "what is this ?", prompt_lookup_num_tokens=4, spec_processed=True)
    assert m.sampling == dict(prompt_lookup_num_tokens=4), "a plain request makes the call it always made"
    serving.generate_content(m, tok, "what is this ?", spec_processed=True, repetition_penalty=1.1)
    assert m.sampling == dict(repetition_penalty=1.1), "no drafts asked for: nothing to keep"
    serving.generate_content(m, tok, "what is this ?", temperature=0.2, presence_penalty=0.5, prompt_lookup_num_tokens=4, spec_sample=True, spec_processed=True)
    assert m.sampling["spec_sample"] is True and m.sampling["spec_processed"] is True and m.sampling["presence_penalty"] == 0.5
    serving.generate_content(m, tok, "what is this ?", temperature=0.2, presence_penalty=0.5, prompt_lookup_num_tokens=4, spec_processed=True)
    assert "prompt_lookup_num_tokens" not in m.sampling and "spec_processed" not in m.sampling, "a sampled request speculates only with spec_sample"
    btok = _BpeTok()
    bm = _Model(btok)
    serving.generate_content(bm, btok, "what is this ?")
    serving.generate_content(bm, btok, "what is this ?", guided_choice=["ared", "red"], prompt_lookup_num_tokens=4, spec_processed=True)
    assert sorted(bm.sampling) == ["constraint", "prompt_lookup_num_tokens", "spec_processed"]


def test_create_app_passes_the_flag_on_for_solo_requests():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    tok = _Tok()
    m = _Model(tok)
    body = {"model": "stub", "max_tokens": 8, "temperature": 0.0, "messages": [{"role": "user", "content": "what is this ?"}], "repetition_penalty": 1.1}
    client = TestClient(serving.create_app(m, tok, model_name="stub", prompt_lookup_num_tokens=4))
    assert client.post("/chat/completions", json=body).status_code == 200
    assert m.sampling == dict(repetition_penalty=1.1), "without the flag the app makes the calls it always made"
    client = TestClient(serving.create_app(m, tok, model_name="stub", prompt_lookup_num_tokens=4, spec_processed=True))
    assert client.post("/chat/completions", json=body).status_code == 200
    assert m.sampling == dict(repetition_penalty=1.1, prompt_lookup_num_tokens=4, spec_processed=True)
    assert client.post("/chat/completions", json={k: v for k, v in body.items() if k != "repetition_penalty"}).status_code == 200
    assert m.sampling == dict(prompt_lookup_num_tokens=4)
    client = TestClient(serving.create_app(m, tok, model_name="stub", spec_processed=True))
    assert client.post("/chat/completions", json=body).status_code == 200 and m.sampling == dict(repetition_penalty=1.1)
