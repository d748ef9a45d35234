"""Speculative decoding for sampled requests, the parts that need no GPU: the three new entry points on both sides of the C ABI, the step
table's spelling for them (beside the refusal it keeps), what `generate(spec_sample=True)` refuses before it touches a device, and the serving
shim's routing with a stub model."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests.test_serving_cpu import _Model, _Tok
from vila_amd import _lib, configs, serving
from vila_amd.modules import _step_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["vila_llm_decode_verify_sample_workspace_bytes", "vila_llm_decode_step_verify_sample", "vila_llm_decode_step_verify_w4_sample"]


def test_new_prototypes_on_both_sides():
    header = open(os.path.join(ROOT, "include", "vila_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", flat)
        assert m, f"{name} is not declared in include/vila_hip.h"
        n_args = 0 if m.group(1).strip() in ("", "void") else m.group(1).count(",") + 1
        assert n_args == len(_lib.PROTOTYPES[name][1]), f"{name}: {n_args} arguments in the header, {len(_lib.PROTOTYPES[name][1])} in _lib.PROTOTYPES"
    # the sampled steps take the greedy steps' arguments and the sampling struct in front of the stream
    for w4 in ("", "_w4"):
        greedy, sampled = _lib.PROTOTYPES["vila_llm_decode_step_verify" + w4][1], _lib.PROTOTYPES["vila_llm_decode_step_verify" + w4 + "_sample"][1]
        assert sampled[:-2] == greedy[:-1] and sampled[-1] is greedy[-1]
        assert sampled[-2]._type_ is _lib.VilaBatchSampling


def test_step_table_spells_the_sampled_verify_step():
    for w4 in (False, True):
        step, ws = _step_symbols(True, w4, True, verify_sample=True)
        assert step == "vila_llm_decode_step_verify" + ("_w4" if w4 else "") + "_sample" and ws == "vila_llm_decode_verify_sample_workspace_bytes"
        assert step in _lib.PROTOTYPES and ws in _lib.PROTOTYPES
        assert len(_lib.PROTOTYPES[step][1]) == 7 + int(w4), step
        assert _step_symbols(False, w4, True, verify_sample=True) == (step, ws)          # one sequence's rows: `batch` is not read
        # the old spelling keeps its refusal and its greedy answer
        with pytest.raises(ValueError, match="verify step is greedy"):
            _step_symbols(True, w4, True, verify=True)
        assert _step_symbols(True, w4, False, verify=True) == ("vila_llm_decode_step_verify" + ("_w4" if w4 else ""), "vila_llm_decode_verify_workspace_bytes")


@pytest.fixture(scope="module")
def cpu_llm():
    from vila_amd.vlm import HipLlavaLlamaModel
    return HipLlavaLlamaModel(configs.tiny("mlp_downsample"), device="cpu").llm


def test_generate_refuses_what_the_sampled_mode_does_not_serve(cpu_llm):
    H = cpu_llm.lcfg.hidden_size
    one, two = torch.zeros(1, 4, H, dtype=torch.bfloat16), torch.zeros(2, 4, H, dtype=torch.bfloat16)
    base = dict(max_new_tokens=4, prompt_lookup_num_tokens=3, do_sample=True, spec_sample=True, seed=1)
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="top_k"):
            cpu_llm.generate(inputs_embeds=one, **dict(base, top_k=k))
    with pytest.raises(ValueError, match="top_k"):                  # draft_ids opens the mode as well
        cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, draft_ids=torch.tensor([1, 2, 3]), do_sample=True, spec_sample=True, top_k=0)
    with pytest.raises(ValueError, match="top_k"):                  # spec_sample is read from generation_config, as batch_sample is
        cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, prompt_lookup_num_tokens=3,
                         generation_config=SimpleNamespace(do_sample=True, spec_sample=True, top_k=100))
    with pytest.raises(ValueError, match="temperature"):
        cpu_llm.generate(inputs_embeds=one, **dict(base, temperature=0.0))
    with pytest.raises(ValueError, match="top_p"):
        cpu_llm.generate(inputs_embeds=one, **dict(base, top_p=0.0))
    with pytest.raises(ValueError, match="batch size 1"):
        cpu_llm.generate(inputs_embeds=two, **base)
    with pytest.raises(ValueError, match="1..15"):
        cpu_llm.generate(inputs_embeds=one, **dict(base, prompt_lookup_num_tokens=16))
    with pytest.raises(ValueError, match="forced_ids"):
        cpu_llm.generate(inputs_embeds=one, forced_ids=torch.tensor([1, 2]), **base)
    with pytest.raises(ValueError, match="return_logits"):
        cpu_llm.generate(inputs_embeds=one, return_logits=True, **base)
    # without the opt-in the refusal is the one it always was
    with pytest.raises(ValueError, match="do_sample"):
        cpu_llm.generate(inputs_embeds=one, max_new_tokens=4, prompt_lookup_num_tokens=3, do_sample=True, spec_sample=False)


def test_generate_content_passes_both_through_for_a_sampled_request():
    tok = _Tok()
    m = _Model(tok)
    serving.generate_content(m, tok, "what is this ?", temperature=0.2, top_p=0.9, prompt_lookup_num_tokens=4, spec_sample=True)
    assert m.sampling["do_sample"] is True and m.sampling["prompt_lookup_num_tokens"] == 4 and m.sampling["spec_sample"] is True
    serving.generate_content(m, tok, "what is this ?", temperature=0.2, top_p=0.9, prompt_lookup_num_tokens=4)
    assert m.sampling["do_sample"] is True and "prompt_lookup_num_tokens" not in m.sampling and "spec_sample" not in m.sampling
    serving.generate_content(m, tok, "what is this ?", prompt_lookup_num_tokens=4, spec_sample=True)          # a greedy request: as ever
    assert m.sampling == {"prompt_lookup_num_tokens": 4}


def test_app_routes_the_default_request_to_the_sampled_verify_step():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    tok = _Tok()
    body = {"model": "stub", "max_tokens": 8, "messages": [{"role": "user", "content": "what is this ?"}]}
    m = _Model(tok)
    r = TestClient(serving.create_app(m, tok, model_name="stub", prompt_lookup_num_tokens=4, spec_sample=True)).post("/chat/completions", json=body)
    assert r.status_code == 200
    # the default request samples at 0.2 / 0.9 / 50 and now speculates
    assert m.sampling["do_sample"] is True and abs(m.sampling["temperature"] - 0.2) < 1e-6 and abs(m.sampling["top_p"] - 0.9) < 1e-6
    assert m.sampling["top_k"] == 50 and m.sampling["prompt_lookup_num_tokens"] == 4 and m.sampling["spec_sample"] is True
    # without the flag the sampled request takes the path it always took
    m2 = _Model(tok)
    r = TestClient(serving.create_app(m2, tok, model_name="stub", prompt_lookup_num_tokens=4)).post("/chat/completions", json=body)
    assert r.status_code == 200 and m2.sampling["do_sample"] is True
    assert "prompt_lookup_num_tokens" not in m2.sampling and "spec_sample" not in m2.sampling
    # a greedy request of the flagged app speculates as before, without the flag's keyword
    r = TestClient(serving.create_app(m, tok, model_name="stub", prompt_lookup_num_tokens=4, spec_sample=True)).post(
        "/chat/completions", json=dict(body, temperature=0.0))
    assert r.status_code == 200 and m.sampling == {"prompt_lookup_num_tokens": 4}


def test_chat_session_passes_spec_sample_on():
    """ChatSession.ask hands `spec_sample` to llm.generate beside the lookup's prompt_ids."""
    tok = _Tok()
    seen = {}

    class _Llm:
        def new_cache(self, max_ctx):
            return SimpleNamespace(max_ctx=max_ctx)

        def generate(self, inputs_embeds, max_new_tokens, cache, **kw):
            seen.update(kw)
            return torch.tensor([[7, 1]])

    cfg = configs.tiny()
    model = SimpleNamespace(cfg=cfg, device=torch.device("cpu"), llm=_Llm(),
                            _embed=lambda ids, media, mc, a, b: (torch.zeros(1, ids.shape[1], 8), None, None))
    s = serving.ChatSession(model, tok, max_ctx=256)
    s.ask("what is this ?", max_new_tokens=2, do_sample=True, temperature=0.2, prompt_lookup_num_tokens=4, spec_sample=True)
    assert seen["spec_sample"] is True and seen["prompt_lookup_num_tokens"] == 4 and seen["prompt_ids"].tolist() == s.ids[:-2]
