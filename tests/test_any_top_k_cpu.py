"""Any top_k for the rows of the batched sampler, the parts that need no GPU: the C ABI (the new symbols declared in the header and bound), the step
table (`_step_symbols(any_k=True)`), the host-side validation (`_check_batch_sampling(any_top_k=True)`), the continuous batcher admitting
top_k = 0 / top_k > 64 requests into rows (`ContinuousBatcher(batch_sampled=True, any_top_k=True)`) and the endpoint's new `top_k` field."""
import ctypes as C
import os
import re
import shutil
import subprocess
import time

import pytest
import torch

from tests.test_batch_sampling_cpu import _Engine, _Llm, _Model, _Tok, _want
from vila_amd import _lib, serving
from vila_amd.modules import HipQwen2ForCausalLM, _step_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vila_sample_batch_any_f32", "vila_llm_decode_batch_any_k_workspace_bytes", "vila_llm_decode_step_batch_any_k", "vila_llm_decode_step_verify_any_k")


# ----------------------------------------------------------------------------------------------------------------------
# C ABI and the step table
# ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_in_the_header_and_bound():
    header = open(os.path.join(ROOT, "include", "vila_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), f"{name} is not declared in include/vila_hip.h"
        assert name in _lib.PROTOTYPES, f"{name} has no PROTOTYPES entry in vila_amd/_lib.py"
    # the operator: vila_sample_batch_f32's arguments with (dense_out, ld_dense) in front of the stream
    _, a = _lib.PROTOTYPES["vila_sample_batch_f32"]
    _, b = _lib.PROTOTYPES["vila_sample_batch_any_f32"]
    assert b == a[:-1] + [C.c_void_p, C.c_int64, a[-1]]
    # the batched step: the constrained entry's arguments (every option nullable), and its workspace query's
    assert _lib.PROTOTYPES["vila_llm_decode_step_batch_any_k"] == _lib.PROTOTYPES["vila_llm_decode_step_batch_constrained"]
    assert _lib.PROTOTYPES["vila_llm_decode_batch_any_k_workspace_bytes"] == _lib.PROTOTYPES["vila_llm_decode_batch_constrained_workspace_bytes"]
    # the verify step: the W4 sampled verify step's arguments (the int4 layers nullable)
    assert _lib.PROTOTYPES["vila_llm_decode_step_verify_any_k"] == _lib.PROTOTYPES["vila_llm_decode_step_verify_w4_sample"]
    assert re.search(r"#define\s+VILA_ABI_VERSION\s+1\b", header) or "vila_abi_version" in header


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_header_with_the_new_entries_compiles_as_c99(tmp_path):
    src = tmp_path / "uses.c"
    src.write_text('#include "vila_hip.h"\n'
                   "int main(void) {\n"
                   "    int (*a)(const float*, int64_t, int, int, const VilaBatchSampling*, const int32_t*, int64_t*, void*, float*, float*, int64_t, vila_stream_t)\n"
                   "        = vila_sample_batch_any_f32;\n"
                   "    size_t (*b)(const VilaLlmShape*, int, int, int) = vila_llm_decode_batch_any_k_workspace_bytes;\n"
                   "    return a == 0 || b == 0;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "uses.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, "include/vila_hip.h must compile as C99 with the any-top_k entries:\n" + r.stderr


def test_library_exports_the_new_symbols():
    lib = _lib.load()                                                 # binds every PROTOTYPES entry: a symbol the library lacks raises here
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1], name


def test_step_symbols_name_the_new_entries_and_refuse_nothing_they_served():
    for w4 in (False, True):
        for prefix in (False, True):
            for pen in (False, True):
                for con in (False, True):
                    got = _step_symbols(True, w4, True, prefix=prefix, penalized=pen, constrained=con, any_k=True)
                    assert got == ("vila_llm_decode_step_batch_any_k", "vila_llm_decode_batch_any_k_workspace_bytes")
        assert _step_symbols(True, w4, False, verify_sample=True, any_k=True) == ("vila_llm_decode_step_verify_any_k", "vila_llm_decode_verify_sample_workspace_bytes")
    for bad in (dict(batch=True, w4=False, sampled=False), dict(batch=False, w4=False, sampled=True), dict(batch=True, w4=False, sampled=False, verify=True)):
        with pytest.raises(ValueError):
            _step_symbols(any_k=True, **bad)                           # an option of a sampled batched pick: not of the greedy, solo or greedy verify steps
    with pytest.raises(ValueError):
        _step_symbols(True, False, False, verify_sample=True, penalized=True, any_k=True)
    # without the flag the table is what it was
    assert _step_symbols(True, False, True) == ("vila_llm_decode_step_batch_sample", "vila_llm_decode_batch_sample_workspace_bytes_ctx")
    assert _step_symbols(True, True, True, prefix=True) == ("vila_llm_decode_step_batch_prefix_w4_sample", "vila_llm_decode_batch_prefix_w4_sample_workspace_bytes")
    assert _step_symbols(True, True, False, verify_sample=True) == ("vila_llm_decode_step_verify_w4_sample", "vila_llm_decode_verify_sample_workspace_bytes")
    assert _step_symbols(True, False, True, constrained=True)[0] == "vila_llm_decode_step_batch_constrained"
    assert _step_symbols(True, False, True, penalized=True)[0] == "vila_llm_decode_step_batch_penalized"
    assert _step_symbols(False, False, True) == ("vila_llm_decode_step_sample", "vila_llm_decode_workspace_bytes")


def test_check_batch_sampling_with_and_without_the_flag():
    chk = HipQwen2ForCausalLM._check_batch_sampling
    assert chk((0.7, 0, 0.9, 5), "x", any_top_k=True) == (0.7, 0, 0.9, 5)
    assert chk((0.7, 152064, 1.0, 5), "x", any_top_k=True) == (0.7, 152064, 1.0, 5)
    assert chk((0.7, 64, 1.0, 5), "x", any_top_k=True) == (0.7, 64, 1.0, 5)
    for bad in ((0.7, -1, 0.9, 5), (0.7, 0, 0.0, 5), (0.7, 0, 1.5, 5), (0.0, 0, 0.9, 5)):
        with pytest.raises(ValueError):
            chk(bad, "x", any_top_k=True)
    for k in (0, 65, 152064):
        with pytest.raises(ValueError, match=r"x: the batched sampler serves top_k in 1\.\.64 \(got %d\); such a request runs solo" % k):
            chk((0.7, k, 0.9, 5), "x")
    assert chk((0.7, 50, 0.9, 5), "x") == (0.7, 50, 0.9, 5)


# ----------------------------------------------------------------------------------------------------------------------
# the batcher over the stub engine of tests/test_batch_sampling_cpu.py
# ----------------------------------------------------------------------------------------------------------------------
class _AnyEngine(_Engine):
    batches_any_top_k = True


def test_batcher_with_the_flag_admits_every_top_k_as_a_row_in_arrival_order():
    eng = _AnyEngine(n_slots=4, step_sleep=0.002)
    b = serving.ContinuousBatcher(eng, max_batch=4, chunk=4, batch_sampled=True, any_top_k=True)
    assert b.batch_sampled and b.any_top_k
    try:
        fa = b.submit("A:30", 48)                                      # greedy, long
        while not any(ev[0] == "run" for ev in b.events):
            time.sleep(0.001)
        f0 = b.submit("K0:4", 16, temperature=0.7, top_k=0, seed=3)
        f1 = b.submit("K100:4", 16, temperature=0.7, top_k=100, seed=4)
        f2 = b.submit("K50:4", 16, temperature=0.7, seed=5)
        assert [f.result(timeout=30) for f in (f0, f1, f2)] == [_want(4)] * 3 and fa.result(timeout=30) == _want(30)
        assert not eng.solos and not any(ev[0] == "solo" for ev in b.events)
        got = {n: sp for n, _, sp in eng.admitted}
        assert got["K0:4"] == (0.7, 0, 1.0, 3) and got["K100:4"] == (0.7, 100, 1.0, 4) and got["K50:4"] == (0.7, 50, 1.0, 5) and got["A:30"] is None
        assert [n for n, _, _ in eng.admitted] == ["A:30", "K0:4", "K100:4", "K50:4"]      # arrival order
        admits = [ev for ev in b.events if ev[0] == "admit"]
        assert admits[1][2] > 0 and admits[1][3] >= 1, admits          # K0 joined after steps had run, beside a live row
        # a negative top_k is served by nobody's row
        assert b.submit("N:4", 16, temperature=0.7, top_k=-2).result(timeout=30) == "solo N:4"
    finally:
        b.close()


def test_batcher_flag_needs_the_engine_and_batch_sampled():
    eng = _Engine(n_slots=2)                                           # an engine that does not say it serves any top_k
    b = serving.ContinuousBatcher(eng, max_batch=2, batch_sampled=True, any_top_k=True)
    try:
        assert b.batch_sampled and not b.any_top_k
        assert b.submit("K0:4", 16, temperature=0.7, top_k=0).result(timeout=30) == "solo K0:4"
    finally:
        b.close()
    b2 = serving.ContinuousBatcher(_AnyEngine(n_slots=2), max_batch=2, any_top_k=True)      # without batch_sampled there is nothing to extend
    try:
        assert not b2.any_top_k
    finally:
        b2.close()


# ----------------------------------------------------------------------------------------------------------------------
# the endpoint's `top_k`
# ----------------------------------------------------------------------------------------------------------------------
class _AnyLlm(_Llm):
    def batch_open(self, n_slots, max_ctx=2048, max_new_tokens=1024, sampling=False, any_top_k=False):
        st = super().batch_open(n_slots, max_ctx, max_new_tokens, sampling)
        self.opened[-1] = (bool(sampling), bool(any_top_k))
        return st


class _SoloModel(_Model):
    """A model whose solo `generate` records its keywords and replies "a red square"."""

    def __init__(self, tok):
        super().__init__(tok)
        self.calls = []

    def generate(self, *a, **k):
        self.calls.append(k)
        return torch.tensor([self.llm.reply])


def _body(**kw):
    return dict({"model": "stub", "max_tokens": 8, "messages": [{"role": "user", "content": "what is this ?"}]}, **kw)


def test_endpoint_top_k_travels_into_the_generate_call():
    pytest.importorskip("fastapi")
    import inspect
    from fastapi.testclient import TestClient
    tok = _Tok()
    m = _SoloModel(tok)
    client = TestClient(serving.create_app(m, tok, model_name="stub"))
    r = client.post("/chat/completions", json=_body())                 # absent: 50, today's call
    assert r.status_code == 200, r.text
    assert r.json()["choices"][0]["message"]["content"][0]["text"] == "a red square"
    assert m.calls[-1]["top_k"] == 50 and m.calls[-1]["do_sample"] and m.calls[-1]["top_p"] == pytest.approx(0.9)
    assert inspect.signature(serving.generate_content).parameters["top_k"].default == 50
    for sent, want in ((0, 0), (-1, 0), (100, 100), (20, 20)):         # -1, vLLM's spelling of "no filter", is HF's 0
        r = client.post("/chat/completions", json=_body(top_k=sent, temperature=0.7))
        assert r.status_code == 200, r.text
        assert m.calls[-1]["top_k"] == want and m.calls[-1]["temperature"] == pytest.approx(0.7)
        assert "any_top_k" not in m.calls[-1] and "spec_sample" not in m.calls[-1]
    n = len(m.calls)
    r = client.post("/chat/completions", json=_body(top_k=-2))
    assert r.status_code == 500 and "top_k" in r.json()["error"] and len(m.calls) == n
    r = client.post("/chat/completions", json=_body(top_k=0, temperature=0))        # a greedy request ignores it
    assert r.status_code == 200 and "top_k" not in m.calls[-1] and "do_sample" not in m.calls[-1]


def test_endpoint_spec_sample_with_any_top_k_passes_the_flag_on():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    tok = _Tok()
    m = _SoloModel(tok)
    client = TestClient(serving.create_app(m, tok, model_name="stub", prompt_lookup_num_tokens=4, spec_sample=True, any_top_k=True))
    assert client.post("/chat/completions", json=_body(top_k=0)).status_code == 200
    assert m.calls[-1]["top_k"] == 0 and m.calls[-1]["spec_sample"] is True and m.calls[-1]["any_top_k"] is True and m.calls[-1]["prompt_lookup_num_tokens"] == 4
    assert client.post("/chat/completions", json=_body()).status_code == 200        # the default request: today's speculative call
    assert m.calls[-1]["top_k"] == 50 and m.calls[-1]["spec_sample"] is True and "any_top_k" not in m.calls[-1]
    m2 = _SoloModel(tok)
    client2 = TestClient(serving.create_app(m2, tok, model_name="stub", prompt_lookup_num_tokens=4, spec_sample=True))
    assert client2.post("/chat/completions", json=_body(top_k=0)).status_code == 200      # without the flag such a request does not speculate
    assert m2.calls[-1]["top_k"] == 0 and "spec_sample" not in m2.calls[-1] and "prompt_lookup_num_tokens" not in m2.calls[-1]


def test_endpoint_pure_top_p_request_reaches_the_flagged_batch_as_a_row():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    tok = _Tok()
    m = _Model(tok)
    m.llm = _AnyLlm(m.llm.reply)
    app = serving.create_app(m, tok, model_name="stub", batch_window_s=0.01, max_batch=4, batch_sampled=True, any_top_k=True)
    batcher = app.state.batcher
    try:
        assert isinstance(batcher, serving.ContinuousBatcher) and batcher.any_top_k and batcher.engine.batches_any_top_k
        r = TestClient(app).post("/chat/completions", json=_body(top_k=-1))
        assert r.status_code == 200, r.text
        assert m.llm.opened == [(True, True)]
        (slot, _, sampling), = m.llm.admitted
        assert sampling[0] == pytest.approx(0.2) and sampling[1] == 0 and sampling[2] == pytest.approx(0.9)
        assert not any(ev[0] == "solo" for ev in batcher.events) and m.solo_calls == 0
    finally:
        batcher.close()
    # without the flag the engine is opened as ever and such a request runs solo
    m2 = _Model(tok)
    app2 = serving.create_app(m2, tok, model_name="stub", batch_window_s=0.01, max_batch=4, batch_sampled=True)
    try:
        assert not app2.state.batcher.any_top_k
        r = TestClient(app2).post("/chat/completions", json=_body(top_k=0))
        assert r.status_code == 500 and m2.solo_calls == 1 and m2.llm.opened == []
    finally:
        app2.state.batcher.close()
