"""Per-row sampling in the batched decode step, the parts that need no GPU: the C ABI (header == ctypes mirror, every new symbol declared
and bound), the continuous batcher admitting sampled requests into rows (`ContinuousBatcher(batch_sampled=True)`), and the endpoint's
default request (temperature 0.2 / top_p 0.9) reaching the batch as a row (`create_app(batch_sampled=True)`)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import time
from types import SimpleNamespace

import pytest
import torch

from vila_amd import _lib, configs, serving

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vila_sample_batch_workspace_bytes", "vila_sample_batch_f32", "vila_llm_decode_batch_sample_workspace_bytes",
       "vila_llm_decode_step_batch_sample", "vila_llm_decode_batch_w4_sample_workspace_bytes", "vila_llm_decode_step_batch_w4_sample")


# ----------------------------------------------------------------------------------------------------------------------
# C ABI
# ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_in_the_header_and_bound():
    header = open(os.path.join(ROOT, "include", "vila_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), f"{name} is not declared in include/vila_hip.h"
        assert name in _lib.PROTOTYPES, f"{name} has no PROTOTYPES entry in vila_amd/_lib.py"
    # the sampled steps take the greedy steps' arguments plus the sampling struct in front of the stream
    for plain, sampled in (("vila_llm_decode_step_batch", "vila_llm_decode_step_batch_sample"),
                           ("vila_llm_decode_step_batch_w4", "vila_llm_decode_step_batch_w4_sample")):
        _, a = _lib.PROTOTYPES[plain]
        _, b = _lib.PROTOTYPES[sampled]
        assert b == a[:-1] + [C.POINTER(_lib.VilaBatchSampling), a[-1]]
    assert _lib.PROTOTYPES["vila_sample_batch_workspace_bytes"] == (C.c_size_t, [C.c_int])
    assert len(_lib.PROTOTYPES["vila_sample_batch_f32"][1]) == 10


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_batch_sampling_struct_has_the_header_layout(tmp_path):
    cls = _lib.VilaBatchSampling
    assert [f[0] for f in cls._fields_] == ["temperature", "top_k", "top_p", "seed"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vila_hip.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(VilaBatchSampling));']
    for f in cls._fields_:
        lines.append(f'    printf("{f[0]} %zu\\n", offsetof(VilaBatchSampling, {f[0]}));')
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, "include/vila_hip.h must compile as C99 with VilaBatchSampling:\n" + r.stderr
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]


# ----------------------------------------------------------------------------------------------------------------------
# the batcher over a stub engine that records admit(slot, e, sampling)
# ----------------------------------------------------------------------------------------------------------------------
class _Engine:
    """`HipBatchEngine(sampling=True)` minus the GPU: a request "name:n" replies tokens 100+i (i < n) then EOS; every slot advances on every step."""
    eos = {1}
    batches_sampled = True

    def __init__(self, n_slots=4, step_sleep=0.0):
        self.n_slots, self.step_sleep = n_slots, step_sleep
        self.script = {b: None for b in range(n_slots)}
        self.n_out = [0] * n_slots
        self.out = [[] for _ in range(n_slots)]
        self.admitted, self.solos, self.seeds = [], [], 0

    def fresh_seed(self):
        self.seeds += 1
        return 1000 + self.seeds

    def embed(self, prompt, system):
        n = int(prompt.split(":")[1])
        return SimpleNamespace(shape=(7,), name=prompt, script=[100 + i for i in range(n)] + [1] + [55] * 64)

    def fits(self, n_prompt, max_new):
        return max_new <= 48

    def admit(self, slot, e, sampling=None):
        self.admitted.append((e.name, slot, sampling))
        self.script[slot], self.n_out[slot], self.out[slot] = e.script, 0, []
        return e.script[0]

    def run(self, k):
        for _ in range(k):
            time.sleep(self.step_sleep)
            for b in range(self.n_slots):
                sc = self.script[b]
                self.out[b].append(sc[1 + self.n_out[b]] if sc is not None else 7)
                self.n_out[b] += 1

    def read(self):
        top = max(max(self.n_out), 1)
        return list(self.n_out), [r[:top] + [0] * (top - len(r)) for r in self.out]

    def release(self, slots):
        for b in slots:
            self.n_out[b], self.out[b], self.script[b] = 0, [], None

    def solo(self, prompt, max_new_tokens, system, **gen):
        self.solos.append((prompt, gen))
        return f"solo {prompt}"

    def decode(self, toks):
        return " ".join(str(t) for t in toks)


def _want(n):
    return " ".join(str(100 + i) for i in range(n))


def test_batcher_admits_a_sampled_request_beside_a_live_greedy_row():
    eng = _Engine(n_slots=4, step_sleep=0.002)
    b = serving.ContinuousBatcher(eng, max_batch=4, chunk=4, batch_sampled=True)
    assert b.batch_sampled
    try:
        fa = b.submit("A:40", 48)                                      # greedy, long
        while not any(ev[0] == "run" for ev in b.events):
            time.sleep(0.001)
        fs = b.submit("S:5", 48, temperature=0.7, top_p=0.8)           # sampled, arrives while A is mid-reply
        assert fs.result(timeout=30) == _want(5) and fa.result(timeout=30) == _want(40)
        admits = [ev for ev in b.events if ev[0] == "admit"]
        assert len(admits) == 2 and admits[1][2] > 0 and admits[1][3] >= 1, admits      # S joined after steps had run, beside a live row
        assert not any(ev[0] == "solo" for ev in b.events) and not eng.solos
        assert eng.admitted[0] == ("A:40", admits[0][1], None)
        name, slot, sampling = eng.admitted[1]
        assert name == "S:5" and slot == admits[1][1]
        assert sampling[:3] == (0.7, 50, 0.8) and isinstance(sampling[3], int)          # HF's default top_k, a derived seed
        # two seedless requests get different seeds; an explicit seed is handed on as it is; top_k travels
        f1 = b.submit("P:3", 48, temperature=0.2, top_p=0.9)
        f2 = b.submit("Q:3", 48, temperature=0.2, top_p=0.9)
        f3 = b.submit("R:3", 48, temperature=0.5, top_p=0.9, top_k=20, seed=77)
        assert [f.result(timeout=30) for f in (f1, f2, f3)] == [_want(3)] * 3
        got = {n: sp for n, _, sp in eng.admitted}
        assert got["P:3"][:3] == (0.2, 50, 0.9) and got["Q:3"][:3] == (0.2, 50, 0.9) and got["P:3"][3] != got["Q:3"][3]
        assert len({got["S:5"][3], got["P:3"][3], got["Q:3"][3]}) == 3
        assert got["R:3"] == (0.5, 20, 0.9, 77)
        assert not eng.solos
        # what the batched sampler does not serve stays solo, in arrival order
        g0 = b.submit("G:12", 48)
        s0 = b.submit("K0:4", 16, temperature=0.7, top_k=0)
        s1 = b.submit("K100:4", 16, temperature=0.7, top_k=100)
        g1 = b.submit("H:4", 48, temperature=0.7, top_k=64)
        assert s0.result(timeout=30) == "solo K0:4" and s1.result(timeout=30) == "solo K100:4"
        assert g0.result(timeout=30) == _want(12) and g1.result(timeout=30) == _want(4)
        assert [p for p, _ in eng.solos] == ["K0:4", "K100:4"]
        assert eng.solos[0][1]["top_k"] == 0 and eng.solos[1][1]["top_k"] == 100 and eng.solos[0][1]["temperature"] == 0.7
        order = [n for n, _, _ in eng.admitted]
        assert order.index("G:12") < order.index("H:4")
        assert dict((n, sp) for n, _, sp in eng.admitted)["H:4"][:3] == (0.7, 64, 1.0)
    finally:
        b.close()


def test_batcher_without_the_switch_keeps_sampled_requests_solo():
    eng = _Engine(n_slots=4)
    b = serving.ContinuousBatcher(eng, max_batch=4, chunk=4)          # batch_sampled defaults to False
    assert not b.batch_sampled
    try:
        assert b.submit("S:5", 48, temperature=0.7, top_p=0.8).result(timeout=30) == "solo S:5"
        assert b.submit("A:6", 48).result(timeout=30) == _want(6)
        assert [ev[0] for ev in b.events if ev[0] in ("solo", "admit")] == ["solo", "admit"]
        assert eng.admitted == [("A:6", 0, None)] and eng.solos[0][1]["temperature"] == 0.7
    finally:
        b.close()
    # an engine that does not say it batches sampled rows: the switch stays off whatever the caller asks
    eng2 = _Engine(n_slots=2)
    eng2.batches_sampled = False
    b2 = serving.ContinuousBatcher(eng2, max_batch=2, batch_sampled=True)
    try:
        assert not b2.batch_sampled
        assert b2.submit("S:5", 48, temperature=0.7).result(timeout=30) == "solo S:5"
    finally:
        b2.close()


# ----------------------------------------------------------------------------------------------------------------------
# the endpoint: the default request becomes a row
# ----------------------------------------------------------------------------------------------------------------------
class _Tok:
    eos_token_id = 1

    def __init__(self):
        self.vocab, self.inv = {"<eos>": 1}, {1: "<eos>"}

    def __call__(self, text, add_special_tokens=False):
        ids = []
        for w in text.split():
            if w not in self.vocab:
                self.vocab[w] = len(self.vocab) + 2
                self.inv[self.vocab[w]] = w
            ids.append(self.vocab[w])
        return SimpleNamespace(input_ids=ids)

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(self.inv[i] for i in ids if not (skip_special_tokens and i == 1))


class _Llm:
    """The session interface `HipBatchEngine` drives, on the CPU: every live row replies "a red square" then EOS."""

    def __init__(self, reply):
        self.reply, self.opened, self.admitted, self._bdecode, self._calls = reply, [], [], None, 0

    def can_batch_decode_step(self):
        return True

    def _fresh_seed(self):
        self._calls += 1
        return 5000 + self._calls

    def batch_open(self, n_slots, max_ctx=2048, max_new_tokens=1024, sampling=False):
        self.opened.append(bool(sampling))
        n = max(n_slots, 2)
        self._bdecode = SimpleNamespace(n_out=torch.zeros(n, dtype=torch.int32), out_ids=torch.zeros((n, max_new_tokens), dtype=torch.int64), live=set())
        return self._bdecode

    def batch_admit(self, st, slot, embeds, sampling=None):
        self.admitted.append((slot, int(embeds.shape[0]), sampling))
        st.n_out[slot] = 0
        st.live.add(slot)
        return self.reply[0]

    def batch_run(self, st, k):
        for _ in range(k):
            for b in range(st.n_out.numel()):
                i = int(st.n_out[b])
                st.out_ids[b, i] = self.reply[1 + i] if (b in st.live and 1 + i < len(self.reply)) else 1
                st.n_out[b] += 1

    def batch_release(self, st, slots):
        for b in slots:
            st.n_out[b] = 0
            st.live.discard(b)


class _Model:
    def __init__(self, tok):
        self.cfg, self.device = configs.tiny(), torch.device("cpu")
        self.llm = _Llm(tok("a red square").input_ids + [1])
        self.solo_calls = 0

    def _embed(self, ids, media, media_config):
        return torch.zeros((1, ids.shape[1], 8)), None, None

    def generate(self, *a, **k):
        self.solo_calls += 1
        raise AssertionError("the request must not run solo")


def test_endpoint_default_request_reaches_the_batch_as_a_row():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    tok = _Tok()
    m = _Model(tok)
    app = serving.create_app(m, tok, model_name="stub", batch_window_s=0.01, max_batch=4, batch_sampled=True)
    batcher = app.state.batcher
    assert isinstance(batcher, serving.ContinuousBatcher) and batcher.batch_sampled and batcher.engine.batches_sampled
    try:
        client = TestClient(app)
        body = {"model": "stub", "max_tokens": 8, "messages": [{"role": "user", "content": "what is this ?"}]}       # no temperature field
        r = client.post("/chat/completions", json=body)
        assert r.status_code == 200, r.text
        assert r.json()["choices"][0]["message"]["content"][0]["text"] == "a red square"
        assert m.llm.opened == [True]                                  # the session was opened with per-row sampling
        (slot, _, sampling), = m.llm.admitted
        assert sampling[0] == pytest.approx(0.2) and sampling[1] == 50 and sampling[2] == pytest.approx(0.9) and sampling[3] == 5001
        assert not any(ev[0] == "solo" for ev in batcher.events) and any(ev[0] == "admit" for ev in batcher.events)
        # an explicit temperature 0 is a greedy row of the same session
        r = client.post("/chat/completions", json=dict(body, temperature=0))
        assert r.status_code == 200 and m.llm.admitted[1][2] is None and m.solo_calls == 0
    finally:
        batcher.close()
    # without the switch the app is what it was: a greedy session, the default request solo
    m2 = _Model(tok)
    app2 = serving.create_app(m2, tok, model_name="stub", batch_window_s=0.01, max_batch=4)
    try:
        assert not app2.state.batcher.batch_sampled and not app2.state.batcher.engine.batches_sampled
        r = TestClient(app2).post("/chat/completions", json=body)
        assert r.status_code == 500 and m2.solo_calls == 1 and any(ev[0] == "solo" for ev in app2.state.batcher.events)
    finally:
        app2.state.batcher.close()
