"""Batched decode past 2048 cached positions, the parts that need no GPU: the new C-ABI symbols are bound, `HipBatchEngine(max_ctx=)` reaches
`batch_open`, and a long prompt takes a row of a long-capacity engine while the default engine still serves it solo."""
from types import SimpleNamespace

import torch

from vila_amd import _lib, serving

NEW = ("vila_llm_decode_batch_workspace_bytes_ctx", "vila_llm_decode_batch_sample_workspace_bytes_ctx", "vila_llm_decode_batch_w4_workspace_bytes_ctx",
       "vila_llm_decode_batch_w4_sample_workspace_bytes_ctx", "vila_attn_decode_batch_workspace_bytes", "vila_attn_decode_batch_bf16",
       "vila_decode_batch_force_slices", "vila_decode_batch_slices")


def test_new_symbols_are_in_the_ctypes_table():
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
    for name in NEW[:4]:                                            # (shape, n, max_ctx) -> bytes, beside the unchanged (shape, n) functions
        res, args = _lib.PROTOTYPES[name]
        res0, args0 = _lib.PROTOTYPES[name[:-len("_ctx")]]
        assert res is res0 and args[:2] == args0 and len(args) == 3
    assert len(_lib.PROTOTYPES["vila_attn_decode_batch_bf16"][1]) == 16


class _Tok:
    eos_token_id = 1

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(i) for i in ids if not (skip_special_tokens and i == 1))


class _Llm:
    """The session interface `HipBatchEngine` drives, on the CPU: every live row replies 7, 8 and then EOS."""
    reply = [7, 8, 1]

    def __init__(self):
        self.opened, self.admitted, self._bdecode = [], [], None

    def batch_open(self, n_slots, max_ctx=2048, max_new_tokens=1024, sampling=False):
        self.opened.append(int(max_ctx))
        n = max(n_slots, 2)
        self._bdecode = SimpleNamespace(n_out=torch.zeros(n, dtype=torch.int32), out_ids=torch.zeros((n, max_new_tokens), dtype=torch.int64), live=set())
        return self._bdecode

    def batch_admit(self, st, slot, embeds, sampling=None):
        self.admitted.append((slot, int(embeds.shape[0])))
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


class _Engine(serving.HipBatchEngine):
    """HipBatchEngine with the tower and the solo path stubbed: a prompt is its token count."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.solos = []

    def embed(self, prompt, system):
        return torch.zeros((int(prompt), 8))

    def solo(self, prompt, max_new_tokens, system, streamer=None, **gen):
        self.solos.append(prompt)
        return f"solo {prompt}"


def _serve(engine, prompt, max_new):
    b = serving.ContinuousBatcher(engine, max_batch=4, chunk=4)
    try:
        return b.submit(prompt, max_new_tokens=max_new).result(timeout=30), list(b.events)
    finally:
        b.close()


def test_a_long_capacity_engine_batches_the_long_prompt_and_the_default_engine_serves_it_solo():
    model = SimpleNamespace(llm=_Llm(), cfg=None, device=torch.device("cpu"))
    eng = _Engine(model, _Tok(), n_slots=4, max_ctx=4096, max_new_tokens=64)
    assert eng.fits(2500, 64) and not eng.fits(4090, 64)
    text, events = _serve(eng, "2500", 64)
    assert model.llm.opened == [4096], "max_ctx did not reach batch_open"
    assert model.llm.admitted == [(0, 2500)] and text == "7 8" and not eng.solos
    assert any(ev[0] == "admit" for ev in events) and not any(ev[0] == "solo" for ev in events)
    # every default stays 2048: the same request does not fit and runs solo
    model2 = SimpleNamespace(llm=_Llm(), cfg=None, device=torch.device("cpu"))
    eng2 = _Engine(model2, _Tok(), n_slots=4, max_new_tokens=64)
    assert eng2.max_ctx == 2048 and not eng2.fits(2500, 64)
    text, events = _serve(eng2, "2500", 64)
    assert text == "solo 2500" and eng2.solos == ["2500"] and not model2.llm.admitted
    assert any(ev[0] == "solo" for ev in events) and not any(ev[0] == "admit" for ev in events)


def test_create_app_hands_max_ctx_to_the_engine_and_defaults_to_2048():
    import pytest
    pytest.importorskip("fastapi")
    model = SimpleNamespace(llm=SimpleNamespace(can_batch_decode_step=lambda: True), cfg=None, device=torch.device("cpu"))
    for kw, want in ((dict(max_ctx=4096), 4096), (dict(), 2048), (dict(max_ctx=8192, batch_sampled=True), 8192)):
        app = serving.create_app(model, _Tok(), model_name="stub", batch_window_s=0.01, max_batch=4, **kw)
        b = app.state.batcher
        try:
            assert isinstance(b, serving.ContinuousBatcher) and b.engine.max_ctx == want and b.engine.n_slots == 4
            assert b.engine.sampling == bool(kw.get("batch_sampled")) and b.engine.fits(2500, 64) == (want > 2048)
        finally:
            b.close()
