"""Batched decode over a shared prompt prefix, the parts that need no GPU: the new C-ABI symbols and the VilaDecodePrefix layout, the names
`_step_symbols` composes, the batcher's sharing policy against a stub engine, and `create_app(share_prefix=)`."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest
import torch

from tests.test_serving_cpu import _StubEngine
from vila_amd import _lib, serving
from vila_amd.modules import _step_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = tuple("vila_llm_decode_step_batch_prefix" + t for t in ("", "_sample", "_w4", "_w4_sample"))
SIZES = tuple("vila_llm_decode_batch_prefix" + t + "_workspace_bytes" for t in ("", "_sample", "_w4", "_w4_sample"))


def test_new_symbols_are_in_the_ctypes_table():
    for name in STEPS + SIZES + ("vila_attn_decode_batch_prefix_bf16", "vila_attn_decode_batch_prefix_workspace_bytes"):
        assert name in _lib.PROTOTYPES, name
    for name in SIZES:                                              # (shape, n, max_ctx) -> bytes
        assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES["vila_llm_decode_batch_workspace_bytes_ctx"]
    for name, plain in zip(STEPS, ("vila_llm_decode_step_batch", "vila_llm_decode_step_batch_sample", "vila_llm_decode_step_batch_w4",
                                   "vila_llm_decode_step_batch_w4_sample")):
        res, args = _lib.PROTOTYPES[name]
        res0, args0 = _lib.PROTOTYPES[plain]
        at = args.index(C.POINTER(_lib.VilaDecodePrefix))           # the plain step's arguments with the descriptor behind the state
        assert res is res0 and args[:at] + args[at + 1:] == args0 and args[at - 1] is C.POINTER(_lib.VilaDecodeBatch)
    assert len(_lib.PROTOTYPES["vila_attn_decode_batch_prefix_bf16"][1]) == 21
    header = open(os.path.join(ROOT, "include", "vila_hip.h")).read()
    for name in STEPS + SIZES:
        assert name + "(" in header, f"{name} is not declared in include/vila_hip.h"


def test_step_symbols_compose_the_prefix_names():
    for w4 in (False, True):
        for sampled in (False, True):
            step, size = _step_symbols(True, w4, sampled, prefix=True)
            assert step in STEPS and size in SIZES and step in _lib.PROTOTYPES and size in _lib.PROTOTYPES
            assert ("_w4" in step) == w4 and step.endswith("_sample") == sampled
            assert _step_symbols(True, w4, sampled) == _step_symbols(True, w4, sampled, prefix=False)
    with pytest.raises(ValueError):
        _step_symbols(False, False, False, prefix=True)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_prefix_descriptor_layout_matches_the_header(tmp_path):
    cls = _lib.VilaDecodePrefix
    assert [f[0] for f in cls._fields_] == ["prefix_slot", "shared_len", "uses"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vila_hip.h"', "int main(void) {",
             '    printf("sizeof %zu\\n", sizeof(VilaDecodePrefix));']
    lines += [f'    printf("{f[0]} %zu\\n", offsetof(VilaDecodePrefix, {f[0]}));' for f in cls._fields_] + ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f in cls._fields_:
        assert int(got[f[0]]) == getattr(cls, f[0]).offset, f[0]


# ---- the batcher's policy ------------------------------------------------------------------------------------------------------------------
class _ShareEngine(_StubEngine):
    """_StubEngine with a prefix slot and slots of 4096 positions.  A request is "media:question:n" (media "" = none): it replies n tokens then EOS.
    `embed` stands for a tower run, `embed_tail` for the text-only embedding, `pin` for the prefill into the prefix slot; "badpin" / "badadmit" in the
    question make that call raise; media "tiny" is a prefix too short to pay, which `pin` declines; media "huge" is a prompt of 5000 positions."""
    shares_prefix = True
    max_ctx = 4096

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.pinned_key, self.admits, self.prepared = None, [], []

    @staticmethod
    def _parts(prompt):
        media, question, n = prompt.split(":")
        return media, question, int(n)

    def fits(self, n_prompt, max_new):
        return max_new <= 48 and n_prompt + max_new <= self.max_ctx

    def prepare(self, prompt, system):
        self.prepared.append(prompt)
        media = self._parts(prompt)[0]
        return SimpleNamespace(key=(media, system) if media else None, prompt=prompt)

    def embed(self, prompt, system, prep=None):
        self._mark("embed")
        media, _, n = self._parts(prompt)
        return SimpleNamespace(shape=(5000 if media == "huge" else 7,), script=[100 + i for i in range(n)] + [1] + [55] * 64, prompt=prompt)

    def pin(self, e, prep):
        self._mark("pin")
        assert e.shape[0] + 1 <= self.max_ctx, "a prompt that fits no slot reached the prefix slot"
        if prep.prompt.startswith("tiny:"):
            return False
        self.pinned_key = None
        if "badpin" in prep.prompt:
            raise RuntimeError("the prefix prefill failed")
        self.pinned_key = prep.key
        return True

    def embed_tail(self, prep):
        self._mark("embed_tail")
        assert prep.key == self.pinned_key, "a tail was embedded against another prefix"
        n = self._parts(prep.prompt)[2]
        return SimpleNamespace(shape=(7,), script=[100 + i for i in range(n)] + [1] + [55] * 64, prompt=prep.prompt), 256

    def admit(self, slot, e, sampling=None, share=False, first_row=0):
        if "badadmit" in e.prompt:
            raise RuntimeError("the prefill failed")
        if share:
            assert (self._parts(e.prompt)[0], None) == self.pinned_key, "a row shares a prefix that is not the pinned one"
        self.admits.append((e.prompt, slot, bool(share), first_row))
        return super().admit(slot, e)

    def solo(self, prompt, max_new_tokens, system, **gen):
        self._mark("solo")
        return f"solo {prompt}"


def _batcher(eng, **kw):
    return serving.ContinuousBatcher(eng, max_batch=4, chunk=1, share_prefix=True, **kw)


def test_share_prefix_is_off_by_default_and_needs_an_engine_that_shares():
    b = serving.ContinuousBatcher(_ShareEngine(), max_batch=4)
    try:
        assert b.share_prefix is False
        assert b.submit("v1:q:2", max_new_tokens=8).result(timeout=30) == "100 101"
        assert b.engine.calls.count("embed") == 1 and "pin" not in b.engine.calls and b.engine.admits == [("v1:q:2", 0, False, 0)]
        assert not b.engine.prepared
    finally:
        b.close()
    b = serving.ContinuousBatcher(_StubEngine(), max_batch=4, share_prefix=True)      # an engine without a prefix slot
    try:
        assert b.share_prefix is False and b.submit("a:2", max_new_tokens=8).result(timeout=30) == "100 101"
    finally:
        b.close()


def test_same_key_requests_share_and_skip_the_tower():
    eng = _ShareEngine(step_sleep=0.002)
    b = _batcher(eng)
    try:
        prompts = ("v1:what:30", "v1:who:3", "v1:where:2", ":no media:2")
        futs = [b.submit(p, max_new_tokens=48) for p in prompts]
        assert [f.result(timeout=30) for f in futs] == [" ".join(str(100 + i) for i in range(n)) for n in (30, 3, 2, 2)]
    finally:
        b.close()
    assert eng.calls.count("pin") == 1 and eng.calls.count("embed_tail") == 2
    assert eng.calls.count("embed") == 2, "the pinning request and the one without media are embedded whole; the sharers skip the tower"
    assert eng.prepared == list(prompts), "a request's media is prepared once"
    assert [(p, s, f) for p, _, s, f in eng.admits] == [("v1:what:30", True, 0), ("v1:who:3", True, 256), ("v1:where:2", True, 256), (":no media:2", False, 0)]
    kinds = [ev[0] for ev in b.events if ev[0] in ("pin", "share")]
    assert kinds == ["pin", "share", "share"] and b._pin_rows == set()


def test_another_key_takes_an_ordinary_row_and_the_pin_moves_once_the_sharers_retired():
    eng = _ShareEngine(step_sleep=0.002)
    b = _batcher(eng)
    try:
        a = b.submit("v1:long:40", max_new_tokens=48)
        other = b.submit("v2:q:2", max_new_tokens=48)                  # arrives while the v1 row lives: ordinary, and it does not wait
        assert other.result(timeout=30) == "100 101"
        assert not a.done(), "the request with another key waited for the sharer"
        assert eng.admits[1] == ("v2:q:2", 1, False, 0) and eng.calls.count("pin") == 1 and eng.pinned_key == ("v1", None)
        a.result(timeout=30)
        assert b.submit("v2:again:2", max_new_tokens=48).result(timeout=30) == "100 101"      # no sharer lives: the pin moves
        assert eng.pinned_key == ("v2", None) and eng.calls.count("pin") == 2 and eng.admits[-1][2] is True
        assert b.submit("v2:third:2", max_new_tokens=48).result(timeout=30) == "100 101"
        assert eng.calls.count("pin") == 2 and eng.calls.count("embed_tail") == 1
    finally:
        b.close()


def test_a_failed_admission_returns_the_slot_and_keeps_the_pin_consistent():
    eng = _ShareEngine()
    b = _batcher(eng)
    try:
        with pytest.raises(RuntimeError, match="the prefill failed"):
            b.submit("v1:badadmit:3", max_new_tokens=8).result(timeout=30)           # pinned, then the admission failed
        assert b._pin_rows == set() and eng.pinned_key == ("v1", None)
        assert b.submit("v1:q:2", max_new_tokens=8).result(timeout=30) == "100 101"    # the pin is valid: this one shares
        assert eng.admits[-1][0] == "v1:q:2" and eng.admits[-1][2:] == (True, 256)
        with pytest.raises(RuntimeError, match="prefix prefill failed"):
            b.submit("v3:badpin:3", max_new_tokens=8).result(timeout=30)             # the pin itself failed: no prefix is left
        assert b._pin_rows == set() and eng.pinned_key is None
        assert b.submit("v1:q:2", max_new_tokens=8).result(timeout=30) == "100 101"    # pins anew instead of sharing what is gone
        assert eng.calls.count("pin") == 3 and eng.admits[-1][0] == "v1:q:2" and eng.admits[-1][2:] == (True, 0)
        failed = [ev[1] for ev in b.events if ev[0] == "admit_failed"]
        for _ in range(3):                                                             # the slot of the failed admission serves again
            assert b.submit("v1:q:2", max_new_tokens=8).result(timeout=30) == "100 101"
        assert len(failed) == 1 and failed[0] in {slot for _, slot, _, _ in eng.admits}
    finally:
        b.close()


def test_a_prefix_too_short_to_pay_takes_ordinary_rows_and_leaves_the_pin_alone():
    eng = _ShareEngine()
    b = _batcher(eng)
    try:
        assert b.submit("v1:q:2", max_new_tokens=8).result(timeout=30) == "100 101"
        assert b.submit("tiny:q:2", max_new_tokens=8).result(timeout=30) == "100 101"     # no sharer lives, yet nothing is pinned for it
        assert eng.admits[-1][2:] == (False, 0) and eng.pinned_key == ("v1", None)
        assert b.submit("v1:again:2", max_new_tokens=8).result(timeout=30) == "100 101"   # the old prefix still serves
        assert eng.admits[-1][2:] == (True, 256) and [ev[0] for ev in b.events if ev[0] in ("pin", "share")] == ["pin", "share"]
    finally:
        b.close()


def test_a_pin_candidate_that_does_not_fit_runs_solo_and_leaves_the_pin_alone():
    """Fit is decided before anything is pinned: a media request too long for a slot, or one whose reply would not fit behind it, runs solo as it
    does without the flag, and the prefix the engine holds stays."""
    eng = _ShareEngine()
    b = _batcher(eng)
    try:
        assert b.submit("v1:q:2", max_new_tokens=8).result(timeout=30) == "100 101"
        assert b.submit("huge:q:2", max_new_tokens=8).result(timeout=30) == "solo huge:q:2"     # 5000 positions: no slot holds it
        assert b.submit("v2:q:2", max_new_tokens=64).result(timeout=30) == "solo v2:q:2"        # the reply does not fit (the stub's 48)
        assert eng.calls.count("pin") == 1 and eng.pinned_key == ("v1", None) and len(eng.admits) == 1
        assert [ev[0] for ev in b.events if ev[0] in ("pin", "share", "solo", "admit_failed")] == ["pin", "solo", "solo"]
        assert b.submit("v1:again:2", max_new_tokens=8).result(timeout=30) == "100 101" and eng.admits[-1][2:] == (True, 256)
    finally:
        b.close()


# ---- HipBatchEngine's side of it, on a stub llm ------------------------------------------------------------------------------------------------
class _Tok:
    eos_token_id = 1

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(i) for i in ids if not (skip_special_tokens and i == 1))


class _Llm:
    """The session interface `HipBatchEngine` drives, on the CPU: every live row replies 7 and then EOS.  `batch_set_prefix` refuses what the real one
    refuses: a prompt that does not fit the prefix slot."""

    def __init__(self):
        self.opened, self.prefixes, self.admitted, self._bdecode = [], [], [], None

    def batch_open(self, n_slots, max_ctx=2048, max_new_tokens=1024, **kw):
        self.opened.append((int(max_ctx), kw))
        n = max(n_slots, 2)
        self._bdecode = SimpleNamespace(n_out=torch.zeros(n, dtype=torch.int32), out_ids=torch.ones((n, max_new_tokens), dtype=torch.int64), max_ctx=int(max_ctx))
        return self._bdecode

    def batch_set_prefix(self, st, embeds, prefix_len=None):
        if int(embeds.shape[0]) + 1 > st.max_ctx:
            raise ValueError("batch_set_prefix: embeds must fit the slot")
        self.prefixes.append((int(embeds.shape[0]), prefix_len))
        return prefix_len // 256 * 256

    def batch_admit(self, st, slot, embeds, **kw):
        self.admitted.append((slot, int(embeds.shape[0]), kw))
        st.n_out[slot] = 0
        return 7

    def batch_run(self, st, k):
        st.n_out += k

    def batch_release(self, st, slots):
        for b in slots:
            st.n_out[b] = 0

    def embed_tokens(self, ids):
        return torch.zeros((ids.shape[0], ids.shape[1], 8))


class _Engine(serving.HipBatchEngine):
    """HipBatchEngine with the media, the tokenizer and the tower stubbed: a prompt is "media:prefix rows:tail tokens"."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.solos, self.towers = [], 0

    def prepare(self, prompt, system):
        media, rows, tail = prompt.split(":")
        return SimpleNamespace(ids=torch.arange(int(tail) + 3), tiles=[], media_config=None, key=(media,) if media else None, n_tail=int(tail), rows=int(rows))

    def embed(self, prompt, system, prep=None):
        self.towers += 1
        prep = prep or self.prepare(prompt, system)
        return torch.zeros((prep.rows + prep.n_tail, 8))

    def solo(self, prompt, max_new_tokens, system, streamer=None, **gen):
        self.solos.append(prompt)
        return f"solo {prompt}"


def _engine(**kw):
    model = SimpleNamespace(llm=_Llm(), cfg=None, device=torch.device("cpu"))
    return _Engine(model, _Tok(), n_slots=4, max_new_tokens=64, share_prefix=True, **kw), model.llm


def test_engine_pins_shares_and_never_sends_to_the_prefix_slot_what_does_not_fit():
    eng, llm = _engine(max_ctx=4096)
    b = serving.ContinuousBatcher(eng, max_batch=4, chunk=4, share_prefix=True)
    try:
        assert b.submit("doc:2400:20", max_new_tokens=8).result(timeout=30) == "7"
        assert llm.prefixes == [(2420, 2400)] and llm.admitted[-1] == (0, 2420, dict(share=True, first_row=0)) and eng.pinned_key == ("doc",)
        assert b.submit("doc:2400:30", max_new_tokens=8).result(timeout=30) == "7"        # the sharer: rows 2304 .. 2399 of the prefix and its 30 tokens
        assert llm.admitted[-1][1:] == (96 + 30, dict(share=True, first_row=2304)) and eng.towers == 1 and len(llm.prefixes) == 1
        assert b.submit("video:5000:20", max_new_tokens=8).result(timeout=30) == "solo video:5000:20"      # fits no slot: solo, no exception
        assert b.submit("scan:4060:20", max_new_tokens=64).result(timeout=30) == "solo scan:4060:20"       # fits, but not with its reply: solo
        assert b.submit("tile:256:20", max_new_tokens=8).result(timeout=30) == "7"                         # below min_shared_len: an ordinary row
        assert llm.admitted[-1][1:] == (276, {}) and len(llm.prefixes) == 1 and eng.pinned_key == ("doc",)
        assert not any(ev[0] == "admit_failed" for ev in b.events)
        # the llm drops the session (weights re-quantised, another batch_open): the engine holds no prefix any more, and the same key pins anew
        llm._bdecode = None
        assert eng.pinned_key is None
        assert b.submit("doc:2400:30", max_new_tokens=8).result(timeout=30) == "7"
        assert len(llm.opened) == 2 and llm.prefixes[-1] == (2430, 2400) and llm.admitted[-1][2] == dict(share=True, first_row=0)
    finally:
        b.close()


def test_engine_refuses_a_capacity_that_can_never_share_and_opens_a_prefix_slot_only_when_asked():
    model = SimpleNamespace(llm=_Llm(), cfg=None, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="min_shared_len"):
        serving.HipBatchEngine(model, _Tok(), n_slots=4, share_prefix=True)                       # max_ctx 2048 against min_shared_len 2048
    with pytest.raises(ValueError, match="min_shared_len"):
        serving.HipBatchEngine(model, _Tok(), n_slots=4, share_prefix=True, max_ctx=1024, min_shared_len=1024)
    for kw, want in ((dict(), {}), (dict(share_prefix=True, max_ctx=4096), dict(shared_prefix=True)), (dict(share_prefix=True, min_shared_len=512), dict(shared_prefix=True)),
                     (dict(share_prefix=True, sampling=True, max_ctx=8192), dict(sampling=True, shared_prefix=True))):
        eng = serving.HipBatchEngine(model, _Tok(), n_slots=4, **kw)
        assert eng.shares_prefix == bool(kw.get("share_prefix"))
        eng._session()
        assert model.llm.opened[-1] == (kw.get("max_ctx", 2048), want)


def test_create_app_hands_share_prefix_through_and_defaults_to_off():
    pytest.importorskip("fastapi")
    model = SimpleNamespace(llm=SimpleNamespace(can_batch_decode_step=lambda: True), cfg=None, device=torch.device("cpu"))
    for kw, want in ((dict(), False), (dict(share_prefix=True, max_ctx=4096), True), (dict(share_prefix=True, batch_sampled=True, max_ctx=8192), True)):
        app = serving.create_app(model, _Tok(), model_name="stub", batch_window_s=0.01, max_batch=4, **kw)
        b = app.state.batcher
        try:
            assert isinstance(b, serving.ContinuousBatcher)
            assert b.share_prefix is want and b.engine.share_prefix is want and b.engine.shares_prefix is want
            assert b.engine.sampling == bool(kw.get("batch_sampled")) and b.engine.max_ctx == kw.get("max_ctx", 2048)
        finally:
            b.close()
    with pytest.raises(ValueError, match="min_shared_len"):                                       # the default capacity can never share
        serving.create_app(model, _Tok(), model_name="stub", batch_window_s=0.01, max_batch=4, share_prefix=True)
