"""W4A16 batched decode without a GPU: the C-ABI surface (prototypes bound and declared) and the batcher choice of `serving.create_app`."""
import os
import re
from types import SimpleNamespace

from vila_amd import _lib, serving
from vila_amd.modules import HipQwen2ForCausalLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vila_gemv_w4_batch_bf16", "vila_llm_decode_batch_w4_workspace_bytes", "vila_llm_decode_step_batch_w4")


def test_batched_w4_prototypes_are_bound_and_declared():
    with open(os.path.join(ROOT, "include", "vila_hip.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
        assert re.search(r"\b" + name + r"\(", header), f"{name} is not declared in include/vila_hip.h"
    # the step takes the bf16 batched step's arguments plus the int4 layer table
    _, args = _lib.PROTOTYPES["vila_llm_decode_step_batch_w4"]
    _, bf16_args = _lib.PROTOTYPES["vila_llm_decode_step_batch"]
    assert args[0] == bf16_args[0] and args[1] == _lib.C.POINTER(_lib.VilaLlmLayerW4) and args[2:] == bf16_args[1:]


class _Llm:
    """Just the state `can_batch_decode_step` reads, with the model's own predicate."""
    can_batch_decode_step = HipQwen2ForCausalLM.can_batch_decode_step
    _w4_batched = HipQwen2ForCausalLM._w4_batched

    def __init__(self, head_dim=128, w4=None, w4_batch=False):
        self.lcfg = SimpleNamespace(head_dim=head_dim)
        self._w4, self._w4_batch = w4, w4_batch


def test_create_app_batcher_choice_follows_the_models_batched_step():
    w4 = object()
    assert serving.continuous_batching(SimpleNamespace(llm=_Llm()))                              # bf16
    assert serving.continuous_batching(SimpleNamespace(llm=_Llm(w4=w4, w4_batch=True)))          # quantize_w4(batch_decode=True)
    assert not serving.continuous_batching(SimpleNamespace(llm=_Llm(w4=w4)))                     # quantize_w4(): rows one at a time
    assert not serving.continuous_batching(SimpleNamespace(llm=_Llm(head_dim=64)))
    assert not serving.continuous_batching(SimpleNamespace(llm=None))
    assert not serving.continuous_batching(SimpleNamespace())


def test_create_app_picks_the_continuous_batcher_for_a_w4_batched_model(monkeypatch):
    import pytest
    pytest.importorskip("fastapi")
    made = []

    class _Engine:
        def __init__(self, model, tokenizer, n_slots=8):
            made.append(n_slots)

    class _Batcher:
        def __init__(self, *a, **k):
            self.model_lock = None

    monkeypatch.setattr(serving, "HipBatchEngine", _Engine)
    monkeypatch.setattr(serving, "ContinuousBatcher", type("ContinuousBatcher", (_Batcher,), {}))
    monkeypatch.setattr(serving, "RequestBatcher", type("RequestBatcher", (_Batcher,), {}))
    on = serving.create_app(SimpleNamespace(llm=_Llm(w4=object(), w4_batch=True)), None, batch_window_s=0.01, max_batch=4)
    assert isinstance(on.state.batcher, serving.ContinuousBatcher) and made == [4]
    off = serving.create_app(SimpleNamespace(llm=_Llm(w4=object())), None, batch_window_s=0.01, max_batch=4)
    assert isinstance(off.state.batcher, serving.RequestBatcher) and made == [4]
