"""Host logic of the decode drivers in vila_amd/modules.py: the step table, the row finisher, the pad rule, the order of a graph capture, the
choice of a one-sequence generate()'s KV cache and the replay loop."""
import contextlib
import itertools
from types import SimpleNamespace

import pytest
import torch

from vila_amd import _lib, modules
from vila_amd.modules import HipQwen2ForCausalLM, _capture, _eos_set, _pad_id, _replay, _step_symbols, finish_rows


def test_step_table_names_exist_in_the_abi():
    combos = list(itertools.product((False, True), repeat=3))
    assert len(combos) == 8
    steps = set()
    for batch, w4, sampled in combos:
        step, ws = _step_symbols(batch, w4, sampled)
        assert step in _lib.PROTOTYPES, step
        assert ws in _lib.PROTOTYPES, ws
        # the step takes the int4 layers / the sampling struct exactly when its name says so
        n_args = 6 + int(w4) + int(sampled)
        assert len(_lib.PROTOTYPES[step][1]) == n_args, step
        assert ("_batch" in step) == batch and ("_w4" in step) == w4 and step.endswith("_sample") == sampled
        if batch:
            assert ws.endswith("_workspace_bytes_ctx") and ("_w4" in ws) == w4 and ("_sample" in ws) == sampled
        else:
            assert ws == "vila_llm_decode_workspace_bytes"
        steps.add(step)
    assert len(steps) == 8
    for w4 in (False, True):
        step, ws = _step_symbols(True, w4, False, verify=True)
        assert step == "vila_llm_decode_step_verify" + ("_w4" if w4 else "") and ws == "vila_llm_decode_verify_workspace_bytes"
        assert step in _lib.PROTOTYPES and ws in _lib.PROTOTYPES
        assert len(_lib.PROTOTYPES[step][1]) == 6 + int(w4), step
        assert _step_symbols(False, w4, False, verify=True) == (step, ws)          # one sequence's rows: `batch` is not read
        with pytest.raises(ValueError, match="verify step is greedy"):
            _step_symbols(True, w4, True, verify=True)
        steps.add(step)
    assert len(steps) == 10


def test_cache_for_keeps_grows_and_refuses():
    made = []
    llm = SimpleNamespace(_own_cache=None)
    llm.new_cache = lambda max_ctx: made.append(max_ctx) or SimpleNamespace(max_ctx=max_ctx)
    cache_for = lambda *a: HipQwen2ForCausalLM._cache_for(llm, *a)
    c = cache_for(20, 6, None)
    assert made == [256] and c.max_ctx == 256 and llm._own_cache is c
    assert cache_for(100, 156, None) is c and made == [256]          # fits exactly: reused
    c2 = cache_for(250, 10, None)
    assert made == [256, 512] and c2.max_ctx == 512 and llm._own_cache is c2
    assert cache_for(20, 6, None) is c2 and made == [256, 512]       # a larger cache is kept, never shrunk
    mine = SimpleNamespace(max_ctx=24)
    with pytest.raises(ValueError, match=r"KV cache too small: 24 < 20 \+ 6"):
        cache_for(20, 6, mine)
    assert cache_for(20, 4, mine) is mine and llm._own_cache is c2 and made == [256, 512]


def test_replay_launches_k_times_and_raises_through_check(monkeypatch):
    calls = []

    class Lib:
        rc = 0

        def vila_graph_launch(self, graph, stream):
            calls.append((graph, stream))
            return self.rc

        def vila_last_error(self):
            return b"launch refused"

    lib = Lib()
    monkeypatch.setattr(modules._lib, "load", lambda *a, **k: lib)
    st = SimpleNamespace(graph="the graph", stream=SimpleNamespace(cuda_stream=1234))
    _replay(st, 3)
    assert calls == [("the graph", 1234)] * 3
    _replay(st, 0)
    assert len(calls) == 3
    lib.rc = 1
    with pytest.raises(_lib.VilaHipError, match="graph_launch: launch refused"):
        _replay(st, 3)
    assert len(calls) == 4, "the first failure ends the loop"


def test_finish_rows_cuts_after_the_first_eos_and_right_pads():
    rows = [[5, 6, 2, 7, 8],        # EOS in the middle: kept, the rest dropped
            [2, 9, 9, 9, 9],        # EOS first
            [4, 4, 4, 4, 4]]        # no EOS
    out = finish_rows(rows, {2}, 0, "cpu")
    assert out.dtype == torch.int64
    assert torch.equal(out, torch.tensor([[5, 6, 2, 0, 0], [2, 0, 0, 0, 0], [4, 4, 4, 4, 4]]))
    # two EOS ids given as a list; every row ends early, so the result is as wide as the longest cut row
    out = finish_rows([[1, 3, 5, 5], [7, 1, 2, 1], [9, 9, 9, 9]], _eos_set([2, 3]), 11, "cpu")
    assert torch.equal(out, torch.tensor([[1, 3, 11, 11], [7, 1, 2, 11], [9, 9, 9, 9]]))
    out = finish_rows([[1, 3, 5, 5], [7, 2, 2, 1]], _eos_set([2, 3]), 11, "cpu")
    assert torch.equal(out, torch.tensor([[1, 3], [7, 2]]))
    out = finish_rows([[3, 1, 1], [2, 1, 1]], _eos_set((2, 3)), 11, "cpu")
    assert torch.equal(out, torch.tensor([[3], [2]]))
    assert rows[0] == [5, 6, 2, 7, 8], "the caller's lists are left alone"


def test_eos_set_falls_back_to_the_default():
    assert _eos_set(None, 151645) == {151645}
    assert _eos_set(7, 151645) == {7}
    assert _eos_set([7, 8], 151645) == {7, 8}
    assert _eos_set((7,)) == {7}
    assert _eos_set(-1) == {-1}


def test_pad_rule():
    assert _pad_id(3, [7, 8], 99) == 3              # pad_token_id wins, also when it is 0
    assert _pad_id(0, 7, 99) == 0
    assert _pad_id(None, [7, 8], 99) == 7           # else the first EOS given
    assert _pad_id(None, 8, 99) == 8
    assert _pad_id(None, None, 99) == 99            # else the config's EOS


def test_capture_order(monkeypatch):
    calls = []

    class Stream:
        cuda_stream = 1234

        def __init__(self, name):
            self.name = name

        def synchronize(self):
            calls.append(f"sync {self.name}")

    class Lib:
        def vila_graph_begin(self, stream):
            calls.append(("begin", stream))
            return 0

        def vila_graph_end(self, stream, out):
            calls.append(("end", stream))
            out._obj.value = 77
            return 0

    @contextlib.contextmanager
    def on_stream(s):
        calls.append(f"enter {s.name}")
        yield
        calls.append(f"exit {s.name}")

    monkeypatch.setattr(modules._lib, "load", lambda *a, **k: Lib())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: Stream("current"))
    monkeypatch.setattr(torch.cuda, "stream", on_stream)
    st = SimpleNamespace(stream=Stream("session"), graph=None)
    _capture(st, lambda: calls.append("step"), lambda: calls.append("restore"))
    assert calls == ["sync current", "enter session", "step", "sync session", "restore", ("begin", 1234), "step", ("end", 1234),
                     "sync session", "exit session"]
    assert [c for c in calls if c in ("step", "restore") or isinstance(c, tuple)] == ["step", "restore", ("begin", 1234), "step", ("end", 1234)]
    assert st.graph is not None and st.graph.value == 77
