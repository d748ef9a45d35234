"""Prefill onto a live KV cache, the parts that need no GPU.

  * ABI: the new entries stand in include/vila_hip.h and in _lib.PROTOTYPES with the same number of arguments.
  * The planted-key inputs of tests/test_gpu_append_prefill.py (`append_probes`: the GPU test runs exactly these) and the proof, in the manner of
    tests/test_decode_probe_cpu.py, that each discriminates: the fp32 reference over the right key set and over the set with the probed key dropped
    (inside) or the next one admitted (outside) differ on every target head by at least 8 x the GPU test's bound.
  * `serving.ChatSession`'s bookkeeping against a fake model that records what `llm.generate` is handed and answers with scripted ids.
  * The argument errors of `generate(past_len=, prefill_chunk=)`, raised before anything touches a device."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests.gpu_util import plant_keys, probe_targets, staircase_alphas
from tests.test_decode_probe_cpu import KV, Probe, _rand_q, base_kv, bound_of, target_refs

GROUPS = [1, 7, 8]
MAX_CTX = 2048
# (T, past), named for what breaks there
CASES = [(1, 0),        # one key
         (1, 63),       # the last key of a tile
         (1, 64),       # the first key of a tile
         (16, 7),       # one wave fragment, prefix shorter than a tile
         (65, 63),      # the query block boundary and the tile boundary both crossed
         (64, 64),      # everything aligned
         (130, 1),      # three 64-row blocks, partial last
         (100, 250),    # prefix ends mid-tile
         (257, 300),    # crosses form A's 256-row block
         (40, 2008)]    # ends on the slot's last row
ROW_MARKS = (0, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256)     # first rows of the fragments, waves and blocks of every form, and the rows before them


def _shared_q(T: int, G: int, seed: int) -> torch.Tensor:
    """Random q whose target heads are the same vector in every row: one planted key then weighs the same for all rows that see it."""
    q = _rand_q(T, G, seed)
    for t in probe_targets(KV, G):
        q[:, t] = q[0, t].clone()
    return q


def append_probes(G: int, T: int, past: int):
    """The planted-key cases of one (T, past): row i reads keys 0 .. past + i of a slot of MAX_CTX positions.
    single keys (inside): key 0, past - 1, past, 63, 64 and past + T - 1, each seen by every row at or behind it;
    own (inside): key past + i carries row i's own q, for every row;
    staircase (outside): for the marked rows i, keys past + i and past + i + 1 carry scores rising by >= 9 per key, so row i returns V[past + i] and a
    row that also sees past + i + 1 (which row i + 1 must) returns that key's V instead."""
    C = MAX_CTX
    kb, vb = base_kv(1, C)
    lens = [past + i + 1 for i in range(T)]
    seed = 7000 + 13 * past + 3 * T + G
    singles = {"key0": 0, "past-1": past - 1, "past": past, "key63": 63, "key64": 64, "last": past + T - 1}
    seen = set()
    for j, (name, key) in enumerate(singles.items()):
        if key < 0 or key > past + T - 1 or key in seen or past + T == 1:     # (a lone key cannot be dropped: no reference without a key)
            continue
        seen.add(key)
        q = _shared_q(T, G, seed + 101 * j)
        k = kb.clone()
        plant_keys(k[0], q[0], [key])
        yield Probe(f"append G={G} T={T} past={past} {name}", "inside", q, k, vb, lens, [key if key <= past + i and past + i > 0 else None for i in range(T)])
    q = _rand_q(T, G, seed + 1)
    k = kb.clone()
    for i in range(T):
        plant_keys(k[0], q[i], [past + i])
    yield Probe(f"append G={G} T={T} past={past} own", "inside", q, k, vb, lens, [past + i if past + i > 0 else None for i in range(T)])
    rows = sorted({i for i in ROW_MARKS + (T - 1, T - 2) if 0 <= i < T and past + i + 1 < C})
    if rows:
        keys = sorted({past + i for i in rows} | {past + i + 1 for i in rows})
        q = _shared_q(T, G, seed + 2)
        k = kb.clone()
        plant_keys(k[0], q[0], keys, staircase_alphas(q[0], KV, len(keys)))
        yield Probe(f"append G={G} T={T} past={past} staircase", "outside", q, k, vb, lens, [past + i + 1 if i in rows else None for i in range(T)])


@pytest.mark.parametrize("G", GROUPS)
def test_every_planted_case_moves_the_reference_by_8x_the_bound(G):
    n_cases = n_rows = 0
    worst = (float("inf"), "")
    for T, past in CASES:
        names = []
        for p in append_probes(G, T, past):
            names.append(p.name.split()[-1])
            bound = bound_of(p.v)
            good, bad = target_refs(p, False), target_refs(p, True)
            for i, f in enumerate(p.flip):
                if f is None:
                    continue
                assert (f < p.lens[i]) == (p.kind == "inside"), (p.name, i)
                moved = float((good[i] - bad[i]).abs().amax(-1).min())            # the target head that moves least
                assert moved >= 8 * bound, f"{p.name} row {i} (key {f} {'dropped' if p.kind == 'inside' else 'admitted'}): moves {moved:.3f} < 8 x {bound:.3f}"
                worst = min(worst, (moved, f"{p.name} row {i}"))
                n_rows += 1
            n_cases += 1
        assert "own" in names and "staircase" in names, (T, past, names)
    print(f"G={G}: {n_cases} cases, {n_rows} probed rows; smallest move {worst[0]:.3f} ({worst[1]})")


def test_the_cases_plant_what_the_issue_names():
    """Key 0, past - 1, past, 63, 64 and past + T - 1 each appear as a single planted key in some case, and the last case ends on the slot's last row."""
    names = {p.name.split()[-1] for T, past in CASES for p in append_probes(7, T, past)}
    assert names == {"key0", "past-1", "past", "key63", "key64", "last", "own", "staircase"}
    assert CASES[-1][0] + CASES[-1][1] == MAX_CTX


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------------
def _header(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(root, "include", name)).read(), flags=re.S)


def _params(flat, name):
    m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", flat)
    assert m, f"{name} is not declared"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_append_entries_are_declared_on_both_sides():
    from vila_amd import _lib
    flat = _header("vila_hip.h")
    for name in ("vila_attn_append_bf16", "vila_llm_prefill_append_workspace_bytes", "vila_llm_prefill_append_w4_workspace_bytes",
                 "vila_llm_prefill_append", "vila_llm_prefill_append_w4"):
        assert len(_params(flat, name)) == len(_lib.PROTOTYPES[name][1]), name
    bf16, w4 = _params(flat, "vila_llm_prefill_append"), _params(flat, "vila_llm_prefill_append_w4")
    assert [a for a in w4 if "qlayers" not in a] == bf16 and len(w4) == len(bf16) + 1, "the W4 entry adds `qlayers` and nothing else"
    assert _lib.PROTOTYPES["vila_llm_prefill_append_w4"][1][2:] == _lib.PROTOTYPES["vila_llm_prefill_append"][1][1:]
    tuning = _header("vila_hip_tuning.h")
    for name in ("vila_attn_force_append", "vila_attn_append_form"):
        assert len(_params(tuning, name)) == len(_lib.PROTOTYPES[name][1]), name


# ---- generate(): argument errors -------------------------------------------------------------------------------------------------------------
def test_generate_refuses_bad_append_arguments_before_anything_runs():
    from vila_amd.modules import HipQwen2ForCausalLM
    llm = object.__new__(HipQwen2ForCausalLM)          # no parameters, no device: the checks come first
    one, two = torch.zeros(1, 4, 8), torch.zeros(2, 4, 8)
    cache = SimpleNamespace(max_ctx=64, n_slots=1)
    with pytest.raises(ValueError, match="past_len.*cache"):
        HipQwen2ForCausalLM.generate(llm, one, past_len=3)
    with pytest.raises(ValueError, match="past_len.*batch size 1"):
        HipQwen2ForCausalLM.generate(llm, two, past_len=3, cache=cache)
    with pytest.raises(ValueError, match="past_len.*non-negative"):
        HipQwen2ForCausalLM.generate(llm, one, past_len=-1, cache=cache)
    for bad in (0, -5):
        with pytest.raises(ValueError, match="prefill_chunk.*positive"):
            HipQwen2ForCausalLM.generate(llm, one, prefill_chunk=bad)
    with pytest.raises(ValueError, match="prefill_chunk.*batch size 1"):
        HipQwen2ForCausalLM.generate(llm, two, prefill_chunk=16)


# ---- ChatSession against a fake model --------------------------------------------------------------------------------------------------------
class _Tok:
    """Whitespace tokenizer over a growing vocabulary; `<image>` is split off by `encode_with_images` before it gets here."""
    eos_token_id = 1

    def __init__(self):
        self.vocab, self.inv = {"<|im_end|>": 1}, {1: "<|im_end|>"}

    def __call__(self, text, add_special_tokens=False):
        ids = []
        for w in text.replace("<|im_end|>", " <|im_end|> ").split():
            if w not in self.vocab:
                self.vocab[w] = len(self.vocab) + 2
                self.inv[self.vocab[w]] = w
            ids.append(self.vocab[w])
        return SimpleNamespace(input_ids=ids)

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(self.inv.get(i, f"<{i}>") for i in ids if not (skip_special_tokens and i == 1))


class _FakeLlm:
    def __init__(self, script):
        self.script, self.calls, self.caches = list(script), [], 0

    def new_cache(self, max_ctx, n_slots=1):
        self.caches += 1
        return SimpleNamespace(max_ctx=max_ctx, n_slots=n_slots)

    def generate(self, inputs_embeds, max_new_tokens, cache, past_len=None, eos_token_id=None, **kw):
        assert cache is not None and inputs_embeds.shape[0] == 1
        self.calls.append(SimpleNamespace(past_len=past_len, n_new=inputs_embeds.shape[1], first=float(inputs_embeds[0, 0, 0]), kw=kw,
                                          max_new_tokens=max_new_tokens, eos=eos_token_id))
        reply = self.script.pop(0)
        if isinstance(reply, Exception):
            raise reply
        assert len(reply) <= max_new_tokens
        return torch.tensor([reply])


class _FakeModel:
    """`_embed` gives every id one row holding the id itself, and an image placeholder IMG_ROWS rows of -1."""
    IMG_ROWS = 5

    def __init__(self, script):
        from vila_amd import configs
        self.cfg = configs.tiny()
        self.device = torch.device("cpu")
        self.llm = _FakeLlm(script)
        self.media_seen = []

    def _embed(self, input_ids, media, media_config=None, labels=None, attention_mask=None):
        self.media_seen.append(len(media.get("image", [])))
        rows = []
        for t in input_ids[0].tolist():
            rows += [[-1.0]] * self.IMG_ROWS if t == self.cfg.image_token_id else [[float(t)]]
        assert sum(1 for t in input_ids[0].tolist() if t == self.cfg.image_token_id) == self.media_seen[-1]
        return torch.tensor(rows)[None], None, None


def _session(script, max_ctx=256, **kw):
    from vila_amd import serving
    tok = _Tok()
    model = _FakeModel(script)
    return serving.ChatSession(model, tok, max_ctx=max_ctx, **kw), model, tok


def test_chat_session_counts_cached_positions_and_feeds_the_last_token_first():
    import numpy as np
    s, model, tok = _session([[40, 41, 42, 1], [50, 51, 52], [60, 1]])
    img = np.zeros((56, 56, 3), np.uint8)
    assert s.ask([img, "what is this"], max_new_tokens=8) == tok.decode([40, 41, 42])
    c0 = model.llm.calls[0]
    S0 = c0.n_new
    assert c0.past_len is None and S0 == len(s.ids) - 4 - 1 + _FakeModel.IMG_ROWS        # one placeholder id became IMG_ROWS positions
    assert s.cached == S0 + 4 - 1, "P + S + n - 1 after a turn cut at its EOS (the EOS included, never fed)"
    ids_after_1 = list(s.ids)
    assert ids_after_1[-4:] == [40, 41, 42, 1]

    # turn 2 ends at max_new_tokens, without an EOS
    s.ask("and the colour", max_new_tokens=3)
    c1 = model.llm.calls[1]
    assert c1.past_len == S0 + 3 and c1.first == 1.0, "the next turn's first new token is the last emitted one"
    assert s.cached == c1.past_len + c1.n_new + 3 - 1
    new2 = s.ids[len(ids_after_1):-3]
    assert c1.n_new == 1 + len(new2) and tok.inv[new2[0]] == "<|im_start|>user", "an EOS-cut reply needs no end-of-turn marker"
    assert model.media_seen == [1, 0], "a text turn encodes no media"
    ids_after_2, cached_2 = list(s.ids), s.cached

    # turn 3: the reply before it had no EOS, so the marker is fed behind its last token
    s.ask("thanks", max_new_tokens=4)
    c2 = model.llm.calls[2]
    assert c2.past_len == cached_2 and c2.first == 52.0
    new3 = s.ids[len(ids_after_2):-2]
    assert new3[0] == 1 and c2.n_new == 1 + len(new3)
    assert s.cached == c2.past_len + c2.n_new + 2 - 1
    assert model.llm.caches == 1, "one cache for the whole conversation"


def test_chat_session_overflow_and_failure_leave_the_state_and_reset_empties_it():
    from vila_amd import serving
    s, model, tok = _session([[40, 1], RuntimeError("boom"), [41, 1], [42, 1]], max_ctx=40)
    s.ask("one two three", max_new_tokens=4)
    before = (list(s.ids), s.cached, s._last, s._closed)
    with pytest.raises(serving.ChatOverflow, match="max_ctx 40"):
        s.ask("four five six", max_new_tokens=30)
    assert (s.ids, s.cached, s._last, s._closed) == before and len(model.llm.calls) == 1
    with pytest.raises(RuntimeError, match="boom"):
        s.ask("four", max_new_tokens=2)
    assert (s.ids, s.cached, s._last, s._closed) == before
    s.ask("four", max_new_tokens=2)                                             # still usable
    assert model.llm.calls[-1].past_len == before[1] and s.cached > before[1]
    s.reset()
    assert s.ids == [] and s.cached == 0
    s.ask("again", max_new_tokens=2)
    assert model.llm.calls[-1].past_len is None and model.llm.caches == 1


def test_chat_session_passes_generation_arguments_and_lookup_history():
    s, model, tok = _session([[40, 1], [41, 1]], temperature=0.5, do_sample=True)
    s.ask("hello", max_new_tokens=2, seed=9)
    assert model.llm.calls[0].kw == {"temperature": 0.5, "do_sample": True, "seed": 9} and model.llm.calls[0].eos == 1
    ids1 = list(s.ids)
    s.ask("more", max_new_tokens=2, do_sample=False, prompt_lookup_num_tokens=4)
    kw = model.llm.calls[1].kw
    assert kw["prompt_lookup_num_tokens"] == 4 and kw["prompt_ids"].tolist() == s.ids[:-2] and kw["prompt_ids"].tolist()[:len(ids1)] == ids1
