"""CPU tests of LoRA serving (vila_amd/lora_serving.py, the C-ABI of vila_amd/csrc/lora_decode.hip and of the step with adapters, the batcher's
routing): the header's new structs and entries as plain C with the ctypes offsets, the bank's packing on the CPU, the step's names and refusals, and
`ContinuousBatcher(adapters=True)` in front of a stub engine."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

from tests import lora_serving_ref as R
from vila_amd import configs, serving

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_STRUCTS = ("VilaLoraBankLayer", "VilaLoraBank", "VilaLoraLayer")
NEW_ENTRIES = {"vila_lora_shrink_bf16": 13, "vila_lora_expand_f32": 14, "vila_gemm_batch_lora_bf16": 17, "vila_gateup_batch_lora_bf16": 13,
               "vila_qkv_batch_lora_bf16": 21, "vila_llm_decode_batch_lora_workspace_bytes": 4, "vila_llm_decode_step_batch_lora": 13,
               "vila_llm_prefill_lora_workspace_bytes": 3, "vila_llm_prefill_lora": 20}


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_new_structs_and_entries_are_plain_c_with_the_ctypes_layout(tmp_path):
    """tests/test_abi_layout_cpu.py for what this feature adds: the header compiles as C99, every new struct has ctypes' size and offsets, and every
    new entry is declared (its address is taken) with the argument count of vila_amd/_lib.py."""
    from vila_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vila_hip.h"', "int main(void) {"]
    for name in NEW_STRUCTS:
        cls = getattr(_lib, name)
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        for field in cls._fields_:
            lines.append(f'    printf("{name} {field[0]} %zu\\n", offsetof({name}, {field[0]}));')
    for fn in NEW_ENTRIES:
        lines.append(f'    printf("{fn} declared %d\\n", {fn} != 0);')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    # -c only: the entries are declared, not linked (the library needs the HIP runtime); the layout program itself is built without them below
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-Wno-address", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "layout.o")], capture_output=True, text=True)
    assert r.returncode == 0, "include/vila_hip.h must compile as C99 with the new structs and entries:\n" + r.stderr
    src.write_text("\n".join(ln for ln in lines if "declared" not in ln) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        s, f, v = line.split()
        got[(s, f)] = int(v)
    for name in NEW_STRUCTS:
        cls = getattr(_lib, name)
        assert got[(name, "sizeof")] == C.sizeof(cls), f"sizeof({name}): header {got[(name, 'sizeof')]} vs ctypes {C.sizeof(cls)}"
        for field in cls._fields_:
            assert got[(name, field[0])] == getattr(cls, field[0]).offset, f"{name}.{field[0]}"
    for fn, n_args in NEW_ENTRIES.items():
        assert fn in _lib.PROTOTYPES and len(_lib.PROTOTYPES[fn][1]) == n_args, fn
    from vila_amd import ops
    assert all(callable(getattr(ops, f)) for f in ("lora_shrink", "lora_expand", "gemm_batch_lora", "qkv_batch_lora"))


# ---- the bank's packing ---------------------------------------------------------------------------------------------------------------------------------
def _lcfg():
    return configs.tiny("mlp_downsample").llm


def test_pack_then_unpack_returns_the_peft_tensors():
    from vila_amd import lora_serving as LS
    c = _lcfg()
    for r_ad, targets in ((16, None), (32, ("q_proj", "v_proj", "down_proj")), (64, ("k_proj", "up_proj"))):
        ad = R.random_adapter(c, r_ad, 32.0, targets, seed=r_ad)
        want = ad.state_dict()
        packed = LS.pack_adapter(c, ad, 64)
        got = LS.unpack_adapter(c, packed, ad.cfg, 64)
        assert set(got) == set(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
        for stack, (A, Bt) in packed.items():                         # ... and through the chunk-major B the expand kernel reads
            bp = LS.pack_b(Bt)
            assert bp.shape == (*Bt.shape[:-2], 8, Bt.shape[-1], 8) and bp.is_contiguous()
            assert torch.equal(LS.unpack_b(bp), Bt)
            j, col = 37 % Bt.shape[-2], 11 % Bt.shape[-1]
            assert torch.equal(bp[0, j // 8, col, j % 8], Bt[0, j, col])          # element (c, col, e) = B[col][8 c + e]


def test_rank_padding_and_absent_modules_are_exact_zeros():
    from vila_amd import lora_serving as LS
    c = _lcfg()
    r = 64
    ad = R.random_adapter(c, 16, 32.0, ("q_proj", "v_proj", "down_proj"), seed=3)
    packed = LS.pack_adapter(c, ad, r)
    is_zero = lambda t: bool((t.contiguous().view(torch.int16) == 0).all())       # +0.0 bit for bit
    shapes = {s: (K, Rs, N, cols) for s, K, Rs, N, cols in LS.stack_shapes(c, r)}
    assert set(packed) == {"qkv", "o", "gateup", "down"}
    for stack, (A, Bt) in packed.items():
        K, Rs, N, cols = shapes[stack]
        assert A.shape == (c.num_hidden_layers, Rs, K) and Bt.shape == (c.num_hidden_layers, r, N)
        for j, (m, c0, width) in enumerate(cols):
            if m in ad.cfg.target_modules:
                assert not is_zero(A[:, j * r:j * r + 16]) and not is_zero(Bt[:, :16, c0:c0 + width]), m
                assert is_zero(A[:, j * r + 16:(j + 1) * r]) and is_zero(Bt[:, 16:, c0:c0 + width]), f"{m}: ranks 16..63 are padding"
            else:
                assert is_zero(A[:, j * r:(j + 1) * r]) and is_zero(Bt[:, :, c0:c0 + width]), f"{m} is not a target module"
    # a rank above the bank's is refused
    with pytest.raises(ValueError, match="exceeds"):
        LS.pack_adapter(c, R.random_adapter(c, 32, 32.0, None, seed=4), 16)


def test_bank_on_the_cpu_loads_unloads_and_keeps_its_buffers(tmp_path):
    from vila_amd import lora, lora_serving as LS
    c = _lcfg()
    bank = LS.AdapterBank(c, capacity=2, r=32, device="cpu")
    ptrs = {(d, s): t.data_ptr() for d, ts in (("a", bank.a), ("b", bank.b), ("bt", bank.bt)) for s, t in ts.items()}
    a1 = R.random_adapter(c, 32, 16.0, None, seed=5)
    a2 = R.random_adapter(c, 16, 32.0, ("q_proj", "o_proj"), seed=6)
    folder = str(tmp_path / "a2")
    lora.save_adapter(a2, folder)
    assert bank.load("one", a1) == 0 and bank.load("two", folder) == 1
    assert bank.scale.tolist() == [0.5, 2.0] and "one" in bank and "three" not in bank and bank.slot_of(None) == -1
    for name, ad in (("one", a1), ("two", a2)):
        got, want = bank.unpack(name), ad.state_dict()
        assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    with pytest.raises(ValueError, match="slots are taken"):
        bank.load("three", a1)
    with pytest.raises(ValueError, match="already loaded"):
        bank.load("one", a1)
    bank.in_use[0] = 1                                                 # a live row under "one"
    with pytest.raises(RuntimeError, match="live rows"):
        bank.unload("one")
    bank.in_use[0] = 0
    bank.unload("one")
    assert bank.names == [None, "two"] and float(bank.scale[0]) == 0.0 and all(not bool(t[:, 0].any()) for d in (bank.a, bank.b, bank.bt) for t in d.values())
    assert bank.load("three", a2) == 0                                 # the freed slot is handed on
    assert ptrs == {(d, s): t.data_ptr() for d, ts in (("a", bank.a), ("b", bank.b), ("bt", bank.bt)) for s, t in ts.items()}, "a bank's buffers never move"
    assert bank.bytes_per_slot() == sum(t[:, 0].numel() * 2 for d in (bank.a, bank.b, bank.bt) for t in d.values()) + 4
    with pytest.raises(KeyError, match="no adapter named"):
        bank.slot_of("one")


def test_non_lora_trainables_projector_is_kept_tower_and_llm_are_refused(tmp_path):
    from vila_amd import lora, lora_serving as LS
    c = _lcfg()
    ad = R.random_adapter(c, 16, 32.0, None, seed=7)
    assert LS.split_non_lora({"mm_projector.layers.1.weight": torch.ones(3)}).keys() == {"layers.1.weight"}
    for bad, word in (("vision_tower.x.weight", "vision_tower"), ("llm.model.norm.weight", "llm")):
        folder = str(tmp_path / word)
        lora.save_adapter(ad, folder, non_lora={bad: torch.ones(4)})
        with pytest.raises(ValueError, match=f"{word} tensors outside the adapters"):
            LS.AdapterBank(c, capacity=1, r=16, device="cpu").load("x", folder)
    folder = str(tmp_path / "proj")
    lora.save_adapter(ad, folder, non_lora={"mm_projector.layers.1.weight": torch.ones(4)})
    with pytest.raises(ValueError, match="need a bank made from a model"):
        LS.AdapterBank(c, capacity=1, r=16, device="cpu").load("x", folder)


# ---- the step's names and refusals ------------------------------------------------------------------------------------------------------------------------
def test_step_symbols_of_the_step_with_adapters_and_its_refusals():
    from vila_amd.modules import _step_symbols
    want = ("vila_llm_decode_step_batch_lora", "vila_llm_decode_batch_lora_workspace_bytes")
    for kw in ({}, dict(penalized=True), dict(constrained=True), dict(any_k=True)):
        for sampled in (False, True):
            assert _step_symbols(True, False, sampled, lora=True, **kw) == want
    for kw, word in ((dict(w4=True), "int4"), (dict(prefix=True), "shared-prefix"), (dict(verify=True), "verify"), (dict(verify_sample=True), "verify"),
                     (dict(processed=True, verify=True), "verify"), (dict(batch=False), "solo")):
        args = dict(batch=True, w4=False, sampled=False)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            _step_symbols(**args, lora=True)
    # without the flag every name is the one it was
    assert _step_symbols(True, False, False) == ("vila_llm_decode_step_batch", "vila_llm_decode_batch_workspace_bytes_ctx")
    assert _step_symbols(True, True, True, prefix=True) == ("vila_llm_decode_step_batch_prefix_w4_sample", "vila_llm_decode_batch_prefix_w4_sample_workspace_bytes")


def test_append_prefill_under_an_adapter_raises():
    from vila_amd.vlm import HipLlavaLlamaModel
    m = HipLlavaLlamaModel(configs.tiny("mlp_downsample"), device="cpu")
    with pytest.raises(ValueError, match="does not run under an unmerged adapter"):
        m.llm.prefill_append(torch.zeros(2, m.cfg.llm.hidden_size, dtype=torch.bfloat16), None, 0, adapter="a")
    with pytest.raises(ValueError, match="have no form under"):
        m.llm.generate(torch.zeros(1, 2, m.cfg.llm.hidden_size, dtype=torch.bfloat16), adapter="a", adapters=object(), prefill_chunk=8)
    with pytest.raises(ValueError, match="pass the AdapterBank"):
        m.llm.generate(torch.zeros(1, 2, m.cfg.llm.hidden_size, dtype=torch.bfloat16), adapter="a")


# ---- the batcher's routing ----------------------------------------------------------------------------------------------------------------------------------
class _StubEngine:
    """tests/test_serving_cpu.py's stub with a bank of names: a request "name:n" replies tokens 100 + i (i < n) then EOS — 200 + i under an adapter
    whose name starts with "b" — and records what `embed` and `admit` were told."""
    eos = {1}
    batches_adapters = True

    def __init__(self, n_slots=4, loaded=("ada", "bob"), **flags):
        self.n_slots, self.loaded = n_slots, set(loaded)
        self.script = {b: None for b in range(n_slots)}
        self.n_out, self.out, self.calls = [0] * n_slots, [[] for _ in range(n_slots)], []
        for k, v in flags.items():
            setattr(self, k, v)

    def has_adapter(self, name):
        return name in self.loaded

    def embed(self, prompt, system, adapter=None):
        from types import SimpleNamespace
        self.calls.append(("embed", prompt, adapter))
        n, base = int(prompt.split(":")[1]), 200 if (adapter or "").startswith("b") else 100
        return SimpleNamespace(shape=(7,), script=[base + i for i in range(n)] + [1] + [55] * 64)

    def fits(self, n_prompt, max_new):
        return max_new <= 48

    def admit(self, slot, e, sampling=None, adapter=None, **kw):
        self.calls.append(("admit", slot, adapter, sampling is not None))
        self.script[slot], self.n_out[slot], self.out[slot] = e.script, 0, []
        return e.script[0]

    def run(self, k):
        for _ in range(k):
            for b in range(self.n_slots):
                sc = self.script[b]
                self.out[b].append(sc[1 + self.n_out[b]] if sc is not None else 7)
                self.n_out[b] += 1

    def read(self):
        top = max(max(self.n_out), 1)
        return list(self.n_out), [r[:top] + [0] * (top - len(r)) for r in self.out]

    def release(self, slots):
        for b in slots:
            self.n_out[b], self.out[b] = 0, []

    def solo(self, prompt, max_new_tokens, system, **gen):
        self.calls.append(("solo", prompt, dict(gen)))
        return f"solo {prompt}"

    def decode(self, toks):
        return " ".join(str(t) for t in toks)


def _reply(n, base=100):
    return " ".join(str(base + i) for i in range(n))


def test_batcher_routes_the_model_field_to_adapters_and_everything_else_to_the_base():
    eng = _StubEngine()
    b = serving.ContinuousBatcher(eng, max_batch=4, chunk=4, adapters=True)
    try:
        fa, fb, fc, fd = (b.submit("A:6", 48, model="ada"), b.submit("B:9", 48, model="bob"), b.submit("C:4", 48, model="NVILA-8B"), b.submit("D:5", 48))
        assert fa.result(timeout=30) == _reply(6) and fb.result(timeout=30) == _reply(9, 200)
        assert fc.result(timeout=30) == _reply(4) and fd.result(timeout=30) == _reply(5)
        admits = {c[1]: c[2] for c in eng.calls if c[0] == "admit"}
        embeds = {c[1]: c[2] for c in eng.calls if c[0] == "embed"}
        assert embeds == {"A:6": "ada", "B:9": "bob", "C:4": None, "D:5": None}, embeds      # an unknown `model` is the base model's request
        assert sorted(v for v in admits.values() if v) == ["ada", "bob"] and list(admits.values()).count(None) == 2
        assert not any(c[0] == "solo" for c in eng.calls)
        # a sampled request under an adapter without batch_sampled: refused by name of the flag, not run solo; the base one still runs solo
        fe = b.submit("E:4", 16, model="ada", temperature=0.7, top_p=0.8)
        with pytest.raises(ValueError, match=r"adapter 'ada'.*batch_sampled=True"):
            fe.result(timeout=30)
        assert b.submit("F:4", 16, model="nobody", temperature=0.7, top_p=0.8).result(timeout=30) == "solo F:4"
        solo = [c for c in eng.calls if c[0] == "solo"]
        assert len(solo) == 1 and "model" not in solo[0][2] and "adapter" not in solo[0][2]
        for gen, word in ((dict(repetition_penalty=1.3), "penalties=True"), (dict(logprobs=True, top_logprobs=2), "logprobs=True"),
                          (dict(guided_choice=["yes", "no"]), "constraints=True")):
            with pytest.raises(ValueError, match=word):
                b.submit("G:4", 16, model="bob", **gen).result(timeout=30)
        with pytest.raises(ValueError, match="do not fit a slot"):
            b.submit("H:4", 200, model="bob").result(timeout=30)
        assert b.submit("I:3", 48, model="bob").result(timeout=30) == _reply(3, 200)           # the line goes on behind every refusal
    finally:
        b.close()


def test_batcher_without_the_flag_drops_the_model_field():
    eng = _StubEngine()
    b = serving.ContinuousBatcher(eng, max_batch=4, chunk=4)
    try:
        assert b.submit("A:6", 48, model="ada").result(timeout=30) == _reply(6)
        assert [c[2] for c in eng.calls if c[0] == "embed"] == [None] and [c[2] for c in eng.calls if c[0] == "admit"] == [None]
    finally:
        b.close()


def test_batcher_with_batch_sampled_gives_a_sampled_adapter_request_a_row():
    eng = _StubEngine(batches_sampled=True)
    b = serving.ContinuousBatcher(eng, max_batch=4, chunk=4, adapters=True, batch_sampled=True)
    try:
        assert b.submit("A:6", 48, model="bob", temperature=0.7, top_p=0.8, seed=5).result(timeout=30) == _reply(6, 200)
        assert [c for c in eng.calls if c[0] == "admit"] == [("admit", 0, "bob", True)]
        with pytest.raises(ValueError, match="any_top_k=True"):
            b.submit("B:6", 48, model="bob", temperature=0.7, top_k=0).result(timeout=30)
    finally:
        b.close()
