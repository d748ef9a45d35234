"""CPU tests of the LoRA feature (vila_amd/lora.py, the C-ABI of vila_amd/csrc/lora.hip): adapter files and their round trip, stacking, the merge
arithmetic, the configuration's limits, the trainable-state count, the header, the per-element bound the GPU operator tests use (proved on a CPU
emulation of each kernel's arithmetic at the same cases) and the gradient exchange over the adapter buffer (gloo, world 2)."""
import json
import os
import shutil
import subprocess

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import lora_ref as LR
from tests.gpu_util import BF16_U, FP32_U, assert_elementwise
from vila_amd import configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny_model(seed=0):
    from vila_amd.vlm import HipLlavaLlamaModel
    m = HipLlavaLlamaModel(configs.tiny("mlp_downsample"), device="cpu")
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return m


def _read(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


# ---- files ------------------------------------------------------------------------------------------------------------------------------------------
def test_adapter_files_have_pefts_keys_and_shapes_and_round_trip_byte_equal(tmp_path):
    from safetensors import safe_open
    from vila_amd import lora
    cfg = configs.tiny("mlp_downsample")
    c = cfg.llm
    tr = lora.LoRATrainer(_tiny_model(), lora.LoraConfig(r=16, alpha=32))
    with torch.no_grad():
        tr.adapters.params.copy_(torch.randn(tr.adapters.numel, generator=torch.Generator().manual_seed(1)))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    lora.save_adapter(tr, a)
    assert sorted(os.listdir(a)) == ["adapter_config.json", "adapter_model.safetensors", "non_lora_trainables.bin"]
    conf = json.load(open(os.path.join(a, "adapter_config.json")))
    assert conf["peft_type"] == "LORA" and conf["r"] == 16 and conf["lora_alpha"] == 32 and conf["lora_dropout"] == 0.0 and conf["bias"] == "none"
    assert conf["target_modules"] == sorted(lora.LLM_TARGETS) and "lm_head" not in conf["target_modules"] and conf["use_dora"] is False
    shapes = {"q_proj": (c.hidden_size, c.q_size), "k_proj": (c.hidden_size, c.kv_size), "v_proj": (c.hidden_size, c.kv_size),
              "o_proj": (c.q_size, c.hidden_size), "gate_proj": (c.hidden_size, c.intermediate_size), "up_proj": (c.hidden_size, c.intermediate_size),
              "down_proj": (c.intermediate_size, c.hidden_size)}
    want = {}
    for i in range(c.num_hidden_layers):
        for m, (fin, fout) in shapes.items():
            parent = "self_attn" if m[0] in "qkvo" else "mlp"
            want[f"base_model.model.llm.model.layers.{i}.{parent}.{m}.lora_A.weight"] = (16, fin)
            want[f"base_model.model.llm.model.layers.{i}.{parent}.{m}.lora_B.weight"] = (fout, 16)
    with safe_open(os.path.join(a, "adapter_model.safetensors"), framework="pt") as fh:
        got = {k: tuple(fh.get_tensor(k).shape) for k in fh.keys()}
    assert got == want
    non = torch.load(os.path.join(a, "non_lora_trainables.bin"), weights_only=True)
    assert set(non) == {"base_model.model.mm_projector." + n for n, _ in tr.model.mm_projector.named_parameters()}
    for n, p in tr.model.mm_projector.named_parameters():
        assert torch.equal(non["base_model.model.mm_projector." + n], p.detach())
    # save -> load into a fresh trainer (other adapters, another projector) -> save: the same bytes, the same parameters, masters re-seeded
    tr2 = lora.LoRATrainer(_tiny_model(seed=5), lora.LoraConfig(r=16, alpha=32, seed=9))
    assert not torch.equal(tr2.flat.params, tr.flat.params)
    lora.load_adapter(tr2, a)
    lora.save_adapter(tr2, b)
    assert _read(a) == _read(b)
    assert torch.equal(tr2.flat.params, tr.flat.params) and torch.equal(tr2.flat.master, tr2.flat.params.float())
    for n, p in tr2.model.mm_projector.named_parameters():                           # the module's parameters ARE the trainer's buffer
        assert torch.equal(p, dict(tr.model.mm_projector.named_parameters())[n])
    with pytest.raises(ValueError, match="does not match"):
        lora.load_adapter(lora.LoRATrainer(_tiny_model(), lora.LoraConfig(r=32)), a)


def test_stacking_then_unstacking_is_the_identity():
    from vila_amd import lora
    c = configs.tiny().llm
    for targets in (lora.LLM_TARGETS, ("q_proj", "v_proj"), ("k_proj", "up_proj", "down_proj")):
        lc = lora.LoraConfig(r=16, target_modules=targets)
        ad = lora.LoraAdapters(c, lc)
        g = torch.Generator().manual_seed(3)
        sd = {}
        for i in range(c.num_hidden_layers):
            for m in lc.target_modules:
                a, bt = ad.pair(i, m)
                key = f"base_model.model.llm.model.layers.{i}.{'self_attn' if m[0] in 'qkvo' else 'mlp'}.{m}."
                sd[key + "lora_A.weight"] = torch.randn(a.shape, generator=g).to(torch.bfloat16)
                sd[key + "lora_B.weight"] = torch.randn(bt.shape[1], bt.shape[0], generator=g).to(torch.bfloat16)
        ad.load_state_dict(sd)
        back = ad.state_dict()
        assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
        if "q_proj" in targets and "v_proj" in targets:                               # the stack holds its members' As in q, k, v order, Bt is B^T
            r = 16
            stack = ad.tensor(0, "A_qkv")
            j = list(ad.stacks[0][2]).index("v_proj")
            assert torch.equal(stack[j * r:(j + 1) * r], sd["base_model.model.llm.model.layers.0.self_attn.v_proj.lora_A.weight"])
            assert torch.equal(ad.tensor(0, "Bt_q"), sd["base_model.model.llm.model.layers.0.self_attn.q_proj.lora_B.weight"].t())
        with pytest.raises(KeyError):
            ad.load_state_dict({k: v for k, v in list(sd.items())[1:]})
    # PEFT's initialisation: B zero, A inside the Kaiming-uniform(a = sqrt 5) interval +- 1 / sqrt(in) and filling it; seeded
    ad = lora.LoraAdapters(c, lora.LoraConfig(r=16, seed=2)).init_()
    for stack, in_dim, members in ad.stacks:
        a = ad.tensor(0, f"A_{stack}").float()
        assert float(a.abs().max()) <= in_dim ** -0.5 * (1 + 2 ** -8) and float(a.abs().max()) > 0.9 * in_dim ** -0.5 and abs(float(a.mean())) < 0.1 * in_dim ** -0.5
        for m in members:
            assert float(ad.tensor(0, f"Bt_{m[:-5]}").float().abs().sum()) == 0.0
    assert torch.equal(ad.params, lora.LoraAdapters(c, lora.LoraConfig(r=16, seed=2)).init_().params)
    assert not torch.equal(ad.params, lora.LoraAdapters(c, lora.LoraConfig(r=16, seed=3)).init_().params)


# ---- merge ------------------------------------------------------------------------------------------------------------------------------------------
def test_merge_is_w_plus_s_b_a_within_one_bf16_rounding():
    """merge_adapter on a CPU model against W + s B @ A in fp64: one bf16 rounding of the result plus the fp32 sum's (r + 2) 2^-24 of the
    magnitudes; q | k | v stay one fused buffer; a model whose bf16 projections were released is refused."""
    from vila_amd import lora
    from vila_amd.modules import _get
    m = _tiny_model(seed=2)
    c = m.cfg.llm
    lc = lora.LoraConfig(r=16, alpha=48)
    ad = LR.random_adapters(m.cfg, lc, 4)
    names = [f"model.layers.{i}.{'self_attn' if t[0] in 'qkvo' else 'mlp'}.{t}.weight" for i in range(c.num_hidden_layers) for t in lc.target_modules]
    before = {n: _get(m.llm, n).detach().clone() for n in names}
    other = {n: p.detach().clone() for n, p in m.llm.named_parameters() if n not in names}
    lora.merge_adapter(m, ad)
    assert m.llm._qkv_fused()
    worst = 0.0
    for i in range(c.num_hidden_layers):
        for t in lc.target_modules:
            n = f"model.layers.{i}.{'self_attn' if t[0] in 'qkvo' else 'mlp'}.{t}.weight"
            a, bt = ad.pair(i, t)
            ref = before[n].double() + lc.scale * (bt.double().t() @ a.double())
            mag = before[n].double().abs() + lc.scale * (bt.double().abs().t() @ a.double().abs())
            worst = max(worst, assert_elementwise(_get(m.llm, n).detach(), ref, BF16_U * ref.abs() + (1 + BF16_U) * (lc.r + 2) * FP32_U * mag, n))
            assert not torch.equal(_get(m.llm, n).detach(), before[n])
    print(f"merge: worst err / bound {worst:.3f}")
    for n, p in m.llm.named_parameters():
        if n not in names:
            assert torch.equal(p.detach(), other[n]), n
    m.llm._bf16_released = True
    try:
        with pytest.raises(RuntimeError, match="release_bf16"):
            lora.merge_adapter(m, ad)
    finally:
        m.llm._bf16_released = False


def test_merge_from_a_folder_also_loads_the_tuned_projector(tmp_path):
    from vila_amd import lora
    tr = lora.LoRATrainer(_tiny_model(seed=1), lora.LoraConfig(r=16))
    with torch.no_grad():
        tr.flat.params.copy_(torch.randn(tr.flat.numel, generator=torch.Generator().manual_seed(8)) * 0.05)
    lora.save_adapter(tr, str(tmp_path))
    from vila_amd.modules import _get
    m = _tiny_model(seed=1)
    base = _get(m.llm, "model.layers.0.mlp.down_proj.weight").detach().clone()
    lora.merge_adapter(m, str(tmp_path))
    for n, p in m.mm_projector.named_parameters():
        assert torch.equal(p.detach(), dict(tr.model.mm_projector.named_parameters())[n].detach()), n
    a, bt = tr.adapters.pair(0, "down_proj")
    got = _get(m.llm, "model.layers.0.mlp.down_proj.weight").detach()
    assert torch.equal(got, lora.merge_weight(base, a, bt, tr.lora.scale)) and not torch.equal(got, base)


# ---- configuration and state ------------------------------------------------------------------------------------------------------------------------
def test_config_names_its_limits():
    from vila_amd.lora import LLM_TARGETS, LoraConfig
    assert LoraConfig().r == 64 and LoraConfig().alpha == 16 and LoraConfig().scale == 0.25 and LoraConfig().target_modules == LLM_TARGETS
    for r in (16, 32, 48, 64):
        assert LoraConfig(r=r, alpha=r).scale == 1.0
    for r in (0, 8, 24, 128):
        with pytest.raises(ValueError, match="r = "):
            LoraConfig(r=r)
    with pytest.raises(ValueError, match="dropout = 0.0"):
        LoraConfig(dropout=0.05)
    with pytest.raises(ValueError, match="DoRA"):
        LoraConfig(use_dora=True)
    with pytest.raises(ValueError, match="lora_vt"):
        LoraConfig(lora_vt=True)
    with pytest.raises(ValueError, match="bias"):
        LoraConfig(bias="all")
    with pytest.raises(ValueError, match="lm_head"):
        LoraConfig(target_modules=("q_proj", "lm_head"))
    assert LoraConfig(target_modules=("v_proj", "q_proj")).target_modules == ("q_proj", "v_proj")
    assert LoraConfig.from_peft(LoraConfig(r=32, alpha=8).to_peft()) == LoraConfig(r=32, alpha=8)


def test_state_numel_is_the_padded_count_of_trainable_elements():
    from vila_amd import lora
    from vila_amd.train import FlatParams
    m = _tiny_model()
    c, r = m.cfg.llm, 16
    pad = lambda n: (n + 7) // 8 * 8
    per_layer = (pad(3 * r * c.hidden_size) + pad(r * c.q_size) + 2 * pad(r * c.kv_size) + pad(r * c.q_size) + pad(r * c.hidden_size)
                 + pad(2 * r * c.hidden_size) + 2 * pad(r * c.intermediate_size) + pad(r * c.intermediate_size) + pad(r * c.hidden_size))
    proj = sum(pad(p.numel()) for p in m.mm_projector.parameters())
    tower = sum(pad(p.numel()) for p in m.vision_tower.parameters())
    tr = lora.LoRATrainer(m, lora.LoraConfig(r=r))
    assert tr.state_numel() == c.num_hidden_layers * per_layer + proj
    assert tr.flat.master.numel() == tr.flat.m.numel() == tr.flat.v.numel() == tr.flat.grads.numel() == tr.state_numel()
    assert tr.base.grads is None and tr.base.master is None                          # the frozen base: no gradients, no optimizer state
    assert tr.state_numel() < FlatParams(_tiny_model()).numel
    assert lora.LoRATrainer(_tiny_model(), lora.LoraConfig(r=r), tune_mm_projector=False).state_numel() == c.num_hidden_layers * per_layer
    assert lora.LoRATrainer(_tiny_model(), lora.LoraConfig(r=r), tune_vision_tower=True).state_numel() == c.num_hidden_layers * per_layer + proj + tower
    assert lora.LoRATrainer(_tiny_model(), lora.LoraConfig(r=r, target_modules=())).state_numel() == proj
    with pytest.raises(ValueError, match="tune_mm_projector"):
        lora.LoRATrainer(_tiny_model(), lora.LoraConfig(r=r), tune_mm_projector=False, tune_vision_tower=True)
    # one bucket per decoder layer, then the projector; frozen tensors have no gradient, the decoder's norms a scratch row
    a0, b0 = tr.flat.span(lora.layer_prefix(0))
    a1, b1 = tr.flat.span(lora.layer_prefix(1))
    assert (a0, b0, a1, b1) == (0, per_layer, per_layer, 2 * per_layer) and tr.flat.span("mm_projector.") == (2 * per_layer, 2 * per_layer + proj)
    assert tr.flat.grad("llm.model.norm.weight").numel() == c.hidden_size
    with pytest.raises(KeyError, match="frozen"):
        tr.flat.grad("llm.model.layers.0.mlp.down_proj.weight")


def test_optimizer_state_of_the_adapter_buffer_round_trips(tmp_path):
    from vila_amd import checkpoint, lora
    tr = lora.LoRATrainer(_tiny_model(), lora.LoraConfig(r=16))
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for t in (tr.flat.master, tr.flat.m, tr.flat.v):
            t.copy_(torch.randn(t.shape, generator=g))
    tr.flat.step_count, tr.flat.bucket_steps = 3, {lora.layer_prefix(0): 3, "mm_projector.": 2}
    lora.save_checkpoint(tr, str(tmp_path))
    tr2 = lora.LoRATrainer(_tiny_model(seed=4), lora.LoraConfig(r=16, seed=1))
    lora.load_checkpoint(tr2, str(tmp_path))
    for k in ("master", "m", "v"):
        assert torch.equal(getattr(tr2.flat, k), getattr(tr.flat, k)), k
    assert torch.equal(tr2.flat.params, tr.flat.master.to(torch.bfloat16)) and tr2.flat.step_count == 3 and tr2.flat.bucket_steps == tr.flat.bucket_steps


# ---- the C-ABI --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_header_declares_the_lora_entries_as_plain_c(tmp_path):
    from vila_amd import _lib
    names = ["vila_lora_down_bf16", "vila_lora_up_bf16", "vila_lora_wgrad_bf16", "vila_lora_down_workspace_bytes", "vila_lora_up_workspace_bytes",
             "vila_lora_wgrad_workspace_bytes"]
    for n in names:
        assert n in _lib.PROTOTYPES, n
    src = tmp_path / "lora_abi.c"
    src.write_text('#include <stddef.h>\n#include "vila_hip.h"\n'
                   "typedef int (*down_t)(const void*, int64_t, const void*, int64_t, void*, int64_t, int, int, int, float, void*, size_t, vila_stream_t);\n"
                   "typedef int (*up_t)(const void*, int64_t, const void*, int64_t, const void*, int64_t, void*, int64_t, int, int, int, float, void*, size_t, vila_stream_t);\n"
                   "typedef int (*wgrad_t)(const void*, int64_t, const void*, int64_t, void*, int64_t, int, int, int, float, int, void*, size_t, vila_stream_t);\n"
                   "typedef size_t (*ws_t)(int, int, int);\n"
                   "down_t p_down = vila_lora_down_bf16; up_t p_up = vila_lora_up_bf16; wgrad_t p_wgrad = vila_lora_wgrad_bf16;\n"
                   "ws_t p_ws[3] = {vila_lora_down_workspace_bytes, vila_lora_up_workspace_bytes, vila_lora_wgrad_workspace_bytes};\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "lora_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, "the LoRA entries of include/vila_hip.h must compile as C99 with these signatures:\n" + r.stderr
    # the ctypes prototypes take the same number of arguments
    assert [len(_lib.PROTOTYPES[n][1]) for n in names] == [13, 15, 14, 3, 3, 3]


# ---- the bound of tests/test_gpu_lora_ops.py, on a CPU emulation of each kernel's arithmetic at the same cases ----------------------------------------
SHARP_MIN = 0.5          # a bound nobody comes near proves nothing: the worst emulated element must reach half of it (one bf16 rounding alone gives 0.996)


def test_element_bounds_hold_for_the_emulated_kernels():
    """fp32 accumulation in the kernel's split order, `scale` on the accumulator, Res / the old G added, one rounding (tests/lora_ref.py *_emulate)
    against the fp64 reference within gemm_elem_bound(..., roundings=1, extra_fp32_ops=3), for every case of the GPU test (the two 18944-wide
    8B shapes only in their first 256 rows: the contraction of `wgrad` is then shorter, which makes its bound tighter, not wider)."""
    worst = {"down": 0.0, "up": 0.0, "wgrad": 0.0}
    for i, (M, K, R, _pad) in enumerate(LR.DOWN_CASES):
        x, a = LR.down_inputs(M, K, R)
        if K == 18944:
            x = x[:256]
        ref, bound = LR.down_ref(x, a, LR.case_scale(i))
        worst["down"] = max(worst["down"], assert_elementwise(LR.down_emulate(x, a, LR.case_scale(i)), ref, bound, f"down [{M}, {K}] R={R}"))
    for i, (M, N, R, with_res, _pad) in enumerate(LR.UP_CASES):
        t, bt, res = LR.up_inputs(M, N, R)
        if N == 18944:
            t, res = t[:256], res[:256]
        res = res if with_res else None
        ref, bound = LR.up_ref(t, bt, res, LR.case_scale(i))
        worst["up"] = max(worst["up"], assert_elementwise(LR.up_emulate(t, bt, res, LR.case_scale(i)), ref, bound, f"up [{M}, {N}] R={R}"))
    for i, (M, C, R, acc, _pad) in enumerate(LR.WGRAD_CASES):
        l, x, old = LR.wgrad_inputs(M, C, R)
        if C == 18944:
            l, x = l[:256], x[:256]
        old = old if acc else None
        ref, bound = LR.wgrad_ref(l, x, old, LR.case_scale(i))
        worst["wgrad"] = max(worst["wgrad"], assert_elementwise(LR.wgrad_emulate(l, x, old, LR.case_scale(i)), ref, bound, f"wgrad [{M}, {C}] R={R}"))
    print("worst err / bound of the emulations:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v >= SHARP_MIN for v in worst.values()), worst


def test_split_policies_of_the_reference_match_the_cases_comments():
    assert LR.down_split(17, 1016) == (1, 1024) and LR.down_split(17, 1024) == (4, 256) and LR.down_split(17, 1032) == (3, 384)
    assert LR.down_split(17, 4088) == (4, 1024) and LR.down_split(17, 4096) == (8, 512) and LR.down_split(17, 4104) == (7, 640)
    assert LR.down_split(8160, 1024)[0] == 4 and LR.down_split(8161, 1024)[0] == 1
    assert LR.wgrad_split(256, 520) == (1, 256) and LR.wgrad_split(257, 520) == (5, 64)
    assert LR.wgrad_split(2048, 520) == (32, 64) and LR.wgrad_split(2049, 520) == (17, 128)
    assert LR.wgrad_split(3076, 8) == (25, 128) and LR.wgrad_split(3076, 18944) == (2, 1600) and LR.wgrad_split(3076, 3584) == (10, 320)


# ---- gradient exchange over the adapter buffer --------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vila_amd import lora
        from vila_amd.train import GradReducer
        tr = lora.LoRATrainer(_tiny_model(), lora.LoraConfig(r=16), optimizer_state=False)
        flat = tr.flat
        flat.grads = flat.grads.float()            # gloo has no bf16 sum on every build; the layout logic is dtype-agnostic
        flat.grads.copy_(torch.randn(flat.numel, generator=torch.Generator().manual_seed(100 + rank)))
        red = GradReducer(flat)
        order = [lora.layer_prefix(i) for i in reversed(range(tr.cfg.llm.num_hidden_layers))] + ["mm_projector."]
        for pre in order:
            red.ready(pre)
        red.wait()
        want = sum(torch.randn(flat.numel, generator=torch.Generator().manual_seed(100 + r)) for r in range(world))
        covered = torch.zeros(flat.numel, dtype=torch.bool)
        for _, s, e in red.log:
            covered[s:e] = True
        q.put((rank, bool(covered.all()) and torch.allclose(flat.grads, want, atol=1e-5), len(red.log), flat.grads.sum().item()))
    finally:
        dist.destroy_process_group()


def test_adapter_gradient_allreduce_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert all(ok for _, ok, _, _ in res), res
    assert len({n for _, _, n, _ in res}) == 1 and res[0][2] == 3
    assert res[0][3] == res[1][3]                                                     # identical summed gradients on both ranks
