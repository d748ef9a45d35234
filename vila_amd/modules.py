"""Drop-in nn.Modules for the three builder seams of the reference:

    build_vision_tower  (llava/model/multimodal_encoder/builder.py:30)      -> HipSiglipVisionTower
    build_mm_projector  (llava/model/multimodal_projector/builder.py:27)    -> HipMultimodalProjector
    build_llm_and_tokenizer (llava/model/language_model/builder.py:64)      -> HipQwen2ForCausalLM

Each keeps the reference's parameter names/shapes so the three-folder checkpoints of
`llava_arch.py:158-204` load with `load_state_dict`, and keeps the reference's call contract
(`vision_tower(images) -> [B,N,C]`, `mm_projector(x) -> [B,N',H]`, `llm(inputs_embeds=..., labels=...)`,
`llm.generate(inputs_embeds=..., attention_mask=...)`).  All math runs in libvila_hip.so.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from types import SimpleNamespace
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, ops, synthetic
from ._lib import check
from .configs import IGNORE_INDEX, LlmConfig, VilaConfig, VisionConfig


# --------------------------------------------------------------------------------------------------------------
# parameter tree with the reference's names; q/k/v projections are views of one fused buffer
# --------------------------------------------------------------------------------------------------------------
def _register(root: nn.Module, dotted: str, param: nn.Parameter) -> None:
    parts = dotted.split(".")
    m = root
    for p in parts[:-1]:
        if not hasattr(m, p):
            m.add_module(p, nn.Module())
        m = getattr(m, p)
    m.register_parameter(parts[-1], param)


def _get(root: nn.Module, dotted: str) -> torch.Tensor:
    m = root
    for p in dotted.split("."):
        m = getattr(m, p)
    return m


def _fuse_groups(names: List[str]) -> Dict[str, Tuple[str, ...]]:
    """q_proj -> (q_proj, k_proj, v_proj) groups (weights and biases) that must be contiguous for the fused kernels."""
    groups = {}
    for n in names:
        if ".self_attn.q_proj." in n:
            groups[n] = (n, n.replace("q_proj", "k_proj"), n.replace("q_proj", "v_proj"))
    return groups


class _HipModule(nn.Module):
    """Builds parameters from (name, shape, kind) specs, caches the ctypes weight structs, owns a grow-only workspace."""

    _decode = None              # the LLM's batch-1 and batched decode sessions (`_decode_session`, `_batch_session`)
    _bdecode = None
    _vdecode = None             # the LLM's verify session (`_verify_session`: greedy speculative decoding)
    _bf16_released = False      # quantize_w4(release_bf16=True) freed the bf16 projection weights

    def _build_params(self, specs, prefix: str, device, dtype, requires_grad=False):
        names = [n for n, _, _ in specs]
        shapes = {n: s for n, s, _ in specs}
        groups = _fuse_groups(names)
        grouped = {m for g in groups.values() for m in g}
        self._fused_groups = [tuple(m[len(prefix):] for m in g) for g in groups.values()]
        for n, shape, _ in specs:
            if n in grouped:
                continue
            _register(self, n[len(prefix):], nn.Parameter(torch.empty(shape, device=device, dtype=dtype), requires_grad=requires_grad))
        for g in groups.values():
            rows = [shapes[m][0] for m in g]
            tail = shapes[g[0]][1:]
            buf = torch.empty((sum(rows), *tail), device=device, dtype=dtype)
            o = 0
            for m, r in zip(g, rows):
                _register(self, m[len(prefix):], nn.Parameter(buf[o:o + r], requires_grad=requires_grad))
                o += r
        self._cstruct = None
        self._ws = None

    def _drop_session(self, attr: str) -> None:
        """Destroy the session's captured graph, if it has one, and forget the session."""
        st = getattr(self, attr)
        if st is not None and getattr(st, "graph", None) is not None:
            _lib.load().vila_graph_destroy(st.graph)
            st.graph = None
        setattr(self, attr, None)

    def _drop_decode_session(self) -> None:
        self._drop_session("_decode")

    def _drop_batch_session(self) -> None:
        self._drop_session("_bdecode")

    def _invalidate(self) -> None:
        """Parameter storage moved (.to(), refuse(), FlatParams re-pointing, W4 quantisation): every cached object that baked in
        a weight pointer is dropped — the ctypes weight struct and, for the LLM, both decode sessions with their captured hipGraphs.
        (A batch-1 session whose cache / length / sampling key changed drops only ITSELF, `_decode_session`: the n-slot batch session
        with its KV cache and graph survives a server that alternates batched and solo requests — ADVICE round 3.)"""
        self._cstruct = None
        self._drop_decode_session()
        self._drop_batch_session()
        self._drop_session("_vdecode")

    def refuse(self) -> None:
        """Re-establish the fused q/k/v storage after an op that re-allocated parameters (.to(), .half(), ...)."""
        if self._bf16_released:
            raise RuntimeError("refuse: the bf16 projection weights were freed by quantize_w4(release_bf16=True); there is no q/k/v buffer to re-fuse")
        for g in self._fused_groups:
            ts = [_get(self, m) for m in g]
            buf = torch.cat([t.data for t in ts], 0)
            o = 0
            for t in ts:
                t.data = buf[o:o + t.shape[0]]
                o += t.shape[0]
        self._invalidate()

    def _apply(self, fn, *a, **k):
        if self._bf16_released:
            # .cuda() / .to() / .half() on a model whose bf16 projections were released: the int4 copies stay where they are, so only a
            # conversion that changes nothing is allowed (it leaves the model as it was); any other would split the model across devices / dtypes
            probe = torch.empty(0, device=self.device, dtype=self.dtype)
            t = fn(probe)
            if t.device == probe.device and t.dtype == probe.dtype:
                return self
            raise RuntimeError(f"cannot move or convert the model to {t.device} / {t.dtype}: its bf16 projection weights were freed by "
                               "quantize_w4(release_bf16=True) and its int4 copies stay on " + str(probe.device))
        r = super()._apply(fn, *a, **k)
        if getattr(self, "_fused_groups", None):
            self.refuse()
        self._invalidate()
        self._ws = None
        return r

    def load_weights(self, w: Dict[str, torch.Tensor], prefix: str) -> None:
        if self._bf16_released:
            raise RuntimeError("load_weights: the bf16 projection weights were freed by quantize_w4(release_bf16=True); build a new model")
        with torch.no_grad():
            for n, p in self.named_parameters():
                p.copy_(w[prefix + n])

    def _workspace(self, nbytes: int, device) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty((int(nbytes),), device=device, dtype=torch.uint8)
        return self._ws

    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def dtype(self):
        return next(self.parameters()).dtype


# --------------------------------------------------------------------------------------------------------------
# Vision tower
# --------------------------------------------------------------------------------------------------------------
class HipSiglipVisionTower(_HipModule):
    """`VisionTower.forward` + `feature_select` of llava/model/multimodal_encoder/vision_encoder.py:44-52,133-177 for
    SiglipVisionTower (siglip_encoder.py:25-63): images [B,3,H,W] -> hidden_states[select_layer] [B,N,C], "cls_patch"."""

    def __init__(self, cfg: VilaConfig, device="cuda", dtype=torch.bfloat16):
        super().__init__()
        self.cfg = cfg
        self.vcfg: VisionConfig = cfg.vision
        self.select_layer = cfg.vision.select_layer
        self.select_feature = "cls_patch"
        self.is_loaded = True
        self._build_params(synthetic.vision_specs(cfg), "vision_tower.", device, dtype)
        self.config = SimpleNamespace(hidden_size=cfg.vision.hidden_size, image_size=cfg.vision.image_size,
                                      patch_size=cfg.vision.patch_size)

    @property
    def hidden_size(self):
        return self.vcfg.hidden_size

    @property
    def num_patches(self):
        return self.vcfg.num_patches

    def _struct(self):
        if self._cstruct is None:
            v = self.vcfg
            vm = self.vision_tower.vision_model
            n_run = v.num_used_layers
            layers = (_lib.VilaVitLayer * max(n_run, 1))()
            for i in range(n_run):
                l = getattr(vm.encoder.layers, str(i))
                L = layers[i]
                L.ln1_w, L.ln1_b = l.layer_norm1.weight.data_ptr(), l.layer_norm1.bias.data_ptr()
                L.wq, L.bq = l.self_attn.q_proj.weight.data_ptr(), l.self_attn.q_proj.bias.data_ptr()
                L.wk, L.bk = l.self_attn.k_proj.weight.data_ptr(), l.self_attn.k_proj.bias.data_ptr()
                L.wv, L.bv = l.self_attn.v_proj.weight.data_ptr(), l.self_attn.v_proj.bias.data_ptr()
                L.wo, L.bo = l.self_attn.out_proj.weight.data_ptr(), l.self_attn.out_proj.bias.data_ptr()
                L.ln2_w, L.ln2_b = l.layer_norm2.weight.data_ptr(), l.layer_norm2.bias.data_ptr()
                L.fc1_w, L.fc1_b = l.mlp.fc1.weight.data_ptr(), l.mlp.fc1.bias.data_ptr()
                L.fc2_w, L.fc2_b = l.mlp.fc2.weight.data_ptr(), l.mlp.fc2.bias.data_ptr()
            w = _lib.VilaVitWeights()
            w.shape = _lib.VilaVitShape(v.hidden_size, v.intermediate_size, v.num_attention_heads, v.image_size, v.patch_size,
                                        v.num_channels, n_run, v.layer_norm_eps)
            w.patch_w = vm.embeddings.patch_embedding.weight.data_ptr()
            w.patch_b = vm.embeddings.patch_embedding.bias.data_ptr()
            w.pos_emb = vm.embeddings.position_embedding.weight.data_ptr()
            w.layers = C.cast(layers, C.POINTER(_lib.VilaVitLayer))
            self._cstruct = (w, layers)
        return self._cstruct[0]

    def quantize_w8(self):
        """W8A8 (BASELINE configs[4]): build int8 per-channel copies of the encoder linears; forward() then runs
        `vila_vit_forward_w8a8` (int8 x int8 matrix-core GEMMs with per-token dynamic activation scales)."""
        from .quant import W8VitWeights
        self._w8 = W8VitWeights(self)
        return self._w8

    @torch.no_grad()
    def forward(self, images: torch.Tensor) -> torch.Tensor:
        if isinstance(images, list):
            images = torch.stack(images, 0)
        ops._need(images, dtype=None, name="images")
        v = self.vcfg
        if images.shape[1:] != (v.num_channels, v.image_size, v.image_size):
            raise ValueError(f"Input image size ({images.shape[2]}*{images.shape[3]}) doesn't match model ({v.image_size}*{v.image_size}).")
        x = images.to(self.dtype).contiguous()
        Bn = x.shape[0]
        lib = _lib.load()
        w = self._struct()
        out = torch.empty((Bn, v.num_patches, v.hidden_size), device=x.device, dtype=self.dtype)
        w8 = getattr(self, "_w8", None)
        if w8 is not None:
            ws = self._workspace(lib.vila_vit_w8a8_workspace_bytes(C.byref(w.shape), Bn), x.device)
            check(lib.vila_vit_forward_w8a8(C.byref(w), w8.ptr, x.data_ptr(), Bn, out.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()),
                  "vila_vit_forward_w8a8")
            return out.to(images.dtype) if images.dtype in (torch.float16, torch.bfloat16) else out
        ws = self._workspace(lib.vila_vit_workspace_bytes(C.byref(w.shape), Bn), x.device)
        check(lib.vila_vit_forward(C.byref(w), x.data_ptr(), Bn, out.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "vila_vit_forward")
        return out.to(images.dtype) if images.dtype in (torch.float16, torch.bfloat16) else out


# --------------------------------------------------------------------------------------------------------------
# Projector
# --------------------------------------------------------------------------------------------------------------
_PROJ_KIND = {"mlp_downsample": 0, "mlp_downsample_2x2_fix": 1, "mlp_downsample_3x3_fix": 2}


class HipMultimodalProjector(_HipModule):
    """`MultimodalProjector.forward` (llava/model/multimodal_projector/base_projector.py:248-252)."""

    def __init__(self, cfg: VilaConfig, device="cuda", dtype=torch.bfloat16):
        super().__init__()
        if cfg.mm_projector_type not in _PROJ_KIND:
            raise ValueError(f"Unknown projector type: {cfg.mm_projector_type}")
        self.cfg = cfg
        self.downsample_rate = cfg.downsample
        self._build_params(synthetic.projector_specs(cfg), "mm_projector.", device, dtype)

    def _struct(self):
        if self._cstruct is None:
            L = self.layers
            w = _lib.VilaProjWeights()
            w.kind = _PROJ_KIND[self.cfg.mm_projector_type]
            w.in_dim, w.out_dim = self.cfg.mm_hidden_size, self.cfg.llm.hidden_size   # dynamic_s2: C * n_scales
            g = lambda i, n: getattr(getattr(L, str(i)), n).data_ptr()
            w.ln1_w, w.ln1_b, w.fc1_w, w.fc1_b = g(1, "weight"), g(1, "bias"), g(2, "weight"), g(2, "bias")
            if w.kind == 2:
                w.ln2_w, w.ln2_b, w.fc2_w, w.fc2_b, w.fc3_w, w.fc3_b = (g(4, "weight"), g(4, "bias"), g(5, "weight"), g(5, "bias"),
                                                                        g(7, "weight"), g(7, "bias"))
            else:
                w.fc2_w, w.fc2_b = g(4, "weight"), g(4, "bias")
            self._cstruct = (w,)
        return self._cstruct[0]

    @torch.no_grad()
    def forward(self, x: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        ops._need(x, dtype=None, name="features")
        xin = x.to(self.dtype).contiguous()
        Bn, N, _ = xin.shape
        lib = _lib.load()
        w = self._struct()
        ws = self._workspace(lib.vila_proj_workspace_bytes(C.byref(w), Bn, N), xin.device)
        No = lib.vila_proj_out_tokens(w.kind, N)
        out = torch.empty((Bn, No, self.cfg.llm.hidden_size), device=xin.device, dtype=self.dtype)
        check(lib.vila_proj_forward(C.byref(w), xin.data_ptr(), Bn, N, out.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "vila_proj_forward")
        return out


# --------------------------------------------------------------------------------------------------------------
# LLM
# --------------------------------------------------------------------------------------------------------------
def _as_i64(u: int) -> int:
    """uint64 bit pattern -> the int64 holding the same bits (torch has no uint64 fill)."""
    u = int(u) & 0xFFFFFFFFFFFFFFFF
    return u - (1 << 64) if u >= (1 << 63) else u


def _step_symbols(batch: bool, w4: bool, sampled: bool, verify: bool = False, verify_sample: bool = False, prefix: bool = False,
                  penalized: bool = False, constrained: bool = False, any_k: bool = False, processed: bool = False, lora: bool = False) -> Tuple[str, str]:
    """(step, workspace query) of one decode step variant, composed the way the C ABI names them.  verify: the greedy verify step, whatever `batch`.
    verify_sample: the sampled verify step, whatever `batch`, `sampled` and `verify` — a spelling of its own, since `verify` with `sampled` stays the
    refusal it always was (that pair names the greedy step asked to sample).  prefix: the batched step of a session with a shared prompt prefix
    (its workspace query takes the capacity and has no `_ctx` twin).  penalized: the step with repetition / presence / frequency penalties in front
    of its pick — ONE entry per driver, which takes the int4 layers, the sampling parameters and (batched) the prefix descriptor as nullable arguments,
    so w4 / sampled / prefix do not change the names.  constrained: the step with a token automaton per row between the penalties and the pick —
    ONE entry per driver as well, which takes the penalties as a nullable argument too, so `penalized` does not change the names either.
    any_k: the sampled pick that serves every top_k >= 0 — ONE entry for the batched step (int4 layers, prefix, penalties and automata nullable, so
    none of them changes the names) and one for the sampled verify step (int4 layers nullable).  It is an option of a sampled pick: the greedy
    steps and the solo step (whose sampler serves any top_k already) have no such form.
    processed: the verify step with penalties / an automaton in front of its pick and logprob records behind its accept — ONE entry for the verify steps
    (int4 layers, sampling parameters, the any_k option, penalties, automaton and records all arguments of it, so none of them changes the names).  A
    spelling of its own: `verify` / `verify_sample` with `penalized` or `constrained` stay the refusals they always were.
    lora: the batched step with a per-row LoRA adapter (`vila_amd.lora_serving.AdapterBank`) — ONE entry, which takes the sampling parameters, the any_k
    option, penalties and automata as nullable arguments, so none of them changes the names.  The adapters add to bf16 projections of rows with caches
    of their own: int4 layers, a shared prefix, the verify steps and the solo step have no such form."""
    if lora:
        if w4:
            raise ValueError("the step with per-row adapters has no int4 form: the adapters add to bf16 projections")
        if prefix:
            raise ValueError("the step with per-row adapters has no shared-prefix form")
        if verify or verify_sample or processed:
            raise ValueError("the verify steps have no adapter form")
        if not batch:
            raise ValueError("the step with per-row adapters is a batched step: the solo step has no adapter form")
        return "vila_llm_decode_step_batch_lora", "vila_llm_decode_batch_lora_workspace_bytes"
    if processed:
        if not (verify or verify_sample) or prefix:
            raise ValueError("the processed step is a verify step")
        return "vila_llm_decode_step_verify_processed", "vila_llm_decode_verify_processed_workspace_bytes"
    if any_k:
        if verify_sample:
            if penalized or constrained or prefix:
                raise ValueError("the verify steps have no penalised, constrained or shared-prefix form")
            return "vila_llm_decode_step_verify_any_k", "vila_llm_decode_verify_sample_workspace_bytes"
        if verify or not batch or not sampled:
            raise ValueError("any top_k is an option of the sampled batched step and of the sampled verify step")
        return "vila_llm_decode_step_batch_any_k", "vila_llm_decode_batch_any_k_workspace_bytes"
    if constrained:
        if verify or verify_sample:
            raise ValueError("the verify steps have no constrained form")
        if prefix and not batch:
            raise ValueError("the shared-prefix step is a batched step")
        return (("vila_llm_decode_step_batch_constrained", "vila_llm_decode_batch_constrained_workspace_bytes") if batch else
                ("vila_llm_decode_step_constrained", "vila_llm_decode_constrained_workspace_bytes"))
    if penalized:
        if verify or verify_sample:
            raise ValueError("the verify steps have no penalised form")
        if prefix and not batch:
            raise ValueError("the shared-prefix step is a batched step")
        return (("vila_llm_decode_step_batch_penalized", "vila_llm_decode_batch_penalized_workspace_bytes") if batch else
                ("vila_llm_decode_step_penalized", "vila_llm_decode_penalized_workspace_bytes"))
    if prefix:
        if not batch or verify or verify_sample:
            raise ValueError("the shared-prefix step is a batched step")
        tail = ("_w4" if w4 else "") + ("_sample" if sampled else "")
        return "vila_llm_decode_step_batch_prefix" + tail, "vila_llm_decode_batch_prefix" + tail + "_workspace_bytes"
    if verify_sample:
        tail = ("_w4" if w4 else "") + "_sample"
        return "vila_llm_decode_step_verify" + tail, "vila_llm_decode_verify_sample_workspace_bytes"
    if verify and sampled:
        raise ValueError("the verify step is greedy: it has no sampled variant")
    tail = ("_w4" if w4 else "") + ("_sample" if sampled else "")
    if verify:
        return "vila_llm_decode_step_verify" + tail, "vila_llm_decode_verify_workspace_bytes"
    if batch:
        return "vila_llm_decode_step_batch" + tail, "vila_llm_decode_batch" + tail + "_workspace_bytes_ctx"
    return "vila_llm_decode_step" + tail, "vila_llm_decode_workspace_bytes"


def _capture(st, step, restore) -> None:
    """Capture `step()` on st.stream into st.graph.  The step runs once outside capture first (kernel attributes cannot be set while
    capturing); `restore()` then puts back the state that warm-up advanced, so the captured step starts where the caller left it."""
    lib = _lib.load()
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(st.stream):
        step()
        st.stream.synchronize()
        restore()
        check(lib.vila_graph_begin(st.stream.cuda_stream), "graph_begin")
        step()
        g = C.c_void_p()
        check(lib.vila_graph_end(st.stream.cuda_stream, C.byref(g)), "graph_end")
        st.graph = g
        st.stream.synchronize()


def _replay(st, k: int) -> None:
    """k launches of st.graph on st.stream.  The caller has made st.stream current and does its own syncs."""
    lib = _lib.load()
    for _ in range(int(k)):
        check(lib.vila_graph_launch(st.graph, st.stream.cuda_stream), "graph_launch")


def _stream_put(streamer, t: int) -> None:
    """One new token to an HF streamer (`put(LongTensor[1])`), if there is one."""
    if streamer is not None:
        streamer.put(torch.tensor([t], dtype=torch.int64))


def _eos_set(eos_token_id, default=None) -> set:
    """The ids that end a row: one id or a list of them, `default` (the config's EOS) where none is given."""
    eos = default if eos_token_id is None else eos_token_id
    return set(eos) if isinstance(eos, (list, tuple)) else {eos}


def _pad_id(pad_token_id, eos_token_id, config_eos) -> int:
    """HF's pad rule: pad_token_id, else the first EOS given, else the config's EOS."""
    eos1 = eos_token_id[0] if isinstance(eos_token_id, (list, tuple)) else eos_token_id
    return int(pad_token_id if pad_token_id is not None else (eos1 if eos1 is not None else config_eos))


def _cut_at_eos(row: List[int], eos_set) -> List[int]:
    """HF stops a row AFTER emitting eos."""
    return row[:next((i + 1 for i, t in enumerate(row) if t in eos_set), len(row))]


def finish_rows(rows: List[List[int]], eos_set, pad: int, device) -> torch.Tensor:
    """Token lists -> [B, n] int64 like HF: each row cut after its first EOS, right-padded with `pad` to the longest."""
    rows = [_cut_at_eos(r, eos_set) for r in rows]
    n = max(len(r) for r in rows)
    return torch.tensor([r + [int(pad)] * (n - len(r)) for r in rows], dtype=torch.int64, device=device)


class Logprobs(NamedTuple):
    """What `generate(logprobs=k)` returns beside the ids [B, n_new] (and `batch_logprobs` / `score` for one row): RAW log-probabilities, i.e. of the
    model's own distribution, independent of temperature, top-k, top-p and penalties.  Pad positions behind a row's EOS hold 0.0 / -inf / -1."""
    token_logprobs: torch.Tensor        # [B, n_new] fp32: the logprob of the token at that position
    top_logprobs: torch.Tensor          # [B, n_new, k] fp32: the k most likely tokens' logprobs, descending, ties towards the lower id
    top_ids: torch.Tensor               # [B, n_new, k] int64: their ids


class CausalLMOutput(SimpleNamespace):
    """Fields of HF CausalLMOutputWithPast that llava_llama.py:134-159 consumes."""


class HipQwen2ForCausalLM(_HipModule):
    """HF `Qwen2ForCausalLM` as used at llava_llama.py:134-141 (`forward`) and llava_arch.py:833 (`generate`)."""

    _w4 = None                  # quant.W4Weights once quantize_w4 ran; the two flags say which other paths read it
    _w4_prefill = False
    _w4_batch = False
    _own_cache = None           # generate()'s KV cache, kept across calls
    _sample_calls = 0

    def __init__(self, cfg: VilaConfig, device="cuda", dtype=torch.bfloat16):
        super().__init__()
        self.cfg = cfg
        self.lcfg: LlmConfig = cfg.llm
        self._build_params(synthetic.llm_specs(cfg), "llm.", device, dtype)
        self.config = SimpleNamespace(hidden_size=cfg.llm.hidden_size, vocab_size=cfg.llm.vocab_size,
                                      eos_token_id=cfg.llm.eos_token_id, tie_word_embeddings=cfg.llm.tie_word_embeddings)
        # `llm.model.embed_tokens(ids)` is called directly by the reference (llava_arch.py:429, encoders/image/basic.py:27)
        emb = self.model.embed_tokens
        emb.forward = lambda ids, _w=emb: ops.embed_tokens(_w.weight, ids)

    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        return ops.embed_tokens(self.model.embed_tokens.weight, ids)

    def _struct(self):
        if self._cstruct is None:
            c = self.lcfg
            layers = (_lib.VilaLlmLayer * c.num_hidden_layers)()
            for i in range(c.num_hidden_layers):
                l = getattr(self.model.layers, str(i))
                L = layers[i]
                L.ln1_w = l.input_layernorm.weight.data_ptr()
                L.wq, L.bq = l.self_attn.q_proj.weight.data_ptr(), l.self_attn.q_proj.bias.data_ptr()
                L.wk, L.bk = l.self_attn.k_proj.weight.data_ptr(), l.self_attn.k_proj.bias.data_ptr()
                L.wv, L.bv = l.self_attn.v_proj.weight.data_ptr(), l.self_attn.v_proj.bias.data_ptr()
                L.wo = l.self_attn.o_proj.weight.data_ptr()
                L.ln2_w = l.post_attention_layernorm.weight.data_ptr()
                L.w_gate, L.w_up, L.w_down = l.mlp.gate_proj.weight.data_ptr(), l.mlp.up_proj.weight.data_ptr(), l.mlp.down_proj.weight.data_ptr()
            w = _lib.VilaLlmWeights()
            w.shape = _lib.VilaLlmShape(c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads,
                                        c.num_key_value_heads, c.head_dim, c.vocab_size, c.rms_norm_eps, c.rope_theta)
            w.embed = self.model.embed_tokens.weight.data_ptr()
            w.layers = C.cast(layers, C.POINTER(_lib.VilaLlmLayer))
            w.norm_w = self.model.norm.weight.data_ptr()
            w.lm_head = (self.model.embed_tokens.weight if c.tie_word_embeddings else self.lm_head.weight).data_ptr()
            self._cstruct = (w, layers)
        return self._cstruct[0]

    # ---- KV cache ---------------------------------------------------------------------------------------
    def new_cache(self, max_ctx: int, n_slots: int = 1):
        c = self.lcfg
        shape = (c.num_hidden_layers, n_slots, c.num_key_value_heads, max_ctx, c.head_dim)
        with torch.inference_mode(False):        # caches are reused across calls (generate() keeps `_own_cache`)
            k = torch.zeros(shape, device=self.device, dtype=self.dtype)
            v = torch.zeros(shape, device=self.device, dtype=self.dtype)
        cs = _lib.VilaKvCache(k.data_ptr(), v.data_ptr(), max_ctx, n_slots)
        return SimpleNamespace(k=k, v=v, c=cs, max_ctx=max_ctx, n_slots=n_slots)

    # ---- packed prefill -------------------------------------------------------------------------------------
    @torch.no_grad()
    def prefill_packed(self, embeds: torch.Tensor, positions: torch.Tensor, cu_seqlens: Optional[torch.Tensor], max_seqlen: int,
                       cache=None, seq_of_tok: Optional[torch.Tensor] = None, last_rows: Optional[torch.Tensor] = None,
                       want_all_logits: bool = False, want_final_hidden: bool = False, want_layer_hidden: bool = False, adapter: Optional[str] = None,
                       adapters=None):
        """embeds [T,H] bf16 packed stream.  Returns a namespace with last_logits / all_logits / final_hidden / layer_hidden.
        adapter=name with adapters=bank (`vila_amd.lora_serving.AdapterBank`): every packed sequence runs under that adapter of the bank, unmerged
        (`vila_llm_prefill_lora`: the trainer's forward dataflow, t and u rounded to bf16); bf16 models, no layer_hidden."""
        ops._need(embeds, name="inputs_embeds")
        if adapter is not None:
            return self._prefill_packed_lora(embeds, positions, cu_seqlens, max_seqlen, cache, seq_of_tok, last_rows, want_all_logits, want_final_hidden,
                                             want_layer_hidden, adapter, adapters)
        c = self.lcfg
        T = embeds.shape[0]
        dev = embeds.device
        lib = _lib.load()
        w = self._struct()
        w4 = self._w4 if self._w4_prefill else None
        if w4 is None:
            self._require_bf16("the bf16 prefill")
        ws_bytes = (lib.vila_llm_prefill_w4_workspace_bytes if w4 is not None else lib.vila_llm_prefill_workspace_bytes)(C.byref(w.shape), T)
        ws = self._workspace(ws_bytes, dev)
        n_seq = 1 if cu_seqlens is None else cu_seqlens.numel() - 1
        n_last = 0 if last_rows is None else last_rows.numel()
        last_logits = torch.empty((n_last, c.vocab_size), device=dev, dtype=torch.float32) if n_last else None
        all_logits = torch.empty((T, c.vocab_size), device=dev, dtype=torch.float32) if want_all_logits else None
        final_hidden = torch.empty((T, c.hidden_size), device=dev, dtype=self.dtype) if want_final_hidden else None
        layer_hidden = torch.empty((c.num_hidden_layers + 1, T, c.hidden_size), device=dev, dtype=self.dtype) if want_layer_hidden else None
        args = (embeds.contiguous().data_ptr(), positions.data_ptr(), ops._p(cu_seqlens), n_seq, T, int(max_seqlen), ops._p(seq_of_tok),
                C.byref(cache.c) if cache is not None else None, ops._p(last_rows), n_last, ops._p(last_logits), ops._p(all_logits),
                ops._p(final_hidden), ops._p(layer_hidden), ws.data_ptr(), ws.numel(), ops._stream())
        if w4 is not None:
            check(lib.vila_llm_prefill_w4(C.byref(w), w4.ptr, *args), "vila_llm_prefill_w4")
        else:
            check(lib.vila_llm_prefill(C.byref(w), *args), "vila_llm_prefill")
        return SimpleNamespace(last_logits=last_logits, all_logits=all_logits, final_hidden=final_hidden, layer_hidden=layer_hidden)

    def _prefill_packed_lora(self, embeds, positions, cu_seqlens, max_seqlen, cache, seq_of_tok, last_rows, want_all_logits, want_final_hidden,
                             want_layer_hidden, adapter, adapters):
        if adapters is None:
            raise ValueError("prefill_packed(adapter=): pass the bank that holds the adapter as adapters=")
        if self._w4 is not None or want_layer_hidden:
            raise ValueError("prefill_packed(adapter=): the prefill under an adapter serves bf16 models and returns no layer_hidden")
        self._require_bf16("the prefill under an adapter")
        c, T, dev, lib, w = self.lcfg, embeds.shape[0], embeds.device, _lib.load(), self._struct()
        layers, r, scale = adapters.c_prefill(adapter)
        ws = self._workspace(lib.vila_llm_prefill_lora_workspace_bytes(C.byref(w.shape), T, r), dev)
        n_seq = 1 if cu_seqlens is None else cu_seqlens.numel() - 1
        n_last = 0 if last_rows is None else last_rows.numel()
        last_logits = torch.empty((n_last, c.vocab_size), device=dev, dtype=torch.float32) if n_last else None
        all_logits = torch.empty((T, c.vocab_size), device=dev, dtype=torch.float32) if want_all_logits else None
        final_hidden = torch.empty((T, c.hidden_size), device=dev, dtype=self.dtype) if want_final_hidden else None
        check(lib.vila_llm_prefill_lora(C.byref(w), layers, r, scale, embeds.contiguous().data_ptr(), positions.data_ptr(), ops._p(cu_seqlens), n_seq, T,
                                        int(max_seqlen), ops._p(seq_of_tok), C.byref(cache.c) if cache is not None else None, ops._p(last_rows), n_last,
                                        ops._p(last_logits), ops._p(all_logits), ops._p(final_hidden), ws.data_ptr(), ws.numel(), ops._stream()),
              "vila_llm_prefill_lora")
        return SimpleNamespace(last_logits=last_logits, all_logits=all_logits, final_hidden=final_hidden, layer_hidden=None)

    # ---- prefill onto a live cache ----------------------------------------------------------------------------
    @torch.no_grad()
    def prefill_append(self, embeds: torch.Tensor, cache, past: int, slot: int = 0, last_rows: Optional[torch.Tensor] = None,
                       want_final_hidden: bool = False, want_layer_hidden: bool = False, adapter: Optional[str] = None):
        """embeds [T,H] bf16: T tokens of ONE sequence appended to `slot` of `cache`, which holds `past` positions.  They take positions
        past .. past + T - 1, their K/V are written there and every row attends the slot's keys 0 .. its own position.  last_rows counts rows
        inside these T tokens.  Returns the namespace of `prefill_packed` (all_logits is None).  The W4 route is taken as there.
        adapter: must be None — the append prefill has no form under an unmerged adapter (prefill_packed(adapter=) has)."""
        if adapter is not None:
            raise ValueError("prefill_append: the append prefill (follow-up turns, prefill_chunk, ChatSession) does not run under an unmerged adapter; "
                             "prefill the whole prompt with prefill_packed(adapter=) / batch_admit(adapter=)")
        ops._need(embeds, name="inputs_embeds")
        c = self.lcfg
        if embeds.dim() != 2 or embeds.shape[1] != c.hidden_size:
            raise ValueError(f"prefill_append: embeds must be [T, {c.hidden_size}] (got {tuple(embeds.shape)})")
        T, past, slot = embeds.shape[0], int(past), int(slot)
        if cache is None:
            raise ValueError("prefill_append: a KV cache that holds the sequence's first `past` positions is required")
        if T < 1 or past < 0 or past + T > cache.max_ctx:
            raise ValueError(f"prefill_append: past ({past}) + T ({T}) must fit the KV cache ({cache.max_ctx} positions), T >= 1, past >= 0")
        if not 0 <= slot < cache.n_slots:
            raise ValueError(f"prefill_append: slot {slot} outside the cache's {cache.n_slots} slots")
        dev = embeds.device
        lib = _lib.load()
        w = self._struct()
        w4 = self._w4 if self._w4_prefill else None
        if w4 is None:
            self._require_bf16("the bf16 prefill")
        ws_bytes = (lib.vila_llm_prefill_append_w4_workspace_bytes if w4 is not None else lib.vila_llm_prefill_append_workspace_bytes)(C.byref(w.shape), T)
        ws = self._workspace(ws_bytes, dev)
        n_last = 0 if last_rows is None else last_rows.numel()
        last_logits = torch.empty((n_last, c.vocab_size), device=dev, dtype=torch.float32) if n_last else None
        final_hidden = torch.empty((T, c.hidden_size), device=dev, dtype=self.dtype) if want_final_hidden else None
        layer_hidden = torch.empty((c.num_hidden_layers + 1, T, c.hidden_size), device=dev, dtype=self.dtype) if want_layer_hidden else None
        args = (embeds.contiguous().data_ptr(), T, past, slot, C.byref(cache.c), ops._p(last_rows), n_last, ops._p(last_logits), ops._p(final_hidden),
                ops._p(layer_hidden), ws.data_ptr(), ws.numel(), ops._stream())
        if w4 is not None:
            check(lib.vila_llm_prefill_append_w4(C.byref(w), w4.ptr, *args), "vila_llm_prefill_append_w4")
        else:
            check(lib.vila_llm_prefill_append(C.byref(w), *args), "vila_llm_prefill_append")
        return SimpleNamespace(last_logits=last_logits, all_logits=None, final_hidden=final_hidden, layer_hidden=layer_hidden)

    # ---- HF-style forward (inference logits / loss; no autograd here: training goes through vila_amd.train) ----
    @torch.no_grad()
    def forward(self, input_ids=None, inputs_embeds: Optional[torch.Tensor] = None, attention_mask: Optional[torch.Tensor] = None,
                position_ids: Optional[torch.Tensor] = None, past_key_values=None, labels: Optional[torch.Tensor] = None,
                seqlens_in_batch: Optional[torch.Tensor] = None, num_items_in_batch: Optional[int] = None, **kw):
        if inputs_embeds is None:
            inputs_embeds = self.embed_tokens(input_ids)
        Bn, S, H = inputs_embeds.shape
        dev = inputs_embeds.device
        if seqlens_in_batch is not None:
            # packed row from repack_multimodal_data (llava_arch.py:744-800); packing.py:12-21 semantics
            assert Bn == 1
            seqlens = seqlens_in_batch.to(device=dev, dtype=torch.int32)
            keep = attention_mask[0].bool() if attention_mask is not None else torch.ones(S, dtype=torch.bool, device=dev)
        else:
            mask = attention_mask.bool() if attention_mask is not None else torch.ones((Bn, S), dtype=torch.bool, device=dev)
            seqlens = mask.sum(1).to(torch.int32)
            keep = mask.reshape(-1)
        idx = torch.nonzero(keep, as_tuple=False).flatten()
        flat = inputs_embeds.reshape(Bn * S, H)
        packed = flat.index_select(0, idx).to(self.dtype)
        cu = torch.zeros(seqlens.numel() + 1, device=dev, dtype=torch.int32)
        cu[1:] = torch.cumsum(seqlens, 0)
        if position_ids is not None:
            pos = position_ids.reshape(-1).index_select(0, idx).to(torch.int32)
        else:
            seq_id = torch.repeat_interleave(torch.arange(seqlens.numel(), device=dev), seqlens.long())
            pos = (torch.arange(idx.numel(), device=dev, dtype=torch.int32) - cu[:-1][seq_id]).to(torch.int32)
        want_logits = labels is None or bool(kw.get("return_logits", False))
        r = self.prefill_packed(packed, pos, cu, int(seqlens.max()), want_all_logits=want_logits, want_final_hidden=labels is not None)
        logits = None
        if want_logits:
            logits = torch.zeros((Bn * S, self.lcfg.vocab_size), device=dev, dtype=torch.float32)
            logits.index_copy_(0, idx, r.all_logits)
            logits = logits.view(Bn, S, -1)
        loss = None
        if labels is not None:
            # HF ForCausalLMLoss: position t predicts labels[t+1] inside each row; only rows WITH a target go through the head:
            # gather -> [n_valid, V] fp32 logits -> ce_kernel (no [B*S, V] tensor, no torch loss kernels on this path)
            lb = labels.to(dev)
            tgt = torch.full((Bn, S), IGNORE_INDEX, dtype=torch.int64, device=dev)
            tgt[:, :-1] = lb[:, 1:]
            inv = torch.full((Bn * S,), -1, dtype=torch.int64, device=dev)
            inv[idx] = torch.arange(idx.numel(), device=dev)
            tgt = tgt.reshape(-1)
            ok = (tgt != IGNORE_INDEX) & (inv >= 0)
            rows = inv[ok].to(torch.int32)
            n_valid = int(rows.numel())
            acc = torch.zeros((1,), device=dev, dtype=torch.float32)
            if n_valid:
                hv = torch.empty((n_valid, H), device=dev, dtype=self.dtype)
                ops.copy_rows(r.final_hidden, hv, rows, None, n_valid)
                head = self.model.embed_tokens.weight if self.lcfg.tie_word_embeddings else self.lm_head.weight
                lg = ops.gemm(hv, head, out_f32=True)
                denom = n_valid if num_items_in_batch is None else int(num_items_in_batch)
                ops.ce_loss(lg, tgt[ok].contiguous(), acc, 1.0 / max(denom, 1))
                loss = acc[0]
            else:
                loss = acc[0] * float("nan") if num_items_in_batch is None else acc[0]     # F.cross_entropy(mean) of no targets is nan
        return CausalLMOutput(loss=loss, logits=logits, past_key_values=None)

    # ---- greedy generate ---------------------------------------------------------------------------------------
    def _weights_key(self) -> tuple:
        """The weight storage a captured graph bakes in: embedding, layer 0's down_proj, the batched int4 down buffer (a re-quantise moves it) or None."""
        q4 = self._w4.mats[0]["down"].q.data_ptr() if self._w4_batched() else None
        return self.model.embed_tokens.weight.data_ptr(), _get(self, "model.layers.0.mlp.down_proj.weight").data_ptr(), q4

    @staticmethod
    def _check_penalties(repetition_penalty, presence_penalty, frequency_penalty):
        """generate()'s three penalties -> None where all are neutral (1, 0, 0 or None: today's path) or (rep, pres, freq) floats.  rep must be > 0
        (HF RepetitionPenaltyLogitsProcessor's error); pres and freq may be any finite float, negative ones reward repeats."""
        rep = 1.0 if repetition_penalty is None else repetition_penalty
        if not isinstance(rep, numbers.Real) or isinstance(rep, bool) or not rep > 0:
            raise ValueError(f"`penalty` has to be a strictly positive float, but is {rep}")
        pres = 0.0 if presence_penalty is None else float(presence_penalty)
        freq = 0.0 if frequency_penalty is None else float(frequency_penalty)
        for name, v in (("repetition_penalty", float(rep)), ("presence_penalty", pres), ("frequency_penalty", freq)):
            if not math.isfinite(v):
                raise ValueError(f"`{name}` has to be a finite float, but is {v}")
        return None if (float(rep), pres, freq) == (1.0, 0.0, 0.0) else (float(rep), pres, freq)

    @staticmethod
    def _penalty_state(st, n: int, vocab: int, dev) -> None:
        """What a session with the `penalties` flag owns: the count table (uint16 bits, one row per sequence) and the three parameter arrays, neutral.
        The values live here, on the device, never in the session key: one captured graph serves any of them."""
        st.counts = torch.zeros((n, vocab), device=dev, dtype=torch.int16)
        st.p_rep = torch.ones(n, device=dev, dtype=torch.float32)
        st.p_pres = torch.zeros(n, device=dev, dtype=torch.float32)
        st.p_freq = torch.zeros(n, device=dev, dtype=torch.float32)
        st.pen = _lib.VilaPenalties(st.p_rep.data_ptr(), st.p_pres.data_ptr(), st.p_freq.data_ptr(), st.counts.data_ptr(), vocab)

    @staticmethod
    def _set_penalties(st, slot: int, penalties) -> None:
        """A request starts in row `slot` of a penalised session: its (rep, pres, freq) — None = neutral — go to the device arrays and its counts to zero."""
        rep, pres, freq = (1.0, 0.0, 0.0) if penalties is None else penalties
        st.p_rep[slot:slot + 1].fill_(float(rep))
        st.p_pres[slot:slot + 1].fill_(float(pres))
        st.p_freq[slot:slot + 1].fill_(float(freq))
        st.counts[slot].zero_()

    CONSTRAIN_MAX_STATES, CONSTRAIN_MAX_CLASSES = 512, 4096          # the table a session of generate(constraint=) holds per row (batch_open: arguments)

    @staticmethod
    def _constraint_caps(max_states, max_classes) -> Tuple[int, int]:
        ms, mc = int(max_states), int(max_classes)
        cap = int(_lib.load().vila_logits_constrain_max_classes())
        if not 1 <= ms <= 32767 or not 1 <= mc <= cap:
            raise ValueError(f"constraints: max_states has to be in 1..32767 and max_classes in 1..{cap} (got {ms}, {mc})")
        return ms, mc

    @staticmethod
    def _constraint_state(st, n: int, vocab: int, caps: Tuple[int, int], dev) -> None:
        """What a session with the `constraints` flag owns: per row the automaton's state (-1 = unconstrained), the class of every token id, the table
        (max_states x max_classes int16 entries; a row's automaton lies in it row-major with its OWN class count) and the class count.  The automata
        live here, on the device, never in the session key: one captured graph serves any of them."""
        ld = (vocab + 3) // 4 * 4                                    # (class rows 8-byte aligned: the launch moves 4 classes per access)
        st.con_state = torch.full((n,), -1, device=dev, dtype=torch.int32)
        st.con_cls = torch.zeros((n, ld), device=dev, dtype=torch.int16)
        st.con_next = torch.full((n, caps[0] * caps[1]), -1, device=dev, dtype=torch.int16)
        st.con_nc = torch.ones(n, device=dev, dtype=torch.int32)
        st.con_caps, st.con_auto = caps, [None] * n
        st.con = _lib.VilaConstraints(st.con_state.data_ptr(), st.con_cls.data_ptr(), ld, st.con_next.data_ptr(), caps[0] * caps[1], st.con_nc.data_ptr())

    def _check_constraint(self, constraint, what: str):
        from .constrain import Automaton
        if not isinstance(constraint, Automaton):
            raise ValueError(f"{what}: constraint has to be a vila_amd.constrain.Automaton (compile_automaton / ConstraintCompiler), got {type(constraint).__name__}")
        if constraint.vocab != self.lcfg.vocab_size:
            raise ValueError(f"{what}: the automaton was compiled for a vocabulary of {constraint.vocab}, the model has {self.lcfg.vocab_size} "
                             "(token_bytes_from_tokenizer(tokenizer, vocab_size=...) pads the tokenizer's)")
        return constraint

    def _set_constraint(self, st, slot: int, constraint) -> None:
        """A request starts in row `slot` of a constrained session: None = an unconstrained row (state -1); else the automaton's classes and table go
        to the row (unless the row holds that very automaton already) and its state to the start.  The host binds the device contents here: the
        table must fit the row, and every state and class in it lies inside the table by construction (`compile_automaton`)."""
        if constraint is None:
            st.con_state[slot:slot + 1].fill_(-1)
            return
        a = self._check_constraint(constraint, "constraint")
        S, Cn = a.n_states, a.n_classes
        if Cn > st.con_caps[1] or S * Cn > st.con_caps[0] * st.con_caps[1]:
            raise ValueError(f"constraint: the automaton's table ({S} states x {Cn} classes = {S * Cn} entries) does not fit the session's "
                             f"{st.con_caps[0] * st.con_caps[1]} table entries per row (max_states x max_classes) with at most {st.con_caps[1]} classes: "
                             "open it with larger max_states / max_classes")
        if not (0 <= a.start < S and int(a.next.max()) < S and int(a.cls.max()) < Cn):
            raise ValueError("constraint: the automaton's table points outside itself")
        if st.con_auto[slot] is not a:
            dev = st.con_state.device
            st.con_auto[slot] = None
            st.con_cls[slot, :a.vocab].copy_(torch.from_numpy(a.cls.view("int16")).to(dev))
            st.con_next[slot, :S * Cn].copy_(torch.from_numpy(a.next.reshape(-1)).to(dev))
            st.con_nc[slot:slot + 1].fill_(Cn)
            st.con_auto[slot] = a
        st.con_state[slot:slot + 1].fill_(a.start)

    @staticmethod
    def _first_constrained(st, slot: int, logits: torch.Tensor) -> torch.Tensor:
        """The logits a constrained row's FIRST token is chosen from: one eager operator call on the prefill's last row (raw logits [V]) with no
        token, so the row is masked from its start state, which the first step then advances by that token.  An unconstrained row: `logits`."""
        if st.con_auto[slot] is None or int(st.con_state[slot].item()) < 0:
            return logits
        x = logits.reshape(1, -1).float().contiguous()
        return ops.logits_constrain(x, st.con_state[slot:slot + 1], st.con_cls[slot:slot + 1], st.con_next[slot:slot + 1], st.con_nc[slot:slot + 1])[0]

    @staticmethod
    def _logprob_state(st, n: int, max_rec: int, dev) -> None:
        """What a session with the `logprobs` flag owns: one record per row and step — the chosen token's logprob and all 20 alternatives, whatever a
        request asks for (the host slices) — the workspace of the launch, and per row the record of the FIRST token, which the host path chooses from
        the prefill's last row (`lp_first[row]`, three tensors, or None)."""
        st.lp_tok = torch.zeros((n, max_rec), device=dev, dtype=torch.float32)
        st.lp_top = torch.full((n, max_rec, ops.LOGPROBS_MAX_TOP), float("-inf"), device=dev, dtype=torch.float32)
        st.lp_id = torch.full((n, max_rec, ops.LOGPROBS_MAX_TOP), -1, device=dev, dtype=torch.int32)
        st.lp_ws = torch.empty((_lib.load().vila_logprobs_workspace_bytes(n),), device=dev, dtype=torch.uint8)
        st.lp_first = [None] * n
        st.lp = _lib.VilaLogprobOut(st.lp_tok.data_ptr(), st.lp_top.data_ptr(), st.lp_id.data_ptr(), max_rec)

    @staticmethod
    def _first_logprobs(st, row: int, logits: torch.Tensor, first: torch.Tensor) -> None:
        """The record of a request's first token: one eager `ops.logprobs` on the prefill's last row (raw logits [V]), kept with the session's row."""
        t, p, i = ops.logprobs(logits.reshape(1, -1).float(), first.reshape(1), ops.LOGPROBS_MAX_TOP)
        st.lp_first[row] = (t.clone(), p.clone(), i.clone())

    @staticmethod
    def _row_logprobs(st, row: int, n_steps: int):
        """(token_logprob [1 + n], top_logprob [1 + n, 20], top_id [1 + n, 20] i32) of a session's row: the first token's record, then those of its
        first n_steps steps (record k belongs to out_ids[row, k])."""
        t0, p0, i0 = st.lp_first[row]
        n = max(0, min(int(n_steps), st.lp_tok.shape[1]))
        return torch.cat([t0, st.lp_tok[row, :n]]), torch.cat([p0, st.lp_top[row, :n]]), torch.cat([i0, st.lp_id[row, :n]])

    @staticmethod
    def _pack_logprobs(rows, lens, n_cols: int, k: int, dev) -> "Logprobs":
        """Per-row records -> the value `generate(logprobs=k)` returns beside ids [B, n_cols]: row b keeps its first lens[b] records (the tokens up to
        and including its EOS), the pad positions behind them hold 0.0 / -inf / -1."""
        B = len(rows)
        tok = torch.zeros((B, n_cols), device=dev, dtype=torch.float32)
        top = torch.full((B, n_cols, k), float("-inf"), device=dev, dtype=torch.float32)
        ids = torch.full((B, n_cols, k), -1, device=dev, dtype=torch.int64)
        for b, (t, p, i) in enumerate(rows):
            m = min(int(lens[b]), n_cols, int(t.shape[0]))
            tok[b, :m] = t[:m]
            top[b, :m] = p[:m, :k]
            ids[b, :m] = i[:m, :k].long()
        return Logprobs(tok, top, ids)

    def batch_logprobs(self, st, slot: int) -> "Logprobs":
        """The records of row `slot` of a session opened with batch_open(logprobs=True): the first token's (chosen at `batch_admit`), then one per
        step the row has taken since, token for token the row's own ids ([first] + out_ids[slot, :n_out]).  All 20 alternatives; RAW logprobs (the
        model's distribution, whatever the row's sampling or penalties).  A slot that served another request before shows only the current one's."""
        if getattr(st, "lp", None) is None:
            raise ValueError("batch_logprobs: the session was opened without batch_open(logprobs=True)")
        if st.lp_first[int(slot)] is None:
            raise ValueError(f"batch_logprobs: no request was admitted into row {int(slot)}")
        st.stream.synchronize()
        t, p, i = self._row_logprobs(st, int(slot), int(st.n_out[int(slot)].item()))
        return Logprobs(t, p, i.long())

    SCORE_MAX_TARGETS = 512

    @torch.no_grad()
    def score(self, inputs_embeds: torch.Tensor, target_ids: torch.Tensor, top_n: int = 0) -> "Logprobs":
        """Per-token log-likelihoods of a GIVEN continuation (HF: `log_softmax(logits).gather(...)` over a forward pass): inputs_embeds [S, H] is the
        whole sequence, target_ids [T] are the ids at its last T positions (whose embeddings are the last T rows of inputs_embeds).  ONE
        `prefill_packed` with last_rows = S - T - 1 .. S - 2 (the rows that predict the targets; a logits buffer of T x V fp32), then ONE
        `ops.logprobs` over those T rows against target_ids.  1 <= T <= 512 and T < S.  bf16, or W4 where quantize_w4(prefill=True).
        -> `Logprobs`(token_logprobs [T], top_logprobs [T, top_n], top_ids [T, top_n] int64): RAW logprobs, the top_n most likely ids per position."""
        ops._need(inputs_embeds, dtype=None, name="inputs_embeds")
        if inputs_embeds.dim() != 2 or inputs_embeds.shape[1] != self.lcfg.hidden_size:
            raise ValueError(f"score: inputs_embeds must be [S, {self.lcfg.hidden_size}] (got {tuple(inputs_embeds.shape)})")
        S, T = int(inputs_embeds.shape[0]), int(target_ids.numel())
        if not 1 <= T <= self.SCORE_MAX_TARGETS:
            raise ValueError(f"score: 1..{self.SCORE_MAX_TARGETS} target ids (got {T}): the logits buffer is T x vocabulary fp32")
        if not T < S:
            raise ValueError(f"score: the {T} targets are the LAST positions of the sequence, behind at least one position of context (got S = {S})")
        if isinstance(top_n, bool) or not isinstance(top_n, numbers.Integral) or not 0 <= int(top_n) <= ops.LOGPROBS_MAX_TOP:
            raise ValueError(f"score: top_n has to be an integer in 0..{ops.LOGPROBS_MAX_TOP}, but is {top_n!r}")
        dev = inputs_embeds.device
        rows = torch.arange(S - T - 1, S - 1, device=dev, dtype=torch.int32)
        r = self.prefill_packed(inputs_embeds.to(self.dtype), torch.arange(S, device=dev, dtype=torch.int32), None, S, last_rows=rows)
        t, p, i = ops.logprobs(r.last_logits, target_ids.reshape(-1).to(device=dev, dtype=torch.int64).contiguous(), int(top_n))
        return Logprobs(t, p, i.long())

    def _decode_session(self, cache, max_new_tokens: int, sampling=None, penalties: bool = False, logprobs: bool = False, constraints=None):
        """Device-resident decode state + workspace (+ captured hipGraph) reused across generate() calls.
        sampling: None (greedy) or (temperature, top_k, top_p, seed) — baked into the captured graph, hence part of the key.
        penalties=True (part of the key; a session without the flag keeps the key it always had): the session steps through
        `vila_llm_decode_step_penalized` and owns the count table and the parameter arrays (`_penalty_state`).
        logprobs=True (part of the key only when set, likewise): `vila_logprobs_f32` runs behind every step, inside the captured graph, and the
        session owns the records (`_logprob_state`); no launch of the step itself changes.
        constraints=(max_states, max_classes) (part of the key only when set, likewise): the session steps through `vila_llm_decode_step_constrained`
        (with its penalties, where it has them, as that entry's nullable argument) and owns the automaton's arrays (`_constraint_state`)."""
        # the seed is NOT part of the key: it lives in a device scalar the sampler reads (VilaSampling.seed_dev), so every sampled request
        # with the same (temperature, top_k, top_p) replays the same captured graph (a fresh seed per call used to drop
        # the graph, the workspace and the weight struct on every sampled request)
        key = (cache.k.data_ptr(), max_new_tokens, *self._weights_key()[:2], None if sampling is None else tuple(sampling[:3]))   # (no int4 pointer: as ever)
        key += (True,) if penalties else ()
        key += ("logprobs",) if logprobs else ()
        key += ("constraints", *constraints) if constraints else ()
        if self._decode is not None and self._decode.key == key:
            if sampling is not None:
                self._decode.seed.fill_(_as_i64(sampling[3]))
            return self._decode
        old = self._decode
        if old is not None and old.key[2:4] != key[2:4]:
            self._invalidate()      # the weight storage moved: nothing that baked in a pointer survives
        else:
            self._drop_decode_session()          # another cache / length / sampling setting: only this session and its graph
        dev = self.device
        lib = _lib.load()
        w = self._struct()
        st = SimpleNamespace(key=key, cache=cache)
        st.sampling = None
        st.pen = None
        st.lp = None
        st.con = None
        # the session outlives the call that creates it: built outside inference mode even when the first generate() runs under
        # torch.inference_mode() (llava_arch.py:823), or a later no_grad caller could not update `pos` / `token` in place
        with torch.inference_mode(False):
            st.pos = torch.zeros(1, device=dev, dtype=torch.int32)
            st.token = torch.zeros(1, device=dev, dtype=torch.int64)
            st.out_ids = torch.zeros(max(max_new_tokens, 1), device=dev, dtype=torch.int64)
            st.n_out = torch.zeros(1, device=dev, dtype=torch.int32)
            st.logits = torch.zeros(self.lcfg.vocab_size, device=dev, dtype=torch.float32)
            ws_bytes = getattr(lib, _step_symbols(False, False, False, penalized=bool(penalties), constrained=bool(constraints))[1])
            st.ws = torch.empty((ws_bytes(C.byref(w.shape), cache.max_ctx),), device=dev, dtype=torch.uint8)
            if constraints:
                self._constraint_state(st, 1, self.lcfg.vocab_size, constraints, dev)
            st.seed = torch.zeros(1, device=dev, dtype=torch.int64)          # the sampler's seed (bit pattern of a uint64)
            if penalties:
                self._penalty_state(st, 1, self.lcfg.vocab_size, dev)
            if logprobs:
                self._logprob_state(st, 1, max(max_new_tokens, 1), dev)
        if sampling is not None:
            st.seed.fill_(_as_i64(sampling[3]))
            st.sampling = _lib.VilaSampling(float(sampling[0]), int(sampling[1]), float(sampling[2]), int(sampling[3]) & 0xFFFFFFFFFFFFFFFF,
                                            st.seed.data_ptr())
        st.c = _lib.VilaDecodeState(st.pos.data_ptr(), st.token.data_ptr(), st.out_ids.data_ptr(), st.n_out.data_ptr(),
                                    max(max_new_tokens, 1), st.logits.data_ptr())
        st.graph = None
        st.stream = torch.cuda.Stream(device=dev)
        self._decode = st
        return st

    _W4_PROJ = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")

    def quantize_w4(self, keep_logical: bool = True, prefill: bool = False, release_bf16: bool = False, batch_decode: bool = False):
        """Build int4 (group-128) copies of the five decoder projections: decode then runs the W4A16 GEMVs (vila_llm_decode_step_w4).
        prefill=False (default): the prefill keeps using the bf16 weights.  prefill=True: every prefill (prefill_packed, generate, forward)
        runs the W4A16 GEMMs as well (vila_llm_prefill_w4), so the model computes from its int4 weights alone.  release_bf16=True (needs
        prefill=True) then frees the bf16 projection weights (`release_bf16_projections`).
        batch_decode=False (default): generate() on a batch decodes its rows one after another with the solo W4 step, and batch_open refuses
        the model.  batch_decode=True: generate(batch), batch_open / batch_admit / batch_run and a serving ContinuousBatcher run the W4A16
        batched step (vila_llm_decode_step_batch_w4: one pass over the int4 weights for up to 16 rows), also after release_bf16.  Its sums
        run in another order than the solo step's, so ids can differ from the row-by-row ones where the top-2 margin is not decisive."""
        if release_bf16 and not prefill:
            raise ValueError("quantize_w4: release_bf16=True needs prefill=True (the bf16 prefill reads the bf16 projections)")
        self._require_bf16("quantize_w4")
        from .quant import W4Weights
        self._w4 = W4Weights(self, keep_logical)
        self._w4_prefill = bool(prefill)
        self._w4_batch = bool(batch_decode)
        self._invalidate()
        if release_bf16:
            self.release_bf16_projections()
        return self._w4

    def release_bf16_projections(self) -> int:
        """Drop the bf16 q/k/v (one fused buffer), o, gate, up and down weights of every layer once the int4 copies serve both prefill and
        decode (quantize_w4(prefill=True)).  Each projection parameter is re-pointed at a zero-element tensor [0, in_features] of its device
        and dtype, so its storage is freed and nothing can read stale memory through it: torch ops see an empty tensor, and every path of
        this package that would use the weights raises a RuntimeError naming release_bf16.  Returns the bytes of bf16 weights dropped."""
        if self._w4 is None or not self._w4_prefill:
            raise RuntimeError("release_bf16 needs quantize_w4(prefill=True) first: the bf16 prefill reads these weights")
        proj = [_get(self, f"model.layers.{i}.{n}.weight") for i in range(self.lcfg.num_hidden_layers) for n in self._W4_PROJ]
        proj_bytes = {}
        for p in proj:
            proj_bytes[p.untyped_storage().data_ptr()] = proj_bytes.get(p.untyped_storage().data_ptr(), 0) + p.numel() * p.element_size()
        others = {p.untyped_storage().data_ptr() for n, p in self.named_parameters() if not any(f".{k}.weight" in "." + n for k in self._W4_PROJ)}
        for p in proj:
            st = p.untyped_storage()
            if st.data_ptr() in others or proj_bytes[st.data_ptr()] != st.nbytes():
                raise RuntimeError("release_bf16: the projection weights share their storage with other tensors (FlatParams?); nothing was freed")
        freed = sum(proj_bytes.values())
        self._invalidate()
        self._bf16_released = True
        for p in proj:
            p.data = torch.empty((0,) + tuple(p.shape[1:]), device=p.device, dtype=p.dtype)
        return freed

    def _load_from_state_dict(self, *a, **k):
        self._require_bf16("load_state_dict")
        return super()._load_from_state_dict(*a, **k)

    def _require_bf16(self, what: str) -> None:
        if self._bf16_released:
            raise RuntimeError(f"{what}: the bf16 projection weights were freed by quantize_w4(release_bf16=True); only the W4A16 "
                               "prefill and decode can run on this model")

    def _step(self, batch: bool, w4, cache, st, sp, verify: bool = False, verify_sample: bool = False) -> None:
        """One decode step on the current stream.  The variant is looked up at call time (`_step_symbols`): a caller may hold a session
        across quantize_w4.  w4: the W4Weights whose int4 layers the step reads, or None; sp: the sampling struct, or None for the greedy pick."""
        px = getattr(st, "px", None)                                    # a session with a shared prompt prefix: its descriptor follows the state
        pen = getattr(st, "pen", None)                                  # a session with the penalties flag: the one entry of its driver, NULLs for what is off
        con = getattr(st, "con", None)                                  # a session with the constraints flag: likewise, the penalties nullable too
        ref = lambda s: None if s is None else C.byref(s)
        if getattr(st, "lora", None) is not None:                       # a session with an adapter bank: the one entry, NULLs for what is off
            name, _ = _step_symbols(batch, w4 is not None, sp is not None, verify, verify_sample, prefix=px is not None, lora=True)
            check(getattr(_lib.load(), name)(C.byref(self._struct()), None, C.byref(cache.c), C.byref(st.c), None, C.byref(st.lora), st.ws.data_ptr(), st.ws.numel(),
                                             ref(sp), ref(pen), ref(con), 1 if getattr(st, "any_k", False) else 0, ops._stream()), name)
        elif getattr(st, "processed", False):                           # a verify session with the processed flag: one entry, NULLs for what is off
            name, _ = _step_symbols(batch, w4 is not None, sp is not None, verify, verify_sample, processed=True)
            check(getattr(_lib.load(), name)(C.byref(self._struct()), w4.ptr if w4 is not None else None, C.byref(cache.c), C.byref(st.c), st.ws.data_ptr(),
                                             st.ws.numel(), ref(sp), 1 if getattr(st, "any_k", False) else 0, ref(pen), ref(con), ref(getattr(st, "lp", None)),
                                             ops._stream()), name)
            return                                                      # (its records are written inside the entry, behind the accept)
        elif getattr(st, "any_k", False):                               # a session with the any_top_k flag: the one entry of its driver, NULLs for what is off
            name, _ = _step_symbols(batch, w4 is not None, sp is not None, verify, verify_sample, prefix=px is not None, any_k=True)
            args = ([C.byref(self._struct()), w4.ptr if w4 is not None else None, C.byref(cache.c), C.byref(st.c)] + ([] if verify_sample else [ref(px)]) +
                    [st.ws.data_ptr(), st.ws.numel(), C.byref(sp)] + ([] if verify_sample else [ref(pen), ref(con)]) + [ops._stream()])
            check(getattr(_lib.load(), name)(*args), name)
        elif con is not None:
            name, _ = _step_symbols(batch, w4 is not None, sp is not None, verify, verify_sample, prefix=px is not None, constrained=True)
            args = ([C.byref(self._struct()), w4.ptr if w4 is not None else None, C.byref(cache.c), C.byref(st.c)] + ([ref(px)] if batch else []) +
                    [st.ws.data_ptr(), st.ws.numel(), ref(sp), ref(pen), C.byref(con), ops._stream()])
            check(getattr(_lib.load(), name)(*args), name)
        elif pen is not None:
            name, _ = _step_symbols(batch, w4 is not None, sp is not None, verify, verify_sample, prefix=px is not None, penalized=True)
            args = ([C.byref(self._struct()), w4.ptr if w4 is not None else None, C.byref(cache.c), C.byref(st.c)] + ([ref(px)] if batch else []) +
                    [st.ws.data_ptr(), st.ws.numel(), ref(sp), C.byref(pen), ops._stream()])
            check(getattr(_lib.load(), name)(*args), name)
        else:
            name, _ = _step_symbols(batch, w4 is not None, sp is not None, verify, verify_sample, prefix=px is not None)
            args = ([C.byref(self._struct())] + ([w4.ptr] if w4 is not None else []) + [C.byref(cache.c), C.byref(st.c)] +
                    ([C.byref(px)] if px is not None else []) + [st.ws.data_ptr(), st.ws.numel()])
            check(getattr(_lib.load(), name)(*args, *([C.byref(sp)] if sp is not None else []), ops._stream()), name)
        lp = getattr(st, "lp", None)                                    # a session with the logprobs flag: the record of the token this step chose
        if lp is not None:
            # behind the step, on its stream (inside the captured graph): token = the step's pick, n_out - 1 = its place in out_ids
            V = self.lcfg.vocab_size
            check(_lib.load().vila_logprobs_f32(st.logits.data_ptr(), V, st.pos.numel(), V, st.token.data_ptr(), ops.LOGPROBS_MAX_TOP, st.n_out.data_ptr(), -1,
                                                C.byref(lp), st.lp_ws.data_ptr(), ops._stream()), "vila_logprobs_f32")

    def decode_step(self, cache, st) -> None:
        if self._w4 is None:
            self._require_bf16("the bf16 decode step")
        self._step(False, self._w4, cache, st, getattr(st, "sampling", None))

    # ---- batched greedy generate: one weight pass per step for up to 16 sequences (vila_llm_decode_step_batch) -----------------------
    def _can_batch_decode(self, inputs_embeds, attention_mask, max_new_tokens, do_sample, forced_ids, return_logits, cache,
                          batch_sample: bool = False, top_k: int = 50, any_top_k: bool = False) -> bool:
        """The greedy batched step serves a padded batch; with batch_sample (opt-in) the same holds for a sampled batch whose top_k the
        batched sampler serves (1..64; with any_top_k every top_k >= 0), teacher forcing included."""
        c = self.lcfg
        Bn, S = inputs_embeds.shape[0], inputs_embeds.shape[1]
        if do_sample:
            ok = batch_sample and (1 <= top_k <= 64 or (any_top_k and top_k >= 0))
        else:
            ok = forced_ids is None and not return_logits
        return (ok and cache is None and self.can_batch_decode_step() and
                max_new_tokens >= 1 and (self._w4_batched() or self._qkv_fused()) and 2 <= Bn <= 16 and c.hidden_size % 64 == 0 and
                c.intermediate_size % 64 == 0 and ((S + max_new_tokens + 255) // 256) * 256 <= self.BATCH_MAX_CTX and
                (S + max_new_tokens <= 2048 or self._long_batch_group_ok()))

    # the batched step's caches: up to 2048 positions one attention slice per 256-key chunk, beyond that blocks that walk chunks (up to Qwen2.5's
    # max_position_embeddings; GQA groups of 1, 2, 4, 7 or 8)
    BATCH_MAX_CTX = 32768

    def _long_batch_group_ok(self) -> bool:
        c = self.lcfg
        return c.num_attention_heads % c.num_key_value_heads == 0 and c.num_attention_heads // c.num_key_value_heads in (1, 2, 4, 7, 8)

    def _w4_batched(self) -> bool:
        """The batched step reads the int4 layers (quantize_w4(batch_decode=True))."""
        return self._w4 is not None and self._w4_batch

    def can_batch_decode_step(self) -> bool:
        """Whether this model has a batched decode step (batch_open / continuous batching): a head-dim-128 decoder that is bf16, or
        quantised with quantize_w4(batch_decode=True).  A model quantised without it decodes its rows one at a time."""
        return self.lcfg.head_dim == 128 and (self._w4 is None or self._w4_batched())

    def _qkv_fused(self) -> bool:
        """q/k/v of every layer are views of one buffer (the batched step reads them as ONE [q + 2kv, hidden] matrix); `refuse()` re-establishes
        it after an op that re-allocated parameters — a model somebody un-fused falls back to the per-row loop instead of raising."""
        c = self.lcfg
        for i in range(c.num_hidden_layers):
            a = _get(self, f"model.layers.{i}.self_attn")
            q, k, v = a.q_proj.weight, a.k_proj.weight, a.v_proj.weight
            if k.data_ptr() != q.data_ptr() + q.numel() * q.element_size() or v.data_ptr() != k.data_ptr() + k.numel() * k.element_size():
                return False
        return True

    def _batch_session(self, n: int, max_ctx: int, max_new_tokens: int, sampling: bool = False, shared_prefix: bool = False, penalties: bool = False,
                       logprobs: bool = False, constraints=None, any_top_k: bool = False, adapters=None):
        """sampling=True: the session owns per-row sampling parameters on the device (temperature / top_k / top_p / seed, every row greedy
        until `_batch_set_sampling` says otherwise) and steps through the `_sample` entry points: one captured graph for any mix of rows.
        shared_prefix=True: the cache has one slot more, the prefix slot (index n), and the session owns the shared length and the rows' flags on
        the device; it steps through the `_prefix` entry points.
        penalties=True (in the key only when set, so every other session keeps its key): the session steps through
        `vila_llm_decode_step_batch_penalized` and owns a count row and (rep, pres, freq) per row (`_penalty_state`), every row neutral until
        `_set_penalties` says otherwise.
        logprobs=True (in the key only when set, likewise): `vila_logprobs_f32` runs behind every step and the session owns a record per row and step
        (`_logprob_state`).
        constraints=(max_states, max_classes) (in the key only when set, likewise): the session steps through
        `vila_llm_decode_step_batch_constrained` and owns an automaton per row (`_constraint_state`), every row unconstrained until
        `_set_constraint` says otherwise.
        any_top_k=True (sampling sessions; in the key only when set, likewise): the session steps through `vila_llm_decode_step_batch_any_k`, whose
        pick serves a row with any top_k >= 0 (0 = no top-k filter) from the same device arrays.
        adapters=bank (an `AdapterBank`; in the key only when set, likewise): the session steps through `vila_llm_decode_step_batch_lora` and owns
        `row_adapter` [n] int32 on the device, every row -1 (the base model) until `batch_admit(adapter=)` / `_set_row_adapter` says otherwise.  bf16
        models, no shared prefix."""
        if any_top_k and not sampling:
            raise ValueError("any_top_k is an option of a sampling session (sampling=True)")
        w4 = self._w4_batched()
        if adapters is not None:
            _step_symbols(True, self._w4 is not None, bool(sampling), prefix=bool(shared_prefix), lora=True)      # (its refusals: int4 layers, a shared prefix)
        if not w4:
            self._require_bf16("the batched decode")
        key = (n, max_ctx, max_new_tokens, bool(sampling), *self._weights_key()) + ((True,) if shared_prefix else ()) + (("penalties",) if penalties else ())
        key += ("logprobs",) if logprobs else ()
        key += ("constraints", *constraints) if constraints else ()
        key += ("any_top_k",) if any_top_k else ()
        key += ("adapters", id(adapters), adapters.capacity, adapters.r) if adapters is not None else ()
        if self._bdecode is not None and self._bdecode.key == key:
            return self._bdecode
        self._drop_session("_bdecode")
        dev, lib, w = self.device, _lib.load(), self._struct()
        st = SimpleNamespace(key=key, graph=None, sampling=bool(sampling), sp=None, px=None, shared_prefix=bool(shared_prefix), pen=None, lp=None, con=None)
        if any_top_k:
            st.any_k = True
        st.lora, st.adapters = None, adapters
        st.attn_slices = int(lib.vila_decode_batch_slices(int(max_ctx)))     # walking-attention slices the steps of this session launch (0: short form)
        with torch.inference_mode(False):
            st.cache = self.new_cache(max_ctx, n_slots=n + 1 if shared_prefix else n)
            if shared_prefix:
                st.prefix_slot = n
                st.shared_len = torch.zeros(1, device=dev, dtype=torch.int32)
                st.uses = torch.zeros(n, device=dev, dtype=torch.int32)
                st.px = _lib.VilaDecodePrefix(n, st.shared_len.data_ptr(), st.uses.data_ptr())
                self._prefix_reset(st)
            st.pos = torch.zeros(n, device=dev, dtype=torch.int32)
            st.token = torch.zeros(n, device=dev, dtype=torch.int64)
            st.out_ids = torch.zeros((n, max(max_new_tokens, 1)), device=dev, dtype=torch.int64)
            st.n_out = torch.zeros(n, device=dev, dtype=torch.int32)
            st.logits = torch.zeros((n, self.lcfg.vocab_size), device=dev, dtype=torch.float32)
            ws_bytes = getattr(lib, _step_symbols(True, w4, bool(sampling), prefix=bool(shared_prefix), penalized=bool(penalties),
                                                  constrained=bool(constraints), **(dict(any_k=True) if any_top_k else {}),
                                                  **(dict(lora=True) if adapters is not None else {}))[1])
            if adapters is not None:
                st.row_adapter = torch.full((n,), -1, device=dev, dtype=torch.int32)
                st.row_names = [None] * n                              # the adapter each live row was admitted under (the bank counts them)
                st.lora = adapters.c_bank(st.row_adapter)
            if constraints:
                self._constraint_state(st, n, self.lcfg.vocab_size, constraints, dev)
            if penalties:
                self._penalty_state(st, n, self.lcfg.vocab_size, dev)
            if logprobs:
                self._logprob_state(st, n, max(max_new_tokens, 1), dev)
            if sampling:
                st.s_temperature = torch.zeros(n, device=dev, dtype=torch.float32)          # 0 = greedy row
                st.s_top_k = torch.full((n,), 50, device=dev, dtype=torch.int32)
                st.s_top_p = torch.ones(n, device=dev, dtype=torch.float32)
                st.s_seed = torch.zeros(n, device=dev, dtype=torch.int64)                   # bit patterns of uint64 seeds
                st.sp = _lib.VilaBatchSampling(st.s_temperature.data_ptr(), st.s_top_k.data_ptr(), st.s_top_p.data_ptr(), st.s_seed.data_ptr())
            ws_args = (int(bool(shared_prefix)),) if penalties or constraints or any_top_k else ()
            if adapters is not None:
                ws_args = (adapters.r,)
            st.ws = torch.empty((ws_bytes(C.byref(w.shape), n, int(max_ctx), *ws_args),), device=dev, dtype=torch.uint8)    # (<= 2048 positions: the size it always had)
        st.c = _lib.VilaDecodeBatch(n, st.pos.data_ptr(), st.token.data_ptr(), st.out_ids.data_ptr(), st.n_out.data_ptr(), max(max_new_tokens, 1),
                                    st.logits.data_ptr())
        st.stream = torch.cuda.Stream(device=dev)
        self._bdecode = st
        return st

    def _batch_step(self, st) -> None:
        self._step(True, self._w4 if self._w4_batched() else None, st.cache, st, st.sp if st.sampling else None)

    # ---- continuous batching (server.py:171-290 serves requests as they arrive): rows join and leave BETWEEN steps ---------
    # `vila_llm_decode_step_batch` takes per-row positions / output counters, so admission is host work: prefill the newcomer alone into its
    # KV slot, set the row's position and first token, replay the same captured graph.  A free row idles at positions 0..15 of its own slot
    # (re-wound after every chunk), which costs nothing extra: the step streams the weights once whatever the number of live rows.
    @staticmethod
    def _check_batch_sampling(sampling, what: str, any_top_k: bool = False):
        """(temperature, top_k, top_p, seed) of ONE row of a sampling batch session, validated where the values are known (the kernel only
        clamps).  The batched sampler serves top_k in 1..64; that of a session with the any_top_k flag every top_k >= 0 (0 = no top-k filter)."""
        temperature, top_k, top_p, seed = float(sampling[0]), int(sampling[1]), float(sampling[2]), int(sampling[3])
        if temperature <= 0:
            raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float, otherwise your next token scores will be invalid.")
        if top_k < 0:
            raise ValueError(f"`top_k` has to be a non-negative integer, but is {top_k}")
        if not 1 <= top_k <= 64 and not any_top_k:
            raise ValueError(f"{what}: the batched sampler serves top_k in 1..64 (got {top_k}); such a request runs solo")
        if not 0.0 < top_p <= 1.0:
            raise ValueError(f"`top_p` has to be a float > 0 and <= 1, but is {top_p}")
        return temperature, top_k, top_p, seed

    @staticmethod
    def _batch_set_sampling(st, slot: int, sampling) -> None:
        """Write one row's sampling parameters (None = greedy row) into the session's device arrays: the next replay reads them."""
        t, k, p, seed = (0.0, 50, 1.0, 0) if sampling is None else sampling
        st.s_temperature[slot:slot + 1].fill_(float(t))
        st.s_top_k[slot:slot + 1].fill_(int(k))
        st.s_top_p[slot:slot + 1].fill_(float(p))
        st.s_seed[slot:slot + 1].fill_(_as_i64(seed))

    @staticmethod
    def _set_row_adapter(st, slot: int, name) -> int:
        """Row `slot` of a session with a bank runs under adapter `name` from its next step on (None: the base model, -1); the bank counts the
        live rows of every slot, so that `unload` can refuse.  -> the bank slot."""
        bank, old = st.adapters, st.row_names[slot]
        new = bank.slot_of(name)
        if old is not None and old in bank:
            bank.in_use[bank.slot_of(old)] -= 1
        if name is not None:
            bank.in_use[new] += 1
        st.row_names[slot] = name
        st.row_adapter[slot:slot + 1].fill_(new)
        return new

    def batch_open(self, n_slots: int, max_ctx: int = 2048, max_new_tokens: int = 1024, sampling: bool = False, shared_prefix: bool = False,
                   penalties: bool = False, logprobs: bool = False, constraints: bool = False, max_states: int = 512, max_classes: int = 4096,
                   any_top_k: bool = False, adapters=None):
        """Open (or re-use) the batched-decode session of `n_slots` rows with its captured step.  sampling=False: the greedy step.  sampling=True:
        the step picks per row from device-resident parameters, so the ONE captured graph serves any mix of greedy and sampled rows
        (`batch_admit(..., sampling=)`); the flag is part of the session key.
        shared_prefix=True (part of the key as well): the session may hold one shared prompt prefix in an extra cache slot (`batch_set_prefix`), and
        rows admitted with `batch_admit(..., share=True)` read its K/V instead of a copy of their own: the step's attention reads the prefix once for
        all of them.  The ONE captured graph serves any shared length and any mix of sharing and ordinary rows.  GQA groups of 1, 2, 4, 7 or 8.
        penalties=True (part of the key as well): rows may carry repetition / presence / frequency penalties (`batch_admit(..., penalties=)`); the
        values and every row's token counts live on the device, so the ONE captured graph serves any mix of penalised and plain rows.
        logprobs=True (part of the key as well): every step also records, per row, the RAW log-probability of the token it chose and of the 20 most
        likely ones (`vila_logprobs_f32` behind the step, in the same graph; `batch_logprobs(st, slot)` reads a row's records).  Raw: the model's
        own distribution, independent of the row's temperature, top-k, top-p and penalties.
        constraints=True (part of the key as well, with max_states and max_classes): rows may carry a token automaton (`batch_admit(..., constraint=)`,
        `vila_amd.constrain`) that holds their reply to a choice list, a regular expression or a JSON schema.  The automata live on the device — per
        row the class of every token id and a table of max_states x max_classes int16 ENTRIES — so the ONE captured graph serves any mix of
        constrained and plain rows and any change of automaton.  The two arguments size the table, they do not bound states on their own: an
        automaton lies in it row-major with its OWN class count, so it fits when states x classes <= max_states x max_classes and classes <=
        max_classes (an automaton with few classes may have more than max_states states).
        any_top_k=True (with sampling=True; part of the key as well): a sampled row may carry ANY top_k >= 0 — 0 = no top-k filter, HF's meaning,
        i.e. pure top-p sampling, and k > 64 — where the session without the flag serves 1..64.  Such a row is drawn on the device by the solo
        sampler's exact path (one launch more per step, one block per row) and gets bit for bit the token `ops.sample` returns for its logits,
        parameters, seed and counter; the ONE captured graph serves any mix of greedy rows, rows of 1..64 and such rows.
        adapters=bank (a `vila_amd.lora_serving.AdapterBank`; part of the key as well, only when set): every row may run under its own LoRA adapter
        of the bank, unmerged (`batch_admit(..., adapter=name)`; None = the base model).  The rows' slots live in a device array and the bank's
        buffers never move, so the ONE captured graph serves any mix of adapters and survives `bank.load` / `bank.unload`.  bf16 models; not with
        shared_prefix.  A row without an adapter keeps the bits of the session without the flag."""
        if any_top_k and not sampling:
            raise ValueError("batch_open: any_top_k=True is an option of a sampling session (sampling=True)")
        if adapters is not None and (self._w4 is not None or shared_prefix):
            raise ValueError("batch_open: adapters= serves bf16 models without a shared prefix (the adapters add to bf16 projections of rows with "
                             "caches of their own)")
        if not self._w4_batched():
            self._require_bf16("batch_open")
        con_caps = self._constraint_caps(max_states, max_classes) if constraints else None
        long_ok = (max_ctx <= 2048 and not shared_prefix) or self._long_batch_group_ok()
        if not (1 <= n_slots <= 16 and 1 <= max_ctx <= self.BATCH_MAX_CTX and long_ok and self.can_batch_decode_step() and
                (self._w4_batched() or self._qkv_fused())):
            raise ValueError("batch_open: the batched decode step serves 1..16 rows of a head-dim-128 model (bf16, or quantize_w4(batch_decode=True)) "
                             f"with caches <= {self.BATCH_MAX_CTX} positions (beyond 2048: GQA groups of 1, 2, 4, 7 or 8 query heads)")
        st = self._batch_session(max(n_slots, 2), max_ctx, max_new_tokens, sampling, shared_prefix, penalties, logprobs,
                                 **({} if con_caps is None else dict(constraints=con_caps)), **(dict(any_top_k=True) if any_top_k else {}),
                                 **({} if adapters is None else dict(adapters=adapters)))
        if getattr(st, "con", None) is not None:
            st.con_state.fill_(-1)                                     # every row starts unconstrained (an idle row never advances)
        if getattr(st, "lora", None) is not None:
            for slot in range(len(st.row_names)):
                self._set_row_adapter(st, slot, None)                  # every row starts on the base model
        def reset():
            st.pos.zero_(); st.n_out.zero_(); st.token.zero_()
            if getattr(st, "pen", None) is not None:
                st.counts.zero_()                                      # (the warm-up step outside capture bumps one count per row)
        reset()
        if getattr(st, "pen", None) is not None:
            st.p_rep.fill_(1.0); st.p_pres.zero_(); st.p_freq.zero_()  # every row starts neutral
        if st.shared_prefix:
            self._prefix_reset(st)                                     # no prefix, every row ordinary
        if st.sampling:
            st.s_temperature.zero_()                                   # every row starts greedy (idle)
        if st.graph is None:
            _capture(st, lambda: self._batch_step(st), reset)
            with torch.cuda.stream(st.stream):
                reset()                                                # the session starts idle whatever the capture left
        return st

    @staticmethod
    def _prefix_reset(st) -> None:
        """A shared-prefix session without a prefix: S = 0, no flag set, nothing staged."""
        st.shared_len.zero_(); st.uses.zero_()
        st.S, st.sharers = 0, set()
        st.staged_len, st.staged_tail, st.staged_logits = None, None, None

    def batch_set_prefix(self, st, embeds: torch.Tensor, prefix_len: Optional[int] = None) -> int:
        """Make embeds [C, H] the shared prefix of a session opened with batch_open(shared_prefix=True): it is prefilled into the prefix slot and its
        first S = C // 256 * 256 positions (whole attention chunks) become the keys every sharing row reads.  Returns S.  Refused while a live row
        shares the current prefix (`batch_release` frees them).  Rows S .. C - 1 of the prefix slot are staging: a request whose whole prompt is
        `embeds` is then admitted without another prefill (`batch_admit(..., share=True)`).
        prefix_len (default C): embeds is a first request's whole prompt of which only the first prefix_len rows are common to the requests that
        will share; S = prefix_len // 256 * 256."""
        if not getattr(st, "shared_prefix", False):
            raise ValueError("batch_set_prefix: the session was opened without batch_open(shared_prefix=True)")
        if st.sharers:
            raise ValueError(f"batch_set_prefix: rows {sorted(st.sharers)} still share the current prefix; release them first")
        ops._need(embeds, dtype=None, name="embeds")
        Cn = int(embeds.shape[0])
        if embeds.dim() != 2 or Cn < 1 or Cn + 1 > st.cache.max_ctx:
            raise ValueError(f"batch_set_prefix: embeds must be [C, H] with 1 <= C < {st.cache.max_ctx} (got {tuple(embeds.shape)})")
        shared = Cn if prefix_len is None else int(prefix_len)
        if not 0 <= shared <= Cn:
            raise ValueError(f"batch_set_prefix: prefix_len ({shared}) outside the {Cn} rows given")
        dev = embeds.device
        st.stream.synchronize()
        self._prefix_reset(st)                                         # a prefill that fails leaves the session without a prefix, not with half of one
        x = embeds.to(self.dtype)
        last = torch.full((1,), Cn - 1, device=dev, dtype=torch.int32)
        r = self.prefill_packed(x, torch.arange(Cn, device=dev, dtype=torch.int32), torch.tensor([0, Cn], device=dev, dtype=torch.int32), Cn, cache=st.cache,
                                seq_of_tok=torch.full((Cn,), st.prefix_slot, device=dev, dtype=torch.int32), last_rows=last)
        S = shared // 256 * 256
        st.shared_len.fill_(S)
        st.S = S
        st.staged_len, st.staged_tail, st.staged_logits = Cn, x[S:].clone(), r.last_logits[0].clone()
        torch.cuda.current_stream().synchronize()
        return S

    def _admit_sharing(self, st, slot: int, embeds: torch.Tensor, first_row: int):
        """The tail S .. P - 1 of a sharing row: prefilled behind the prefix in the prefix slot's staging rows (unless the rows staged there are this
        very tail) and copied to the row's own slot, every layer.  Returns the logits of the prompt's last row."""
        S, P = st.S, first_row + int(embeds.shape[0])
        tail = embeds.to(self.dtype)[S - first_row:]
        staged = st.staged_len == P and (P == S or torch.equal(st.staged_tail, tail))
        if not staged:
            if P == S:
                raise ValueError(f"batch_admit(share=True): a prompt that ends with the prefix (P = S = {S}) is served only right after the "
                                 "batch_set_prefix of that same prompt, which kept the logits of its last row")
            last = torch.full((1,), P - S - 1, device=tail.device, dtype=torch.int32)
            r = self.prefill_append(tail, st.cache, S, st.prefix_slot, last_rows=last)
            st.staged_len, st.staged_tail, st.staged_logits = P, tail.clone(), r.last_logits[0].clone()
        if P > S:
            for c in (st.cache.k, st.cache.v):
                c[:, slot, :, S:P].copy_(c[:, st.prefix_slot, :, S:P])
        return st.staged_logits

    def batch_admit(self, st, slot: int, embeds: torch.Tensor, sampling=None, share: bool = False, first_row: int = 0, penalties=None,
                    constraint=None, adapter: Optional[str] = None) -> int:
        """Prefill ONE sequence [P, H] into KV slot `slot` of the open batch and make the row live: position P, first token = argmax of the
        prefill's last row (returned), output counter 0.  sampling = (temperature, top_k in 1..64 — any top_k >= 0 in a session opened with
        any_top_k=True —, top_p, seed), sampling sessions only: the
        row samples — its parameters go to the device arrays, its first token is drawn from the prefill's last row with counter P - 1 (as the
        solo generate draws it), the steps draw with the position of the token they consume.  None = greedy row.
        share=True (sessions opened with shared_prefix=True, after `batch_set_prefix`): embeds is the WHOLE prompt [P, H], whose first S positions
        (S = the session's shared length) are the session's prefix (the caller's word: they are not compared) and P >= S.  Only the tail S .. P - 1 is prefilled, onto the prefix, and
        copied to the row's own slot; the row's flag is set, so its steps read keys 0 .. S - 1 from the prefix slot.
        first_row (share=True only, 0 <= first_row <= S): embeds holds the prompt's rows first_row .. P - 1 only — rows below S are never read, so a
        caller that has no embeddings of the prefix (a server that skipped the tower) passes the rest.
        penalties = (repetition, presence, frequency), sessions opened with penalties=True only: the row's picks run on the penalised logits.  The
        row's counts start from zero whatever the slot held before; the first token, chosen from the prefill, is never penalised (nothing has been
        generated yet).  None = a neutral row.
        constraint = a `vila_amd.constrain.Automaton`, sessions opened with constraints=True only: its classes and table go to the row, the first
        token is chosen from the prefill's last row masked from the start state (one eager operator call), and every step advances the state by the
        token it consumes and masks its pick.  None = an unconstrained row (state -1).
        adapter = the name of an adapter loaded into the session's bank, sessions opened with adapters= only: the prompt is prefilled under the
        adapter (`prefill_packed(adapter=)`) and the row's entry of `row_adapter` is set, so its steps add the adapter's deltas.  None = the base
        model (-1)."""
        if adapter is not None:
            if getattr(st, "lora", None) is None:
                raise ValueError("batch_admit: a row under an adapter needs a session opened with batch_open(adapters=bank)")
            st.adapters.slot_of(adapter)                               # (raises for a name that is not loaded)
        if constraint is not None:
            if getattr(st, "con", None) is None:
                raise ValueError("batch_admit: a constrained row needs a session opened with batch_open(constraints=True)")
            self._check_constraint(constraint, "batch_admit")
        if penalties is not None:
            penalties = self._check_penalties(*penalties)
            if penalties is not None and getattr(st, "pen", None) is None:
                raise ValueError("batch_admit: a penalised row needs a session opened with batch_open(penalties=True)")
        if sampling is not None:
            if not st.sampling:
                raise ValueError("batch_admit: a sampled row needs a session opened with batch_open(sampling=True)")
            sampling = self._check_batch_sampling(sampling, "batch_admit", **(dict(any_top_k=True) if getattr(st, "any_k", False) else {}))
        first_row = int(first_row)
        if first_row != 0 and not (share and 0 <= first_row <= getattr(st, "S", 0)):
            raise ValueError(f"batch_admit: first_row ({first_row}) is for share=True and lies in 0 .. the shared length")
        P = first_row + int(embeds.shape[0])
        if P + 1 > st.cache.max_ctx:
            raise ValueError(f"KV cache too small: {st.cache.max_ctx} < {P} + 1")
        if share:
            if not getattr(st, "shared_prefix", False):
                raise ValueError("batch_admit: share=True needs a session opened with batch_open(shared_prefix=True)")
            if st.S <= 0:
                raise ValueError("batch_admit: share=True needs a prefix of at least 256 positions (batch_set_prefix)")
            if P < st.S:
                raise ValueError(f"batch_admit: the prompt ({P} positions) is shorter than the shared prefix ({st.S})")
        dev = embeds.device
        st.stream.synchronize()                                        # no step is reading the cache while the newcomer's rows are written
        if not share and getattr(st, "shared_prefix", False):          # (behind the synchronise: no step in flight sees the flag change)
            st.uses[slot:slot + 1].zero_()
            st.sharers.discard(int(slot))
        last = torch.full((1,), P - 1, device=dev, dtype=torch.int32)
        if share:
            logits = self._admit_sharing(st, int(slot), embeds, first_row)
            st.uses[slot:slot + 1].fill_(1)
            st.sharers.add(int(slot))
        else:
            pos = torch.arange(P, device=dev, dtype=torch.int32)
            seq = torch.full((P,), int(slot), device=dev, dtype=torch.int32)
            cu = torch.tensor([0, P], device=dev, dtype=torch.int32)
            lora_kw = {} if adapter is None else dict(adapter=adapter, adapters=st.adapters)
            logits = self.prefill_packed(embeds.to(self.dtype), pos, cu, P, cache=st.cache, seq_of_tok=seq, last_rows=last, **lora_kw).last_logits[0]
        if getattr(st, "lora", None) is not None:
            self._set_row_adapter(st, int(slot), adapter)
        pick_from = logits
        if getattr(st, "con", None) is not None:
            self._set_constraint(st, int(slot), constraint)
            pick_from = self._first_constrained(st, int(slot), logits)
        first = (ops.argmax(pick_from) if sampling is None else
                 ops.sample(pick_from, sampling[0], sampling[1], sampling[2], sampling[3], counter=last))
        if st.sampling:
            self._batch_set_sampling(st, slot, sampling)
        if getattr(st, "pen", None) is not None:
            self._set_penalties(st, slot, penalties)
        if getattr(st, "lp", None) is not None:
            self._first_logprobs(st, int(slot), logits, first)         # the row's records are its own from here: n_out restarts at 0 below
        st.pos[slot:slot + 1].fill_(P)
        st.n_out[slot:slot + 1].zero_()
        st.token[slot:slot + 1].copy_(first)
        tok = int(first.item())                                        # (also orders the prefill before the next replay on st.stream)
        return tok

    def batch_run(self, st, k: int) -> None:
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(st.stream):
            _replay(st, k)
        st.stream.synchronize()

    def batch_release(self, st, slots) -> None:
        """Rows that finished (or never started): re-wound to position 0 of their own slot so an idle row never walks off its cache."""
        slots = list(slots)
        if slots:
            idx = torch.tensor(slots, device=st.pos.device, dtype=torch.int64)
            st.pos.index_fill_(0, idx, 0)
            st.n_out.index_fill_(0, idx, 0)
            if getattr(st, "lora", None) is not None:
                for s_ in slots:
                    self._set_row_adapter(st, int(s_), None)           # an idle row runs on the base model
            if getattr(st, "con", None) is not None:
                st.con_state.index_fill_(0, idx, -1)                   # an idle row is an unconstrained row
            if st.sampling:
                st.s_temperature.index_fill_(0, idx, 0.0)              # an idle row is a greedy row
            if getattr(st, "shared_prefix", False):
                st.uses.index_fill_(0, idx, 0)                         # ... and an ordinary one
                st.sharers.difference_update(int(s) for s in slots)

    def _generate_shared(self, inputs_embeds, n: int, max_new_tokens, eos_token_id, pad_token_id, use_graph: bool, return_logits: bool, sampling,
                         penalties=None, logprobs=None, constraint=None, any_top_k: bool = False):
        """generate(num_return_sequences=n): ONE prefill of the prompt into the prefix slot of a shared-prefix sampling session, n sharing rows that
        differ in their seeds.  Returns [n, n_new] like `_generate_batch`; return_logits: (ids [n, n_new], logits [n_new, n, V] fp32), eager steps.
        A prompt below 256 positions has no whole chunk to share: nothing goes into the prefix slot and the n rows are ordinary rows of the same
        session, each prefilled on its own (return_logits is refused for it by the caller).
        penalties: None, or the request's (rep, pres, freq): the session is opened with the penalties flag and every row carries them, with counts of
        its own.
        logprobs: None, or k: the session is opened with the logprobs flag and the call returns (ids, `Logprobs`) with k alternatives per token.
        any_top_k: the session is opened with the any_top_k flag, so the rows' top_k may be 0 or above 64."""
        x = inputs_embeds[0]
        P, dev = int(x.shape[0]), x.device
        max_ctx = ((P + max_new_tokens + 255) // 256) * 256
        con_kw = {} if constraint is None else dict(constraints=True, max_states=self.CONSTRAIN_MAX_STATES, max_classes=self.CONSTRAIN_MAX_CLASSES)
        row_kw = {} if constraint is None else dict(constraint=constraint)      # (every row carries the request's automaton, with a state of its own)
        st = self.batch_open(n, max_ctx, max_new_tokens, sampling=True, shared_prefix=True, penalties=penalties is not None,
                             **({} if logprobs is None else dict(logprobs=True)), **con_kw, **(dict(any_top_k=True) if any_top_k else {}))
        self.batch_release(st, range(st.pos.numel()))
        if P < 256:
            first_h = [self.batch_admit(st, j, x, sampling=sampling[j], penalties=penalties, **row_kw) for j in range(n)]
        else:
            self.batch_set_prefix(st, x)
            first_h = [self.batch_admit(st, j, x, sampling=sampling[j], share=True, penalties=penalties, **row_kw) for j in range(n)]
        first = torch.tensor(first_h, device=dev, dtype=torch.int64)
        eos_set = _eos_set(eos_token_id, self.lcfg.eos_token_id)
        n_steps = max_new_tokens - 1
        try:
            if return_logits:
                # the first token's logits are the prompt's last row for every sequence
                step_logits, ids = [st.staged_logits.float()[None].expand(n, -1).clone()], [first]
                torch.cuda.current_stream().synchronize()
                with torch.cuda.stream(st.stream):
                    for _ in range(n_steps):
                        self._batch_step(st)
                        step_logits.append(st.logits[:n].float().clone())
                        ids.append(st.token[:n].clone())
                st.stream.synchronize()
                return torch.stack(ids, 1), torch.stack(step_logits, 0)
            done_rows = [t in eos_set for t in first_h]
            done = 0
            torch.cuda.current_stream().synchronize()
            with torch.cuda.stream(st.stream):
                while done < n_steps and not all(done_rows):
                    chunk = min(16, n_steps - done)
                    if use_graph:
                        _replay(st, chunk)
                    else:
                        for _ in range(chunk):
                            self._batch_step(st)
                    done += chunk
                    got = st.out_ids[:n, :done].tolist()
                    done_rows = [first_h[b] in eos_set or any(t in eos_set for t in got[b]) for b in range(n)]
            st.stream.synchronize()
            toks = torch.cat([first[:, None], st.out_ids[:n, :done]], 1)
            out = finish_rows(toks.tolist(), eos_set, _pad_id(pad_token_id, eos_token_id, self.lcfg.eos_token_id), dev)
            if logprobs is not None:
                lens = [len(_cut_at_eos(r, eos_set)) for r in toks.tolist()]
                return out, self._pack_logprobs([self._row_logprobs(st, b, done) for b in range(n)], lens, out.shape[1], logprobs, dev)
            return out
        finally:
            self.batch_release(st, range(st.pos.numel()))

    def _generate_batch(self, inputs_embeds, attention_mask, max_new_tokens, eos_token_id, pad_token_id, use_graph: bool = True,
                        forced_ids: Optional[torch.Tensor] = None, return_logits: bool = False, sampling=None, penalties=None, logprobs=None,
                        constraint=None, any_top_k: bool = False, adapter=None, adapters=None):
        """The padded batch as ONE packed prefill (every row into its own KV-cache slot) + batched decode steps: the weights are streamed
        once per step for all rows.  Returns [B, n_new] right-padded with pad_token_id behind each row's EOS, like HF.
        forced_ids [B, n_new] / return_logits: teacher forcing for the parity tests (eager launches; the ids fed after step t are
        forced_ids[:, t]); returns (argmax ids [B, n_new], logits [n_new, B, V] fp32).
        sampling: None (greedy session) or one entry per row, (temperature, top_k in 1..64, top_p, seed) or None for a greedy row: the batch
        runs in a sampling session (`_batch_session(sampling=True)`), row b draws its first token with counter len_b - 1 and every step with
        the position of the token it consumes; under teacher forcing the returned ids are the ones each step CHOSE.
        penalties: None, or (rep, pres, freq) for every row (or one such entry / None per row): the batch runs in a session with the penalties flag,
        whose steps count the tokens they consume and pick from the penalised logits; the returned logits stay raw, the returned ids are the ones
        each step chose.
        logprobs: None, or k: the batch runs in a session with the logprobs flag and the call returns (ids, `Logprobs`) with k alternatives per
        token (not with forced_ids / return_logits).
        constraint: None, or an `Automaton` for every row (or a list with one / None per row): the batch runs in a session with the constraints flag;
        the first tokens are chosen from the prefill's rows masked from the start states, the returned logits stay raw, the returned ids are the
        ones each step chose.
        any_top_k (with sampling): the session carries the any_top_k flag, so a row's top_k may be 0 (no top-k filter) or above 64.
        adapters=bank with adapter = one name / None per row: the batch (1..16 rows; one row runs in a session of two) runs in a session with the
        bank, every row under its own adapter, unmerged.  The prefill is one packed call per adapter, over the rows that share it."""
        ops._need(inputs_embeds, dtype=None, name="inputs_embeds")
        any_kw = dict(any_top_k=True) if any_top_k and sampling is not None else {}
        if sampling is not None:
            sampling = [None if sp is None else self._check_batch_sampling(sp, "generate(batch_sample=True)", **any_kw) for sp in sampling]
        Bn, S, H = inputs_embeds.shape
        dev = inputs_embeds.device
        mask = attention_mask.bool() if attention_mask is not None else torch.ones((Bn, S), dtype=torch.bool, device=dev)
        lens = [int(v) for v in mask.sum(1).tolist()]
        packed = inputs_embeds.reshape(Bn * S, H)[mask.reshape(-1)].to(self.dtype).contiguous()
        cu_h = [0]
        for n in lens:
            cu_h.append(cu_h[-1] + n)
        cu = torch.tensor(cu_h, device=dev, dtype=torch.int32)
        pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).to(dev)
        seq = torch.cat([torch.full((n,), b, dtype=torch.int32) for b, n in enumerate(lens)]).to(dev)
        last = torch.tensor([c - 1 for c in cu_h[1:]], device=dev, dtype=torch.int32)
        max_ctx = ((max(lens) + max_new_tokens + 255) // 256) * 256
        if adapters is not None:
            return self._generate_batch_adapters(packed, lens, cu_h, max_ctx, max_new_tokens, eos_token_id, pad_token_id, use_graph, forced_ids, return_logits,
                                                 sampling, penalties, logprobs, constraint, any_kw, list(adapter), adapters)
        st = self._batch_session(Bn, max_ctx, max_new_tokens, sampling is not None, penalties=penalties is not None,
                                 **({} if logprobs is None else dict(logprobs=True)),
                                 **({} if constraint is None else dict(constraints=self._constraint_caps(self.CONSTRAIN_MAX_STATES, self.CONSTRAIN_MAX_CLASSES))),
                                 **any_kw)
        if penalties is not None:
            rows_pen = list(penalties) if isinstance(penalties, list) else [penalties] * Bn
            for b in range(Bn):
                self._set_penalties(st, b, rows_pen[b])
        r = self.prefill_packed(packed, pos, cu, max(lens), cache=st.cache, seq_of_tok=seq, last_rows=last)
        pick_from = r.last_logits
        if constraint is not None:
            rows_con = list(constraint) if isinstance(constraint, (list, tuple)) else [constraint] * Bn
            for b in range(Bn):
                self._set_constraint(st, b, rows_con[b])
            pick_from = [self._first_constrained(st, b, r.last_logits[b]) for b in range(Bn)]
        if sampling is None:
            first = torch.cat([ops.argmax(pick_from[b]) for b in range(Bn)])
        else:
            ctr = torch.tensor([n - 1 for n in lens], device=dev, dtype=torch.int32)
            first = torch.cat([ops.argmax(pick_from[b]) if sp is None else
                               ops.sample(pick_from[b], sp[0], sp[1], sp[2], sp[3], counter=ctr[b:b + 1]) for b, sp in enumerate(sampling)])
            for b, sp in enumerate(sampling):
                self._batch_set_sampling(st, b, sp)
        st.pos.copy_(torch.tensor(lens, dtype=torch.int32))
        st.n_out.zero_()
        st.token.copy_(first)
        if logprobs is not None:
            for b in range(Bn):
                self._first_logprobs(st, b, r.last_logits[b], first[b:b + 1])
        eos_set = _eos_set(eos_token_id, self.lcfg.eos_token_id)
        n_steps = max_new_tokens - 1
        if forced_ids is not None or return_logits:
            step_logits, ids = [r.last_logits[:Bn].float().clone()], [first]
            if forced_ids is not None:
                st.token.copy_(forced_ids[:, 0].to(dev))
            torch.cuda.current_stream().synchronize()
            with torch.cuda.stream(st.stream):
                for t in range(n_steps):
                    self._batch_step(st)
                    step_logits.append(st.logits[:Bn].float().clone())
                    ids.append(torch.cat([ops.argmax(st.logits[b]) for b in range(Bn)]) if sampling is None and getattr(st, "pen", None) is None and getattr(st, "con", None) is None else st.token[:Bn].clone())
                    if forced_ids is not None and t + 1 < forced_ids.shape[1]:
                        st.token.copy_(forced_ids[:, t + 1].to(dev))
            st.stream.synchronize()
            return torch.stack(ids, 1), torch.stack(step_logits, 0)
        if use_graph and st.graph is None and n_steps > 0:
            def restore():
                st.pos.copy_(torch.tensor(lens, dtype=torch.int32)); st.n_out.zero_(); st.token.copy_(first)
                if getattr(st, "pen", None) is not None:
                    st.counts.zero_()                              # the warm-up step outside capture bumped one count per row
                if constraint is not None:                         # ... and advanced every automaton by its first token
                    for b in range(Bn):
                        self._set_constraint(st, b, rows_con[b])
            _capture(st, lambda: self._batch_step(st), restore)
        first_h = first.tolist()
        done_rows = [t in eos_set for t in first_h]
        done = 0
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(st.stream):
            while done < n_steps and not all(done_rows):
                chunk = min(16, n_steps - done)
                if use_graph:
                    _replay(st, chunk)
                else:
                    for _ in range(chunk):
                        self._batch_step(st)
                done += chunk
                got = st.out_ids[:, :done].tolist()                 # one sync per 16 steps
                done_rows = [first_h[b] in eos_set or any(t in eos_set for t in got[b]) for b in range(Bn)]
        st.stream.synchronize()
        toks = torch.cat([first[:, None], st.out_ids[:, :done]], 1)
        out = finish_rows(toks.tolist(), eos_set, _pad_id(pad_token_id, eos_token_id, self.lcfg.eos_token_id), dev)
        if logprobs is not None:
            cut = [len(_cut_at_eos(row, eos_set)) for row in toks.tolist()]
            return out, self._pack_logprobs([self._row_logprobs(st, b, done) for b in range(Bn)], cut, out.shape[1], logprobs, dev)
        return out

    def _generate_batch_adapters(self, packed, lens, cu_h, max_ctx, max_new_tokens, eos_token_id, pad_token_id, use_graph, forced_ids, return_logits,
                                 sampling, penalties, logprobs, constraint, any_kw, names, bank):
        """`_generate_batch` in a session with an adapter bank: row b runs under names[b] (None: the base model).  The rows are those of a
        continuous-batching session: prefilled per adapter group into their slots, made live, stepped by the session's ONE graph, released."""
        Bn, dev = len(lens), packed.device
        st = self.batch_open(Bn, max_ctx, max_new_tokens, sampling=sampling is not None, penalties=penalties is not None,
                             **({} if logprobs is None else dict(logprobs=True)),
                             **({} if constraint is None else dict(constraints=True, max_states=self.CONSTRAIN_MAX_STATES, max_classes=self.CONSTRAIN_MAX_CLASSES)),
                             **any_kw, adapters=bank)
        self.batch_release(st, range(st.pos.numel()))
        try:
            st.stream.synchronize()
            last_logits = torch.empty((Bn, self.lcfg.vocab_size), device=dev, dtype=torch.float32)
            for name in dict.fromkeys(names):                          # one packed prefill per adapter, over the rows that share it
                rows = [b for b in range(Bn) if names[b] == name]
                x = torch.cat([packed[cu_h[b]:cu_h[b + 1]] for b in rows])
                cu = torch.tensor([0] + list(torch.tensor([lens[b] for b in rows]).cumsum(0).tolist()), device=dev, dtype=torch.int32)
                pos = torch.cat([torch.arange(lens[b], dtype=torch.int32) for b in rows]).to(dev)
                seq = torch.cat([torch.full((lens[b],), b, dtype=torch.int32) for b in rows]).to(dev)
                last = (cu[1:] - 1).contiguous()
                r = self.prefill_packed(x, pos, cu, max(lens[b] for b in rows), cache=st.cache, seq_of_tok=seq, last_rows=last,
                                        **({} if name is None else dict(adapter=name, adapters=bank)))
                last_logits[rows] = r.last_logits
            rows_pen = (list(penalties) if isinstance(penalties, list) else [penalties] * Bn) if penalties is not None else None
            rows_con = (list(constraint) if isinstance(constraint, (list, tuple)) else [constraint] * Bn) if constraint is not None else None
            ctr = torch.tensor([n - 1 for n in lens], device=dev, dtype=torch.int32)

            def arm():
                """Rows 0 .. Bn - 1 live at their prompts' ends with their first tokens; also what the capture's warm-up step is undone with."""
                firsts = []
                for b in range(Bn):
                    self._set_row_adapter(st, b, names[b])
                    pick_from = last_logits[b]
                    if rows_con is not None:
                        self._set_constraint(st, b, rows_con[b])
                        pick_from = self._first_constrained(st, b, last_logits[b])
                    sp = None if sampling is None else sampling[b]
                    firsts.append(ops.argmax(pick_from) if sp is None else ops.sample(pick_from, sp[0], sp[1], sp[2], sp[3], counter=ctr[b:b + 1]))
                    if sampling is not None:
                        self._batch_set_sampling(st, b, sp)
                    if rows_pen is not None:
                        self._set_penalties(st, b, rows_pen[b])
                first = torch.cat(firsts)
                st.pos[:Bn].copy_(torch.tensor(lens, dtype=torch.int32)); st.n_out.zero_(); st.token[:Bn].copy_(first)
                return first
            first = arm()
            if logprobs is not None:
                for b in range(Bn):
                    self._first_logprobs(st, b, last_logits[b], first[b:b + 1])
            eos_set = _eos_set(eos_token_id, self.lcfg.eos_token_id)
            n_steps = max_new_tokens - 1
            if forced_ids is not None or return_logits:
                step_logits, ids = [last_logits.clone()], [first]
                if forced_ids is not None:
                    st.token[:Bn].copy_(forced_ids[:, 0].to(dev))
                plain = sampling is None and rows_pen is None and rows_con is None
                torch.cuda.current_stream().synchronize()
                with torch.cuda.stream(st.stream):
                    for t in range(n_steps):
                        self._batch_step(st)
                        step_logits.append(st.logits[:Bn].float().clone())
                        ids.append(torch.cat([ops.argmax(st.logits[b]) for b in range(Bn)]) if plain else st.token[:Bn].clone())
                        if forced_ids is not None and t + 1 < forced_ids.shape[1]:
                            st.token[:Bn].copy_(forced_ids[:, t + 1].to(dev))
                st.stream.synchronize()
                return torch.stack(ids, 1), torch.stack(step_logits, 0)
            first_h = first.tolist()
            done_rows = [t in eos_set for t in first_h]
            done = 0
            torch.cuda.current_stream().synchronize()
            with torch.cuda.stream(st.stream):
                while done < n_steps and not all(done_rows):
                    chunk = min(16, n_steps - done)
                    if use_graph:
                        _replay(st, chunk)
                    else:
                        for _ in range(chunk):
                            self._batch_step(st)
                    done += chunk
                    got = st.out_ids[:Bn, :done].tolist()
                    done_rows = [first_h[b] in eos_set or any(t in eos_set for t in got[b]) for b in range(Bn)]
            st.stream.synchronize()
            toks = torch.cat([first[:, None], st.out_ids[:Bn, :done]], 1)
            out = finish_rows(toks.tolist(), eos_set, _pad_id(pad_token_id, eos_token_id, self.lcfg.eos_token_id), dev)
            if logprobs is not None:
                cut = [len(_cut_at_eos(row, eos_set)) for row in toks.tolist()]
                return out, self._pack_logprobs([self._row_logprobs(st, b, done) for b in range(Bn)], cut, out.shape[1], logprobs, dev)
            return out
        finally:
            self.batch_release(st, range(st.pos.numel()))

    def _fresh_seed(self) -> int:
        """The seed of a sampled request that names none: torch's initial seed stepped once per request."""
        self._sample_calls += 1
        return (torch.initial_seed() + 0x9E3779B97F4A7C15 * self._sample_calls) & 0xFFFFFFFFFFFFFFFF

    @torch.no_grad()
    def generate(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, max_new_tokens: Optional[int] = None,
                 eos_token_id=None, do_sample: Optional[bool] = None, temperature: Optional[float] = None, top_k: Optional[int] = None,
                 top_p: Optional[float] = None, seed: Optional[int] = None, pad_token_id: Optional[int] = None, generation_config=None,
                 use_graph: bool = True, return_logits: bool = False, forced_ids: Optional[torch.Tensor] = None, cache=None,
                 max_length: Optional[int] = None, streamer=None, batch_sample: Optional[bool] = None,
                 prompt_lookup_num_tokens: Optional[int] = None, max_matching_ngram_size: Optional[int] = None,
                 prompt_ids: Optional[torch.Tensor] = None, draft_ids: Optional[torch.Tensor] = None, past_len: Optional[int] = None,
                 prefill_chunk: Optional[int] = None, spec_sample: Optional[bool] = None, num_return_sequences: Optional[int] = None,
                 repetition_penalty: Optional[float] = None, presence_penalty: Optional[float] = None, frequency_penalty: Optional[float] = None,
                 logprobs: Optional[int] = None, constraint=None, any_top_k: Optional[bool] = None, spec_processed: Optional[bool] = None,
                 adapter=None, adapters=None, **kw):
        """`llm.generate(inputs_embeds=, attention_mask=, **generation_kwargs)` as called at llava_arch.py:833 (HF semantics: returns ONLY the
        new tokens, [B, n_new]).  Greedy search or sampling (do_sample: temperature / top_k / top_p, HF order, on the device); explicit
        keyword arguments override `generation_config` (HF GenerationConfig-like: do_sample, temperature, top_k, top_p, max_new_tokens,
        eos_token_id, pad_token_id).  The whole step (28 layers + lm_head + token choice + position advance) is one hipGraph replay; the host
        polls for EOS every 16 tokens.  A padded batch (B > 1) is served one sequence at a time through the same cache and graph (each row
        costs a batch-1 decode: weights are streamed once per row and token) and right-padded with pad_token_id like HF.
        batch_sample (opt-in, also read from generation_config; default False): a padded batch of 2..16 rows with do_sample and top_k in 1..64
        runs the batched step with its per-row sampler — one weight pass per step for all rows, row b seeded `seed + b` as the row-by-row loop
        seeds it.  The batched step sums in another order than the solo step, so the ids are no longer those of the rows' solo runs.
        num_return_sequences=n (HF's name; with do_sample=True and batch_sample=True, n in 2..16, top_k in 1..64, inputs_embeds [1, P, H]): n
        samples of ONE prompt, returned as [n, n_new].  The prompt is prefilled once (from 256 positions on; a shorter one shares nothing and is
        prefilled per row); its first P // 256 * 256 positions are the shared prefix of n sharing rows of a batch session (`batch_open(shared_prefix=True)`), whose steps read that K/V once for all rows.  Row j draws with seed
        `seed + j`, the seeds a padded batch of n copies would get.  Anything else (greedy, n > 16, a padded batch) raises a ValueError.
        forced_ids = teacher forcing for margin-aware parity tests.
        prompt_lookup_num_tokens=k (HF's name, also read from generation_config; 1..15; default None = off): greedy speculative decoding.  One
        graph replay runs the last token and up to k drafted ones as k + 1 positions of the sequence (`vila_llm_decode_step_verify`) and keeps the
        longest run the model itself would have chosen, so the ids are those of the same session drafting nothing.  Drafts come from an n-gram
        lookup (sizes max_matching_ngram_size, default 2, down to 1) in `prompt_ids` (LongTensor, optional) followed by what has been generated;
        draft_ids (LongTensor: a predicted output, token for token) replaces the lookup, with k = 7 unless given.  Batch 1 and greedy only;
        forced_ids and return_logits are not served in this mode.
        spec_sample (opt-in, also read from generation_config; default False): with do_sample=True, speculative decoding for a SAMPLED request
        (`vila_llm_decode_step_verify_sample`).  The sampler is counter-based: the token behind position p is a pure function of (logits bits,
        temperature, top_k, top_p, seed, p).  Row i of a step draws with counter pos + i, and a draft is accepted exactly when it equals that
        draw, so the ids are bit for bit those of the same sampled session drafting nothing — no statistical argument involved.  (Not HF's
        assisted-sampling rule: there a point-mass draft x is accepted with probability p(x); "the draw hits x" has the same probability,
        coupled to the request's fixed random stream.)  top_k in 1..64; without spec_sample a sampled request is refused in this mode as ever.
        streamer = HF's `generate(streamer=...)` contract (what server.py:243 streams from): `put(LongTensor[1])` once per new token — the EOS
        included, nothing for a prompt given as embeddings — as the host learns of them (every 16 graph replays), then `end()`; batch size 1.
        past_len=P with cache=c (both required together; batch size 1): slot 0 of `c` already holds the K/V of the sequence's first P positions
        (a previous generate on it), inputs_embeds holds only the NEW tokens, which are appended at P (`prefill_append`), and decoding goes on
        from P + S.  After n returned tokens the cache holds P + S + n - 1 valid positions: the last token was never fed.
        prefill_chunk=C (batch size 1): a prompt longer than C is fed as the usual prefill of its first C tokens and `prefill_append` calls of
        at most C, logits only from the last, so the prefill workspace is that of C tokens.  Both default to None: the one-shot path.
        repetition_penalty (HF's name and rule, also read from generation_config; > 0), presence_penalty, frequency_penalty (OpenAI's definitions,
        also read from generation_config; any finite float, negative ones reward repeats): applied on the device in front of the pick, greedy or
        sampled, solo or batched, bf16 or W4 (`vila_llm_decode_step[_batch]_penalized`).  They count the tokens this request has GENERATED: the
        prompt, given as embeddings, is not counted (HF's input_ids is empty then), so the first token is never penalised.  return_logits stays
        the raw model logits.  Neutral values (1, 0, 0 or None) take the unpenalised path, sessions and graphs untouched; the values never enter a
        session key, so one captured graph serves every penalised request.  With prompt_lookup_num_tokens / draft_ids / spec_sample only under
        spec_processed=True (below).
        logprobs=k (None = off, today's call and return value; 0..20): returns (ids, lp) with lp a `Logprobs`: token_logprobs [B, n_new] fp32 — the
        log-probability of every returned token —, top_logprobs [B, n_new, k] fp32 and top_ids [B, n_new, k] int64 — the k most likely tokens at
        that position, descending, ties towards the lower id.  They are RAW: log_softmax of the model's logits in fp32, independent of temperature,
        top-k, top-p and penalties (vLLM's default; `return_logits` is raw as well), computed on the device behind every step, inside the captured
        graph (`vila_logprobs_f32`).  The positions behind a row's EOS (the pads of `ids`) hold 0.0 / -inf / -1.  The session carries a `logprobs`
        flag in its key and always records 20 alternatives, so one graph serves any k.  Served on every path above except speculative decoding
        (prompt_lookup_num_tokens / draft_ids: only under spec_processed=True, below) and not together with return_logits or forced_ids.
        constraint = a `vila_amd.constrain.Automaton` (None = off, today's call): structured output.  The reply is held to the automaton's language —
        a choice list, a regular expression or a JSON schema compiled over this model's vocabulary (`ConstraintCompiler`).  On the device, between
        the penalties and temperature / top-k / top-p (where HF runs a caller's logits_processor): every step advances the automaton by the token
        it consumes and masks the disallowed ids to -inf before the pick (`vila_llm_decode_step[_batch]_constrained`), so a constrained step still
        replays from one graph; the automaton lives in device arrays, never in a session key.  Greedy or sampled, solo or batched (every row carries
        the automaton, with a state of its own), bf16 or W4, with batch_sample, num_return_sequences, penalties, logprobs (which stay RAW), cache= /
        past_len= / prefill_chunk.  return_logits stays raw, and its ids are the ones each step chose.  EOS is allowed exactly where the text is a
        member of the language; max_new_tokens can still cut the reply before that.  Not served with prompt_lookup_num_tokens / draft_ids /
        spec_sample unless spec_processed=True (below), and not with forced_ids (a forced token may leave the language).
        any_top_k (opt-in, also read from generation_config; default False): with it, batch_sample, num_return_sequences and spec_sample serve EVERY
        top_k >= 0 — 0 = no top-k filter (pure temperature / top-p sampling, HF's meaning) and k > 64 — where they serve 1..64 without it (a padded
        batch then runs row by row, the other two raise).  Such rows are drawn on the device by the solo sampler's exact selection, one block per
        row and one launch more per step (`vila_llm_decode_step_batch_any_k`, `vila_llm_decode_step_verify_any_k`): a row's token is bit for bit
        what `ops.sample` returns for the same logits, parameters, seed and counter.  The flag enters the session key, the values do not.
        spec_processed (opt-in, also read from generation_config; default False): with it, speculative decoding (prompt_lookup_num_tokens / draft_ids,
        with spec_sample and any_top_k where the request samples) also serves repetition_penalty / presence_penalty / frequency_penalty, constraint=
        and logprobs=k, in any mix, where each of them raises without it.  The verify step then runs the processing chain in front of its pick on
        the device (`vila_llm_decode_step_verify_processed`): row i of a step is penalised with the counts behind the tokens the step has consumed
        up to it and masked from the automaton's state behind them, the table and the state are committed behind the accept for the accepted
        rows only, and every emitted token gets its RAW record.  The ids (and the records) are bit for bit those of the same session drafting
        nothing.  With logprobs the call returns (ids, `Logprobs`), as the solo path does.  Batch 1; bf16 or W4; the flags enter the session key,
        the values and the automaton do not.
        adapters=bank (a `vila_amd.lora_serving.AdapterBank`; None = off, today's call) with adapter = the name of a loaded adapter, or one name /
        None per row: the 1..16 rows run under their adapters UNMERGED, through a batched session with the bank (`batch_open(adapters=)`; one row is
        a session of one live row) — the base weights stay as they are and rows of different adapters share every weight pass.  Prefill is one packed
        call per adapter; a row with None is the base model.  Served where the batched step is (bf16, head_dim 128, no cache=; sampling needs
        batch_sample=True with top_k in 1..64, or any_top_k), with penalties, logprobs, constraint, forced_ids and return_logits; anything else
        raises a ValueError.  Speculative decoding, past_len, prefill_chunk and num_return_sequences have no adapter form."""
        if adapter is not None or adapters is not None:
            if adapters is None:
                raise ValueError("generate(adapter=): pass the AdapterBank that holds the adapter as adapters=")
            gc_ = generation_config
            if (past_len is not None or prefill_chunk is not None or prompt_lookup_num_tokens is not None or draft_ids is not None or spec_sample or
                    (num_return_sequences is not None and int(num_return_sequences) != 1) or streamer is not None or
                    (gc_ is not None and getattr(gc_, "prompt_lookup_num_tokens", None) is not None)):
                raise ValueError("generate(adapters=): speculative decoding, past_len, prefill_chunk, num_return_sequences and streamer have no form under "
                                 "an unmerged adapter")
        self._check_append_args(inputs_embeds, cache, past_len, prefill_chunk)
        spec_processed = bool(spec_processed if spec_processed is not None else
                              (getattr(generation_config, "spec_processed", None) if generation_config is not None else False) or False)
        if constraint is not None:
            self._check_constraint(constraint, "generate")
            gc_ = generation_config
            if not spec_processed and (prompt_lookup_num_tokens is not None or draft_ids is not None or spec_sample or
                    (gc_ is not None and (getattr(gc_, "prompt_lookup_num_tokens", None) is not None or getattr(gc_, "spec_sample", None)))):
                raise ValueError("constraint is not served with speculative decoding (prompt_lookup_num_tokens, draft_ids, spec_sample): the verify "
                                 "steps have no constrained form")
            if forced_ids is not None:
                raise ValueError("constraint is not served with forced_ids: a forced token may leave the language")
        if logprobs is not None:
            if isinstance(logprobs, bool) or not isinstance(logprobs, numbers.Integral) or not 0 <= int(logprobs) <= ops.LOGPROBS_MAX_TOP:
                raise ValueError(f"`logprobs` has to be None or an integer in 0..{ops.LOGPROBS_MAX_TOP} (the number of top alternatives), but is {logprobs!r}")
            if return_logits or forced_ids is not None:
                raise ValueError("logprobs is not served together with return_logits / forced_ids: ask for one of them")
            gc_ = generation_config
            if not spec_processed and (prompt_lookup_num_tokens is not None or draft_ids is not None or
                                       (gc_ is not None and getattr(gc_, "prompt_lookup_num_tokens", None) is not None)):
                raise ValueError("logprobs is not served with speculative decoding (prompt_lookup_num_tokens / draft_ids): the verify steps have no "
                                 "logprob form")
            logprobs = int(logprobs)
        gc = generation_config
        pick = lambda v, name, default: v if v is not None else (getattr(gc, name, None) if gc is not None and getattr(gc, name, None) is not None else default)
        penalties = self._check_penalties(pick(repetition_penalty, "repetition_penalty", None), pick(presence_penalty, "presence_penalty", None),
                                          pick(frequency_penalty, "frequency_penalty", None))
        if penalties is not None and not spec_processed and (pick(prompt_lookup_num_tokens, "prompt_lookup_num_tokens", None) is not None or
                                                             draft_ids is not None or bool(pick(spec_sample, "spec_sample", False))):
            raise ValueError("repetition_penalty / presence_penalty / frequency_penalty are not served with speculative decoding "
                             "(prompt_lookup_num_tokens, draft_ids, spec_sample): the verify step has no penalised form")
        if num_return_sequences is not None and int(num_return_sequences) != 1:
            return self._generate_return_sequences(inputs_embeds, attention_mask, int(num_return_sequences), max_new_tokens, eos_token_id, do_sample,
                                                   temperature, top_k, top_p, seed, pad_token_id, generation_config, use_graph, return_logits,
                                                   forced_ids, cache, streamer, batch_sample, prompt_lookup_num_tokens, draft_ids, past_len, prefill_chunk,
                                                   penalties, **({} if logprobs is None else dict(logprobs=logprobs)),
                                                   **({} if constraint is None else dict(constraint=constraint)),
                                                   **({} if any_top_k is None else dict(any_top_k=any_top_k)))
        if streamer is not None and inputs_embeds.shape[0] > 1:
            raise ValueError("TextStreamer only supports batch size 1")          # transformers/generation/streamers.py, TextStreamer.put
        do_sample = bool(pick(do_sample, "do_sample", False))
        temperature, top_k, top_p = float(pick(temperature, "temperature", 1.0)), int(pick(top_k, "top_k", 50)), float(pick(top_p, "top_p", 1.0))
        max_new_tokens = int(pick(max_new_tokens, "max_new_tokens", 32))
        eos_token_id = pick(eos_token_id, "eos_token_id", None)
        pad_token_id = pick(pad_token_id, "pad_token_id", None)
        batch_sample = bool(pick(batch_sample, "batch_sample", False))
        any_top_k = bool(pick(any_top_k, "any_top_k", False))
        k_spec = pick(prompt_lookup_num_tokens, "prompt_lookup_num_tokens", None)
        if k_spec is not None or draft_ids is not None:
            k_spec = 7 if k_spec is None else int(k_spec)
            spec_sample = bool(pick(spec_sample, "spec_sample", False))
            if do_sample and not spec_sample:
                raise ValueError("prompt_lookup_num_tokens / draft_ids: speculative decoding here is greedy; do_sample=True is not supported with it "
                                 "(spec_sample=True opts a sampled request in)")
            if inputs_embeds.shape[0] != 1:
                raise ValueError("prompt_lookup_num_tokens / draft_ids: speculative decoding serves batch size 1 (as HF's assisted generation does)")
            if not 1 <= k_spec <= 15:
                raise ValueError(f"prompt_lookup_num_tokens has to be in 1..15 (a step runs k + 1 <= 16 rows), but is {k_spec}")
            max_ngram = int(pick(max_matching_ngram_size, "max_matching_ngram_size", 2))
            if max_ngram < 1:
                raise ValueError(f"max_matching_ngram_size has to be a positive integer, but is {max_ngram}")
            if forced_ids is not None or return_logits:
                raise ValueError("prompt_lookup_num_tokens / draft_ids: forced_ids and return_logits are not supported in this mode")
            sampling = None
            if do_sample:
                if temperature <= 0:
                    raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float, otherwise your next token scores will be invalid.")
                if any_top_k and top_k < 0:
                    raise ValueError(f"`top_k` has to be a non-negative integer, but is {top_k}")
                if not 1 <= top_k <= 64 and not any_top_k:
                    raise ValueError(f"spec_sample: the sampled verify step serves top_k in 1..64 (got top_k = {top_k})")
                if not 0.0 < top_p <= 1.0:
                    raise ValueError(f"`top_p` has to be a float > 0 and <= 1, but is {top_p}")
                sampling = (temperature, top_k, top_p, int(self._fresh_seed() if seed is None else seed))
            proc_kw = {}                                              # (keywords only when asked: a call without them makes the calls it always made)
            if spec_processed:
                proc_kw = dict(**({} if penalties is None else dict(penalties=penalties)), **({} if logprobs is None else dict(logprobs=logprobs)),
                               **({} if constraint is None else dict(constraint=constraint)))
            return self._generate_verify(inputs_embeds, attention_mask, max_new_tokens, eos_token_id, k_spec, max_ngram, prompt_ids, draft_ids, cache, streamer,
                                         past_len, prefill_chunk, sampling, **(dict(any_top_k=True) if any_top_k and sampling is not None else {}), **proc_kw)
        if do_sample and temperature <= 0:
            raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float, otherwise your next token scores will be invalid.")
        if do_sample and top_k < 0:
            raise ValueError(f"`top_k` has to be a non-negative integer, but is {top_k}")       # (0 = no top-k filter, like HF)
        # (a penalised greedy batch is teacher-forced and returns its logits through the batched step as well: its ids are the step's own picks)
        pen_kw = {} if penalties is None else dict(penalties=penalties)
        if logprobs is not None:                                       # (keyword only when asked: a call without it makes the calls it always made)
            pen_kw = dict(pen_kw, logprobs=logprobs)
        if constraint is not None:                                     # (likewise)
            pen_kw = dict(pen_kw, constraint=constraint)
        processed = penalties is not None or constraint is not None    # (a constrained greedy batch returns its logits through the batched step too)
        if adapters is not None:
            Bn = inputs_embeds.shape[0]
            names = list(adapter) if isinstance(adapter, (list, tuple)) else [adapter] * Bn
            if len(names) != Bn:
                raise ValueError(f"generate(adapter=): {len(names)} adapter names for {Bn} rows")
            for nm in names:
                adapters.slot_of(nm)                                   # (raises for a name that is not loaded)
            # what `_can_batch_decode` asks of a batch, on 1..16 rows (it asks for 2..16: one row joins a session of two)
            probe = inputs_embeds if Bn > 1 else inputs_embeds.expand(2, -1, -1)
            if self._w4 is not None or not self._can_batch_decode(probe, attention_mask, max_new_tokens, do_sample, None, False, cache, batch_sample, top_k,
                                                                 **(dict(any_top_k=True) if any_top_k else {})):
                raise ValueError("generate(adapters=): rows under unmerged adapters run through the batched step — 1..16 rows of a bf16 head-dim-128 "
                                 "model, no cache=, and for do_sample batch_sample=True with top_k in 1..64 (any top_k with any_top_k=True)")
            rows = None
            if do_sample:
                if seed is None:
                    seed = self._fresh_seed()
                rows = [(temperature, top_k, top_p, (int(seed) + b) & 0xFFFFFFFFFFFFFFFF) for b in range(Bn)]
            return self._generate_batch(inputs_embeds, attention_mask, max_new_tokens, eos_token_id, pad_token_id, use_graph, forced_ids, return_logits,
                                        sampling=rows, **pen_kw, **(dict(any_top_k=True) if any_top_k else {}), adapter=names, adapters=adapters)
        if inputs_embeds.shape[0] > 1 and self._can_batch_decode(inputs_embeds, attention_mask, max_new_tokens, do_sample,
                                                                 forced_ids if not processed else None, return_logits and not processed, cache,
                                                                 batch_sample, top_k, **(dict(any_top_k=True) if any_top_k else {})):
            if not do_sample:
                if not processed and logprobs is None:
                    return self._generate_batch(inputs_embeds, attention_mask, max_new_tokens, eos_token_id, pad_token_id, use_graph)
                return self._generate_batch(inputs_embeds, attention_mask, max_new_tokens, eos_token_id, pad_token_id, use_graph, forced_ids,
                                            return_logits, **pen_kw)
            if seed is None:
                seed = self._fresh_seed()
            rows = [(temperature, top_k, top_p, (int(seed) + b) & 0xFFFFFFFFFFFFFFFF) for b in range(inputs_embeds.shape[0])]
            return self._generate_batch(inputs_embeds, attention_mask, max_new_tokens, eos_token_id, pad_token_id, use_graph, forced_ids,
                                        return_logits, sampling=rows, **pen_kw, **(dict(any_top_k=True) if any_top_k else {}))
        if inputs_embeds.shape[0] > 1:
            rows = []
            row_pen = {} if penalties is None else dict(repetition_penalty=penalties[0], presence_penalty=penalties[1], frequency_penalty=penalties[2])
            if logprobs is not None:
                row_pen = dict(row_pen, logprobs=logprobs)
            if constraint is not None:
                row_pen = dict(row_pen, constraint=constraint)
            recs = []
            for b in range(inputs_embeds.shape[0]):
                m = None if attention_mask is None else attention_mask[b:b + 1]
                got = self.generate(inputs_embeds[b:b + 1], m, max_new_tokens, eos_token_id, do_sample, temperature, top_k, top_p,
                                    None if seed is None else seed + b, pad_token_id, None, use_graph, False, None, cache, max_length, **row_pen)
                if logprobs is not None:
                    got, lp = got
                    recs.append((lp.token_logprobs[0], lp.top_logprobs[0], lp.top_ids[0]))
                rows.append(got[0])
            out = finish_rows([r.tolist() for r in rows], _eos_set(eos_token_id, self.lcfg.eos_token_id),
                              _pad_id(pad_token_id, eos_token_id, self.lcfg.eos_token_id), rows[0].device)
            if logprobs is not None:                                   # (a solo row is cut at its EOS already: its records are its tokens)
                return out, self._pack_logprobs(recs, [r.numel() for r in rows], out.shape[1], logprobs, out.device)
            return out
        sampling = None
        if do_sample:
            if seed is None:
                seed = self._fresh_seed()
            sampling = (temperature, top_k, top_p, int(seed))
        return self._generate_solo(inputs_embeds, attention_mask, max_new_tokens, eos_token_id, sampling, use_graph, return_logits, forced_ids, cache,
                                   streamer, past_len, prefill_chunk, **pen_kw)

    def _generate_return_sequences(self, inputs_embeds, attention_mask, n, max_new_tokens, eos_token_id, do_sample, temperature, top_k, top_p, seed,
                                   pad_token_id, gc, use_graph, return_logits, forced_ids, cache, streamer, batch_sample, k_spec, draft_ids, past_len,
                                   prefill_chunk, penalties=None, logprobs=None, constraint=None, any_top_k=None):
        """generate(num_return_sequences=n): what is served, refused with a ValueError that says so otherwise."""
        pick = lambda v, name, default: v if v is not None else (getattr(gc, name, None) if gc is not None and getattr(gc, name, None) is not None else default)
        what = "num_return_sequences: n samples of ONE prompt over its shared K/V"
        if not bool(pick(do_sample, "do_sample", False)):
            raise ValueError(f"{what} needs do_sample=True (greedy search returns n copies of one sequence; it is not served)")
        if not bool(pick(batch_sample, "batch_sample", False)):
            raise ValueError(f"{what} runs the batched sampler: pass batch_sample=True")
        if not 2 <= n <= 16:
            raise ValueError(f"{what} serves n in 2..16 (got {n})")
        if inputs_embeds.dim() != 3 or inputs_embeds.shape[0] != 1 or (attention_mask is not None and not bool(attention_mask.bool().all())):
            raise ValueError(f"{what} takes inputs_embeds [1, P, H] without padding (a padded batch is not served)")
        if (forced_ids is not None or cache is not None or streamer is not None or k_spec is not None or draft_ids is not None or past_len is not None or
                prefill_chunk is not None):
            raise ValueError(f"{what} does not combine with forced_ids, cache, streamer, speculative decoding, past_len or prefill_chunk")
        temperature, top_k, top_p = float(pick(temperature, "temperature", 1.0)), int(pick(top_k, "top_k", 50)), float(pick(top_p, "top_p", 1.0))
        max_new_tokens = int(pick(max_new_tokens, "max_new_tokens", 32))
        if max_new_tokens < 1 or not self.can_batch_decode_step() or not self._long_batch_group_ok() or not (self._w4_batched() or self._qkv_fused()):
            raise ValueError(f"{what} needs max_new_tokens >= 1 and a model the batched step serves (head_dim 128, GQA group 1, 2, 4, 7 or 8)")
        if inputs_embeds.shape[1] + max_new_tokens > self.BATCH_MAX_CTX:
            raise ValueError(f"{what}: prompt and output must fit {self.BATCH_MAX_CTX} positions")
        if return_logits and inputs_embeds.shape[1] < 256:
            raise ValueError(f"{what}: return_logits needs a prompt of at least 256 positions (a shorter one shares nothing and its rows are admitted "
                             "one by one)")
        if seed is None:
            seed = self._fresh_seed()
        any_kw = dict(any_top_k=True) if bool(pick(any_top_k, "any_top_k", False)) else {}
        rows = [self._check_batch_sampling((temperature, top_k, top_p, (int(seed) + j) & 0xFFFFFFFFFFFFFFFF), "generate(num_return_sequences=)", **any_kw)
                for j in range(n)]
        return self._generate_shared(inputs_embeds, n, max_new_tokens, pick(eos_token_id, "eos_token_id", None), pick(pad_token_id, "pad_token_id", None),
                                     use_graph, return_logits, rows, **({} if penalties is None else dict(penalties=penalties)),
                                     **({} if logprobs is None else dict(logprobs=logprobs)),
                                     **({} if constraint is None else dict(constraint=constraint)), **any_kw)

    @staticmethod
    def _check_append_args(inputs_embeds, cache, past_len, prefill_chunk) -> None:
        """generate()'s past_len / prefill_chunk, refused before anything runs."""
        if past_len is not None:
            if cache is None:
                raise ValueError("past_len: the caller's `cache` (whose slot 0 holds the first past_len positions) is required with it")
            if inputs_embeds.shape[0] != 1:
                raise ValueError(f"past_len: continuing a cache serves batch size 1 (got {inputs_embeds.shape[0]})")
            if int(past_len) < 0:
                raise ValueError(f"past_len has to be a non-negative integer, but is {past_len}")
        if prefill_chunk is not None:
            if int(prefill_chunk) < 1:
                raise ValueError(f"prefill_chunk has to be a positive integer, but is {prefill_chunk}")
            if inputs_embeds.shape[0] != 1:
                raise ValueError(f"prefill_chunk: a chunked prefill serves batch size 1 (got {inputs_embeds.shape[0]})")

    def _cache_for(self, S: int, max_new_tokens: int, cache):
        """A one-sequence generate()'s KV cache: the caller's, or `_own_cache`, re-made at the next multiple of 256 when missing or too small."""
        if cache is None:
            cache = self._own_cache
            if cache is None or cache.max_ctx < S + max_new_tokens:
                cache = self._own_cache = self.new_cache(((S + max_new_tokens + 255) // 256) * 256)
        if cache.max_ctx < S + max_new_tokens:
            raise ValueError(f"KV cache too small: {cache.max_ctx} < {S} + {max_new_tokens}")
        return cache

    def _prefill_one(self, inputs_embeds, attention_mask, max_new_tokens, cache, admit=None, past_len=None, prefill_chunk=None):
        """The opening of a one-sequence generate(): the row cut by its mask, its cache, the prefill.  admit(cache) may refuse the cache before
        any kernel runs.  Returns (S, cache, the prefill's result, the last row's index as a device int32[1]).  With past_len or a prompt longer
        than prefill_chunk the prompt reaches the cache through `prefill_append`; S is then the number of positions the cache holds afterwards
        and the index that of the last position, as for a one-shot prefill of the whole sequence."""
        ops._need(inputs_embeds, dtype=None, name="inputs_embeds")
        x = inputs_embeds[0]
        if attention_mask is not None:
            x = x[attention_mask[0].bool()]
        S, dev = x.shape[0], x.device
        P = 0 if past_len is None else int(past_len)
        cache = self._cache_for(P + S, max_new_tokens, cache)
        if admit is not None:
            admit(cache)
        if past_len is not None or (prefill_chunk is not None and S > int(prefill_chunk)):
            x = x.to(self.dtype)
            step = S if prefill_chunk is None else int(prefill_chunk)
            off, r = 0, None
            if past_len is None:                                    # an empty cache: the first chunk is the prefill as it always was
                self.prefill_packed(x[:step], torch.arange(step, device=dev, dtype=torch.int32), None, step, cache=cache)
                off = step
            while off < S:
                n = min(step, S - off)
                rows = torch.full((1,), n - 1, device=dev, dtype=torch.int32) if off + n == S else None
                r = self.prefill_append(x[off:off + n], cache, P + off, 0, last_rows=rows)
                off += n
            return P + S, cache, r, torch.full((1,), P + S - 1, device=dev, dtype=torch.int32)
        pos = torch.arange(S, device=dev, dtype=torch.int32)
        last = torch.full((1,), S - 1, device=dev, dtype=torch.int32)          # (a fill kernel, not a host copy)
        return S, cache, self.prefill_packed(x.to(self.dtype), pos, None, S, cache=cache, last_rows=last), last

    def _generate_solo(self, inputs_embeds, attention_mask, max_new_tokens, eos_token_id, sampling, use_graph, return_logits, forced_ids, cache,
                       streamer, past_len=None, prefill_chunk=None, penalties=None, logprobs=None, constraint=None):
        """generate() for one sequence: prefill, then the batch-1 step (one hipGraph replay per token, or step by step under `use_graph=False`,
        `return_logits` or `forced_ids`).  sampling: None (greedy) or (temperature, top_k, top_p, seed).
        penalties: None, or (rep, pres, freq): the session carries the penalties flag, its counts start from zero here (a request starts), and the
        ids returned with return_logits are the ones each step chose from the penalised logits.
        logprobs: None, or k: the session carries the logprobs flag and the call returns (ids, `Logprobs`) with k alternatives per token.
        constraint: None, or an `Automaton`: the session carries the constraints flag, the automaton starts from its start state here, the first
        token is chosen from the prefill's row masked from that state, and the ids returned with return_logits are the ones each step chose."""
        S, cache, r, last = self._prefill_one(inputs_embeds, attention_mask, max_new_tokens, cache, None, past_len, prefill_chunk)
        dev = inputs_embeds.device
        eos_set = _eos_set(eos_token_id, self.lcfg.eos_token_id)
        st = self._decode_session(cache, max_new_tokens, sampling, **({} if penalties is None else dict(penalties=True)),
                                  **({} if logprobs is None else dict(logprobs=True)),
                                  **({} if constraint is None else dict(constraints=self._constraint_caps(self.CONSTRAIN_MAX_STATES, self.CONSTRAIN_MAX_CLASSES))))
        if penalties is not None:
            self._set_penalties(st, 0, penalties)
        pick_from = r.last_logits[0]
        if constraint is not None:
            self._set_constraint(st, 0, constraint)
            pick_from = self._first_constrained(st, 0, pick_from)
        # the sampler mixes a device counter into its random number: the decode steps use the position of the token they consume
        # (S, S+1, ...); the first token, drawn from the prefill's logits, uses S - 1
        first = ops.argmax(pick_from) if sampling is None else ops.sample(pick_from, *sampling, counter=last)
        step_logits = [r.last_logits[0].clone()] if return_logits else None
        if logprobs is not None:
            self._first_logprobs(st, 0, r.last_logits[0], first)
        st.pos.fill_(S)
        st.n_out.zero_()
        st.token.copy_(first if forced_ids is None else forced_ids[:1].to(dev))
        ids = [first]
        eager = (not use_graph) or return_logits or (forced_ids is not None)
        if not eager and st.graph is None:
            def restore():
                st.pos.fill_(S); st.n_out.zero_(); st.token.copy_(first)
                if penalties is not None:
                    st.counts.zero_()                              # the warm-up step outside capture bumped the first token's count
                if constraint is not None:
                    self._set_constraint(st, 0, constraint)        # ... and advanced the automaton by it
            _capture(st, lambda: self.decode_step(cache, st), restore)
        n_steps = max_new_tokens - 1
        if eager:
            for t in range(n_steps):
                self.decode_step(cache, st)
                if return_logits:
                    step_logits.append(st.logits.clone())
                    ids.append(ops.argmax(st.logits) if sampling is None and penalties is None and constraint is None else st.token.clone())
                if forced_ids is not None and t + 1 < forced_ids.numel():
                    st.token.copy_(forced_ids[t + 1:t + 2].to(dev))
            if not return_logits:
                out = torch.cat([first, st.out_ids[:n_steps]])
            else:
                out = torch.cat(ids)
        else:
            torch.cuda.current_stream().synchronize()
            done = 0
            first_id = first.item()
            stop = first_id in eos_set
            _stream_put(streamer, first_id)
            with torch.cuda.stream(st.stream):
                while done < n_steps and not stop:
                    chunk = min(16, n_steps - done)
                    _replay(st, chunk)
                    got = st.out_ids[:done + chunk].tolist()       # one sync per 16 tokens
                    if streamer is not None:
                        for t in got[done:]:
                            _stream_put(streamer, t)
                            if t in eos_set:
                                break
                    done += chunk
                    stop = any(t in eos_set for t in got)
            st.stream.synchronize()
            out = torch.cat([first, st.out_ids[:done]])
        if forced_ids is None:
            out = out[:len(_cut_at_eos(out.tolist(), eos_set))]
        if streamer is not None:
            if eager:                                       # the step-by-step paths learn of their tokens at the end
                for t in out.tolist():
                    _stream_put(streamer, t)
            streamer.end()
        out = out[None]
        if logprobs is not None:                                   # (cut at the EOS like `out`: record t belongs to out[0, t])
            m = out.shape[1]
            return out, self._pack_logprobs([self._row_logprobs(st, 0, m - 1)], [m], m, logprobs, dev)
        return (out, torch.stack(step_logits)) if return_logits else out

    # ---- speculative decoding: lookup drafts, k + 1 rows of one sequence per step (vila_llm_decode_step_verify[_sample]) -------------------
    spec_trace = None           # diagnostics / tests: set to a list and _generate_verify syncs after every replay and appends its n_accept
    spec_probe = None           # ... and, with spec_trace set, a callable invoked with the session after every such replay (one replay, synced): it may
                                # read st.logits, st.token, st.n_out, st.n_accept of that replay

    def _verify_refusal(self) -> Optional[str]:
        """Why this model has no verify step, or None.  The restrictions are the batched step's."""
        c = self.lcfg
        if c.head_dim != 128 or c.num_attention_heads * c.head_dim != c.hidden_size or not self._long_batch_group_ok():
            return ("the verify step needs head_dim 128, q_heads * head_dim == hidden and a GQA group of 1, 2, 4, 7 or 8 query heads per kv head "
                    f"(got head_dim {c.head_dim}, {c.num_attention_heads} / {c.num_key_value_heads} heads, hidden {c.hidden_size})")
        if self._w4 is not None and not self._w4_batched():
            return "a quantised model needs quantize_w4(batch_decode=True) for the verify step (it runs the W4A16 batched GEMVs)"
        if self._w4 is None and not self._qkv_fused():
            return "the verify step reads q/k/v as one fused [q + 2kv, hidden] buffer (refuse() re-establishes it)"
        return None

    def _verify_session(self, cache, n: int, max_out: int, max_ngram: int, sampled: bool = False, any_top_k: bool = False, penalties: bool = False,
                        constraints=None, logprobs: bool = False):
        """Device-resident state of a verify session (+ its captured hipGraph), keyed like `_decode_session`.  sampled: the session steps through
        the `_sample` entry points (another graph, hence part of the key) and owns the request's four sampling parameters as ONE-entry device
        tensors that `_verify_set_sampling` rewrites per request: neither the parameters nor the seed are baked into the graph.
        any_top_k (sampled sessions; in the key only when set): the session steps through `vila_llm_decode_step_verify_any_k`, whose draws serve
        every top_k >= 0.
        penalties / constraints=(max_states, max_classes) / logprobs (each in the key only when set): the session steps through
        `vila_llm_decode_step_verify_processed` and owns ONE count row with the three one-entry parameter tensors (`_penalty_state`), the bound
        automaton arrays (`_constraint_state`) and the record arrays (`_logprob_state`), all at n = 1: the step's rows are ONE sequence.  The
        values and the automaton are rewritten per request; the graph stays."""
        w4 = self._w4_batched()
        key = (cache.k.data_ptr(), cache.max_ctx, n, max_out, max_ngram, bool(sampled), *self._weights_key()) + (("any_top_k",) if any_top_k and sampled else ())
        processed = bool(penalties) or bool(constraints) or bool(logprobs)
        key += ("penalties",) if penalties else ()
        key += ("constraints", *constraints) if constraints else ()
        key += ("logprobs",) if logprobs else ()
        if self._vdecode is not None and self._vdecode.key == key:
            return self._vdecode
        self._drop_session("_vdecode")
        dev, lib, w = self.device, _lib.load(), self._struct()
        st = SimpleNamespace(key=key, cache=cache, graph=None, n=n, max_out=max_out, w4=w4, sampled=bool(sampled), sp=None)
        if any_top_k and sampled:
            st.any_k = True
        i32 = lambda m: torch.zeros(m, device=dev, dtype=torch.int32)
        with torch.inference_mode(False):
            st.pos, st.n_draft, st.n_out, st.n_accept, st.n_hist, st.n_cand = i32(1), i32(1), i32(1), i32(1), i32(1), i32(1)
            st.token = torch.zeros(n, device=dev, dtype=torch.int64)
            st.out_ids = torch.zeros(max_out, device=dev, dtype=torch.int64)
            st.cand = torch.zeros(max_out, device=dev, dtype=torch.int64)
            st.hist = torch.zeros(cache.max_ctx + max_out + 1, device=dev, dtype=torch.int64)
            st.logits = torch.zeros((n, self.lcfg.vocab_size), device=dev, dtype=torch.float32)
            ws_bytes = getattr(lib, _step_symbols(True, w4, False, verify=not sampled, verify_sample=bool(sampled), **(dict(processed=True) if processed else {}))[1])
            st.ws = torch.empty((ws_bytes(C.byref(w.shape), n, cache.max_ctx),), device=dev, dtype=torch.uint8)
            if processed:
                st.processed = True
                if penalties:
                    self._penalty_state(st, 1, self.lcfg.vocab_size, dev)
                if constraints:
                    self._constraint_state(st, 1, self.lcfg.vocab_size, constraints, dev)
                if logprobs:
                    self._logprob_state(st, 1, max_out, dev)
            if sampled:                                             # ONE entry each: every row of a step reads entry 0
                st.s_temperature = torch.zeros(1, device=dev, dtype=torch.float32)
                st.s_top_k = torch.full((1,), 50, device=dev, dtype=torch.int32)
                st.s_top_p = torch.ones(1, device=dev, dtype=torch.float32)
                st.s_seed = torch.zeros(1, device=dev, dtype=torch.int64)                   # bit pattern of a uint64 seed
                st.sp = _lib.VilaBatchSampling(st.s_temperature.data_ptr(), st.s_top_k.data_ptr(), st.s_top_p.data_ptr(), st.s_seed.data_ptr())
        st.c = _lib.VilaDecodeVerify(n, 0, st.pos.data_ptr(), st.token.data_ptr(), st.n_draft.data_ptr(), st.out_ids.data_ptr(), st.n_out.data_ptr(), max_out,
                                     st.logits.data_ptr(), st.n_accept.data_ptr(), st.hist.data_ptr(), st.n_hist.data_ptr(), st.hist.numel(), max_ngram,
                                     st.cand.data_ptr(), st.n_cand.data_ptr())
        st.stream = torch.cuda.Stream(device=dev)
        self._vdecode = st
        return st

    @staticmethod
    def _verify_set_sampling(st, sampling) -> None:
        """Write a request's (temperature, top_k, top_p, seed) into a sampled verify session's one-entry device tensors: the next replay reads them."""
        t, k, p, seed = sampling
        st.s_temperature.fill_(float(t))
        st.s_top_k.fill_(int(k))
        st.s_top_p.fill_(float(p))
        st.s_seed.fill_(_as_i64(seed))

    def verify_step(self, cache, st) -> None:
        """One verify step on the current stream: draft, forward of st.n rows, pick or draw, accept."""
        if not st.w4:
            self._require_bf16("the bf16 verify step")
        self._step(True, self._w4 if st.w4 else None, cache, st, st.sp if st.sampled else None, verify=not st.sampled, verify_sample=st.sampled)

    def _generate_verify(self, inputs_embeds, attention_mask, max_new_tokens, eos_token_id, k, max_ngram, prompt_ids, draft_ids, cache, streamer,
                         past_len=None, prefill_chunk=None, sampling=None, any_top_k: bool = False, penalties=None, logprobs=None, constraint=None):
        """generate() for one sequence with the verify step: prefill as `_generate_solo`, first token from the prefill, then graph replays
        that each append 1 .. k + 1 tokens.  The host cuts at EOS and at max_new_tokens (a step may overshoot by up to k).
        sampling: None (greedy) or (temperature, top_k in 1..64, top_p, seed): the first token is drawn from the prefill's last row with counter
        S - 1, as `_generate_solo` draws it, and the steps draw with the positions of the tokens they consume (S, S + 1, ...).
        any_top_k (with sampling): the session carries the any_top_k flag, so top_k may be 0 (no top-k filter) or above 64.
        penalties / logprobs / constraint (generate(spec_processed=True)): as `_generate_solo` takes them.  The session carries the matching flags and
        steps through the processed verify step; the first token is picked / drawn and recorded eagerly from the prefill's last row — penalties see
        an empty table, the mask runs from the start state with no advance — and with logprobs the call returns (ids, `Logprobs`)."""
        why = self._verify_refusal()
        if why is not None:
            raise ValueError("prompt_lookup_num_tokens / draft_ids: " + why)
        def admit(c):
            if c.max_ctx > self.BATCH_MAX_CTX:
                raise ValueError(f"prompt_lookup_num_tokens / draft_ids: the verify step serves caches up to {self.BATCH_MAX_CTX} positions (got {c.max_ctx})")
        S, cache, r, last = self._prefill_one(inputs_embeds, attention_mask, max_new_tokens, cache, admit, past_len, prefill_chunk)
        dev, n = inputs_embeds.device, k + 1
        eos_set = _eos_set(eos_token_id, self.lcfg.eos_token_id)
        need = max_new_tokens - 1                                   # tokens wanted from the steps
        st = self._verify_session(cache, n, max(max_new_tokens, 1) + k, max_ngram, sampling is not None,
                                  **(dict(any_top_k=True) if any_top_k and sampling is not None else {}),
                                  **({} if penalties is None else dict(penalties=True)),
                                  **({} if constraint is None else dict(constraints=self._constraint_caps(self.CONSTRAIN_MAX_STATES, self.CONSTRAIN_MAX_CLASSES))),
                                  **({} if logprobs is None else dict(logprobs=True)))
        if sampling is not None:
            self._verify_set_sampling(st, sampling)
        if penalties is not None:
            self._set_penalties(st, 0, penalties)
        pick_from = r.last_logits[0]
        if constraint is not None:
            self._set_constraint(st, 0, constraint)
            pick_from = self._first_constrained(st, 0, pick_from)
        first = ops.argmax(pick_from) if sampling is None else ops.sample(pick_from, *sampling, counter=last)
        if logprobs is not None:
            self._first_logprobs(st, 0, r.last_logits[0], first)
        # the history the lookup starts from: the prompt's ids (its tail, if longer than the room) and the first token
        room = st.hist.numel() - st.max_out - 1
        pids = torch.zeros(0, dtype=torch.int64, device=dev) if prompt_ids is None else prompt_ids.reshape(-1).to(device=dev, dtype=torch.int64)[-room:]
        n0 = pids.numel() + 1
        st.hist[:n0 - 1].copy_(pids)
        st.hist[n0 - 1:n0].copy_(first)
        if draft_ids is not None:                                   # a predicted output: its token t is the draft for output token t (t = 0 is `first`)
            cand = draft_ids.reshape(-1).to(device=dev, dtype=torch.int64)[1:st.max_out + 1]
            st.cand[:cand.numel()].copy_(cand)
            st.n_cand.fill_(cand.numel())
        else:
            st.n_cand.fill_(-1)

        def restore():
            st.pos.fill_(S); st.n_out.zero_(); st.n_hist.fill_(n0); st.token[:1].copy_(first)
            if penalties is not None:
                st.counts.zero_()                                   # the warm-up step outside capture committed what it consumed
            if constraint is not None:
                self._set_constraint(st, 0, constraint)             # ... moved the automaton
            if logprobs is not None:                                # ... and wrote the records of what it emitted
                st.lp_tok.zero_(); st.lp_top.fill_(float("-inf")); st.lp_id.fill_(-1)
        restore()
        if st.graph is None:
            _capture(st, lambda: self.verify_step(cache, st), restore)
        torch.cuda.current_stream().synchronize()
        first_id = first.item()
        stop = first_id in eos_set
        _stream_put(streamer, first_id)
        got: List[int] = []
        trace = self.spec_trace
        with torch.cuda.stream(st.stream):
            while len(got) < need and not stop:
                # every replay appends at least one token: never more replays than tokens still wanted, at most 16 between two looks at the ids
                chunk = 1 if trace is not None else max(1, min(16, (need - len(got) + n - 1) // n))
                _replay(st, chunk)
                n_out = min(int(st.n_out.item()), need, st.max_out)  # (the sync)
                if trace is not None:
                    trace.append(int(st.n_accept.item()))
                    if self.spec_probe is not None:
                        self.spec_probe(st)
                new = st.out_ids[len(got):n_out].tolist()
                for t in new:
                    got.append(t)
                    _stream_put(streamer, t)
                    if t in eos_set:
                        stop = True
                        break
        st.stream.synchronize()
        out = torch.tensor(_cut_at_eos([first_id] + got, eos_set)[:max(max_new_tokens, 1)], dtype=torch.int64, device=dev)
        if streamer is not None:
            streamer.end()
        if logprobs is not None:                                    # (cut like `out`: record t - 1 of the session belongs to out[0, t])
            m = out.numel()
            return out[None], self._pack_logprobs([self._row_logprobs(st, 0, m - 1)], [m], m, logprobs, dev)
        return out[None]
