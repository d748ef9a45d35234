"""LoRA fine-tuning of the LLM (reference llava/train/args.py:243-252, train.py:149-171, 648-706, 903-914; model/builder.py:63-128).

Every targeted linear of every decoder layer (q, k, v, o, gate, up, down; never lm_head: `find_all_linear_names`) gets a rank-r adapter
    y = x W^T + b + s (x A^T) B^T,      s = alpha / r,
the base weights stay frozen, the mm_projector stays fully trainable (the reference: "currently assume fft for mm projector").

Storage.  Per layer, A is stored as PEFT stores it ([r, in]) and B transposed (Bt [r, out]).  Projections that share an input stack their As:
A_qkv [3r, H] and A_gateup [2r, H], so one `lora_down` serves q, k and v.  All adapters, the tuned projector and (optionally) the tuned tower live
in ONE flat bf16 parameter buffer with a gradient buffer of the same layout and fp32 master / moments of the same length (`LoraFlat`, the
interface of `train.FlatParams`): one bucket per decoder layer, prefix `llm.model.layers.{i}.lora.`.  The frozen base has no gradient buffer
and no optimizer state.

Dataflow per target linear (the three skinny products are vila_amd/csrc/lora.hip; the base GEMMs are untouched):
    forward    t = lora_down(h, A)            once per stack
               u = lora_up(t_slice, Bt, s, res=<the linear's residual>)
               y = gemm(h, W, bias, residual=u)
    backward   dt = lora_down(dy_slice, Bt, s)      into the stack's [T, 3r] / [T, 2r] buffer
               dBt = lora_wgrad(t, dy, s);  dA = lora_wgrad(dt, h)
               dx = gemm_t(dy, W, b_cm=True, residual=lora_up(dt, A, 1, res=dx_residual))
The base weight-gradient GEMMs and their side stream are not run.  t and u are rounded to bf16 on the way (two roundings a merged-weight fp32
forward does not have)."""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch

LORA_RANKS = (16, 32, 48, 64)
LLM_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
_PARENT = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn",
           "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}
PEFT_PREFIX = "base_model.model."


@dataclass
class LoraConfig:
    r: int = 64
    alpha: float = 16.0
    target_modules: Tuple[str, ...] = LLM_TARGETS
    dropout: float = 0.0
    bias: str = "none"
    use_dora: bool = False
    lora_vt: bool = False
    seed: int = 0

    def __post_init__(self):
        if self.r not in LORA_RANKS:
            raise ValueError(f"LoraConfig: r = {self.r} is not supported; the rank-r kernels take r in {LORA_RANKS}")
        if float(self.dropout) != 0.0:
            raise ValueError(f"LoraConfig: dropout = {self.dropout} is not supported; the limit of this implementation is dropout = 0.0")
        if self.bias != "none":
            raise ValueError(f"LoraConfig: bias = {self.bias!r} is not supported; only bias = 'none'")
        if self.use_dora:
            raise ValueError("LoraConfig: DoRA (use_dora) is out of scope")
        if self.lora_vt:
            raise ValueError("LoraConfig: adapters on the vision tower (lora_vt) are out of scope; tune it in full with tune_vision_tower=True")
        unknown = set(self.target_modules) - set(LLM_TARGETS)
        if unknown:
            raise ValueError(f"LoraConfig: unknown target modules {sorted(unknown)}; the LLM's linears are {LLM_TARGETS} (lm_head is never adapted)")
        self.target_modules = tuple(m for m in LLM_TARGETS if m in set(self.target_modules))      # canonical order

    @property
    def scale(self) -> float:
        return float(self.alpha) / float(self.r)

    def to_peft(self) -> dict:
        """adapter_config.json with PEFT's field names."""
        return {"peft_type": "LORA", "task_type": "CAUSAL_LM", "base_model_name_or_path": None, "r": int(self.r), "lora_alpha": self.alpha,
                "lora_dropout": 0.0, "target_modules": sorted(self.target_modules), "bias": "none", "fan_in_fan_out": False,
                "inference_mode": True, "init_lora_weights": True, "modules_to_save": None, "use_dora": False, "use_rslora": False,
                "layers_to_transform": None, "layers_pattern": None, "rank_pattern": {}, "alpha_pattern": {}, "revision": None}

    @classmethod
    def from_peft(cls, d: dict) -> "LoraConfig":
        if d.get("peft_type", "LORA") != "LORA":
            raise ValueError(f"adapter_config.json: peft_type {d.get('peft_type')!r} is not LORA")
        if d.get("use_rslora") or d.get("rank_pattern") or d.get("alpha_pattern") or d.get("fan_in_fan_out"):
            raise ValueError("adapter_config.json: rslora, rank / alpha patterns and fan_in_fan_out are not supported")
        tm = d.get("target_modules") or LLM_TARGETS
        return cls(r=int(d["r"]), alpha=float(d["lora_alpha"]), target_modules=tuple(tm), dropout=float(d.get("lora_dropout", 0.0)),
                   bias=d.get("bias", "none"), use_dora=bool(d.get("use_dora", False)))


# ----------------------------------------------------------------------------------------------------------------------
# layout of one layer's adapters
# ----------------------------------------------------------------------------------------------------------------------
def _groups(lcfg) -> List[Tuple[str, int, List[Tuple[str, int]]]]:
    """(stack name, input width, [(module, output width)]): the projections of a decoder layer by the input they share."""
    H, I, q, kv = lcfg.hidden_size, lcfg.intermediate_size, lcfg.q_size, lcfg.kv_size
    return [("qkv", H, [("q_proj", q), ("k_proj", kv), ("v_proj", kv)]), ("o", q, [("o_proj", H)]),
            ("gateup", H, [("gate_proj", I), ("up_proj", I)]), ("down", I, [("down_proj", H)])]


def layer_layout(lcfg, cfg: LoraConfig):
    """-> [(stack, input width, [module, ...])] of the targeted projections, and the tensors of one layer [(name, shape)]: A_<stack> [n r, in]
    followed by Bt_<module without _proj> [r, out] of its members."""
    stacks, specs = [], []
    for name, in_dim, members in _groups(lcfg):
        ms = [(m, o) for m, o in members if m in cfg.target_modules]
        if not ms:
            continue
        stacks.append((name, in_dim, [m for m, _ in ms]))
        specs.append((f"A_{name}", (len(ms) * cfg.r, in_dim)))
        specs += [(f"Bt_{m[:-5]}", (cfg.r, o)) for m, o in ms]
    return stacks, specs


def layer_prefix(i: int) -> str:
    return f"llm.model.layers.{i}.lora."


def adapter_index(lcfg, cfg: LoraConfig, offset: int = 0) -> Tuple[Dict[str, Tuple[int, int, torch.Size]], int]:
    """name -> (offset, numel, shape) of every adapter tensor, layer by layer, each 16-byte aligned (the rule of FlatParams); -> (index, end)."""
    _, specs = layer_layout(lcfg, cfg)
    index, off = {}, offset
    for i in range(lcfg.num_hidden_layers):
        for n, shape in specs:
            k = shape[0] * shape[1]
            index[layer_prefix(i) + n] = (off, k, torch.Size(shape))
            off += (k + 7) // 8 * 8
    return index, off


class LoraAdapters:
    """The adapters of every decoder layer in one flat bf16 buffer (its own, or a slice of a trainer's)."""

    def __init__(self, lcfg, cfg: LoraConfig, device="cpu", buffer: Optional[torch.Tensor] = None):
        self.lcfg, self.cfg = lcfg, cfg
        self.index, self.numel = adapter_index(lcfg, cfg)
        self.stacks, _ = layer_layout(lcfg, cfg)
        if buffer is None:
            buffer = torch.zeros(self.numel, device=device, dtype=torch.bfloat16)
        assert buffer.numel() == self.numel and buffer.dtype == torch.bfloat16
        self.params = buffer

    def tensor(self, layer: int, name: str) -> torch.Tensor:
        o, k, shape = self.index[layer_prefix(layer) + name]
        return self.params[o:o + k].view(shape)

    def init_(self, seed: Optional[int] = None) -> "LoraAdapters":
        """PEFT's initialisation: A = kaiming_uniform_(a = sqrt(5)), i.e. U(-1 / sqrt(in), 1 / sqrt(in)) per projection, B = 0; from a seeded
        CPU generator, projection by projection in layer order, so the draw does not depend on the device or on the stacking."""
        g = torch.Generator(device="cpu").manual_seed(self.cfg.seed if seed is None else seed)
        r = self.cfg.r
        with torch.no_grad():
            self.params.zero_()
            for i in range(self.lcfg.num_hidden_layers):
                for stack, in_dim, members in self.stacks:
                    a = self.tensor(i, f"A_{stack}")
                    bound = 1.0 / math.sqrt(in_dim)
                    for j in range(len(members)):
                        a[j * r:(j + 1) * r].copy_((torch.rand((r, in_dim), generator=g) * 2.0 - 1.0) * bound)
        return self

    def pair(self, layer: int, module: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """(A [r, in], Bt [r, out]) of one projection: its rows of the stack, and its Bt."""
        r = self.cfg.r
        for stack, _, members in self.stacks:
            if module in members:
                j = members.index(module)
                return self.tensor(layer, f"A_{stack}")[j * r:(j + 1) * r], self.tensor(layer, f"Bt_{module[:-5]}")
        raise KeyError(f"{module} is not a target module of this adapter ({self.cfg.target_modules})")

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """PEFT's keys and orientation: ...{module}.lora_A.weight [r, in], ...lora_B.weight [out, r] (un-stacked, B transposed back)."""
        sd = {}
        for i in range(self.lcfg.num_hidden_layers):
            for m in self.cfg.target_modules:
                a, bt = self.pair(i, m)
                key = f"{PEFT_PREFIX}llm.model.layers.{i}.{_PARENT[m]}.{m}."
                sd[key + "lora_A.weight"] = a.detach().to("cpu").contiguous().clone()
                sd[key + "lora_B.weight"] = bt.detach().to("cpu").t().contiguous().clone()
        return sd

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        """Inverse of state_dict: stack the As, transpose the Bs.  Every key of this layout must be present with its shape; nothing else may be."""
        want = {}
        for i in range(self.lcfg.num_hidden_layers):
            for m in self.cfg.target_modules:
                a, bt = self.pair(i, m)
                key = f"{PEFT_PREFIX}llm.model.layers.{i}.{_PARENT[m]}.{m}."
                want[key + "lora_A.weight"] = (a, tuple(a.shape), False)
                want[key + "lora_B.weight"] = (bt, (bt.shape[1], bt.shape[0]), True)
        missing, extra = [k for k in want if k not in sd], [k for k in sd if k not in want]
        if missing or extra:
            raise KeyError(f"adapter state: {len(missing)} keys missing (first {missing[:3]}), {len(extra)} unexpected (first {extra[:3]})")
        bad = [k for k, (_, shape, _) in want.items() if tuple(sd[k].shape) != shape]
        if bad:
            raise ValueError(f"adapter state: '{bad[0]}' has shape {tuple(sd[bad[0]].shape)}, expected {want[bad[0]][1]} ({len(bad)} mismatching)")
        with torch.no_grad():
            for k, (dst, _, transposed) in want.items():
                dst.copy_(sd[k].t() if transposed else sd[k])


def merge_weight(w: torch.Tensor, a: torch.Tensor, bt: torch.Tensor, scale: float) -> torch.Tensor:
    """bf16(W + s B A), computed in fp32 on W's device with ONE rounding (W [out, in], A [r, in], Bt [r, out])."""
    return (w.float() + float(scale) * (bt.float().t() @ a.float())).to(w.dtype)


# ----------------------------------------------------------------------------------------------------------------------
# files: adapter_config.json, adapter_model.safetensors, non_lora_trainables.bin (reference train.py:903-914)
# ----------------------------------------------------------------------------------------------------------------------
def _write_adapter(folder: str, cfg: LoraConfig, sd: Dict[str, torch.Tensor], non_lora: Dict[str, torch.Tensor]) -> None:
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "adapter_config.json"), "w") as fh:
        json.dump(cfg.to_peft(), fh, indent=2, sort_keys=True)
    save_file(sd, os.path.join(folder, "adapter_model.safetensors"), metadata={"format": "pt"})
    torch.save({PEFT_PREFIX + n: t.detach().to("cpu").contiguous().clone() for n, t in non_lora.items()}, os.path.join(folder, "non_lora_trainables.bin"))


def read_adapter(folder: str):
    """-> (LoraConfig, PEFT state dict, {parameter name: tensor} of non_lora_trainables.bin without the `base_model.model.` prefix)."""
    from safetensors import safe_open
    cfg = LoraConfig.from_peft(json.load(open(os.path.join(folder, "adapter_config.json"))))
    sd = {}
    with safe_open(os.path.join(folder, "adapter_model.safetensors"), framework="pt", device="cpu") as fh:
        for k in fh.keys():
            sd[k] = fh.get_tensor(k)
    path = os.path.join(folder, "non_lora_trainables.bin")
    raw = torch.load(path, map_location="cpu", weights_only=True) if os.path.exists(path) else {}
    non_lora = {(k[len(PEFT_PREFIX):] if k.startswith(PEFT_PREFIX) else k): v for k, v in raw.items()}
    return cfg, sd, non_lora


def save_adapter(src, folder: str, non_lora: Optional[Dict[str, torch.Tensor]] = None) -> None:
    """`src`: a LoRATrainer (its adapters and its tuned projector / tower) or a LoraAdapters (+ `non_lora`: parameter name -> tensor)."""
    if isinstance(src, LoraAdapters):
        _write_adapter(folder, src.cfg, src.state_dict(), dict(non_lora or {}))
        return
    src.sync()
    _write_adapter(folder, src.lora, src.adapters.state_dict(), src.non_lora_trainables())


def load_adapter(target, folder: str) -> LoraAdapters:
    """Read an adapter folder into `target`: a LoRATrainer (adapters, tuned projector / tower and their fp32 masters), a LoraAdapters of the same
    layout, or a model (-> a new LoraAdapters on its device, for merge_adapter; its non_lora_trainables are copied into the model)."""
    cfg, sd, non_lora = read_adapter(folder)
    if isinstance(target, LoraAdapters):
        _same_config(target.cfg, cfg)
        target.load_state_dict(sd)
        return target
    if hasattr(target, "adapters") and hasattr(target, "non_lora_trainables"):      # a LoRATrainer
        _same_config(target.lora, cfg)
        target.sync()
        target.adapters.load_state_dict(sd)
        want = target.non_lora_trainables()
        if set(want) != set(non_lora):
            raise KeyError(f"non_lora_trainables.bin holds {len(non_lora)} tensors, the trainer tunes {len(want)} outside the adapters")
        with torch.no_grad():
            for n, t in want.items():
                t.copy_(non_lora[n])
        target.flat.sync_master_from_params()
        return target.adapters
    model = target
    ad = LoraAdapters(model.cfg.llm, cfg, device=model.device)
    ad.load_state_dict(sd)
    _load_non_lora(model, non_lora)
    return ad


def _same_config(a: LoraConfig, b: LoraConfig) -> None:
    if (a.r, float(a.alpha), a.target_modules) != (b.r, float(b.alpha), b.target_modules):
        raise ValueError(f"the adapter on disk (r {b.r}, alpha {b.alpha}, {b.target_modules}) does not match this one (r {a.r}, alpha {a.alpha}, {a.target_modules})")


def _load_non_lora(model, non_lora: Dict[str, torch.Tensor]) -> None:
    from .modules import _get
    mods = {"mm_projector.": model.mm_projector, "vision_tower.": model.vision_tower, "llm.": model.llm}
    with torch.no_grad():
        for n, t in non_lora.items():
            prefix = next((p for p in mods if n.startswith(p)), None)
            if prefix is None:
                raise KeyError(f"non_lora_trainables.bin: '{n}' belongs to no component of the model")
            _get(mods[prefix], n[len(prefix):]).copy_(t)
    for p in {p for n in non_lora for p in mods if n.startswith(p)}:
        mods[p]._invalidate()


def merge_adapter(model, src) -> None:
    """W += s B A for every adapted projection, once, in fp32 on the device with one rounding to bf16; `src` is an adapter folder or a
    LoraAdapters.  The weights are rewritten in place (q|k|v stay one fused buffer; a model somebody un-fused is re-fused), then every weight
    struct and captured graph is dropped (`_invalidate`).  Afterwards prefill, decode, batched decode and quantize_w4 serve the tuned model."""
    from .modules import _get
    llm = model.llm
    if getattr(llm, "_bf16_released", False):
        raise RuntimeError("merge_adapter: the bf16 projection weights were freed by quantize_w4(release_bf16=True); merge before quantising")
    if getattr(llm, "_w4", None) is not None:
        raise RuntimeError("merge_adapter: the model already holds int4 copies of its projections; merge first, then quantize_w4")
    ad = load_adapter(model, src) if isinstance(src, (str, os.PathLike)) else src
    if not llm._qkv_fused():
        llm.refuse()
    with torch.no_grad():
        for i in range(ad.lcfg.num_hidden_layers):
            for m in ad.cfg.target_modules:
                w = _get(llm, f"model.layers.{i}.{_PARENT[m]}.{m}.weight")
                a, bt = ad.pair(i, m)
                w.data.copy_(merge_weight(w.data, a.to(w.device), bt.to(w.device), ad.cfg.scale))
    llm._invalidate()


# ----------------------------------------------------------------------------------------------------------------------
# flat storage of the trainable elements and the trainer
# ----------------------------------------------------------------------------------------------------------------------
def _trainer_classes():
    from . import ops
    from .modules import _get
    from .train import FlatParams, SFTTrainer, _cm_ok

    class LoraFlat(FlatParams):
        """`FlatParams` over the TRAINABLE elements only: the adapters (one bucket per decoder layer), then the tuned projector, then the tuned
        tower, in the order the frozen base keeps them (q/k/v adjacent).  `param` falls back to the base for every frozen tensor; `grad` of a
        frozen 1-D tensor (the decoder's norms, whose dw the backward kernel writes anyway) is a scratch row that nobody reads."""

        def __init__(self, model, base: FlatParams, cfg: LoraConfig, tuned: Tuple[str, ...], with_optimizer_state: bool = True):
            self.model, self.base = model, base
            dev = model.device
            self.index, off = adapter_index(model.cfg.llm, cfg)
            n_adapter = off
            moved = [n for n in base.index if n.startswith(tuned)] if tuned else []
            for n in moved:
                _, k, shape = base.index[n]
                self.index[n] = (off, k, shape)
                off += (k + 7) // 8 * 8
            self.numel = off
            self.params = torch.zeros(off, device=dev, dtype=torch.bfloat16)
            self.grads = torch.zeros(off, device=dev, dtype=torch.bfloat16)
            self.adapters = LoraAdapters(model.cfg.llm, cfg, buffer=self.params[:n_adapter]).init_()
            mods = {"vision_tower.": model.vision_tower, "mm_projector.": model.mm_projector}
            with torch.no_grad():
                for n in moved:                       # the tuned modules' parameters become views of THIS buffer
                    view = self.param(n)
                    view.copy_(base.param(n))
                    prefix = next(p for p in mods if n.startswith(p))
                    _get(mods[prefix], n[len(prefix):]).data = view
            for p, mod in mods.items():
                if p in tuned:
                    mod._invalidate()
            widest = max([k for _, k, shape in base.index.values() if len(shape) == 1] + [8])
            self._scratch = torch.zeros(widest, device=dev, dtype=torch.bfloat16)
            self.master = self.m = self.v = None
            if with_optimizer_state:
                self.master = self.params.float()
                self.m = torch.zeros_like(self.master)
                self.v = torch.zeros_like(self.master)
            self.step_count = 0
            self.bucket_steps = {}

        def has(self, prefix: str) -> bool:
            return any(n.startswith(prefix) for n in self.index)

        def param(self, name: str) -> torch.Tensor:
            if name in self.index:
                return FlatParams.param(self, name)
            return self.base.param(name)

        def grad(self, name: str) -> torch.Tensor:
            if name in self.index:
                return FlatParams.grad(self, name)
            _, k, shape = self.base.index[name]
            if len(shape) != 1:
                raise KeyError(f"'{name}' is frozen under LoRA: it has no gradient")
            return self._scratch[:k]

    class LoRATrainer(SFTTrainer):
        """SFTTrainer with the LLM frozen under rank-r adapters: the media planning, the tower and projector forward / backward, the loss,
        `step`, `step_accumulated`, `max_grad_norm` and `optimizer_step` are the parent's; the decoder's forward and backward are replaced."""

        def __init__(self, model, lora_config: Optional[LoraConfig] = None, tune_mm_projector: bool = True, tune_vision_tower: bool = False,
                     lr: float = 2e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, max_grad_norm: Optional[float] = None,
                     optimizer_state: bool = True, group=None, decay_groups: bool = True):
            if tune_vision_tower and not tune_mm_projector:
                raise ValueError("LoRATrainer: tune_vision_tower=True needs tune_mm_projector=True (the tower's gradient passes through the projector's backward)")
            self.lora = lora_config or LoraConfig()
            self._tuned = tuple(p for p, on in (("mm_projector.", tune_mm_projector), ("vision_tower.", tune_vision_tower)) if on)
            super().__init__(model, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                             optimizer_state=optimizer_state, group=group, decay_groups=decay_groups)
            self.skip_vit_bwd = not tune_vision_tower
            self.skip_proj_bwd = not tune_mm_projector
            self.adapters = self.flat.adapters
            self.stacks = {name: members for name, _, members in self.adapters.stacks}

        def _make_flat(self, model, optimizer_state: bool):
            self.base = FlatParams(model, with_optimizer_state=False, with_grads=False)
            return LoraFlat(model, self.base, self.lora, self._tuned, with_optimizer_state=optimizer_state)

        # ---- bookkeeping ----
        def state_numel(self) -> int:
            """Elements that carry a gradient and fp32 master / moments: the adapters, the tuned projector, the tuned tower (padded to 8 each)."""
            return int(self.flat.numel)

        def sync(self) -> None:
            """Wait for the optimizer and wgrad streams: the parameter buffer is final (before it is read or overwritten from the host)."""
            for st in (self.opt, self.side):
                if st is not None:
                    torch.cuda.current_stream().wait_stream(st)

        def non_lora_trainables(self) -> Dict[str, torch.Tensor]:
            return {n: self.flat.param(n) for n in self.flat.index if ".lora." not in n}

        def _ready(self, prefix: str) -> None:
            if self.flat.has(prefix):                 # the frozen base's buckets (lm_head, final norm, embedding) are never announced
                super()._ready(prefix)

        def _fused(self, prefix: str, kind: str) -> torch.Tensor:
            f = self.flat if (prefix + "q_proj." + kind) in self.flat.index else self.base
            o, k, shape = f.index[prefix + "q_proj." + kind]
            o2, k2, _ = f.index[prefix + "v_proj." + kind]
            t = f.params[o:o2 + k2]
            return t.view((o2 + k2 - o) // shape[1], shape[1]) if len(shape) == 2 else t

        def forward_backward_c(self, *a, **k):
            raise NotImplementedError("the one-call C-ABI driver (VILA_SFT_C_ABI=1, forward_backward_c) does not run with adapters attached; "
                                      "unset VILA_SFT_C_ABI to use the Python-orchestrated driver")

        def _head_bwd(self, hv, head, dlog, head_name):
            return self._dgrad(dlog, head, None)      # the head is frozen: d(hidden) only

        def _embed_bwd(self, dx0, p, txt_dst, nl_src, nl_dst, n_nl) -> None:
            return None                               # the embedding is frozen

        def _dgrad(self, dy: torch.Tensor, w: torch.Tensor, residual: Optional[torch.Tensor]) -> torch.Tensor:
            """dX = dY W (+ residual), W read as it lies where the contraction-major kernels take the shape (train.linear_bwd's two routes)."""
            if _cm_ok(dy.shape[0], dy.shape[1], w.shape[1]):
                return ops.gemm_t(dy, w, b_cm=True, residual=residual, ws=self.ws)
            return ops.gemm(dy, ops.transpose(w), residual=residual)

        # ---- one adapted linear ----
        def _cols(self, stack: str, module: str) -> slice:
            j, r = self.stacks[stack].index(module), self.lora.r
            return slice(j * r, (j + 1) * r)

        def _lin_fwd(self, i: int, stack: str, h: torch.Tensor, t: Optional[torch.Tensor], module: str, w, bias=None, residual=None, ws=None):
            """y = h W^T + bias + residual + s (h A^T) Bt of one projection; t = the stack's lora_down, or None when the module is no target."""
            if t is not None and module in self.stacks[stack]:
                residual = ops.lora_up(t[:, self._cols(stack, module)], self.adapters.tensor(i, f"Bt_{module[:-5]}"), self.lora.scale, res=residual)
            return ops.gemm(h, w, bias=bias, residual=residual, ws=ws)

        def _lin_bwd(self, i: int, stack: str, module: str, t: torch.Tensor, dt: torch.Tensor, dy: torch.Tensor) -> None:
            """dt[:, module's columns] = s dy Bt^T and dBt = s t^T dy of one target projection (dA and dx follow per stack)."""
            G = self.flat.grad
            bt = self.adapters.tensor(i, f"Bt_{module[:-5]}")
            cols = self._cols(stack, module)
            ops.lora_down(dy, bt, self.lora.scale, out=dt[:, cols])
            ops.lora_wgrad(t[:, cols], dy, G(layer_prefix(i) + f"Bt_{module[:-5]}"), self.lora.scale)

        def _stack_bwd(self, i: int, stack: str, dt: torch.Tensor, h: torch.Tensor, dx_residual: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
            """dA = dt^T h of the stack; -> dx_lora = dt A (+ dx_residual), the residual of the base dgrad."""
            ops.lora_wgrad(dt, h, self.flat.grad(layer_prefix(i) + f"A_{stack}"))
            return ops.lora_up(dt, self.adapters.tensor(i, f"A_{stack}"), 1.0, res=dx_residual)

        def _t(self, i: int, stack: str, h: torch.Tensor) -> Optional[torch.Tensor]:
            return ops.lora_down(h, self.adapters.tensor(i, f"A_{stack}")) if stack in self.stacks else None

        # ---- the decoder ----
        def _llm_fwd(self, x: torch.Tensor, pos: torch.Tensor, cu: torch.Tensor, max_seqlen: int):
            c = self.cfg.llm
            P = self.flat.param
            T = x.shape[0]
            nq, nkv, hd = c.num_attention_heads, c.num_key_value_heads, c.head_dim
            cs, sn = ops.rope_table(pos, hd, c.rope_theta)
            saved = SimpleNamespace(layers=[], cs=cs, sn=sn, cu=cu, max_seqlen=max_seqlen)
            widths = {"q_proj": c.q_size, "k_proj": c.kv_size, "v_proj": c.kv_size}
            for i in range(c.num_hidden_layers):
                l = f"llm.model.layers.{i}."
                s = SimpleNamespace(x_in=x)
                s.h1 = ops.rmsnorm(x, P(l + "input_layernorm.weight"), c.rms_norm_eps)
                s.t_qkv = self._t(i, "qkv", s.h1)
                u = None
                if s.t_qkv is not None:               # the three contributions fill the column slices of ONE buffer, the fused GEMM's residual
                    members = self.stacks["qkv"]
                    u = (torch.empty if len(members) == 3 else torch.zeros)((T, (nq + 2 * nkv) * hd), device=x.device, dtype=torch.bfloat16)
                    c0 = 0
                    for m in ("q_proj", "k_proj", "v_proj"):
                        if m in members:
                            ops.lora_up(s.t_qkv[:, self._cols("qkv", m)], self.adapters.tensor(i, f"Bt_{m[:-5]}"), self.lora.scale, out=u[:, c0:c0 + widths[m]])
                        c0 += widths[m]
                s.qkv = ops.gemm(s.h1, self._fused(l + "self_attn.", "weight"), bias=self._fused(l + "self_attn.", "bias"), residual=u)
                ops.rope_fwd_(s.qkv, cs, sn, pos, nq, nkv, hd)
                q3 = s.qkv.view(T, nq + 2 * nkv, hd)
                s.a, s.lse = ops.attn_fwd(q3[:, :nq], q3[:, nq:nq + nkv], q3[:, nq + nkv:], True, cu_seqlens=cu, max_seqlen=max_seqlen, return_lse=True)
                a2 = s.a.view(T, nq * hd)
                s.t_o = self._t(i, "o", a2)
                s.x_mid = self._lin_fwd(i, "o", a2, s.t_o, "o_proj", P(l + "self_attn.o_proj.weight"), residual=x)
                s.h2 = ops.rmsnorm(s.x_mid, P(l + "post_attention_layernorm.weight"), c.rms_norm_eps)
                s.t_gu = self._t(i, "gateup", s.h2)
                s.g = self._lin_fwd(i, "gateup", s.h2, s.t_gu, "gate_proj", P(l + "mlp.gate_proj.weight"))
                s.u = self._lin_fwd(i, "gateup", s.h2, s.t_gu, "up_proj", P(l + "mlp.up_proj.weight"))
                s.act = ops.silu_mul(s.g, s.u)
                s.t_d = self._t(i, "down", s.act)
                x = self._lin_fwd(i, "down", s.act, s.t_d, "down_proj", P(l + "mlp.down_proj.weight"), residual=s.x_mid, ws=self.ws)
                saved.layers.append(s)
            saved.x_out = x
            saved.hn = ops.rmsnorm(x, P("llm.model.norm.weight"), c.rms_norm_eps)
            return saved

        def _group_bwd(self, i: int, stack: str, t, h: torch.Tensor, parts, dx_residual=None) -> torch.Tensor:
            """Backward of the projections that share the input h.  parts: [(module, W, dy)] in the stack's order -> dh (+ dx_residual)."""
            res = dx_residual
            if t is not None:
                members = self.stacks[stack]
                dt = torch.empty((h.shape[0], len(members) * self.lora.r), device=h.device, dtype=torch.bfloat16)   # every member is in `parts`
                for m, _, dy in parts:
                    if m in members:
                        self._lin_bwd(i, stack, m, t, dt, dy)
                res = self._stack_bwd(i, stack, dt, h, res)
            for _, w, dy in parts:
                res = self._dgrad(dy, w, res)
            return res

        def _llm_bwd(self, dx: torch.Tensor, saved) -> torch.Tensor:
            c = self.cfg.llm
            P, G = self.flat.param, self.flat.grad
            T = dx.shape[0]
            nq, nkv, hd = c.num_attention_heads, c.num_key_value_heads, c.head_dim
            q, kv = c.q_size, c.kv_size
            for i in reversed(range(c.num_hidden_layers)):
                l = f"llm.model.layers.{i}."
                s = saved.layers[i]
                dact = self._group_bwd(i, "down", s.t_d, s.act, [("down_proj", P(l + "mlp.down_proj.weight"), dx)])
                dg, du = ops.silu_mul_bwd(s.g, s.u, dact)
                dh2 = self._group_bwd(i, "gateup", s.t_gu, s.h2, [("gate_proj", P(l + "mlp.gate_proj.weight"), dg), ("up_proj", P(l + "mlp.up_proj.weight"), du)])
                dxm = ops.norm_bwd(s.x_mid, P(l + "post_attention_layernorm.weight"), dh2, G(l + "post_attention_layernorm.weight"), None, c.rms_norm_eps, True)
                dx_mid = ops.add(dx, dxm)
                da = self._group_bwd(i, "o", s.t_o, s.a.view(T, nq * hd), [("o_proj", P(l + "self_attn.o_proj.weight"), dx_mid)])
                dqkv = torch.empty_like(s.qkv)
                q3, d3 = s.qkv.view(T, nq + 2 * nkv, hd), dqkv.view(T, nq + 2 * nkv, hd)
                ops.attn_bwd(q3[:, :nq], q3[:, nq:nq + nkv], q3[:, nq + nkv:], s.a, da.view(T, nq, hd), s.lse, True,
                             d3[:, :nq], d3[:, nq:nq + nkv], d3[:, nq + nkv:], cu_seqlens=saved.cu, max_seqlen=saved.max_seqlen)
                ops.rope_bwd_(dqkv, saved.cs, saved.sn, nq, nkv, hd)
                res = None
                if s.t_qkv is not None:
                    members = self.stacks["qkv"]
                    dt = torch.empty((T, len(members) * self.lora.r), device=dx.device, dtype=torch.bfloat16)
                    for m, c0, c1 in (("q_proj", 0, q), ("k_proj", q, q + kv), ("v_proj", q + kv, q + 2 * kv)):
                        if m in members:
                            self._lin_bwd(i, "qkv", m, s.t_qkv, dt, dqkv[:, c0:c1])
                    res = self._stack_bwd(i, "qkv", dt, s.h1, None)
                dh1 = self._dgrad(dqkv, self._fused(l + "self_attn.", "weight"), res)      # ONE base dgrad over the fused q|k|v weight
                dxi = ops.norm_bwd(s.x_in, P(l + "input_layernorm.weight"), dh1, G(l + "input_layernorm.weight"), None, c.rms_norm_eps, True)
                dx = ops.add(dx_mid, dxi)
                self._ready(layer_prefix(i))
            return dx

    return LoraFlat, LoRATrainer


def __getattr__(name: str):
    # LoraFlat / LoRATrainer subclass train.py's classes, which import the HIP library's wrappers: built on first use, so that the configuration,
    # the adapter files and the merge arithmetic import without them
    if name in ("LoraFlat", "LoRATrainer"):
        LoraFlat, LoRATrainer = _trainer_classes()
        globals().update(LoraFlat=LoraFlat, LoRATrainer=LoRATrainer)
        return globals()[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# ----------------------------------------------------------------------------------------------------------------------
# resume: save_fn / load_fn / final_save_fn of run.train
# ----------------------------------------------------------------------------------------------------------------------
def save_checkpoint(trainer, folder: str) -> None:
    from . import checkpoint
    save_adapter(trainer, folder)
    checkpoint.save_optimizer(trainer, folder)


def load_checkpoint(trainer, folder: str) -> None:
    from . import checkpoint
    load_adapter(trainer, folder)
    checkpoint.load_optimizer(trainer, folder)            # also re-derives the bf16 parameters from the restored masters


def save_final(trainer, folder: str) -> None:
    """The adapter folder of a finished run, plus the base model's config.json (the mark run.train reads as `finished`)."""
    from dataclasses import asdict
    save_adapter(trainer, folder)
    with open(os.path.join(folder, "config.json"), "w") as fh:
        json.dump({"lora": trainer.lora.to_peft(), "model": asdict(trainer.cfg)}, fh, indent=1, default=str)
