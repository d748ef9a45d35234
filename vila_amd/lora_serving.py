"""LoRA adapters served unmerged: the adapter bank of the batched decode step (kernels: vila_amd/csrc/lora_decode.hip).

`merge_adapter` serves ONE tuned model per process: it rewrites the base weights and drops every captured graph.  A bank keeps up to `capacity`
adapters beside the untouched base in device buffers whose addresses never change, and every row of a batched session names its slot in a device
array (`row_adapter`, -1 = the base model): ONE captured graph serves any mix of adapters, and loading or unloading one does not touch it.

Layout, per decoder layer and per stack of projections that share an input (vila_amd.lora._groups: q|k|v, o, gate|up, down), for every slot:
    A   [Rs, K]        the members' lora_A stacked, member j in rows j r .. j r + r_adapter - 1 (the trainer's A_<stack>, padded to the bank's rank r)
    B   [r / 8, N, 8]  lora_B of the members side by side over the stack's N output columns, chunk-major: (c, col, e) = B[col][8 c + e] — the
                       decode step's expand kernel reads one contiguous KB per wave and chunk
    Bt  [r, N]         the same matrices in the trainer's orientation, for the prefill under the adapter (lora_down / lora_up)
and one fp32 scale alpha / r_adapter per slot.  Rank padding and projections outside `target_modules` are zeros, which contribute exact zeros.
An empty slot holds zeros and scale 0."""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .lora import LORA_RANKS, PEFT_PREFIX, LoraAdapters, LoraConfig, _PARENT, _groups, read_adapter

MAX_SLOTS = 32              # LORA_MAX_SLOTS of vila_amd/csrc/kernels.h


def stack_shapes(lcfg, r: int) -> List[Tuple[str, int, int, int, List[Tuple[str, int, int]]]]:
    """[(stack, K, Rs, N, [(module, first column, columns)])] of a bank of rank r: every stack with ALL its members, targeted or not."""
    out = []
    for name, K, members in _groups(lcfg):
        cols, c0 = [], 0
        for m, width in members:
            cols.append((m, c0, width))
            c0 += width
        out.append((name, K, len(members) * r, c0, cols))
    return out


def pack_b(bt: torch.Tensor) -> torch.Tensor:
    """Bt [..., r, N] -> the expand kernel's chunk-major B [..., r / 8, N, 8]."""
    r, N = bt.shape[-2:]
    return bt.reshape(*bt.shape[:-2], r // 8, 8, N).transpose(-1, -2).contiguous()


def unpack_b(bp: torch.Tensor) -> torch.Tensor:
    """pack_b's inverse: [..., r / 8, N, 8] -> Bt [..., r, N]."""
    c, N, _ = bp.shape[-3:]
    return bp.transpose(-1, -2).reshape(*bp.shape[:-3], c * 8, N).contiguous()


def pack_adapter(lcfg, ad: LoraAdapters, r: int) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """One adapter in the bank's shapes: {stack: (A [layers, Rs, K], Bt [layers, r, N])} bf16 on the adapter's device, zero where the adapter has
    nothing (ranks r_adapter .. r - 1, projections outside its target_modules)."""
    ra = ad.cfg.r
    if ra > r:
        raise ValueError(f"the adapter's rank ({ra}) exceeds the bank's ({r})")
    L, dev = lcfg.num_hidden_layers, ad.params.device
    out = {}
    for stack, K, Rs, N, cols in stack_shapes(lcfg, r):
        A = torch.zeros((L, Rs, K), dtype=torch.bfloat16, device=dev)
        Bt = torch.zeros((L, r, N), dtype=torch.bfloat16, device=dev)
        for j, (m, c0, width) in enumerate(cols):
            if m not in ad.cfg.target_modules:
                continue
            for i in range(L):
                a, bt = ad.pair(i, m)
                A[i, j * r:j * r + ra].copy_(a)
                Bt[i, :ra, c0:c0 + width].copy_(bt)
        out[stack] = (A, Bt)
    return out


def unpack_adapter(lcfg, packed: Dict[str, Tuple[torch.Tensor, torch.Tensor]], cfg: LoraConfig, r: int) -> Dict[str, torch.Tensor]:
    """pack_adapter's inverse for an adapter of configuration cfg: the PEFT state dict (LoraAdapters.state_dict's keys and orientation)."""
    sd = {}
    for stack, K, Rs, N, cols in stack_shapes(lcfg, r):
        A, Bt = packed[stack]
        for j, (m, c0, width) in enumerate(cols):
            if m not in cfg.target_modules:
                continue
            for i in range(lcfg.num_hidden_layers):
                key = f"{PEFT_PREFIX}llm.model.layers.{i}.{_PARENT[m]}.{m}."
                sd[key + "lora_A.weight"] = A[i, j * r:j * r + cfg.r].detach().to("cpu").contiguous().clone()
                sd[key + "lora_B.weight"] = Bt[i, :cfg.r, c0:c0 + width].detach().to("cpu").t().contiguous().clone()
    return sd


def split_non_lora(non_lora: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The tuned-projector tensors of an adapter folder ({name without `mm_projector.`: tensor}); anything else tuned outside the adapters is refused:
    a bank serves adapters beside ONE base model, whose tower and LLM weights every request shares."""
    other = sorted(n for n in non_lora if not n.startswith("mm_projector."))
    if other:
        kind = "vision_tower" if other[0].startswith("vision_tower.") else ("llm" if other[0].startswith("llm.") else "unknown")
        raise ValueError(f"AdapterBank.load: the adapter folder tunes {len(other)} {kind} tensors outside the adapters (first '{other[0]}'); a bank "
                         "serves vision_tower.* and llm.* from the shared base model, so such an adapter can only be served merged (merge_adapter)")
    return {n[len("mm_projector."):]: t for n, t in non_lora.items()}


class AdapterBank:
    """Fixed device buffers for `capacity` adapters of rank <= r over the model's LLM.  `model`: a HipLlavaLlamaModel (its tuned-projector copies are
    made from model.mm_projector), or an LlmConfig for a bank without a model (`device` then says where; the CPU tests pack there)."""

    def __init__(self, model, capacity: int = 4, r: int = 64, device=None):
        if r not in LORA_RANKS:
            raise ValueError(f"AdapterBank: r = {r} is not supported; the rank-r kernels take r in {LORA_RANKS}")
        if not 1 <= int(capacity) <= MAX_SLOTS:
            raise ValueError(f"AdapterBank: 1..{MAX_SLOTS} slots (got {capacity})")
        self.model = model if hasattr(model, "llm") else None
        self.lcfg = model.cfg.llm if self.model is not None else model
        self.capacity, self.r = int(capacity), int(r)
        dev = torch.device(device if device is not None else (self.model.device if self.model is not None else "cpu"))
        self.device = dev
        L = self.lcfg.num_hidden_layers
        self.shapes = stack_shapes(self.lcfg, self.r)
        # [layers, capacity, ...]: a layer's slots are contiguous, slot stride Rs K / r N as the step assumes
        self.a = {s: torch.zeros((L, self.capacity, Rs, K), dtype=torch.bfloat16, device=dev) for s, K, Rs, N, _ in self.shapes}
        self.b = {s: torch.zeros((L, self.capacity, self.r // 8, N, 8), dtype=torch.bfloat16, device=dev) for s, K, Rs, N, _ in self.shapes}
        self.bt = {s: torch.zeros((L, self.capacity, self.r, N), dtype=torch.bfloat16, device=dev) for s, K, Rs, N, _ in self.shapes}
        self.scale = torch.zeros(self.capacity, dtype=torch.float32, device=dev)
        self.names: List[Optional[str]] = [None] * self.capacity
        self.configs: List[Optional[LoraConfig]] = [None] * self.capacity
        self.projectors: List[Optional[torch.nn.Module]] = [None] * self.capacity
        self.in_use = [0] * self.capacity                # live rows per slot (batch_admit / batch_release)
        self._c_layers = None
        self._c_prefill = {}

    # ---- slots --------------------------------------------------------------------------------------------------------------------------------------
    def slot_of(self, name: Optional[str]) -> int:
        """The slot of a loaded adapter; None -> -1 (the base model)."""
        if name is None:
            return -1
        if name not in self.names:
            raise KeyError(f"AdapterBank: no adapter named '{name}' is loaded (loaded: {[n for n in self.names if n is not None]})")
        return self.names.index(name)

    def __contains__(self, name) -> bool:
        return name is not None and name in self.names

    def bytes_per_slot(self) -> int:
        return sum(t[:, 0].numel() * t.element_size() for d in (self.a, self.b, self.bt) for t in d.values()) + 4

    def load(self, name: str, src) -> int:
        """Copy an adapter (a folder written by save_adapter, or a LoraAdapters) into a free slot -> the slot."""
        if not isinstance(name, str) or not name:
            raise ValueError("AdapterBank.load: the adapter needs a name")
        if name in self.names:
            raise ValueError(f"AdapterBank.load: an adapter named '{name}' is already loaded (slot {self.names.index(name)})")
        if None not in self.names:
            raise ValueError(f"AdapterBank.load: all {self.capacity} slots are taken ({self.names}); unload one first")
        proj_sd: Dict[str, torch.Tensor] = {}
        if isinstance(src, (str, os.PathLike)):
            cfg, sd, non_lora = read_adapter(str(src))
            proj_sd = split_non_lora(non_lora)
            ad = LoraAdapters(self.lcfg, cfg, device="cpu")
            ad.load_state_dict(sd)
        else:
            ad = src
        if (ad.lcfg.hidden_size, ad.lcfg.intermediate_size, ad.lcfg.q_size, ad.lcfg.kv_size, ad.lcfg.num_hidden_layers) != \
                (self.lcfg.hidden_size, self.lcfg.intermediate_size, self.lcfg.q_size, self.lcfg.kv_size, self.lcfg.num_hidden_layers):
            raise ValueError("AdapterBank.load: the adapter was made for an LLM of other widths or depth")
        packed = pack_adapter(self.lcfg, ad, self.r)
        projector = self._tuned_projector(proj_sd) if proj_sd else None
        slot = self.names.index(None)
        with torch.no_grad():
            for s, (A, Bt) in packed.items():
                self.a[s][:, slot].copy_(A)
                self.bt[s][:, slot].copy_(Bt)
                self.b[s][:, slot].copy_(pack_b(Bt))
            self.scale[slot:slot + 1].fill_(ad.cfg.scale)
        self.names[slot], self.configs[slot], self.projectors[slot] = name, ad.cfg, projector
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)          # loading is not hot: the copies have landed before any step may read the slot
        return slot

    def unload(self, name: str) -> None:
        """Free the adapter's slot (zeros, scale 0).  Refused while a live row of a session runs under it."""
        slot = self.slot_of(name)
        if self.in_use[slot] > 0:
            raise RuntimeError(f"AdapterBank.unload: {self.in_use[slot]} live rows run under '{name}' (slot {slot}); release them first")
        with torch.no_grad():
            for d in (self.a, self.b, self.bt):
                for t in d.values():
                    t[:, slot].zero_()
            self.scale[slot:slot + 1].zero_()
        self.names[slot], self.configs[slot], self.projectors[slot] = None, None, None
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def unpack(self, name: str) -> Dict[str, torch.Tensor]:
        """The PEFT state dict of a loaded adapter, read back from its slot."""
        slot = self.slot_of(name)
        packed = {s: (self.a[s][:, slot], unpack_b(self.b[s][:, slot])) for s, *_ in self.shapes}
        return unpack_adapter(self.lcfg, packed, self.configs[slot], self.r)

    def projector(self, name: Optional[str]):
        """The tuned projector kept with the adapter, or None: its requests encode their media through the base model's."""
        return None if name is None else self.projectors[self.slot_of(name)]

    def _tuned_projector(self, proj_sd: Dict[str, torch.Tensor]):
        if self.model is None:
            raise ValueError("AdapterBank.load: the adapter folder holds tuned-projector tensors, which need a bank made from a model")
        from .modules import HipMultimodalProjector, _get
        base = self.model.mm_projector
        proj = HipMultimodalProjector(self.model.cfg, base.device, base.dtype)
        with torch.no_grad():
            for (n, p), (n0, p0) in zip(proj.named_parameters(), base.named_parameters()):
                assert n == n0
                p.copy_(p0)
            for n, t in proj_sd.items():
                _get(proj, n).copy_(t)
        proj._invalidate()
        return proj

    # ---- what the C entries read --------------------------------------------------------------------------------------------------------------------
    def c_bank(self, row_adapter: torch.Tensor) -> "_lib.VilaLoraBank":
        """The step's descriptor over this bank and a session's row_adapter [n] int32."""
        if self._c_layers is None:
            arr = (_lib.VilaLoraBankLayer * self.lcfg.num_hidden_layers)()
            for i in range(self.lcfg.num_hidden_layers):
                for s, *_ in self.shapes:
                    setattr(arr[i], f"a_{s}", self.a[s][i].data_ptr())
                    setattr(arr[i], f"b_{s}", self.b[s][i].data_ptr())
            self._c_layers = arr
        return _lib.VilaLoraBank(self._c_layers, self.scale.data_ptr(), row_adapter.data_ptr(), self.capacity, self.r)

    def c_prefill(self, name: str):
        """(VilaLoraLayer array, r, scale) of a loaded adapter for vila_llm_prefill_lora."""
        slot = self.slot_of(name)
        arr = self._c_prefill.get(slot)
        if arr is None:
            arr = (_lib.VilaLoraLayer * self.lcfg.num_hidden_layers)()
            for i in range(self.lcfg.num_hidden_layers):
                for s, *_ in self.shapes:
                    setattr(arr[i], f"a_{s}", self.a[s][i, slot].data_ptr())
                    setattr(arr[i], f"bt_{s}", self.bt[s][i, slot].data_ptr())
            self._c_prefill[slot] = arr
        return arr, self.r, float(self.configs[slot].scale)
