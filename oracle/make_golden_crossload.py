"""REFERENCE-EXECUTED fixture for the checkpoint cross-load tests (tests/test_checkpoint_crossload_cpu.py) — TEST INFRASTRUCTURE.

Both directions of the three-folder checkpoint boundary (llava/model/llava_arch.py:157-220), executed once through the reference's own code
and recorded, so that the tests run without the reference tree:
  ours_in_reference   a checkpoint written by `vila_amd.checkpoint.save_pretrained` (tiny configs, `rand_model` seed 5) loaded into the
                      reference's `SiglipVisionModel` (state_dict and from_pretrained) and `MultimodalProjector`: every parameter name and shape
                      those classes have, what their loaders reported missing / unexpected, and the CRC32 of every tensor as it arrived
  reference_writer    the reference's own `LlavaMetaModel.save_pretrained` (ast-extracted, executed unchanged) over HF `Qwen2ForCausalLM`, the
                      reference tower + `SiglipImageProcessor` and projector holding `synthetic.make_weights(cfg, 21)` in bf16: every JSON file it
                      wrote verbatim (the checkpoint directory replaced by `{CKPT}`), and per safetensors file its metadata and, per tensor, its
                      name, the `make_weights` key it holds, dtype, shape and CRC32 (the randomly initialised `vision_model.head.*`, which VILA never
                      uses, without a source) — the tests rebuild the checkpoint from that
  config_loader       the reference's `LlavaConfig.from_pretrained` + `prepare_config_for_eval` + `get_model_config` (llava/model/builder.py,
                      llava/model/utils/utils.py, extracted and executed unchanged) over a `save_pretrained` checkpoint (seed 7)

    python oracle/make_golden_crossload.py       # seconds; writes tests/golden/checkpoint_crossload_ref.json; needs the reference tree
"""
from __future__ import annotations

import ast
import json
import os
import os.path as osp
import sys
import tempfile
import textwrap
import zlib
from collections import OrderedDict
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as G  # noqa: E402
from vila_amd import checkpoint, configs, synthetic  # noqa: E402
from vila_amd.vlm import HipLlavaLlamaModel  # noqa: E402

REF = G.REF
OUT = os.path.join(ROOT, "tests", "golden", "checkpoint_crossload_ref.json")
CASES = (("mlp_downsample", False), ("mlp_downsample_3x3_fix", True))
CKPT = "{CKPT}"
PREFIX = {"llm": "llm.", "vision_tower": "vision_tower.vision_tower.", "mm_projector": "mm_projector."}


def crc(t: torch.Tensor) -> int:
    return zlib.crc32(t.detach().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())


def rand_model(cfg, seed):
    """Every parameter drawn from one seeded CPU generator, in parameter order.  tests/test_checkpoint_crossload_cpu.py imports this (and `crc`):
    the fixture's `ours_in_reference` and `config_loader` records hold for exactly these models."""
    m = HipLlavaLlamaModel(cfg, device="cpu")
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g).to(p.dtype))
    return m


def ours_in_reference(proj, tied, d):
    cfg = configs.tiny(proj, tied=tied)
    checkpoint.save_pretrained(rand_model(cfg, 5), d, max_shard_bytes=1 << 20)
    rec = {}
    ms = G.ref_siglip()
    vcfg = json.load(open(os.path.join(d, "vision_tower", "config.json")))
    sig_cfg = ms.SiglipVisionConfig(**{k: v for k, v in vcfg.items() if k != "model_type"})
    rec["tower_config"] = {k: getattr(sig_cfg, k) for k in vcfg if k != "model_type"}
    tower = ms.SiglipVisionModel(sig_cfg)
    missing, unexpected = tower.load_state_dict(dict(checkpoint._folder_tensors(os.path.join(d, "vision_tower"))), strict=False)
    rec["tower_params"] = {k: list(t.shape) for k, t in tower.state_dict().items()}
    rec["tower_load_state_dict"] = {"missing": sorted(missing), "unexpected": sorted(unexpected)}
    rec["tower_crc"] = {k: crc(t.to(torch.bfloat16)) for k, t in tower.state_dict().items() if k not in missing}
    tower2, info = ms.SiglipVisionModel.from_pretrained(os.path.join(d, "vision_tower"), torch_dtype=torch.bfloat16, output_loading_info=True)
    rec["tower_from_pretrained"] = {k: sorted(str(x) for x in info[k]) for k in ("missing_keys", "unexpected_keys", "mismatched_keys")}
    rec["tower_from_pretrained_crc"] = {k: crc(t) for k, t in tower2.state_dict().items()}
    bp = G.ref_projector()
    pcfg = json.load(open(os.path.join(d, "mm_projector", "config.json")))
    top = json.load(open(os.path.join(d, "config.json")))
    projector = bp.MultimodalProjector(bp.MultimodalProjectorConfig(pcfg["mm_projector_type"]),
                                       SimpleNamespace(mm_hidden_size=top["mm_hidden_size"], hidden_size=top["hidden_size"]))
    projector.load_state_dict(dict(checkpoint._folder_tensors(os.path.join(d, "mm_projector"))), strict=True)
    rec["projector_type"] = projector.config.mm_projector_type if hasattr(projector, "config") else pcfg["mm_projector_type"]
    rec["projector_params"] = {k: list(t.shape) for k, t in projector.state_dict().items()}
    rec["projector_crc"] = {k: crc(t.to(torch.bfloat16)) for k, t in projector.state_dict().items()}
    return rec


def reference_save_pretrained():
    """`LlavaMetaModel.save_pretrained` / get_llm / get_vision_tower / get_mm_projector (llava/model/llava_arch.py:157-220), taken from the file
    with ast and executed unchanged inside a class of the same name (`import llava.model` itself needs deepspeed)."""
    src = open(f"{REF}/llava/model/llava_arch.py").read()
    want = ["save_pretrained", "get_llm", "get_vision_tower", "get_mm_projector"]
    body = []
    for node in ast.parse(src).body:
        if isinstance(node, ast.ClassDef) and node.name == "LlavaMetaModel":
            got = {fn.name: ast.get_source_segment(src, fn) for fn in node.body if isinstance(fn, ast.FunctionDef)}
            body = [textwrap.indent(textwrap.dedent(got[n]), "    ") for n in want]
    ns = {"os": os, "osp": osp, "OrderedDict": OrderedDict, "torch": torch}
    exec(compile("class LlavaMetaModel(torch.nn.Module):\n" + "\n\n".join(body) + "\n", "llava_arch.py", "exec"), ns)
    return ns["LlavaMetaModel"]


def reference_writer(proj, tied, d):
    from safetensors import safe_open
    from transformers import SiglipImageProcessor
    cfg = configs.tiny(proj, tied=tied)
    w = {k: v.to(torch.bfloat16) for k, v in synthetic.make_weights(cfg, 21).items()}
    ms, bp = G.ref_siglip(), G.ref_projector()
    lc = G.load_by_path("ref_configuration_llava", f"{REF}/llava/model/configuration_llava.py")
    v = cfg.vision
    vc = ms.SiglipVisionConfig(hidden_size=v.hidden_size, intermediate_size=v.intermediate_size, num_hidden_layers=v.num_hidden_layers,
                               num_attention_heads=v.num_attention_heads, image_size=v.image_size, patch_size=v.patch_size,
                               num_channels=v.num_channels, layer_norm_eps=v.layer_norm_eps, hidden_act="gelu_pytorch_tanh")
    tower = ms.SiglipVisionModel(vc).to(torch.bfloat16)
    tower.load_state_dict({k[len(PREFIX["vision_tower"]):]: t for k, t in w.items() if k.startswith("vision_tower.")}, strict=False)
    projector = bp.MultimodalProjector(bp.MultimodalProjectorConfig(cfg.mm_projector_type),
                                       SimpleNamespace(mm_hidden_size=cfg.mm_hidden_size, hidden_size=cfg.llm.hidden_size)).to(torch.bfloat16)
    projector.load_state_dict({k[len("mm_projector."):]: t for k, t in w.items() if k.startswith("mm_projector.")}, strict=True)
    llm, _ = G.build_hf_llm(cfg, {k: t.float() for k, t in w.items()})
    m = reference_save_pretrained()()
    m.llm = llm.to(torch.bfloat16)
    m.mm_projector = projector
    wrapper = torch.nn.Module()                                    # VisionTower (multimodal_encoder/vision_encoder.py:32-52): .vision_tower, .config, .image_processor
    wrapper.vision_tower = tower
    wrapper.config = tower.config
    wrapper.image_processor = SiglipImageProcessor(size={"height": v.image_size, "width": v.image_size})
    m.vision_tower = wrapper
    m.config = lc.LlavaConfig(hidden_size=cfg.llm.hidden_size, mm_hidden_size=cfg.mm_hidden_size, mm_vision_select_layer=-2,
                              mm_vision_select_feature="cls_patch", mm_projector_type=cfg.mm_projector_type)
    m.save_pretrained(d)                                             # the reference's own writer
    files = {}
    for dirpath, _, names in os.walk(d):
        for n in sorted(names):
            path = os.path.join(dirpath, n)
            rel = os.path.relpath(path, d)
            if n.endswith(".json"):
                text = open(path).read()
                files[rel] = {"json": text.replace(d, CKPT)}
            elif n.endswith(".safetensors"):
                tensors = []
                with safe_open(path, framework="pt") as f:
                    meta = f.metadata()
                    for k in f.keys():
                        t = f.get_tensor(k)
                        folder = rel.split(os.sep)[0]
                        src = PREFIX[folder] + k
                        if src not in w and tied and src == "llm.lm_head.weight":
                            src = "llm.model.embed_tokens.weight"
                        if src not in w and k.startswith("vision_model.head."):     # the pooling head VILA never uses: randomly initialised,
                            tensors.append([k, None, str(t.dtype).replace("torch.", ""), list(t.shape), None])   # the tests write zeros
                            continue
                        assert src in w and torch.equal(w[src].to(t.dtype).reshape(t.shape), t), (rel, k)
                        tensors.append([k, src, str(t.dtype).replace("torch.", ""), list(t.shape), crc(t)])
                files[rel] = {"safetensors": {"metadata": meta, "tensors": tensors}}
            else:
                raise RuntimeError(f"unexpected file in the reference-written checkpoint: {rel}")
    return {"seed": 21, "files": files}


def config_loader(d):
    from transformers import AutoConfig, PretrainedConfig
    cfg = configs.tiny("mlp_downsample")
    checkpoint.save_pretrained(rand_model(cfg, 7), d)
    lc = G.load_by_path("ref_configuration_llava", f"{REF}/llava/model/configuration_llava.py")
    config = lc.LlavaConfig.from_pretrained(d)
    config.resume_path = d                                               # llava/model/builder.py:110-113 does this right after loading the config
    rec = {"llava_config": {k: getattr(config, k) for k in ("hidden_size", "mm_hidden_size", "mm_vision_select_layer", "mm_vision_select_feature")},
           "sub_config_types": {k: type(getattr(config, k, None)).__name__ for k in ("llm_cfg", "vision_tower_cfg", "mm_projector_cfg")}}
    bsrc = open(f"{REF}/llava/model/builder.py").read()
    pfn = next(n for n in ast.parse(bsrc).body if isinstance(n, ast.FunctionDef) and n.name == "prepare_config_for_eval")
    bns = {"PretrainedConfig": PretrainedConfig}
    exec(compile(ast.get_source_segment(bsrc, pfn), "builder.py", "exec"), bns)
    bns["prepare_config_for_eval"](config, {"torch_dtype": torch.bfloat16})
    rec["model_dtype"] = config.model_dtype
    rec["vision_tower_cfg_type_for_eval"] = type(config.vision_tower_cfg).__name__
    src = open(f"{REF}/llava/model/utils/utils.py").read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "get_model_config")
    ns = {"os": os, "osp": osp, "PretrainedConfig": PretrainedConfig, "repo_exists": lambda p: False, "HFValidationError": Exception,
          "snapshot_download": None}
    exec(compile(ast.get_source_segment(src, fn), "utils.py", "exec"), ns)
    paths = ns["get_model_config"](config)
    rec["paths"] = [os.path.relpath(p, d) for p in paths]
    rec["llm_model_type"] = AutoConfig.from_pretrained(paths[0]).model_type      # language_model/builder.py:66-70
    return rec


def main():
    fx = {"cases": {}}
    for proj, tied in CASES:
        with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
            fx["cases"][proj] = {"tied": tied, "ours_in_reference": ours_in_reference(proj, tied, os.path.join(a, "ckpt")),
                                 "reference_writer": reference_writer(proj, tied, os.path.join(b, "ref_ckpt"))}
    with tempfile.TemporaryDirectory() as c:
        fx["config_loader"] = config_loader(os.path.join(c, "ckpt"))
    with open(OUT, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
