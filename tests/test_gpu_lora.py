"""The LoRA step (vila_amd/lora.py LoRATrainer) on the GPU against fp32 autograd through the unchanged CPU oracle: the oracle gets a weight dict
whose seven projections per layer are W + s (B @ A), built from leaf tensors A and B, so A.grad and B.grad are the references (tests/lora_ref.py).
B is random non-zero.  Bounds are the project's own: loss 1e-2 relative, every gradient tensor cosine >= GRAD_COS_MIN (0.999) and rel-L2 <= 6e-2.

Measured on MI355X: tiny (r = 16) loss 9.2136 against 9.2230, worst gradient cosine 0.99963, worst rel-L2 0.027; NVILA-8B widths (r = 64) loss 14.4810
against 14.4797, worst cosine 0.99981, worst rel-L2 0.020; two micro-batches accumulated 0.99963 / 0.027; zero B: the loss equals the plain trainer's
bit for bit; merged prefill logits rel-L2 1.2e-2 (the un-merged model's are 0.36 away).  No per-tensor exception."""
import os

import pytest
import torch

from tests import lora_ref as LR
from tests.gpu_util import GRAD_COS_MIN, grad_cos, rel_l2
from vila_amd import configs, run, synthetic

pytestmark = pytest.mark.gpu

# Per-tensor exceptions to the stated bounds: (test tag, tensor-name suffix) -> (cosine bound, rel-L2 bound, measured, why).  None so far.
GRAD_EXCEPTIONS = {}
REL_MAX = 6e-2


def _bounds(tag, name):
    for (t, suffix), (cos, rel, _measured, _why) in GRAD_EXCEPTIONS.items():
        if t == tag and name.endswith(suffix):
            return cos, rel
    return GRAD_COS_MIN, REL_MAX


def _tiny_batch(cfg):
    """The batch of test_sft_forward_backward_matches_oracle_autograd: two packed samples, three images."""
    g = torch.Generator().manual_seed(22)
    L = 14
    ids = torch.randint(0, 900, (2, L), generator=g)
    ids[0, 0] = cfg.image_token_id
    ids[1, 0] = cfg.image_token_id; ids[1, 5] = cfg.image_token_id
    mask = torch.ones(2, L, dtype=torch.bool); mask[0, 11:] = False
    labels = torch.randint(0, 900, (2, L), generator=g); labels[:, :6] = -100
    return ids, labels, mask, 3


def _weights(cfg, seed):
    return {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, seed).items()}


def _trainer(cfg, w, lora_cfg, ad=None, **kw):
    from vila_amd.lora import LoRATrainer
    from vila_amd.vlm import build_model
    tr = LoRATrainer(build_model(cfg, weights=w), lora_cfg, **kw)
    if ad is not None:
        tr.adapters.load_state_dict(ad.state_dict())
        tr.flat.sync_master_from_params()
    return tr


def _compare(tag, tr, ref_grads):
    grads = tr.flat.named_grads()
    assert set(grads) == set(ref_grads), sorted(set(grads) ^ set(ref_grads))[:6]
    bad, worst = [], (1.0, 0.0)
    for name, gref in ref_grads.items():
        got = grads[name].float().cpu()
        if float(gref.norm()) < 1e-6:
            assert float(got.norm()) < 1e-3, name
            continue
        cos, rel = grad_cos(tag, name, got, gref), rel_l2(got, gref)
        worst = (min(worst[0], cos), max(worst[1], rel))
        cmin, rmax = _bounds(tag, name)
        if cos < cmin or rel > rmax:
            bad.append((name, round(cos, 5), round(rel, 4)))
    print(f"{tag}: {len(ref_grads)} gradient tensors, worst cosine {worst[0]:.5f}, worst rel-L2 {worst[1]:.4f}")
    assert not bad, bad
    return worst


def _lora_vs_oracle(tag, cfg, lora_cfg, seed, ids, labels, mask, n_images):
    from vila_amd.train import count_targets
    w = _weights(cfg, seed)
    px = synthetic.make_pixels(cfg, n_images, seed).to(torch.bfloat16)
    ad = LR.random_adapters(cfg, lora_cfg, seed)
    n_items = count_targets(ids, labels, mask, (cfg.image_token_id, cfg.video_token_id))
    ref, ref_grads = LR.oracle_lora_grads(cfg, ad, w, px, ids, labels, mask, n_items)
    tr = _trainer(cfg, w, lora_cfg, ad, optimizer_state=False)
    loss = tr.forward_backward(ids, [p.cuda() for p in px], labels, mask, n_items)
    torch.cuda.synchronize()
    print(f"{tag}: loss {float(loss):.5f} vs oracle {ref:.5f}")
    assert abs(float(loss) - ref) < 1e-2 * abs(ref), (float(loss), ref)
    _compare(tag, tr, ref_grads)
    assert [p for p, _, _ in tr.reducer.log] == [f"llm.model.layers.{i}.lora." for i in reversed(range(cfg.llm.num_hidden_layers))] + ["mm_projector."]
    return tr


def test_lora_gradients_match_oracle_autograd_tiny():
    from vila_amd.lora import LoraConfig
    cfg = configs.tiny("mlp_downsample")
    ids, labels, mask, n_img = _tiny_batch(cfg)
    _lora_vs_oracle("lora_tiny", cfg, LoraConfig(r=16), 3, ids, labels, mask, n_img)


def test_lora_gradients_match_oracle_autograd_at_8b_widths():
    """NVILA-8B widths, 4 ViT + 2 LLM layers, r = 64, 64 text tokens per sample: the R = 192 stacks, N = 18944 and the 512-wide k / v slices."""
    from vila_amd.lora import LoraConfig
    cfg = configs.reduced_8b(layers_v=4, layers_l=2, vocab=32000)
    cfg.image_token_id, cfg.llm.eos_token_id = 31999, 31998
    b, T = 2, 64
    ids = torch.stack([synthetic.make_prompt(cfg, T, 1, 40 + i) for i in range(b)], 0)
    labels = ids.clone()
    labels[:, : 1 + T - 32] = -100
    mask = torch.ones_like(ids, dtype=torch.bool)
    _lora_vs_oracle("lora_8b_width", cfg, LoraConfig(r=64), 17, ids, labels, mask, b)


def test_zero_b_forward_is_the_plain_forward():
    """PEFT's initial state (B = 0): the LoRA trainer's loss against the plain SFTTrainer's on the same batch, within 1e-2 relative."""
    from vila_amd.lora import LoraConfig
    from vila_amd.train import SFTTrainer, count_targets
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    ids, labels, mask, n_img = _tiny_batch(cfg)
    w = _weights(cfg, 3)
    px = [p.cuda() for p in synthetic.make_pixels(cfg, n_img, 3).to(torch.bfloat16)]
    n = count_targets(ids, labels, mask, (cfg.image_token_id, cfg.video_token_id))
    plain = float(SFTTrainer(build_model(cfg, weights=w), optimizer_state=False).forward_backward(ids, px, labels, mask, n))
    tr = _trainer(cfg, w, LoraConfig(r=16), optimizer_state=False)
    assert float(tr.adapters.params.float().abs().sum()) > 0 and all(float(tr.adapters.tensor(0, n_).float().abs().sum()) == 0 for n_ in ("Bt_q", "Bt_down"))
    got = float(tr.forward_backward(ids, px, labels, mask, n))
    print(f"zero B: LoRA loss {got!r} vs plain {plain!r}; bit-equal: {got == plain}")
    assert abs(got - plain) < 1e-2 * abs(plain)


def test_two_identical_lora_steps_produce_identical_bits_and_move_only_the_trainables():
    from vila_amd.lora import LoraConfig
    cfg = configs.tiny("mlp_downsample")
    ids, labels, mask, n_img = _tiny_batch(cfg)
    w = _weights(cfg, 3)
    px = [p.cuda() for p in synthetic.make_pixels(cfg, n_img, 3).to(torch.bfloat16)]
    ad = LR.random_adapters(cfg, LoraConfig(r=16), 5)
    outs = []
    for _ in range(2):
        tr = _trainer(cfg, w, LoraConfig(r=16), ad, lr=1e-2)
        base_before = tr.base.params.clone()
        p0 = tr.flat.params.clone()
        losses = [float(tr.step(ids, px, labels, mask)) for _ in range(4)]
        torch.cuda.synchronize()
        a, b = tr.base.span("llm.")
        assert torch.equal(tr.base.params[a:b].view(torch.int16), base_before[a:b].view(torch.int16)), "a step changed a bit of the LLM's base parameters"
        moved = tr.flat.params != p0
        na = tr.adapters.numel
        assert bool(moved[:na].any()) and bool(moved[na:].any()), "the adapters and the tuned projector must both move"
        assert losses[-1] < losses[0], losses
        outs.append((losses, tr.flat.params.clone(), tr.flat.master.clone(), tr.flat.m.clone(), tr.flat.v.clone()))
        assert tr.state_numel() == tr.flat.master.numel() == tr.flat.grads.numel() and tr.base.grads is None
    print(f"losses over 4 steps: {outs[0][0]}")
    assert outs[0][0] == outs[1][0], (outs[0][0], outs[1][0])
    for x, y in zip(outs[0][1:], outs[1][1:]):
        assert torch.equal(x, y), "two identical LoRA runs differ: a reduction is order-dependent"


def test_accumulated_lora_update_matches_one_oracle_run_on_the_union():
    from vila_amd.lora import LoraConfig
    from vila_amd.train import count_targets
    cfg = configs.tiny("mlp_downsample")
    ids, labels, mask, n_img = _tiny_batch(cfg)
    w = _weights(cfg, 3)
    px = synthetic.make_pixels(cfg, n_img, 3).to(torch.bfloat16)
    lc = LoraConfig(r=16)
    ad = LR.random_adapters(cfg, lc, 3)
    n = count_targets(ids, labels, mask, (cfg.image_token_id, cfg.video_token_id))
    _, ref_grads = LR.oracle_lora_grads(cfg, ad, w, px, ids, labels, mask, n)
    tr = _trainer(cfg, w, lc, ad, lr=0.0)
    micro = [dict(input_ids=ids[:1], images=[px[0].cuda()], labels=labels[:1], attention_mask=mask[:1]),
             dict(input_ids=ids[1:], images=[px[1].cuda(), px[2].cuda()], labels=labels[1:], attention_mask=mask[1:])]
    tr.step_accumulated(micro)
    torch.cuda.synchronize()
    _compare("lora_accumulated", tr, ref_grads)


def test_lora_c_abi_driver_raises():
    from vila_amd.lora import LoraConfig
    cfg = configs.tiny("mlp_downsample")
    ids, labels, mask, n_img = _tiny_batch(cfg)
    tr = _trainer(cfg, _weights(cfg, 3), LoraConfig(r=16), optimizer_state=False)
    with pytest.raises(NotImplementedError, match="adapters"):
        tr.forward_backward_c(ids, [], labels, mask)


def _samples(cfg, n, seed):
    out = []
    for i in range(n):
        ids = synthetic.make_prompt(cfg, 12 + i % 3, 1 if i % 2 == 0 else 0, seed + i)
        labels = ids.clone(); labels[: 6] = -100
        px = synthetic.make_pixels(cfg, 1, seed + i).to(torch.bfloat16)[0] if i % 2 == 0 else None
        out.append({"input_ids": ids, "labels": labels, "image": [px] if px is not None else []})
    return out


def _collate(insts):
    L = max(int(x["input_ids"].numel()) for x in insts)
    ids = torch.full((len(insts), L), 0, dtype=torch.int64)
    lab = torch.full((len(insts), L), -100, dtype=torch.int64)
    mask = torch.zeros((len(insts), L), dtype=torch.bool)
    for r, x in enumerate(insts):
        n = int(x["input_ids"].numel())
        ids[r, :n], lab[r, :n], mask[r, :n] = x["input_ids"], x["labels"], True
    return {"input_ids": ids, "labels": lab, "attention_mask": mask,
            "media": {"image": [t.cuda() for x in insts for t in x["image"]], "video": []}, "media_config": {"image": {}}}


def test_resumed_lora_run_equals_the_uninterrupted_one(tmp_path):
    """run.train for 4 updates against 2 updates, checkpoint, a fresh trainer, load, 2 more: adapters, projector and optimizer state bit-equal."""
    from vila_amd import lora
    cfg = configs.tiny("mlp_downsample")
    data = _samples(cfg, 8, 70)
    w = _weights(cfg, 12)
    mk = lambda d: run.TrainArgs(output_dir=str(tmp_path / d), per_device_train_batch_size=2, num_train_epochs=1, save_steps=2, save_total_limit=2,
                                 learning_rate=1e-3, warmup_ratio=0.1)
    kw = dict(save_fn=lora.save_checkpoint, load_fn=lora.load_checkpoint, final_save_fn=lora.save_final)
    fresh = lambda: _trainer(cfg, w, lora.LoraConfig(r=16, seed=4), lr=1e-3)
    a = fresh()
    sa = run.train(a, data, _collate, mk("a"), **kw)
    assert sa.global_step == 4
    for f in ("adapter_config.json", "adapter_model.safetensors", "non_lora_trainables.bin", "config.json"):
        assert os.path.isfile(tmp_path / "a" / f), f
    c = fresh()
    calls, real = {"n": 0}, c.step

    def capped(*a_, **k_):
        if calls["n"] == 2:
            raise KeyboardInterrupt
        calls["n"] += 1
        return real(*a_, **k_)
    c.step = capped
    with pytest.raises(KeyboardInterrupt):
        run.train(c, data, _collate, mk("c"), **kw)
    assert os.listdir(tmp_path / "c") == ["checkpoint-2"]
    d = fresh()
    sd = run.train(d, data, _collate, mk("c"), **kw)
    torch.cuda.synchronize()
    assert sd.global_step == 4 and [r["loss"] for r in sd.log_history[-2:]] == [r["loss"] for r in sa.log_history[-2:]]
    for name in ("params", "master", "m", "v"):
        assert torch.equal(getattr(d.flat, name), getattr(a.flat, name)), f"{name} of the resumed run differs from the uninterrupted run"
    assert d.flat.bucket_steps == a.flat.bucket_steps and d.flat.step_count == a.flat.step_count == 4


def test_merged_adapter_serves_prefill_and_a_captured_decode_graph():
    """merge_adapter: prefill_packed logits against the oracle on the merged fp32 weights within tests/test_gpu_model.py's bound for prefill logits
    (rel-L2 < 3e-2); a decode graph captured before the merge produces the merged model's ids after it."""
    from oracle import vila_oracle as O
    from vila_amd.lora import LoraConfig, merge_adapter
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    w = _weights(cfg, 6)
    model = build_model(cfg, weights=w)
    ad = LR.random_adapters(cfg, LoraConfig(r=16), 6)
    px = synthetic.make_pixels(cfg, 1, 6).to(torch.bfloat16)
    ids = synthetic.make_prompt(cfg, 16, 1, 6)[None]
    media = {"image": [px[0].cuda()]}
    kw = dict(max_new_tokens=6, eos_token_id=-1)
    e, _, _ = model._embed(ids, media)
    before = model.llm.generate(inputs_embeds=e, use_graph=True, **kw)               # captures the graph on the un-merged weights
    _, lg0 = model.llm.generate(inputs_embeds=e, return_logits=True, use_graph=False, **kw)
    merge_adapter(model, ad)
    S = e.shape[1]
    r = model.llm.prefill_packed(e[0], torch.arange(S, dtype=torch.int32, device="cuda"), None, S, want_all_logits=True)
    wm = {k: v.detach() for k, v in LR.merged_weights(w, ad).items()}
    logits, _ = O.qwen2_forward(e.float().cpu(), wm, cfg.llm)[:2]
    rel = rel_l2(r.all_logits, logits[0])
    plain, _ = O.qwen2_forward(e.float().cpu(), w, cfg.llm)[:2]
    print(f"merged prefill logits rel-L2 {rel:.3e} (the un-merged model's logits are {rel_l2(plain[0], logits[0]):.3e} away)")
    assert rel < 3e-2 and rel_l2(plain[0], logits[0]) > 3 * rel
    graph = model.llm.generate(inputs_embeds=e, use_graph=True, **kw)
    eager, lg1 = model.llm.generate(inputs_embeds=e, return_logits=True, use_graph=False, **kw)
    assert torch.equal(graph, eager)
    assert float((lg1[0] - lg0[0]).abs().max()) > 1e-2                                # the weights really moved
    del before


def test_plain_sft_step_announces_the_buckets_it_always_did():
    """No adapters: the launch log of a plain SFTTrainer step (reducer.log) has the bucket order of the parent commit."""
    from vila_amd.train import SFTTrainer, count_targets
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    ids, labels, mask, n_img = _tiny_batch(cfg)
    px = [p.cuda() for p in synthetic.make_pixels(cfg, n_img, 3).to(torch.bfloat16)]
    tr = SFTTrainer(build_model(cfg, weights=_weights(cfg, 3)), optimizer_state=False)
    tr.forward_backward(ids, px, labels, mask, count_targets(ids, labels, mask, (cfg.image_token_id, cfg.video_token_id)))
    pre = "vision_tower.vision_tower.vision_model."
    want = (["llm.lm_head.", "llm.model.norm."] + [f"llm.model.layers.{i}." for i in reversed(range(cfg.llm.num_hidden_layers))]
            + ["llm.model.embed_tokens.", "mm_projector."] + [f"{pre}encoder.layers.{i}." for i in reversed(range(cfg.vision.num_used_layers))]
            + [pre + "embeddings."])
    assert [p for p, _, _ in tr.reducer.log] == want
