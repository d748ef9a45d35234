"""The decode drivers (vila_amd/modules.py: the step table, `_capture`, the row finisher) on the device: a captured step replays exactly what
the step-by-step launches compute, for every (W4?, sampled?) variant of the solo and the batched step.  The capture runs the step once before it
records it and restores the state in between; a restore that is off by one position shifts every token, which is what these cases catch.

Tiny config with intermediate_size 1152 (hidden 512, 2 layers, 4 query / 2 kv heads of 128, vocab 1000): one shape serves bf16 and W4."""
import pytest
import torch

from vila_amd import configs, synthetic

pytestmark = pytest.mark.gpu

N_NEW = 6
VARIANTS = [(False, False), (False, True), (True, False), (True, True)]
_llms = {}


def _llm(w4):
    from vila_amd.vlm import build_model
    if w4 not in _llms:
        cfg = configs.tiny("mlp_downsample")
        cfg.llm.intermediate_size = 1152
        w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 5).items()}
        llm = build_model(cfg, weights=w).llm
        if w4:
            llm.quantize_w4(batch_decode=True)
        _llms[w4] = llm
    return _llms[w4]


def _prompts(llm, lens, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 900, (len(lens), max(lens)), generator=g)
    mask = torch.zeros(len(lens), max(lens), dtype=torch.bool)
    for b, n in enumerate(lens):
        mask[b, :n] = True
    return llm.embed_tokens(ids.cuda()), mask.cuda()


@pytest.mark.parametrize("w4,sampled", VARIANTS)
def test_solo_graph_equals_eager_and_is_reused(w4, sampled):
    llm = _llm(w4)
    e, _ = _prompts(llm, [20], 11)
    kw = dict(inputs_embeds=e, max_new_tokens=N_NEW, eos_token_id=-1)
    if sampled:
        kw.update(do_sample=True, top_k=50, seed=1234)
    llm._drop_decode_session()
    eager = llm.generate(use_graph=False, **kw)
    assert llm._decode.graph is None
    first = llm.generate(use_graph=True, **kw)
    st, graph = llm._decode, llm._decode.graph
    assert graph is not None
    second = llm.generate(use_graph=True, **kw)
    assert eager.shape == (1, N_NEW)
    assert torch.equal(first, eager), (first.tolist(), eager.tolist())
    assert torch.equal(second, first), (second.tolist(), first.tolist())
    assert llm._decode is st and st.graph is graph


@pytest.mark.parametrize("w4,sampled", VARIANTS)
def test_batch_graph_equals_eager(w4, sampled):
    llm = _llm(w4)
    lens = [20, 13, 5]
    e, mask = _prompts(llm, lens, 12)
    sampling = [(1.0, 50, 1.0, 4321 + b) for b in range(len(lens))] if sampled else None
    llm._drop_batch_session()
    eager = llm._generate_batch(e, mask, N_NEW, -1, None, use_graph=False, sampling=sampling)
    assert llm._bdecode.graph is None and llm._bdecode.sampling == sampled
    graph = llm._generate_batch(e, mask, N_NEW, -1, None, use_graph=True, sampling=sampling)
    assert llm._bdecode.graph is not None
    assert eager.shape == (len(lens), N_NEW)
    assert torch.equal(graph, eager), (graph.tolist(), eager.tolist())


@pytest.mark.parametrize("w4", [False, True])
def test_verify_graph_is_captured_once_and_replays_the_same_ids(w4):
    llm = _llm(w4)
    e, _ = _prompts(llm, [20], 13)
    ids = torch.randint(0, 900, (1, 20), generator=torch.Generator().manual_seed(13))        # the ids `_prompts` embedded
    kw = dict(inputs_embeds=e, max_new_tokens=N_NEW, eos_token_id=-1, prompt_lookup_num_tokens=3)
    llm._drop_session("_vdecode")
    first = llm.generate(prompt_ids=ids, **kw)                       # captures: the warm-up step advances the state, `restore` puts it back
    st, graph = llm._vdecode, llm._vdecode.graph
    assert graph is not None and first.shape == (1, N_NEW)
    second = llm.generate(prompt_ids=ids, **kw)
    assert torch.equal(second, first), (second.tolist(), first.tolist())
    assert llm._vdecode is st and st.graph is graph
    third = llm.generate(prompt_ids=ids, draft_ids=first, **kw)      # candidate mode: n_cand is a device scalar, so the same graph serves it
    assert torch.equal(third, first), (third.tolist(), first.tolist())
    assert llm._vdecode is st and st.graph is graph
