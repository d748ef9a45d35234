"""LoRA adapters served unmerged, end to end: the batched session with an adapter bank (vila_amd/lora_serving.py AdapterBank, batch_open(adapters=),
vila_llm_decode_step_batch_lora, vila_llm_prefill_lora), generate(adapter=, adapters=) and the continuous batcher's routing.

(a) rows without an adapter, and rows under an adapter whose B is zero, against the session without the flag: same ids, same last-step logits bits
    (the step is compared: the rows are prefilled by the base prefill, see the test).
(b) against the fp32 oracle: NVILA-8B widths, 2 layers, five rows of 72 .. 28 keys under an r = 64 adapter (all seven projections), an r = 16
    adapter (q, v and down only; zero-padded to the bank's 64) and the base model; every row teacher-forced against `O.greedy_generate` on the fp32
    weights W + s B A of ITS adapter (nothing rounded).  Logits rel-L2 < 3e-2 (the bound of tests/test_gpu_batch_decode.py::
    test_batched_decode_logits_of_every_row_vs_the_fp32_oracle_at_8b_widths), prefill row and decode rows separately, ids under margin_aware_ids with
    at least one decisive decode step per row.  The adapters' B are normal with standard deviation 0.08 (r = 64, s = 0.25) and 0.03 (r = 16, s = 2):
    with them the oracle's merged and base logits differ by rel-L2 0.31 - 0.35 on these prompts (asserted >= 0.3 below), and the oracle alone — run
    on the CPU before any GPU run, the model's weights are drawn with the CPU generator for that — has in every row a decode step whose top-1 / top-2
    margin is at least 0.93 (rows: 2.09, 1.26, 1.08, 1.39, 0.93), above 4 x 1.5e-2 x max |logit| = 0.79 - 1.01, the error a rel-L2 of 1.5e-2 allows.
(c) a row's ids and logits are the same bits whether the session's other rows idle or run under other adapters.
(d) unload an adapter, load another into the same slot: the session and its captured graph are the same objects and serve the new adapter like a
    fresh session; unloading under a live row raises.
(e) one session with sampling + penalties + logprobs + adapters: a sampled, penalised row under an adapter draws, bit for bit, `ops.sample` of that
    step's penalised logits; graph replays equal eager launches; the records are log-softmax of the raw logits.
(f) `ContinuousBatcher(adapters=True)`: two concurrent requests under different adapters reply what generate(adapter=) gives each alone, an unknown
    `model` is the base model's request, a sampled adapter request without batch_sampled fails by name of the flag.
(g) an adapter folder with tuned-projector tensors: `_embed` under it equals `_embed` of a model whose projector was overwritten; a folder that
    tunes the vision tower is refused."""
import time

import pytest
import torch

from oracle import vila_oracle as O
from tests import lora_serving_ref as R
from tests.gpu_util import margin_aware_ids, rel_l2
from tests.lora_serving_ref import assert_bits_equal
from tests.penalty_ref import counts_of, penalize_ref
from vila_amd import configs, serving, synthetic

pytestmark = pytest.mark.gpu

N_NEW = 8
NAMES = ["a64", "a16", None, "a64", "a16"]


def _i32(t):
    return t.contiguous().view(torch.int32)


# ---- the tiny model: (a), (f), (g) ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    model = build_model(cfg, seed=21)
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(0, 900, (3, 20), generator=g)
    mask = torch.ones(3, 20, dtype=torch.bool); mask[1, 13:] = False; mask[2, 5:] = False
    return cfg, model, model.llm.embed_tokens(ids.cuda()), mask.cuda()


def test_zero_b_adapters_and_rows_without_one_keep_the_bits_of_the_session_without_the_flag(tiny):
    """Three rows of 20, 13 and 5 keys, 10 steps.  The STEP is what is compared: every row is prefilled by the base prefill (under a zero-B adapter the
    model is the base model; the prefill under an adapter is other launches than the base prefill — no RoPE / norm hand-offs, gate and up as two
    GEMMs, no last-row pruning — and is held to the oracle in (b), not to the base prefill's bits), then its entry of row_adapter is set.  Rows under
    the zero-B adapter add D = +0.0 to the fp32 sums, rows with -1 add nothing: ids and last-step logits are those of the session without the flag,
    bit for bit.  Through generate(adapter=) with no adapter named, prefill included, the same holds."""
    from vila_amd import lora
    from vila_amd.lora_serving import AdapterBank
    cfg, model, e, mask = tiny
    llm = model.llm
    lens = [int(v) for v in mask.sum(1).tolist()]
    bank = AdapterBank(model, capacity=2, r=16)
    bank.load("zero", lora.LoraAdapters(cfg.llm, lora.LoraConfig(r=16, alpha=32)).init_(3))          # PEFT's initialisation: A random, B = 0

    def run(st, names):
        llm.batch_release(st, range(st.pos.numel()))
        first = [llm.batch_admit(st, b, e[b, :lens[b]]) for b in range(3)]
        for b, name in enumerate(names):
            if name is not None:
                llm._set_row_adapter(st, b, name)
        llm.batch_run(st, 10)
        out = (first, st.out_ids[:3, :10].clone(), st.logits[:3].clone())
        llm.batch_release(st, range(st.pos.numel()))
        return out
    st0 = llm.batch_open(3, 256, 16)
    assert getattr(st0, "lora", None) is None
    want = run(st0, [None] * 3)
    st = llm.batch_open(3, 256, 16, adapters=bank)
    assert st is not st0 and st.lora is not None and st.graph is not None
    for names in ([None, None, None], ["zero", None, "zero"], ["zero", "zero", "zero"]):
        got = run(st, names)
        print(f"rows under {names}: ids equal {got[0] == want[0] and bool(torch.equal(got[1], want[1]))}, logits bits equal "
              f"{bool(torch.equal(_i32(got[2]), _i32(want[2])))}")
        assert got[0] == want[0] and torch.equal(got[1], want[1]), (names, got[0], got[1].tolist(), want[0], want[1].tolist())
        assert_bits_equal(got[2], want[2], f"last-step logits of rows under {names} vs the session without the flag")
    assert bank.in_use == [0, 0]
    # generate(): the padded batch through the session with the bank, no adapter named, against the session without it
    want_ids = llm._generate_batch(e, mask, 11, -1, None)
    want_lg = llm._bdecode.logits[:3].clone()
    got_ids = llm.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=11, eos_token_id=-1, adapter=[None] * 3, adapters=bank)
    assert llm._bdecode.lora is not None, "the batch did not run in a session with the bank"
    assert torch.equal(got_ids, want_ids), (got_ids.tolist(), want_ids.tolist())
    assert_bits_equal(llm._bdecode.logits[:3], want_lg, "last-step logits of generate(adapter=[None, None, None])")


# ---- NVILA-8B widths: (b) - (e) ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    from vila_amd.lora_serving import AdapterBank
    from vila_amd.vlm import build_model
    cfg = configs.reduced_8b(layers_v=2, layers_l=2, vocab=32000)
    cfg.image_token_id, cfg.llm.eos_token_id = 31999, 31998
    model = build_model(cfg, seed=31, draw_device="cpu")             # (CPU-drawn: the oracle's margins were checked on the CPU on these weights)
    llm = model.llm
    w = {"llm." + n: p.detach().float().cpu() for n, p in llm.named_parameters()}
    ads = {"a64": R.random_adapter(cfg.llm, 64, 16.0, None, seed=1, b_std=0.08),
           "a16": R.random_adapter(cfg.llm, 16, 32.0, ("q_proj", "v_proj", "down_proj"), seed=2, b_std=0.03)}
    bank = AdapterBank(model, capacity=3, r=64)
    assert bank.load("a64", ads["a64"]) == 0 and bank.load("a16", ads["a16"]) == 1
    g = torch.Generator().manual_seed(31)
    ids = torch.randint(0, 31000, (5, 72), generator=g)
    lens = [72 - 11 * b for b in range(5)]                             # 72, 61, 50, 39, 28 keys
    mask = torch.ones(5, 72, dtype=torch.bool)
    for b in range(5):
        mask[b, lens[b]:] = False
    return dict(cfg=cfg, model=model, llm=llm, w=w, ads=ads, bank=bank, e=llm.embed_tokens(ids.cuda()), lens=lens, mask=mask.cuda())


def test_every_row_against_the_fp32_oracle_on_the_merged_weights_of_its_adapter(big):
    cfg, llm, w, bank, e, lens = big["cfg"], big["llm"], big["w"], big["bank"], big["e"], big["lens"]
    merged = {k: R.merged_llm_weights(w, ad) for k, ad in big["ads"].items()}
    want_ids, want_lg = [], []
    for b in range(5):
        eb = e[b:b + 1, :lens[b]].float().cpu()
        io, lo = O.greedy_generate(eb, w if NAMES[b] is None else merged[NAMES[b]], cfg, N_NEW, stop_at_eos=False)
        want_ids.append(io); want_lg.append(lo)
        if NAMES[b] is not None:                                       # the adapter matters: base logits on the same ids are far away
            _, base = O.greedy_generate(eb, w, cfg, N_NEW, stop_at_eos=False, forced_ids=io)
            assert rel_l2(lo, base) >= 0.3, f"row {b} ({NAMES[b]}): oracle merged vs base rel-L2 {rel_l2(lo, base):.3f}"
    forced = torch.stack(want_ids, 0)
    got_ids, got_lg = llm.generate(inputs_embeds=e, attention_mask=big["mask"], max_new_tokens=N_NEW, eos_token_id=-1, forced_ids=forced, return_logits=True,
                                   use_graph=False, adapter=NAMES, adapters=bank)
    assert llm._bdecode.lora is not None and got_lg.shape == (N_NEW, 5, cfg.llm.vocab_size)
    for b in range(5):
        lg_b = got_lg[:, b].cpu()
        pre, dec = rel_l2(lg_b[:1], want_lg[b][:1]), rel_l2(lg_b[1:], want_lg[b][1:])
        print(f"row {b} ({NAMES[b]}, {lens[b]} keys): prefill row rel-L2 {pre:.3e}, decode rows {dec:.3e}, max abs err {float((lg_b - want_lg[b]).abs().max()):.3e}")
        assert pre < 3e-2, f"row {b} ({NAMES[b]}): prefill-row logits vs oracle rel={pre:.3e}"
        assert dec < 3e-2, f"row {b} ({NAMES[b]}): decode-step logits vs oracle rel={dec:.3e}"
        decisive = margin_aware_ids(lg_b, want_lg[b], want_ids[b])
        assert torch.equal(got_ids[b].cpu()[decisive], want_ids[b][decisive])
        assert int(decisive[1:].sum()) >= 1, f"row {b} ({NAMES[b]}): no decisive decode step"
    # the free-running graph replay follows the oracle up to each row's first non-decisive step
    free = llm.generate(inputs_embeds=e, attention_mask=big["mask"], max_new_tokens=N_NEW, eos_token_id=-1, adapter=NAMES, adapters=bank)
    for b in range(5):
        margin_aware_ids(got_lg[:, b].cpu(), want_lg[b], want_ids[b], free_ids=free[b])


def _run_rows(llm, st, rows, k):
    """Admit {slot: (prompt embeddings, adapter)}, run k steps -> {slot: (first token, ids [k], last-step logits)}; everything released afterwards."""
    llm.batch_release(st, range(st.pos.numel()))
    first = {s: llm.batch_admit(st, s, x, adapter=name) for s, (x, name) in rows.items()}
    llm.batch_run(st, k)
    out = {s: (first[s], st.out_ids[s, :k].clone(), st.logits[s].clone()) for s in rows}
    llm.batch_release(st, range(st.pos.numel()))
    return out


def test_a_row_does_not_depend_on_what_the_other_rows_run_under(big):
    llm, bank, e, lens = big["llm"], big["bank"], big["e"], big["lens"]
    st = llm.batch_open(4, 256, 16, adapters=bank)
    x = {b: e[b, :lens[b]] for b in range(5)}
    alone = _run_rows(llm, st, {1: (x[0], "a64")}, 6)[1]
    beside = _run_rows(llm, st, {0: (x[1], "a16"), 1: (x[0], "a64"), 2: (x[2], None), 3: (x[4], "a16")}, 6)
    assert alone[0] == beside[1][0] and torch.equal(alone[1], beside[1][1]), (alone[0], alone[1].tolist(), beside[1][0], beside[1][1].tolist())
    assert_bits_equal(beside[1][2], alone[2], "logits of the a64 row beside rows under a16 and the base model")
    base_alone = _run_rows(llm, st, {2: (x[2], None)}, 6)[2]
    assert base_alone[0] == beside[2][0] and torch.equal(base_alone[1], beside[2][1])
    assert_bits_equal(beside[2][2], base_alone[2], "logits of the base row beside rows under adapters")
    assert bank.in_use == [0, 0, 0]


def test_a_reloaded_slot_is_served_by_the_same_session_and_graph(big):
    from vila_amd.lora_serving import AdapterBank
    model, llm, ads, e, lens = big["model"], big["llm"], big["ads"], big["e"], big["lens"]
    x = e[3, :lens[3]]
    bank = AdapterBank(model, capacity=1, r=64)
    assert bank.load("first", ads["a64"]) == 0
    llm._drop_batch_session()
    st = llm.batch_open(2, 256, 16, adapters=bank)
    graph = st.graph
    llm.batch_release(st, range(2))
    tok_a = llm.batch_admit(st, 0, x, adapter="first")
    llm.batch_run(st, 4)
    ids_a = st.out_ids[0, :4].clone()
    with pytest.raises(RuntimeError, match="live rows"):
        bank.unload("first")
    llm.batch_release(st, [0, 1])
    bank.unload("first")
    with pytest.raises(KeyError):
        llm.batch_admit(st, 0, x, adapter="first")
    assert bank.load("second", ads["a16"]) == 0                        # the same slot, the same buffers
    assert llm.batch_open(2, 256, 16, adapters=bank) is st and st.graph is graph, "loading into the bank must not cost the session or its graph"
    got = _run_rows(llm, st, {0: (x, "second")}, 4)[0]
    fresh_bank = AdapterBank(model, capacity=1, r=64)
    fresh_bank.load("second", ads["a16"])
    llm._drop_batch_session()
    st2 = llm.batch_open(2, 256, 16, adapters=fresh_bank)
    assert st2 is not st
    want = _run_rows(llm, st2, {0: (x, "second")}, 4)[0]
    assert got[0] == want[0] and torch.equal(got[1], want[1]), (got[0], got[1].tolist(), want[0], want[1].tolist())
    assert_bits_equal(got[2], want[2], "logits under the adapter loaded into a reused slot vs a fresh session")
    assert (tok_a, ids_a.tolist()) != (got[0], got[1].tolist()), "the two adapters gave the same reply: the test shows nothing"


def test_sampling_penalties_logprobs_and_adapters_in_one_session(big):
    from vila_amd import ops
    cfg, llm, bank, e, lens = big["cfg"], big["llm"], big["bank"], big["e"], big["lens"]
    V, P, k = cfg.llm.vocab_size, lens[1], 5
    smp, pen = (0.9, 30, 0.95, 77), (1.3, 0.5, 0.25)
    st = llm.batch_open(3, 256, 16, sampling=True, penalties=True, logprobs=True, adapters=bank)
    assert st.lora is not None and st.sp is not None and st.pen is not None and st.lp is not None and st.graph is not None

    def run(step):
        llm.batch_release(st, range(3))
        toks = [llm.batch_admit(st, 0, e[1, :P], sampling=smp, penalties=pen, adapter="a64")]
        llm.batch_admit(st, 1, e[2, :lens[2]])                         # a greedy base row beside it
        raw = []
        for _ in range(k):
            step()
            raw.append(st.logits[0].clone())
            toks.append(int(st.token[0]))
        lp = llm.batch_logprobs(st, 0)
        llm.batch_release(st, range(3))
        return toks, raw, lp

    def eager():
        torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(st.stream):
            llm._batch_step(st)
        st.stream.synchronize()
    toks, raw, lp = run(lambda: llm.batch_run(st, 1))
    for j in range(1, k + 1):                                          # step j consumed toks[j - 1] at position P - 1 + j and has counted toks[:j]
        y = penalize_ref(raw[j - 1][None].cpu(), counts_of(toks[:j], V), *pen)[0]
        want = int(ops.sample(y.cuda(), smp[0], smp[1], smp[2], smp[3], counter=torch.tensor([P - 1 + j], dtype=torch.int32, device="cuda")))
        assert toks[j] == want, (j, toks, want)
        ref_lp = float(torch.log_softmax(raw[j - 1].double(), -1)[toks[j]])
        assert abs(float(lp.token_logprobs[j]) - ref_lp) < 1e-3, (j, float(lp.token_logprobs[j]), ref_lp)
    toks_e, raw_e, _ = run(eager)
    assert toks_e == toks, (toks_e, toks)
    for a, b in zip(raw_e, raw):
        assert_bits_equal(a, b, "eager launches vs graph replays: the adapter row's logits")


# ---- serving: (f) -----------------------------------------------------------------------------------------------------------------------------------------
def test_continuous_batcher_serves_requests_under_different_adapters_in_one_batch(tiny):
    from tests.test_serving_cpu import _Tok
    from vila_amd.lora_serving import AdapterBank

    class Tok(_Tok):
        def decode(self, ids, skip_special_tokens=True):
            return " ".join(f"w{int(i)}" for i in ids)

    cfg, model, _, _ = tiny
    llm, tok = model.llm, Tok()
    bank = AdapterBank(model, capacity=2, r=16)
    bank.load("ada", R.random_adapter(cfg.llm, 16, 32.0, None, seed=11, b_std=0.05))
    bank.load("bob", R.random_adapter(cfg.llm, 16, 32.0, ("q_proj", "v_proj", "down_proj"), seed=12, b_std=0.08))
    prompts = {"ada": "describe the image in many words", "bob": "what is this ?", None: "describe the image in many words"}
    eng = serving.HipBatchEngine(model, tok, n_slots=4, max_ctx=256, max_new_tokens=64, eos_token_id=-1, adapters=bank)
    want = {}
    for name, prompt in prompts.items():
        ids = llm.generate(inputs_embeds=eng.embed(prompt, None)[None], max_new_tokens=12, eos_token_id=-1, adapter=name, adapters=bank)
        want[name] = tok.decode(ids[0].tolist())
    assert len(set(want.values())) == 3, f"the adapters do not change the replies: the test shows nothing ({want})"
    cb = serving.ContinuousBatcher(eng, max_batch=4, chunk=2, adapters=True)
    try:
        fa = cb.submit(prompts["ada"], 12, model="ada")
        while not any(ev[0] == "run" for ev in cb.events):
            time.sleep(0.001)
        fb = cb.submit(prompts["bob"], 12, model="bob")                # joins while the first row decodes
        fc = cb.submit(prompts[None], 12, model="somebody-else")       # an unknown `model`: the base model's request
        assert fa.result(timeout=120) == want["ada"] and fb.result(timeout=120) == want["bob"] and fc.result(timeout=120) == want[None]
        assert llm._bdecode.lora is not None and not any(ev[0] == "solo" for ev in cb.events)
        admits = [ev for ev in cb.events if ev[0] == "admit"]
        assert len(admits) == 3 and admits[1][3] >= 1, admits           # the second request joined beside a live row
        with pytest.raises(ValueError, match="batch_sampled=True"):
            cb.submit(prompts["bob"], 12, model="bob", temperature=0.7, top_p=0.9).result(timeout=120)
        assert bank.in_use == [0, 0]
    finally:
        cb.close()


# ---- the tuned projector: (g) -------------------------------------------------------------------------------------------------------------------------------
def test_an_adapter_with_a_tuned_projector_embeds_its_media_through_it(tiny, tmp_path):
    from vila_amd import lora
    from vila_amd.lora_serving import AdapterBank
    from vila_amd.vlm import build_model
    cfg, model, _, _ = tiny
    ad = R.random_adapter(cfg.llm, 16, 32.0, None, seed=5)
    g = torch.Generator().manual_seed(5)
    tuned = {"mm_projector." + n: (p.detach().float().cpu() + 0.05 * torch.randn(p.shape, generator=g)).to(torch.bfloat16)
             for n, p in model.mm_projector.named_parameters()}
    folder = str(tmp_path / "tuned")
    lora.save_adapter(ad, folder, non_lora=tuned)
    bank = AdapterBank(model, capacity=2, r=16)
    bank.load("tuned", folder)
    bank.load("plain", ad)
    assert bank.projector("tuned") is not None and bank.projector("plain") is None and bank.projector(None) is None
    px = synthetic.make_pixels(cfg, 1, 11).to(torch.bfloat16)
    ids = synthetic.make_prompt(cfg, 12, 1, 11)[None]
    media = {"image": [px[0].cuda()]}
    base, _, _ = model._embed(ids, media)
    under, _, _ = model._embed(ids, media, adapter="tuned", adapters=bank)
    plain, _, _ = model._embed(ids, media, adapter="plain", adapters=bank)
    other = build_model(cfg, seed=21)                                  # the same model with its projector overwritten
    with torch.no_grad():
        for n, p in other.mm_projector.named_parameters():
            p.copy_(tuned["mm_projector." + n])
    other.mm_projector._invalidate()
    want, _, _ = other._embed(ids, media)
    assert_bits_equal(under[0], want[0], "_embed under the adapter vs a model whose projector was overwritten")
    assert_bits_equal(plain[0], base[0], "_embed under an adapter without a tuned projector vs the base model")
    assert not torch.equal(under, base), "the tuned projector changed nothing: the test shows nothing"
    after, _, _ = model._embed(ids, media)
    assert_bits_equal(after[0], base[0], "the base model's _embed after a call under the adapter")
    bad = str(tmp_path / "tower")
    lora.save_adapter(ad, bad, non_lora={"vision_tower." + next(iter(dict(model.vision_tower.named_parameters()))): torch.zeros(2)})
    with pytest.raises(ValueError, match="vision_tower tensors outside the adapters"):
        AdapterBank(model, capacity=1, r=16).load("tower", bad)
