"""The batch-1 decode GEMVs as ONE block of 8..16 waves per CU (activation staged once per CU) and the greedy pick fused into lm_head + one
final launch: the shapes at which the wide block can go wrong.

GEMV tolerances are those of tests/test_gpu_ops.py against the same fp32 torch expressions: 1e-4 fp32 out, 4e-3 bias + residual, 2e-3 normed,
8e-3 gate/up.  Row counts come from the device's CU count C, as the kernels take it:
  N = 8C + 2 -> 4C + 1 row pairs: the CU map with 8 waves per block, 4 pairs on most CUs and 5 on one (waves without work, one wave with two)
  N = 8C + 3 -> 4C + 2 pairs, the last pair holds ONE row
  N = 4C + 1 -> 2C + 1 pairs: the small-grid path (256-thread blocks, plain walk), odd N
K = 3584 (448 16-byte chunks: fewer than threads), 8200 (1025: the first size past the single-pass norm, ragged by one), 18944 (2368: three
ragged passes of 1024 threads)."""
import functools

import pytest
import torch

from tests.gpu_util import margin_aware_ids, randn_bf16, rel_l2
from vila_amd import configs, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from vila_amd import ops as _ops
    return _ops


def _cus() -> int:
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@functools.lru_cache(maxsize=None)
def _operands(K):
    """x, gain, the widest weight / bias / residual of a K (rows are sliced per case) and the fp32 references, computed once per K."""
    n_max = 8 * _cus() + 3
    x = randn_bf16(K, seed=127)
    w = randn_bf16(n_max, K, seed=128, scale=K ** -0.5)
    b = randn_bf16(n_max, seed=129)
    r = randn_bf16(n_max, seed=130)
    g = randn_bf16(K, seed=131, scale=0.1) + 1
    x32 = x.float()
    xn = (g * (x32 * torch.rsqrt(x32.pow(2).mean() + 1e-6)).to(torch.bfloat16)).float()
    return x, w, b, r, g, w.float() @ x32, w.float() @ xn


@pytest.mark.parametrize("K", [3584, 8200, 18944])
@pytest.mark.parametrize("n_of", ["8C+2", "8C+3", "4C+1"])
def test_gemv_wide_block_shapes(ops, n_of, K):
    C = _cus()
    N = {"8C+2": 8 * C + 2, "8C+3": 8 * C + 3, "4C+1": 4 * C + 1}[n_of]
    x, w, b, r, g, ref, ref_n = _operands(K)
    w, b, r, ref, ref_n = w[:N], b[:N].contiguous(), r[:N].contiguous(), ref[:N], ref_n[:N]
    out = ops.gemv(x, w, out_f32=True)
    e = rel_l2(out, ref)
    print(f"N={N} K={K} plain f32 rel={e:.3e}")
    assert e < 1e-4, f"f32 rel={e:.3e}"
    out = ops.gemv(x, w, bias=b, residual=r)
    ref2 = (ref + b.float()).to(torch.bfloat16).float() + r.float()
    e = rel_l2(out, ref2)
    print(f"N={N} K={K} bias+res rel={e:.3e}")
    assert e < 4e-3, f"bias+res rel={e:.3e}"
    out = ops.gemv(x, w, norm_w=g, eps=1e-6, out_f32=True)
    e = rel_l2(out, ref_n)
    print(f"N={N} K={K} normed rel={e:.3e}")
    assert e < 2e-3, f"norm rel={e:.3e}"


def test_gemv_gateup_odd_group_count(ops):
    K, N = 512, 8 * _cus() + 2
    x = randn_bf16(K, seed=132)
    wg, wu = randn_bf16(N, K, seed=133, scale=K ** -0.5), randn_bf16(N, K, seed=134, scale=K ** -0.5)
    g = randn_bf16(K, seed=135, scale=0.1) + 1
    ref = torch.nn.functional.silu(wg.float() @ x.float()) * (wu.float() @ x.float())
    out = ops.gemv(x, wg, w2=wu)
    assert rel_l2(out, ref) < 8e-3, f"rel={rel_l2(out, ref):.3e}"
    x32 = x.float()
    xn = (g * (x32 * torch.rsqrt(x32.pow(2).mean() + 1e-6)).to(torch.bfloat16)).float()
    ref = torch.nn.functional.silu(wg.float() @ xn) * (wu.float() @ xn)
    out = ops.gemv(x, wg, w2=wu, norm_w=g, eps=1e-6)
    assert rel_l2(out, ref) < 8e-3, f"normed rel={rel_l2(out, ref):.3e}"


# ---------------------------------------------------------------------------------------------------------------------
# attention-merge staging (o_proj reads the decode attention's 256-key partials): one slice, a slice boundary, two slices
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_model():
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 0).items()}
    return cfg, w, build_model(cfg, weights=w)


@pytest.mark.parametrize("S", [255, 256, 257])
def test_attention_merge_at_the_slice_boundary_vs_oracle(tiny_model, S):
    """First decoded position S = 255 / 256 / 257: the merge in the o_proj prologue sees one slice, the first key of the second slice, two slices."""
    from oracle import vila_oracle as O
    cfg, w, model = tiny_model
    g = torch.Generator().manual_seed(40 + S)
    e = (torch.randn(1, S, cfg.llm.hidden_size, generator=g) * 0.5).to(torch.bfloat16)
    n = 4
    ids_o, lg_o = O.greedy_generate(e.float(), w, cfg, n, stop_at_eos=False)
    _, lg = model.llm.generate(inputs_embeds=e.cuda(), max_new_tokens=n, return_logits=True, forced_ids=ids_o, use_graph=False)
    assert rel_l2(lg, lg_o) < 3e-2, f"logits rel={rel_l2(lg, lg_o):.3e}"
    free = model.llm.generate(inputs_embeds=e.cuda(), max_new_tokens=n, use_graph=True, eos_token_id=-1)
    margin_aware_ids(lg, lg_o, ids_o, free_ids=free[0])


# ---------------------------------------------------------------------------------------------------------------------
# the greedy pick inside lm_head + the final pick / advance launch
# ---------------------------------------------------------------------------------------------------------------------
def _block_of_row(n_rows: int, C: int):
    """Block that computes each lm_head row: the mirror of launch_gemv's grid (gemv.hip balanced_grid) and the kernel's walk — small grids: block b
    takes row pairs 4b..4b+3, then + 4 x grid; CU map (gemv_common.h CuMap, skew 0): pair g belongs to CU g % C."""
    n_groups = (n_rows + 1) // 2
    want = (n_groups + 3) // 4
    blk = []
    for row in range(n_rows):
        g = row // 2
        if want <= C:
            blk.append((g // 4) % want)
        elif C % 8 == 0 and g >= (n_groups // C) * C:          # the remainder goes to the even CUs in rank order
            r = (g - (n_groups // C) * C) % (C // 2)
            blk.append((r // 4) * 8 + (r % 4) * 2)
        else:
            blk.append(g % C)
    return blk, (want if want <= C else C)


def _step_once(model, e, token):
    """prefill e, then ONE greedy decode step fed `token`: returns the step's state (token, logits, out_ids, n_out, pos)."""
    model.llm.generate(inputs_embeds=e, max_new_tokens=2, forced_ids=torch.tensor([token]), use_graph=False, eos_token_id=-1)
    return model.llm._decode


@pytest.mark.parametrize("vocab_of", ["1000", "8C+6"])
def test_fused_pick_ties_go_to_the_lower_index(vocab_of):
    """Two identical lm_head rows carrying the maximum, the first computed by the first block and the second by the last block, then both inside
    one wave's row pair: the step returns the lower index and the logits hold equal values at both.  vocab 1000: the small-grid walk;
    8C + 6: the CU map with 8 waves per block."""
    from vila_amd.vlm import build_model
    C = _cus()
    cfg = configs.tiny("mlp_downsample")
    V = 1000 if vocab_of == "1000" else 8 * C + 6
    cfg.llm.vocab_size = V
    model = build_model(cfg, seed=9)
    head = model.llm.lm_head.weight
    g = torch.Generator().manual_seed(41)
    e = (torch.randn(1, 20, cfg.llm.hidden_size, generator=g) * 0.5).to(torch.bfloat16).cuda()
    st = _step_once(model, e, 7)
    top = int(torch.argmax(st.logits))
    assert int(st.token) == top and float(st.logits[top]) > 0
    blk, grid = _block_of_row(V, C)
    first = min(i for i in range(V) if blk[i] == 0)
    last = max(i for i in range(V) if blk[i] == grid - 1)
    assert first < last and blk[first] != blk[last]
    pair = 2 * (V // 4)                                          # rows 2g, 2g + 1 of one wave
    orig = head.data.clone()
    for lo, hi in ((first, last), (pair, pair + 1)):
        head.data.copy_(orig)
        row = orig[top] * 4                                      # exact in bf16: 4 x the maximum logit, bit-equal at both rows
        head.data[lo] = row
        head.data[hi] = row
        st = _step_once(model, e, 7)
        assert float(st.logits[lo]) == float(st.logits[hi]) == float(st.logits.max()), (lo, hi)
        assert int(st.token) == lo, f"rows {lo} and {hi} tie: the step picked {int(st.token)}"
        assert int(st.out_ids[0]) == lo and int(st.n_out) == 1 and int(st.pos) == 21


def test_fused_pick_follows_argmax_and_advances_the_state(ops):
    """20 greedy steps of a plain tiny model: every step's token is torch.argmax of its logits; out_ids / n_out / pos advance as the separate
    advance launch did, and nothing is written once n_out >= max_out."""
    from vila_amd import _lib
    from vila_amd.vlm import build_model
    import ctypes as C
    cfg = configs.tiny("mlp_downsample")
    model = build_model(cfg, seed=10)
    llm = model.llm
    g = torch.Generator().manual_seed(42)
    S, n = 24, 21
    e = (torch.randn(1, S, cfg.llm.hidden_size, generator=g) * 0.5).to(torch.bfloat16).cuda()
    llm.generate(inputs_embeds=e, max_new_tokens=n, use_graph=False, eos_token_id=-1)       # opens the cache and the session (max_out = 21)
    st, cache = llm._decode, llm._decode.cache
    first = 5
    st.pos.fill_(S); st.n_out.zero_(); st.token.fill_(first); st.out_ids.fill_(-1)
    got = []
    for t in range(20):
        llm.decode_step(cache, st)
        assert int(st.token) == int(torch.argmax(st.logits)), f"step {t}"
        got.append(int(st.token))
        assert int(st.n_out) == t + 1 and int(st.pos) == S + t + 1
    assert st.out_ids[:20].tolist() == got and int(st.out_ids[20]) == -1
    # a full output buffer: the counters still advance, no id is written
    st.n_out.fill_(n)
    keep = st.out_ids.clone()
    llm.decode_step(cache, st)
    assert int(st.n_out) == n + 1 and int(st.pos) == S + 21 and torch.equal(st.out_ids, keep)
    assert int(st.token) == int(torch.argmax(st.logits))
    lib = _lib.load()
    assert lib.vila_llm_decode_launches(C.byref(llm._struct().shape), cache.max_ctx) == 1 + 5 * cfg.llm.num_hidden_layers + 2


    # a NaN logit never wins, in the step's pick as in ops.argmax (which keeps its two stages)
    llm.lm_head.weight.data[3] = float("nan")
    llm.decode_step(cache, st)
    assert bool(torch.isnan(st.logits[3])) and int(torch.isnan(st.logits).sum()) == 1
    assert int(st.token) == int(ops.argmax(st.logits)) != 3


def test_argmax_keeps_its_non_finite_rules(ops):
    """-inf rows give their lowest index, a NaN is skipped."""
    x = torch.full((5000,), float("-inf"), device="cuda")
    assert int(ops.argmax(x)) == 0
    x[17] = float("nan"); x[4000] = -3.0
    assert int(ops.argmax(x)) == 4000
