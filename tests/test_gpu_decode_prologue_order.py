"""The batch-1 decode kernels request their prologue's inputs before they know the position (the ordering rule): the first K/V
chunk of `attn_decode_head` is bounded by the cache's capacity, the o_proj merge prologue fetches the partial slots of every slice of the
capacity, and down_proj stages all of x in one pass in front of its first weight batch.  What that can break is that a value loaded before the
position was known reaches a result, so:

* stale K/V rows: every cache row past `pos` set to NaN, and to +inf, must give the output that zeros there give, bit for bit, and finite;
* stale partial slots: a decode step on a workspace of zeros and on one of 0xFF bytes (fp32 NaN) must give the same logits, bit for bit, and so
  must attention + o_proj at the step's own shape (28 heads, N = 8 CUs + 2: the CU map's 512-thread merge) through the C entry point;
* down_proj's staging: K = 18944 (2368 chunks, 5 per thread of a 512-thread block with the last pass ragged) and K = 18952 (2369: one chunk more
  than a multiple of 64) without a norm, with a residual, against the fp32 product at the bias + residual tolerance of tests/test_gpu_ops.py
  (4e-3: one bf16 rounding of the output); N = 8 CUs + 2 takes the CU map (512-thread blocks), N = 1000 the small grid (256-thread blocks, two
  staging passes), and a row both compute must come out bit-equal.

No case reads outside a buffer: positions stay below the capacity, as `ops.attn_decode` demands."""
import functools

import pytest
import torch

from tests.gpu_util import randn_bf16, rel_l2
from vila_amd import configs, synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from vila_amd import ops as _ops
    return _ops


def _cus() -> int:
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# stale K/V rows
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _qkv(nq, nkv, cap):
    return randn_bf16(nq, 128, seed=301), randn_bf16(nkv, cap, 128, seed=302 + cap), randn_bf16(nkv, cap, 128, seed=303 + cap)


@functools.lru_cache(maxsize=None)
def _oproj(nq, wide):
    """o_proj weight and residual: 8 CUs + 2 rows take the CU map (512-thread blocks), 40 rows the small grid (256-thread blocks)."""
    N = 8 * _cus() + 2 if wide else 40
    return randn_bf16(N, nq * 128, seed=304, scale=(nq * 128) ** -0.5), randn_bf16(N, seed=305)


@pytest.mark.parametrize("cap", [300, 512, 1024])
@pytest.mark.parametrize("G,nkv", [(7, 4), (7, 1), (1, 4), (1, 1)])
@pytest.mark.parametrize("form", ["head", "slices256"])
def test_rows_past_the_position_never_reach_the_output(ops, form, G, nkv, cap):
    nq = G * nkv
    q, k, v = _qkv(nq, nkv, cap)
    kw = {}
    if form == "slices256":
        w, r = _oproj(nq, G == 7 and nkv == 4)
        kw = dict(w=w, residual=r)
    for p in sorted({0, 15, 16, 255, 256, 257, cap - 1}):
        pos = torch.tensor([p], dtype=torch.int32, device="cuda")
        outs = {}
        for name, fill in (("zero", 0.0), ("nan", float("nan")), ("inf", float("inf"))):
            kk, vv = k.clone(), v.clone()
            kk[:, p + 1:] = fill
            vv[:, p + 1:] = fill
            outs[name] = ops.attn_decode(q, kk, vv, pos, form=form, **kw)
        assert bool(torch.isfinite(outs["zero"].float()).all()), f"pos {p}: the output over zeroed rows is not finite"
        for name in ("nan", "inf"):
            assert bool(torch.isfinite(outs[name].float()).all()), f"pos {p}: {name} rows past the position reached the output"
            assert torch.equal(_bits(outs[name]), _bits(outs["zero"])), f"pos {p}: {name} rows past the position changed the output"


# ---------------------------------------------------------------------------------------------------------------------
# stale partial slots
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_llm():
    from vila_amd.vlm import build_model
    cfg = configs.tiny("mlp_downsample")                          # head_dim 128, 4 query heads on 2 kv heads
    w = {k: v.to(torch.bfloat16).float() for k, v in synthetic.make_weights(cfg, 0).items()}
    return build_model(cfg, weights=w).llm


@pytest.mark.parametrize("S", [10, 300])
def test_step_does_not_depend_on_what_the_workspace_held(ops, tiny_llm, S):
    """A cache of 1024 positions has four partial slots per head; at position 10 one is written, at 300 two.  The o_proj prologue fetches all four."""
    llm = tiny_llm
    ids = torch.randint(0, 900, (S,), generator=torch.Generator().manual_seed(500 + S))
    cache = llm.new_cache(1024)
    _, cache, r, _ = llm._prefill_one(llm.embed_tokens(ids[None].cuda()), None, 2, cache)
    first = ops.argmax(r.last_logits[0])
    st = llm._decode_session(cache, 2)
    got = {}
    for name, byte in (("zeros", 0), ("0xFF", 0xFF)):
        st.ws.fill_(byte)
        st.pos.fill_(S); st.n_out.zero_(); st.token.copy_(first)
        llm.decode_step(cache, st)
        torch.cuda.synchronize()
        assert int(st.pos) == S + 1
        got[name] = (st.logits.clone(), int(st.token))
    for name, (lg, _) in got.items():
        assert bool(torch.isfinite(lg).all()), f"position {S}, workspace of {name}: logits not finite"
    assert torch.equal(_bits(got["0xFF"][0]), _bits(got["zeros"][0])), f"position {S}: the logits depend on what the workspace held"
    assert got["0xFF"][1] == got["zeros"][1]


@pytest.mark.parametrize("p", [10, 300, 1023])
def test_cu_map_merge_does_not_depend_on_what_the_workspace_held(ops, p):
    """The step's own shape of the merge: 28 heads, N = 8 CUs + 2 rows (the CU map, 512-thread blocks: every chunk of the partials is requested up
    front), a cache of 1024 positions (four slots; one, two and four of them live).  `ops.attn_decode` brings its own workspace, so this goes
    through the same C entry point on a workspace filled beforehand."""
    from vila_amd import _lib
    from vila_amd.ops import check, _stream
    lib = _lib.load()
    nq, nkv, cap = 28, 4, 1024
    q, k, v = _qkv(nq, nkv, cap)
    w, r = _oproj(nq, True)
    N = w.shape[0]
    pos = torch.tensor([p], dtype=torch.int32, device="cuda")
    ws = torch.empty((lib.vila_attn_decode_workspace_bytes(nq, cap),), device="cuda", dtype=torch.uint8)
    got = {}
    for name, byte in (("zeros", 0), ("0xFF", 0xFF)):
        ws.fill_(byte)
        y = torch.empty((N,), device="cuda", dtype=torch.bfloat16)
        check(lib.vila_attn_decode_oproj_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), pos.data_ptr(), w.data_ptr(), r.data_ptr(), y.data_ptr(), N,
                                              nq, nkv, cap, 128 ** -0.5, ws.data_ptr(), ws.numel(), _stream()), "attn_decode_oproj")
        got[name] = y
    assert bool(torch.isfinite(got["0xFF"].float()).all()), f"pos {p}: stale partial slots reached the output"
    assert torch.equal(_bits(got["0xFF"]), _bits(got["zeros"])), f"pos {p}: the output depends on what the workspace held"
    assert torch.equal(_bits(got["zeros"]), _bits(ops.attn_decode(q, k, v, pos, form="slices256", w=w, residual=r)))


# ---------------------------------------------------------------------------------------------------------------------
# down_proj's single-pass staging
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [18944, 18952])
def test_down_proj_staging_without_norm(ops, K):
    big, small = 8 * _cus() + 2, 1000
    assert big > small
    x = randn_bf16(K, seed=311)
    w = randn_bf16(big, K, seed=312, scale=K ** -0.5)
    r = randn_bf16(big, seed=313)
    ref = (w.float() @ x.float()).to(torch.bfloat16).float() + r.float()
    out_big = ops.gemv(x, w, residual=r)
    out_small = ops.gemv(x, w[:small], residual=r[:small].contiguous())
    for name, out, n in (("8 CUs + 2", out_big, big), ("1000", out_small, small)):
        e = rel_l2(out, ref[:n])
        print(f"K={K} N={name}: rel={e:.3e}")
        assert e < 4e-3, f"K={K} N={name}: rel={e:.3e}"
    assert torch.equal(_bits(out_big[:small]), _bits(out_small)), f"K={K}: rows differ between the CU-map grid and the small grid"
