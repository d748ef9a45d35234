"""The prefill / SFT attention element by element: every form of the forward (vila_attn_force_fwd: A / B / C / D / v1), both backward
implementations (vila_attn_force_bwd: v1 / DMA, and both dK / dV variants of v1) and the append prefill (forms A - D) against fp64 references
with the derived per-element bounds of tests/gpu_util.py (attn_fwd_bounds, attn_bwd_bounds; tests/test_attn_bound_cpu.py proves them on the
CPU at this file's shapes and inputs).

  - Every output (o, lse, delta, dq, dk, dv) sits in its own frame holding a NaN bit pattern: an element never written fails as non-finite, a
    write outside the view fails the frame.  q / k / v / do / o are views of NaN-padded buffers with NaN guard rows: a read past the tensor that
    reaches a result shows there.
  - The backward is judged on its own: it is given o = bf16(reference o) and lse = fp32(reference lse); one case per implementation runs end to
    end from the project's forward against a bound that carries the forward's own o and lse bounds through delta and P.
  - Planted pairs (gpu_util.plant_pairs): with random keys one key of L carries 1 / L of a row, so a key lost or admitted at a tile seam, the
    odd / even split, the causal diagonal or the end of a sequence hides inside any bound; a planted key carries about half of its row's weight
    (asserted from the reference, 0.3 .. 0.7), so the pair moves o by O(|v|), dv by O(|do|) and dq / dk by O(1).
No tolerance here is a measured number; the measured worst err / bound per output are printed (and, with VILA_DUMP_PROBE=<file>, appended as
JSON lines) and recorded in CHANGELOG.md."""
import contextlib
import functools
import json
import os

import pytest
import torch

from tests.gpu_util import (_int_view, _pattern_of, assert_elementwise, attn_bwd_bounds, attn_fwd_bounds, framed_flat, framed_thd,
                            framed_thd_operand, plant_pairs, randn_bf16)
from tests.test_gpu_attention_forms import FORMS, VARLEN

pytestmark = pytest.mark.gpu

IMPLS = {1: "v1", 2: "dma"}
VARLEN_513 = VARLEN + [513]                 # + two 256-row blocks and one row, nine key tiles (an odd number)
UNIFORM = (2, 203)                          # n_seq x max_seqlen without cu_seqlens: 203 is a multiple of no block height (16 .. 256)
DIMS = (64, 72, 128)
HEADS = ((2, 2), (14, 2))                   # GQA 1:1 and 7:1
STRESS_T = 300
STRESS_HEADS = (4, 2)
STRESS_CU = [0, 65, 165, 300]
PLANT_LENS = [513, 300, 65]
PLANT_HEADS = {64: (14, 2), 72: (2, 2), 128: (14, 2)}
APPEND = (150, 101, 320)                    # T, past (no multiple of 64), max_ctx
# (row, key) token pairs of the planted sets over PLANT_LENS (sequences at 0, 513, 813).  Rows of the first sequence: both sides of every wave and
# block edge (16 / 32 rows per wave, 64 / 128 / 256-row blocks, the backward's 32-row query tiles, 64- and 128-row dQ blocks) and its last rows.
_ROWS = (15, 16, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512)
PLANT_SETS = {
    # the row's own key (the causal diagonal) / the key before it; the last row of every sequence with the last key
    "diag": [(r, r) for r in _ROWS] + [(514, 514), (812, 812), (877, 877)],
    "prev": [(r, r - 1) for r in _ROWS] + [(812, 811), (877, 876)],
    # first and last key of even tiles (0, 2, 4) and of odd tiles (1, 3), below the diagonal
    "tiles": [(63, 0), (64, 63), (127, 64), (128, 127), (255, 128), (256, 191), (511, 192), (512, 255), (812, 769), (641, 640), (877, 876)],
    # non-causal: the last key of every sequence (read by its first row), first and last keys of even and odd tiles above the diagonal
    "edges": [(0, 512), (15, 0), (16, 63), (31, 64), (32, 127), (63, 128), (64, 191), (127, 448), (128, 447), (255, 511), (256, 192), (511, 255),
              (512, 384), (513, 812), (812, 769), (641, 640), (813, 877), (877, 876)],
}
PLANT_FOR = {True: ("diag", "prev", "tiles"), False: ("edges", "diag")}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from vila_amd import _lib
    return _lib.load()


@contextlib.contextmanager
def _forced(lib, fwd=0, bwd=0, append=0):
    lib.vila_attn_force_fwd(fwd)
    lib.vila_attn_force_bwd(bwd)
    lib.vila_attn_force_append(append)
    try:
        yield
    finally:
        lib.vila_attn_force_fwd(0)
        lib.vila_attn_force_bwd(0)
        lib.vila_attn_force_append(0)


def _dump(case, **figures):
    print(f"{case}: " + ", ".join(f"{k} {v:.3f}" for k, v in figures.items()))
    path = os.environ.get("VILA_DUMP_PROBE")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": case, **figures}) + "\n")


# ---- shapes and inputs (tests/test_attn_bound_cpu.py builds the same on the CPU) -------------------------------------------------------------------
def qkv_inputs(T, Hq, Hkv, D, seed, q_scale=1.0, device="cuda"):
    """q / k / v [T, H, D] bf16 drawn as test_gpu_attention_forms._qkv draws them (one fused buffer, q scaled afterwards)."""
    qkv = randn_bf16(T, (Hq + 2 * Hkv) * D, seed=seed, device=device)
    q = qkv[:, : Hq * D].view(T, Hq, D)
    if q_scale != 1.0:
        q.copy_((q.float() * q_scale).to(torch.bfloat16))
    return q, qkv[:, Hq * D:(Hq + Hkv) * D].view(T, Hkv, D), qkv[:, (Hq + Hkv) * D:].view(T, Hkv, D)


def cu_of(lens, device="cuda"):
    return torch.tensor([0] + torch.tensor(list(lens)).cumsum(0).tolist(), dtype=torch.int32, device=device)


def attn_case(kind, D, causal, heads, device="cuda"):
    """One problem -> dict: q / k / v / do, cu (the reference's sequences), kcu / max_seqlen / n_seq (what the kernel is told), scale, and for a
    planted kind the weights the planted keys reached.  Kinds: "varlen", "uniform", "scale" (one sequence of 257, scale 0.25), the stresses
    "jump" / "vjump" / "large" / "zero" of test_every_form_survives_softmax_stress, "plant:<set>"."""
    Hq, Hkv = heads
    c = {"kind": kind, "D": D, "causal": causal, "heads": heads, "scale": None, "weights": None}
    if kind == "varlen":
        c["cu"] = c["kcu"] = cu_of(VARLEN_513, device)
        T, c["max_seqlen"], c["n_seq"], seed = sum(VARLEN_513), max(VARLEN_513), len(VARLEN_513), 1100 + D
    elif kind == "uniform":
        n, S = UNIFORM
        T, c["max_seqlen"], c["n_seq"], seed = n * S, S, n, 1200 + D
        c["cu"], c["kcu"] = cu_of([S] * n, device), None
    elif kind == "scale":
        T, c["max_seqlen"], c["n_seq"], seed, c["scale"] = 257, 257, 1, 1300 + D, 0.25
        c["cu"], c["kcu"] = cu_of([257], device), None
    elif kind in ("jump", "vjump", "large", "zero"):
        T, seed = STRESS_T, {"jump": 400, "vjump": 400, "large": 401, "zero": 402}[kind]
        lens = [b - a for a, b in zip(STRESS_CU[:-1], STRESS_CU[1:])] if kind == "vjump" else [T]
        c["cu"] = cu_of(lens, device)
        c["kcu"], c["max_seqlen"], c["n_seq"] = (c["cu"], max(lens), len(lens)) if kind == "vjump" else (None, T, 1)
    else:
        assert kind.startswith("plant:"), kind
        c["cu"] = c["kcu"] = cu_of(PLANT_LENS, device)
        T, c["max_seqlen"], c["n_seq"], seed = sum(PLANT_LENS), max(PLANT_LENS), len(PLANT_LENS), 1400 + D
    q, k, v = qkv_inputs(T, Hq, Hkv, D, seed, q_scale=27.0 if kind == "large" else 1.0, device="cpu")
    if kind in ("jump", "vjump"):
        G = Hq // Hkv
        for qi, kj, f in ((120, 100, 1.5), (250, 200, 1.5), (290, 280, 2.0), (299, 193, 1.5), (70, 66, -2.0)):
            k[kj] = (q[qi, ::G].float() * f).to(torch.bfloat16)         # kv head g spikes against the first q head of its group
    if kind == "zero":
        q.zero_()
    if kind.startswith("plant:"):
        c["weights"] = plant_pairs(q, k, PLANT_SETS[kind[6:]], causal, cu_of(PLANT_LENS, "cpu"))
    c["q"], c["k"], c["v"] = (t.to(device) for t in (q, k, v))
    c["do"] = randn_bf16(T, Hq, D, seed=seed + 1, device=device)
    return c


def fwd_bounds_of(c):
    if "fwd" not in c:
        c["fwd"] = attn_fwd_bounds(c["q"], c["k"], c["v"], c["causal"], c["cu"], c["scale"])
    return c["fwd"]


def bwd_inputs_of(c):
    """What the backward is given when it is judged alone: o = bf16(reference o), lse = fp32(reference lse)."""
    f = fwd_bounds_of(c)
    return f["o"][0].to(torch.bfloat16), f["lse"][0].float()


def bwd_bounds_of(c):
    if "bwd" not in c:
        o_bf, lse32 = bwd_inputs_of(c)
        c["bwd"] = attn_bwd_bounds(c["q"], c["k"], c["v"], c["do"], o_bf, lse32, c["causal"], c["cu"], c["scale"])
    return c["bwd"]


def assert_planted(c):
    """Every planted key carries 0.3 .. 0.7 of its target row by the fp64 reference: no case silently degenerates."""
    w = c["weights"]
    assert w is not None and w.numel() > 0 and bool(((w >= 0.3) & (w <= 0.7)).all()), f"{c['kind']}: planted weights {w.min():.3f} .. {w.max():.3f}"


def v1_dkv_blocks(c):
    """Blocks of the v1 dK / dV launch (attn_bwd.hip:460-462): at most 320 take the two-group kernel (NG = 2), more the one-group kernel."""
    return -(-c["max_seqlen"] // 64) * c["heads"][1] * c["n_seq"]


@functools.lru_cache(maxsize=2)
def _case(kind, D, causal, heads):
    return attn_case(kind, D, causal, heads, "cuda")


# ---- framed launches --------------------------------------------------------------------------------------------------------------------------------
def _operands(c):
    if "framed" not in c:
        o_bf, lse32 = bwd_inputs_of(c)
        c["framed"] = {n: framed_thd_operand(t) for n, t in (("q", c["q"]), ("k", c["k"]), ("v", c["v"]), ("do", c["do"]), ("o", o_bf))}
        c["framed"]["lse"] = lse32.contiguous()
    return c["framed"]


def _frames(c, names):
    T, (Hq, Hkv), D = c["q"].shape[0], c["heads"], c["D"]
    out, checks = {}, {}
    for n in names:
        if n in ("lse", "delta"):
            flat, checks[n] = framed_flat(Hq * T, dtype=torch.float32)
            out[n] = flat.view(Hq, T)
        else:
            out[n], checks[n] = framed_thd(T, Hq if n in ("o", "dq") else Hkv, D)
    return out, checks


def _untouched(t):
    return bool((_int_view(t.contiguous()) == _pattern_of(t)).all())


def run_fwd(lib, c, form):
    from vila_amd import _lib
    from vila_amd.ops import _p, _stream
    f = _operands(c)
    q, k, v = f["q"], f["k"], f["v"]
    T, Hq, D = q.shape
    out, checks = _frames(c, ("o", "lse"))
    o, lse = out["o"], out["lse"]
    scale = float(c["scale"] if c["scale"] is not None else D ** -0.5)
    with _forced(lib, fwd=form):
        _lib.check(lib.vila_attn_fwd_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), q.stride(0), k.stride(0), v.stride(0), o.stride(0),
                                          q.stride(1), k.stride(1), v.stride(1), o.stride(1), _p(c["kcu"]), c["n_seq"], T, int(c["max_seqlen"]), Hq,
                                          k.shape[1], D, int(c["causal"]), scale, lse.data_ptr(), _stream()), "attn_fwd")
    return out, checks


def run_bwd(lib, c, impl, o=None, lse=None, parts=7, into=None):
    from vila_amd import ops
    f = _operands(c)
    out, checks = into if into is not None else _frames(c, ("delta", "dq", "dk", "dv"))
    kw = dict(cu_seqlens=c["kcu"], max_seqlen=c["max_seqlen"]) if c["kcu"] is not None else dict(n_seq=c["n_seq"])
    with _forced(lib, bwd=impl):
        ops.attn_bwd(f["q"], f["k"], f["v"], f["o"] if o is None else o, f["do"], f["lse"] if lse is None else lse, c["causal"], out["dq"], out["dk"],
                     out["dv"], scale=c["scale"], parts=parts, delta=out["delta"], **kw)
    return out, checks


def judge(tag, out, checks, bounds, names):
    """assert_elementwise on every named output ([T, H, D] as [T, H * D]: a failure names (token, head * D + d); lse / delta as [head, token]),
    then every frame.  -> {name: worst err / bound}."""
    worst = {}
    for n in names:
        ref, bound, _ = bounds[n]
        got = out[n]
        if got.dim() == 3:
            got, ref, bound = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1), bound.reshape(bound.shape[0], -1)
        worst[n] = assert_elementwise(got, ref, bound, f"{tag} {n}")
    for n in names:
        checks[n]()
    return worst


def _tag(c):
    return f"{c['kind']} D={c['D']} causal={c['causal']} heads={c['heads']}"


# ---- forward ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", HEADS, ids=["gqa1", "gqa7"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("kind", ["varlen", "uniform", "scale"])
def test_forward_every_form_every_element(lib, kind, D, causal, heads):
    c = _case(kind, D, causal, heads)
    worst = {}
    for form, name in sorted(FORMS.items()):
        out, checks = run_fwd(lib, c, form)
        for n, w in judge(f"form {name} {_tag(c)}", out, checks, fwd_bounds_of(c), ("o", "lse")).items():
            worst[f"{n}_{name}"] = w
    _dump(f"forward {_tag(c)}", **worst)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("kind", ["jump", "vjump", "large", "zero"])
def test_forward_softmax_stress_every_element(lib, kind, causal):
    """Running-max jumps in both key groups, rows whose odd-tile key group is empty, scores of about +-80, uniform scores (q = 0)."""
    c = _case(kind, 128, causal, STRESS_HEADS)
    if kind == "large":
        assert float(fwd_bounds_of(c)["lse"][0].abs().max()) > 60, "the large-logit case lost its range"
    worst = {}
    for form, name in sorted(FORMS.items()):
        out, checks = run_fwd(lib, c, form)
        for n, w in judge(f"form {name} {_tag(c)}", out, checks, fwd_bounds_of(c), ("o", "lse")).items():
            worst[f"{n}_{name}"] = w
    _dump(f"forward stress {_tag(c)}", **worst)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", DIMS)
def test_forward_planted_pairs_every_form(lib, D, causal):
    worst = {}
    for which in PLANT_FOR[causal]:
        c = _case("plant:" + which, D, causal, PLANT_HEADS[D])
        assert_planted(c)
        for form, name in sorted(FORMS.items()):
            out, checks = run_fwd(lib, c, form)
            for n, w in judge(f"form {name} {_tag(c)}", out, checks, fwd_bounds_of(c), ("o", "lse")).items():
                worst[f"{n}_{name}"] = max(w, worst.get(f"{n}_{name}", 0.0))
    _dump(f"forward planted D={D} causal={causal}", **worst)


# ---- backward -----------------------------------------------------------------------------------------------------------------------------------------
GRADS = ("delta", "dq", "dk", "dv")


def _bwd_both(lib, c, worst):
    for impl, name in IMPLS.items():
        out, checks = run_bwd(lib, c, impl)
        for n, w in judge(f"impl {name} {_tag(c)}", out, checks, bwd_bounds_of(c), GRADS).items():
            worst[f"{n}_{name}"] = max(w, worst.get(f"{n}_{name}", 0.0))


@pytest.mark.parametrize("heads", HEADS, ids=["gqa1", "gqa7"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("kind", ["varlen", "uniform"])
def test_backward_alone_every_element(lib, kind, D, causal, heads):
    """o = bf16(reference o) and lse = fp32(reference lse) go in: the backward's arithmetic alone.  The varlen batch launches v1's one-group
    dK / dV kernel (more than 320 blocks), the uniform batch the two-group kernel."""
    c = _case(kind, D, causal, heads)
    assert (v1_dkv_blocks(c) > 320) == (kind == "varlen"), v1_dkv_blocks(c)
    worst = {}
    _bwd_both(lib, c, worst)
    _dump(f"backward {_tag(c)}", **worst)


@pytest.mark.parametrize("causal", [False, True])
def test_backward_large_logits_every_element(lib, causal):
    c = _case("large", 128, causal, STRESS_HEADS)
    worst = {}
    _bwd_both(lib, c, worst)
    _dump(f"backward {_tag(c)}", **worst)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", DIMS)
def test_backward_planted_pairs(lib, D, causal):
    """The pairs sit at the seams of the backward's own tiling: 64- and 128-row dQ blocks, 64-key dK / dV blocks, the 32-row query tiles of v1 (the
    64-row ones of DMA), the last query row and the last key of a sequence.  These batches take v1's two-group dK / dV kernel."""
    worst = {}
    for which in PLANT_FOR[causal]:
        c = _case("plant:" + which, D, causal, PLANT_HEADS[D])
        assert_planted(c)
        assert v1_dkv_blocks(c) <= 320
        _bwd_both(lib, c, worst)
    _dump(f"backward planted D={D} causal={causal}", **worst)


@pytest.mark.parametrize("impl", sorted(IMPLS), ids=list(IMPLS.values()))
def test_backward_parts_into_frames(lib, impl):
    """parts 1 (delta), 4 (dK / dV) and 2 (dQ) launched one by one: each writes its own outputs and leaves the others' frames AND views untouched;
    the result is judged per element and equals parts = 7 bit for bit."""
    c = _case("varlen", 128, True, (14, 2))
    whole, wchecks = run_bwd(lib, c, impl)
    into = _frames(c, GRADS)
    out, checks = into
    run_bwd(lib, c, impl, parts=1, into=into)
    assert all(_untouched(out[n]) for n in ("dq", "dk", "dv")), "parts = 1 wrote a gradient"
    run_bwd(lib, c, impl, parts=4, into=into)
    assert _untouched(out["dq"]), "parts = 4 wrote dq"
    run_bwd(lib, c, impl, parts=2, into=into)
    judge(f"impl {IMPLS[impl]} parts 1, 4, 2", out, checks, bwd_bounds_of(c), GRADS)
    for n in GRADS:
        wchecks[n]()
        assert torch.equal(out[n], whole[n]), f"impl {IMPLS[impl]}: {n} of the split launch differs from parts = 7"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("impl", sorted(IMPLS), ids=list(IMPLS.values()))
def test_backward_end_to_end_from_the_projects_forward(lib, impl, causal):
    """o and lse come from the project's forward (automatic form); the reference uses the exact ones, the bound adds the forward's own o and lse
    bounds carried through delta and P (attn_bwd_bounds' o_err / lse_err)."""
    c = _case("varlen", 128, causal, (14, 2))
    f = fwd_bounds_of(c)
    fo, fchecks = run_fwd(lib, c, 0)
    judge(f"forward {_tag(c)}", fo, fchecks, f, ("o", "lse"))
    o_in = framed_thd_operand(fo["o"].contiguous())
    out, checks = run_bwd(lib, c, impl, o=o_in, lse=fo["lse"].contiguous())
    bounds = attn_bwd_bounds(c["q"], c["k"], c["v"], c["do"], f["o"][0], f["lse"][0], causal, c["cu"], c["scale"], o_err=f["o"][1], lse_err=f["lse"][1])
    worst = judge(f"impl {IMPLS[impl]} end to end {_tag(c)}", out, checks, bounds, ("dq", "dk", "dv"))
    _dump(f"backward end to end impl {IMPLS[impl]} causal={causal}", **worst)


# ---- append prefill -----------------------------------------------------------------------------------------------------------------------------------
def append_case(device="cuda"):
    """q [T, 14, 128] at positions past .. past + T - 1, a slot [2, max_ctx, 128] whose rows at and beyond past + T hold NaN."""
    T, past, max_ctx = APPEND
    q = randn_bf16(T, 14, 128, seed=1500, device=device)
    k, v = randn_bf16(2, max_ctx, 128, seed=1501, device=device), randn_bf16(2, max_ctx, 128, seed=1502, device=device)
    return q, k, v


def append_bounds(q, k, v):
    T, past, _ = APPEND
    return attn_fwd_bounds(q, k[:, :past + T].transpose(0, 1), v[:, :past + T].transpose(0, 1), True, past=past)


def test_append_prefill_every_element(lib):
    from vila_amd import ops
    T, past, max_ctx = APPEND
    q, k, v = append_case()
    bounds = append_bounds(q, k, v)
    slots = torch.full((2, 4, max_ctx, 128), float("nan"), dtype=torch.bfloat16, device="cuda")     # a NaN kv head before and behind each slot
    for s, t in enumerate((k, v)):
        slots[s, 1:3, :past + T] = t[:, :past + T]
    fq = framed_thd_operand(q)
    worst = {}
    for form in (1, 2, 3, 4):
        o, check = framed_thd(T, 14, 128)
        with _forced(lib, append=form):
            ops.attn_append(fq, slots[0, 1:3], slots[1, 1:3], past, out=o)
        worst[f"o_{FORMS[form]}"] = judge(f"append form {FORMS[form]}", {"o": o}, {"o": check}, bounds, ("o",))["o"]
        again, _ = framed_thd(T, 14, 128)
        with _forced(lib, append=form):
            ops.attn_append(fq, slots[0, 1:3], slots[1, 1:3], past, out=again)
        assert torch.equal(_int_view(o.contiguous()), _int_view(again.contiguous())), f"append form {FORMS[form]}: two calls differ"
    _dump(f"append T={T} past={past}", **worst)


# ---- determinism --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,causal,heads", [(128, True, (14, 2)), (72, False, (2, 2))])
def test_two_calls_are_bit_equal_in_every_framed_output(lib, D, causal, heads):
    c = _case("varlen", D, causal, heads)
    for form, name in sorted(FORMS.items()):
        a, _ = run_fwd(lib, c, form)
        b, _ = run_fwd(lib, c, form)
        for n in ("o", "lse"):
            assert torch.equal(_int_view(a[n].contiguous()), _int_view(b[n].contiguous())), f"form {name} D={D}: two calls differ in {n}"
    for impl, name in IMPLS.items():
        a, _ = run_bwd(lib, c, impl)
        b, _ = run_bwd(lib, c, impl)
        for n in GRADS:
            assert torch.equal(_int_view(a[n].contiguous()), _int_view(b[n].contiguous())), f"impl {name} D={D}: two calls differ in {n}"
