"""The element-wise bounds of the prefill / SFT attention (tests/gpu_util.py attn_fwd_bounds, attn_bwd_bounds), proved on the CPU before they
judge a kernel (tests/test_gpu_attn_elements.py), at that file's shapes and inputs.

  - Each bound admits an fp32 torch emulation of the kernels' formula: online softmax over 64-key tiles, P rounded to bf16 before PV, l summed from
    the unrounded e, o = bf16(O * (1 / l)), lse = m scale + log l; the backward with P = exp2(s c - lse log2 e), bf16 P before dV, bf16 t before
    dQ and dK.  Two summation orders: every tile in order, and the even and the odd tiles walked separately and merged (the key-split forms; the
    backward's sums split the same way).  Worst err / bound <= 1 at every case.
  - The check stays sharp: the fp32 part of a bound stays below its rounding part for at least 99 % of the elements of every case, with the derived
    exceptions of SHARP_EXCEPTIONS.
  - The bound rejects each injected fault (a) - (g) of FAULTS, and test_old_assertions_pass_the_faults states which of them the assertions of
    tests/test_gpu_attention_forms.py (o rel-L2 < 8e-3 overall and per sequence, lse max-abs < 1e-4, dq / dk / dv rel-L2 < 1.5e-2) let through
    on that file's own inputs."""
import functools

import pytest
import torch

from tests.gpu_util import (BF16_U, FP32_U, _attn_blocks, assert_elementwise, attn_bwd_bounds, attn_fwd_bounds, attn_ref, attn_ref_grads, attn_visible, f32,
                            max_abs, randn_bf16, rel_l2)
from tests.test_gpu_attention_forms import GRAD_REL, LSE_MAX_ABS, O_REL, VARLEN
from tests.test_gpu_attn_elements import (APPEND, DIMS, HEADS, PLANT_FOR, PLANT_HEADS, STRESS_HEADS, append_bounds, append_case, assert_planted, attn_case,
                                          bwd_bounds_of, bwd_inputs_of, cu_of, fwd_bounds_of, qkv_inputs)

ORDERS = (0, 1)
NEG_BIG = -1.0e30
SHARP_MIN = 0.99
MIN_COUNT = 1000
# Where the fp32 part cannot stay below the rounding part for 99 % of the elements, and why; the fraction asserted instead.
#   "large" (q scaled by 27, scores of about +-80): a row's softmax is one key with P within 1e-3 of 1 for most rows.  There dP - delta cancels
#       (delta = o . do with o ~ that key's v row, dP = do . v): t = P (dP - delta) scale is of the size of (1 - P) |do| |v| scale, while the carried
#       fp32 error of dP - delta, (D + 1 + 12) u |do| |v| scale ~ 1e-5 |do . v|, and the relative error of P, (3 |x| + 2 |lse| + ..) u ~ 500 u = 3e-5,
#       do not shrink with it.  The rounding part 2^-8 sum |t| |K| falls below the carried part wherever 1 - P < 2^8 * 1e-5 ~ 3e-3: the share of
#       such (row, key) mass is what decides an element.  dq sums one row's keys, so a peaked row is lost as a whole: most rows.  dk sums a key's
#       rows over the group, and a few unpeaked rows with an ordinary t keep the rounding part on top: most elements stay sharp.  dv = P^T do has
#       no cancellation and stays sharp.  How many rows are peaked: 1 - P < 3e-3 needs the row's top two scores 5.8 apart; the gap at the top of L
#       normal scores of spread 27 is about exponential with mean 27 / sqrt(2 ln L) = 8 at L = 300, so e^(-5.8 / 8) ~ half of the rows are peaked and
#       half of dq's elements are expected to stay sharp (0.41 - 0.42 here; dk 0.85 - 0.86).  Asserted: half of that expectation for dq, 0.25, and
#       two thirds for dk, whose elements mix peaked and unpeaked rows.
SHARP_EXCEPTIONS = {("large", "dq"): 0.25, ("large", "dk"): 0.66}


def _k(v):
    return torch.tensor(v, dtype=torch.float32)


LOG2E = _k(1.4426950408889634)


def _sharp(bounds, name, rnd):
    _, _, acc = bounds[name]
    return float(((1.0 + BF16_U) * FP32_U * acc <= rnd).double().mean())


def _flat(t):
    return t.reshape(t.shape[0], -1) if t.dim() == 3 else t


def _admit(out, bounds, name, what):
    ref, bound, _ = bounds[name]
    w = assert_elementwise(_flat(out), _flat(ref), _flat(bound), what)
    assert w <= 1.0
    return w


def _rejects(out, bounds, name):
    ref, bound, _ = bounds[name]
    with pytest.raises(AssertionError, match="over the bound"):
        assert_elementwise(_flat(out), _flat(ref), _flat(bound), name)


# ---- fp32 emulations of the kernels' formulas --------------------------------------------------------------------------------------------------
def emu_fwd(q, k, v, causal, cu, scale, order, past=0, fault=None):
    """-> o [T, Hq, D] bf16, lse [Hq, T] fp32.  order 0: one key group walks every tile; 1: the even and the odd tiles, merged.  fault = (kind,
    token row, head): "lose" (a) the row loses key 63 of its sequence, "admit" (b) the row sees the key just above its diagonal, "a1" (c) the odd
    group's partial is merged with a1 = 1 (order 1), "inv" (d) the row is normalised with 1 / l of the row before it."""
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    s32 = _k(f32(D ** -0.5 if scale is None else scale))
    cc = s32 * LOG2E
    o = torch.zeros((T, Hq, D), dtype=torch.bfloat16)
    lse = torch.zeros((Hq, T), dtype=torch.float32)
    fk, frow, fh = fault if fault is not None else (None, -1, -1)
    for a, b, g in _attn_blocks(T, Hkv, cu):
        hs = slice(g * G, (g + 1) * G)
        q32 = q[a:b, hs].float().transpose(0, 1)
        k32, v32 = (t[(slice(None) if past else slice(a, b)), g].float() for t in (k, v))
        L, Lk = b - a, k32.shape[0]
        vis = attn_visible(L, Lk, causal, past)[None].expand(G, -1, -1).clone()
        hit = a <= frow < b and g * G <= fh < (g + 1) * G
        if hit and fk == "lose":
            vis[fh - g * G, frow - a, 63] = False
        if hit and fk == "admit":
            vis[fh - g * G, frow - a, frow - a + 1] = True
        nt = -(-Lk // 64)
        parts = []
        for tiles in ([range(nt)] if order == 0 else [range(0, nt, 2), range(1, nt, 2)]):
            m = torch.full((G, L), NEG_BIG)
            l = torch.zeros((G, L))
            O = torch.zeros((G, L, D))
            for t in tiles:
                ks = slice(t * 64, min(Lk, t * 64 + 64))
                vt = vis[:, :, ks]
                act = vt.any(-1)
                if not bool(act.any()):
                    continue
                sc = torch.where(vt, q32 @ k32[ks].t(), _k(NEG_BIG))
                m_new = torch.maximum(m, sc.max(-1).values)
                alpha = torch.exp2((m - m_new) * cc)
                e = torch.exp2(sc * cc - (m_new * cc)[..., None])
                l_new = l * alpha + e.sum(-1)
                O_new = O * alpha[..., None] + e.to(torch.bfloat16).float() @ v32[ks]
                m, l, O = torch.where(act, m_new, m), torch.where(act, l_new, l), torch.where(act[..., None], O_new, O)
            parts.append((m, l, O))
        m, l, O = parts[0]
        if len(parts) == 2:
            m1, l1, O1 = parts[1]
            mm = torch.maximum(m, m1)
            a0, a1 = torch.exp2((m - mm) * cc), torch.exp2((m1 - mm) * cc)
            if hit and fk == "a1":
                a1[fh - g * G, frow - a] = 1.0
            m, l, O = mm, l * a0 + l1 * a1, O * a0[..., None] + O1 * a1[..., None]
        inv = 1.0 / l
        if hit and fk == "inv":
            inv[fh - g * G, frow - a] = inv[fh - g * G, frow - a - 1]
        o[a:b, hs] = (O * inv[..., None]).to(torch.bfloat16).transpose(0, 1)
        lse[hs, a:b] = m * s32 + torch.log(l)
    return o, lse


def _split_sum(terms, x, w, order, dim):
    """sum over `dim` blocks of 64 of einsum(terms, x_block, w_block) in fp32: order 0 at once, order 1 even and odd blocks separately, then added."""
    if order == 0:
        return torch.einsum(terms, x, w)
    n = x.shape[dim]
    idx = torch.arange(n)
    out = 0.0
    for par in (0, 1):
        sel = idx[(idx // 64) % 2 == par]
        if sel.numel():
            out = out + torch.einsum(terms, x.index_select(dim, sel), w.index_select(0 if w.dim() == 2 else 1, sel))
    return out


def emu_bwd(q, k, v, do, o, lse, causal, cu, scale, order, fault=None):
    """-> delta [Hq, T] fp32, dq, dk, dv bf16.  fault = (kind, token, head): "dv_tile" (e) dv of that key misses the last 64-row query tile of its
    sequence, "dk_head" (f) dk of the key's 64-key block (kv head `head`) misses the last head of its group, "delta" (g) dq of that row and head
    is formed with delta of the next head."""
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    s32 = _k(f32(D ** -0.5 if scale is None else scale))
    cc = s32 * LOG2E
    dq, dk, dv = (torch.zeros(t.shape, dtype=torch.bfloat16) for t in (q, k, v))
    delta = torch.zeros((Hq, T), dtype=torch.float32)
    fk, ftok, fh = fault if fault is not None else (None, -1, -1)
    for a, b, g in _attn_blocks(T, Hkv, cu):
        hs = slice(g * G, (g + 1) * G)
        L = b - a
        q32, do32, o32 = (t[a:b, hs].float().transpose(0, 1) for t in (q, do, o))
        k32, v32 = k[a:b, g].float(), v[a:b, g].float()
        vis = attn_visible(L, L, causal)
        pr = o32 * do32
        dl = pr.sum(-1) if order == 0 else pr.reshape(G, L, -1, 8).sum(-1).sum(-1)
        delta[hs, a:b] = dl
        dl_q = dl
        in_seq = a <= ftok < b
        if in_seq and fk == "delta" and g * G <= fh < (g + 1) * G - 1:
            dl_q = dl.clone()
            dl_q[fh - g * G, ftok - a] = dl[fh - g * G + 1, ftok - a]
        P = torch.where(vis, torch.exp2((q32 @ k32.t()) * cc - (lse[hs, a:b].float() * LOG2E)[..., None]), _k(0.0))
        dP = do32 @ v32.t()
        tq = (P * (dP - dl_q[..., None]) * s32).to(torch.bfloat16).float()
        tk = (P * (dP - dl[..., None]) * s32).to(torch.bfloat16).float()
        Pb = P.to(torch.bfloat16).float()
        dq[a:b, hs] = _split_sum("hqk,kd->hqd", tq, k32, order, 2).to(torch.bfloat16).transpose(0, 1)
        dk_ = _split_sum("hqk,hqd->kd", tk, q32, order, 1)
        dv_ = _split_sum("hqk,hqd->kd", Pb, do32, order, 1)
        if in_seq and fh == g and fk == "dv_tile":
            last = (L - 1) // 64 * 64
            dv_[ftok - a] = torch.einsum("hq,hqd->d", Pb[:, :last, ftok - a], do32[:, :last])
        if in_seq and fh == g and fk == "dk_head":
            k0 = (ftok - a) // 64 * 64
            dk_[k0:k0 + 64] = torch.einsum("hqk,hqd->kd", tk[:G - 1, :, k0:k0 + 64], q32[:G - 1])
        dk[a:b, g], dv[a:b, g] = dk_.to(torch.bfloat16), dv_.to(torch.bfloat16)
    return delta, dq, dk, dv


# ---- admission and sharpness at every GPU shape ------------------------------------------------------------------------------------------------------
def _prove(c, backward=True):
    kind = c["kind"]
    f = fwd_bounds_of(c)
    n = f["o"][0].numel()
    worst = {}
    for order in ORDERS:
        o, lse = emu_fwd(c["q"], c["k"], c["v"], c["causal"], c["cu"], c["scale"], order)
        worst[f"o{order}"] = _admit(o, f, "o", f"{kind} o order {order}")
        worst[f"lse{order}"] = _admit(lse, f, "lse", f"{kind} lse order {order}")
    if n >= MIN_COUNT:
        sh = _sharp(f, "o", f["rnd_o"])
        assert sh >= SHARP_EXCEPTIONS.get((kind, "o"), SHARP_MIN), f"{kind}: o's fp32 part is below the rounding part for only {sh:.4f} of the elements"
    if not backward:
        return worst
    bw = bwd_bounds_of(c)
    o_bf, lse32 = bwd_inputs_of(c)
    for order in ORDERS:
        outs = emu_bwd(c["q"], c["k"], c["v"], c["do"], o_bf, lse32, c["causal"], c["cu"], c["scale"], order)
        for name, out in zip(("delta", "dq", "dk", "dv"), outs):
            worst[f"{name}{order}"] = _admit(out, bw, name, f"{kind} {name} order {order}")
    for name in ("dq", "dk", "dv"):
        if bw[name][0].numel() >= MIN_COUNT:
            sh = _sharp(bw, name, bw["rnd_" + name])
            assert sh >= SHARP_EXCEPTIONS.get((kind, name), SHARP_MIN), f"{kind}: {name}'s fp32 part is below the rounding part for only {sh:.4f}"
    return worst


@pytest.mark.parametrize("heads", HEADS, ids=["gqa1", "gqa7"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("kind", ["varlen", "uniform", "scale"])
def test_bounds_admit_the_emulation(kind, D, causal, heads):
    w = _prove(attn_case(kind, D, causal, heads, "cpu"), backward=kind != "scale")
    print(kind, D, causal, heads, {k: round(v, 3) for k, v in w.items()})


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("kind", ["jump", "vjump", "large", "zero"])
def test_bounds_admit_the_emulation_under_stress(kind, causal):
    w = _prove(attn_case(kind, 128, causal, STRESS_HEADS, "cpu"), backward=kind == "large")
    print(kind, causal, {k: round(v, 3) for k, v in w.items()})


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", DIMS)
def test_bounds_admit_the_emulation_on_planted_pairs(D, causal):
    for which in PLANT_FOR[causal]:
        c = attn_case("plant:" + which, D, causal, PLANT_HEADS[D], "cpu")
        assert_planted(c)
        w = _prove(c)
        print(which, D, causal, {k: round(v, 3) for k, v in w.items()})


def test_append_bound_admits_the_emulation():
    T, past, _ = APPEND
    q, k, v = append_case("cpu")
    bounds = append_bounds(q, k, v)
    kt, vt = k[:, :past + T].transpose(0, 1), v[:, :past + T].transpose(0, 1)
    for order in ORDERS:
        o, _ = emu_fwd(q, kt, vt, True, None, None, order, past=past)
        _admit(o, bounds, "o", f"append order {order}")
    assert _sharp(bounds, "o", bounds["rnd_o"]) >= SHARP_MIN


def test_end_to_end_bound_admits_the_emulated_forward():
    """The backward on the emulated forward's o and lse against the exact reference, under the bound that carries the forward's o and lse bounds."""
    c = attn_case("uniform", 128, True, (14, 2), "cpu")
    f = fwd_bounds_of(c)
    bounds = attn_bwd_bounds(c["q"], c["k"], c["v"], c["do"], f["o"][0], f["lse"][0], True, c["cu"], c["scale"], o_err=f["o"][1], lse_err=f["lse"][1])
    for order in ORDERS:
        o, lse = emu_fwd(c["q"], c["k"], c["v"], True, c["cu"], c["scale"], order)
        outs = emu_bwd(c["q"], c["k"], c["v"], c["do"], o, lse, True, c["cu"], c["scale"], order)
        for name, out in zip(("delta", "dq", "dk", "dv"), outs):
            if name != "delta":
                _admit(out, bounds, name, f"end to end {name} order {order}")


# ---- injected faults, on the inputs of tests/test_gpu_attention_forms.py -----------------------------------------------------------------------------
FAULT_D, FAULT_HEADS = 128, (14, 2)
_S300 = sum(VARLEN) - 300                   # first token of the batch's last sequence (300 rows)
# (name, pass, (kind, token, head), the outputs the fault reaches)
FAULTS = [
    ("a: a row loses the last key of a 64-key tile", "fwd", ("lose", _S300 + 200, 3), ("o", "lse")),
    ("b: a row admits the key above the causal diagonal", "fwd", ("admit", _S300 + 200, 3), ("o", "lse")),
    ("c: the odd-tile key group merged with a1 = 1 for a row", "fwd", ("a1", _S300 + 200, 3), ("o", "lse")),
    ("d: the last row of a sequence takes 1 / l of the row before it", "fwd", ("inv", _S300 + 299, 3), ("o",)),
    ("e: dv of a key misses the last query tile of its sequence", "bwd", ("dv_tile", _S300 + 100, 1), ("dv",)),
    ("f: dk of a kv head's key block misses the last head of its group", "bwd", ("dk_head", _S300 + 100, 1), ("dk",)),
    ("g: dq of a row formed with delta of the neighbouring head", "bwd", ("delta", _S300 + 200, 3), ("dq",)),
]


@functools.lru_cache(maxsize=1)
def _old_inputs():
    """test_every_form_matches_the_reference's varlen inputs (seed 100 + D) and test_backward_both_implementations' (700 + D, do 701), causal,
    with their fp32 references and the new bounds."""
    Hq, Hkv = FAULT_HEADS
    cu = cu_of(VARLEN, "cpu")
    T = sum(VARLEN)
    fq, fk, fv = qkv_inputs(T, Hq, Hkv, FAULT_D, 100 + FAULT_D, device="cpu")
    bq, bk, bv = qkv_inputs(T, Hq, Hkv, FAULT_D, 700 + FAULT_D, device="cpu")
    do = randn_bf16(T, Hq, FAULT_D, seed=701, device="cpu")
    d = {"cu": cu, "fwd": (fq, fk, fv), "bwd": (bq, bk, bv, do)}
    d["fwd_ref"] = attn_ref(fq, fk, fv, True, cu, return_lse=True)
    d["fwd_bounds"] = attn_fwd_bounds(fq, fk, fv, True, cu)
    d["bwd_ref"] = attn_ref_grads(bq, bk, bv, do, True, cu)[1:]
    d["bwd_o_lse"] = emu_fwd(bq, bk, bv, True, cu, None, 1)             # the old test: o and lse from the forward
    f = attn_fwd_bounds(bq, bk, bv, True, cu)
    d["bwd_alone"] = (f["o"][0].to(torch.bfloat16), f["lse"][0].float())  # the new check: bf16(reference o), fp32(reference lse)
    d["bwd_bounds"] = attn_bwd_bounds(bq, bk, bv, do, *d["bwd_alone"], True, cu)
    return d


def _old_forward_passes(d, o, lse):
    """The assertions of test_gpu_attention_forms._check_fwd -> (passes, worst o rel-L2 of the batch and its sequences, lse max-abs)."""
    ref, lse_ref = d["fwd_ref"]
    rels = [rel_l2(o, ref)] + [rel_l2(o[a:b], ref[a:b]) for a, b in zip(d["cu"].tolist()[:-1], d["cu"].tolist()[1:])]
    err = max_abs(lse, lse_ref)
    ok = bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all()) and max(rels) < O_REL and err < LSE_MAX_ABS
    return ok, max(rels), err


def _old_backward_passes(d, grads):
    rels = {n: rel_l2(g, r) for n, g, r in zip(("dq", "dk", "dv"), grads, d["bwd_ref"])}
    return all(r < GRAD_REL for r in rels.values()), rels


def _run_fault(d, which, fault, old=False):
    """The emulation with the fault -> (outputs, the new bounds).  The backward takes what each check gives it: o and lse of the (emulated) forward
    under the old assertions, bf16(reference o) and fp32(reference lse) under the new check."""
    if which == "fwd":
        o, lse = emu_fwd(*d["fwd"], True, d["cu"], None, 1, fault=fault)
        return {"o": o, "lse": lse}, d["fwd_bounds"]
    o, lse = d["bwd_o_lse"] if old else d["bwd_alone"]
    _, dq, dk, dv = emu_bwd(*d["bwd"], o, lse, True, d["cu"], None, 1, fault=fault)
    return {"dq": dq, "dk": dk, "dv": dv}, d["bwd_bounds"]


def test_fault_free_emulation_passes_both_checks():
    d = _old_inputs()
    out, bounds = _run_fault(d, "fwd", None)
    assert _old_forward_passes(d, out["o"], out["lse"])[0]
    for n in ("o", "lse"):
        _admit(out[n], bounds, n, f"old inputs {n}")
    out, _ = _run_fault(d, "bwd", None, old=True)
    assert _old_backward_passes(d, (out["dq"], out["dk"], out["dv"]))[0]
    out, bounds = _run_fault(d, "bwd", None)
    for n in ("dq", "dk", "dv"):
        _admit(out[n], bounds, n, f"old inputs {n}")


@pytest.mark.parametrize("name,which,fault,reached", FAULTS, ids=[f[0][0] for f in FAULTS])
def test_bound_rejects_the_fault(name, which, fault, reached):
    out, bounds = _run_fault(_old_inputs(), which, fault)
    _rejects(out[reached[0]], bounds, reached[0])


# Which faults today's assertions let through on their own inputs (figures: CHANGELOG.md).  Every forward fault passes the o rel-L2 assertions
# (2.0e-3 .. 3.7e-3 against 8e-3, overall and in its sequence).  (a), (b) and (c) change the row's l, so they move its lse by about the weight of
# the key (1e-2, 1.3e-3) or by the whole odd group (0.16): the old lse max-abs of 1e-4 sees those three; (d) leaves lse alone and passes.  (e) and
# (g) pass the gradients' rel-L2 (3.2e-3 and 2.6e-3 against 1.5e-2); (f) drops a seventh of 64 whole dk rows, 3.3e-2 of the tensor, and is seen.
OLD_ASSERTIONS_PASS = {"a": False, "b": False, "c": False, "d": True, "e": True, "f": False, "g": True}


def test_old_assertions_pass_the_faults():
    d = _old_inputs()
    passed = {}
    for name, which, fault, _ in FAULTS:
        out, _ = _run_fault(d, which, fault, old=True)
        if which == "fwd":
            ok, rel, err = _old_forward_passes(d, out["o"], out["lse"])
            print(f"{name}: old assertions {'pass' if ok else 'FAIL'} (worst o rel-L2 {rel:.3e}, lse max-abs {err:.3e})")
        else:
            ok, rels = _old_backward_passes(d, (out["dq"], out["dk"], out["dv"]))
            print(f"{name}: old assertions {'pass' if ok else 'FAIL'} (" + ", ".join(f"{n} rel-L2 {r:.3e}" for n, r in rels.items()) + ")")
        passed[name[0]] = ok
    assert sum(passed.values()) >= 3, passed
    assert passed == OLD_ASSERTIONS_PASS, passed
