import json
import os

import torch

# "grads cosine >= 0.999" — the stated bound of every model-gradient comparison (bf16 HIP step vs fp32 autograd).
# A tensor that cannot meet it carries a per-tensor exception at its call site, with the measured value and the reason.
GRAD_COS_MIN = 0.999


def grad_cos(test: str, name: str, got: torch.Tensor, ref: torch.Tensor) -> float:
    """Cosine of a gradient tensor against its fp32 reference.  With VILA_DUMP_COS=<file> every measured value is appended as a JSON line
    (what the per-tensor exceptions in the tests were read from)."""
    cos = float(torch.nn.functional.cosine_similarity(got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten(), dim=0))
    path = os.environ.get("VILA_DUMP_COS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": test, "tensor": name, "cos": cos, "ref_norm": float(ref.norm()), "numel": ref.numel()}) + "\n")
    return cos


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    return float((a - b).norm() / (b.norm() + 1e-30))


def max_abs(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def randn_bf16(*shape, seed=0, scale=1.0, device="cuda"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(device=device, dtype=torch.bfloat16)


def margin_aware_ids(lg, lg_o, ids_o, free_ids=None):
    """SURVEY §8c id rule.  `lg` [n,V]: teacher-forced GPU logits (the oracle's ids were fed), `lg_o` / `ids_o`: the oracle's.  At every
    step whose oracle top-1/top-2 margin exceeds 4x the observed max-abs logit error the argmax must be bit-exact; `free_ids` (a
    free-running greedy run of the same model) must equal the oracle's ids up to the first non-decisive step — until then it was fed
    exactly the teacher-forced inputs.  Returns the decisive mask."""
    import torch
    lg, lg_o = lg.detach().float().cpu(), lg_o.detach().float().cpu()
    err = float((lg - lg_o).abs().max())
    top2 = lg_o.topk(2, -1).values
    decisive = (top2[:, 0] - top2[:, 1]) > 4 * err
    assert bool(decisive.any()), f"no decisive step (err {err:.3e}, margins {(top2[:, 0] - top2[:, 1]).tolist()})"
    got = lg.argmax(-1)
    assert torch.equal(got[decisive], ids_o[decisive]), f"ids {got.tolist()} vs oracle {ids_o.tolist()} (err {err:.3e}, decisive {decisive.tolist()})"
    if free_ids is not None:
        free_ids = free_ids.detach().cpu().reshape(-1)
        nd = (~decisive).nonzero().flatten()
        k = int(nd[0]) if nd.numel() else len(ids_o)
        assert torch.equal(free_ids[:k], ids_o[:k]), f"free-running ids {free_ids.tolist()} vs oracle {ids_o.tolist()} (first {k} must match)"
    return decisive


def attn_ref(q, k, v, causal, cu=None, scale=None, return_lse=False):
    """fp32 attention reference: softmax(scale * Q K^T + mask) V per sequence (`cu` = cu_seqlens, None = one sequence), GQA: q head h reads
    kv head h // (Hq / Hkv); scale defaults to D^-0.5.  Computed per sequence and kv head so that the fp32 score matrices of long shapes stay
    a few GB.  -> o [T, Hq, D] fp32 (+ lse [Hq, T] fp32, the natural-log sum of exp(scale * s) over the visible keys)."""
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    scale = D ** -0.5 if scale is None else scale
    out = torch.zeros((T, Hq, D), device=q.device, dtype=torch.float32)
    lse = torch.zeros((Hq, T), device=q.device, dtype=torch.float32)
    bounds = [0, T] if cu is None else cu.tolist()
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b == a:
            continue
        future = torch.triu(torch.ones(b - a, b - a, dtype=torch.bool, device=q.device), 1) if causal else None
        for g in range(Hkv):
            hs = slice(g * G, (g + 1) * G)
            s = torch.einsum("qhd,kd->hqk", q[a:b, hs].float(), k[a:b, g].float()) * scale
            if causal:
                s = s.masked_fill(future, float("-inf"))
            lse[hs, a:b] = torch.logsumexp(s, -1)
            out[a:b, hs] = torch.einsum("hqk,kd->qhd", torch.softmax(s, -1), v[a:b, g].float())
    return (out, lse) if return_lse else out


def attn_ref_grads(q, k, v, do, causal, cu=None, scale=None):
    """fp32 autograd through attn_ref's formula, one kv head (and its q-head group) at a time.  -> o, dq, dk, dv (fp32)."""
    T, Hq, D = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    scale = D ** -0.5 if scale is None else scale
    bounds = [0, T] if cu is None else cu.tolist()
    o = torch.zeros((T, Hq, D), device=q.device, dtype=torch.float32)
    dq, dk, dv = torch.zeros_like(o), torch.zeros((T, Hkv, D), device=q.device, dtype=torch.float32), torch.zeros((T, Hkv, D), device=q.device, dtype=torch.float32)
    for g in range(Hkv):
        hs = slice(g * G, (g + 1) * G)
        qf = q[:, hs].float().detach().requires_grad_(True)
        kf = k[:, g].float().detach().requires_grad_(True)
        vf = v[:, g].float().detach().requires_grad_(True)
        outs = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            s = torch.einsum("qhd,kd->hqk", qf[a:b], kf[a:b]) * scale
            if causal:
                s = s.masked_fill(torch.triu(torch.ones(b - a, b - a, dtype=torch.bool, device=q.device), 1), float("-inf"))
            outs.append(torch.einsum("hqk,kd->qhd", torch.softmax(s, -1), vf[a:b]))
        og = torch.cat(outs, 0)
        og.backward(do[:, hs].float())
        o[:, hs], dq[:, hs], dk[:, g], dv[:, g] = og.detach(), qf.grad, kf.grad, vf.grad
    return o, dq, dk, dv
