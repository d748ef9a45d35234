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


# ---- planted-key inputs for the decode attentions (tests/test_decode_probe_cpu.py, tests/test_gpu_decode_keys.py) -------------------------
# With i.i.d. random Q/K/V one key of L carries about 1/L of a head's softmax weight, so a key lost or admitted at a chunk, slice or capacity
# boundary moves the output by less than the tests' bound once L is a few hundred.  A PLANTED key is alpha * q of one target query head per kv
# head: its score alpha |q|^2 / sqrt(128) is about 22 at alpha = 2 against N(0, 1) for the random keys, so it takes essentially all of that
# head's weight and the head returns that key's (random) V row.  Lose the key or admit one too many and the target heads move by O(|V|).
def probe_targets(kv: int, G: int):
    """The target query head of every kv head: another member of the group for each (kv head h -> head h * G + h % G)."""
    return [h * G + h % G for h in range(kv)]


def plant_keys(k_slot: torch.Tensor, q_row: torch.Tensor, keys, alpha=2.0) -> None:
    """In place: k_slot [kv, C, 128] bf16 gets, for every kv head h, rows `keys` = bf16(alpha * q_row[target head of h]) (q_row [nq, 128] bf16);
    alpha a number or one per key.  The V rows stay as they are."""
    kv, G = k_slot.shape[0], q_row.shape[0] // k_slot.shape[0]
    keys = list(keys)
    alphas = [float(alpha)] * len(keys) if not hasattr(alpha, "__len__") else [float(a) for a in alpha]
    for h, t in enumerate(probe_targets(kv, G)):
        for key, a in zip(keys, alphas):
            k_slot[h, key] = (a * q_row[t].float()).to(torch.bfloat16)


def staircase_alphas(q_row: torch.Tensor, kv: int, n_keys: int, step: float = 9.0, alpha0: float = 2.0):
    """alpha of planted key j = alpha0 + j * c with c chosen so that the score alpha |q|^2 / sqrt(128) of EVERY kv head's target rises by at least
    `step` per key (c from the smallest |q_t|^2): key j then outweighs all earlier ones by e^step."""
    G = q_row.shape[0] // kv
    n2 = min(float(q_row[t].float().pow(2).sum()) for t in probe_targets(kv, G))
    c = step * 128 ** 0.5 / n2
    return [alpha0 + j * c for j in range(n_keys)]


def decode_attn_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, visible: torch.Tensor, scale=None) -> torch.Tensor:
    """fp32 softmax over exactly the visible keys: q [n, nq, 128], k / v [n or 1, kv, C, 128] (row i reads slot i, or all rows the one slot),
    visible [n, C] bool -> o [n, nq, 128] fp32.  One kv head at a time, nothing expanded."""
    n, nq, D = q.shape
    kv = k.shape[1]
    G = nq // kv
    scale = D ** -0.5 if scale is None else scale
    out = torch.empty((n, nq, D), dtype=torch.float32, device=q.device)
    hide = ~visible[:, None, :]
    assert k.shape[0] in (1, n) and k.shape == v.shape and visible.shape == (n, k.shape[2])
    for h in range(kv):
        kh, vh = k[:, h].float().expand(n, -1, -1), v[:, h].float().expand(n, -1, -1)      # (a view: one slot serves every row)
        s = torch.einsum("ngd,ncd->ngc", q[:, h * G:(h + 1) * G].float(), kh) * scale
        p = torch.softmax(s.masked_fill(hide, float("-inf")), -1)
        out[:, h * G:(h + 1) * G] = torch.einsum("ngc,ncd->ngd", p, vh)
    return out


def visible_upto(lens, C: int, device="cpu") -> torch.Tensor:
    """[n, C] bool: row i sees keys 0 .. lens[i] - 1."""
    return torch.arange(C, device=device)[None, :] < torch.as_tensor(list(lens), device=device)[:, None]
