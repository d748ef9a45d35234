"""The reference of the logprob operator (vila_logprobs_f32): float64 log_softmax of the raw fp32 logits, and the top-n by a STABLE sort on
(value descending, index ascending) of the raw fp32 values.  tests/test_logprobs_cpu.py pins it to torch.log_softmax / torch.topk."""
import math

import torch

MAX_TOP = 20
EPS = 2.0 ** -23


def logprob_ref(x: torch.Tensor, top_n: int = MAX_TOP):
    """x [n, V] fp32 (CPU) -> (lp [n, V] float64 log_softmax, lse [n] float64, top_id [n, top_n] int64, top_lp [n, top_n] float64); places that a
    vocabulary below top_n cannot fill hold id -1 / -inf."""
    x = x.detach().cpu().float()
    n, V = x.shape
    x64 = x.double()
    lse = torch.logsumexp(x64, 1)
    lp = x64 - lse[:, None]
    order = torch.sort(x, dim=1, descending=True, stable=True).indices          # equal values keep their index order: the lower index first
    top_id = torch.full((n, top_n), -1, dtype=torch.int64)
    top_lp = torch.full((n, top_n), -math.inf, dtype=torch.float64)
    m = min(top_n, V)
    top_id[:, :m] = order[:, :m]
    top_lp[:, :m] = torch.gather(lp, 1, order[:, :m])
    return lp, lse, top_id, top_lp


def bound(x: torch.Tensor, lse: torch.Tensor) -> torch.Tensor:
    """Per row: 32 * 2^-23 * max(1, max |finite x|, |lse|) — three roundings at the magnitude of x / lse in x - (M + log L), a summation chain of
    at most ~40 roundings of relative 2^-24 on L, 1 - 2 ulp in exp."""
    x = x.detach().cpu().double()
    fin = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).amax(1)
    return 32 * EPS * torch.maximum(torch.ones_like(fin), torch.maximum(fin, lse.abs()))


def check_rows(x, token, tok_lp, top_lp, top_id, top_n, what="", ref=None):
    """The operator's three outputs for rows x [n, V] against the reference: every logprob within the row's bound, every id exactly the
    reference's.  token [n] (ids outside 0 .. V - 1 must give NaN).  top_lp / top_id: [n, >= top_n] (None with top_n = 0).  ref: logprob_ref(x, m)
    with m >= top_n, where the caller has it already.  Returns the worst error as a fraction of its bound."""
    x = x.detach().cpu().float()
    n, V = x.shape
    lp, lse, rid, rlp = logprob_ref(x, top_n) if ref is None else ref
    rid, rlp = rid[:, :top_n], rlp[:, :top_n]
    b = bound(x, lse)
    token, tok_lp = token.cpu(), tok_lp.detach().cpu().double()
    worst = 0.0
    for r in range(n):
        t = int(token[r])
        if 0 <= t < V:
            err = 0.0 if float(tok_lp[r]) == float(lp[r, t]) else abs(float(tok_lp[r]) - float(lp[r, t]))
            assert not math.isnan(err), f"{what} row {r}: token logprob {float(tok_lp[r])} vs {float(lp[r, t])}"
            assert err <= float(b[r]), f"{what} row {r}: token logprob {float(tok_lp[r])} vs {float(lp[r, t])}, error {err:.3e} > bound {float(b[r]):.3e}"
            worst = max(worst, err / float(b[r]))
        else:
            assert math.isnan(float(tok_lp[r])), f"{what} row {r}: token {t} outside the vocabulary must give NaN, got {float(tok_lp[r])}"
    if top_n:
        gid, glp = top_id.detach().cpu()[:, :top_n].long(), top_lp.detach().cpu()[:, :top_n].double()
        assert torch.equal(gid, rid), f"{what}: top ids differ from the reference order in rows {(gid != rid).any(1).nonzero().flatten().tolist()[:8]}"
        real = rid >= 0
        assert bool((glp[~real] == -math.inf).all()), f"{what}: an unused place does not hold -inf"
        err = torch.where(real & (glp != rlp), (glp - rlp).abs(), torch.zeros_like(rlp))      # (an -inf logit: -inf on both sides)
        over = ~(err <= b[:, None])
        assert not bool(over.any()), f"{what}: top logprob error {float(err.max()):.3e} over the bound in rows {over.any(1).nonzero().flatten().tolist()[:8]}"
        worst = max(worst, float((err / b[:, None]).max()))
    return worst
