"""The reference of the processed verify step's chain, in plain Python on the CPU, shared by tests/test_spec_processed_cpu.py and
tests/test_gpu_spec_processed.py.

A verify step runs n rows of ONE sequence; row i consumes token[i] behind token[0 .. i - 1].  The closed forms the kernels implement:
  penalties   row i sees c_i(v) = min(65535, counts[v] + #{j <= i : token[j] == v}); ids outside 0 .. V - 1 count nothing
  automaton   s_0 = adv(state, token[0]), s_i = adv(s_{i-1}, token[i]); a transition < 0, an id out of range or a class >= C leaves the state, -1 stays
and their sequential twins: one `penalize_ref` / `constrain_ref` call per row, the table bumped (saturating) and the state advanced between the calls,
which is what the session drafting nothing does.  tests/test_spec_processed_cpu.py shows the two equal."""
import numpy as np
import torch

from tests.constrain_ref import constrain_ref
from tests.penalty_ref import penalize_ref


def chain_counts(counts, tokens, i: int) -> torch.Tensor:
    """counts [V] integer, tokens: the step's token[] -> c_i [V] int64, the closed form."""
    c = counts.detach().cpu().to(torch.int64).reshape(-1).clone()
    V = c.numel()
    add = torch.zeros(V, dtype=torch.int64)
    for t in list(tokens)[:i + 1]:
        if 0 <= int(t) < V:
            add[int(t)] += 1
    return (c + add).clamp_(max=65535)


def penalize_chain_ref(x, counts, tokens, rep, pres, freq) -> torch.Tensor:
    """x [n, V] fp32, counts [V] -> y [n, V]: row i by `penalize_ref` on the closed-form counts."""
    x = x.detach().cpu().float()
    return torch.cat([penalize_ref(x[i:i + 1], chain_counts(counts, tokens, i)[None], rep, pres, freq) for i in range(x.shape[0])])


def penalize_sequential_ref(x, counts, tokens, rep, pres, freq):
    """The session drafting nothing: bump (saturating), then penalise, row by row -> (y [n, V], the table behind every row [n, V])."""
    x = x.detach().cpu().float()
    c = counts.detach().cpu().to(torch.int64).reshape(-1).clone()
    V = c.numel()
    ys, tables = [], []
    for i in range(x.shape[0]):
        t = int(tokens[i])
        if 0 <= t < V:
            c[t] = min(65535, int(c[t]) + 1)
        ys.append(penalize_ref(x[i:i + 1], c[None], rep, pres, freq))
        tables.append(c.clone())
    return torch.cat(ys), torch.stack(tables)


def adv(s: int, t: int, cls, nxt, C: int, V: int) -> int:
    """constrain.hip's advance rule.  cls [>= V] (uint16 values), nxt: the flat table."""
    s, t, C = int(s), int(t), int(C)
    if s < 0 or not 0 <= t < V or C < 1 or (s + 1) * C > len(nxt):
        return s
    c = int(cls[t]) & 0xFFFF
    if c >= C:
        return s
    s2 = int(nxt[s * C + c])
    return s2 if s2 >= 0 else s


def chain_states(state: int, tokens, cls, nxt, C: int, V: int):
    out, s = [], int(state)
    for t in tokens:
        s = adv(s, t, cls, nxt, C, V)
        out.append(s)
    return out


def constrain_chain_ref(x, state: int, cls, nxt, C: int, tokens):
    """x [n, V] fp32 -> (y [n, V] fp32 numpy, states [n]): row i masked from s_i by `constrain_ref` (no token: the chain has advanced already)."""
    x = np.asarray(x, dtype=np.float32)
    n, V = x.shape
    cls, nxt = np.asarray(cls).reshape(-1), np.asarray(nxt).reshape(-1)
    states = chain_states(state, tokens, cls, nxt, C, V)
    y = np.concatenate([constrain_ref(x[i:i + 1], [states[i]], cls[None], nxt[None], [C])[0] for i in range(n)])
    return y, states


def constrain_sequential_ref(x, state: int, cls, nxt, C: int, tokens):
    """The session drafting nothing: one `constrain_ref` with the consumed token per row, the state carried along."""
    x = np.asarray(x, dtype=np.float32)
    n, V = x.shape
    cls, nxt = np.asarray(cls).reshape(-1), np.asarray(nxt).reshape(-1)
    ys, states, s = [], [], int(state)
    for i in range(n):
        t = int(tokens[i])
        y, s2 = constrain_ref(x[i:i + 1], [s], cls[None], nxt[None], [C], token=[t] if 0 <= t < V else None)
        s = int(s2[0])
        ys.append(y)
        states.append(s)
    return np.concatenate(ys), states
