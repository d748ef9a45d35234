"""The reference of the penalised pick, in torch on the CPU, shared by tests/test_penalties_cpu.py and tests/test_gpu_penalties.py.

counts[r, i] = how often row r's request has generated id i (HF's `input_ids` as a histogram: the prompt is given as embeddings and not counted).
Where c > 0: y = x * rep if x < 0 else x / rep (HF RepetitionPenaltyLogitsProcessor); then y = y - freq * c; then y = y - pres where c > 0 (OpenAI's
definition, vLLM's order).  Every step is one torch op on fp32 tensors, hence one correctly rounded fp32 operation per element."""
import torch


def penalize_ref(x: torch.Tensor, counts: torch.Tensor, rep, pres, freq) -> torch.Tensor:
    """x [n, V] fp32, counts [n, V] integer (values 0..65535), rep / pres / freq: floats or [n] tensors -> y [n, V] fp32."""
    x = x.detach().cpu().float()
    n = x.shape[0]
    def col(v):
        t = torch.as_tensor(v, dtype=torch.float32).detach().cpu().reshape(-1)
        return (t.expand(n) if t.numel() == 1 else t).reshape(n, 1)
    r, p, f = col(rep), col(pres), col(freq)
    c = counts.detach().cpu().to(torch.int64)
    seen = c > 0
    y = torch.where(seen, torch.where(x < 0, x * r, x / r), x)
    y = y - f * c.to(torch.float32)
    return torch.where(seen, y - p, y)


def first_argmax(y: torch.Tensor) -> int:
    """The first index of the maximum of a 1-D tensor (what the greedy pick returns)."""
    return int((y == y.max()).nonzero()[0])


def counts_of(ids, vocab: int) -> torch.Tensor:
    """Histogram [1, vocab] of a list of ids (ids outside 0 .. vocab - 1 count nothing), saturating at 65535."""
    c = torch.zeros(vocab, dtype=torch.int64)
    for t in ids:
        if 0 <= int(t) < vocab:
            c[int(t)] += 1
    return c.clamp_(max=65535)[None]


def u16_bits(c: torch.Tensor) -> torch.Tensor:
    """Integer counts 0..65535 -> the int16 tensor holding the same 16 bits (what the device table stores)."""
    c = c.to(torch.int64)
    return torch.where(c >= 32768, c - 65536, c).to(torch.int16)


def from_u16_bits(c16: torch.Tensor) -> torch.Tensor:
    return c16.detach().cpu().to(torch.int64) & 0xFFFF
