"""References and fixtures of the LoRA serving tests (tests/test_gpu_lora_serving_ops.py, tests/test_gpu_lora_serving.py, tests/test_lora_serving_cpu.py):
fp64 references of the shrink and expand kernels of vila_amd/csrc/lora_decode.hip on the kernel's own inputs, framed banks, and adapters with
weights worth testing (B != 0) for the end-to-end tests."""
import torch

from tests.gpu_util import assert_bits_equal as _assert_bits_equal_bf16, framed_operand

NAN_SLOT = 1                                             # the slot no map names: it holds NaN, a read of it shows in the result
CAPACITY = 3
MAPS = ("none", "one", "mixed")
SCALES = (0.25, 16.0 / 48.0, 2.0)                        # per slot, as fp32 holds them (alpha / r of three adapters)


def row_map(kind: str, n: int):
    """The rows' slots: all -1, all slot 2, or (2, 0, -1) in turn.  No map names NAN_SLOT."""
    if kind == "none":
        return [-1] * n
    if kind == "one":
        return [2] * n
    return [(2, 0, -1)[i % 3] for i in range(n)]


def rand_bf16(shape, seed, scale=1.0, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=device) * scale).to(torch.bfloat16)


def rand_f32(shape, seed, scale=1.0, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(shape, generator=g, device=device) * scale


def framed_bank(t: torch.Tensor, guard: int = 1) -> torch.Tensor:
    """[capacity, ...] values as a view between NaN guard slots, with slot NAN_SLOT itself NaN: the kernels read slot a of a row that names a only."""
    buf = torch.full((t.shape[0] + 2 * guard, *t.shape[1:]), float("nan"), dtype=t.dtype, device=t.device)
    view = buf[guard:guard + t.shape[0]]
    view.copy_(t)
    view[NAN_SLOT].fill_(float("nan"))
    return view


def scales(device="cuda") -> torch.Tensor:
    return framed_operand(torch.tensor(SCALES, dtype=torch.float32, device=device), 0, 1)


def slots_tensor(slots, device="cuda") -> torch.Tensor:
    """row_adapter [n] int32 between guards that name NAN_SLOT: a read past the n rows makes a row read the NaN slot."""
    return framed_operand(torch.tensor(list(slots), dtype=torch.int32, device=device), 0, 1, pad=NAN_SLOT)


def shrink_ref(x: torch.Tensor, a_bank: torch.Tensor, scale: torch.Tensor, slots):
    """-> (T [n, Rs], |.| sums) in fp64: scale[a] * x_i . A_a^T on the scaled products; zero rows for -1."""
    n, Rs = x.shape[0], a_bank.shape[1]
    ref = torch.zeros((n, Rs), dtype=torch.float64, device=x.device)
    ab = torch.zeros_like(ref)
    for i, a in enumerate(slots):
        if a >= 0:
            s = float(scale[a])
            ref[i] = s * (x[i].double() @ a_bank[a].double().t())
            ab[i] = abs(s) * (x[i].double().abs() @ a_bank[a].double().abs().t())
    return ref, ab


def expand_ref(t: torch.Tensor, bt_bank: torch.Tensor, slots, c1: int, c2: int):
    """-> (D [n, N], |.| sums) in fp64 from Bt [capacity, r, N]: columns [0, c1) | [c1, c2) | [c2, N) read t's first, second, third r-wide slice."""
    n, (r, N) = t.shape[0], bt_bank.shape[1:]
    ref = torch.zeros((n, N), dtype=torch.float64, device=t.device)
    ab = torch.zeros_like(ref)
    segs = [(0, c1, 0), (c1, c2, r), (c2, N, 2 * r)]
    for i, a in enumerate(slots):
        if a < 0:
            continue
        for lo, hi, off in segs:
            if hi > lo:
                ti, b = t[i, off:off + r].double(), bt_bank[a, :, lo:hi].double()
                ref[i, lo:hi] = ti @ b
                ab[i, lo:hi] = ti.abs() @ b.abs()
    return ref, ab


def assert_bits_equal(out: torch.Tensor, ref: torch.Tensor, what: str = "") -> None:
    """tests/gpu_util.py assert_bits_equal for bf16; the same check on the int32 bit patterns for the fp32 outputs of shrink, expand and the logits."""
    if out.dtype == torch.bfloat16:
        return _assert_bits_equal_bf16(out, ref, what)
    assert out.shape == ref.shape and out.dtype == ref.dtype == torch.float32, (tuple(out.shape), tuple(ref.shape), out.dtype, ref.dtype)
    o, r = out.contiguous().view(torch.int32), ref.to(out.device).contiguous().view(torch.int32)
    bad = o != r
    k = int(bad.sum())
    if k:
        of, rf = out.contiguous().reshape(-1), ref.to(out.device).contiguous().reshape(-1)
        at = [(int(i), float(of[i]), float(rf[i])) for i in bad.reshape(-1).nonzero()[:8, 0].tolist()]
        raise AssertionError(f"{what}: {k} of {out.numel()} elements differ bit for bit; first (flat index, got, expected) {at}")


def is_plus_zero(t: torch.Tensor) -> bool:
    return bool((t.contiguous().view(torch.int32) == 0).all())


# ---- adapters for the end-to-end tests --------------------------------------------------------------------------------------------------------------
def random_adapter(lcfg, r: int, alpha: float, targets=None, seed: int = 0, b_std: float = 0.02, device="cpu"):
    """A LoraAdapters with PEFT's A (init_) and a NORMAL B of standard deviation b_std (PEFT's B = 0 makes the adapter the identity)."""
    from vila_amd import lora
    cfg = lora.LoraConfig(r=r, alpha=alpha, **({} if targets is None else dict(target_modules=tuple(targets))))
    ad = lora.LoraAdapters(lcfg, cfg, device=device).init_(seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 7919)
    with torch.no_grad():
        for i in range(lcfg.num_hidden_layers):
            for m in cfg.target_modules:
                _, bt = ad.pair(i, m)
                bt.copy_((torch.randn(bt.shape, generator=g) * b_std).to(torch.bfloat16))
    return ad


def merged_llm_weights(weights: dict, ad, prefix: str = "llm.") -> dict:
    """fp32 copies of the model's weights with W + s B A on every projection the adapter targets (the oracle's merged model; nothing is rounded)."""
    from vila_amd.lora import _PARENT
    out = {k: v.detach().float().cpu().clone() for k, v in weights.items()}
    for i in range(ad.lcfg.num_hidden_layers):
        for m in ad.cfg.target_modules:
            a, bt = ad.pair(i, m)
            key = f"{prefix}model.layers.{i}.{_PARENT[m]}.{m}.weight"
            out[key] = out[key] + ad.cfg.scale * (bt.float().cpu().t() @ a.float().cpu())
    return out
