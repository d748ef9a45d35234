"""References, cases and bounds of the three LoRA operators (vila_amd/csrc/lora.hip), shared by tests/test_lora_cpu.py (which proves the bound on a
CPU emulation of each kernel's arithmetic) and tests/test_gpu_lora_ops.py (which holds the kernels to it), and the fp32-autograd reference of the
LoRA step (tests/test_gpu_lora.py).

The bound is the project's GEMM bound (tests/gpu_util.py gemm_elem_bound) with one rounding and three fp32 operations behind the products: the
product with `scale`, the addition of Res (or of the old G), and one for the ordered sum of the split partials, whose additions replace additions
of the unsplit chain (a slice's chain plus the slices stay below the contraction length: the splits start at K = 1024 and M = 257)."""
import torch

from tests.gpu_util import f32, gemm_elem_bound

EXTRA_OPS = 3


# ---- the host's split policies (lora.hip down_split / wgrad_split) --------------------------------------------------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def _up(a, b):
    return _cdiv(a, b) * b


def down_split(M, K):
    """-> (slices, k per slice): none below K = 1024 or from 256 row blocks on; 4 below K = 4096, 8 from there; whole 128-wide chunks."""
    want = 1 if (K < 1024 or _cdiv(M, 32) >= 256) else (4 if K < 4096 else 8)
    per = _up(_cdiv(K, want), 128)
    return _cdiv(K, per), per


def wgrad_split(M, C):
    """-> (slices, rows per slice): none up to 256 rows; above, enough for about 512 blocks, at most 32, whole 64-row stages."""
    if M <= 256:
        return 1, _up(M, 64)
    want = min(32, _cdiv(512, _cdiv(C, 64)))
    per = _up(_cdiv(M, want), 64)
    return _cdiv(M, per), per


# ---- cases: (M, K or N or C, R, flags), each with the dispatch edge it is for ---------------------------------------------------------------------
# down (M, K, R, ld_pad of T): a block is one wave of 32 rows (two MFMA row tiles) and walks K in 128-wide chunks, 8-element granules
DOWN_CASES = (
    [(M, K, R, pad) for M, (R, pad) in ((1, (16, 0)), (17, (48, 8)), (129, (192, 0))) for K in (32, 40, 3584)]   # row tail 1 / 17 / 4 blocks + 1 row;
    #                                                   K below a chunk, K % 32 != 0, 28 whole chunks; R = 48 and 192: tile buckets 3 and 12
    + [(17, K, 32, 0) for K in (1016, 1024, 1032)]      # no K split below 1024; 1024: 4 slices of 256; 1032: 3 of 384, the last 264 wide
    + [(17, K, 80, 16) for K in (4088, 4096, 4104)]     # 4 slices below 4096 (1024 wide, the last 1016), 8 of 512 at 4096, 7 of 640 at 4104; R = 80 runs in the 6-tile bucket
    + [(8160, 1024, 16, 0), (8161, 1024, 16, 0)]        # 255 row blocks: split; 256: not
    + [(3076, 3584, 192, 0), (3076, 18944, 64, 128)]    # the 8B shapes: t of the q|k|v stack; dt of gate / up into a [T, 2r] stack's slice
)
# up (M, N, R, with Res, ld_pad of Y and Res): a block is 64 columns x rows_per_block rows, a wave walks 16-row tiles 64 rows apart
UP_CASES = (
    [(M, N, R, res, pad) for (M, res, pad) in ((1, False, 0), (17, True, 8), (129, True, 0), (257, False, 24)) for N in (8, 72, 512) for R in (16, 48, 192)]
    #                                                   one row / a row tail / a wave's second and a block's fifth tile; N below 16, 64 + 8, 8 strips;
    #                                                   R = 16 and 48: the zero-padded half of a 32-deep MFMA step, 192: six steps
    + [(1100, 4096, 32, True, 0)]                       # rows_per_block = 128 (more than one 64-row round per block), 9 row blocks, the last partial
    + [(3076, 18944, 64, True, 0), (3076, 3584, 192, True, 0)]   # the 8B shapes: gate's contribution; dx of the q|k|v stack
)
# wgrad (M, C, R, accumulate, ld_pad of L): a block is 64 columns x one M slice in 64-row stages of two 32-row MFMA steps
WGRAD_CASES = (
    [(M, C, R, acc, pad) for (M, acc, pad) in ((1, False, 0), (31, True, 16), (33, False, 0), (64, True, 0), (65, False, 16)) for C in (8, 520) for R in (16, 192)]
    #                                                   below / above one MFMA step, one stage exactly, a second stage of one row; C below a wave's 16
    #                                                   columns, 8 strips + 8 columns
    + [(M, 520, 48, acc, 0) for M, acc in ((256, False), (257, True), (2048, False), (2049, True))]
    #                                                   no M split up to 256 rows; 257: 5 slices of 64 (the last one row); 2048 -> 2049: 32 slices of 64
    #                                                   become 17 of 128 (every other M edge is a slice count one higher at the same width)
    + [(3076, 8, 16, False, 0), (3076, 520, 192, True, 0)]      # 25 and 25 slices, the last short
    + [(3076, 18944, 64, False, 64), (3076, 3584, 192, False, 0)]  # the 8B shapes: dBt of gate from the [T, 2r] stack's slice; dA of q|k|v
)
SCALES = (0.25, 1.0, 0.37)


def case_scale(i):
    return SCALES[i % len(SCALES)]


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _bf(t):
    return t.to(torch.bfloat16)


def down_inputs(M, K, R):
    g = _gen(M + 3 * K + 7 * R)
    return _bf(torch.randn(M, K, generator=g)), _bf(torch.randn(R, K, generator=g) * 0.5)


def up_inputs(M, N, R):
    g = _gen(M + 3 * N + 7 * R + 1)
    return _bf(torch.randn(M, R, generator=g)), _bf(torch.randn(R, N, generator=g) * 0.5), _bf(torch.randn(M, N, generator=g) * 2.0)


def wgrad_inputs(M, C, R):
    g = _gen(M + 3 * C + 7 * R + 2)
    return _bf(torch.randn(M, R, generator=g)), _bf(torch.randn(M, C, generator=g) * 0.5), _bf(torch.randn(R, C, generator=g) * 2.0)


# ---- fp64 references and bounds (on the device the inputs live on) --------------------------------------------------------------------------------
def down_ref(x, a, scale):
    s = f32(scale)
    ref = s * (x.double() @ a.double().T)
    return ref, gemm_elem_bound(ref, abs(s) * (x.double().abs() @ a.double().abs().T), x.shape[1], roundings=1, extra_fp32_ops=EXTRA_OPS)


def up_ref(t, bt, res, scale):
    s = f32(scale)
    ref = s * (t.double() @ bt.double())
    absprod = abs(s) * (t.double().abs() @ bt.double().abs())
    if res is not None:
        ref, absprod = ref + res.double(), absprod + res.double().abs()
    return ref, gemm_elem_bound(ref, absprod, t.shape[1], roundings=1, extra_fp32_ops=EXTRA_OPS)


def wgrad_ref(l, x, old, scale):
    s = f32(scale)
    ref = s * (l.double().T @ x.double())
    absprod = abs(s) * (l.double().abs().T @ x.double().abs())
    if old is not None:
        ref, absprod = ref + old.double(), absprod + old.double().abs()
    return ref, gemm_elem_bound(ref, absprod, l.shape[0], roundings=1, extra_fp32_ops=EXTRA_OPS)


# ---- CPU emulations of the kernels' arithmetic: fp32 accumulation in the split order, scale on the accumulator, one rounding -----------------------
def down_emulate(x, a, scale):
    M, K = x.shape
    n, per = down_split(M, K)
    xf, af = x.float(), a.float()
    acc = None
    for i in range(n):
        p = xf[:, i * per:(i + 1) * per] @ af[:, i * per:(i + 1) * per].T
        acc = p if acc is None else acc + p
    return (torch.tensor(scale, dtype=torch.float32) * acc).to(torch.bfloat16)


def up_emulate(t, bt, res, scale):
    v = torch.tensor(scale, dtype=torch.float32) * (t.float() @ bt.float())
    if res is not None:
        v = v + res.float()
    return v.to(torch.bfloat16)


def wgrad_emulate(l, x, old, scale):
    M, C = x.shape
    n, per = wgrad_split(M, C)
    lf, xf = l.float(), x.float()
    acc = None
    for i in range(n):
        p = lf[i * per:(i + 1) * per].T @ xf[i * per:(i + 1) * per]
        acc = p if acc is None else acc + p
    v = torch.tensor(scale, dtype=torch.float32) * acc
    if old is not None:
        v = v + old.float()
    return v.to(torch.bfloat16)


# ---- the LoRA step against fp32 autograd through the unchanged CPU oracle ------------------------------------------------------------------------
def random_adapters(cfg, lora_cfg, seed):
    """PEFT-initialised As and RANDOM NON-ZERO Bs (N(0, 0.05^2), bf16): with PEFT's zero B every dA is zero and a test shows nothing."""
    from vila_amd.lora import LoraAdapters
    ad = LoraAdapters(cfg.llm, lora_cfg).init_(seed)
    g = _gen(seed + 1)
    for name, (o, k, shape) in ad.index.items():
        if ".Bt_" in name:
            ad.params[o:o + k].copy_((torch.randn(k, generator=g) * 0.05).to(torch.bfloat16))
    return ad


def merged_weights(w, ad, leaves=None):
    """The oracle's weight dict with every adapted projection replaced by W + s (B @ A) in fp32.  leaves: a dict to receive the (A, B) leaf
    tensors (requiring grad) the products are built from, keyed by (layer, module)."""
    from vila_amd.lora import _PARENT
    out = dict(w)
    for i in range(ad.lcfg.num_hidden_layers):
        for m in ad.cfg.target_modules:
            a, bt = ad.pair(i, m)
            A, B = a.float().clone(), bt.float().t().contiguous().clone()
            if leaves is not None:
                A.requires_grad_(True); B.requires_grad_(True)
                leaves[(i, m)] = (A, B)
            name = f"llm.model.layers.{i}.{_PARENT[m]}.{m}.weight"
            out[name] = w[name] + ad.cfg.scale * (B @ A)
    return out


def oracle_lora_grads(cfg, ad, w, px, ids, labels, mask, n_items, tuned=("mm_projector.",)):
    """-> (loss, {flat gradient name: fp32 reference}): autograd through oracle.vlm_sft_loss on the merged weights, A.grad / B.grad stacked and
    transposed into the trainer's layout, plus the gradients of the tuned components."""
    from oracle import vila_oracle as O
    from vila_amd.lora import layer_prefix
    leaves = {}
    wr = {k: (v.clone().requires_grad_(True) if k.startswith(tuple(tuned)) else v) for k, v in w.items()}
    wm = merged_weights(wr, ad, leaves)
    ref = O.vlm_sft_loss([p.float() for p in px], ids, labels, mask, wm, cfg, num_items_in_batch=n_items, packed=True)
    ref.backward()
    grads = {k: v.grad for k, v in wr.items() if v.requires_grad and v.grad is not None}
    for i in range(ad.lcfg.num_hidden_layers):
        for stack, _, members in ad.stacks:
            grads[layer_prefix(i) + f"A_{stack}"] = torch.cat([leaves[(i, m)][0].grad for m in members], 0)
            for m in members:
                grads[layer_prefix(i) + f"Bt_{m[:-5]}"] = leaves[(i, m)][1].grad.t().contiguous()
    return float(ref.detach()), grads
