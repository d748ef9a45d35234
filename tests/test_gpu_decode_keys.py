"""Every decode attention form reads keys 0 .. pos of its row and no others: the planted-key cases of tests/test_decode_probe_cpu.py (which proves
on the CPU that each of them moves the reference by >= 8 x the bound when its probed key is lost or admitted) run through
  * bdec_attn_kernel and bdec_attn_walk_kernel (ops.attn_decode_batch), the latter under vila_decode_batch_force_slices 0 / 16 / 3,
  * bdec_attn_shared_kernel (ops.attn_decode_verify), force 0 / 3,
  * the batch-1 forms (ops.attn_decode): attn_decode_head<false>, attn_decode_head<true> merged in the o_proj GEMV's prologue (bf16: gemv_kernel<2>,
    W4: gemv_w4_kernel<4>), attn_decode_partial + attn_decode_merge,
against an fp32 softmax over exactly the permitted keys.  The bound is the random-input tests' max|o - ref| <= 2^-7 max|V|
(test_walking_attention_against_fp32_softmax: a convex combination of V rows rounded once to bf16, relative 2^-9, times 4 for __expf and the summation
order).  VILA_DUMP_PROBE=<file> appends the largest error of every test as a JSON line (the figures in CHANGELOG.md)."""
import json
import os

import pytest
import torch

from tests.gpu_util import decode_attn_ref
from tests.test_decode_probe_cpu import (BATCH_SHORT_CTX, GROUPS, KV, SOLO, VERIFY_CTX, VERIFY_FORCE, VERIFY_N, VERIFY_POS, WALK_CTX, WALK_FORCE,
                                         batch_short_probes, bound_of, solo_probes, verify_probes, walk_probes)
from vila_amd import _lib, ops

pytestmark = pytest.mark.gpu


class _Slices:
    """vila_decode_batch_force_slices for a `with` block; always back to automatic."""

    def __init__(self, nsl):
        self.nsl = nsl

    def __enter__(self):
        _lib.load().vila_decode_batch_force_slices(int(self.nsl))

    def __exit__(self, *a):
        _lib.load().vila_decode_batch_force_slices(0)


_vdev = {}


def _on_gpu(p):
    """(q, k, v, positions, fp32 reference over the permitted keys, bound); the V base goes to the device once."""
    if id(p.v) not in _vdev:
        _vdev.clear()
        _vdev[id(p.v)] = (p.v, p.v.cuda())
    v = _vdev[id(p.v)][1]
    q, k = p.q.cuda(), p.k.cuda()
    ref = decode_attn_ref(q, k, v, p.visible(device="cuda"))
    pos = torch.tensor([L - 1 for L in p.lens], dtype=torch.int32, device="cuda")
    return q, k, v, pos, ref, bound_of(p.v)


class _Worst:
    def __init__(self, test):
        self.test, self.err, self.at, self.bound, self.n = test, 0.0, "", 0.0, 0

    def check(self, p, o, ref, bound, what=""):
        assert o.shape == ref.shape, (tuple(o.shape), tuple(ref.shape))
        assert bool(torch.isfinite(o.float()).all()), f"{p.name} {what}: non-finite output"
        err = (o.float() - ref).abs().amax((1, 2))
        e = float(err.max())
        if e >= self.err:
            self.err, self.at = e, f"{p.name} {what}"
        self.bound, self.n = bound, self.n + 1
        assert e <= bound, f"{p.name} {what}: row of {p.lens[int(err.argmax())]} keys: max|o - ref| = {e:.3e} > {bound:.3e}"

    def report(self):
        print(f"{self.test}: {self.n} launches, largest max|o - ref| = {self.err:.3e} at {self.at} (bound {self.bound:.3e})")
        path = os.environ.get("VILA_DUMP_PROBE")
        if path:
            with open(path, "a") as f:
                f.write(json.dumps({"test": self.test, "launches": self.n, "max_err": self.err, "at": self.at, "bound": self.bound}) + "\n")


@pytest.mark.parametrize("G", GROUPS)
def test_batched_short_form_reads_exactly_its_keys(G):
    """bdec_attn_kernel (caches up to 2048 positions): rows of 1, 257 and 2048 keys in one launch."""
    assert _lib.load().vila_decode_batch_slices(BATCH_SHORT_CTX) == 0, "the short form was expected at this capacity"
    w = _Worst(f"batch short G={G}")
    for p in batch_short_probes(G):
        q, k, v, pos, ref, bound = _on_gpu(p)
        w.check(p, ops.attn_decode_batch(q, k, v, pos), ref, bound)
    w.report()


@pytest.mark.parametrize("G", GROUPS)
def test_walking_form_reads_exactly_its_keys(G):
    """bdec_attn_walk_kernel in a 4096-position cache: the automatic 8 slices (up to 2 chunks per block), 16 (one chunk per block) and 3 (up to 6)."""
    lib = _lib.load()
    w = _Worst(f"batch walking G={G}")
    for p in walk_probes(G):
        q, k, v, pos, ref, bound = _on_gpu(p)
        for force in WALK_FORCE:
            with _Slices(force):
                assert lib.vila_decode_batch_slices(WALK_CTX) == (force or 8)
                w.check(p, ops.attn_decode_batch(q, k, v, pos), ref, bound, f"force={force}")
    w.report()


@pytest.mark.parametrize("n", VERIFY_N)
@pytest.mark.parametrize("G", GROUPS)
def test_shared_form_rows_read_exactly_their_keys(G, n):
    """bdec_attn_shared_kernel: row i reads keys 0 .. min(pos + i, 4095).  The staircase makes a row that sees one key too many return the next
    row's V; in `own` every row's last key carries that row's own q."""
    w = _Worst(f"verify G={G} n={n}")
    for p0 in VERIFY_POS:
        for p in verify_probes(G, n, p0):
            q, k, v, pos, ref, bound = _on_gpu(p)
            for force in VERIFY_FORCE:
                with _Slices(force):
                    w.check(p, ops.attn_decode_verify(q, k[0], v[0], pos[:1]), ref, bound, f"force={force}")
    assert VERIFY_CTX == 4096
    w.report()


# ---- the batch-1 forms ------------------------------------------------------------------------------------------------------------------------
def _one_hot_rows(nq: int, seed: int):
    """An o_proj weight [nq * 128, nq * 128] with ONE non-zero power of two per row: row r = 2^e[r] at column perm[r].  y = W o is then a scaled,
    permuted copy of the merged attention output, exact in bf16, and the attention bound carries over times 2^e[r]."""
    g = torch.Generator().manual_seed(seed)
    K = nq * 128
    perm = torch.randperm(K, generator=g)
    exps = torch.randint(-2, 2, (K,), generator=g)
    return perm, exps


def _dense(perm, exps):
    K = perm.numel()
    w = torch.zeros((K, K), dtype=torch.float32)
    w[torch.arange(K), perm] = torch.exp2(exps.float())
    return w


def _one_hot_w4(perm, exps):
    """The same matrix as int4 groups of 128 that represent it exactly: nibble 1 at the column, scale 2^e[r], zero point 0 (built in the logical
    format of vila_amd.quant, whose quantiser would put the group's scale at 2^e / 15)."""
    from vila_amd import quant
    K = perm.numel()
    wq = torch.zeros((K, K // 8), dtype=torch.int32)
    e = perm % 8
    nib = torch.where(e % 2 == 0, e // 2, e // 2 + 4)
    wq[torch.arange(K), perm // 8] = (1 << (4 * nib)).to(torch.int32)
    s_bits = torch.exp2(exps.float()).to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF
    z_bits = int(torch.tensor(128.0).to(torch.bfloat16).view(torch.int16)) & 0xFFFF
    wsz = (s_bits | (z_bits << 16))[:, None].expand(K, K // 128).contiguous()
    assert torch.equal(quant.dequantize_w4(wq, wsz), _dense(perm, exps)), "the int4 groups do not represent the matrix exactly"
    q_t, sz_t = quant.tile_w4(wq, wsz)
    return quant.W4Matrix(q_t.cuda(), sz_t.cuda(), K, K, 0, (wq, wsz))


def _solo(form, weight, G):
    w = _Worst(f"solo {form}{'' if weight is None else ' ' + weight} G={G}")
    nq = KV * G
    if weight is not None:
        perm, exps = _one_hot_rows(nq, 700 + G)
        mat = _dense(perm, exps).to(torch.bfloat16).cuda() if weight == "bf16" else _one_hot_w4(perm, exps)
        perm, inv_scale = perm.cuda(), torch.exp2(-exps.float()).cuda()
    for p in solo_probes(form, G):
        q, k, v, pos, ref, bound = _on_gpu(p)
        if weight is None:
            o = ops.attn_decode(q[0], k[0], v[0], pos, form)
        else:
            y = ops.attn_decode(q[0], k[0], v[0], pos, form, w=mat)
            o = torch.empty(nq * 128, device="cuda", dtype=torch.float32)
            o[perm] = y.float() * inv_scale                              # y[r] = 2^e[r] o[perm[r]]
            o = o.view(nq, 128)
        w.check(p, o[None], ref, bound)
    w.report()


@pytest.mark.parametrize("G", GROUPS)
def test_solo_head_form_reads_exactly_its_keys(G):
    """attn_decode_head<false>: one block per query head, wave w takes the 16-key chunks w, w + 16, ...; positions 0, 255, 256, 2047 of 2048."""
    _solo("head", None, G)


@pytest.mark.parametrize("weight", ["bf16", "w4"])
@pytest.mark.parametrize("G", GROUPS)
def test_solo_slices256_form_reads_exactly_its_keys(G, weight):
    """attn_decode_head<true> + the merge over ceil((pos + 1) / 256) slices in the o_proj GEMV's prologue (bf16 mode 2, W4 mode 4), seen through a
    one-hot power-of-two weight.  The W4 GEMV computes scale * (sum x (128 + q) - 128 sum x) in fp32, so its copy of o carries an absolute error
    of about 1e-3 before the bf16 store; the bound is not widened for it."""
    _solo("slices256", weight, G)


@pytest.mark.parametrize("G", GROUPS)
def test_solo_split64_form_reads_exactly_its_keys(G):
    """attn_decode_partial + attn_decode_merge in a 2304-position cache: positions 63, 64 and the last one."""
    _solo("split64", None, G)


def test_solo_forms_refuse_what_they_do_not_serve():
    """A position at or past the capacity never reaches a solo kernel (they read pos + 1 keys unguarded): refused in Python, nothing launched.  The
    C entry names the capacity each form serves and that the 256-key slices have no output of their own."""
    g = torch.Generator().manual_seed(1)
    q = torch.randn((4, 128), generator=g).to(torch.bfloat16).cuda()
    i32 = lambda x: torch.tensor([x], dtype=torch.int32, device="cuda")
    for form, C in (("head", 512), ("split64", 2304)):
        k = torch.zeros((2, C, 128), dtype=torch.bfloat16, device="cuda")
        for bad in (C, C + 5, -1):
            with pytest.raises(ValueError, match="outside the cache"):
                ops.attn_decode(q, k, k, i32(bad), form)
    k = torch.zeros((2, 512, 128), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="outside the cache"):
        ops.attn_decode(q, k, k, i32(512), "slices256", w=torch.zeros((8, 512), dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ValueError, match="slices256"):
        ops.attn_decode(q, k, k, i32(3), "slices256")
    with pytest.raises(ValueError, match="slices256"):
        ops.attn_decode(q, k, k, i32(3), "head", w=torch.zeros((8, 512), dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ValueError, match="64-key split"):
        ops.attn_decode(q, k, k, i32(3), "split64")
    big = torch.zeros((2, SOLO["split64"][0], 128), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="per-head forms"):
        ops.attn_decode(q, big, big, i32(3), "head")
    lib = _lib.load()
    ws = torch.empty(lib.vila_attn_decode_workspace_bytes(4, 512), dtype=torch.uint8, device="cuda")
    o = torch.empty((4, 128), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="no attention output of its own"):
        _lib.check(lib.vila_attn_decode_bf16(q.data_ptr(), k.data_ptr(), k.data_ptr(), i32(3).data_ptr(), o.data_ptr(), 4, 2, 512, 0.1, 1, ws.data_ptr(),
                                             ws.numel(), None), "attn_decode")
    with pytest.raises(ValueError, match="workspace too small"):
        _lib.check(lib.vila_attn_decode_bf16(q.data_ptr(), k.data_ptr(), k.data_ptr(), i32(3).data_ptr(), o.data_ptr(), 4, 2, 512, 0.1, 0, ws.data_ptr(),
                                             64, None), "attn_decode")
    torch.cuda.synchronize()
