"""The planted-key inputs of tests/test_gpu_decode_keys.py, and the proof (on the CPU, no kernel involved) that they discriminate.

Every decode attention form must read keys 0 .. pos of its row and no others.  With random Q/K/V a key lost or admitted at a boundary moves the
output by about 1/L, below the tests' bound 2^-7 max|V| once L is a few hundred, so the GPU tests plant keys (tests/gpu_util.py plant_keys) that
take all of a target head's weight.  This file builds those cases (`all_probes`: the GPU tests run exactly these) and asserts the CONDITION ON THE
INPUTS that makes them worth running: the fp32 reference over the correct key set and over the set with the probed key dropped (inside cases) or
admitted (outside cases) differ, on every target head, by at least 8 x the bound.  A case that does not meet it would be reworked, not exempted."""
import os
import re
from dataclasses import dataclass
from typing import List, Optional

import pytest
import torch

from tests.gpu_util import decode_attn_ref, plant_keys, probe_targets, staircase_alphas, visible_upto

KV = 2
GROUPS = [1, 7, 8]                       # G = 7: the partial column tile of the shared kernel; G = 1: every column a target head; G = 8: the widest group
_base = {}


def base_kv(slots: int, C: int):
    """The random K/V every probe starts from: seed 5, as the random-input tests of the batched and the verify attention.  bf16, on the CPU."""
    if (slots, C) not in _base:
        g = torch.Generator().manual_seed(5)
        k = torch.randn((slots, KV, C, 128), generator=g).to(torch.bfloat16)
        v = torch.randn((slots, KV, C, 128), generator=g).to(torch.bfloat16)
        _base[(slots, C)] = (k, v)
    return _base[(slots, C)]


def bound_of(v: torch.Tensor) -> float:
    """max|o - ref| <= 2^-7 max|V|: the bound and rationale of test_walking_attention_against_fp32_softmax (tests/test_gpu_long_batch_decode.py)."""
    return 2.0 ** -7 * float(v.float().abs().max())


@dataclass
class Probe:
    name: str
    kind: str                            # "inside": the flipped key is one the row must read; "outside": the first one it must not
    q: torch.Tensor                      # [n, nq, 128] bf16
    k: torch.Tensor                      # [n or 1, KV, C, 128] bf16, keys planted
    v: torch.Tensor
    lens: List[int]                      # row i reads keys 0 .. lens[i] - 1
    flip: List[Optional[int]]            # row i: the key whose visibility the wrong kernel would flip (None: the row carries no probe)

    def visible(self, wrong: bool = False, device="cpu") -> torch.Tensor:
        vis = visible_upto(self.lens, self.k.shape[2], device)
        if wrong:
            for i, f in enumerate(self.flip):
                if f is not None:
                    vis[i, f] = not bool(vis[i, f])
        return vis


def _rand_q(n: int, G: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, KV * G, 128), generator=g).to(torch.bfloat16)


def placements(L: int, C: int, bounds) -> dict:
    """name -> (kind, planted keys, flipped key) for a row of L visible keys in a cache of C positions: the first and the last key, both sides of
    every boundary in `bounds` that the row reaches (plus the start of its last 256-key chunk), two equal-score keys a third of the way in and at
    the end (weight 1/2 each: the merge weights matter), and the first key the row must not read."""
    if L == 1:                           # the only key cannot be dropped (no reference without a key): it is planted, the probe is the outside one
        out = {"first": ("inside", [0], None)}
    else:
        out = {"first": ("inside", [0], 0), "last": ("inside", [L - 1], L - 1)}
    marks = [(f"b{b}", b) for b in bounds] + [("bL", 256 * ((L - 1) // 256))]
    used = set()
    for label, b in marks:
        for side, key in (("lo", b - 1), ("hi", b)):
            if 0 < key < L - 1 and key not in used:
                out[label + side] = ("inside", [key], key)
                used.add(key)
    if L >= 2:
        out["two"] = ("inside", [(L - 1) // 3, L - 1], (L - 1) // 3)
    if L < C:
        out["outside"] = ("outside", [L], L)
    return out


def row_probes(form: str, G: int, lens, C: int, bounds, seed: int):
    """One probe per placement name for a launch of len(lens) rows, each row in its own slot (the batched forms; one row: the solo forms)."""
    n = len(lens)
    kb, vb = base_kv(n, C)
    per_row = [placements(L, C, bounds) for L in lens]
    names = []
    for p in per_row:
        names += [m for m in p if m not in names]
    for j, name in enumerate(names):
        q = _rand_q(n, G, seed + 31 * j)
        k = kb.clone()
        flip, kind = [], "inside"
        for i, p in enumerate(per_row):
            if name in p:
                kind, keys, f = p[name]
                plant_keys(k[i], q[i], keys)
                flip.append(f)
            else:
                flip.append(None)
        yield Probe(f"{form} G={G} keys={list(lens)} {name}", kind, q, k, vb, list(lens), flip)


# ---- the cases of every form ----------------------------------------------------------------------------------------------------------------
BATCH_SHORT_CTX, BATCH_SHORT_LENS = 2048, (1, 257, 2048)
WALK_CTX = 4096
WALK_LAUNCHES = [(1, 4096, 257), (255, 1536, 2049), (256, 769, 4096)]      # LAUNCHES of tests/test_gpu_long_batch_decode.py
WALK_FORCE = [0, 16, 3]
VERIFY_CTX = 4096
VERIFY_N, VERIFY_POS, VERIFY_FORCE = [16, 5], [0, 250, 2047, 4080, 4090], [0, 3]     # positions from CASES of tests/test_gpu_spec_decode.py
SOLO = {"head": (2048, (0, 255, 256, 2047)), "slices256": (2048, (0, 255, 256, 2047)), "split64": (2304, (63, 64, 2303))}


def batch_short_probes(G: int):
    """bdec_attn_kernel: a wave's 16-key piece, the 256-key slice."""
    yield from row_probes("batch", G, BATCH_SHORT_LENS, BATCH_SHORT_CTX, (16, 256), 1000 + G)


def walk_probes(G: int):
    """bdec_attn_walk_kernel: the 16-key piece, the chunks 1, 3, 8 and 15 (where a slice of force_slices 3 / automatic 8 / 16 hands over or walks
    on) and the row's last chunk.  A planted key in a later chunk forces an e^-20 rescale of everything a block has accumulated."""
    for j, lens in enumerate(WALK_LAUNCHES):
        yield from row_probes("walk", G, lens, WALK_CTX, (16, 256, 768, 2048, 3840), 2000 + 100 * j + G)


def solo_probes(form: str, G: int):
    """attn_decode_head (16-key chunks per wave, 256-key slices when SPLIT) and attn_decode_partial (64-key splits)."""
    C, poss = SOLO[form]
    for j, p in enumerate(poss):
        yield from row_probes(form, G, (p + 1,), C, (16, 64, 256), 3000 + 100 * j + G)


def verify_probes(G: int, n: int, pos: int):
    """bdec_attn_shared_kernel, row i limited to min(pos + i, C - 1).
    staircase: all rows share the target heads' q, keys pos .. pos + n carry scores rising by >= 9 per key, so row i returns V[pos + i] and a row
    that sees key pos + i + 1 returns the next step's V instead (outside).  own: row i's key pos + i is aligned with row i's own q (inside)."""
    C = VERIFY_CTX
    kb, vb = base_kv(1, C)
    lens = [min(pos + i, C - 1) + 1 for i in range(n)]
    q = _rand_q(n, G, 4000 + 17 * pos + n + G)
    for t in probe_targets(KV, G):
        q[:, t] = q[0, t]
    keys = [key for key in range(pos, pos + n + 1) if key < C]
    k = kb.clone()
    plant_keys(k[0], q[0], keys, staircase_alphas(q[0], KV, len(keys)))
    yield Probe(f"verify G={G} n={n} pos={pos} staircase", "outside", q, k, vb, lens, [L if L < C else None for L in lens])
    q = _rand_q(n, G, 5000 + 17 * pos + n + G)
    k = kb.clone()
    for i in range(n):
        if pos + i < C:
            plant_keys(k[0], q[i], [pos + i])
    # a clamped row reads key C - 1, which carries the q of row C - 1 - pos: only that row (and the ones before it) own their last key
    yield Probe(f"verify G={G} n={n} pos={pos} own", "inside", q, k, vb, lens, [pos + i if 0 < pos + i < C else None for i in range(n)])


def all_probes(G: int):
    yield from batch_short_probes(G)
    yield from walk_probes(G)
    for form in SOLO:
        yield from solo_probes(form, G)
    for n in VERIFY_N:
        for pos in VERIFY_POS:
            yield from verify_probes(G, n, pos)


def target_refs(p: Probe, wrong: bool) -> torch.Tensor:
    """The fp32 reference of the target heads alone ([n, KV, 128]): one query head per kv head is a GQA group of 1."""
    G = p.q.shape[1] // KV
    return decode_attn_ref(p.q[:, probe_targets(KV, G)], p.k, p.v, p.visible(wrong))


@pytest.mark.parametrize("G", GROUPS)
def test_every_planted_case_moves_the_reference_by_8x_the_bound(G):
    n_cases = n_rows = 0
    worst = (float("inf"), "")
    for p in all_probes(G):
        bound = bound_of(p.v)
        if all(f is None for f in p.flip):                                    # a lone row of one key: planted and run, nothing to flip
            assert p.lens == [1], p.name
            continue
        good, bad = target_refs(p, False), target_refs(p, True)
        for i, f in enumerate(p.flip):
            if f is None:
                continue
            assert (f < p.lens[i]) == (p.kind == "inside"), (p.name, i)
            moved = float((good[i] - bad[i]).abs().amax(-1).min())            # the target head that moves least
            assert moved >= 8 * bound, f"{p.name} row {i} (key {f} {'dropped' if p.kind == 'inside' else 'admitted'}): moves {moved:.3f} < 8 x {bound:.3f}"
            worst = min(worst, (moved, f"{p.name} row {i}"))
            n_rows += 1
        n_cases += 1
    print(f"G={G}: {n_cases} cases, {n_rows} probed rows; smallest move {worst[0]:.3f} ({worst[1]}) against a bound of {bound:.4f}")


def test_staircase_rows_return_their_own_step():
    """The staircase's reading: row i of the reference IS V[min(pos + i, C - 1)] on the target heads, to well within the bound."""
    for p in verify_probes(7, 16, 250):
        if p.name.endswith("staircase"):
            ref = target_refs(p, False)
            for i, L in enumerate(p.lens):
                assert float((ref[i] - p.v[0, :, L - 1].float()).abs().max()) < 0.1 * bound_of(p.v), i


def test_solo_attention_entries_are_declared_on_both_sides():
    """The operator-level entries of the batch-1 attention: in include/vila_hip.h and in _lib.PROTOTYPES with the same number of arguments, and the
    form numbers of ops.attn_decode are the header's."""
    from vila_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    flat = re.sub(r"/\*.*?\*/", " ", open(os.path.join(root, "include", "vila_hip.h")).read(), flags=re.S)
    for name in ("vila_attn_decode_workspace_bytes", "vila_attn_decode_bf16", "vila_attn_decode_oproj_bf16", "vila_attn_decode_oproj_w4"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", flat)
        assert m, f"{name} is not declared in include/vila_hip.h"
        assert m.group(1).count(",") + 1 == len(_lib.PROTOTYPES[name][1]), name
    enum = dict(re.findall(r"VILA_ATTN_DECODE_([A-Z0-9]+)\s*=\s*(\d+)", flat))
    assert {k.lower(): int(v) for k, v in enum.items()} == ops.ATTN_DECODE_FORMS
