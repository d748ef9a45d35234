"""The launch plan of the bf16 GEMMs (vila_amd/csrc/gemm_plan.h: gemm_plan) is a pure host function, so what the dispatcher will do for a shape
can be pinned without a GPU: a small driver is compiled with g++ against that header ALONE, prints the plan of every row of
tests/golden/gemm_plan.json, and every printed plan must equal the row's expectation.

The file holds the shape table of the dispatcher — the LLM N / K pairs of both model configs (q|k|v, o_proj, fused gate/up, plain gate, down,
lm_head with fp32 out) at M = 64 .. 3076, the tower's four GEMMs at 1 / 2 / 4 / 14 images, the projectors' GEMMs, the SFT dgrad / wgrad
contraction-major forms at the 4 x 769 batch, each with and without a workspace, forced tiles 1..17 and forced schedules, and the rows the prefill
and the tower launch with a RoPE or normalisation offer — plus rows on each side of every threshold (tiles256 149 / 150, K-tiles 127 / 128,
M 511 / 512, tail 96 / 97, tiles_ring 560 / 561 and the 128-wide bound 269 / 270 that binds before it).  Every row carries a `source`:
`"trace"` = the launch was read off a kernel trace of the commit before gemm_plan.h existed (kernel names, grids, reduce kernels); `"derived"` =
NO trace was taken for the row, its expectation was worked out from that commit's source (gemm.hip launch_t / launch_gemm_cm, gemm256.hip
try_hybrid / launch_gateup / launch_gemm256, gemm_ring_splitk.hip), and the row says so in `why`.  Neither kind is output of the code under test."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan.json")
FIELDS = ("family", "grid", "slices", "tail", "ex", "bm", "sched", "ring", "pipe", "reduce")

DRIVER = r'''
#include "gemm_plan.h"
#include <cstdio>
struct Row { int M, N, K, epi, f32, a_cm, b_cm; unsigned long long ws; int offers, tile, sched; };
static const Row rows[] = {
%s
};
int main() {
    for (const Row& r : rows) {
        GemmShape h;
        h.M = r.M; h.N = r.N; h.K = r.K; h.lda = r.a_cm ? r.M : r.K; h.ldw = r.b_cm ? r.N : r.K;
        h.epi = r.epi; h.out_f32 = r.f32; h.a_cm = r.a_cm; h.b_cm = r.b_cm; h.ws = r.ws > 0; h.ws_bytes = (size_t)r.ws;
        h.norm_offer = r.offers & 1; h.rope_offer = (r.offers & 2) != 0;
        GemmKnobs k;
        k.force_tile = r.tile; k.sched = r.sched;
        const GemmPlan p = gemm_plan(h, k);
        // a K-sliced launch over the whole grid carries its slices in grid.y; a hybrid's whole launch has one slice and its tail launch `splits`
        printf("%%s %%d %%d %%d %%d %%d %%d %%d %%d %%s\n", gemm_family_name(p.family), p.n_full, p.splits, p.n_tail, p.ex, p.bm, p.sched, p.ring, p.pipe,
               gemm_reduce_name(p.reduce));
    }
    return 0;
}
'''


def load_rows():
    with open(GOLDEN) as f:
        return json.load(f)["rows"]


def plan_tuple(plan):
    return tuple(str(plan[k]) for k in FIELDS)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_gemm_plan_equals_the_recorded_launches(tmp_path):
    rows = load_rows()
    assert len(rows) >= 320 and {r["plan"]["family"] for r in rows} == {"256", "256_sliced", "256_hybrid", "cm", "cm_sliced", "cm_hybrid", "ring", "ring_splitk",
                                                                        "reg128x128", "reg128x64", "reg256x128"}
    assert {r["plan"]["reduce"] for r in rows} == {"none", "plain", "norm", "rope", "tail", "gateup"}
    assert {r["knobs"].get("tile", 0) for r in rows} >= set(range(18)) and {r["knobs"].get("sched", 0) for r in rows} >= {0, 1, 2, 3, 5, 6, 10}
    lines = []
    for r in rows:
        kn = r.get("knobs", {})
        lines.append("    {%d, %d, %d, %d, %d, %d, %d, %dull, %d, %d, %d}," % (r["M"], r["N"], r["K"], r["epi"], r["out_f32"], r["a_cm"], r["b_cm"],
                                                                             r["ws_bytes"], r.get("offers", 0), kn.get("tile", 0), kn.get("sched", 0)))
    src = tmp_path / "gemm_plan_check.cpp"
    src.write_text(DRIVER % "\n".join(lines))
    exe = tmp_path / "gemm_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "vila_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, "gemm_plan.h must compile with plain g++ (no HIP types, <cstdint> / <cstddef> only):\n" + r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    wrong = []
    for row, line in zip(rows, out):
        got = tuple(line.split())
        if got != plan_tuple(row["plan"]):
            wrong.append(f"{row['tag']} ({row['source']}): plan {dict(zip(FIELDS, got))} vs recorded {row['plan']}")
    assert not wrong, "\n".join(wrong[:20])


def test_the_header_is_host_only():
    """No HIP types, no device code, no includes beyond <cstdint> / <cstddef>: the property that lets g++ compile it and a GPU-less host call it."""
    text = open(os.path.join(ROOT, "vila_amd", "csrc", "gemm_plan.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert sorted(includes) == ["<cstddef>", "<cstdint>"]
    for word in ("__device__", "__global__", "hipStream_t", "getenv"):
        assert word not in text
