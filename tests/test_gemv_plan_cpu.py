"""The CU map of the batch-1 decode GEMVs is planned on the host (vila_amd/csrc/gemv_plan.h: gemv_plan) and read on the device without a
division (GemvPlan::count / gid).  It must be, group for group, the map the kernels used to work out themselves: CuMap of gemv_common.h, whose
formulas are written out below in Python (integer divisions and all).  A small driver is compiled with g++ against the header ALONE and prints
count(cu) and every gid(cu, j) of every case; both are compared with the transcription, and every group must be owned exactly once.

Also checked: the multiply-shift that replaces the QKV kernel's `group / (head_dim / 2)` and the attention kernel's `head / group size`."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_GROUPS = [1, 7, 8, 9, 255, 256, 257, 7 * 256, 9 * 256 + 1, 37 * 256, 297 * 256 + 3]
NCUS = [8, 104, 250, 256, 304]
SKEWS = [0, 1]
INTERLEAVED = 0x3fffffff

DRIVER = r'''
#include "gemv_plan.h"
#include <cstdio>
int main() {
    static const int ns[] = {%s}, cus[] = {%s}, skews[] = {%s};
    for (int n : ns) for (int ncu : cus) for (int skew : skews) {
        const GemvPlan p = gemv_plan(n, ncu, skew);
        printf("case %%d %%d %%d %%d\n", n, ncu, skew, p.cf);
        for (int cu = 0; cu < ncu; ++cu) {
            const int c = p.count(cu);
            printf("%%d", c);
            for (int j = 0; j < c; ++j) printf(" %%d", p.gid(cu, j));
            printf("\n");
        }
    }
    // the multiply-shift division: every n up to the bound the kernels' launchers check, for the divisors they can meet
    static const unsigned ds[] = {2, 3, 7, 8, 32, 48, 64, 128, 250};
    for (unsigned d : ds) {
        const uint32_t m = udiv_magic(d);
        unsigned bad = 0;
        const uint64_t lim = (1ull << 32) / d;
        for (uint64_t n = 0; n < lim; n += (n < 100000 || n + 100000 >= lim) ? 1 : 9973) bad += udiv_by_magic((uint32_t)n, m) != (uint32_t)n / d;
        printf("div %%u %%u\n", d, bad);
    }
    return 0;
}
'''


class CuMapRef:
    """gemv_common.h CuMap, transcribed: the constructor, rank, count and gid."""

    def __init__(self, n_groups, ncu, skew):
        self.ncu = ncu
        self.n_fast = ncu >> 1
        can = (ncu & 7) == 0
        self.cf = n_groups // ncu - (skew if can else 0)
        self.cf = 0 if self.cf < 0 else self.cf
        self.rem = n_groups - self.cf * ncu
        if not can:
            self.cf, self.rem = INTERLEAVED, 0
        self.n_total = n_groups

    @staticmethod
    def rank(cu):
        return (cu >> 3) * 4 + ((cu & 7) >> 1)

    def count(self, cu):
        if self.cf == INTERLEAVED:
            return (self.n_total - cu + self.ncu - 1) // self.ncu if self.n_total > cu else 0
        fast = (cu & 1) == 0
        r = self.rank(cu)
        return self.cf + ((self.rem - r + self.n_fast - 1) // self.n_fast if (fast and self.rem > r) else 0)

    def gid(self, cu, j):
        if self.cf == INTERLEAVED or j < self.cf:
            return j * self.ncu + cu
        return self.cf * self.ncu + (j - self.cf) * self.n_fast + self.rank(cu)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_plan_is_the_device_map(tmp_path):
    src = tmp_path / "gemv_plan_check.cpp"
    src.write_text(DRIVER % (", ".join(map(str, N_GROUPS)), ", ".join(map(str, NCUS)), ", ".join(map(str, SKEWS))))
    exe = tmp_path / "gemv_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "vila_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, "gemv_plan.h must compile with plain g++ (no HIP types, <cstdint> only):\n" + r.stderr[-3000:]
    lines = iter(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    n_cases = 0
    for n in N_GROUPS:
        for ncu in NCUS:
            for skew in SKEWS:
                head = next(lines).split()
                assert head[:4] == ["case", str(n), str(ncu), str(skew)]
                ref = CuMapRef(n, ncu, skew)
                if ncu % 8 != 0:
                    assert int(head[4]) == INTERLEAVED and ref.cf == INTERLEAVED, f"ncu={ncu} must take the interleaved map"
                else:
                    assert int(head[4]) == ref.cf
                owned = []
                for cu in range(ncu):
                    got = [int(v) for v in next(lines).split()]
                    want = [ref.gid(cu, j) for j in range(ref.count(cu))]
                    assert got[0] == ref.count(cu) and got[1:] == want, f"n_groups={n} ncu={ncu} skew={skew} cu={cu}: {got[:6]} vs {[len(want)] + want[:5]}"
                    owned += got[1:]
                assert sorted(owned) == list(range(n)), f"n_groups={n} ncu={ncu} skew={skew}: every group exactly once"
                n_cases += 1
    assert n_cases == len(N_GROUPS) * len(NCUS) * len(SKEWS)
    divs = [next(lines).split() for _ in range(9)]
    assert all(d[0] == "div" and d[2] == "0" for d in divs), divs
    assert next(lines, None) is None
