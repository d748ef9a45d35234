"""What stands between a weight batch's last request and its first multiply-add, and how does a row group end?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --offload-device-only -S -w [per-source flags of vila_amd/build.py] gemv.hip -o gemv.s
    python tools/kernel_tail_asm.py gemv.s [substring of a mangled kernel name ...]

A listing tool for DPP / wait placement, the companion of tools/kernel_head_asm.py.  For every kernel of the file (or those whose mangled name
contains one of the substrings) it prints, in program text order:

* the reductions: `ds_bpermute_b32` (an LDS trip each) and DPP / row-swap instructions (`row_ror`, `quad_perm`, `v_permlane*_swap`) from the first
  weight request on — the group loop and what follows it — and, of the former, those behind the LAST 16-byte global load, the kernel's tail;
* one line per weight batch — a run of non-temporal `global_load_dwordx4 ... nt` not interrupted by a multiply-add: how many requests, the
  `vmcnt` immediates of the waits between the batch's last request and the first `v_fma` / `v_fmac` / `v_pk_fma` behind it, and the immediates that
  follow up to the next label, branch or weight request.  A batch that is consumed chunk by chunk shows a descending run that starts near its
  size; `vmcnt(1), vmcnt(0)` or a lone `vmcnt(0)` in front of the first multiply-add is a batch that is waited for as a whole.

Program text is not a path: both arms of a branch are listed, and a batch whose requests sit in predicated blocks shows as several short runs."""
import re
import sys

from kernel_head_asm import kernels

_FMA = ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32")
_DPP = ("row_ror", "quad_perm", "v_permlane16_swap", "v_permlane32_swap")


def _vmcnt(s):
    m = re.search(r"vmcnt\((\d+)\)", s)
    return int(m.group(1)) if m and s.startswith("s_waitcnt") else None


def batches(lines):
    """[(requests, [vmcnt in front of the first multiply-add], [vmcnt behind it, up to the next label / branch / weight request])]"""
    out, i, n = [], 0, len(lines)
    while i < n:
        if not (lines[i].startswith("global_load_dwordx4") and lines[i].endswith(" nt")):
            i += 1
            continue
        cnt, last, j = 0, i, i
        while j < n and not lines[j].startswith(_FMA) and not lines[j].startswith("s_endpgm"):
            if lines[j].startswith("global_load_dwordx4") and lines[j].endswith(" nt"):
                cnt, last = cnt + 1, j
            j += 1
        before = [v for v in map(_vmcnt, lines[last + 1:j]) if v is not None]
        after = []
        k = j
        while k < n and not lines[k].endswith(":") and not lines[k].startswith(("s_cbranch", "s_branch", "s_endpgm")) \
                and not (lines[k].startswith("global_load_dwordx4") and lines[k].endswith(" nt")):
            v = _vmcnt(lines[k])
            if v is not None:
                after.append(v)
            k += 1
        out.append((cnt, before, after))
        i = max(k, last + 1)
    return out


def main(argv):
    if not argv:
        print(__doc__)
        return 2
    ks, preload = kernels(argv[0])
    for name, lines in ks.items():
        if argv[1:] and not any(a in name for a in argv[1:]):
            continue
        if name not in preload:
            continue                      # a device function, not a kernel
        loads = [i for i, s in enumerate(lines) if s.startswith("global_load_dwordx4")]
        weights = [i for i in loads if lines[i].endswith(" nt")]
        if not weights:
            continue
        body, tail = lines[weights[0]:], lines[loads[-1]:]
        bp = sum(1 for s in body if s.startswith("ds_bpermute_b32"))
        bp_tail = sum(1 for s in tail if s.startswith("ds_bpermute_b32"))
        dpp = sum(1 for s in body if any(d in s for d in _DPP))
        print(f"{name}\n  from the first weight request on: {bp} ds_bpermute_b32, {dpp} DPP / row-swap instructions; behind the last 16-byte global load: "
              f"{bp_tail} ds_bpermute_b32")
        for cnt, before, after in batches(lines):
            print(f"    batch of {cnt:2d} requests: vmcnt in front of the first multiply-add {before or '(none)'}, then {after or '(none)'}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
