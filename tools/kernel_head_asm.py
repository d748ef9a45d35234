"""What stands in front of a kernel's first 16-byte global load?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --offload-device-only -S -w [per-source flags of vila_amd/build.py] gemv.hip -o gemv.s
    python tools/kernel_head_asm.py gemv.s [substring of a demangled-ish kernel name ...]

For every kernel of the file (or those whose mangled name contains one of the substrings) prints the descriptor's
`.amdhsa_user_sgpr_kernarg_preload_length`, and the scalar loads, `s_waitcnt` with an lgkmcnt term and `v_rcp_iflag_f32` (the integer
division sequence) that precede, in program text order, the first `global_load_dwordx4` — the first weight or K/V request of the decode kernels.
With kernarg preload a kernel opens with the compatibility prologue for firmware without the feature (loads of the leading arguments, a wait and
a branch over padding to the next 256-byte boundary); it is reported on its own line and the main path is counted from behind it."""
import re
import sys


def kernels(path):
    out, cur, name = {}, None, None
    preload = {}
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name = m.group(1)
            cur = out.setdefault(name, [])
            continue
        m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", ln)
        if m and name:
            preload[name] = int(m.group(1))
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        s = re.sub(r"\s*;.*$", "", ln.strip())
        if s:
            cur.append(s)
    return out, preload


def head(lines):
    """(compatibility prologue, main-path instructions up to the first global_load_dwordx4)"""
    compat, start = [], 0
    for i, s in enumerate(lines[:16]):
        if s.startswith(".p2align") and i > 0 and lines[i - 1].startswith("s_branch"):
            compat, start = [x for x in lines[:i] if not x.startswith(".")], i + 1
            break
    main = []
    for s in lines[start:]:
        if s.startswith("global_load_dwordx4"):
            break
        main.append(s)
    return compat, main


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
        compat, mainp = head(lines)
        picked = [s for s in mainp if s.startswith("s_load") or s.startswith("s_buffer_load") or (s.startswith("s_waitcnt") and "lgkmcnt" in s)
                  or s.startswith("v_rcp_iflag")]
        n_inst = sum(1 for s in mainp if not s.startswith(".") and not s.endswith(":"))
        print(f"{name}\n  kernarg_preload_length {preload[name]}; {n_inst} instructions in front of the first global_load_dwordx4")
        if compat:
            print("  compatibility prologue: " + "; ".join(compat))
        for s in picked:
            print("    " + s)
        if not picked:
            print("    (no scalar load, lgkmcnt wait or division)")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
