"""Do two builds of one HIP source give the same machine code, kernel by kernel?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --offload-device-only -S -w OLD/attn.hip -o old.s     (the flags of vila_amd/build.py)
    hipcc ...                                                                                      NEW/attn.hip -o new.s
    python tools/compare_kernel_asm.py old.s new.s [--rename FROM=TO ...]

Compares the instruction stream of every function of old.s with the function of the same name in new.s: instructions and branch labels only
(comments, directives and the kernel descriptors are left out; labels are compared without their function number).  `--rename` rewrites a
substring of the NEW file's mangled names first, for a change that adds a defaulted template parameter or re-spells a parameter type without
touching the code, e.g. for attn.hip's prefix mode:
    --rename ELb0EEvNSt11conditionalIXT3_E14AttnAppendArgs8AttnArgsE4typeEi=EEv8AttnArgsi
Prints one line per differing function and the functions only the new file has; exit status 1 if any function of old.s differs or is missing."""
import re
import sys


def functions(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        s = re.sub(r"\s*;.*$", "", ln.strip())
        if not s or (s.startswith(".") and not s.startswith(".LBB")):
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def main(argv):
    files, renames = [], []
    it = iter(argv)
    for a in it:
        if a == "--rename":
            renames.append(next(it).split("=", 1))
        else:
            files.append(a)
    if len(files) != 2:
        print(__doc__)
        return 2
    old, new = functions(files[0]), functions(files[1])

    def norm(name):
        for a, b in renames:
            name = name.replace(a, b)
        return name
    new_n = {norm(k): v for k, v in new.items()}
    same = bad = 0
    for k, v in old.items():
        w = new_n.get(k)
        if w is None:
            print(f"MISSING in {files[1]}: {k}")
            bad += 1
        elif v == w:
            same += 1
        else:
            print(f"DIFFERENT: {k} ({len(v)} / {len(w)} lines)")
            bad += 1
    print(f"{len(old)} functions in {files[0]}: {same} identical, {bad} different or missing; {len(new_n) - len(set(new_n) & set(old))} only in {files[1]}")
    for k in new_n:
        if k not in old:
            print(f"  new: {k} ({len(new_n[k])} lines)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
