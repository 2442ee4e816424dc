"""Are the kernels of one device-assembly file all present, instruction for instruction, in another?  (adding an
instantiation to a kernel template must leave the existing instantiations' code alone.)

Build both files the same way, e.g. for csrc/gsr_render.hip of the parent commit and of this tree:

    hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=fast -DNDEBUG --cuda-device-only -S gsr_render.hip -o new.s
    python tools/kernel_asm_diff.py parent.s new.s

A kernel's body is its lines between its label and the end of the function, comments dropped, with symbol names and the numbering
of local labels normalised (a template that gains a parameter changes its instantiations' mangled names, not their code).  Prints
SAME / DIFF per kernel of the first file; exit status 1 if any differs.
"""
import hashlib
import re
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        t = line.split(";")[0].rstrip()
        if t.strip():
            out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", t)))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    digest = lambda v: hashlib.sha1("\n".join(v).encode()).hexdigest()
    have = {digest(v): k for k, v in b.items()}
    same = True
    for k, v in a.items():
        h = digest(v)
        print(("SAME " if h in have else "DIFF ") + f"{len(v):6d} lines  {k}" + (f"\n{'':19s}-> {have[h]}" if h in have and have[h] != k else ""))
        same &= h in have
    print(f"{len(a)} kernels in {sys.argv[1]}, {len(b)} in {sys.argv[2]}: " + ("all of the first are in the second" if same else "SOME DIFFER"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
