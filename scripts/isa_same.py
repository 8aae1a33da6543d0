"""No GPU needed: is the gfx950 assembly of kernel sources in the working tree that of another revision?

    python scripts/isa_same.py <git-rev> <file.hip> ...

Exports radfoam_amd/csrc and include of <git-rev> with ``git archive`` into a temporary directory, compiles every named
file of radfoam_amd/csrc from there and from the working tree (``build.HIPCC_FLAGS`` plus ``--cuda-device-only -S``),
drops the lines that carry the ``__hip_cuid_<hash>`` symbol of the compilation unit, and prints per file ``identical``
or the first differing lines.  A plain comparison of text.  Exits non-zero on any difference: what a refactor of the
device code that claims to change nothing has to pass.
"""
import difflib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join("radfoam_amd", "csrc")


def assembly(tree, name, out):
    from radfoam_amd import build

    cmd = [build._hipcc()] + build.HIPCC_FLAGS + ["--cuda-device-only", "-S", os.path.join(tree, CSRC, name), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(" ".join(cmd) + "\n" + res.stdout + res.stderr)
    with open(out) as f:
        return [line for line in f if "__hip_cuid_" not in line]


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    rev, names = sys.argv[1], [os.path.basename(n) for n in sys.argv[2:]]
    different = 0
    with tempfile.TemporaryDirectory() as tmp:
        archive = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], capture_output=True, check=True)
        subprocess.run(["tar", "-x", "-C", tmp], input=archive.stdout, check=True)
        for name in names:
            old = assembly(tmp, name, os.path.join(tmp, name + ".old.s"))
            new = assembly(ROOT, name, os.path.join(tmp, name + ".new.s"))
            if old == new:
                print(f"{name}: identical ({len(new)} lines)")
                continue
            different += 1
            diff = list(difflib.unified_diff(old, new, rev, "working tree", n=0))
            print(f"{name}: DIFFERENT ({sum(l[0] in '+-' for l in diff[2:])} differing lines)")
            sys.stdout.writelines(diff[:40])
    sys.exit(1 if different else 0)


if __name__ == "__main__":
    main()
