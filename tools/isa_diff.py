#!/usr/bin/env python3
"""Is the device code of the working tree the device code of a git revision?  (CPU only; two builds, about three minutes each, run side by side.)

    python tools/isa_diff.py [REV] [-DSWITCH ...]        # REV defaults to HEAD

Exports REV with `git archive`, builds that tree and the working tree with their own lib.hipcc_command(...) plus --save-temps, each in a temporary
directory, and compares per kernel of every translation unit the text between the kernel's label and its .Lfunc_end and its .amdhsa_kernel block
(lines naming __hip_cuid_, a per-unit symbol hashed from the source path, are ignored; so are comments, and local labels are compared without
the index of their function in the unit, which moves when a kernel is added in front of it).  Prints each kernel's resources; exits 1 on any difference.
A refactor of the engine source is done when this prints no DIFFERS for the product build and for every diagnostic switch the tools build with
(-DLM_STAMPS=1, -DLM_STAMPS=2, -DLM_COUNT_PASS2, -DLM_WAVES2)."""
import concurrent.futures
import glob
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOURCES = [("vgpr", "next_free_vgpr"), ("accum", "accum_offset"), ("sgpr", "next_free_sgpr"), ("scratch", "private_segment_fixed_size"),
             ("lds", "group_segment_fixed_size")]


def device_asm(tree, extra, work):
    """{unit: assembly text} of the gfx950 code objects of `tree`, built in `work`."""
    spec = importlib.util.spec_from_file_location("lib_" + os.path.basename(work), os.path.join(tree, "locomanipulationrl_amd", "lib.py"))
    lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lib)
    subprocess.run(lib.hipcc_command(extra=["--save-temps", *extra], out=os.path.join(work, "lib.so")), cwd=work, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return {os.path.basename(f).split("-hip-")[0]: open(f).read() for f in sorted(glob.glob(os.path.join(work, "*-hip-amdgcn-*gfx950.s")))}


def kernels(asm):
    """{kernel: (body lines, .amdhsa_kernel block lines)} of one unit's assembly."""
    def keep(text):
        # instructions only: comments carry the names of inlined device functions, and a local label carries the index of its function in the
        # unit (.LBB<function>_<block>, .Lpost_getpc<n>), which moves when a kernel is added in front of it; neither changes an instruction
        lines = (re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].rstrip())) for ln in text.split("\n") if "__hip_cuid_" not in ln)
        return [ln for ln in lines if ln]
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\s*\.amdhsa_kernel \1\n(.*?)^\s*\.end_amdhsa_kernel\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S):
        out[m.group(1)] = (keep(m.group(2) + m.group(4)), keep(m.group(3)))
    return out


def main():
    args = sys.argv[1:]
    extra = [a for a in args if a.startswith("-D")]
    rev = ([a for a in args if not a.startswith("-D")] or ["HEAD"])[0]
    with tempfile.TemporaryDirectory() as tmp:
        old_tree, old_work, new_work = (os.path.join(tmp, d) for d in ("old_tree", "old_build", "new_build"))
        for d in (old_tree, old_work, new_work):
            os.mkdir(d)
        archive = subprocess.run(["git", "-C", ROOT, "archive", rev], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", old_tree], input=archive, check=True)
        with concurrent.futures.ThreadPoolExecutor(2) as pool:
            old, new = pool.map(device_asm, (old_tree, ROOT), (extra, extra), (old_work, new_work))
    bad, total = set(old) ^ set(new), 0
    print("%-12s %-50s %-8s %-8s %5s %5s %5s %8s %6s" % ("unit", "kernel", "text", "block", *[r[0] for r in RESOURCES]))
    for unit in sorted(set(old) & set(new)):
        ko, kn = kernels(old[unit]), kernels(new[unit])
        bad |= {unit + ":" + k for k in set(ko) ^ set(kn)}
        for k in sorted(set(ko) & set(kn)):
            same = [ko[k][i] == kn[k][i] for i in (0, 1)]
            res = [next((ln.split()[-1] for ln in kn[k][1] if ln.split()[:1] == [".amdhsa_" + name]), "-") for _, name in RESOURCES]
            print("%-12s %-50s %-8s %-8s %5s %5s %5s %8s %6s" % (unit, k, *["same" if s else "DIFFERS" for s in same], *res))
            total += 1
            if not all(same):
                bad.add(unit + ":" + k)
    print("%d kernels compared against %s %s: %s" % (total, rev, " ".join(extra), "DIFFERENT or missing: " + ", ".join(sorted(bad)) if bad else "all identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
